"""CPU emulation with dtype-following models of the fused colour head, for its fp16 flavour (csrc/fmlp.hip: fcolour_fwd_kernel<.., F16>,
fcolour_bwd_kernel<F16>).

tests/cpu_ops_emulation.py models `fcolour_fwd` with the first layer's activations rounded to bf16 and `fcolour_bwd` with d_raw_rgb and every
stored gradient rounded to bf16; the kernels round to the dtype of the weight stream.  `emulate_ops_colour_fp16()` enters
`emulate_ops_fp16()` and then overrides those two names on snerf_amd.ops with copies whose rounding type is `stream.dtype` (for a bf16
stream they are the originals, value for value)."""
import contextlib

import torch

import cpu_ops_emulation as emu
import cpu_ops_emulation_fp16 as emu16


def fcolour_fwd(CB, stream, bias, raw_rgb, acts=None, bits=None, variant=0):
    """model of fcolour_fwd_kernel in either flavour: cond_layers.0 K-MAJOR (66 k-steps x 4 blocks), then two 128-wide layers and the rgb head"""
    assert stream.shape[0] == 336 and bias.numel() == 13 * 32
    assert CB.dtype == stream.dtype and (acts is None or all(y.dtype == stream.dtype for y in acts))
    dt = stream.dtype
    st = emu._FStream(stream, bias)                   # (its dense / block round to the stream's dtype already)
    M = CB.shape[0]
    acc = [bias[32 * j:32 * j + 32].clone()[None, :].expand(M, 32).clone() for j in range(4)]
    st.nb = 4
    for x in emu._rows_to_ksteps(CB, 66):
        for j in range(4):
            acc[j] = acc[j] + x @ st.frag().t()
    p = []
    for j in range(4):
        y = torch.relu(acc[j].to(dt).float())
        if acts is not None:
            acts[0][:, 32 * j:32 * j + 32] = y.to(acts[0].dtype)
        p += [y[:, emu._P], y[:, 16 + emu._P]]
    q = st.dense([p], 4, True, None if acts is None else acts[1])
    p = st.dense([q], 4, True, None if acts is None else acts[2])
    raw_rgb[:, :3] = st.block([p], False, to_frags=False)[:, :3]
    assert st.f == 336 and st.nb == 13
    if acts is not None:
        for y, w in zip(acts, bits):
            emu._BITS[w.data_ptr()] = y[:, :128].float() > 0


def fcolour_bwd(d_raw_rgb, stream, bits, dC, dB, g_bias):
    """model of fcolour_bwd_kernel in either flavour: the data-gradient chain on the transposed weights; masks, bias gradients (of the masked
    fp32 accumulators), stores in the stream's 16-bit type"""
    assert stream.shape[0] == 336
    dt = stream.dtype
    assert dB.dtype == dt and all(y.dtype == dt for y in dC)
    st = emu._FStream(stream, torch.zeros(44 * 32))
    M = d_raw_rgb.shape[0]
    g = torch.zeros(M, 16)
    g[:, :3] = d_raw_rgb.to(dt).float()

    def layer(inp, nblocks, mask, out, gb):
        frs = []
        for j in range(nblocks):
            a = st.block([inp], False, to_frags=False) * mask[:, 32 * j:32 * j + 32]
            gb[32 * j:32 * j + 32] += a.sum(0)
            y = a.to(dt).float()
            out[:, 32 * j:32 * j + 32] = y.to(out.dtype)
            frs += [y[:, emu._P], y[:, 16 + emu._P]]
        return frs
    m = [emu._BITS[b.data_ptr()].float() for b in bits]
    p = layer([g], 4, m[0], dC[0], g_bias[0])
    p = layer(p, 4, m[1], dC[1], g_bias[1])
    p = layer(p, 4, m[2], dC[2], g_bias[2])
    layer(p, 32, m[3], dB, g_bias[3])
    assert st.f == 324


@contextlib.contextmanager
def emulate_ops_colour_fp16():
    """emulate_ops_fp16() with the dtype-following models of fcolour_fwd and fcolour_bwd"""
    with emu16.emulate_ops_fp16() as ops:
        saved = (ops.fcolour_fwd, ops.fcolour_bwd)
        ops.fcolour_fwd, ops.fcolour_bwd = fcolour_fwd, fcolour_bwd
        try:
            yield ops
        finally:
            ops.fcolour_fwd, ops.fcolour_bwd = saved
