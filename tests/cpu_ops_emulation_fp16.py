"""CPU emulation with the two fused-kernel models that hard-code bf16 replaced by dtype-following ones, for the fp16 flavour of the fused
256-wide networks (csrc/fmlp.hip: fmlp_kernel<.., F16>, fchain_bwd_kernel<.., F16>).

tests/cpu_ops_emulation.py models `fmlp_classic_pts_fwd` with embeddings padded into bf16 and `fchain_bwd` with d_raw and every dz rounded
to bf16; the kernels round to the dtype of the weight stream.  `emulate_ops_fp16()` enters `emulate_ops()` and then overrides those two
names on snerf_amd.ops with copies whose rounding type is `stream.dtype` (for a bf16 stream they are the originals, value for value)."""
import contextlib

import torch

import cpu_ops_emulation as emu
from oracle import classic as oc


def fmlp_classic_pts_fwd(pts, viewdirs, S, stream, bias, raw):
    M = pts.shape[0]
    pad = lambda t, w: torch.cat([t, torch.zeros(M, w - t.shape[1])], -1).to(stream.dtype)
    emu.fmlp_classic_fwd(pad(oc.embed(pts, 10), 64), pad(oc.embed(viewdirs[:, None].expand(-1, S, -1).reshape(-1, 3), 4), 64), stream, bias, raw)


def fchain_bwd(net, d_raw, stream, bits, dz, g_bias):
    """model of fchain_bwd_kernel in either flavour: the data-gradient chains of the 256-wide networks on the transposed weights
    (masks, stores in the stream's 16-bit type, bias gradients = column sums of the stored gradients)"""
    classic = net == 0
    assert stream.shape[0] == (1104 if classic else 400)
    dt = stream.dtype
    st = emu._FStream(stream, torch.zeros(80 * 32))
    M = d_raw.shape[0]
    d_raw = d_raw.reshape(M, -1)

    def head(cols):
        g = torch.zeros(M, 16)
        g[:, :len(cols)] = d_raw[:, cols].to(dt).float()
        return g

    def layer(segs, nblocks, mask, out, gb):
        frs = []
        for j in range(nblocks):
            a = st.block(segs, False, to_frags=False)
            if mask is not None:
                a = a * mask[:, 32 * j:32 * j + 32]
            y = a.to(dt).float()
            gb[32 * j:32 * j + 32] += y.sum(0)
            out[:, 32 * j:32 * j + 32] = y.to(out.dtype)
            frs += [y[:, emu._P], y[:, 16 + emu._P]]
        return frs
    m = [emu._BITS[b.data_ptr()].float() for b in bits]
    if classic:
        p = layer([[head([0, 1, 2])]], 4, m[8][:, :128], dz[0], g_bias[0])
        p = layer([p], 8, None, dz[1], g_bias[1])
        p = layer([p, [head([3])]], 8, m[7], dz[2], g_bias[2])
        for i in range(6, -1, -1):
            p = layer([p], 8, m[i], dz[9 - i], g_bias[9 - i])
        assert st.f == 1100
    else:
        p = layer([[head([0])]], 8, m[3], dz[0], g_bias[0])
        for i in range(2, -1, -1):
            p = layer([p], 8, m[i], dz[3 - i], g_bias[3 - i])
        assert st.f == 392


@contextlib.contextmanager
def emulate_ops_fp16():
    """emulate_ops() with the dtype-following models of fmlp_classic_pts_fwd and fchain_bwd"""
    with emu.emulate_ops() as ops:
        saved = (ops.fmlp_classic_pts_fwd, ops.fchain_bwd)
        ops.fmlp_classic_pts_fwd, ops.fchain_bwd = fmlp_classic_pts_fwd, fchain_bwd
        try:
            yield ops
        finally:
            ops.fmlp_classic_pts_fwd, ops.fchain_bwd = saved
