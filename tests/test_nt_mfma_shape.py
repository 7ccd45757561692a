"""The two MFMA flavours of the persistent NT kernel (gemm_nt8p_kernel, MSHAPE = 32 | 16; csrc/gemm.hip) through snerf_linear_fwd, bf16, against
the float64 product of the rounded operands.  SNERF_NT_MFMA = 16 | 32 forces the flavour (read at launch time; it picks the flavour and nothing
else).  Every case runs both flavours on the same inputs, three times: plainly, directly behind a launch of another persistent GEMM (which leaves
its own tiles, bias and mask words in LDS), and with an LDS scribble before every library call (what SNERF_TEST_SCRIBBLE_LDS=1 does for the suite).

Bounds (derived, the same for both flavours):
  output       |y - ref| <= 2^-8 |ref| + K 2^-23 (|A| |W|^T): one rounding of the output to bf16, fp32 accumulation of exact products
  produced bits  bit == (stored y > 0), exactly, for every stored element
  column sums  against the float64 column sums of the launch's OWN stored output, within M 2^-24 sum|y| per column (fp32 additions of M values)
  padding      rows >= M and columns >= n_store of Y keep their sentinel
The mask words an ACT_MASK_BITS launch consumes come from an ACT_RELU_BITS launch of the OTHER flavour: the layout is shared."""
import functools
import importlib.util
import os

import pytest
import torch

# (M, N, K, n_store); K >= 192: K = 128 has instantiations of its own, which stay on the 32 flavour
CASES = [(200, 256, 192, 256),        # one ragged tile; an odd number of k-tiles
         (256, 256, 256, 200),        # an even number of k-tiles; the col_ok edge inside a lane group
         (1000, 512, 1088, 512),      # the step's K: 17 k-tiles
         (22100, 768, 192, 768)]      # 261 tiles on 256 workgroups: a second tile per workgroup, ragged last row tile, a column-block change (early flush_colsum)
SENTINEL = 7.0
PAD_ROWS = 3
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lds_addressing_both_flavours():
    """every fragment read, slab write and read-back of both flavours lands on the element the MFMA operand / accumulator map asks for, the reads are
    conflict-free on the shared images, and no instruction of the 16 flavour has a higher conflict degree than its 32 counterpart"""
    spec = importlib.util.spec_from_file_location("nt8p_lds_bank_check", os.path.join(REPO, "tools", "probes", "nt8p_lds_bank_check.py"))
    probe = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(probe)
    r32, r16 = probe.check(32), probe.check(16)
    for r in (r32, r16):
        assert r["wrong"] == 0 and r["frag_reads"] == 16 and r["frag_worst"] == 1 and r["readback_worst"] == 1
    assert r16["write_worst"] <= r32["write_worst"]
    assert probe.main() == 0


@functools.lru_cache(maxsize=None)
def _case(M, N, K):
    """operands rounded to bf16, a bias, a bf16 mask source, and (float64, on the device) their product and the magnitude term of the bound"""
    g = torch.Generator().manual_seed(7 * M + 3 * N + K)
    A = torch.randn(M, K, generator=g).to(torch.bfloat16)
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16)
    bias = torch.randn(N, generator=g)
    aux = torch.randn(M, N, generator=g).to(torch.bfloat16)
    Ad, Wd = A.cuda().double(), W.cuda().double()
    prod = Ad @ Wd.t()
    mag = Ad.abs() @ Wd.abs().t()
    return A.cuda(), W.cuda(), bias.cuda(), aux.cuda(), prod, mag


def _decode_bits(words, M, N):
    """[M, N] bool from the mask words: word `lane` of block (32-row block rb, 64-column group cg) holds in bit 8 it + e the element at
    row 32 rb + 8 it + (lane >> 3), column 64 cg + 8 (lane & 7) + e"""
    rbs, ncg = 8 * ((M + 255) // 256), N // 64
    w = words[:rbs * ncg * 64].view(rbs, ncg, 8, 8, 1)                        # [rb, cg, prow, pch, 1]
    sh = torch.arange(32, device=words.device, dtype=torch.int32)
    b = ((w >> sh) & 1).view(rbs, ncg, 8, 8, 4, 8)                            # [rb, cg, prow, pch, it, e]
    return b.permute(0, 4, 2, 1, 3, 5).reshape(rbs * 32, N)[:M].bool()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["plain", "behind_nt", "lds_scribbled"])
@pytest.mark.parametrize("M,N,K,n_store", CASES)
def test_nt8p_mshape16_and_mshape32(monkeypatch, M, N, K, n_store, mode):
    from snerf_amd import _lib, ops
    dt = ops.BF16
    A, W, bias, aux, prod, mag = _case(M, N, K)
    tol_acc = K * 2.0 ** -23 * mag[:, :n_store]
    # the launch in front: another shape, another flavour of the persistent kernel
    A0 = torch.randn(512, 256, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16).cuda()
    W0 = torch.randn(256, 256, generator=torch.Generator().manual_seed(6)).to(torch.bfloat16).cuda()
    b0 = torch.randn(256, generator=torch.Generator().manual_seed(7)).cuda()
    Y0 = torch.empty(512, 256, dtype=torch.bfloat16, device="cuda")
    real, n = _lib.call, [0]
    if mode == "lds_scribbled":
        def call(name, *args):
            if name != "snerf_debug_lds_scribble":
                n[0] += 1
                real("snerf_debug_lds_scribble", (n[0] * 2654435761) & 0x7fffffff, ops._stream())
            return real(name, *args)
        monkeypatch.setattr(_lib, "call", call)
    assert ops.relu_bits_ok(A, W, torch.empty(M, N, dtype=torch.bfloat16, device="cuda"), K, n_store, dt, 8)    # the persistent kernel's conditions hold

    def launch(mshape, act, with_bias=False, aux=None, colsum=False):
        monkeypatch.setenv("SNERF_NT_MFMA", str(mshape))
        buf = torch.full((M + PAD_ROWS, N), SENTINEL, dtype=torch.bfloat16, device="cuda")
        cs = torch.zeros(N, dtype=torch.float32, device="cuda") if colsum else None
        if mode == "behind_nt":
            ops.linear_fwd(A0, W0, b0, Y0, 256, 256, ops.ACT_RELU, dt, variant=8)
        ops.linear_fwd(A, W, bias if with_bias else None, buf[:M], K, n_store, act, dt, aux=aux, colsum=cs, variant=8)
        assert bool((buf[M:] == SENTINEL).all()) and bool((buf[:M, n_store:] == SENTINEL).all()), f"MSHAPE {mshape} act {act}: wrote outside Y[:M, :n_store]"
        return buf[:M, :n_store], cs

    def check_one(name, mshape, y, ref, same=None):
        d = (y.double() - ref).abs()
        print(f"MEASURED nt8p MSHAPE {mshape} {name} M={M} N={N} K={K} n_store={n_store} {mode}: rel L2 {(d.norm() / ref.norm()).item():.3e}, "
              f"max-abs {d.max().item():.3e}" + ("" if same is None else f", bit-identical to MSHAPE 32: {same}"))
        bad = int((d > 2.0 ** -8 * ref.abs() + tol_acc).sum())
        assert bad == 0, f"MSHAPE {mshape} {name}: {bad} elements outside the bound"

    def check(name, outs, ref):
        check_one(name, 32, outs[32], ref)
        check_one(name, 16, outs[16], ref, torch.equal(outs[16], outs[32]))

    biased = (prod + bias.double())[:, :n_store]
    check("none + bias", {m: launch(m, ops.ACT_NONE, True)[0] for m in (32, 16)}, biased)
    check("relu + bias", {m: launch(m, ops.ACT_RELU, True)[0] for m in (32, 16)}, torch.relu(biased))
    h, bits = {}, {}
    for m in (32, 16):
        bits[m] = torch.zeros(ops.mask_bits_words(M, N), dtype=torch.int32, device="cuda")
        h[m] = launch(m, ops.ACT_RELU_BITS, True, aux=bits[m])[0]
        got = _decode_bits(bits[m], M, N)[:, :n_store]
        assert torch.equal(got, h[m] > 0), f"MSHAPE {m}: {int((got != (h[m] > 0)).sum())} mask bits differ from (stored y > 0)"
    check("relu_bits + bias", h, torch.relu(biased))
    assert 0.2 < float((h[32] > 0).float().mean()) < 0.8
    check("mask", {m: launch(m, ops.ACT_MASK, aux=aux)[0] for m in (32, 16)}, prod[:, :n_store] * (aux[:, :n_store] > 0))
    other = {32: 16, 16: 32}
    for with_cs in (False, True):
        outs = {}
        for m in (32, 16):
            outs[m], cs = launch(m, ops.ACT_MASK_BITS, aux=bits[other[m]], colsum=with_cs)
            assert torch.equal(outs[m] != 0, (outs[m] != 0) & (h[other[m]] > 0)), f"MSHAPE {m}: a masked element is not zero"
            if with_cs:
                y = outs[m].double()
                err = (cs[:n_store].double() - y.sum(0)).abs()
                bound = M * 2.0 ** -24 * y.abs().sum(0)
                print(f"MEASURED nt8p MSHAPE {m} column sums M={M} N={N} K={K} {mode}: max err {err.max().item():.3e}, smallest bound {bound.min().item():.3e}")
                assert bool((err <= bound).all()), f"MSHAPE {m}: column sums off by up to {(err - bound).max().item():.3e} beyond the bound"
        # (the two flavours' producers may differ in a rounding, so each consumer is checked against its own mask)
        for m in (32, 16):
            check_one(f"mask_bits{' + colsum' if with_cs else ''} (mask words of MSHAPE {other[m]})", m, outs[m], prod[:, :n_store] * (h[other[m]] > 0),
                      torch.equal(outs[16], outs[32]) if m == 16 else None)
