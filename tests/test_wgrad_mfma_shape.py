"""The two MFMA flavours of the 256 x 256 weight-gradient kernel (gemm_tn8_kernel, MSHAPE = 32 | 16; csrc/gemm.hip) against the float64 product
of the 16-bit-rounded operands.  Both flavours add the same exact products in fp32 and differ only in the order of the additions, so the 16 flavour's
error must stay within 1.5 x the 32 flavour's on the same inputs (+ 1e-7): relative L2 and max-abs over max.  SNERF_WGRAD_MFMA forces the flavour,
SNERF_WGRAD_TN8=1 the 256 x 256 kernel for shapes the launch rules would give to the 128 x 128 one; both are read at launch time.  Every launch runs directly behind a launch of another kernel family that fills LDS, and every
case runs once more with an LDS scribble before every library call (what SNERF_TEST_SCRIBBLE_LDS=1 does for the whole suite)."""
import functools
import importlib.util
import os

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (M, N, K, partial tiles + fold, operands as column ranges of wider buffers)
CASES = [(64, 256, 256, False, False),        # one slice, one k-tile: prologue and the first body only
         (192, 256, 256, False, False),       # slices of two k-tiles and of one: both copies of the body
         (1000, 256, 256, False, False),      # the last k-tile has 40 valid rows (the rest read as zeros through the descriptor)
         (8192, 512, 320, True, False),       # 4 output tiles x 64 slices, k_valid inside a tile; partial tiles + fold
         (8192, 512, 320, False, False),      # ... and fp32 atomics (ops.WGRAD_FOLD off: linear_wgrad would pick the fold for this shape by itself)
         (1000, 256, 320, True, True),        # ldz > N, ldx > K, as the trainer passes them
         (8192, 512, 320, False, True),
         (8192, 1024, 1024, True, False)]     # 16 tiles x 16 slices of 8 k-tiles: the steady state of the k-loop (buffers restaged, s_kt >= 2)


def _plan_tn8(M, N, K):
    """slices and workspace floats of the 256 x 256 kernel's plan (tn_plan in csrc/gemm.hip) for shapes far inside 32-bit offsets"""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = (N // 256) * ((K + 255) // 256)
    mc = -(-M // max(1, n_cu // tiles))
    mc = -(-mc // 128) * 128
    slices = -(-M // mc)
    return slices, slices * N * (-(-K // 256) * 256)


def _bank_probe():
    spec = importlib.util.spec_from_file_location("tn8_lds_bank_check", os.path.join(REPO, "tools", "probes", "tn8_lds_bank_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_lds_bank_rule_both_flavours():
    """every fragment read of both flavours is conflict-free on its LDS image and lands on the element the MFMA operand map asks for; the
    16 x 16 x 32 read on the 32 flavour's image would be 2-way (why the 16 flavour has its own)"""
    probe = _bank_probe()
    for mshape in (32, 16):
        worst, reads, wrong = probe.check(mshape)
        print(f"MEASURED tn8 LDS reads MSHAPE {mshape}: {reads} fragments, worst conflict degree {worst}, wrong elements {wrong}")
        assert reads == 64 and worst == 1 and wrong == 0
    assert probe.naive_16_on_32_image() == 2
    assert probe.main() == 0


@functools.lru_cache(maxsize=None)
def _operands(dt_name, M, N, K):
    """random operands of mixed sign with about half zeros (as after ReLU and its mask), rounded to 16 bits, and their float64 product"""
    tdt = getattr(torch, dt_name)
    g = torch.Generator().manual_seed(1000 * M + N + K)
    dZ = (torch.randn(M, N, generator=g) * (torch.rand(M, N, generator=g) < 0.5)).to(tdt)
    X = (torch.randn(M, K, generator=g) * (torch.rand(M, K, generator=g) < 0.5)).to(tdt)
    ref = dZ.double().t() @ X.double()
    return dZ, X, ref


def _errors(dW, ref):
    d = dW.double().cpu() - ref
    return (d.norm() / ref.norm()).item(), (d.abs().max() / ref.abs().max()).item()


@pytest.mark.gpu
@pytest.mark.parametrize("scribble", [False, True], ids=["behind_nt", "lds_scribbled"])
@pytest.mark.parametrize("dt_name", ["bfloat16", "float16"])
@pytest.mark.parametrize("M,N,K,fold,wide", CASES)
def test_mshape16_against_mshape32(monkeypatch, M, N, K, fold, wide, dt_name, scribble):
    from snerf_amd import _lib, ops
    dt = ops.BF16 if dt_name == "bfloat16" else ops.F16
    tdt = ops.torch_dtype(dt)
    dZc, Xc, ref = _operands(dt_name, M, N, K)
    if wide:
        zbuf = torch.full((M, N + 136), 7.0, dtype=tdt); zbuf[:, 72:72 + N] = dZc
        xbuf = torch.full((M, K + 72), -5.0, dtype=tdt); xbuf[:, 8:8 + K] = Xc         # neighbours of the column ranges must not leak in
        dZ, X = zbuf.cuda()[:, 72:72 + N], xbuf.cuda()[:, 8:8 + K]
    else:
        dZ, X = dZc.cuda(), Xc.cuda()
    # the launch in front: an NT forward of the persistent 8-phase kernel, which leaves its own tiles in LDS
    A = torch.randn(512, 256, generator=torch.Generator().manual_seed(5)).to(tdt).cuda()
    W = torch.randn(256, 256, generator=torch.Generator().manual_seed(6)).to(tdt).cuda()
    Y = torch.empty(512, 256, dtype=tdt, device="cuda")
    real, n, called = _lib.call, [0], []

    def call(name, *args):
        if name != "snerf_debug_lds_scribble":
            called.append(name)
            if scribble:
                n[0] += 1
                real("snerf_debug_lds_scribble", (n[0] * 2654435761) & 0x7fffffff, ops._stream())
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", call)
    if not fold:
        monkeypatch.setattr(ops, "WGRAD_FOLD", False)                                   # (as tests/test_gpu_kernels.py does for its atomic cases)
    monkeypatch.setenv("SNERF_WGRAD_TN8", "1")

    # which kernel the library plans: the 256 x 256 kernel's workspace under either flavour, and not what the default rules give this shape
    slices, ws_tn8 = _plan_tn8(M, N, K)
    for mshape in ("16", "32"):
        monkeypatch.setenv("SNERF_WGRAD_MFMA", mshape)
        assert _lib.query("snerf_linear_wgrad_ws_floats", M, N, K, dZ.stride(0), X.stride(0), dt, 2) == ws_tn8
    if (M, N, K) not in ((64, 256, 256), (8192, 1024, 1024)):                           # (one slice of one tile either way; the default's own shape)
        monkeypatch.delenv("SNERF_WGRAD_TN8")
        assert _lib.query("snerf_linear_wgrad_ws_floats", M, N, K, dZ.stride(0), X.stride(0), dt, 2) != ws_tn8
        monkeypatch.setenv("SNERF_WGRAD_TN8", "1")

    def launch(mshape):
        monkeypatch.setenv("SNERF_WGRAD_MFMA", str(mshape))
        buf = torch.full((N + 2, K + 8), 3.0, dtype=torch.float32, device="cuda")
        dW = buf[1:N + 1, 4:4 + K]
        dW.zero_()
        ops.linear_fwd(A, W, None, Y, 256, 256, ops.ACT_RELU, dt, variant=8)
        del called[:]
        ops.linear_wgrad(dZ, X, dW, N, K, dt, variant=2, deterministic=fold)
        assert called == ["snerf_linear_wgrad_det" if fold else "snerf_linear_wgrad"], called     # partial tiles + fold / fp32 atomics, as the case says
        out = dW.clone()
        dW.fill_(3.0)
        assert bool((buf == 3.0).all()), f"MSHAPE {mshape}: wrote outside dW[:n_valid, :k_valid]"
        return out

    d32, d16 = launch(32), launch(16)
    (l2_32, mx_32), (l2_16, mx_16) = _errors(d32, ref), _errors(d16, ref)
    tag = f"M={M} N={N} K={K} {slices} slices {dt_name} {'fold' if fold else 'atomics'}{' wide' if wide else ''}{' scribbled' if scribble else ''}"
    print(f"MEASURED wgrad MSHAPE 32 {tag}: rel L2 {l2_32:.3e}, max-abs/max {mx_32:.3e}")
    print(f"MEASURED wgrad MSHAPE 16 {tag}: rel L2 {l2_16:.3e}, max-abs/max {mx_16:.3e}, bit-identical to MSHAPE 32: {torch.equal(d16, d32)}")
    # the yardstick kernel itself: fp32 accumulation of exact products, at worst one rounding of 2^-24 relative per added row
    assert l2_32 <= M * 2.0 ** -24, f"the 32 flavour is off by itself: rel L2 {l2_32:.3e}"
    assert l2_16 <= 1.5 * l2_32 + 1e-7, f"rel L2 {l2_16:.3e} (16) vs {l2_32:.3e} (32)"
    assert mx_16 <= 1.5 * mx_32 + 1e-7, f"max-abs/max {mx_16:.3e} (16) vs {mx_32:.3e} (32)"
    if fold:
        assert torch.equal(d16, launch(16)), "two launches through partial tiles on the same inputs differ"
