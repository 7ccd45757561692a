"""Frame metrics (snerf_amd.metrics, snerf_frame_metrics): PSNR and SSIM of rendered frames.

Without a GPU: the host model against a literal restatement of what skimage's structural_similarity calls (scipy's uniform_filter on
float64 casts), the quantisation and grey rules, the library's refusals, MetricHarness / EvalMeter on host inputs.
On the GPU: the kernel against the host model at the smallest shapes at which each piece of its indexing can go wrong, and one full frame.

Tolerances (each derived, none tuned):
  mse_u8           bit-equal: an exact integer sum and one correctly rounded division on both sides
  psnr_u8, psnr_f  relative 1e-12: log implementations differ by ulps
  mse_f            relative 1e-12: both sides sum the same fp32 squares in double, in different orders
  ssim             absolute 1e-10 (1e-9 for the 1280 x 1920 frame): each S carries about 1e-15 of rounding (C2 = 58.5 bounds the
                   cancellation in Sxx / 49 - ux^2), the summation-order bound n eps is 3e-13 at n <= 2500 and 2.7e-10 at 2.4 M outputs
  host model vs the skimage restatement: |d ssim| <= 1e-12 (they differ in the order of exact integer sums and a few double roundings)"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from snerf_amd import _lib, metrics, ops

gpu = pytest.mark.gpu

SHAPES = [(1, 7, 7), (1, 7, 40), (1, 40, 7), (1, 8, 39), (1, 39, 8), (1, 38, 38), (1, 45, 70), (3, 45, 70)]
CONTENTS = ["identical", "constant", "independent", "noise", "span"]
GRAYS = ["cv4", "cv3"]
SSIM_0_VS_255 = 9.999000099990003e-05
METER_FRAMES = [((1, 8, 39), "noise"), ((1, 38, 38), "independent"), ((1, 45, 70), "span")]   # frames of different sizes and PSNRs
CONSTANT_PAIRS = [(0, 255), (255, 0), (64, 192)]            # (pred, gt) levels of frame 0, 1, 2


def decode(k):
    """uint8 -> the fp32 image the batchers decode it to"""
    return (k.astype(np.float64) / 255.0).astype(np.float32)


_cases = {}


def case(shape, content, u8):
    """-> (pred fp32 [F,H,W,3], gt fp32 or uint8 [F,H,W,3]) from a seeded generator; built once and never written to"""
    key = (shape, content, u8)
    if key not in _cases:
        F, H, W = shape
        rng = np.random.default_rng([F, H, W, CONTENTS.index(content), int(u8)])
        gt8 = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
        gtf = decode(gt8) if u8 else rng.random((F, H, W, 3), dtype=np.float32)
        if content == "identical":
            pred = gtf.copy()
        elif content == "constant":
            pred, gt8 = np.empty((F, H, W, 3), np.float32), np.empty((F, H, W, 3), np.uint8)
            for f in range(F):
                pred[f], gt8[f] = decode(np.uint8(CONSTANT_PAIRS[f][0])), CONSTANT_PAIRS[f][1]
            gtf = decode(gt8)
        elif content == "independent":
            pred = rng.random((F, H, W, 3), dtype=np.float32)
        elif content == "noise":
            pred = gtf + rng.uniform(-20. / 255., 20. / 255., (F, H, W, 3)).astype(np.float32)
        else:                                                                   # every sample of [-0.001, 1.001], in a shuffled order
            pred = rng.permutation(np.linspace(-0.001, 1.001, F * H * W * 3, dtype=np.float32)).reshape(F, H, W, 3)
        pred.setflags(write=False)
        gt = gt8 if u8 else gtf
        gt.setflags(write=False)
        _cases[key] = (pred, gt)
    return _cases[key]


_refs = {}


def host_ref(shape, content, u8, gray):
    key = (shape, content, u8, gray)
    if key not in _refs:
        _refs[key] = metrics.frame_metrics_host(*case(shape, content, u8), gray=gray)
        _refs[key].setflags(write=False)
    return _refs[key]


def check_rows(got, ref, ssim_tol=1e-10, what=""):
    """got, ref float64 [F,5]: the tolerances of the module docstring, every figure printed before it is asserted"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == np.float64
    for f in range(ref.shape[0]):
        g, r = dict(zip(ops.FRAME_METRIC_NAMES, got[f])), dict(zip(ops.FRAME_METRIC_NAMES, ref[f]))
        print(what, "frame", f, "got", got[f].tolist(), "ref", ref[f].tolist())
        assert g["mse_u8"] == r["mse_u8"], (what, f, g["mse_u8"], r["mse_u8"])
        for name in ("psnr_u8", "psnr_f", "mse_f"):
            if np.isinf(r[name]) or r[name] == 0.:
                assert g[name] == r[name], (what, f, name, g[name], r[name])
            else:
                assert abs(g[name] - r[name]) <= 1e-12 * abs(r[name]), (what, f, name, g[name], r[name])
        assert abs(g["ssim"] - r["ssim"]) <= ssim_tol, (what, f, g["ssim"], r["ssim"])


# ------------------------------------------------------------------ without a GPU ----
def skimage_restated(gx, gy):
    """structural_similarity(gx, gy, data_range=255) of two uint8 grey images as skimage documents it, with the calls it makes itself"""
    from scipy.ndimage import uniform_filter
    gx, gy = gx.astype(np.float64), gy.astype(np.float64)
    NP = 7 ** 2
    cov_norm = NP / (NP - 1)
    ux, uy = uniform_filter(gx, size=7), uniform_filter(gy, size=7)
    uxx, uyy, uxy = uniform_filter(gx * gx, size=7), uniform_filter(gy * gy, size=7), uniform_filter(gx * gy, size=7)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    A1, A2, B1, B2 = 2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2
    S = (A1 * A2) / (B1 * B2)
    return S[3:-3, 3:-3].mean(dtype=np.float64)


@pytest.mark.parametrize("shape", SHAPES + [(1, 128, 200)], ids=lambda s: "x".join(map(str, s)))
def test_host_model_against_the_skimage_restatement(shape):
    worst = 0.
    for content, u8, gray in itertools.product(CONTENTS, (False, True), GRAYS):
        pred, gt = case(shape, content, u8)
        ref = host_ref(shape, content, u8, gray)
        for f in range(shape[0]):
            qp, qg = metrics.quantise(pred[f]), gt[f] if u8 else metrics.quantise(gt[f])
            gp, gg = metrics.to_gray(qp, gray).astype(np.uint8), metrics.to_gray(qg, gray).astype(np.uint8)
            d = abs(ref[f, 4] - skimage_restated(gp, gg))
            worst = max(worst, d)
            assert d <= 1e-12, (content, u8, gray, f, ref[f, 4], d)
            assert ref[f, 2] == np.mean((qp.astype(np.float64) - qg) ** 2)                              # skimage's mean_squared_error, bit for bit
            if content == "identical":
                assert ref[f, 4] == 1.0 and ref[f, 3] == np.inf and ref[f, 0] == 0. and ref[f, 1] == np.inf
    print("largest |ssim host model - skimage restatement|:", worst)
    assert abs(host_ref(shape, "constant", True, "cv4")[0, 4] - SSIM_0_VS_255) <= 1e-15


def test_quantisation():
    k = np.arange(256)
    assert np.array_equal(metrics.quantise((k / 255.0).astype(np.float32)), k)                          # the double division
    assert np.array_equal(metrics.quantise(k.astype(np.float32) / np.float32(255.0)), k)                # the fp32 division
    x = np.array([-0.001, 1.001, -5., 7., np.nan, np.inf, -np.inf, -0., 0.999, 1. / 255., 0.5], dtype=np.float32)
    assert metrics.quantise(x).tolist() == [0, 255, 0, 255, 0, 255, 0, 0, 254, 1, 127]
    inside = np.linspace(-0.0039, 1.0039, 4001, dtype=np.float32)                                       # where numpy's own cast is defined
    assert np.array_equal(metrics.quantise(inside), (inside * 255).astype(np.uint8))


def test_grey_weights():
    lv = np.array([0, 1, 127, 128, 254, 255])
    rgb = np.array(list(itertools.product(lv, lv, lv)), dtype=np.uint8)
    for gray, (wr, wg, wb, shift) in (("cv4", (9798, 19235, 3735, 15)), ("cv3", (4899, 9617, 1868, 14))):
        assert metrics.GRAY_WEIGHTS[gray] == (wr, wg, wb, shift) and wr + wg + wb == 1 << shift
        want = [(int(r) * wr + int(g) * wg + int(b) * wb + (1 << (shift - 1))) >> shift for r, g, b in rgb]
        assert metrics.to_gray(rgb, gray).tolist() == want
        assert metrics.to_gray(rgb, (wr, wg, wb, shift)).tolist() == want
        k = np.arange(256, dtype=np.uint8)
        assert np.array_equal(metrics.to_gray(np.stack([k, k, k], -1), gray), k)


def test_refusals_without_a_gpu():
    """argument validation happens before any launch; the buffers are host memory that a refused call never touches"""
    assert ops.frame_metrics_ws(1, 6, 9) == 0 and ops.frame_metrics_ws(1, 9, 6) == 0 and ops.frame_metrics_ws(0, 9, 9) == 0
    need = ops.frame_metrics_ws(2, 9, 12)
    assert need >= 2 * 24 and ops.frame_metrics_ws(1, 7, 7) > 0
    buf = lambda n: ctypes.create_string_buffer(n)
    pred, gt, ws, out = buf(2 * 9 * 12 * 12), buf(2 * 9 * 12 * 12), buf(need), buf(2 * 5 * 8)
    gw = lambda *w: (ctypes.c_int * 4)(*w)
    good = dict(pred=pred, gt=gt, u8=0, F=2, H=9, W=12, gray_w=None, ws=ws, ws_bytes=need, out=out)
    bad = [dict(pred=None), dict(gt=None), dict(ws=None), dict(out=None), dict(F=0), dict(F=-1), dict(H=6), dict(W=6),
           dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(gray_w=gw(9798, 19235, 3735, 0)), dict(gray_w=gw(9798, 19235, 3735, 21)),
           dict(gray_w=gw(-1, 19235, 3735, 15)), dict(gray_w=gw(9798, -19235, 3735, 15)), dict(gray_w=gw(9798, 19235, -3735, 15)),
           dict(gray_w=gw(9798, 19235, 3736, 15))]
    for change in bad:
        a = dict(good, **change)
        with pytest.raises(_lib.SnerfHipError, match="bad argument"):
            _lib.call("snerf_frame_metrics", a["pred"], a["gt"], a["u8"], a["F"], a["H"], a["W"], a["gray_w"], a["ws"], a["ws_bytes"], a["out"], None)
    with pytest.raises(AssertionError):
        metrics.gray_weights((1, 1, 1, 0))
    assert ops.FRAME_METRIC_NAMES == ("mse_f", "psnr_f", "mse_u8", "psnr_u8", "ssim")


def test_metric_harness_on_numpy_inputs():
    pred, gt = case((1, 45, 70), "noise", False)
    got = metrics.MetricHarness()(pred[0], gt[0], name_fn=lambda s: "test_" + s)
    ref = host_ref((1, 45, 70), "noise", False, "cv4")[0]
    assert set(got) == {"test_psnr", "test_ssim"} and type(got["test_psnr"]) is float and type(got["test_ssim"]) is float
    assert got["test_psnr"] == ref[3] and got["test_ssim"] == ref[4]
    assert set(metrics.MetricHarness(gray="cv3")(pred[0], gt[0])) == {"psnr", "ssim"}


def test_eval_meter_on_cpu_tensors_is_the_mean_of_the_frame_psnrs():
    meter = metrics.EvalMeter(capacity=1)                                       # grows twice
    rows = []
    for shape, content in METER_FRAMES:
        pred, gt = (torch.from_numpy(v[0].copy()) for v in case(shape, content, False))
        meter.add(pred, gt)
        rows.append(host_ref(shape, content, False, "cv4")[0])
        mse = ((pred.double() - gt.double()) ** 2).mean()
        # d is rounded to fp32 in the metric (eval.py's own arithmetic): at most 6e-8 relative per sample, 1.2e-7 on the MSE, 5.2e-7 dB
        assert abs(float(meter.psnr(pred, gt)) - float(metrics.mse_to_psnr(mse))) < 1e-6
    rows = np.stack(rows)
    res = meter.result()
    assert np.array_equal(res["frames"], rows)
    assert res["psnr"] == rows[:, 1].mean() and res["psnr_u8"] == rows[:, 3].mean() and res["ssim"] == rows[:, 4].mean()
    assert abs(res["psnr"] - metrics.mse_to_psnr(rows[:, 0].mean())) > 1e-6     # not the PSNR of the mean MSE
    ident = torch.from_numpy(case((1, 7, 7), "identical", False)[0][0].copy())
    meter.add(ident, ident)
    assert meter.result()["psnr_u8"] == np.inf and meter.result()["frames"].shape == (4, 5)


def test_conversions():
    assert abs(metrics.mse_to_psnr(0.01) - 20.) < 1e-12 and abs(metrics.psnr_to_mse(20.) - 0.01) < 1e-15
    assert np.allclose(metrics.psnr_to_mse(metrics.mse_to_psnr(np.array([0.5, 0.001]))), [0.5, 0.001], rtol=1e-14, atol=0)
    t = metrics.mse_to_psnr(torch.tensor([0.01], dtype=torch.float64))
    assert torch.is_tensor(t) and abs(float(t) - 20.) < 1e-12 and abs(float(metrics.psnr_to_mse(t)) - 0.01) < 1e-15
    assert metrics.ssim_to_dssim(0.5) == 0.25 and metrics.dssim_to_ssim(0.25) == 0.5
    assert metrics.dssim_to_ssim(metrics.ssim_to_dssim(torch.tensor(0.75))) == 0.75


# ------------------------------------------------------------------ on the GPU ----
@gpu
@pytest.mark.parametrize("gray", GRAYS)
@pytest.mark.parametrize("u8", (False, True), ids=("f32", "u8"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_against_the_host_model(shape, u8, gray):
    for content in CONTENTS:
        pred, gt = (torch.from_numpy(v.copy()).cuda() for v in case(shape, content, u8))
        ref = host_ref(shape, content, u8, gray)
        got = metrics.frame_metrics(pred, gt, gray=gray)
        assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (shape[0], 5)
        got = got.cpu().numpy()
        check_rows(got, ref, what=f"{shape} {content} u8={u8} {gray}")
        if content == "identical":
            assert (got[:, 4] == 1.0).all() and (got[:, 3] == np.inf).all() and (got[:, 0] == 0.).all()
        if content == "constant":
            assert abs(got[0, 4] - SSIM_0_VS_255) <= 1e-10


@gpu
def test_a_single_frame_needs_no_frame_axis():
    pred, gt = (torch.from_numpy(v[0].copy()).cuda() for v in case((1, 45, 70), "noise", True))
    check_rows(ops.frame_metrics(pred, gt).cpu().numpy(), host_ref((1, 45, 70), "noise", True, "cv4"))


@gpu
def test_full_size_frame():
    H, W = 1280, 1920
    rng = np.random.default_rng(1280)
    gt = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    pred = decode(gt) + rng.uniform(-20. / 255., 20. / 255., (H, W, 3)).astype(np.float32)
    ref = metrics.frame_metrics_host(pred, gt)
    got = metrics.frame_metrics(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()).cpu().numpy()
    check_rows(got, ref, ssim_tol=1e-9, what="1280x1920")


@gpu
def test_bit_reproducible_and_graph_capturable():
    shape = (3, 45, 70)
    pred, gt = (torch.from_numpy(v.copy()).cuda() for v in case(shape, "noise", True))
    eager = ops.frame_metrics(pred, gt)
    again = ops.frame_metrics(pred, gt)
    assert torch.equal(eager.view(torch.int64), again.view(torch.int64))
    out = torch.zeros(3, 5, dtype=torch.float64, device="cuda")
    ws = torch.empty(ops.frame_metrics_ws(*shape), dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.frame_metrics(pred, gt, out=out, ws=ws)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.frame_metrics(pred, gt, out=out, ws=ws)
    for _ in range(2):
        out.fill_(3.0)
        ws.fill_(0xff)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int64), eager.view(torch.int64))


@gpu
def test_metric_harness_and_eval_meter_on_device_tensors():
    pred, gt = (torch.from_numpy(v[0].copy()).cuda() for v in case((1, 45, 70), "noise", False))
    got = metrics.MetricHarness()(pred, gt, name_fn=lambda s: "test_" + s)
    ref = host_ref((1, 45, 70), "noise", False, "cv4")[0]
    assert type(got["test_psnr"]) is float and type(got["test_ssim"]) is float
    assert abs(got["test_psnr"] - ref[3]) <= 1e-12 * abs(ref[3]) and abs(got["test_ssim"] - ref[4]) <= 1e-10
    meter = metrics.EvalMeter(capacity=1)
    rows = []
    for shape, content in METER_FRAMES:
        pred, gt = (torch.from_numpy(v[0].copy()).cuda() for v in case(shape, content, True))
        meter.add(pred, gt)
        rows.append(host_ref(shape, content, True, "cv4")[0])
        p = meter.psnr(pred, gt)
        assert p.is_cuda and p.dim() == 0 and abs(float(p) - rows[-1][1]) <= 1e-12 * abs(rows[-1][1])
    rows = np.stack(rows)
    res = meter.result()
    check_rows(res["frames"], rows, what="EvalMeter")
    assert res["psnr"] == res["frames"][:, 1].mean() and abs(res["psnr"] - rows[:, 1].mean()) <= 1e-12 * abs(rows[:, 1].mean())
    assert abs(res["psnr_u8"] - rows[:, 3].mean()) <= 1e-12 * abs(rows[:, 3].mean()) and abs(res["ssim"] - rows[:, 4].mean()) <= 1e-10
