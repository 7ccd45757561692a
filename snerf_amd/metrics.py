"""Image metrics of rendered frames, computed where the frame is: on the device.

  frame_metrics        device tensors in, a float64 [F,5] device tensor out (ops.FRAME_METRIC_NAMES); nothing is read back
  frame_metrics_host   the same five numbers per frame in numpy: the host model the kernel is pinned against, and what runs for CPU tensors
  MetricHarness        image.MetricHarness of s-nerfpp/zipnerf (internal/image.py:110-125): {'psnr': uint8 PSNR, 'ssim': grey SSIM}
  EvalMeter            the per-frame PSNR list of s-nerf/eval.py (:152-155, 170, 190-193) as a device table with one host read at the end
  mse_to_psnr, psnr_to_mse, ssim_to_dssim, dssim_to_ssim     internal/image.py:7-24

The arithmetic is that of skimage.metrics.peak_signal_noise_ratio / structural_similarity(data_range=255) on the images quantised as
(x * 255).astype(np.uint8) and grey-converted as OpenCV's 8-bit RGB2GRAY, restated from their documented behaviour (neither package is
needed): see snerf_frame_metrics in include/snerf_hip.h.  Two stated deviations: quantisation saturates (numpy's cast of a value outside
(-1, 256) is undefined), and the grey weights are an argument (GRAY_WEIGHTS) because they differ between OpenCV 3 and 4."""
import numpy as np
import torch

from . import ops

# 8-bit RGB2GRAY as (wr, wg, wb, shift): grey = (r wr + g wg + b wb + (1 << (shift - 1))) >> shift.  "cv4" is the C-ABI's default.
GRAY_WEIGHTS = {"cv4": (9798, 19235, 3735, 15), "cv3": (4899, 9617, 1868, 14)}
SSIM_WIN = 7


def _log(x):
    return torch.log(x) if torch.is_tensor(x) else np.log(x)


def mse_to_psnr(mse):
    """PSNR of an MSE (the maximum pixel value is 1)"""
    return -10. / np.log(10.) * _log(mse)


def psnr_to_mse(psnr):
    """MSE of a PSNR (the maximum pixel value is 1)"""
    x = -0.1 * np.log(10.) * psnr
    return torch.exp(x) if torch.is_tensor(x) else np.exp(x)


def ssim_to_dssim(ssim):
    return (1 - ssim) / 2


def dssim_to_ssim(dssim):
    return 1 - 2 * dssim


def gray_weights(gray):
    """"cv4" | "cv3" | (wr, wg, wb, shift) -> the tuple of four ints"""
    w = GRAY_WEIGHTS[gray] if isinstance(gray, str) else tuple(int(v) for v in gray)
    ops._require(len(w) == 4 and 1 <= w[3] <= 20 and min(w[:3]) >= 0 and sum(w[:3]) <= 1 << w[3], "gray: (wr, wg, wb, shift)")
    return w


def quantise(x):
    """(x * 255).astype(np.uint8) made total: one fp32 product truncated toward zero, below 0 -> 0, above 255 -> 255, NaN -> 0"""
    p = np.asarray(x, dtype=np.float32) * np.float32(255.)
    with np.errstate(invalid="ignore"):
        p = np.where(p >= 255, np.float32(255.), np.where(p > 0, p, np.float32(0.)))
    return np.trunc(p).astype(np.uint8)


def to_gray(q, gray="cv4"):
    """uint8 [...,3] -> the 8-bit grey image, int64 [...]"""
    wr, wg, wb, shift = gray_weights(gray)
    q = np.asarray(q).astype(np.int64)
    return (q[..., 0] * wr + q[..., 1] * wg + q[..., 2] * wb + (1 << (shift - 1))) >> shift


def _window_sums(a):
    """int64 [H,W] -> the sums over every 7 x 7 window that fits, int64 [H-6,W-6] (exact: two cumulative sums)"""
    c = np.zeros((a.shape[0] + 1, a.shape[1] + 1), dtype=np.int64)
    c[1:, 1:] = a.cumsum(0).cumsum(1)
    n = SSIM_WIN
    return c[n:, n:] - c[:-n, n:] - c[n:, :-n] + c[:-n, :-n]


def ssim_host(gx, gy):
    """skimage's structural_similarity(gx, gy, data_range=255) with its defaults on two grey images [H,W] of integers in 0..255: 7 x 7
    uniform window, K1 = 0.01, K2 = 0.03, sample covariance, border of 3 cropped.  Integer window sums, then float64."""
    gx, gy = np.asarray(gx).astype(np.int64), np.asarray(gy).astype(np.int64)
    ops._require(gx.shape == gy.shape and gx.ndim == 2 and min(gx.shape) >= SSIM_WIN, "the 7 x 7 window must fit")
    NP = float(SSIM_WIN * SSIM_WIN)
    cov = NP / (NP - 1.)
    sx, sy = _window_sums(gx).astype(np.float64), _window_sums(gy).astype(np.float64)
    sxx, syy, sxy = (_window_sums(v).astype(np.float64) for v in (gx * gx, gy * gy, gx * gy))
    ux, uy = sx / NP, sy / NP
    vx, vy, vxy = cov * (sxx / NP - ux * ux), cov * (syy / NP - uy * uy), cov * (sxy / NP - ux * uy)
    C1, C2 = (0.01 * 255.) ** 2, (0.03 * 255.) ** 2
    S = ((2. * ux * uy + C1) * (2. * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return float(S.sum() / S.size)


def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def frame_metrics_host(pred, gt, gray="cv4"):
    """The host model of snerf_frame_metrics: pred [H,W,3] or [F,H,W,3] floats, gt of the same shape, floats or uint8 -> float64 [F,5]
    in the order of ops.FRAME_METRIC_NAMES (numpy arrays or tensors in, a numpy array out)."""
    pred, gt = _np(pred), _np(gt)
    ops._require(pred.ndim in (3, 4) and pred.shape[-1] == 3 and gt.shape == pred.shape, "pred [H,W,3] or [F,H,W,3], gt of the same shape")
    if pred.ndim == 3:
        pred, gt = pred[None], gt[None]
    pred = pred.astype(np.float32, copy=False)
    out = np.empty((pred.shape[0], 5), dtype=np.float64)
    for f in range(pred.shape[0]):
        p, g = pred[f], gt[f]
        if g.dtype == np.uint8:
            qg, g = g, (g.astype(np.float64) / 255.0).astype(np.float32)
        else:
            g = g.astype(np.float32, copy=False)
            qg = quantise(g)
        qp = quantise(p)
        n = float(p.size)
        d = p - g                                                             # fp32
        mse_f = np.float64((d * d).sum(dtype=np.float64)) / n
        e = qp.astype(np.int64) - qg
        mse_u8 = np.float64(int((e * e).sum())) / n
        with np.errstate(divide="ignore"):
            out[f] = (mse_f, -10. / np.log(10.) * np.log(mse_f), mse_u8, 10. * np.log10(255. ** 2 / mse_u8),
                      ssim_host(to_gray(qp, gray), to_gray(qg, gray)))
    return out


def frame_metrics(pred, gt, gray="cv4", out=None, ws=None):
    """pred [H,W,3] or [F,H,W,3] against gt (fp32 or uint8) -> float64 [F,5] (ops.FRAME_METRIC_NAMES) on the tensors' device.  Device
    tensors go through snerf_frame_metrics and nothing is read back (`out` / `ws`: ops.frame_metrics' preallocated buffers, for graph
    capture); CPU tensors go through frame_metrics_host."""
    if not pred.is_cuda:
        return torch.from_numpy(frame_metrics_host(pred, gt, gray))
    if pred.dtype != torch.float32:
        pred = pred.float()
    if gt.dtype not in (torch.uint8, torch.float32):
        gt = gt.float()
    return ops.frame_metrics(pred.contiguous(), gt.contiguous(), None if gray == "cv4" else gray_weights(gray), out=out, ws=ws)


_PSNR_U8, _SSIM = ops.FRAME_METRIC_NAMES.index("psnr_u8"), ops.FRAME_METRIC_NAMES.index("ssim")
_PSNR_F = ops.FRAME_METRIC_NAMES.index("psnr_f")


class MetricHarness:
    """image.MetricHarness with its call signature: harness(rgb_pred, rgb_gt, name_fn) -> {name_fn('psnr'), name_fn('ssim')} as python
    floats, for one frame [H,W,3].  numpy arrays (the drop-in call) run the host model; device tensors run the kernel, and the only
    transfer is the two numbers."""

    def __init__(self, gray="cv4"):
        self.gray = gray

    def __call__(self, rgb_pred, rgb_gt, name_fn=lambda s: s):
        ops._require(rgb_pred.ndim == 3, "one frame [H,W,3]")
        if torch.is_tensor(rgb_pred) and rgb_pred.is_cuda:
            psnr, ssim = frame_metrics(rgb_pred, rgb_gt, self.gray)[0, _PSNR_U8:_SSIM + 1].tolist()
        else:
            row = frame_metrics_host(rgb_pred, rgb_gt, self.gray)[0]
            psnr, ssim = float(row[_PSNR_U8]), float(row[_SSIM])
        return {name_fn('psnr'): psnr, name_fn('ssim'): ssim}


class EvalMeter:
    """eval.py's PSNR list without a host read per frame: add(pred, gt) appends the frame's metrics to a table on the frames' device
    (it grows by doubling), result() reads the table once."""

    def __init__(self, gray="cv4", capacity=16):
        self.gray, self.capacity, self.n, self.table = gray, int(capacity), 0, None

    def add(self, pred, gt):
        """append the metrics of one frame [H,W,3] (or of F frames [F,H,W,3]); -> their rows of the table, float64 [F,5]"""
        F = 1 if pred.dim() == 3 else pred.shape[0]
        if self.table is None or self.n + F > self.table.shape[0]:
            cap = max(self.capacity, 1) if self.table is None else self.table.shape[0]
            while cap < self.n + F:
                cap *= 2
            table = torch.empty(cap, 5, dtype=torch.float64, device=pred.device)
            if self.table is not None:
                table[:self.n] = self.table[:self.n]
            self.table = table
        rows = self.table[self.n:self.n + F]
        if pred.is_cuda:
            frame_metrics(pred, gt, self.gray, out=rows)
        else:
            rows.copy_(frame_metrics(pred, gt, self.gray))
        self.n += F
        return rows

    def psnr(self, pred, gt):
        """mse_to_psnr(((pred - gt) ** 2).mean()) of one frame as a scalar on its device (eval.py:152 without the float()); adds nothing"""
        return frame_metrics(pred, gt, self.gray)[0, _PSNR_F]

    def result(self):
        """one host read -> {'psnr', 'psnr_u8', 'ssim'}: means over the frames of the per-frame values (eval.py:170's
        np.array(PSNR).mean(), not the PSNR of the mean MSE; one frame with psnr_u8 = inf makes that mean inf), and 'frames': the
        table, float64 [n,5] in the order of ops.FRAME_METRIC_NAMES"""
        ops._require(self.n > 0, "no frame added")
        frames = self.table[:self.n].cpu().numpy()
        col = lambda name: float(frames[:, ops.FRAME_METRIC_NAMES.index(name)].mean())
        return {"psnr": col("psnr_f"), "psnr_u8": col("psnr_u8"), "ssim": col("ssim"), "frames": frames}
