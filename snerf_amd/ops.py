"""Thin torch-tensor -> C-ABI wrappers (device pointers, strides, current HIP stream).

PyTorch is plumbing here: it owns device memory and the stream.  Every
function launches hand-written HIP kernels from libsnerf_hip.so through
``_lib.call``; nothing in this file computes on the host or falls back to
torch ops.
"""
import ctypes
import os as _os

import torch

from . import _lib

F32, BF16, F16, F64 = 0, 1, 2, 3
BF16X3 = 4                                 # GEMMs only: split-bf16 operands, the fp32-parity mode at bf16 MFMA rates (csrc/gemm.hip, GemmNT::split)
F16F8 = 5                                  # snerf_linear_fwd only: fp16 + fp8 split operands, the same contract in two pass-equivalents (GemmNT::split == 2)
SPLIT_DTS = (BF16X3, F16F8)                # activation buffers hold 2 physical 2-byte columns per logical column
ACT_NONE, ACT_RELU, ACT_MASK = 0, 1, 2
ACT_RELU_BITS, ACT_MASK_BITS = 3, 4        # ReLU that also writes a 1-bit-per-element mask / ReLU backward from that mask
_TORCH_DT = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16, BF16X3: torch.bfloat16, F16F8: torch.float16}


def torch_dtype(dt: int):
    return _TORCH_DT[dt]


def gran(dt: int) -> int:
    """reduction-axis granularity of the GEMM tiles: 128-byte LDS rows."""
    return 32 if dt == F32 else 64                    # (BF16X3: 64 LOGICAL columns = one 128-column physical group)


def roundup(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


# ---- argument checks: everything a caller hands in is checked here, before its data_ptr() reaches a launch.  They raise
# _lib.SnerfArgumentError (a ValueError) and survive `python -O`; a message is only built when a check fails.
_DT_NAME = {torch.float32: "fp32", torch.float64: "fp64", torch.bfloat16: "bf16", torch.float16: "fp16", torch.int32: "int32",
            torch.int64: "int64", torch.uint8: "uint8"}


def _require(ok, msg, *fmt):
    """predicate check: `msg` names the argument and the expected form (%-formatted with `fmt` on failure)"""
    if not ok:
        raise _lib.SnerfArgumentError(msg % fmt if fmt else msg)


def _arg(names, i, n):
    """the name of tensor i of n for a message: `names` holds n space-separated names, or one name for all of them"""
    parts = names.split()
    return parts[i] if len(parts) == n else names


def _dev(names, *ts, dtype=torch.float32, shape=None, optional=False, msg=None):
    """device-tensor check: every tensor of `ts` (`names`: their names, space separated, or one name for all) is a contiguous CUDA tensor
    of `dtype` (one dtype or a tuple of them) and, with `shape`, of exactly that shape (None = any extent); `optional`: None passes.
    dtype=None is the weaker class for an argument the wrapper asks no form of (a view passed with its own stride, a buffer only the
    kernel interprets): on the device, nothing else.  -> the first tensor"""
    for i, t in enumerate(ts):
        if t is None:
            if optional:
                continue
        elif dtype is None:
            if t.is_cuda:
                continue
        elif t.is_cuda and t.is_contiguous() and (t.dtype == dtype or (type(dtype) is tuple and t.dtype in dtype)) and (
                shape is None or (len(t.shape) == len(shape) and all(s is None or s == n for s, n in zip(shape, t.shape)))):
            continue
        if msg is None:
            dts = "" if dtype is None else "contiguous " + " / ".join(_DT_NAME.get(d, str(d)) for d in (dtype if type(dtype) is tuple else (dtype,))) + " "
            form = "" if shape is None else " of shape [" + ",".join("*" if s is None else str(s) for s in shape) + "]"
            msg = f"{_arg(names, i, len(ts))}: expected a {dts}CUDA tensor{form}"
        raise _lib.SnerfArgumentError(msg)
    return ts[0]


def _chk2d(names, *ts, dt=None):
    """row-major 2-D CUDA views (unit column stride, any row stride) of dtype `dt` (None: any) -> the first one"""
    for i, t in enumerate(ts):
        if not (t.is_cuda and t.dim() == 2 and t.stride(1) == 1):
            raise _lib.SnerfArgumentError(f"{_arg(names, i, len(ts))}: expected a row-major 2-D CUDA view")
        if dt is not None and t.dtype != dt:
            raise _lib.SnerfArgumentError(f"{_arg(names, i, len(ts))}: dtype {t.dtype} != {dt}")
    return ts[0]


def _ws_given(ws, dtype, msg, min_bytes=0):
    """a workspace the caller brings: a contiguous CUDA tensor of `dtype` (None: of any) holding >= `min_bytes` bytes -- given where the
    wrapper owns that check; elsewhere the library refuses a short buffer"""
    if ws is None or not (ws.is_cuda and ws.is_contiguous() and (dtype is None or ws.dtype == dtype) and ws.numel() * ws.element_size() >= min_bytes):
        raise _lib.SnerfArgumentError(msg)
    return ws


def _ws(ws, numel, dtype, device, msg, min_bytes=0):
    """an optional workspace: None -> a fresh `dtype` buffer of `numel` elements on `device` (`numel` may be a callable: the size
    queries are library calls, made only when the buffer is allocated); given -> _ws_given"""
    if ws is None:
        return torch.empty(numel() if callable(numel) else numel, dtype=dtype, device=device)
    return _ws_given(ws, dtype, msg, min_bytes)


_zeros_cache = {}


def lds_scribble(seed):
    """test utility: fill every CU's LDS with a seeded pattern (tests/test_stale_lds.py)"""
    _lib.call("snerf_debug_lds_scribble", int(seed), _stream())


def zero_page(device):
    z = _zeros_cache.get(device)
    if z is None:
        z = torch.zeros(64, dtype=torch.float32, device=device)
        _zeros_cache[device] = z
    return z


# ------------------------------------------------------------------ GEMMs ----
def linear_fwd(A, W, bias, Y, K, n_store, act, dt, out_f32=False, aux=None, colsum=None, variant=0, deterministic=False, aux_split=False):
    """Y[:, :n_store] = act(A[:, :K] @ W[:, :K]^T + bias); A/W/Y are 2-D views (row stride = ld).  `deterministic`: the bias-gradient
    partials (`colsum`) are folded in a fixed order.  `aux_split` (plain bf16 launch, ACT_MASK): the mask source is an activation a
    split-bf16 forward saved (interleaved hi / lo; its hi half is tested).
    The persistent kernel's plain bf16 launches with K >= 192 have two MFMA flavours (16 x 16 x 32: the default; 32 x 32 x 16: everything else);
    the library reads SNERF_NT_MFMA = 16 | 32 at every launch (A/B runs, tests) and runs that flavour where both exist."""
    if deterministic:
        variant |= 256
    if aux_split and act == ACT_MASK:
        _require(dt in (BF16, F16) and aux is not None and aux.shape[1] >= 2 * roundup(n_store, 64) - 64,
                 "aux_split: dt bf16 / fp16 and aux [M, >= 2 roundup(n_store, 64) - 64], the activation a split forward saved")
        variant |= 1 << 14
    tdt = _TORCH_DT[dt]
    # (the checks of this wrapper are inline where they can be: it runs some fifty times per step, and a helper call costs 0.1 - 0.2 us)
    if not (A.is_cuda and A.dim() == 2 and A.stride(1) == 1 and A.dtype == tdt and W.is_cuda and W.dim() == 2 and W.stride(1) == 1 and W.dtype == tdt
            and Y.is_cuda and Y.dim() == 2 and Y.stride(1) == 1 and Y.dtype == (torch.float32 if out_f32 else tdt)):
        _chk2d("A W", A, W, dt=tdt); _chk2d("Y", Y, dt=torch.float32 if out_f32 else tdt)          # (names the one that fails)
    if (bias is not None and not bias.is_cuda) or (colsum is not None and not colsum.is_cuda):
        _dev("bias colsum", bias, colsum, dtype=None, optional=True)
    M = A.shape[0]
    sp = dt in SPLIT_DTS                                  # split-bf16: A [M, 2 K], W [N, 3 K], a bf16 Y [M, 2 n_store] (interleaved layout); fp16 + fp8: W [N, 2 K]
    if not (Y.shape[0] == M and A.shape[1] >= K * (2 if sp else 1) and W.shape[1] >= K * ((3 if dt == BF16X3 else 2) if sp else 1)):
        raise _lib.SnerfArgumentError("A [M, >= K], W [N, >= K], Y [M, ...] (split operands: 2 K / 3 K physical columns)")
    if not (Y.shape[1] >= n_store * (2 if sp and not out_f32 else 1) or (sp and not out_f32 and Y.shape[1] >= 2 * roundup(n_store, 64) - 64)):
        raise _lib.SnerfArgumentError("Y [M, >= n_store] (a split bf16 Y: 2 n_store interleaved columns)")
    if aux is not None and act < ACT_RELU_BITS:
        _chk2d("aux", aux, dt=_TORCH_DT[dt])
    if act >= ACT_RELU_BITS:
        _dev("aux", aux, dtype=torch.int32)
        _require(aux.numel() >= mask_bits_words(M, W.shape[0]), "aux: int32 [>= mask_bits_words(M, N)], the ReLU bit mask")
    ws = None
    if colsum is not None:  # partial column sums (no atomics), one row per row slab or per (workgroup, wave row); folded into `colsum` by a second kernel
        tiles = ((M + 255) // 256) * max(W.shape[0] // 256, 1)
        ws = torch.empty(max(2 * ((M + 127) // 128), 2 * min(tiles, 1024)), W.shape[0], dtype=torch.float32, device=A.device)
    _lib.call("snerf_linear_fwd", _p(A), A.stride(0), _p(W), W.stride(0), _p(bias), _p(Y), Y.stride(0),
              _p(aux), 0 if (aux is None or act >= ACT_RELU_BITS) else aux.stride(0), _p(colsum), _p(ws), M, W.shape[0], K, n_store, act, dt,
              1 if out_f32 else 0, variant, _stream())


def fast_epilogue_ok(Y, n_store, dt, out_f32=False, aux=None, act=ACT_NONE):
    """Whether snerf_linear_fwd takes its LDS-transposed 16-byte epilogue for this launch (mirrors the dispatch in gemm.hip): the only
    epilogue whose bias-gradient column sums can be folded deterministically (the direct-store epilogue adds them with atomics)."""
    epc = 4 if dt == F32 else 8
    ok = not (out_f32 and dt in (BF16, F16)) and Y.stride(0) % epc == 0 and Y.data_ptr() % 16 == 0 and n_store % epc == 0
    if act == ACT_MASK and aux is not None:
        ok = ok and aux.stride(0) % epc == 0 and aux.data_ptr() % 16 == 0
    return ok


def mask_bits_words(M, N):
    """int32 words of the ReLU bit mask of an [M, N] activation (N % 64 == 0): one 64-word block per (32 rows, 64 columns)."""
    return 8 * ((M + 255) // 256) * (N // 64) * 64


def relu_bits_ok(A, W, Y, K, n_store, dt, variant, consumer=False):
    """Whether snerf_linear_fwd accepts ACT_RELU_BITS (producer) / ACT_MASK_BITS (consumer) for this launch: the persistent
    8-phase kernel's conditions (mirrors the dispatch in gemm.hip)."""
    N = W.shape[0]
    return (dt in (BF16, BF16X3, F16, F16F8) and (variant & 8) and N % 256 == 0 and K * (3 if dt == BF16X3 else 1) >= 128 and Y.dtype == _TORCH_DT[dt]
            and not (dt == F16F8 and (consumer or K < 128))
            and Y.stride(0) % 8 == 0 and Y.data_ptr() % 16 == 0 and n_store % 8 == 0
            and A.stride(0) * 512 < (1 << 31) and W.stride(0) * 512 < (1 << 31) and mask_bits_words(A.shape[0], N) * 4 < (1 << 31))


# the environment switch (A/B runs, tools/probes/wgrad_fold_ab.sh): "0" = fp32 atomics everywhere, "wide" = the fold for the wide layers only (round 5's
# policy), anything else = the policy below
WGRAD_FOLD = __import__("os").environ.get("SNERF_WGRAD_FOLD", "1") != "0"
WGRAD_FOLD_WIDE_ONLY = __import__("os").environ.get("SNERF_WGRAD_FOLD", "1") == "wide"
WGRAD_FOLD_SMALL_M = __import__("os").environ.get("SNERF_WGRAD_FOLD_SMALL_M", "1") != "0"      # (A/B switch of the small-M rule below)


def wgrad_uses_fold(M, N, K, dt, variant, n_valid=None, k_valid=None):
    """the default cross-slice reduction of linear_wgrad: True = partial tiles + fixed-order fold (see there), False = fp32 atomics.
    A launch runs ~256 (256 x 256 kernel) or ~1024 (128 x 128 kernel) workgroups whatever M is, and every one of them ends with one fp32 atomic per
    valid element of its tile: 16.8 M atomics per launch on full tiles, all issued at the same moment -- 25-70 us per launch that the partial tiles +
    fold replace by 10-25.  So: the wide layers (>= 8 tiles of the 256 x 256 kernel: any M, round 5) and, up to 2^20 rows, its few-tile launches and
    the 128 x 128 kernel's launches with up to four output tiles of >= 8 valid rows (more tiles -- N = 128, K = 1051; N = 1024, K = 96 -- stream
    enough operand bytes per atomic to hide them: measured neutral; a head's 1-3 valid rows issue few atomics).  Beyond 2^20 rows a workgroup's slice
    is long enough for the bursts to drift apart: path C's 2.1 M-row launches are neutral, path B's 8.4 M-row launches LOSE 0.4 ms per step to the
    partial tiles + folds (alternating A/B).  profiles/r6_z_wgrad_fold_narrow_ab.txt"""
    if not WGRAD_FOLD or dt not in (BF16, F16) or M < 4096:
        return False
    few_ok = not WGRAD_FOLD_WIDE_ONLY and M <= (1 << 20)
    if (variant & 2) and N % 256 == 0 and K >= 256:                   # tn_plan's condition for the 256 x 256 kernel
        return (N // 256) * ((K + 255) // 256) >= 8 or few_ok
    if not few_ok:
        return False
    nv = N if n_valid is None else n_valid
    tiles = ((N + 127) // 128) * ((K + 127) // 128)
    # (small M: the 16.8 M atomics are most of a many-tile launch too -- N = 128, K = 1051 and N = 1024, K = 96 of the 512-ray step)
    return nv >= 8 and (tiles <= 4 or (WGRAD_FOLD_SMALL_M and M <= 131072 and tiles <= 16))


def linear_wgrad(dZ, X, dW, n_valid, k_valid, dt, variant=0, deterministic=False, x_split_hi=False):
    """dW[:n_valid, :k_valid] += dZ^T @ X.  dZ [M,N], X [M,K] views, dW fp32 view.  The M slices of a launch either add with fp32 atomics (order varies
    run to run) or store partial tiles into a workspace that a second launch folds in slice order (bit-reproducible): `deterministic`
    forces the fold; it is also the default for the wide layers (below).  `x_split_hi` (dt bf16): X is an activation a split-bf16 forward
    saved ([M, 2 K] interleaved hi / lo) and its hi half is multiplied.
    The 256 x 256 kernel has two MFMA flavours (16 x 16 x 32: the bf16 default; 32 x 32 x 16: fp16, split-bf16).  The library reads two environment
    variables at every launch (A/B runs, tests): SNERF_WGRAD_MFMA = 16 | 32 runs that flavour where the 256 x 256 kernel is launched anyway;
    SNERF_WGRAD_TN8 = 1 launches the 256 x 256 kernel wherever it can run, whatever the rules on M say."""
    _chk2d("dZ X", dZ, X, dt=_TORCH_DT[dt]); _chk2d("dW", dW, dt=torch.float32)
    _require(dZ.shape[0] == X.shape[0] and dW.shape[0] >= n_valid and dW.shape[1] >= k_valid, "dZ [M,N], X [M,K], dW [>= n_valid, >= k_valid]")
    Kx = X.shape[1]
    if x_split_hi:
        _require(dt in (BF16, F16) and Kx % 128 == 0, "x_split_hi: dt bf16 / fp16 and X [M, 2 K] with 2 K % 128 == 0")
        Kx //= 2
        variant |= 1 << 14
    if dt == BF16X3:
        # dZ / X are the interleaved split operands (physical widths, multiples of 128); the kernels fold the hi / lo combinations
        _require(not deterministic, "the split-bf16 weight gradient has no deterministic fold")
        _require(dZ.shape[1] % 128 == 0 and X.shape[1] % 128 == 0, "dZ, X: split-bf16 operands of physical widths % 128 == 0")
    # wide layers on the 256 x 256 kernel (>= 8 output tiles, i.e. <= 32 M slices): the slices store their partial tiles and a second
    # launch folds them in slice order instead of adding 256 x 256 fp32 atomics per slice -- bit-reproducible, and faster: the atomics
    # of 16 slices (16.8 M per launch at N = K = 1024, whatever M is) cost 24-71 us, the stores + fold 7-26 (tools/probes/
    # tn_epilogue_probe.py); 512-ray step 4.55 -> 4.24 ms, 4096-ray step 25.65 -> 25.47 (A/B on one box, tools/probes/wgrad_fold_ab.sh)
    if not deterministic and wgrad_uses_fold(dZ.shape[0], dZ.shape[1], Kx, dt, variant, n_valid, k_valid):
        deterministic = True
    if deterministic:
        nws = _lib.query("snerf_linear_wgrad_ws_floats", dZ.shape[0], dZ.shape[1], Kx, dZ.stride(0), X.stride(0), dt, variant)
        ws = torch.empty(max(int(nws), 1), dtype=torch.float32, device=dZ.device)
        _lib.call("snerf_linear_wgrad_det", _p(dZ), dZ.stride(0), _p(X), X.stride(0), _p(dW), dW.stride(0), _p(zero_page(dZ.device)),
                  dZ.shape[0], dZ.shape[1], Kx, n_valid, k_valid, dt, variant, _p(ws), ws.numel(), _stream())
        return
    _lib.call("snerf_linear_wgrad", _p(dZ), dZ.stride(0), _p(X), X.stride(0), _p(dW), dW.stride(0),
              _p(zero_page(dZ.device)), dZ.shape[0], dZ.shape[1], Kx, n_valid, k_valid, dt, variant, _stream())


# ------------------------------------------------------------ fused MLPs ----
def _fmlp_dt(stream):
    """the 16-bit flavour of a fused 256-wide launch = the dtype of its packed weight stream (bf16 or fp16); operand rows, stored activations,
    xin copies and dz must carry the same one"""
    _dev("stream", stream, dtype=(torch.bfloat16, torch.float16), msg="stream: the fused 256-wide networks run in bf16 or fp16 (contiguous, on the device)")
    return stream.dtype, _zip_dt(stream)


def fmlp_classic_fwd(E, VE, stream, bias, raw):
    """The whole classic NeRF 8 x 256 network in one launch (csrc/fmlp.hip): E [M,>=64] / VE [M,>=32] embeddings in the stream's dtype
    (bf16 or fp16), `stream` / `bias` from mlp.fmlp_pack -> raw [M,4] fp32."""
    tdt, dt = _fmlp_dt(stream)
    _chk2d("E VE", E, VE, dt=tdt); _dev("bias", bias); _dev("raw", raw, shape=(None, 4))
    _require(E.shape[1] >= 64 and VE.shape[1] >= 32 and VE.shape[0] == E.shape[0] == raw.shape[0], "E [M, >= 64], VE [M, >= 32], raw [M, 4]")
    _lib.call("snerf_fmlp_classic_fwd_dt", _p(E), E.stride(0), _p(VE), VE.stride(0), _p(stream), stream.shape[0], _p(bias), bias.numel() // 32,
              _p(raw), E.shape[0], dt, _stream())


def fmlp_classic_pts_fwd(pts, viewdirs, S, stream, bias, raw):
    """fmlp_classic_fwd with the embeddings computed in the kernel: pts [M,3] fp32, viewdirs [M/S,3] fp32 -> raw [M,4] fp32."""
    _dev("pts", pts); _chk2d("viewdirs", viewdirs, dt=torch.float32)
    _, dt = _fmlp_dt(stream)
    _require(viewdirs.shape[1] == 3 and pts.shape[0] == viewdirs.shape[0] * S, "viewdirs [M / S, 3] for pts [M, 3]")
    _dev("bias", bias); _dev("raw", raw, shape=(pts.shape[0], 4))
    _lib.call("snerf_fmlp_classic_pts_fwd_dt", _p(pts), _p(viewdirs), viewdirs.stride(0), int(S), _p(stream), stream.shape[0], _p(bias),
              bias.numel() // 32, _p(raw), pts.shape[0], dt, _stream())


def _x_rows(x):
    """pre-embedded classic input rows: fp32 [M, >= 90] CUDA view with unit column stride (any row stride)"""
    _require(x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and x.shape[1] >= 90, "x: expected fp32 [M, >= 90] rows")
    _require(x.shape[0] < (1 << 31) and (x.shape[0] <= 1 or x.stride(0) >= 90), "x: fewer than 2^31 rows that do not overlap (row stride >= 90)")
    return x


def fmlp_classic_x_fwd(x, stream, bias, raw):
    """fmlp_classic_fwd on the caller's pre-embedded fp32 rows x [M, >= 90] = [embedded pts (63) | embedded views (27)] (any row
    stride; rounded to the stream's dtype in the kernel as cast_pad rounds) -> raw [M,4] fp32."""
    _x_rows(x)
    _, dt = _fmlp_dt(stream)
    _dev("bias", bias); _dev("raw", raw, shape=(x.shape[0], 4))
    _lib.call("snerf_fmlp_classic_x_fwd_dt", _p(x), max(x.stride(0), 90), _p(stream), stream.shape[0], _p(bias), bias.numel() // 32, _p(raw),
              x.shape[0], dt, _stream())


def _mat_arrays(mats, M, widths, tdt, aligned=False):
    """the HOST arrays (device pointers, row strides in elements) the fused entries take for a list of stored 16-bit matrices: 2-D views
    [M, >= widths[i]] of dtype `tdt` with unit column stride; `aligned`: 16-byte aligned with row strides % 8 == 0 asserted here as well"""
    _require(len(mats) == len(widths), "stored matrices: %d expected", len(widths))
    for y, w in zip(mats, widths):
        _chk2d("mats (the stored 16-bit matrices)", y, dt=tdt)
        _require(y.shape[0] == M and y.shape[1] >= w, "stored matrix: [M, >= %d]", w)
        _require(not aligned or (y.data_ptr() % 16 == 0 and y.stride(0) % 8 == 0), "stored matrix: 16-byte aligned, row stride % 8 == 0")
    return (ctypes.c_void_p * len(mats))(*[y.data_ptr() for y in mats]), (ctypes.c_long * len(mats))(*[y.stride(0) for y in mats])


def _mask_array(bits, M, widths):
    """... and for the ReLU bit masks of M rows of widths[i] columns (contiguous int32, mask_bits_words each)"""
    _require(len(bits) == len(widths), "bits: %d ReLU bit masks expected", len(widths))
    for b, w in zip(bits, widths):
        _dev("bits", b, dtype=torch.int32)
        _require(b.numel() >= mask_bits_words(M, w), "bits: int32 [>= mask_bits_words(M, %d)]", w)
    return (ctypes.c_void_p * len(bits))(*[b.data_ptr() for b in bits])


def _bias_array(g_bias, widths):
    """... and for the fp32 bias gradients (contiguous, exactly widths[i] floats) the gradient chains add to"""
    _require(len(g_bias) == len(widths), "g_bias: %d bias gradients expected", len(widths))
    for gb, w in zip(g_bias, widths):
        _dev("g_bias", gb)
        _require(gb.numel() == w, "g_bias: fp32 [%d]", w)
    return (ctypes.c_void_p * len(g_bias))(*[g.data_ptr() for g in g_bias])


_CLASSIC_WIDTHS = [256] * 9 + [128]                 # pts_linears.0 .. .7, feature_linear, views_linears.0
_CLASSIC_MASKS = [256] * 8 + [128]                  # pts_linears.0 .. .7, views_linears.0


def fmlp_classic_x_train_fwd(x, stream, bias, raw, xin, acts, bits):
    """fmlp_classic_train_fwd on pre-embedded fp32 rows x (as fmlp_classic_x_fwd); additionally writes the rounded inputs into
    `xin` = [E [M, >= 64], skip-buffer head [M, >= 64], view tail [M, >= 32]] (row-major views in the stream's dtype, 16-byte aligned, row
    strides % 8 == 0)."""
    _x_rows(x)
    tdt, dt = _fmlp_dt(stream)
    _dev("bias", bias); _dev("raw", raw, shape=(x.shape[0], 4))
    M = x.shape[0]
    ptrs, lds = _mat_arrays(acts, M, _CLASSIC_WIDTHS, tdt, aligned=True)
    xp, xl = _mat_arrays(xin, M, [64, 64, 32], tdt, aligned=True)
    _lib.call("snerf_fmlp_classic_x_train_fwd_dt", _p(x), max(x.stride(0), 90), _p(stream), stream.shape[0], _p(bias), bias.numel() // 32, _p(raw),
              xp, xl, ptrs, lds, _mask_array(bits, M, _CLASSIC_MASKS), M, dt, _stream())


def fmlp_proposal_fwd(E, stream, bias, raw_density):
    """The proposal MLP 96 -> 4 x 256 -> 1 in one launch: E [M,>=96] IPE rows in the stream's dtype (bf16 or fp16) -> raw density [M,1] fp32."""
    tdt, dt = _fmlp_dt(stream)
    _chk2d("E", E, dt=tdt); _dev("bias raw_density", bias, raw_density)
    _require(E.shape[1] >= 96 and raw_density.numel() == E.shape[0], "E [M, >= 96], raw_density [M, 1]")
    _lib.call("snerf_fmlp_proposal_fwd_dt", _p(E), E.stride(0), _p(stream), stream.shape[0], _p(bias), bias.numel() // 32, _p(raw_density),
              E.shape[0], dt, _stream())


def fmlp_classic_train_fwd(E, VE, stream, bias, raw, acts, bits):
    """fmlp_classic_fwd that also stores the ten hidden-layer outputs (`acts`: pts_linears.0..7 [M,256], feature [M,256], views
    [M,128], row-major views in the stream's dtype) and the ReLU bit masks of the eight trunk layers (`bits[0..7]`: int32 [mask_bits_words(M, 256)]
    each) and of views_linears.0 (`bits[8]`: [mask_bits_words(M, 128)]) for the backward pass."""
    tdt, dt = _fmlp_dt(stream)
    _chk2d("E VE", E, VE, dt=tdt); _dev("bias", bias); _dev("raw", raw, shape=(None, 4))
    M = E.shape[0]
    _require(E.shape[1] >= 64 and VE.shape[1] >= 32 and VE.shape[0] == M == raw.shape[0], "E [M, >= 64], VE [M, >= 32], raw [M, 4]")
    ptrs, lds = _mat_arrays(acts, M, _CLASSIC_WIDTHS, tdt, aligned=True)
    _lib.call("snerf_fmlp_classic_train_fwd_dt", _p(E), E.stride(0), _p(VE), VE.stride(0), _p(stream), stream.shape[0], _p(bias),
              bias.numel() // 32, _p(raw), ptrs, lds, _mask_array(bits, M, _CLASSIC_MASKS), M, dt, _stream())


def fmlp_proposal_train_fwd(E, stream, bias, raw_density, acts, bits):
    """fmlp_proposal_fwd that also stores the four hidden-layer outputs (`acts`: [M,256] each, the stream's dtype) and their ReLU bit masks."""
    tdt, dt = _fmlp_dt(stream)
    _chk2d("E", E, dt=tdt); _dev("bias raw_density", bias, raw_density)
    M = E.shape[0]
    _require(E.shape[1] >= 96 and raw_density.numel() == M, "E [M, >= 96], raw_density [M, 1]")
    ptrs, lds = _mat_arrays(acts, M, [256] * 4, tdt, aligned=True)
    _lib.call("snerf_fmlp_proposal_train_fwd_dt", _p(E), E.stride(0), _p(stream), stream.shape[0], _p(bias), bias.numel() // 32,
              _p(raw_density), ptrs, lds, _mask_array(bits, M, [256] * 4), M, dt, _stream())


def fmlp_zip_fwd(Fb, D, stream, bias, raw_rgb, raw_d, x32=None):
    """NeRF MLP of the zipnerf path at inference in ONE launch (csrc/fmlp.hip, fzip_fwd_kernel): Fb [M, >= 64] grid features, D [M, >= 16]
    direction encoding (bf16 or fp16 = the stream's dtype, zero padded) -> raw_rgb [M, 3], raw_d [M, 1] fp32; x32 (optional [M, >= 32],
    compute dtype): the first 32 channels of the bottleneck x (the semantic logits are x[:, 1:1+C])."""
    _chk2d("Fb D", Fb, D, dt=Fb.dtype); _chk2d("raw_rgb raw_d", raw_rgb, raw_d, dt=torch.float32)
    M = Fb.shape[0]
    _require(Fb.dtype in (torch.bfloat16, torch.float16), "Fb: bf16 or fp16")
    _dev("stream", stream, dtype=Fb.dtype); _dev("bias", bias)
    _require(D.shape[0] == M and raw_rgb.shape[0] == M and raw_d.shape[0] == M and Fb.shape[1] >= 64 and D.shape[1] >= 16 and raw_rgb.shape[1] >= 3,
             "Fb [M, >= 64], D [M, >= 16], raw_rgb [M, >= 3], raw_d [M, 1]")
    if x32 is not None:
        _chk2d("x32", x32, dt=Fb.dtype)
        _require(x32.shape[0] == M and x32.shape[1] >= 32, "x32 [M, >= 32]")
    _lib.call("snerf_fmlp_zip_fwd", _p(Fb), Fb.stride(0), _p(D), D.stride(0), _p(stream), stream.shape[0], _p(bias), bias.numel() // 32,
              _p(raw_rgb), raw_rgb.stride(0), _p(raw_d), raw_d.stride(0), _p(x32), 0 if x32 is None else x32.stride(0), M, _zip_dt(Fb), _stream())


def fmlp_zip_train_fwd(Fb, D, stream, bias, raw_rgb, raw_d, acts, bits):
    """The training forward of the zipnerf NeRF MLP in ONE launch (fzip_fwd_kernel<.., STORE>): as fmlp_zip_fwd, plus acts = [H1 [M, >= 64],
    x, h, H3 [M, >= 256]] (compute dtype 2-D views, written) and bits = 3 x int32: the ReLU bit masks of H1 [mask_bits_words(M, 64)], h and H3
    [mask_bits_words(M, 256)]."""
    _chk2d("Fb D", Fb, D, dt=Fb.dtype); _chk2d("raw_rgb raw_d", raw_rgb, raw_d, dt=torch.float32)
    M = Fb.shape[0]
    _require(Fb.dtype in (torch.bfloat16, torch.float16), "Fb: bf16 or fp16")
    _dev("stream", stream, dtype=Fb.dtype); _dev("bias", bias)
    _require(D.shape[0] == M and raw_rgb.shape[0] == M and raw_d.shape[0] == M and Fb.shape[1] >= 64 and D.shape[1] >= 16,
             "Fb [M, >= 64], D [M, >= 16], raw_rgb [M, >= 3], raw_d [M, 1]")
    pa, pl = _mat_arrays(acts, M, [64, 256, 256, 256], Fb.dtype)
    _lib.call("snerf_fmlp_zip_train_fwd", _p(Fb), Fb.stride(0), _p(D), D.stride(0), _p(stream), stream.shape[0], _p(bias), bias.numel() // 32,
              _p(raw_rgb), raw_rgb.stride(0), _p(raw_d), raw_d.stride(0), pa, pl, _mask_array(bits, M, [64, 256, 256]), M, _zip_dt(Fb), _stream())


def fmlp_zip_chain_bwd(d_rgb, d_den, stream, bits, dz, g_bias):
    """Data-gradient chain of the zipnerf NeRF MLP in ONE launch (fzip_chain_bwd_kernel): d_rgb [M,3], d_den [M, 1 + C <= 32] fp32 -> dz = [dH3, dh,
    dx ([M, >= 256]), dH1, dF ([M, >= 64])] (compute dtype views, written); bits = the forward's masks of H1, h, H3; the bias gradients of
    lin_second_stage_1 / _0, density_layer.2 / .0 are added to g_bias[0..3] (not bit-reproducible)."""
    _chk2d("d_rgb d_den", d_rgb, d_den, dt=torch.float32)
    M = d_rgb.shape[0]
    _require(d_den.shape[0] == M and 1 <= d_den.shape[1] <= 32, "d_den [M, 1 + C <= 32]")
    _fmlp_dt(stream)
    pb = _mask_array(bits, M, [64, 256, 256])
    pz, pl = _mat_arrays(dz, M, [256, 256, 256, 64, 64], stream.dtype)
    pg = _bias_array(g_bias, [256, 256, 256, 64])
    nws = _lib.query("snerf_fmlp_zip_chain_ws_floats", M)
    ws = torch.empty(max(int(nws), 1), dtype=torch.float32, device=d_rgb.device)
    _lib.call("snerf_fmlp_zip_chain_bwd", _p(d_rgb), d_rgb.stride(0), _p(d_den), d_den.stride(0), d_den.shape[1], _p(stream), stream.shape[0],
              pb, pz, pl, pg, _p(ws), ws.numel(), M, _zip_dt(stream), _stream())


def fcolour_fwd(CB, stream, bias, raw_rgb, acts=None, bits=None, variant=0):
    """Fused colour head of the mip path's NeRF MLP (csrc/fmlp.hip): CB [M, >= 1056] = [bottleneck 1024 | view encoding 27 | 0] in the
    stream's dtype (bf16 or fp16) -> raw_rgb [M,3] fp32 in ONE launch.  Training: `acts` = 3 x [M, >= 128] in the same dtype (outputs of
    cond_layers.0..2), `bits` = 3 x int32 [mask_bits_words(M, 128)] (their ReLU bit masks), stored for fcolour_bwd and the weight-gradient GEMMs."""
    tdt, dt = _fmlp_dt(stream)
    _chk2d("CB", CB, dt=tdt)
    M = CB.shape[0]
    _require(CB.shape[1] >= 1056, "CB [M, >= 1056]")
    _dev("bias", bias); _dev("raw_rgb", raw_rgb, shape=(M, 3))
    pa = pl = pb = None
    if acts is not None:
        pa, pl = _mat_arrays(acts, M, [128] * 3, tdt)
        pb = _mask_array(bits, M, [128] * 3)
    _lib.call("snerf_fcolour_fwd_dt", _p(CB), CB.stride(0), _p(stream), stream.shape[0], _p(bias), bias.numel() // 32, _p(raw_rgb),
              pa, pl, pb, M, int(variant), dt, _stream())


def fcolour_bwd(d_raw_rgb, stream, bits, dC, dB, g_bias):
    """Fused data-gradient chain of the colour head: d_raw_rgb [M,3] fp32 -> dC = [dC2, dC1, dC0] ([M, >= 128] each) and dB
    ([M, >= 1024] view), all in the stream's dtype (bf16 or fp16; in fp16 d_raw_rgb arrives already multiplied by the loss scale);
    bits = ReLU bit masks of [cond_layers.2, .1, .0, bottleneck]; the bias gradients are added to g_bias = [cond_layers.2, .1, .0,
    bottleneck] (fp32 views of the gradient arena) in a fixed order."""
    tdt, dt = _fmlp_dt(stream)
    _dev("d_raw_rgb", d_raw_rgb, shape=(None, 3)); _chk2d("dB", dB, dt=tdt)
    M = d_raw_rgb.shape[0]
    _require(dB.shape[0] == M and dB.shape[1] >= 1024, "dB [M, >= 1024]")
    pb = _mask_array(bits, M, [128, 128, 128, 1024])
    pc, pl = _mat_arrays(dC, M, [128] * 3, tdt)
    pg = _bias_array(g_bias, [128, 128, 128, 1024])
    nws = _lib.query("snerf_fcolour_bwd_ws_floats", M)
    ws = torch.empty(max(int(nws), 1), dtype=torch.float32, device=dB.device)
    _lib.call("snerf_fcolour_bwd_dt", _p(d_raw_rgb), _p(stream), stream.shape[0], pb, pc, pl, _p(dB), dB.stride(0), pg, _p(ws), ws.numel(), M, dt,
              _stream())


CHAIN_CLASSIC, CHAIN_PROPOSAL = 0, 1


def fchain_bwd(net, d_raw, stream, bits, dz, g_bias):
    """Fused data-gradient chain of a 256-wide network (csrc/fmlp.hip fchain_bwd_kernel), ONE launch instead of one GEMM per layer.
    CHAIN_CLASSIC: d_raw [M,4] fp32 -> dz = [d views_linears.0 (128), d feature_linear (256), d pts_linears.7 .. .0 (256)]; bits =
    masks of pts_linears.0..7 + views_linears.0.  CHAIN_PROPOSAL: d_raw [M] / [M,1] (d raw density) -> dz = [d layers.3 .. .0]; bits =
    masks of layers.0..3.  The bias gradient of step i is added to g_bias[i] (not bit-reproducible: workgroup-level LDS atomics).
    `stream` and every dz carry one 16-bit dtype, bf16 or fp16; in fp16 d_raw arrives already multiplied by the loss scale."""
    classic = net == CHAIN_CLASSIC
    _dev("d_raw", d_raw)
    M = d_raw.shape[0]
    widths = ([128] + [256] * 9) if classic else [256] * 4
    tdt, dt = _fmlp_dt(stream)
    _require(d_raw.numel() == M * (4 if classic else 1), "d_raw: [M, 4] (classic) or [M] / [M, 1] (proposal)")
    pb = _mask_array(bits, M, _CLASSIC_MASKS if classic else [256] * 4)
    pz, pl = _mat_arrays(dz, M, widths, tdt)
    pg = _bias_array(g_bias, widths)
    nws = _lib.query("snerf_fchain_bwd_ws_floats", net, M)
    ws = torch.empty(max(int(nws), 1), dtype=torch.float32, device=d_raw.device)
    _lib.call("snerf_fchain_bwd_dt", net, _p(d_raw), _p(stream), stream.shape[0], pb, pz, pl, pg, _p(ws), ws.numel(), M, dt, _stream())


# --------------------------------------------------------------- encoders ----
def classic_embed(pts, viewdirs, S, L, Lv, dst1, dst2, w_pts, dstv, w_views, dt):
    _dev("pts", pts); M = pts.shape[0]
    _require(pts.shape[1] == 3, "pts [M,3] fp32")
    if dt in SPLIT_DTS:
        # the exact fp32 embeddings, then the hi / lo (fp16 + fp8) split into each destination's GEMM operand layout
        t1 = torch.empty(M, w_pts, dtype=torch.float32, device=pts.device)
        tv = None if viewdirs is None else torch.empty(M, w_views, dtype=torch.float32, device=pts.device)
        classic_embed(pts, viewdirs, S, L, Lv, t1, None, w_pts, tv, w_views, F32)
        cast_pad(t1, w_pts, dst1, w_pts, dt)
        if dst2 is not None:
            cast_pad(t1, w_pts, dst2, w_pts, dt)
        if tv is not None:
            cast_pad(tv, w_views, dstv, w_views, dt)
        return
    if viewdirs is not None:
        _chk2d("viewdirs", viewdirs, dt=torch.float32)
        _require(viewdirs.shape[1] == 3 and M == viewdirs.shape[0] * S, "viewdirs [M / S, 3] for pts [M, 3]")
    _lib.call("snerf_classic_embed", _p(pts), _p(viewdirs), 0 if viewdirs is None else viewdirs.stride(0), S, M, L, Lv,
              _p(dst1), dst1.stride(0), _p(dst2), 0 if dst2 is None else dst2.stride(0), w_pts,
              _p(dstv), 0 if dstv is None else dstv.stride(0), w_views, dt, _stream())


def _ids(sample_id):
    if sample_id is None:
        return None, 0
    return _dev("sample_id", sample_id, dtype=torch.int32), sample_id.shape[0]


def mip_encode(s_vals, origins, directions, radii, near, far, cone, transform_idx, max_deg, dst1, dst2, width, dt,
               means_out=None, covs_out=None, sample_id=None, warp=None):
    """cone: ray shape (True / 1 = cone, False / 0 = cylinder); + 2 = --disable_integration (models.py:132-133: the covariances are replaced
    by zeros before the encoding).  sample_id (int32 [rows], optional): encode only the samples ray * S + i listed there, row j of dst <- sample_id[j].
    warp: None = the contraction (model argument fn = 1), or (viewc [3] host floats, far_max device scalar) = the view-centred warp
    fn = 0 (mip.py:367-378)."""
    n, P = s_vals.shape
    _dev("s_vals origins directions radii near far", s_vals, origins, directions, radii, near, far)
    _dev("means_out covs_out", means_out, covs_out, optional=True)
    ids, rows = _ids(sample_id)
    if dt in SPLIT_DTS:
        # the exact fp32 encoding, then the hi / lo split into the GEMM operand layout
        _require(dst2 is None, "dst2: a split dtype encodes into dst1 alone")
        tmp = torch.empty(dst1.shape[0], width, dtype=torch.float32, device=dst1.device)
        mip_encode(s_vals, origins, directions, radii, near, far, cone, transform_idx, max_deg, tmp, None, width, F32, means_out, covs_out, sample_id, warp)
        return cast_pad(tmp, width, dst1, width, dt)
    if warp is not None:
        (vx, vy, vz), far_max = warp
        _dev("far_max", far_max)
        _require(far_max.numel() == 1 and far_max.device == s_vals.device, "far_max: one fp32 element on the rays' device")
        return _lib.call("snerf_mip_encode_warp", _p(s_vals), _p(origins), _p(directions), _p(radii), _p(near), _p(far), n, P - 1,
                         int(cone), transform_idx, max_deg, _p(dst1), dst1.stride(0), _p(dst2),
                         0 if dst2 is None else dst2.stride(0), width, _p(means_out), _p(covs_out), dt, _p(ids), rows,
                         0, float(vx), float(vy), float(vz), _p(far_max), _stream())
    _lib.call("snerf_mip_encode", _p(s_vals), _p(origins), _p(directions), _p(radii), _p(near), _p(far), n, P - 1,
              int(cone), transform_idx, max_deg, _p(dst1), dst1.stride(0), _p(dst2),
              0 if dst2 is None else dst2.stride(0), width, _p(means_out), _p(covs_out), dt, _p(ids), rows, _stream())


def mip_viewenc(viewdirs, S, deg, dst, width, dt, sample_id=None):
    _dev("viewdirs", viewdirs)
    ids, rows = _ids(sample_id)
    if dt in SPLIT_DTS:
        tmp = torch.empty(dst.shape[0], width, dtype=torch.float32, device=dst.device)
        mip_viewenc(viewdirs, S, deg, tmp, width, F32, sample_id)
        return cast_pad(tmp, width, dst, width, dt)
    _lib.call("snerf_mip_viewenc", _p(viewdirs), viewdirs.shape[0], S, deg, _p(dst), dst.stride(0), width, dt, _p(ids), rows, _stream())


class _IndexCheckSlots:
    """Per-device ring of range-check slots: one int32 device counter, one pinned host mirror and one event per slot, all allocated
    once.  A check zeroes its counter, runs snerf_index_check, copies the counter into the pinned mirror (non_blocking) and records the
    event behind the copy; a poll reads the HOST value of slots whose event has completed -- no device synchronisation, no
    allocation per call (`cnt.item()` was a memcpy + stream sync behind the step's queued kernels)."""
    SLOTS = 16

    def __init__(self, device):
        self.dev = torch.zeros(self.SLOTS, dtype=torch.int32, device=device)
        self.host = torch.zeros(self.SLOTS, dtype=torch.int32).pin_memory()
        self.events = [torch.cuda.Event() for _ in range(self.SLOTS)]
        self.msgs = [None] * self.SLOTS            # None = free
        self.head = 0

    def poll(self, block=False):
        for k in range(self.SLOTS):
            if self.msgs[k] is None:
                continue
            if block:
                self.events[k].synchronize()
            elif not self.events[k].query():
                continue
            msg, self.msgs[k] = self.msgs[k], None
            if int(self.host[k]) != 0:
                raise IndexError(msg)

    def acquire(self):
        for _ in range(self.SLOTS):
            k, self.head = self.head, (self.head + 1) % self.SLOTS
            if self.msgs[k] is None:
                return k
        k = self.head                                # every slot pending (16 checks in flight): wait for the oldest one
        self.events[k].synchronize()
        self.poll()
        return self.acquire()


_index_slots = {}            # device index -> _IndexCheckSlots


def poll_index_checks(block=False):
    """Raise IndexError for an embedding index outside its table seen by an EARLIER launch (torch.nn.Embedding raises on one; the
    kernels clamp).  Without `block` only checks whose result has already arrived in pinned host memory are read: the step never waits
    for the check and never synchronises the device."""
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        return
    for slots in _index_slots.values():
        slots.poll(block)


def index_check(idx, n_rows, what):
    """asynchronous range check of a float index vector against a table of n_rows rows; reported by a later poll_index_checks()"""
    poll_index_checks()
    if torch.cuda.is_current_stream_capturing():
        return                                           # (a captured step replays with fresh data nobody checks: validate before capturing)
    di = idx.device.index if idx.device.index is not None else torch.cuda.current_device()
    slots = _index_slots.get(di)
    if slots is None:
        slots = _index_slots[di] = _IndexCheckSlots(idx.device)
    k = slots.acquire()
    cnt = slots.dev[k:k + 1]
    cnt.zero_()
    _lib.call("snerf_index_check", _p(idx), idx.numel(), int(n_rows), _p(cnt), _stream())
    slots.host[k:k + 1].copy_(cnt, non_blocking=True)
    slots.events[k].record()
    slots.msgs[k] = f"{what}: index out of range for a table of {n_rows} rows (torch.nn.Embedding raises here; the kernel clamped)"


def app_embed(emb, app, S, dst, dt, sample_id=None, check=True):
    """appearance embedding rows into the condition block: dst[ray * S + i, :dim] = emb[int(app[ray])] (models.py:153-159).  `check`:
    indices outside the table are reported (IndexError, as nn.Embedding would) by a later call of this module -- see index_check."""
    _dev("emb app", emb, app)
    if check:
        index_check(app, emb.shape[0], "embedding lookup")
    ids, rows = _ids(sample_id)
    _lib.call("snerf_app_embed", _p(emb), _p(app), emb.shape[0], app.numel(), int(S), emb.shape[1], _p(dst), dst.stride(0), dt, _p(ids), rows, _stream())


def app_embed_bwd(dV, app, S, g_emb, deterministic=False):
    """g_emb[int(app[ray])] += sum over the ray's S samples of dV[ray * S + i, :dim] (fp32); `deterministic`: in a fixed order (no atomics)"""
    _chk2d("dV", dV, dt=torch.float32); _dev("app g_emb", app, g_emb)
    _require(dV.shape[0] == app.numel() * S and dV.shape[1] >= g_emb.shape[1], "dV [rays * S, >= dim] for app [rays], g_emb [rows, dim]")
    _lib.call("snerf_app_embed_bwd_det" if deterministic else "snerf_app_embed_bwd", _p(dV), dV.stride(0), _p(app), g_emb.shape[0], app.numel(), int(S),
              g_emb.shape[1], _p(g_emb), _stream())


def ert_compact(s0, w0, s1, eps_t, eps_w):
    """Early ray termination + sample compaction from the proposal histogram (inference): -> (row_index int32 [N,S1] with -1 for
    skipped samples, sample_id int32 [rows] of the kept samples in ray-major order).  One device->host sync for the row count."""
    _dev("s0 w0 s1", s0, w0, s1)
    n, S0, S1 = s0.shape[0], s0.shape[1] - 1, s1.shape[1] - 1
    dev = s0.device
    masks = torch.empty(n, (S1 + 63) // 64, dtype=torch.int64, device=dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    row_index = torch.empty(n, S1, dtype=torch.int32, device=dev)
    sample_id = torch.empty(n * S1, dtype=torch.int32, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    _lib.call("snerf_ert_compact", _p(s0), _p(w0), _p(s1), n, S0, S1, float(eps_t), float(eps_w), _p(masks), _p(counts), _p(row_index),
              _p(sample_id), _p(total), _stream())
    return row_index, sample_id[:int(total.item())]


# --------------------------------------------------------------- samplers ----
def _u_arg(u, n, nf):
    _dev("u", u)
    if u.dim() == 1:
        _require(u.shape[0] == nf, "u: fp32 [nf] (shared by the rays) or [n, nf]")
        return u, 0
    _require(u.shape == (n, nf), "u: fp32 [nf] (shared by the rays) or [n, nf]")
    return u, nf


def classic_sample_pdf(bins, weights, u, mid_mode, want_inds=False, want_std=False):
    """mid_mode True: bins = z_vals [N,S], weights [N,S] (the kernel uses mids and weights[:,1:-1]);
    mid_mode False: bins [N,nb], weights [N,nb-1]."""
    _dev("bins weights", bins, weights)
    n = bins.shape[0]
    if mid_mode:
        _require(weights.shape == bins.shape, "mid_mode: weights [N,S] like bins")
        nc, wptr = bins.shape[1] - 1, weights.data_ptr() + 4
    else:
        _require(weights.shape[1] == bins.shape[1] - 1, "weights [N, nb - 1] for bins [N, nb]")
        nc, wptr = bins.shape[1], weights.data_ptr()
    nf = u.shape[-1]
    u, us = _u_arg(u, n, nf)
    dev = bins.device
    out = torch.empty(n, nf, dtype=torch.float32, device=dev)
    inds = torch.empty(n, nf, dtype=torch.int32, device=dev) if want_inds else None
    std = torch.empty(n, dtype=torch.float32, device=dev) if want_std else None
    _lib.call("snerf_classic_sample_pdf", _p(bins), bins.stride(0), 1 if mid_mode else 0, wptr, weights.stride(0), nc,
              _p(u), us, n, nf, _p(out), _p(inds), _p(std), _stream())
    return out, inds, std


def classic_points(rays, z_vals):
    _chk2d("rays", rays, dt=torch.float32); _dev("z_vals", z_vals)
    n, S = z_vals.shape
    pts = torch.empty(n, S, 3, dtype=torch.float32, device=z_vals.device)
    _lib.call("snerf_classic_points", _p(rays), rays.stride(0), _p(z_vals), n, S, _p(pts), _stream())
    return pts


def classic_merge_sort(a, b):
    _dev("a b", a, b)
    n = a.shape[0]
    out = torch.empty(n, a.shape[1] + b.shape[1], dtype=torch.float32, device=a.device)
    _lib.call("snerf_classic_merge_sort", _p(a), a.shape[1], _p(b), b.shape[1], n, _p(out), _stream())
    return out


def mip_resample(s_vals, weights, u, resample_padding=0.01, want_idx=False):
    _dev("s_vals weights", s_vals, weights)
    n, P = s_vals.shape
    nf = u.shape[-1]
    u, us = _u_arg(u, n, nf)
    out = torch.empty(n, nf, dtype=torch.float32, device=s_vals.device)
    idx = torch.empty(n, nf, dtype=torch.int32, device=s_vals.device) if want_idx else None
    _lib.call("snerf_mip_resample", _p(s_vals), _p(weights), _p(u), us, n, P - 1, nf, float(resample_padding), _p(out), _p(idx), _stream())
    return out, idx


def jitter_u(jit, s):
    """math_ops.py:50-54: min(arange(P) * s + jit, 1 - eps) IN PLACE over the uniform draw jit [N, P] (one launch, the eager expression's bits)"""
    _dev("jit", jit)
    _lib.call("snerf_jitter_u", _p(jit), jit.shape[0], jit.shape[1], float(s), _stream())
    return jit


def stratified(base, rnd, near, far, n, mode, lindisp=False):
    """mode 0: classic z-values from near/far [N] views (stride in elements); mode 1: mip s-values."""
    _dev("base", base); _dev("rnd", rnd, optional=True)
    P = base.shape[0]
    out = torch.empty(n, P, dtype=torch.float32, device=base.device)
    nfs = 0
    if mode == 0:
        _require(near.is_cuda and far.is_cuda and near.dtype == torch.float32 and far.dtype == torch.float32 and near.stride(0) == far.stride(0),
                 "near, far: fp32 [N] CUDA views of one stride")
        nfs = near.stride(0)
    _lib.call("snerf_stratified", _p(base), _p(rnd), _p(near), _p(far), nfs, n, P, mode, 1 if lindisp else 0, _p(out), _stream())
    return out


# ------------------------------------------------------------- compositing ----
def mip_composite_fwd(raw_rgb, raw_density, noise, s_vals, dirs, near, far, transform_idx, white, rgb_padding, density_bias,
                      row_index=None):
    """row_index (int32 [n,S], optional): raw_* hold compacted rows; sample (ray, i) reads row row_index[ray, i], -1 = empty."""
    _dev("s_vals dirs near far", s_vals, dirs, near, far); _dev("noise", noise, optional=True)
    _dev("raw_rgb raw_density row_index", raw_rgb, raw_density, row_index, dtype=None, optional=True)
    n, P = s_vals.shape
    S = P - 1
    dev = s_vals.device
    comp = torch.empty(n, 3, dtype=torch.float32, device=dev) if raw_rgb is not None else None
    dist = torch.empty(n, dtype=torch.float32, device=dev)
    acc = torch.empty(n, dtype=torch.float32, device=dev)
    w = torch.empty(n, S, dtype=torch.float32, device=dev)
    _lib.call("snerf_mip_composite_fwd", _p(raw_rgb), 0 if raw_rgb is None else raw_rgb.stride(0), _p(raw_density),
              raw_density.stride(0), _p(noise), _p(s_vals), _p(dirs), _p(near), _p(far), n, S,
              transform_idx, 1 if white else 0, float(rgb_padding), float(density_bias), _p(comp), _p(dist), _p(acc), _p(w),
              _p(row_index), _stream())
    return comp, dist, acc, w


def mip_composite_bwd(raw_rgb, raw_density, noise, s_vals, dirs, near, far, transform_idx, white, rgb_padding, density_bias,
                      weights, distance, g_rgb, g_dist, g_acc, g_w, d_raw_rgb, d_raw_density, g_dirs=None):
    """`g_dirs` (optional fp32 [n,3], written): d loss / d directions through the interval lengths (t1 - t0) * |d|."""
    n, P = s_vals.shape
    _dev("g_rgb g_dist g_acc g_w weights distance g_dirs", g_rgb, g_dist, g_acc, g_w, weights, distance, g_dirs, optional=True)
    _lib.call("snerf_mip_composite_bwd", _p(raw_rgb), 0 if raw_rgb is None else raw_rgb.stride(0), _p(raw_density),
              raw_density.stride(0), _p(noise), _p(s_vals), _p(dirs), _p(near), _p(far), n, P - 1, transform_idx,
              1 if white else 0, float(rgb_padding), float(density_bias), _p(weights), _p(distance), _p(g_rgb), _p(g_dist),
              _p(g_acc), _p(g_w), _p(d_raw_rgb), 0 if d_raw_rgb is None else d_raw_rgb.stride(0), _p(d_raw_density),
              d_raw_density.stride(0), _p(g_dirs), _stream())


def mip_encode_bwd(s_vals, origins, directions, radii, near, far, cone, transform_idx, max_deg, dE, warp=None):
    """d loss / d (origins, directions) from the IPE feature gradients dE fp32 [n*S, >= 6*max_deg] (pose refinement).  `warp` = the
    forward's ((vx, vy, vz), far_max): the view-centred warp of an fn = 0 model (snerf_mip_encode_warp_bwd)."""
    _dev("s_vals", s_vals); _chk2d("dE", dE, dt=torch.float32)
    n, P = s_vals.shape
    _require(dE.shape[0] == n * (P - 1), "dE [n * S, >= 6 max_deg] for s_vals [n, S + 1]")
    g_o = torch.empty(n, 3, dtype=torch.float32, device=s_vals.device)
    g_d = torch.empty_like(g_o)
    if warp is not None:
        (vx, vy, vz), far_max = warp
        _dev("far_max", far_max)
        _lib.call("snerf_mip_encode_warp_bwd", _p(s_vals), _p(origins), _p(directions), _p(radii), _p(near), _p(far), n, P - 1, int(cone),
                  int(transform_idx), int(max_deg), _p(dE), dE.stride(0), _p(g_o), _p(g_d), 0, float(vx), float(vy), float(vz), _p(far_max), _stream())
        return g_o, g_d
    _lib.call("snerf_mip_encode_bwd", _p(s_vals), _p(origins), _p(directions), _p(radii), _p(near), _p(far), n, P - 1, int(cone),
              int(transform_idx), int(max_deg), _p(dE), dE.stride(0), _p(g_o), _p(g_d), _stream())
    return g_o, g_d


def mip_viewenc_bwd(viewdirs, S, deg, dV):
    """d loss / d viewdirs from the view-encoding feature gradients dV fp32 [n*S, >= 3 + 6*deg]."""
    _dev("viewdirs", viewdirs); _chk2d("dV", dV, dt=torch.float32)
    n = viewdirs.shape[0]
    _require(dV.shape[0] == n * S, "dV [n * S, >= 3 + 6 deg] for viewdirs [n, 3]")
    g = torch.empty(n, 3, dtype=torch.float32, device=viewdirs.device)
    _lib.call("snerf_mip_viewenc_bwd", _p(viewdirs), n, int(S), int(deg), _p(dV), dV.stride(0), _p(g), _stream())
    return g


def classic_composite_fwd(raw, noise, z_vals, rays_d, white):
    _chk2d("raw rays_d", raw, rays_d, dt=torch.float32); _dev("z_vals", z_vals); _dev("noise", noise, optional=True)
    n, S = z_vals.shape
    dev = z_vals.device
    rgb = torch.empty(n, 3, dtype=torch.float32, device=dev)
    disp, acc, depth = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(3))
    w = torch.empty(n, S, dtype=torch.float32, device=dev)
    _lib.call("snerf_classic_composite_fwd", _p(raw), raw.stride(0), _p(noise), _p(z_vals), _p(rays_d), rays_d.stride(0), n, S,
              1 if white else 0, _p(rgb), _p(disp), _p(acc), _p(w), _p(depth), _stream())
    return rgb, disp, acc, w, depth


def classic_composite_bwd(raw, noise, z_vals, rays_d, white, weights, acc, depth, g_rgb, g_disp, g_acc, g_depth, g_w, d_raw):
    n, S = z_vals.shape
    _dev("weights acc depth g_rgb g_disp g_acc g_depth g_w", weights, acc, depth, g_rgb, g_disp, g_acc, g_depth, g_w, optional=True)
    _lib.call("snerf_classic_composite_bwd", _p(raw), raw.stride(0), _p(noise), _p(z_vals), _p(rays_d), rays_d.stride(0), n, S,
              1 if white else 0, _p(weights), _p(acc), _p(depth), _p(g_rgb), _p(g_disp), _p(g_acc), _p(g_depth), _p(g_w),
              _p(d_raw), d_raw.stride(0), _stream())


# ------------------------------------------------------------ training tail ----
NONFINITE = {"keep": 0, "zero": 1, "nan_to_num": 2}


def adam_step(p, g, m, v, lr, b1, b2, eps, step, grad_scale=1.0, zero_grad=True, nonfinite="zero", grad_max_val=0.0, clip_coef=None,
              step_dev=None, lr_dev=None, dropped=None):
    """Fused Adam over a flat arena (snerf_adam_step_ex).  Gradient hygiene in the reference's order (train_utils.py:234-243):
    `clip_coef` (device float, see grad_clip_coef) -> value clip `grad_max_val` -> `nonfinite` policy ("zero": NaN/Inf gradients are
    dropped so that they can never poison m, v or the parameters; "nan_to_num": torch's nan_to_num_ exactly; "keep": plain Adam).
    `step_dev` (int32 [1] on the device, incremented by the launch) / `lr_dev` (fp32 [1]) replace the host scalars: graph-capturable."""
    _dev("p g m v lr_dev clip_coef", p, g, m, v, lr_dev, clip_coef, optional=True)
    _dev("step_dev", step_dev, dtype=torch.int32, optional=True)
    _dev("dropped", dropped, dtype=torch.int64, optional=True)   # int64 [1] on the device: += the number of NaN / +-Inf gradient elements of this launch (never reset here)
    if (step_dev is not None and step_dev.numel() != 1) or (lr_dev is not None and lr_dev.numel() != 1) or (dropped is not None and dropped.numel() != 1):
        raise _lib.SnerfArgumentError("step_dev int32 [1], lr_dev fp32 [1], dropped int64 [1]")
    _lib.call("snerf_adam_step_cnt", _p(p), _p(g), _p(m), _p(v), p.numel(), float(lr), float(b1), float(b2), float(eps), int(step),
              _p(step_dev), _p(lr_dev), float(grad_scale), 1 if zero_grad else 0, NONFINITE[nonfinite], float(grad_max_val), _p(clip_coef),
              _p(dropped), _stream())


def adam_step_dev(p, g, m, v, lr, b1, b2, eps, step_dev, grad_scale=1.0, zero_grad=True, **kw):
    """adam_step with the step counter in device memory (int32 [1], incremented by the launch): graph-capturable.  (The C-ABI also keeps
    the plain entries snerf_adam_step / snerf_adam_step_dev = snerf_adam_step_ex without the hygiene options.)"""
    adam_step(p, g, m, v, lr, b1, b2, eps, 0, grad_scale, zero_grad, step_dev=step_dev, **kw)


def sgd_step(p, g, lr, grad_scale=1.0, nonfinite="zero", grad_max_val=0.0, clip_coef=None, dropped=None):
    """Plain SGD over a flat buffer (snerf_sgd_step; torch.optim.SGD without momentum or weight decay): p -= lr * hygiene(g * grad_scale),
    g = 0.  The hygiene options are adam_step's, in the same order."""
    _dev("p g", p, g); _dev("clip_coef", clip_coef, optional=True); _dev("dropped", dropped, dtype=torch.int64, optional=True)
    _require(p.numel() == g.numel() and (dropped is None or dropped.numel() == 1), "p, g: fp32 of one size; dropped int64 [1]")
    _lib.call("snerf_sgd_step", _p(p), _p(g), p.numel(), float(lr), float(grad_scale), float(grad_max_val), _p(clip_coef), NONFINITE[nonfinite],
              _p(dropped), _stream())


def grad_clip_coef(g, grad_scale, max_norm):
    """-> fp32 [2] on the device = (min(1, max_norm / (|grad_scale| ||g|| + 1e-6)), the norm): clip_grad_norm_'s coefficient for adam_step.
    A NaN in g gives (NaN, NaN) as in torch -- adam_step's `nonfinite` policy then decides about the whole step; +-Inf gives (0, Inf)."""
    _dev("g", g)
    ws = torch.empty(1024, dtype=torch.float64, device=g.device)
    out = torch.empty(2, dtype=torch.float32, device=g.device)
    _lib.call("snerf_grad_clip_coef", _p(g), g.numel(), float(grad_scale), float(max_norm), _p(ws), _p(out), _stream())
    return out


def nonfinite_flag(g, flag):
    """flag (int32 [1] on the device, zeroed by the caller) |= 1 when any fp32 element of `g` is NaN / +-Inf: the found-inf pass of a
    dynamic loss scaler (snerf_nonfinite_flag).  No host sync."""
    _dev("g", g); _dev("flag", flag, dtype=torch.int32)
    _require(flag.numel() >= 1, "flag: int32 [1] on the device")
    _lib.call("snerf_nonfinite_flag", _p(g), g.numel(), _p(flag), _stream())


def colsum_f32(x, C, out, deterministic=False):
    _chk2d("x", x, dt=torch.float32)
    _lib.call("snerf_colsum_f32_det" if deterministic else "snerf_colsum_f32", _p(x), x.stride(0), x.shape[0], C, _p(out), _stream())


def split_cast(src, C, dst, Cpad):
    """fp32 [M, >= C] -> split-bf16 rows in the GEMMs' interleaved layout: dst [M, >= 2 Cpad] bf16, Cpad % 64 == 0 logical columns
    (hi at physical [128 j, 128 j + 64), lo at [128 j + 64, 128 j + 128) of logical columns [64 j, 64 j + 64); columns >= C zero)."""
    _chk2d("src", src, dt=torch.float32); _chk2d("dst", dst, dt=torch.bfloat16)
    _require(dst.shape[0] == src.shape[0] and dst.shape[1] >= 2 * Cpad and src.shape[1] >= C, "src [M, >= C], dst [M, >= 2 Cpad]")
    _lib.call("snerf_split_cast", _p(src), src.stride(0), src.shape[0], C, Cpad, _p(dst), dst.stride(0), _stream())


def split8_cast(src, C, dst, Cpad, weight=False):
    """fp32 [M, >= C] -> rows in the fp16 + fp8 split layout (dtype F16F8; csrc/gemm.hip, GemmNT::split == 2): dst [M, >= 2 Cpad] fp16-typed, per 64
    logical columns [fp16(x) x 64 | 128 e4m3 bytes]: the residual x - fp16(x) scaled by 2^13 and x scaled by 2^2 (activations), or -- `weight` --
    w scaled by 2^9 and its residual scaled by 2^20; columns >= C zero."""
    _chk2d("src", src, dt=torch.float32); _chk2d("dst", dst, dt=torch.float16)
    _require(dst.shape[0] == src.shape[0] and dst.shape[1] >= 2 * Cpad and src.shape[1] >= C, "src [M, >= C], dst [M, >= 2 Cpad]")
    _lib.call("snerf_split8_cast", _p(src), src.stride(0), src.shape[0], C, Cpad, _p(dst), dst.stride(0), 1 if weight else 0, _stream())


def cast_pad(src, C, dst, Cpad, dt):
    if dt == BF16X3:
        return split_cast(src, C, dst, Cpad)
    if dt == F16F8:
        return split8_cast(src, C, dst, Cpad)
    _chk2d("src", src, dt=torch.float32)
    _lib.call("snerf_cast_pad", _p(src), src.stride(0), src.shape[0], C, Cpad, _p(dst), dst.stride(0), dt, _stream())


def classic_x_grad(g0, g5, gv, ic, icv, dx):
    """gradient w.r.t. the classic network's pre-embedded input: dx[:, :ic] = g0 + g5 (the data gradients reaching the point block
    through pts_linears.0 and the skip layer), dx[:, ic:ic + icv] = gv (through views_linears.0; None when icv == 0).  fp32 2-D views."""
    _chk2d("g0 g5 dx", g0, g5, dx, dt=torch.float32)
    M = dx.shape[0]
    _require(g0.shape[0] == g5.shape[0] == M and g0.shape[1] >= ic and g5.shape[1] >= ic and dx.shape[1] >= ic + icv, "g0, g5 [M, >= ic], dx [M, >= ic + icv]")
    if icv > 0:
        _chk2d("gv", gv, dt=torch.float32)
        _require(gv.shape[0] == M and gv.shape[1] >= icv, "gv [M, >= icv]")
    _lib.call("snerf_classic_x_grad", _p(g0), g0.stride(0), _p(g5), g5.stride(0), _p(gv), 0 if gv is None else gv.stride(0), M, int(ic),
              int(icv), _p(dx), dx.stride(0), _stream())

def gather_pack(flat, idx, dst, tiles=None):
    """dst[i] = flat[idx[i]] (idx -1 -> 0, -2 -> 1) rounded to dst's dtype: all packed operands of a network in one launch.  `tiles` (int32
    [n, 4] = dst_off, src_base, src_stride, dst_ld: 16 x 64 transposed tiles, their elements marked idx = -3): snerf_gather_pack_tiles."""
    _dev("flat", flat); _dev("idx", idx, dtype=torch.int32); _dev("dst", dst, dtype=(torch.float32, torch.bfloat16, torch.float16))
    _require(dst.numel() == idx.numel(), "dst: one element per idx")
    if tiles is None or tiles.numel() == 0:
        _lib.call("snerf_gather_pack", _p(flat), _p(idx), idx.numel(), _p(dst), _zip_dt(dst), _stream())
        return
    _dev("tiles", tiles, dtype=torch.int32, shape=(None, 4))
    _lib.call("snerf_gather_pack_tiles", _p(flat), _p(idx), idx.numel(), _p(dst), _zip_dt(dst), _p(tiles), tiles.shape[0], _stream())


def gather_pack_pair(flat, idx, dst, tiles, idx32, dst32):
    """gather_pack of a 16-bit pool (with its transposed tiles, or None) and of the network's fp32 pool in ONE launch (snerf_gather_pack_pair)"""
    _dev("flat dst32", flat, dst32); _dev("idx idx32", idx, idx32, dtype=torch.int32); _dev("dst", dst, dtype=(torch.bfloat16, torch.float16))
    _require(dst.numel() == idx.numel() and dst32.numel() == idx32.numel(), "dst, dst32: one element per idx, idx32")
    nt = 0 if tiles is None else tiles.shape[0]
    _dev("tiles", tiles, dtype=torch.int32, shape=(None, 4), optional=True)
    _lib.call("snerf_gather_pack_pair", _p(flat), _p(idx), idx.numel(), _p(dst), _zip_dt(dst), _p(tiles), nt, _p(idx32), idx32.numel(), _p(dst32), _stream())


# ------------------------------------------------------------ hash grid ----
def grid_per_level_scale(base_resolution, desired_resolution, num_levels):
    """growth factor that puts level num_levels - 1 at desired_resolution (gridencoder/grid.py:104-106)"""
    import numpy as np
    return float(np.exp2(np.log2(desired_resolution / base_resolution) / (num_levels - 1)))


def grid_level_layout(input_dim, num_levels, per_level_scale, base_resolution, log2_hashmap_size, align_corners=False):
    """Row layout of a multiresolution hash table (gridencoder/grid.py:122-141), all levels at once: level l has
    ceil(base * scale^l) (+ 1 unless align_corners) grid points per axis and min(2^log2T, points^D) rows rounded up to a multiple of 8.
    -> (offsets int32 [L + 1], grid_sizes int32 [L]); shared by the drop-in GridEncoder and the zipnerf Model's fused encoders."""
    import numpy as np
    lv = np.arange(num_levels, dtype=np.float64)
    sizes = np.ceil(base_resolution * np.asarray(per_level_scale, dtype=np.float64) ** lv).astype(np.int64) + (0 if align_corners else 1)
    dense = np.array([int(r) ** input_dim for r in sizes], dtype=object)             # (python ints: 8193^5 does not fit int64)
    rows = np.array([-(-min(int(d), 2 ** log2_hashmap_size) // 8) * 8 for d in dense], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(rows)])
    if offsets[-1] >= 2 ** 31:
        raise ValueError("hash table rows exceed int32 offsets")
    return offsets.astype(np.int32), sizes.astype(np.int32)


_GRID_DT = {torch.float32: F32, torch.float16: F16, torch.float64: F64}    # the reference's three instantiations (gridencoder.cu:469)
_GRID_DTS = tuple(_GRID_DT)


def grid_encode_fwd(inputs, embeddings, offsets, L, S, H, gridtype, align_corners, interp, want_dy_dx=False, level_major=False, reference_form=None):
    """inputs fp32 [B,D] in [0,1]; embeddings [sO,C] fp32/fp16 -> outputs [B, L*C] (or [L,B,C] if level_major) in the
    table dtype (+ dy_dx [B, L*D*C]).  reference_form (default: not GRID_FAST): kernel_grid's one-thread-per-(point, level) form for every
    instantiation (snerf_grid_encode_fwd_ref) -- the A/B partner of the measurement legs; same bits."""
    _dev("inputs", inputs); _dev("embeddings", embeddings, dtype=_GRID_DTS); _dev("offsets", offsets, dtype=torch.int32)
    B, D = inputs.shape
    C = embeddings.shape[1]
    dt = _GRID_DT[embeddings.dtype]
    if level_major:
        out = torch.empty(L, B, C, dtype=embeddings.dtype, device=inputs.device); sl, sb = B * C, C
    else:
        out = torch.empty(B, L * C, dtype=embeddings.dtype, device=inputs.device); sl, sb = C, L * C
    dy_dx = torch.empty(B, L * D * C, dtype=embeddings.dtype, device=inputs.device) if want_dy_dx else None
    ref = (not GRID_FAST) if reference_form is None else bool(reference_form)
    _lib.call("snerf_grid_encode_fwd_ref" if ref else "snerf_grid_encode_fwd", _p(inputs), _p(embeddings), _p(offsets), _p(out), B, D, C, L, float(S), int(H), _p(dy_dx),
              int(gridtype), 1 if align_corners else 0, int(interp), dt, sl, sb, _stream())
    return out, dy_dx


def grid_encode_bwd(grad, inputs, embeddings, offsets, L, S, H, gridtype, align_corners, interp, dy_dx=None, level_major=False):
    """grad [B, L*C] (or [L,B,C]) in the table dtype -> (grad_embeddings like embeddings, grad_inputs [B,D] or None)."""
    _dev("inputs", inputs); _dev("grad", grad, dtype=embeddings.dtype)
    B, D = inputs.shape
    C = embeddings.shape[1]
    dt = _GRID_DT[embeddings.dtype]
    sl, sb = (B * C, C) if level_major else (C, L * C)
    g_emb = torch.zeros_like(embeddings)
    g_in = torch.zeros(B, D, dtype=embeddings.dtype, device=inputs.device) if dy_dx is not None else None
    _lib.call("snerf_grid_encode_bwd", _p(grad), _p(inputs), _p(embeddings), _p(offsets), _p(g_emb), B, D, C, L, float(S), int(H),
              _p(dy_dx), _p(g_in), int(gridtype), 1 if align_corners else 0, int(interp), dt, sl, sb, _stream())
    return g_emb, g_in


def grid_fast_ok(D, C, gridtype, align_corners, interp, dtype, want_dy_dx=False):
    """the instantiations that run on the pair-loading gather / binned table gradient (csrc/zip.hip g3_*): D = 3, hash, linear -- what
    zipnerf constructs (internal/models.py:413-421: C = 4 / 1), at every channel count.  Everything else -- and SNERF_GRID_FAST=0 -- runs the one-thread-per-(point, level) kernels of csrc/grid.hip."""
    return (GRID_FAST and D == 3 and C in (1, 2, 4, 8) and int(gridtype) == 0 and not align_corners and int(interp) == 0 and not want_dy_dx
            and dtype in (torch.float32, torch.float16))


GRID_FAST = _os.environ.get("SNERF_GRID_FAST", "1") != "0"          # (python-side default of the A/B choice; the library itself holds no switch)


def grid_set_fast_path(on: bool):
    """default form of the stand-alone encoder for callers that do not say (bench.py's grid_encoder leg times both in one process):
    picks the ENTRY POINT grid_encode_fwd calls and whether GridEncoder.backward takes the binned table gradient.  Returns the previous value."""
    global GRID_FAST
    prev = GRID_FAST
    GRID_FAST = bool(on)
    return prev


def grid_host_offsets(offsets):
    """host copy (numpy int32) of a GridEncoder's device `offsets` buffer -- the bin plan of the binned table gradient is made on the
    host.  The copy rides on the tensor OBJECT (with the tensor's version), so a module's buffer is copied once; a foreign or rebuilt
    tensor costs one device->host copy per call.  (Never keyed by address: a freed buffer's address can come back with other contents.)"""
    c = getattr(offsets, "_snerf_host_offsets", None)
    if c is not None and c[0] == offsets._version:
        return c[1]
    import numpy as np
    h = np.ascontiguousarray(offsets.detach().cpu().numpy().astype(np.int32))
    try:
        offsets._snerf_host_offsets = (offsets._version, h)
    except AttributeError:
        pass
    return h


GRID_BWD_WS_BYTES = int(_os.environ.get("SNERF_GRID_BWD_WS", "0"))        # workspace of the binned table gradient; 0: the library's recommendation (<= 1 GiB)


def grid_encode_bwd_binned(grad, inputs, offsets, C, L, S, H, out_dtype=torch.float32, half_records=None, level_major=False, offsets_host=None, ws_bytes=None):
    """Table gradient of the stand-alone GridEncoder without atomics (snerf_grid_encode_bwd_binned; D = 3, hash, linear, C in {1, 2, 4, 8}):
    grad [B, L*C] (or [L,B,C]) fp32 / fp16 -> grad_embeddings [rows, C] in `out_dtype`, bit-reproducible.  `half_records` (default:
    follows the gradient's dtype): contributions travel as fp16 -- the reference adds __half2 atomics into a half table's gradient.
    `ws_bytes`: size of the workspace the call may use (default: snerf_grid_encode_bwd_binned_ws_bytes, at most 1 GiB at any B); the
    call chunks the points to fit it."""
    _dev("inputs", inputs); _dev("grad", grad, dtype=(torch.float32, torch.float16))
    _require(out_dtype in (torch.float32, torch.float16) and C in (1, 2, 4, 8), "out_dtype fp32 / fp16, C in (1, 2, 4, 8)")
    B = inputs.shape[0]
    oh = grid_host_offsets(offsets) if offsets_host is None else offsets_host
    if half_records is None:
        half_records = grad.dtype == torch.float16 and C in (1, 4)        # (C = 2 / 8 travel as fp32 records)
    g_emb = torch.zeros(int(oh[-1]), C, dtype=out_dtype, device=inputs.device)
    if B == 0:
        return g_emb
    nb = _lib.query("snerf_grid_encode_bwd_binned_ws_bytes", B, C, L, oh.ctypes.data, 1 if half_records else 0)
    if nb < 0:
        raise ValueError("grid_encode_bwd_binned: level layout outside the binned kernels' range (more than 1024 row ranges per level)")
    want = int(ws_bytes if ws_bytes is not None else (GRID_BWD_WS_BYTES or nb))
    ws = _zb_workspace(inputs.device, "g3ws", (want + 255) // 256 * 256, torch.uint8)
    sl, sb = (B * C, C) if level_major else (C, L * C)
    _lib.call("snerf_grid_encode_bwd_binned", _p(grad), _p(inputs), _p(offsets), oh.ctypes.data, _p(g_emb), B, C, L, float(S), int(H),
              _GRID_DT[grad.dtype], _GRID_DT[out_dtype], sl, sb, 1 if half_records else 0, _p(ws), want, _stream())
    return g_emb


def grid_encode_bwd_binned_plan(B, C, L, offsets_host, half_records, grad_dtype=torch.float16, level_major=False, ws_bytes=None):
    """what snerf_grid_encode_bwd_binned would run on a workspace of ws_bytes (default: the recommended size): dict(chunks, chunk_points,
    levels_per_transposed_group, launches, chunk_record_capacity, bytes_used, ws_bytes)"""
    import numpy as np
    oh = np.ascontiguousarray(np.asarray(offsets_host, dtype=np.int32))
    if ws_bytes is None:
        ws_bytes = _lib.query("snerf_grid_encode_bwd_binned_ws_bytes", B, C, L, oh.ctypes.data, 1 if half_records else 0)
    out = (ctypes.c_long * 6)()
    _lib.call("snerf_grid_encode_bwd_binned_plan", B, C, L, oh.ctypes.data, 1 if half_records else 0, _GRID_DT[grad_dtype], 1 if level_major else 0,
              int(ws_bytes), ctypes.addressof(out))
    return dict(chunks=out[0], chunk_points=out[1], levels_per_transposed_group=out[2], launches=out[3], chunk_record_capacity=out[4], bytes_used=out[5],
                ws_bytes=int(ws_bytes))


def grid_tv_grad(inputs, embeddings, grad, offsets, weight, L, S, H, gridtype, align_corners):
    _dev("inputs", inputs); _dev("embeddings", embeddings, dtype=_GRID_DTS); _dev("grad", grad, dtype=embeddings.dtype)
    B, D = inputs.shape
    dt = _GRID_DT[embeddings.dtype]
    _lib.call("snerf_grid_tv_grad", _p(inputs), _p(embeddings), _p(grad), _p(offsets), float(weight), B, D, embeddings.shape[1], L,
              float(S), int(H), int(gridtype), 1 if align_corners else 0, dt, _stream())


# ------------------------------------------------------------ zipnerf path ----
def zip_resample(sdist, weights, u, n, near, far, dilation, dilate, anneal, resample_padding=0.0, lam=-1.5, dom=(0.0, 1.0)):
    _dev("sdist weights near far", sdist, weights, near, far)
    R, P0 = sdist.shape
    u, us = _u_arg(u, R, n)
    so = torch.empty(R, n + 1, dtype=torch.float32, device=sdist.device)
    to = torch.empty_like(so)
    _lib.call("snerf_zip_resample", _p(sdist), _p(weights), P0 - 1, _p(u), us, n, _p(near), _p(far), R, float(dilation), 1 if dilate else 0,
              float(anneal), float(resample_padding), float(lam), float(dom[0]), float(dom[1]), _p(so), _p(to), _stream())
    return so, to


_ZIP_DT = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}
_ZIP_DTS = tuple(_ZIP_DT)


def _zip_dt(t):
    return _ZIP_DT[t.dtype]


def round_mode(dt):
    """rounding mode of the fused proposal networks (their activations are rounded like the GEMM route's buffers of that compute dtype):
    0 none (fp32), 1 bf16, 2 fp16.  Accepts a compute dtype code or the older bool (True = bf16)."""
    if isinstance(dt, bool):
        return 1 if dt else 0
    return {F32: 0, BF16: 1, F16: 2}[int(dt)]


def zip_encode_fwd(tdist, origins, directions, radii, base_x, base_y, deg_jitter, table, offsets, grid_sizes, feat, L, C, n, m, Sl, H, std_scale,
                   levels_per_thread=0):
    _dev("tdist origins directions radii base_x base_y deg_jitter", tdist, origins, directions, radii, base_x, base_y, deg_jitter, optional=True)
    R, P = tdist.shape
    _dev("table", table, dtype=_ZIP_DTS); _dev("offsets grid_sizes", offsets, grid_sizes, dtype=torch.int32)
    _lib.call("snerf_zip_encode_fwd", _p(tdist), _p(origins), _p(directions), _p(radii), _p(base_x), _p(base_y), _p(deg_jitter), _p(table),
              _p(offsets), _p(grid_sizes), _p(feat), feat.stride(0), R, P - 1, L, C, n, m, float(Sl), int(H), float(std_scale), _zip_dt(table),
              _zip_dt(feat), int(levels_per_thread), _stream())


def zip_encode_fwd_count(tdist, origins, directions, radii, base_x, base_y, deg_jitter, table, offsets, grid_sizes, feat, L, C, n, m, Sl, H, std_scale,
                         ksplit, level_rows):
    """zip_encode_fwd (one thread per (interval, level)) that also counts the records of the binned table gradient and reserves the
    workgroups' ranges: pass 0 of zip_encode_bwd_binned in the forward's sweep.  -> (counts, wg_offsets) to hand to zip_encode_bwd_binned
    as `precounted`.  wg_offsets is a buffer of its own per call: it lives until the backward."""
    import numpy as np
    _dev("tdist origins directions radii base_x base_y deg_jitter", tdist, origins, directions, radii, base_x, base_y, deg_jitter, optional=True)
    R, P = tdist.shape
    S = P - 1
    _dev("table", table, dtype=_ZIP_DTS); _dev("offsets grid_sizes", offsets, grid_sizes, dtype=torch.int32)
    _require(C in (1, 4) and n <= 8 and L <= 16, "the counting forward runs C in (1, 4), n <= 8, L <= 16")
    ks = np.ascontiguousarray(np.asarray(ksplit, dtype=np.int32))
    lr = np.ascontiguousarray(np.asarray(level_rows, dtype=np.int32))
    _require(ks.shape == (L,) and lr.shape == (L,), "ksplit, level_rows: one int per level (zip_bin_plan)")
    counts = torch.zeros(L, ZB_NBMAX, dtype=torch.int32, device=tdist.device)
    wgo = torch.empty(L * ((R * S + 255) // 256) * ZB_NBMAX, dtype=torch.int32, device=tdist.device)
    _lib.call("snerf_zip_encode_fwd_count", _p(tdist), _p(origins), _p(directions), _p(radii), _p(base_x), _p(base_y), _p(deg_jitter), _p(table),
              _p(offsets), _p(grid_sizes), _p(feat), feat.stride(0), R, S, L, C, n, m, float(Sl), int(H), float(std_scale), _zip_dt(table),
              _zip_dt(feat), ks.ctypes.data, lr.ctypes.data, _p(counts), _p(wgo), _stream())
    return counts, wgo


def zip_prop_mlp_fwd(F, L, w1, b1, w2, b2, round_bf16):
    """Proposal MLP of a training step in one launch: F [P, >= L] (fp32 / bf16, compact) -> raw density [P, 1] fp32."""
    _chk2d("F", F, dt=F.dtype)
    _dev("w1 b1 w2 b2", w1, b1, w2, b2)
    P, hidden = F.shape[0], b1.numel()
    _require(F.dtype in _ZIP_DT and w1.numel() == hidden * L and w2.numel() == hidden and b2.numel() == 1 and hidden <= 64 and L <= 16,
             "F fp32 / bf16 / fp16; w1 [hidden, L], b1, w2 [hidden], b2 [1] with hidden <= 64, L <= 16")
    raw = torch.empty(P, 1, dtype=torch.float32, device=F.device)
    _lib.call("snerf_zip_prop_mlp_fwd", _p(F), F.stride(0), P, int(L), _p(w1), _p(b1), _p(w2), _p(b2), hidden, round_mode(round_bf16), _zip_dt(F),
              _p(raw), _stream())
    return raw


def zip_prop_mlp_bwd(F, d_raw, L, w1, b1, w2, b2, round_bf16, g_w1, g_b1, g_w2, g_b2):
    """Backward of zip_prop_mlp_fwd: -> dF (F's shape and dtype); the parameter gradients are ADDED into g_* (fp32 views of the
    parameters' shapes), bit-reproducibly."""
    _chk2d("F", F, dt=F.dtype)
    _dev("d_raw w1 b1 w2 b2 g_w1 g_b1 g_w2 g_b2", d_raw, w1, b1, w2, b2, g_w1, g_b1, g_w2, g_b2)
    P, hidden = F.shape[0], b1.numel()
    _require(d_raw.numel() == P and F.shape[1] <= 64, "d_raw [P, 1] for F [P, <= 64]")
    _require(g_w1.numel() == hidden * L and g_b1.numel() == hidden and g_w2.numel() == hidden and g_b2.numel() == 1, "g_*: the parameters' sizes")
    dF = torch.empty(P, F.shape[1], dtype=F.dtype, device=F.device)
    nws = _lib.query("snerf_zip_prop_mlp_ws_floats", int(L), hidden, P)
    ws = torch.empty(max(int(nws), 1), dtype=torch.float32, device=F.device)
    _lib.call("snerf_zip_prop_mlp_bwd", _p(F), F.stride(0), _p(d_raw), P, int(L), _p(w1), _p(b1), _p(w2), _p(b2), hidden, round_mode(round_bf16),
              _zip_dt(F), _p(dF), dF.stride(0), _p(g_w1), _p(g_b1), _p(g_w2), _p(g_b2), _p(ws), ws.numel(), _stream())
    return dF


def zip_encode_prop_fwd(tdist, origins, directions, radii, base_x, base_y, deg_jitter, table, offsets, grid_sizes, L, n, m, Sl, H, std_scale,
                        w1, b1, w2, b2, round_bf16):
    """Fused featurisation + proposal MLP of one proposal level (inference) -> raw density [R*S, 1] fp32."""
    _dev("tdist origins directions radii base_x base_y deg_jitter w1 b1 w2 b2", tdist, origins, directions, radii, base_x, base_y, deg_jitter, w1, b1, w2, b2, optional=True)
    R, P = tdist.shape
    hidden = b1.numel()
    _dev("table", table, dtype=_ZIP_DTS)
    _require(table.shape[-1] == 1 and w1.numel() == hidden * L and w2.numel() == hidden and b2.numel() == 1,
             "table [rows, 1]; w1 [hidden, L], w2 [hidden], b2 [1]")
    out = torch.empty(R * (P - 1), 1, dtype=torch.float32, device=tdist.device)
    _lib.call("snerf_zip_encode_prop_fwd", _p(tdist), _p(origins), _p(directions), _p(radii), _p(base_x), _p(base_y), _p(deg_jitter), _p(table),
              _p(offsets), _p(grid_sizes), R, P - 1, L, n, m, float(Sl), int(H), float(std_scale), _zip_dt(table), _p(w1), _p(b1), _p(w2), _p(b2),
              hidden, round_mode(round_bf16), _p(out), _stream())
    return out


def zip_encode_bwd(tdist, origins, directions, radii, base_x, base_y, deg_jitter, offsets, grid_sizes, grad_feat, grad_table, L, C, n, m, Sl, H,
                   std_scale, lds_levels=0, lds_cells=0, lds_slabs=0, grad_table_bf16=None):
    _dev("tdist origins directions radii base_x base_y deg_jitter offsets grid_sizes grad_feat", tdist, origins, directions, radii, base_x, base_y,
         deg_jitter, offsets, grid_sizes, grad_feat, dtype=None, optional=True)
    R, P = tdist.shape
    _dev("grad_table", grad_table); _dev("grad_table_bf16", grad_table_bf16, dtype=torch.bfloat16, optional=True)
    _require(grad_table_bf16 is None or grad_table_bf16.numel() == grad_table.numel(), "grad_table_bf16: grad_table's size")
    _lib.call("snerf_zip_encode_bwd", _p(tdist), _p(origins), _p(directions), _p(radii), _p(base_x), _p(base_y), _p(deg_jitter), _p(offsets),
              _p(grid_sizes), _p(grad_feat), grad_feat.stride(0), _p(grad_table), R, P - 1, L, C, n, m, float(Sl), int(H), float(std_scale),
              _zip_dt(grad_feat), int(lds_levels), int(lds_cells), int(lds_slabs), _p(grad_table_bf16), _stream())


ZB_NBMAX, ZB_TARGET = 1024, 2_000_000


def zip_bin_plan(offsets_host, C, records_per_level):
    """Host-side plan of the binned table gradient: per level the number of replicas K of every row range (levels with few, hot rows
    are split so that a bin holds ~ZB_TARGET records) and the number of leading table rows the int64 meeting image must cover."""
    br = 4096 if C == 4 else 16384
    ks, g64_rows, level_rows = [], 0, []
    for l in range(len(offsets_host) - 1):
        rows = int(offsets_host[l + 1] - offsets_host[l])
        rowbins = max((rows + br - 1) // br, 1)
        if rowbins > ZB_NBMAX:
            raise ValueError(f"binned table gradient: level {l} has {rows} rows = {rowbins} row ranges of {br}, more than the {ZB_NBMAX} bins per "
                             "level of the kernels; use table_grad_mode='atomic' for tables this large")
        k = max(1, min(-(-int(records_per_level) // (rowbins * ZB_TARGET)), ZB_NBMAX // rowbins))
        ks.append(k)
        level_rows.append(rows)
        if k > 1:
            g64_rows = int(offsets_host[l + 1])
    return ks, g64_rows, level_rows


_zb_ws = {}


def _zb_workspace(dev, key, numel, dtype):
    """the binned backward's worst-case buffers, kept across calls (one stream: a call's kernels finish before the next call reuses
    them); grown, never shrunk"""
    t = _zb_ws.get((dev, key))
    if t is None or t.numel() < numel or t.dtype != dtype:
        t = torch.empty(numel, dtype=dtype, device=dev)
        _zb_ws[(dev, key)] = t
    return t


ZIP_BIN_ALL_LEVELS = _os.environ.get("SNERF_ZIP_ALL_LEVELS", "") != ""   # probe switch: A/B runs of tools/bench_zip.py
ZIP_BIN_STAGED = _os.environ.get("SNERF_ZIP_UNSTAGED", "") == ""      # (the environment switch: A/B runs of tools/bench_zip.py)


def zip_encode_bwd_binned(tdist, origins, directions, radii, base_x, base_y, deg_jitter, offsets, grid_sizes, grad_feat, grad_table, L, C, n, m, Sl, H,
                          std_scale, ksplit, g64_rows, level_rows, precounted=None, half_records=False):
    """The table gradient of zip_encode_bwd without L2 atomics on the hashed levels and bit-reproducible: records binned by destination,
    accumulated per bin in LDS with fixed-point integer atomics (snerf_zip_encode_bwd_binned: count, scan on the device, write, accumulate).
    The fixed-point grid follows the gradient's magnitude (snerf_zip_bin_scale: 34 bits below max |grad_feat|).  `precounted` = the
    (counts, wg_offsets) pair zip_encode_fwd_count returned for the same intervals and bin plan: the count pass is then skipped.
    `half_records`: the records carry fp16 values scaled by the launch's exponent (10 / 4 instead of 18 / 8 bytes per record at C = 4 / 1):
    every contribution is rounded to 11 significant bits once, the sums stay exact and order-independent (csrc/zip.hip, ZB_HALF_SHIFT)."""
    import numpy as np
    R, P = tdist.shape
    S = P - 1
    dev = tdist.device
    _dev("grad_table", grad_table)
    _require(C in (1, 4) and L <= 16, "the binned table gradient runs C in (1, 4), L <= 16")
    ks = np.ascontiguousarray(np.asarray(ksplit, dtype=np.int32))
    lr = np.ascontiguousarray(np.asarray(level_rows, dtype=np.int32))
    _require(ks.shape == (L,) and lr.shape == (L,), "ksplit, level_rows: one int per level (zip_bin_plan)")
    scale = torch.empty(2, dtype=torch.int32, device=dev)
    _lib.call("snerf_zip_bin_scale", _p(grad_feat), grad_feat.stride(0), R * S, L * C, _zip_dt(grad_feat), _p(scale), _stream())
    args = (_p(tdist), _p(origins), _p(directions), _p(radii), _p(base_x), _p(base_y), _p(deg_jitter), _p(offsets), _p(grid_sizes), _p(grad_feat),
            grad_feat.stride(0), _p(grad_table), R, S, L, C, n, m, float(Sl), int(H), float(std_scale), _zip_dt(grad_feat), ks.ctypes.data,
            lr.ctypes.data)
    if precounted is not None:
        # the training forward (zip_encode_fwd_count) already counted the records and reserved the workgroups' ranges
        counts, wgo = precounted
        _dev("precounted", counts, wgo, dtype=None)
        _require(counts.shape == (L, ZB_NBMAX) and wgo.numel() >= L * ((R * S + 255) // 256) * ZB_NBMAX,
                 "precounted: zip_encode_fwd_count's (counts, wg_offsets) of the same intervals and bin plan")
    else:
        # pass 0 also reserves each workgroup's record range inside the bins it touches (offsets relative to the bin's start)
        counts = torch.zeros(L, ZB_NBMAX, dtype=torch.int32, device=dev)
        wgo = _zb_workspace(dev, "wgo", L * ((R * S + 255) // 256) * ZB_NBMAX, torch.int32)
        _lib.call("snerf_zip_encode_bwd_binned", 0, *args, _p(counts), _p(wgo), None, None, None, 0, None, 0, None, _stream())
    starts = torch.empty(L * ZB_NBMAX, dtype=torch.int64, device=dev)
    _lib.call("snerf_zip_bin_scan", _p(counts), _p(starts), L, _stream())                  # exclusive scan of the bin counts, on the device
    capacity = R * S * n * 8 * L                               # every (interval, level) emits at most n cells x 8 corners: no host sync
    rec_row = _zb_workspace(dev, "row", capacity if C == 4 else 1, torch.int16)          # (C = 1 records carry their row)
    rec_val = _zb_workspace(dev, "val", capacity * max(C, 2), torch.float32)       # C = 1: {row, value} pairs in one 8-byte record
    # pass 1: the records staged in LDS and written run by run; ZIP_BIN_STAGED = False (A/B probes, tests): pass 3, every thread
    # writes its records where they fall (same records, another order inside a (workgroup, bin) run)
    wpass = (5 if ZIP_BIN_STAGED else 6) if half_records else (1 if ZIP_BIN_STAGED else 3)
    if ZIP_BIN_ALL_LEVELS and ZIP_BIN_STAGED:            # (probe: the all-levels direct writer for the four-channel grid too)
        wpass = 9 if half_records else 8
    _lib.call("snerf_zip_encode_bwd_binned", wpass, *args, _p(counts), _p(wgo), _p(starts), _p(rec_row), _p(rec_val), capacity,
              None, 0, _p(scale) if half_records else None, _stream())
    g64 = torch.zeros(max(g64_rows, 1) * C, dtype=torch.int64, device=dev) if g64_rows > 0 else None
    _lib.call("snerf_zip_encode_bwd_binned", 7 if half_records else 2, *args, _p(counts), _p(wgo), _p(starts), _p(rec_row), _p(rec_val), capacity, _p(g64), int(g64_rows),
              _p(scale), _stream())


def colsum_wide_f32(x, C, out, deterministic=False):
    """out[:C] += x[:, :C].sum(0) for any C (fp32)"""
    _chk2d("x", x, dt=torch.float32); _dev("out", out)
    _require(out.numel() >= C and x.shape[1] >= C, "x [M, >= C], out [>= C]")
    _lib.call("snerf_colsum_wide_f32", _p(x), x.stride(0), x.shape[0], int(C), _p(out), 1 if deterministic else 0, _stream())


def zip_glo_modulate(X, SS, S, out):
    """out = X * exp(scale) + shift per ray (GLO modulation of the bottleneck, internal/models.py:620-630): X / out [R * S, >= B] in the
    compute dtype, SS [R, 2 B] fp32 = (scale | shift)"""
    B = SS.shape[1] // 2
    _chk2d("X out", X, out, dt=X.dtype); _chk2d("SS", SS, dt=torch.float32)
    R = SS.shape[0]
    _require(X.shape[0] == R * S == out.shape[0] and X.shape[1] >= B and out.shape[1] >= B and X.dtype in _ZIP_DT,
             "X, out [R * S, >= B] fp32 / bf16 / fp16 for SS [R, 2 B]")
    _lib.call("snerf_zip_glo_modulate", _p(X), X.stride(0), _p(SS), SS.stride(0), R, S, B, _p(out), out.stride(0), _zip_dt(X),
              _stream())


def zip_glo_modulate_bwd(dXm, X, SS, d_head, S, dX):
    """-> (dSS [R, 2 B] fp32, dxsum [R, B] fp32); writes dX = dXm * exp(scale) (+ d_head in its leading columns)."""
    B = SS.shape[1] // 2
    R = SS.shape[0]
    _chk2d("dXm X dX", dXm, X, dX, dt=X.dtype); _chk2d("SS", SS, dt=torch.float32)
    _require(all(t.shape[0] == R * S and t.shape[1] >= B for t in (dXm, X, dX)), "dXm, X, dX [R * S, >= B] for SS [R, 2 B]")
    nh = 0 if d_head is None else d_head.shape[1]
    if d_head is not None:
        _chk2d("d_head", d_head, dt=torch.float32)
        _require(d_head.shape[0] == R * S and nh <= B, "d_head [R * S, <= B]")
    dSS = torch.empty(R, 2 * B, dtype=torch.float32, device=X.device)
    dxsum = torch.empty(R, B, dtype=torch.float32, device=X.device)
    _lib.call("snerf_zip_glo_modulate_bwd", _p(dXm), dXm.stride(0), _p(X), X.stride(0), _p(SS), SS.stride(0), _p(d_head), 0 if d_head is None else d_head.stride(0),
              nh, R, S, B, _p(dX), dX.stride(0), _p(dSS), dSS.stride(0), _p(dxsum), dxsum.stride(0), _zip_dt(X), _stream())
    return dSS, dxsum


def zip_composite_fwd(raw_rgb, raw_density, tdist, dirs, opaque, bg, rgb_padding, density_bias):
    _dev("tdist dirs", tdist, dirs)
    R, P = tdist.shape
    dev = tdist.device
    rgb = torch.empty(R, 3, dtype=torch.float32, device=dev)
    depth, acc = torch.empty(R, dtype=torch.float32, device=dev), torch.empty(R, dtype=torch.float32, device=dev)
    w = torch.empty(R, P - 1, dtype=torch.float32, device=dev)
    _lib.call("snerf_zip_composite_fwd", _p(raw_rgb), 0 if raw_rgb is None else raw_rgb.stride(0), _p(raw_density), raw_density.stride(0),
              _p(tdist), _p(dirs), R, P - 1, 1 if opaque else 0, float(bg), float(rgb_padding), float(density_bias), _p(rgb), _p(depth), _p(acc),
              _p(w), _stream())
    return rgb, depth, acc, w


def zip_composite_bwd(raw_rgb, raw_density, tdist, dirs, opaque, bg, rgb_padding, density_bias, weights, acc, depth, g_rgb, g_depth, g_acc, g_w,
                      d_raw_rgb, d_raw_density, g_dirs=None):
    """`g_dirs` (optional fp32 [R,3], written): d loss / d directions through the interval lengths (t1 - t0) |d|."""
    R, P = tdist.shape
    _dev("g_rgb g_depth g_acc g_w weights acc depth g_dirs", g_rgb, g_depth, g_acc, g_w, weights, acc, depth, g_dirs, optional=True)
    _lib.call("snerf_zip_composite_bwd", _p(raw_rgb), 0 if raw_rgb is None else raw_rgb.stride(0), _p(raw_density), raw_density.stride(0),
              _p(tdist), _p(dirs), R, P - 1, 1 if opaque else 0, float(bg), float(rgb_padding), float(density_bias), _p(weights), _p(acc),
              _p(depth), _p(g_rgb), _p(g_depth), _p(g_acc), _p(g_w), _p(d_raw_rgb), 0 if d_raw_rgb is None else d_raw_rgb.stride(0),
              _p(d_raw_density), d_raw_density.stride(0), _p(g_dirs), _stream())


def zip_encode_ray_bwd(tdist, origins, directions, radii, base_x, base_y, deg_jitter, table, offsets, grid_sizes, grad_feat, L, C, n, m, Sl, H,
                       std_scale, g_o, g_d, g_bx, g_by):
    """Featurisation backward to the rays (cal_input_grad): accumulates d loss / d (origins, directions, base_x, base_y) [R,3]."""
    _dev("tdist origins directions radii base_x base_y deg_jitter g_o g_d g_bx g_by", tdist, origins, directions, radii, base_x, base_y, deg_jitter, g_o, g_d, g_bx, g_by, optional=True)
    R, P = tdist.shape
    _dev("table", table, dtype=_ZIP_DTS); _require(grad_feat.is_cuda and grad_feat.stride(1) == 1, "grad_feat: a row-major CUDA view")
    _lib.call("snerf_zip_encode_ray_bwd", _p(tdist), _p(origins), _p(directions), _p(radii), _p(base_x), _p(base_y), _p(deg_jitter), _p(table),
              _p(offsets), _p(grid_sizes), _p(grad_feat), grad_feat.stride(0), R, P - 1, L, C, n, m, float(Sl), int(H), float(std_scale),
              _zip_dt(table), _zip_dt(grad_feat), _p(g_o), _p(g_d), _p(g_bx), _p(g_by), _stream())


# ------------------------------------------------- callers ----
def pinhole_rays(coords, first_pixel, n, W, H, pose, cx, cy, fx, fy, training, near, far, device):
    """Rays of n pixels of a pinhole camera (coords int32 [n,2] = (row, col) on `device`, or None = pixels first_pixel.. row-major).
    `pose`: host [3,4] (or [4,4]) camera-to-world.  -> origins, directions, viewdirs [n,3], radii, near, far [n,1]."""
    import numpy as np
    p = np.ascontiguousarray(np.asarray(pose, dtype=np.float32)[:3, :4])
    if coords is not None:
        _dev("coords", coords, dtype=torch.int32, shape=(n, 2))
    o, d, v = (torch.empty(n, 3, dtype=torch.float32, device=device) for _ in range(3))
    r, nr, fr = (torch.empty(n, 1, dtype=torch.float32, device=device) for _ in range(3))
    _lib.call("snerf_pinhole_rays", _p(coords), int(first_pixel), int(W), int(H), p.ctypes.data, float(cx), float(cy), float(fx), float(fy),
              int(bool(training)), float(near), float(far), int(n), _p(o), _p(d), _p(v), _p(r), _p(nr), _p(fr), _stream())
    return o, d, v, r, nr, fr


def _host12(c2w):
    """[3,4] (or [4,4]) camera-to-world matrix -> contiguous host float32 [12] (one device->host copy per frame if it lives on the GPU)"""
    import numpy as np
    if c2w is None:
        return None
    a = c2w.detach().float().cpu().numpy() if torch.is_tensor(c2w) else np.asarray(c2w, dtype=np.float32)
    return np.ascontiguousarray(a[:3, :4], dtype=np.float32)


def classic_get_rays(H, W, focal, c2w, cx, cy, device):
    """get_rays (run_nerf_helpers.py:247-258) -> rays_o, rays_d [H,W,3] on `device`."""
    p = _host12(c2w)
    o = torch.empty(H, W, 3, dtype=torch.float32, device=device)
    d = torch.empty_like(o)
    _lib.call("snerf_classic_get_rays", int(H), int(W), float(focal), float(cx), float(cy), p.ctypes.data, _p(o), _p(d), _stream())
    return o, d


def classic_ndc_rays(H, W, focal, near, rays_o, rays_d):
    """ndc_rays (run_nerf_helpers.py:314-332) on [...,3] fp32 tensors."""
    o, d = rays_o.contiguous(), rays_d.contiguous()
    _dev("rays_o rays_d", o, d)
    oo, dd = torch.empty_like(o), torch.empty_like(d)
    _lib.call("snerf_classic_ndc_rays", int(H), int(W), float(focal), float(near), _p(o), _p(d), o.numel() // 3, _p(oo), _p(dd), _stream())
    return oo, dd


def classic_ray_batch(H, W, focal, cx, cy, c2w, c2w_static, rays_o, rays_d, n, ndc, near, far, depths, use_viewdirs, device):
    """The ray-batch assembly of render() (render.py:50-77) in one launch -> rows [n, 8 (+1) (+3)] fp32."""
    p, ps = _host12(c2w), _host12(c2w_static)
    ld = 8 + (1 if depths is not None else 0) + (3 if use_viewdirs else 0)
    rows = torch.empty(n, ld, dtype=torch.float32, device=device)
    if rays_o is not None:
        _dev("rays_o rays_d", rays_o, rays_d, shape=(n, 3))
    if depths is not None:
        _dev("depths", depths)
        _require(depths.numel() == n, "depths: one fp32 per ray")
    _lib.call("snerf_classic_ray_batch", int(H), int(W), float(focal), float(cx), float(cy), None if p is None else p.ctypes.data,
              None if ps is None else ps.ctypes.data, _p(rays_o), _p(rays_d), int(n), 1 if ndc else 0, float(near), float(far), _p(depths),
              1 if use_viewdirs else 0, _p(rows), ld, _stream())
    return rows


def ert_f2b_step(prev_raw_d, prev_base, s1, dirs, near, far, g0, G, next_g0, next_G, transform_idx, density_bias, eps_t, state, row_base):
    """One step of the front-to-back early ray termination (snerf_ert_f2b_step): fold the evaluated group [g0, g0 + G) into the rays'
    optical depth and assign the next group to the rays still above eps_t.  `state` = (tau, flags, counts, row_index, sample_id, total)
    from ert_f2b_state.  -> sample_id[:rows] of the next group (one device->host sync for the row count)."""
    tau, flags, counts, row_index, sample_id, total = state
    n, S1 = row_index.shape
    _lib.call("snerf_ert_f2b_step", _p(prev_raw_d), 0 if prev_raw_d is None else prev_raw_d.stride(0), int(prev_base), _p(s1), _p(dirs), _p(near), _p(far),
              n, S1, int(g0), int(G), int(next_g0), int(next_G), int(transform_idx), float(density_bias), float(eps_t), _p(tau), _p(flags), _p(counts),
              _p(row_index), _p(sample_id), int(row_base), _p(total), _stream())
    return sample_id[:int(total.item())]


def classic_ert_points(rays, z_all, alive, g0, G):
    """positions [n, G, 3] and view directions [n, 3] (None for 8-column ray rows) of the rows (alive[i], g0 + k): the next group of the
    classic path's front-to-back fine pass (snerf_classic_ert_points); alive None = every ray"""
    _chk2d("rays", rays, dt=torch.float32); _dev("z_all", z_all)
    N, S = z_all.shape
    n = N if alive is None else alive.numel()
    pts = torch.empty(n, G, 3, dtype=torch.float32, device=rays.device)
    vd = torch.empty(n, 3, dtype=torch.float32, device=rays.device) if rays.shape[1] > 9 else None
    _lib.call("snerf_classic_ert_points", _p(rays), rays.stride(0), _p(z_all), S, _p(alive), n, int(g0), int(G), _p(pts), _p(vd), rays.shape[1] - 3, _stream())
    return pts, vd


def classic_ert_step(raw_g, alive, z_all, rays, g0, G, eps_t, T, raw_full, scratch):
    """one step of that pass (snerf_classic_ert_step): scatter the evaluated group, update the transmittances, compact the survivors.
    `scratch` = (keep, offs, alive_next int32 [N], total int64 [1]).  -> alive_next[:count] (one device->host read of the count)"""
    N, S = z_all.shape
    n = N if alive is None else alive.numel()
    keep, offs, nxt, total = scratch
    _dev("raw_g raw_full", raw_g, raw_full)
    _require(raw_g.numel() == n * G * raw_full.shape[-1], "raw_g [n, G, channels] for raw_full [N, S, channels]")
    _lib.call("snerf_classic_ert_step", _p(raw_g), raw_full.shape[-1], _p(alive), n, _p(z_all), S, _p(rays), rays.stride(0), int(g0), int(G), float(eps_t),
              _p(T), _p(raw_full), _p(keep), _p(offs), _p(nxt), _p(total), _stream())
    return nxt[:int(total.item())].clone()


def ert_f2b_state(n, S1, group, device):
    return (torch.zeros(n, dtype=torch.float32, device=device), torch.empty(n, dtype=torch.int32, device=device),
            torch.empty(n, dtype=torch.int32, device=device), torch.full((n, S1), -1, dtype=torch.int32, device=device),
            torch.empty(n * group, dtype=torch.int32, device=device), torch.zeros(1, dtype=torch.int64, device=device))


def mip_loss_tail(rgb, tgt, dist1, dist0, tdepth, conf, s_f, w_f, s_c, w_c, disparity, depth_lambda, coarse_mult, prop_lambda):
    """-> (out[5] = {#valid, rgb, depth, proposal loss, total}, g_rgb, g_dist1, g_dist0, g_wc); absent terms return None gradients."""
    n = rgb.shape[0]
    dev = rgb.device
    out = torch.empty(5, dtype=torch.float32, device=dev)
    g_rgb = torch.empty(n, 3, dtype=torch.float32, device=dev)
    g1 = g0 = gw = None
    if tdepth is not None:
        g1, g0 = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
    Pf = Sc = 0
    if s_c is not None:
        Pf, Sc = s_f.shape[1], w_c.shape[1]
        _require(w_f.shape[1] == Pf - 1 and s_c.shape[1] == Sc + 1, "s_f [n, Pf], w_f [n, Pf - 1], s_c [n, Sc + 1], w_c [n, Sc]")
        gw = torch.empty(n, Sc, dtype=torch.float32, device=dev)
    _dev("rgb tgt dist1 dist0 tdepth conf s_f w_f s_c w_c", rgb, tgt, dist1, dist0, tdepth, conf, s_f, w_f, s_c, w_c, optional=True)
    _lib.call("snerf_mip_loss_tail", _p(rgb), _p(tgt), _p(dist1), _p(dist0), _p(tdepth), _p(conf), _p(s_f), _p(w_f),
              _p(s_c), _p(w_c), n, Pf, Sc, int(bool(disparity)), float(depth_lambda), float(coarse_mult), float(prop_lambda), _p(out),
              _p(g_rgb), _p(g1), _p(g0), _p(gw), _stream())
    return out, g_rgb, g1, g0, gw


def classic_loss_tail_ws(n):
    """bytes of scratch classic_loss_tail needs for n rays (snerf_classic_loss_tail_ws)"""
    return int(_lib.query("snerf_classic_loss_tail_ws", int(n)))


def classic_loss_tail(rgb, rgb0, tgt, ws=None, out=None, g_rgb=None, g_rgb0=None):
    """snerf_classic_loss_tail: the stock loss of the classic training loop, img2mse(rgb, tgt) + img2mse(rgb0, tgt) (rgb0 None: the
    one-level render) and mse2psnr, with d loss / d rgb and d loss / d rgb0 -> (out[4] = {loss, img_loss, img_loss0, psnr}, g_rgb,
    g_rgb0 or None).  fp32 [n,3] contiguous; double sums in a fixed order, no atomics.  ws: uint8 / fp64 scratch of >=
    classic_loss_tail_ws(n) bytes (allocated when None); out / g_rgb / g_rgb0: preallocated results (allocated when None)."""
    _dev("rgb tgt", rgb, tgt); _dev("rgb0 out g_rgb g_rgb0", rgb0, out, g_rgb, g_rgb0, optional=True)
    _require(rgb.dim() == 2 and rgb.shape[1] == 3 and rgb.shape[0] > 0 and tgt.shape == rgb.shape and (rgb0 is None or rgb0.shape == rgb.shape),
             "rgb / rgb0 / tgt: fp32 [n, 3] with n >= 1")
    n, dev = rgb.shape[0], rgb.device
    need = classic_loss_tail_ws(n)
    ws = torch.empty(need // 8, dtype=torch.float64, device=dev) if ws is None else _ws_given(ws, None, "ws: >= classic_loss_tail_ws(n) bytes of device scratch", need)
    out = torch.empty(4, dtype=torch.float32, device=dev) if out is None else out
    g_rgb = torch.empty_like(rgb) if g_rgb is None else g_rgb
    if rgb0 is None:
        _require(g_rgb0 is None, "g_rgb0 goes with rgb0")
    elif g_rgb0 is None:
        g_rgb0 = torch.empty_like(rgb0)
    _require(out.numel() == 4 and g_rgb.shape == rgb.shape and (g_rgb0 is None or g_rgb0.shape == rgb.shape), "out fp32 [4]; g_rgb, g_rgb0 like rgb")
    _lib.call("snerf_classic_loss_tail", _p(rgb), _p(rgb0), _p(tgt), n, _p(ws), _p(out), _p(g_rgb), _p(g_rgb0), _stream())
    return out, g_rgb, g_rgb0


def mip_loss_tail_masked(rgb, tgt, dist1, dist0, tdepth, conf, s_f, w_f, s_c, w_c, disparity, depth_lambda, coarse_mult, prop_lambda,
                         sem=None, labels=None, semantic_lambda=0.1, rows=None, img_i=None, rgb_row_limit=None, depth_row_limit=None,
                         sem_valid=None, depth_keep=None, want_g_conf=False):
    """snerf_mip_loss_tail_masked: mip_loss_tail with the per-image rules of s-nerf/train.py:131-209 (each new argument None = absent).
    want_g_conf (needs tdepth): snerf_mip_loss_tail_gconf -- the same outputs, bit for bit, followed by g_conf [n] = d total / d conf,
    the input of conf_grad.
    sem [n,C] fp32 composited logits + labels [n] (int32, or fp32 holding exact integers -- a batcher's extras row; -100 = ignored, and
    so is any other label outside [0, C): the reference raises on one); rows = the batcher's sel_coords (int64 [n,2]), img_i int64 [1]
    device tensor (read by the kernel, never on the host) and the three int32 per-image tables (trainer.MipLossRules): all or none;
    depth_keep [n] fp32: a ray counts for the depth term only where it is 0.  A term whose count is 0 is 0 with zero gradients.
    -> (out[8] = {#depth rays, rgb, depth, proposal, total, semantic, #rgb rays, #semantic rays}, g_rgb, g_dist1, g_dist0, g_wc, g_sem);
    absent terms return None gradients."""
    n = rgb.shape[0]
    dev = rgb.device
    out = torch.empty(8, dtype=torch.float32, device=dev)
    g_rgb = torch.empty(n, 3, dtype=torch.float32, device=dev)
    g1 = g0 = gw = gs = None
    if tdepth is not None:
        g1, g0 = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
    Pf = Sc = C = lab_f32 = 0
    if s_c is not None:
        Pf, Sc = s_f.shape[1], w_c.shape[1]
        _require(w_f.shape[1] == Pf - 1 and s_c.shape[1] == Sc + 1, "s_f [n, Pf], w_f [n, Pf - 1], s_c [n, Sc + 1], w_c [n, Sc]")
        gw = torch.empty(n, Sc, dtype=torch.float32, device=dev)
    _dev("rgb tgt dist1 dist0 tdepth conf s_f w_f s_c w_c sem depth_keep", rgb, tgt, dist1, dist0, tdepth, conf, s_f, w_f, s_c, w_c, sem, depth_keep,
         optional=True)
    if sem is not None:
        C = sem.shape[1]
        _dev("labels", labels, dtype=(torch.int32, torch.float32))
        _require(labels.numel() == n, "labels: int32 / fp32 [n]")
        lab_f32 = 1 if labels.dtype == torch.float32 else 0
        gs = torch.empty(n, C, dtype=torch.float32, device=dev)
    n_img = 0
    if rows is not None:
        _dev("rows", rows, dtype=torch.int64, shape=(n, 2), msg="rows: the batcher's sel_coords, int64 [n, 2]")
        _require(torch.is_tensor(img_i) and img_i.is_cuda and img_i.dtype == torch.int64 and img_i.numel() == 1, "img_i: an int64 [1] CUDA tensor")
        _dev("rgb_row_limit depth_row_limit sem_valid", rgb_row_limit, depth_row_limit, sem_valid, dtype=torch.int32)
        n_img = rgb_row_limit.numel()
        _require(depth_row_limit.numel() == n_img == sem_valid.numel(), "rgb_row_limit, depth_row_limit, sem_valid: int32 [n_images]")
    args = (_p(rgb), _p(tgt), _p(dist1), _p(dist0), _p(tdepth), _p(conf), _p(s_f), _p(w_f),
            _p(s_c), _p(w_c), _p(sem), _p(labels), lab_f32, C, _p(rows), _p(img_i), _p(rgb_row_limit), _p(depth_row_limit), _p(sem_valid),
            n_img, _p(depth_keep), n, Pf, Sc, int(bool(disparity)), float(depth_lambda), float(coarse_mult), float(prop_lambda),
            float(semantic_lambda), _p(out), _p(g_rgb), _p(g1), _p(g0), _p(gw), _p(gs))
    if want_g_conf:
        _require(tdepth is not None, "g_conf is a by-product of the depth term: tdepth is needed")
        gc = torch.empty(n, dtype=torch.float32, device=dev)
        _lib.call("snerf_mip_loss_tail_gconf", *args, _p(gc), _stream())
        return out, g_rgb, g1, g0, gw, gs, gc
    _lib.call("snerf_mip_loss_tail_masked", *args, _stream())
    return out, g_rgb, g1, g0, gw, gs


def zip_pixels_to_rays(pix_x, pix_y, cam_idx, pixtocams, camtoworlds, want_imageplane=False):
    """camera_utils.pixels_to_rays on device: int32 pixel coordinates [n] (+ int32 camera index [n] or None) and the stacked
    [ncam,3,3] inverse intrinsics / [ncam,3,4] extrinsics -> dict(origins, directions, viewdirs, radii [n,1], base_x, base_y
    (, imageplane))."""
    n, dev = pix_x.shape[0], pix_x.device
    _dev("pix_x pix_y cam_idx", pix_x, pix_y, cam_idx, dtype=torch.int32, shape=(n,), optional=True)
    k, c = pixtocams.contiguous(), camtoworlds.contiguous()   # (torch.linalg.inv returns column-major)
    k = _dev("pixtocams camtoworlds", k, c).reshape(-1, 3, 3)
    _require(c.shape[1:] == (3, 4) and c.shape[0] == k.shape[0], "pixtocams [ncam,3,3], camtoworlds [ncam,3,4]")
    o, d, v, bx, by = (torch.empty(n, 3, dtype=torch.float32, device=dev) for _ in range(5))
    r = torch.empty(n, 1, dtype=torch.float32, device=dev)
    ip = torch.empty(n, 2, dtype=torch.float32, device=dev) if want_imageplane else None
    _lib.call("snerf_zip_pixels_to_rays", _p(pix_x), _p(pix_y), _p(cam_idx), _p(k), _p(c), k.shape[0], n, _p(o), _p(d), _p(v), _p(r), _p(ip),
              _p(bx), _p(by), _stream())
    out = dict(origins=o, directions=d, viewdirs=v, radii=r, base_x=bx, base_y=by)
    if ip is not None:
        out["imageplane"] = ip
    return out


_U8_F32 = (torch.uint8, torch.float32)             # the image dtypes; the entries take `u8` = 1 for the first


def mip_image_batch(images, depths, poses, intrinsics, near, far, app, extras, i_train, seed, counter, n, i0, i1, out):
    """snerf_mip_image_batch: rows [i0, i1) of step counter[0]'s global batch of n pixels into the preallocated `out` (dict: origins,
    directions, viewdirs [m,3], radii, lossmult, near, far, app [m,1], rgb [m,3], depth [m] or None, extras [k,m] or None,
    sel_coords int64 [m,2], img int64 [1]; m = i1 - i0); advances counter[0].  images [N,H,W,3] uint8 / fp32, depths [N,H,W],
    poses [N,3,4], intrinsics [N,4] = (cx, cy, fx, fy), near / far / app [N], extras [k,N,H,W] or None, i_train int32."""
    u8 = 1 if _dev("images", images, dtype=_U8_F32).dtype == torch.uint8 else 0
    N, H, W = images.shape[:3]
    _dev("depths poses intrinsics near far app extras", depths, poses, intrinsics, near, far, app, extras, optional=True)
    _dev("i_train", i_train, dtype=torch.int32); _dev("counter", counter, dtype=torch.int64)
    _require(counter.numel() == 2, "counter: int64 [2]")
    k = 0 if extras is None else extras.shape[0]
    _lib.call("snerf_mip_image_batch", _p(images), u8, _p(depths), _p(poses), _p(intrinsics), _p(near), _p(far), _p(app), _p(extras), k,
              _p(i_train), i_train.numel(), N, H, W, int(seed), _p(counter), int(n), int(i0), int(i1), _p(out["origins"]),
              _p(out["directions"]), _p(out["viewdirs"]), _p(out["radii"]), _p(out["lossmult"]), _p(out["near"]), _p(out["far"]),
              _p(out["app"]), _p(out["rgb"]), _p(out.get("depth")), _p(out.get("extras")), _p(out["sel_coords"]), _p(out["img"]), _stream())
    return out


def mip_image_patch_batch(images, depths, poses, intrinsics, near, far, app, extras, i_train, seed, counter, n, i0, i1, n_patch, patch_sz, k0,
                          k1, out):
    """snerf_mip_image_patch_batch: mip_image_batch's rows [i0, i1) followed by patches [k0, k1) of the step's n_patch depth patches of
    patch_sz^2 pixels (--smooth_loss) into `out` (as for mip_image_batch, with m = (i1 - i0) + (k1 - k0) patch_sz^2 rows); one launch,
    advances counter[0].  n_patch = 0 is mip_image_batch."""
    u8 = 1 if _dev("images", images, dtype=_U8_F32).dtype == torch.uint8 else 0
    N, H, W = images.shape[:3]
    _dev("depths poses intrinsics near far app extras", depths, poses, intrinsics, near, far, app, extras, optional=True)
    _dev("i_train", i_train, dtype=torch.int32); _dev("counter", counter, dtype=torch.int64)
    _require(counter.numel() == 2, "counter: int64 [2]")
    m = (int(i1) - int(i0)) + (int(k1) - int(k0)) * int(patch_sz) ** 2
    _require(out["rgb"].shape[0] == m and out["sel_coords"].shape[0] == m and (out.get("extras") is None or out["extras"].shape[1] == m),
             "out: (i1 - i0) + (k1 - k0) patch_sz^2 rows")
    k = 0 if extras is None else extras.shape[0]
    _lib.call("snerf_mip_image_patch_batch", _p(images), u8, _p(depths), _p(poses), _p(intrinsics), _p(near), _p(far), _p(app), _p(extras), k,
              _p(i_train), i_train.numel(), N, H, W, int(seed), _p(counter), int(n), int(i0), int(i1), _p(out["origins"]),
              _p(out["directions"]), _p(out["viewdirs"]), _p(out["radii"]), _p(out["lossmult"]), _p(out["near"]), _p(out["far"]),
              _p(out["app"]), _p(out["rgb"]), _p(out.get("depth")), _p(out.get("extras")), _p(out["sel_coords"]), _p(out["img"]),
              int(n_patch), int(patch_sz), int(k0), int(k1), _stream())
    return out


def classic_train_batch(images, c2w, intrinsics, i_train, seed, counter, n, i0, i1, ndc, near, far, use_viewdirs, rows, rgb):
    """snerf_classic_train_batch: rows [i0, i1) of step counter[0]'s global batch of n rays of the classic training loop (every ray of
    the training images in a shuffled order, n per step) into the preallocated `rows` [i1 - i0, 8 | 11] = [o3, d3, near, far, (viewdir3)]
    and `rgb` [i1 - i0, 3]; one launch, advances counter[0].  images [N,H,W,3] uint8 / fp32, c2w fp32 [N,3,4], intrinsics fp64 [N,3] =
    (focal, cx, cy), i_train int32 with entries in [0, N)."""
    u8 = 1 if _dev("images", images, dtype=_U8_F32).dtype == torch.uint8 else 0
    _require(images.dim() == 4 and images.shape[3] == 3, "images: [N, H, W, 3]")
    N, H, W = images.shape[:3]
    _dev("c2w", c2w, shape=(N, 3, 4), msg="c2w: fp32 [N, 3, 4]"); _dev("rows rgb", rows, rgb)
    _dev("intrinsics", intrinsics, dtype=torch.float64, shape=(N, 3), msg="intrinsics: fp64 [N, 3] = (focal, cx, cy)")
    _dev("i_train", i_train, dtype=torch.int32); _dev("counter", counter, dtype=torch.int64)
    _require(i_train.numel() >= 1 and counter.numel() == 2, "i_train: int32 [>= 1]; counter: int64 [2]")
    m, ld = int(i1) - int(i0), 11 if use_viewdirs else 8
    _require(0 <= int(i0) <= int(i1) <= int(n) and tuple(rows.shape) == (m, ld) and tuple(rgb.shape) == (m, 3), "rows [i1 - i0, 8 | 11], rgb [i1 - i0, 3]")
    _lib.call("snerf_classic_train_batch", _p(images), u8, _p(c2w), _p(intrinsics), _p(i_train), i_train.numel(), N, H, W, int(seed), _p(counter),
              int(n), int(i0), int(i1), 1 if ndc else 0, float(near), float(far), 1 if use_viewdirs else 0, _p(rows), ld, _p(rgb), _stream())
    return rows, rgb


def smooth_loss_ws(P):
    """doubles of scratch smooth_loss needs for P patches (snerf_smooth_loss_ws)"""
    return int(_lib.query("snerf_smooth_loss_ws", int(P)))


def smooth_loss(rgb, dist, sky, P, p, weight, out=None, total=None, g_dist=None, accumulate=False, ws=None):
    """snerf_smooth_loss: the edge-aware smoothness (SmoothLoss over edge_aware_loss_v2) of P patches of p x p rays, value and gradient in
    one pass.  rgb [P p p, 3] target colours, dist [P p p] renderer distances, sky [P p p] or None (fp32, any shape of that size) ->
    (out[3] = {weight * (x mean + y mean), x mean, y mean}, g_dist [P p p] = d loss / d dist).  total: a device float the loss is
    added into; g_dist given: stored into (accumulate=False) or added into (True).  Deterministic (float64 sums in a fixed order, no
    atomics).  ws: fp64 scratch of >= smooth_loss_ws(P) elements (allocated when None).  P = 0 launches nothing."""
    P, p = int(P), int(p)
    dev = dist.device
    _dev("rgb dist sky total g_dist out", rgb, dist, sky, total, g_dist, out, optional=True)
    _require(rgb.numel() == 3 * P * p * p and dist.numel() == P * p * p and (sky is None or sky.numel() == P * p * p), "rgb [P,p,p,3], dist / sky [P,p,p]")
    if out is None:
        out = torch.zeros(3, dtype=torch.float32, device=dev)
    if g_dist is None:
        _require(not accumulate, "accumulate=True adds into a given g_dist")
        g_dist = torch.empty(P * p * p, dtype=torch.float32, device=dev)
    _require(out.numel() == 3 and g_dist.numel() == P * p * p and (total is None or total.numel() == 1), "out fp32 [3], g_dist fp32 [P p p], total fp32 [1]")
    ws = _ws(ws, lambda: max(smooth_loss_ws(P), 1), torch.float64, dev, "ws: a contiguous fp64 CUDA tensor of >= smooth_loss_ws(P) elements")
    _lib.call("snerf_smooth_loss", _p(rgb), _p(dist), _p(sky), P, p, float(weight), _p(ws), ws.numel(), _p(out), _p(total), _p(g_dist),
              int(bool(accumulate)), _stream())
    return out, g_dist


def _cam_args(cam, name="cam"):
    """camera index of the pose entries -> (device pointer or None, host index): an int64 [1] device tensor (a batcher's `img`) is read
    by the kernel, anything else is a python int"""
    if torch.is_tensor(cam):
        _require(cam.is_cuda and cam.dtype == torch.int64 and cam.numel() == 1, "%s: camera index: a python int or an int64 [1] CUDA tensor", name)
        return _p(cam), 0
    return None, int(cam)


def pose_apply(r, t, cam, origins, directions, viewdirs, pose_out=None):
    """snerf_pose_apply: the pose branch of sample_rays on row `cam` of the LearnPose table r [n_cams,3] / t [n_cams,3] (None = no
    translation) -> new (origins + t, R directions, R viewdirs); the inputs are left as they are (pose_grad needs them).  `cam`: a python
    int, or an int64 [1] device tensor that the kernel reads (no host sync).  pose_out: fp32 [3,4], receives the applied transform."""
    _dev("r", r, shape=(None, 3)); _dev("t", t, shape=tuple(r.shape), optional=True)
    n = origins.shape[0]
    _dev("origins directions viewdirs", origins, directions, viewdirs, shape=(n, 3)); _dev("pose_out", pose_out, optional=True)
    _require(pose_out is None or pose_out.numel() == 12, "pose_out: fp32 [3,4]")
    o2, d2, v2 = torch.empty_like(origins), torch.empty_like(directions), torch.empty_like(viewdirs)
    cam_dev, cam_host = _cam_args(cam)
    _lib.call("snerf_pose_apply", _p(r), _p(t), r.shape[0], cam_dev, cam_host, _p(origins), _p(directions), _p(viewdirs), n, _p(o2), _p(d2),
              _p(v2), _p(pose_out), _stream())
    return o2, d2, v2


def pose_grad_ws(n):
    """doubles of scratch pose_grad needs for n rays (snerf_pose_grad_ws)"""
    return int(_lib.query("snerf_pose_grad_ws", int(n)))


def pose_grad(r, cam, g_o, g_d, g_v, directions, viewdirs, grad_r, grad_t=None, ws=None):
    """snerf_pose_grad: d loss / d (transformed origins, directions, viewdirs) [n,3] and the UNtransformed directions / viewdirs reduced
    to the gradient of table row `cam`, ADDED into grad_r [n_cams,3] (and grad_t, when the translation is trained; either may be None).
    Deterministic (double sums in a fixed order, no atomics).  ws: fp64 scratch of >= pose_grad_ws(n) elements (allocated when None)."""
    _dev("r", r, shape=(None, 3)); _dev("grad_r grad_t", grad_r, grad_t, shape=tuple(r.shape), optional=True)
    n = g_d.shape[0]
    _dev("g_o g_d g_v directions viewdirs", g_o, g_d, g_v, directions, viewdirs, shape=(n, 3), optional=True)
    ws = _ws(ws, lambda: pose_grad_ws(n), torch.float64, r.device, "ws: a contiguous fp64 CUDA tensor of >= pose_grad_ws(n) elements")
    cam_dev, cam_host = _cam_args(cam)
    _lib.call("snerf_pose_grad", _p(r), r.shape[0], cam_dev, cam_host, _p(g_o), _p(g_d), _p(g_v), _p(directions), _p(viewdirs), n, _p(ws),
              ws.numel(), _p(grad_r), _p(grad_t), _stream())


def pose_compose_apply(r, t, cam, origins, directions, viewdirs, pose_out=None):
    """snerf_pose_compose_apply: row `cam` of the LearnPose table composed with the initial pose (eval.py:88-89, make_c2w(r, t) @
    init_c2w[img]) on the rays of the INITIAL pose -> new (R origins + t, R directions, R viewdirs); t None = no translation.  Arguments
    as pose_apply; the inputs are left as they are (pose_compose_grad needs all three)."""
    _dev("r", r, shape=(None, 3)); _dev("t", t, shape=tuple(r.shape), optional=True)
    n = origins.shape[0]
    _dev("origins directions viewdirs", origins, directions, viewdirs, shape=(n, 3)); _dev("pose_out", pose_out, optional=True)
    _require(pose_out is None or pose_out.numel() == 12, "pose_out: fp32 [3,4]")
    o2, d2, v2 = torch.empty_like(origins), torch.empty_like(directions), torch.empty_like(viewdirs)
    cam_dev, cam_host = _cam_args(cam)
    _lib.call("snerf_pose_compose_apply", _p(r), _p(t), r.shape[0], cam_dev, cam_host, _p(origins), _p(directions), _p(viewdirs), n, _p(o2),
              _p(d2), _p(v2), _p(pose_out), _stream())
    return o2, d2, v2


def pose_compose_grad(r, cam, g_o, g_d, g_v, origins, directions, viewdirs, grad_r, grad_t=None, ws=None):
    """snerf_pose_compose_grad: pose_grad for rays moved by pose_compose_apply -- the UNtransformed origins join the reduction (the
    rotation's gradient gains sum g_o o^T), so g_o is needed with or without grad_t.  ws: fp64 scratch of >= pose_grad_ws(n) elements."""
    _dev("r", r, shape=(None, 3)); _dev("grad_r grad_t", grad_r, grad_t, shape=tuple(r.shape), optional=True)
    n = g_d.shape[0]
    _dev("g_o g_d g_v origins directions viewdirs", g_o, g_d, g_v, origins, directions, viewdirs, shape=(n, 3))
    ws = _ws(ws, lambda: pose_grad_ws(n), torch.float64, r.device, "ws: a contiguous fp64 CUDA tensor of >= pose_grad_ws(n) elements")
    cam_dev, cam_host = _cam_args(cam)
    _lib.call("snerf_pose_compose_grad", _p(r), r.shape[0], cam_dev, cam_host, _p(g_o), _p(g_d), _p(g_v), _p(origins), _p(directions),
              _p(viewdirs), n, _p(ws), ws.numel(), _p(grad_r), _p(grad_t), _stream())


def pose_table(r, t, t_ratio=1.0, out=None):
    """snerf_pose_table: the LearnPoseV2 table r [n_cams,3] / t [n_cams,3] (None = no translation) -> fp32 [n_cams,3,4], row c =
    [R(r_c) | t_c * t_ratio] (posenet_v2.py:89,99), the rotation formed in double and rounded once."""
    _dev("r", r, shape=(None, 3)); _dev("t", t, shape=tuple(r.shape), optional=True)
    if out is None:
        out = torch.empty(r.shape[0], 3, 4, dtype=torch.float32, device=r.device)
    _dev("out", out, shape=(r.shape[0], 3, 4))
    _lib.call("snerf_pose_table", _p(r), _p(t), r.shape[0], float(t_ratio), _p(out), _stream())
    return out


def pose_rays_apply(table, cam, origins, directions, viewdirs, base_x, base_y):
    """snerf_pose_rays_apply: every ray moved by its own row of `table` (pose_table's) -- zipnerf/train.py:186-196.  cam fp32 [n]: the
    rays' rows, truncated toward zero like the reference's .int(); a ray whose row is outside the table passes through unchanged.
    -> new (origins + t, R directions, R viewdirs, R base_x, R base_y); the inputs are left as they are (pose_rays_grad needs them)."""
    rays = (origins, directions, viewdirs, base_x, base_y)
    n = origins.shape[0]
    _dev("table", table, shape=(None, 3, 4)); _dev("cam", cam); _dev("origins directions viewdirs base_x base_y", *rays, shape=(n, 3))
    _require(cam.numel() == n, "cam: fp32 [n], the rays' table rows")
    outs = tuple(torch.empty_like(x) for x in rays)
    _lib.call("snerf_pose_rays_apply", _p(table), table.shape[0], _p(cam), *[_p(x) for x in rays], n, *[_p(x) for x in outs], _stream())
    return outs


def pose_rays_grad_ws(n, n_cams):
    """doubles of scratch pose_rays_grad needs for n rays over n_cams table rows (snerf_pose_rays_grad_ws)"""
    return int(_lib.query("snerf_pose_rays_grad_ws", int(n), int(n_cams)))


def pose_rays_grad(r, t_ratio, cam, g_o, g_d, g_v, g_bx, g_by, directions, viewdirs, base_x, base_y, grad_r, grad_t=None, ws=None):
    """snerf_pose_rays_grad: d loss / d (the moved origins, directions, viewdirs, base_x, base_y) [n,3] and the UNmoved directions /
    viewdirs / base_x / base_y reduced camera by camera (cam fp32 [n], as pose_rays_apply) to the gradient of the table rows that own a
    ray, ADDED into grad_r [n_cams,3] (and grad_t, which takes t_ratio * sum g_o; either may be None, g_o too without grad_t); rows without
    a ray are not written.  Deterministic (double sums in a fixed order, no atomics).  ws: fp64 scratch of >= pose_rays_grad_ws(n,
    n_cams) elements (allocated when None)."""
    rays = (g_d, g_v, g_bx, g_by, directions, viewdirs, base_x, base_y)
    n = g_d.shape[0]
    _dev("r", r, shape=(None, 3)); _dev("grad_r grad_t", grad_r, grad_t, shape=tuple(r.shape), optional=True); _dev("cam", cam)
    _dev("g_d g_v g_bx g_by directions viewdirs base_x base_y", *rays, shape=(n, 3)); _dev("g_o", g_o, shape=(n, 3), optional=True)
    _require(cam.numel() == n, "cam: fp32 [n], the rays' table rows")
    ws = _ws(ws, lambda: pose_rays_grad_ws(n, r.shape[0]), torch.float64, r.device,
             "ws: a contiguous fp64 CUDA tensor of >= pose_rays_grad_ws(n, n_cams) elements")
    _lib.call("snerf_pose_rays_grad", _p(r), r.shape[0], float(t_ratio), _p(cam), _p(g_o), *[_p(x) for x in rays], n, _p(ws), ws.numel(),
              _p(grad_r), _p(grad_t), _stream())


def _conf_args(maps, slot_of_image, lambdas, sky, img, coords):
    """checks and the leading arguments shared by snerf_conf_apply / snerf_conf_grad"""
    _dev("maps lambdas", maps, lambdas)
    _require(maps.dim() == 4 and lambdas.dim() == 2 and lambdas.shape[0] == maps.shape[0], "maps [M,P,H,W] and lambdas [M,n_images]")
    M, P, H, W = maps.shape
    n_img = lambdas.shape[1]
    _dev("slot_of_image", slot_of_image, dtype=torch.int32)
    _require(slot_of_image.numel() == n_img, "slot_of_image: int32 [n_images]")
    _dev("sky", sky, dtype=torch.uint8, shape=(n_img, H, W), optional=True, msg="sky: uint8 [n_images,H,W]")
    _dev("coords", coords, dtype=torch.int64, shape=(None, 2), msg="coords: the batcher's sel_coords, int64 [n, 2]")
    img_dev, img_host = _cam_args(img, "img")
    return (_p(maps), M, P, H, W, _p(slot_of_image), _p(lambdas), n_img, _p(sky), img_dev, img_host, _p(coords)), coords.shape[0]


def conf_apply(maps, slot_of_image, lambdas, sky, img, coords):
    """snerf_conf_apply: the learned confidence of the rays at pixels coords (int64 [n,2] = (row, col)) of image `img` (a python int, or
    an int64 [1] device tensor that the kernel reads: no host sync) -> conf [n] = sum_k sigmoid(lambdas[k,img]) maps[k,slot,row,col] /
    sum_k sigmoid(lambdas[k,img]), 1 on sky pixels (sky uint8 [n_images,H,W] or None) and for an image without maps.
    maps fp32 [M,P,H,W], slot_of_image int32 [n_images], lambdas fp32 [M,n_images] (confidence.ConfidenceMaps / Confidence)."""
    head, n = _conf_args(maps, slot_of_image, lambdas, sky, img, coords)
    conf = torch.empty(n, dtype=torch.float32, device=maps.device)
    _lib.call("snerf_conf_apply", *head, n, _p(conf), _stream())
    return conf


def conf_grad_ws(n):
    """doubles of scratch conf_grad needs for n rays (snerf_conf_grad_ws)"""
    return int(_lib.query("snerf_conf_grad_ws", int(n)))


def conf_grad(maps, slot_of_image, lambdas, sky, img, coords, g_conf, grad_lambdas, ws=None):
    """snerf_conf_grad: g_conf [n] = d loss / d conf reduced to the gradient of column `img` of lambdas, ADDED into grad_lambdas
    [M,n_images].  Deterministic (double sums in a fixed order, no atomics).  ws: fp64 scratch of >= conf_grad_ws(n) elements
    (allocated when None)."""
    head, n = _conf_args(maps, slot_of_image, lambdas, sky, img, coords)
    _dev("g_conf", g_conf); _dev("grad_lambdas", grad_lambdas, shape=tuple(lambdas.shape))
    _require(g_conf.numel() == n, "g_conf: fp32 [n]")
    ws = _ws(ws, lambda: conf_grad_ws(n), torch.float64, maps.device, "ws: a contiguous fp64 CUDA tensor of >= conf_grad_ws(n) elements")
    _lib.call("snerf_conf_grad", *head, _p(g_conf), n, _p(ws), ws.numel(), _p(grad_lambdas), _stream())


REPROJ_MODES = ("rgb", "ssim", "depth")                # bit k of snerf_reproj_conf's `modes`


def reproj_conf_ws(H, W):
    """bytes of scratch reproj_conf needs for H x W images (snerf_reproj_conf_ws)"""
    return int(_lib.query("snerf_reproj_conf_ws", int(H), int(W)))


def reproj_conf(images, depths, poses, intrinsics, base, neighbours, modes, tau, out=None, ws=None):
    """snerf_reproj_conf: the reprojection confidence maps of image `base` against `neighbours` (python ints, in the reference's sel_ids
    order: the last one decides the depth-mask zeroing) -> fp32 [len(modes), H, W] in the order of `modes` (names out of rgb / ssim /
    depth).  images [N,H,W,3] uint8 / fp32 in [0,1], depths [N,H,W], poses [N,3,4], intrinsics [N,4] = (cx, cy, fx, fy), all resident
    (an ImageRayBatcher's tensors as they are).  No host read or sync; graph-capturable when `out` and `ws` (uint8, >= reproj_conf_ws(H, W)
    elements) are preallocated."""
    u8 = 1 if _dev("images", images, dtype=_U8_F32).dtype == torch.uint8 else 0
    N, H, W = images.shape[:3]
    _dev("depths poses intrinsics", depths, poses, intrinsics)
    _require(images.dim() == 4 and images.shape[3] == 3 and tuple(depths.shape) == (N, H, W) and tuple(poses.shape) == (N, 3, 4) and
             tuple(intrinsics.shape) == (N, 4), "images [N,H,W,3], depths [N,H,W], poses [N,3,4], intrinsics [N,4]")
    modes = list(modes)
    _require(modes and len(set(modes)) == len(modes) and all(m in REPROJ_MODES for m in modes), "modes: distinct names out of %s", REPROJ_MODES)
    if out is None:
        out = torch.empty(len(modes), H, W, dtype=torch.float32, device=images.device)
    _dev("out", out, shape=(len(modes), H, W))
    need = reproj_conf_ws(H, W)
    ws = _ws(ws, need, torch.uint8, images.device, "ws: a contiguous uint8 CUDA tensor of >= reproj_conf_ws(H, W) elements", need)
    planes = [_p(out[modes.index(m)]) if m in modes else None for m in REPROJ_MODES]
    nb = (ctypes.c_int * max(len(neighbours), 1))(*[int(i) for i in neighbours])
    _lib.call("snerf_reproj_conf", _p(images), u8, _p(depths), _p(poses), _p(intrinsics), N, H, W, int(base), nb, len(neighbours),
              sum(1 << REPROJ_MODES.index(m) for m in modes), float(tau), _p(ws), ws.numel(), *planes, _stream())
    return out


FRAME_METRIC_NAMES = ("mse_f", "psnr_f", "mse_u8", "psnr_u8", "ssim")      # the columns of snerf_frame_metrics' out


def frame_metrics_ws(F, H, W):
    """bytes of scratch frame_metrics needs for F frames of H x W (snerf_frame_metrics_ws; 0 where the call would be refused)"""
    return int(_lib.query("snerf_frame_metrics_ws", int(F), int(H), int(W)))


def frame_metrics(pred, gt, gray_w=None, out=None, ws=None):
    """snerf_frame_metrics: pred [H,W,3] or [F,H,W,3] fp32 against gt of the same shape, fp32 or uint8 -> float64 [F,5] on the device in
    the order of FRAME_METRIC_NAMES (float MSE / PSNR of eval.py, uint8 MSE / PSNR and grey SSIM of image.MetricHarness).  gray_w:
    (wr, wg, wb, shift) python ints, None = the library's default (OpenCV 4's RGB2GRAY).  No host read or sync; graph-capturable when
    `out` (float64 [F,5]) and `ws` (uint8, >= frame_metrics_ws(F, H, W) elements) are preallocated."""
    _dev("pred", pred)
    u8 = 1 if _dev("gt", gt, dtype=_U8_F32).dtype == torch.uint8 else 0
    _require(pred.dim() in (3, 4) and pred.shape[-1] == 3 and gt.shape == pred.shape, "pred [H,W,3] or [F,H,W,3] fp32, gt of the same shape")
    F = 1 if pred.dim() == 3 else pred.shape[0]
    H, W = pred.shape[-3], pred.shape[-2]
    need = frame_metrics_ws(F, H, W)
    _require(need > 0, "frame_metrics: 1 <= F <= 65535 frames of at least 7 x 7 pixels (the 7 x 7 SSIM window must fit)")
    if out is None:
        out = torch.empty(F, 5, dtype=torch.float64, device=pred.device)
    _dev("out", out, dtype=torch.float64, shape=(F, 5))
    ws = _ws(ws, need, torch.uint8, pred.device, "ws: a contiguous uint8 CUDA tensor of >= frame_metrics_ws(F, H, W) elements", need)
    gw = None
    if gray_w is not None:
        _require(len(gray_w) == 4, "gray_w: (wr, wg, wb, shift)")
        gw = (ctypes.c_int * 4)(*[int(v) for v in gray_w])
    _lib.call("snerf_frame_metrics", _p(pred), _p(gt), u8, F, H, W, gw, _p(ws), ws.numel(), _p(out), _stream())
    return out


def zip_ray_batch(images, depths, semantics, masks, pixtocams, camtoworlds, local2global, near, far, border, patch_size, single_image, seed,
                  counter, n, i0, i1, out):
    """snerf_zip_ray_batch: rows [i0, i1) of step counter[0]'s global batch of n rays into the preallocated `out` (dict: origins,
    directions, viewdirs, base_x, base_y [m,3], radii, lossmult, near, far, cam_idx [m,1], imageplane [m,2] / glo_idx [m,1] / depth [m] /
    semantic int32 [m] / mask [m] or absent, rgb [m,3], pix_x_int / pix_y_int int32 [m]); advances counter[0]."""
    u8 = 1 if _dev("images", images, dtype=_U8_F32).dtype == torch.uint8 else 0
    N, H, W = images.shape[:3]
    _dev("depths masks pixtocams camtoworlds", depths, masks, pixtocams, camtoworlds, optional=True)
    _dev("semantics local2global", semantics, local2global, dtype=torch.int32, optional=True); _dev("counter", counter, dtype=torch.int64)
    _require(counter.numel() == 2, "counter: int64 [2]")
    _lib.call("snerf_zip_ray_batch", _p(images), u8, _p(depths), _p(semantics), _p(masks), _p(pixtocams), _p(camtoworlds), _p(local2global),
              N, H, W, float(near), float(far), int(border), int(patch_size), int(bool(single_image)), int(seed), _p(counter), int(n), int(i0),
              int(i1), _p(out["origins"]), _p(out["directions"]), _p(out["viewdirs"]), _p(out["radii"]), _p(out.get("imageplane")),
              _p(out["base_x"]), _p(out["base_y"]), _p(out["lossmult"]), _p(out["near"]), _p(out["far"]), _p(out["cam_idx"]),
              _p(out.get("glo_idx")), _p(out["rgb"]), _p(out.get("depth")), _p(out.get("semantic")), _p(out.get("mask")), _p(out["pix_x_int"]),
              _p(out["pix_y_int"]), _stream())
    return out


def zip_ray_patch_batch(images, depths, semantics, masks, pixtocams, camtoworlds, local2global, near, far, border, patch_size, single_image,
                        seed, counter, n, k0, k1, i0, i1, out):
    """snerf_zip_ray_patch_batch: patches [k0, k1) of step counter[0]'s n_patch = (n // 4) // patch_size^2 patches, then positions
    [i0, i1) of its single pixels (n_patch patch_size^2 <= i0), into the preallocated `out` (as for zip_ray_batch, with
    m = (k1 - k0) patch_size^2 + (i1 - i0) rows); one launch, advances counter[0]."""
    u8 = 1 if _dev("images", images, dtype=_U8_F32).dtype == torch.uint8 else 0
    N, H, W = images.shape[:3]
    _dev("depths masks pixtocams camtoworlds", depths, masks, pixtocams, camtoworlds, optional=True)
    _dev("semantics local2global", semantics, local2global, dtype=torch.int32, optional=True); _dev("counter", counter, dtype=torch.int64)
    _require(counter.numel() == 2, "counter: int64 [2]")
    m = (int(k1) - int(k0)) * int(patch_size) ** 2 + (int(i1) - int(i0))
    _require(all(v is None or v.shape[0] == m for v in out.values()), "out: (k1 - k0) patch_size^2 + (i1 - i0) rows")
    _lib.call("snerf_zip_ray_patch_batch", _p(images), u8, _p(depths), _p(semantics), _p(masks), _p(pixtocams), _p(camtoworlds),
              _p(local2global), N, H, W, float(near), float(far), int(border), int(patch_size), int(bool(single_image)), int(seed), _p(counter),
              int(n), int(k0), int(k1), int(i0), int(i1), _p(out["origins"]), _p(out["directions"]), _p(out["viewdirs"]), _p(out["radii"]),
              _p(out.get("imageplane")), _p(out["base_x"]), _p(out["base_y"]), _p(out["lossmult"]), _p(out["near"]), _p(out["far"]),
              _p(out["cam_idx"]), _p(out.get("glo_idx")), _p(out["rgb"]), _p(out.get("depth")), _p(out.get("semantic")), _p(out.get("mask")),
              _p(out["pix_x_int"]), _p(out["pix_y_int"]), _stream())
    return out


def zip_smooth_loss_ws(P):
    """doubles of scratch zip_smooth_loss needs for P patches (snerf_zip_smooth_loss_ws)"""
    return int(_lib.query("snerf_zip_smooth_loss_ws", int(P)))


def zip_smooth_loss(rgb, depth, sem, mask, P, p, d_mult=0.001, s_mult=0.001, grad_mult=1.0, out=None, total=None, g_depth=None, g_sem=None,
                    accumulate=False, ws=None):
    """snerf_zip_smooth_loss: the patch terms of the zipnerf loop (d_smo, s_smo: masked edge-aware smoothness of the rendered disparity
    and class probabilities) of P patches of p x p rays, values and gradients in one pass.  rgb [P p p, 3] target colours, depth [P p p]
    rendered, sem [P p p, C] rendered probabilities (a row-major view, row stride >= C) or None, mask [P p p] (> 0 = masked out) or None
    (fp32; rgb / depth / mask of any shape of that size) -> (out[4] = {d_smo, s_smo, Nx, Ny}, g_depth [P p p], g_sem like sem or None)
    = grad_mult * d (d_smo + s_smo) / d (depth, sem).  total: a device float the two values are added into; g_depth / g_sem given:
    stored into (accumulate=False) or added into (True); g_sem has sem's row stride.  Deterministic (float64 sums in a fixed order, no
    float atomics).  ws: fp64 scratch of >= zip_smooth_loss_ws(P) elements (allocated when None).  P = 0 launches nothing."""
    P, p = int(P), int(p)
    n, dev = P * p * p, depth.device
    _dev("rgb depth mask total g_depth out", rgb, depth, mask, total, g_depth, out, optional=True)
    _require(rgb.numel() == 3 * n and depth.numel() == n and (mask is None or mask.numel() == n), "rgb [P,p,p,3], depth / mask [P,p,p]")
    C = ld = 0
    if sem is not None:
        _chk2d("sem", sem, dt=torch.float32)
        C, ld = sem.shape[1], sem.stride(0) if n > 1 else sem.shape[1]
        _require(sem.shape[0] == n and ld >= C, "sem [P p p, C]")
        if g_sem is None:
            _require(not accumulate, "accumulate=True adds into a given g_sem")
            g_sem = torch.empty_strided((n, C), (ld, 1), dtype=torch.float32, device=dev)
        _chk2d("g_sem", g_sem, dt=torch.float32)
        _require(g_sem.shape == sem.shape and (n <= 1 or g_sem.stride(0) == ld), "g_sem: sem's shape and row stride")
    if out is None:
        out = torch.zeros(4, dtype=torch.float32, device=dev)
    if g_depth is None:
        _require(not accumulate, "accumulate=True adds into a given g_depth")
        g_depth = torch.empty(n, dtype=torch.float32, device=dev)
    _require(out.numel() == 4 and g_depth.numel() == n and (total is None or total.numel() == 1), "out fp32 [4], g_depth fp32 [P p p], total fp32 [1]")
    ws = _ws(ws, lambda: max(zip_smooth_loss_ws(P), 1), torch.float64, dev, "ws: a contiguous fp64 CUDA tensor of >= zip_smooth_loss_ws(P) elements")
    _lib.call("snerf_zip_smooth_loss", _p(rgb), _p(depth), _p(sem), ld, C, _p(mask), P, p, float(d_mult), float(s_mult), float(grad_mult),
              _p(ws), ws.numel(), _p(out), _p(total), _p(g_depth), _p(g_sem) if sem is not None else None, int(bool(accumulate)), _stream())
    return out, g_depth, (g_sem if sem is not None else None)


ZIP_LOSS_NAMES = ("data", "mse", "depth", "d_complete", "sem", "interlevel", "distortion")


def zip_loss_tail(rgb, tgt, lossmult=None, depth=None, tdepth=None, dmask=None, cmask=None, sem=None, labels=None, smask=None, hist=None,
                  mse=False, charb_padding=0.001, data_mult=1.0, depth_lambda=0.5, com_mult=0.2, sem_mult=0.04, pulse_width=(0.03, 0.003),
                  interlevel_mult=0.01, distortion_mult=0.005):
    """One launch for the zipnerf loss tail.  `hist` = [(sdist, weights)] * 3 (proposal, proposal, NeRF) or None.
    -> (out[11] (see include/snerf_hip.h), dict of gradients: rgb, depth, semantic, w0, w1, w2 -- None where the term is off)."""
    R, dev = rgb.shape[0], rgb.device
    _dev("rgb tgt lossmult depth tdepth dmask cmask sem smask", rgb, tgt, lossmult, depth, tdepth, dmask, cmask, sem, smask, optional=True)
    new = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=dev)
    out, g_rgb = new(11), new(R, 3)
    g_depth = new(R) if depth is not None else None
    C = 0
    g_sem = None
    if sem is not None:
        C = sem.shape[1]
        _dev("labels", labels, dtype=torch.int32, shape=(R,))
        g_sem = new(R, C)
    s = [None] * 3; w = [None] * 3; S = [0] * 3; gw = [None] * 3
    if hist is not None:
        for i, (sd, wt) in enumerate(hist):
            if sd is None:
                continue
            _dev("hist", sd, wt)
            s[i], w[i], S[i] = sd, wt, wt.shape[1]
            _require(sd.shape == (R, S[i] + 1) and wt.shape[0] == R, "hist: (sdist [R, S + 1], weights [R, S]) per level")
        _require(s[2] is not None, "hist: the NeRF level (the third pair) is needed")
        if distortion_mult > 0:
            gw[2] = new(R, S[2])
        if interlevel_mult > 0:
            for i in (0, 1):
                if s[i] is not None:
                    gw[i] = new(R, S[i])
    _lib.call("snerf_zip_loss_tail", _p(rgb), _p(tgt), _p(lossmult), _p(depth), _p(tdepth), _p(dmask), _p(cmask), _p(sem),
              _p(labels), _p(smask), C, _p(s[0]), _p(w[0]), S[0], _p(s[1]), _p(w[1]), S[1], _p(s[2]), _p(w[2]), S[2], R, int(bool(mse)),
              float(charb_padding), float(data_mult), float(depth_lambda), float(com_mult), float(sem_mult), float(pulse_width[0]),
              float(pulse_width[1]), float(interlevel_mult), float(distortion_mult), _p(out), _p(g_rgb), _p(g_depth), _p(g_sem), _p(gw[0]),
              _p(gw[1]), _p(gw[2]), _stream())
    return out, dict(rgb=g_rgb, depth=g_depth, semantic=g_sem, w0=gw[0], w1=gw[1], w2=gw[2])


def zip_percentiles(tdist, weights, t_far, ps=(5, 50, 95)):
    """weighted percentiles (in %) of the ray histograms extended to t_far -> [R, len(ps)] (render.py:255-267)."""
    import numpy as np
    R, S = weights.shape
    tf = t_far.reshape(-1).contiguous()
    _dev("tdist weights t_far", tdist, weights, tf)
    _require(tdist.shape == (R, S + 1) and tf.shape[0] == R, "tdist [R, S + 1], weights [R, S], t_far [R]")
    p = np.ascontiguousarray(np.asarray(ps, dtype=np.float32))
    out = torch.empty(R, len(ps), dtype=torch.float32, device=weights.device)
    _lib.call("snerf_zip_percentiles", _p(tdist), _p(weights), _p(tf), R, S, p.ctypes.data, len(ps), _p(out), _stream())
    return out


def frame_quantize(rgb=None, depth=None, semantic=None, color_map=None, scale_factor=1.0):
    """Quantise rendered frame buffers for the S-NeRF++ wire format in one launch (random_render_waymo_seq.py:214-227):
    rgb [..,3] -> uint8, depth [..] -> uint16 (= depth * 256 / scale_factor), semantic [..,C] -> argmax label uint8 (+ paint uint8 [..,3]
    through `color_map` uint8 [C,3]).  -> dict with the keys of the inputs given ('rgb', 'depth', 'semantic', 'paint'), device tensors."""
    ref = rgb if rgb is not None else (depth if depth is not None else semantic)
    dev = ref.device
    out = {}
    P = (rgb.numel() // 3) if rgb is not None else (depth.numel() if depth is not None else semantic.numel() // semantic.shape[-1])
    r = d = s = cm = r8 = d16 = l8 = p8 = None
    C, ld = 0, 0
    if rgb is not None:
        r = _dev("rgb", rgb.contiguous())
        _require(r.shape[-1] == 3 and r.numel() == 3 * P, "rgb [..., 3] fp32")
        r8 = out["rgb"] = torch.empty(r.shape, dtype=torch.uint8, device=dev)
    if depth is not None:
        d = _dev("depth", depth.contiguous())
        _require(d.numel() == P, "depth: one fp32 per pixel")
        d16 = out["depth"] = torch.empty(d.shape, dtype=torch.uint16, device=dev)
    if semantic is not None:
        s = _dev("semantic", semantic.contiguous())
        C = ld = s.shape[-1]
        _require(s.numel() == C * P and C <= 256, "semantic [..., C <= 256] fp32")
        l8 = out["semantic"] = torch.empty(s.shape[:-1], dtype=torch.uint8, device=dev)
        if color_map is not None:
            cm = _dev("color_map", color_map.contiguous(), dtype=torch.uint8, shape=(C, 3))
            p8 = out["paint"] = torch.empty(tuple(s.shape[:-1]) + (3,), dtype=torch.uint8, device=dev)
    _lib.call("snerf_frame_quantize", _p(r), _p(d), _p(s), ld, C, _p(cm), P, float(scale_factor), _p(r8), _p(d16), _p(l8), _p(p8), _stream())
    return out


def hash_decay(table, grad, offsets, L, C, mult, loss=None, grad_mult=1.0):
    """grad += grad_mult * d/d table of mult * mean_{level, channel}(mean over the level's rows of table^2) (train_utils.py:184-203);
    `loss` (1-element fp32 device tensor, optional) accumulates the value.  `grad_mult`: the trainer's loss scale (the term is linear in
    `mult`, so the kernel runs with mult * grad_mult and the value is divided back)."""
    _dev("table grad", table, grad); _dev("offsets", offsets, dtype=torch.int32)
    _require(table.shape == grad.shape, "grad: table's shape")
    if grad_mult != 1.0 and loss is not None:
        tmp = torch.zeros_like(loss)
        _lib.call("snerf_hash_decay", _p(table), _p(grad), _p(offsets), int(L), int(C), float(mult) * float(grad_mult), _p(tmp), _stream())
        loss.add_(tmp, alpha=1.0 / float(grad_mult))
        return
    _lib.call("snerf_hash_decay", _p(table), _p(grad), _p(offsets), int(L), int(C), float(mult) * float(grad_mult), _p(loss), _stream())


def semantic_composite_fwd(weights, logits, C, softmax, row_index=None):
    """semantic [R,C] = sum_i w[r,i] f(logits[r*S+i, :C]), f = softmax (zipnerf) or identity (live mip path); logits: 2-D view.
    `row_index` (int32 [R,S], -1 = skipped): the logits are the rows of a compacted evaluation (ert_compact)."""
    R, S = weights.shape
    _dev("weights", weights); _chk2d("logits", logits); _dev("row_index", row_index, dtype=torch.int32, optional=True)
    _require(row_index is None or row_index.numel() == R * S, "row_index: int32 [R, S]")
    sem = torch.empty(R, C, dtype=torch.float32, device=weights.device)
    _lib.call("snerf_semantic_composite_fwd", _p(weights), _p(logits), logits.stride(0), _zip_dt(logits), R, S, C, int(bool(softmax)),
              _p(row_index), _p(sem), _stream())
    return sem


def semantic_composite_bwd(weights, logits, g_sem, C, softmax, d_logits, want_g_w=False):
    """d_logits (fp32 2-D view, >= C columns) <- gradient of the logits; returns d weights [R,S] when `want_g_w` (identity flavour)."""
    R, S = weights.shape
    _dev("weights g_sem", weights, g_sem); _chk2d("logits", logits); _chk2d("d_logits", d_logits, dt=torch.float32)
    g_w = torch.empty(R, S, dtype=torch.float32, device=weights.device) if want_g_w else None
    _lib.call("snerf_semantic_composite_bwd", _p(weights), _p(logits), logits.stride(0), _zip_dt(logits), _p(g_sem), R, S, C, int(bool(softmax)),
              _p(d_logits), d_logits.stride(0), _p(g_w), _stream())
    return g_w


MESH_NO_CULL, MESH_UNIFORM = 1, 2       # flags of the trace entries: every chunk entered / chunks read by wave-uniform loads, not staged in LDS (both: measurements)


def mesh_ws_bytes(F):
    """bytes of device memory mesh_prepare fills for F faces (snerf_mesh_ws_bytes; 0 for F <= 0)"""
    return int(_lib.query("snerf_mesh_ws_bytes", int(F)))


_MESH_WS = "ws: uint8 CUDA tensor of >= mesh_ws_bytes(F) elements, filled by mesh_prepare"       # (F = 0: no workspace is read, anything passes)


def mesh_prepare(vertices, faces, face_ids=None, transform=None, ws=None):
    """snerf_mesh_prepare: vertices [V,3] fp32, faces [F,3] int32 in the order the tracer walks them (meshtrace.RayTracer sorts them by
    Morton code once), face_ids [F] int32 = the caller's id of each ordered face (None: its position), transform = a [3,4] fp32 DEVICE
    tensor or None -> ws (uint8, mesh_ws_bytes(F) elements; allocated when None) holding the transformed triangles and the chunk and
    group boxes.  Faces with an index outside [0, V), a non-finite vertex or no area are dropped by the kernel.  No host read."""
    _dev("vertices", vertices, shape=(None, 3), msg="vertices [V,3] fp32")
    _dev("faces", faces, dtype=torch.int32, shape=(None, 3), msg="faces [F,3] int32")
    V, F = vertices.shape[0], faces.shape[0]
    _dev("face_ids", face_ids, dtype=torch.int32, optional=True, msg="face_ids [F] int32")
    _require(face_ids is None or face_ids.numel() == F, "face_ids [F] int32")
    _dev("transform", transform, shape=(3, 4), optional=True, msg="transform [3,4] fp32 on the device")
    if ws is None:
        ws = torch.empty(mesh_ws_bytes(F), dtype=torch.uint8, device=vertices.device)
    elif F != 0:
        _ws_given(ws, torch.uint8, _MESH_WS, mesh_ws_bytes(F))
    _lib.call("snerf_mesh_prepare", _p(vertices), V, _p(faces), _p(face_ids), F, _p(transform), _p(ws), ws.numel(), _stream())
    return ws


def mesh_trace(ws, F, rays_o, rays_d, t_max=100., positions=True, normals=True, flags=0):
    """snerf_mesh_trace: rays_o, rays_d [R,3] fp32 against the prepared mesh -> (depth [R] = t of the nearest hit with 0 < t < t_max, else
    t_max; face_id [R] int32 in the caller's numbering, -1 on a miss; positions [R,3] or None; normals [R,3] or None).  No host read."""
    _dev("rays_o", rays_o, shape=(None, 3), msg="rays_o, rays_d [R,3] fp32"); _dev("rays_d", rays_d, shape=tuple(rays_o.shape), msg="rays_o, rays_d [R,3] fp32")
    R, dev = rays_o.shape[0], rays_o.device
    if F != 0:
        _ws_given(ws, torch.uint8, _MESH_WS, mesh_ws_bytes(F))
    depth = torch.empty(R, dtype=torch.float32, device=dev)
    face_id = torch.empty(R, dtype=torch.int32, device=dev)
    pos = torch.empty(R, 3, dtype=torch.float32, device=dev) if positions else None
    nrm = torch.empty(R, 3, dtype=torch.float32, device=dev) if normals else None
    _lib.call("snerf_mesh_trace", _p(ws), int(F), _p(rays_o), _p(rays_d), R, float(t_max), int(flags), _p(depth), _p(face_id), _p(pos),
              _p(nrm), _stream())
    return depth, face_id, pos, nrm


def mesh_trace_pinhole(ws, F, fx, fy, cx, cy, pixel_center, H, W, mask=None, t_max=100., miss_value=100., want_hit=False, flags=0, device=None):
    """snerf_mesh_trace_pinhole: the rays d = ((x + c - cx) / fx, -(y + c - cy) / fy, -1) of an H x W camera at the origin (c = 0.5 with
    pixel_center), generated in the kernel -> (depth [H,W] fp32: t = z-depth of a hit, miss_value on a traced miss, 0 outside `mask`
    ([H,W,3] uint8, channel 0 > 0 = traced; None: every pixel); hit [H,W,3] uint8 = 255 on a hit, or None).  No host read."""
    H, W = int(H), int(W)
    dev = ws.device if ws is not None else (mask.device if mask is not None else torch.device("cuda", torch.cuda.current_device()) if device is None else device)
    _dev("mask", mask, dtype=torch.uint8, shape=(H, W, 3), optional=True, msg="mask [H,W,3] uint8")
    if F != 0:
        _ws_given(ws, torch.uint8, _MESH_WS, mesh_ws_bytes(F))
    depth = torch.empty(H, W, dtype=torch.float32, device=dev)
    hit = torch.empty(H, W, 3, dtype=torch.uint8, device=dev) if want_hit else None
    _lib.call("snerf_mesh_trace_pinhole", _p(ws), int(F), float(fx), float(fy), float(cx), float(cy), int(bool(pixel_center)), H, W,
              _p(mask), float(t_max), float(miss_value), int(flags), _p(depth), _p(hit), _stream())
    return depth, hit


def mesh_render_scratch_bytes(H, W):
    """bytes of device scratch the validity rule of mesh_render_pinhole needs (snerf_mesh_render_scratch_bytes; 0 for H or W <= 0)"""
    return int(_lib.query("snerf_mesh_render_scratch_bytes", int(H), int(W)))


def mesh_render_pinhole(ws, F, fx, fy, cx, cy, H, W, faces=None, vertex_color=None, uvs=None, face_uvs_idx=None, face_material_idx=None, texels=None,
                        materials=None, t_max=100., miss_value=100., validate=True, flags=0, want_image_f=False, want_mask=True, want_depth=False,
                        want_face_id=False, device=None):
    """snerf_mesh_render_pinhole: the pixel-centre rays of mesh_trace_pinhole against the prepared mesh, shaded from exactly one attribute
    source -- vertex_color [V,3] fp32 through the ORDERED faces [F,3] int32, or uvs [U,2] fp32 through face_uvs_idx [F,3] int32,
    face_material_idx [F] int32 (both in the tracer's order), texels [T,4] fp32 (r, g, b, 0) and materials [M,4] int32 = (texel offset,
    Hm, Wm, 0) -> (image [H,W,3] uint8, image_f [H,W,3] fp32 or None, mask [H,W,3] uint8 or None, depth [H,W] fp32 or None, face_id [H,W]
    int32 or None).  `validate`: mesh_renderer.py's frame-validity rule, decided and applied on the device.  No host read."""
    H, W, F = int(H), int(W), int(F)
    dev = ws.device if ws is not None else (torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device))
    V = U = M = T = 0
    if F > 0:
        _require((vertex_color is None) != (face_uvs_idx is None), "exactly one of vertex_color and face_uvs_idx")
        _ws_given(ws, torch.uint8, _MESH_WS, mesh_ws_bytes(F))
    if vertex_color is not None:
        _dev("vertex_color", vertex_color, shape=(None, 3), msg="vertex_color [V,3] fp32")
        V = vertex_color.shape[0]
        _dev("faces", faces, dtype=torch.int32, shape=(F, 3))
    if face_uvs_idx is not None:
        _dev("uvs", uvs, shape=(None, 2), msg="uvs [U,2] fp32"); _dev("texels", texels, shape=(None, 4), msg="texels [T,4] fp32")
        U, T = uvs.shape[0], texels.shape[0]
        _dev("face_uvs_idx", face_uvs_idx, dtype=torch.int32, shape=(F, 3)); _dev("face_material_idx", face_material_idx, dtype=torch.int32, shape=(F,))
        M = _dev("materials", materials, dtype=torch.int32, shape=(None, 4)).shape[0]
    image = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
    image_f = torch.empty(H, W, 3, dtype=torch.float32, device=dev) if want_image_f else None
    mask = torch.empty(H, W, 3, dtype=torch.uint8, device=dev) if want_mask else None
    depth = torch.empty(H, W, dtype=torch.float32, device=dev) if want_depth else None
    face_id = torch.empty(H, W, dtype=torch.int32, device=dev) if want_face_id else None
    scratch = torch.empty(mesh_render_scratch_bytes(H, W), dtype=torch.uint8, device=dev) if validate else None
    _lib.call("snerf_mesh_render_pinhole", _p(ws), F, float(fx), float(fy), float(cx), float(cy), H, W, float(t_max), float(miss_value),
              int(flags), _p(faces), _p(vertex_color), V, _p(uvs), U, _p(face_uvs_idx), _p(face_material_idx), _p(texels), T, _p(materials), M,
              int(bool(validate)), _p(scratch), 0 if scratch is None else scratch.numel(), _p(image), _p(image_f), _p(mask), _p(depth), _p(face_id),
              _stream())
    return image, image_f, mask, depth, face_id


def shadow_ws_bytes(H, W, N=0, r=20, iter=3):
    """bytes of device scratch the three shadow stages share (snerf_shadow_ws_bytes; raises for a shape or parameter the library refuses)"""
    n = int(_lib.query("snerf_shadow_ws_bytes", int(H), int(W), int(N), int(r), int(iter)))
    if n <= 0:
        raise _lib.SnerfHipError(f"snerf_shadow_ws_bytes refuses H={H} W={W} N={N} r={r} iter={iter}")
    return n


def shadow_ws_views(ws, H, W):
    """(info, counts): int32 views into ws at snerf_shadow_ws_offset(H, W, 0 / 1) -- info = (any, kw, kh, xmin, xmax, ymin, ymax, 0) and
    counts [H,W], as the last shadow_fuse with a non-empty mask left them (what the tests compare with the CPU model)"""
    o_info, o_counts = (int(_lib.query("snerf_shadow_ws_offset", int(H), int(W), k)) for k in (0, 1))
    _require(o_info >= 0 and o_counts >= 0, "snerf_shadow_ws_offset refuses this shape")
    return ws[o_info:o_info + 32].view(torch.int32), ws[o_counts:o_counts + 4 * H * W].view(torch.int32).view(H, W)


_SHADOW_WS = "ws: a contiguous uint8 CUDA tensor (shadow_ws_bytes)"           # (the library refuses a short one)


def shadow_project(vertices, xf, ground_mode, H, W, ws, mask_out=None):
    """snerf_shadow_project: vertices [N,3] fp32 or fp64 on the device, xf = 28 HOST doubles (placement 3 x 4, light vector, ground
    height, world-to-pixel 3 x 4; a ctypes array or anything numpy converts), ground_mode 0 = that height, 1 = the smallest placed z, 2 = no
    ground projection -> the splat mask in ws (the input of shadow_close(None,
    ...)), and in mask_out [H,W,3] uint8 when given.  No host read of device memory."""
    _dev("vertices", vertices, dtype=(torch.float32, torch.float64), shape=(None, 3), msg="vertices [N,3] fp32 / fp64 on the device")
    if not isinstance(xf, ctypes.Array):
        import numpy as np
        xf = (ctypes.c_double * 28)(*np.asarray(xf, dtype=np.float64).reshape(28).tolist())
    _require(len(xf) == 28, "xf: 28 host doubles")
    _dev("mask_out", mask_out, dtype=torch.uint8, shape=(H, W, 3), optional=True); _ws_given(ws, torch.uint8, _SHADOW_WS)
    _lib.call("snerf_shadow_project", _p(vertices), int(vertices.dtype == torch.float64), vertices.shape[0], ctypes.addressof(xf), int(ground_mode),
              int(H), int(W), _p(mask_out), _p(ws), ws.numel(), _stream())
    return mask_out


def shadow_close(mask_in, H, W, r, iter, ws, mask_out=None):
    """snerf_shadow_close: the closing of utils.py:195-211 interpolate on mask_in [H,W,3] uint8 (None: the splat shadow_project left in
    ws) -> the closed mask in ws (the input of shadow_fuse(..., None, ...)), and in mask_out when given (mask_out may be mask_in)."""
    _dev("mask_in mask_out", mask_in, mask_out, dtype=torch.uint8, shape=(H, W, 3), optional=True); _ws_given(ws, torch.uint8, _SHADOW_WS)
    _lib.call("snerf_shadow_close", _p(mask_in), int(H), int(W), int(r), int(iter), _p(mask_out), _p(ws), ws.numel(), _stream())
    return mask_out


def shadow_fuse(im, total_mask, shadow_mask, H, W, light_scale, check, ws):
    """snerf_shadow_fuse: in place on im [H,W,3] uint8 -- mesh_shadow.py:89-107 blur_shadow with shadow_mask [H,W,3] uint8 (None: the
    closed mask shadow_close left in ws), or with check the blanking im[mask > 0] = 0 (total_mask may then be None)."""
    _dev("im total_mask shadow_mask", im, total_mask, shadow_mask, dtype=torch.uint8, shape=(H, W, 3), optional=True); _ws_given(ws, torch.uint8, _SHADOW_WS)
    _lib.call("snerf_shadow_fuse", _p(im), _p(total_mask), _p(shadow_mask), int(H), int(W), float(light_scale), int(bool(check)), _p(ws), ws.numel(), _stream())
    return im
