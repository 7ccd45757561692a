"""The patch terms of the zipnerf loop (d_smo, s_smo; s-nerfpp/zipnerf/train.py:280-293) inside the fused path C step: the loss kernel
(snerf_zip_smooth_loss / ops.zip_smooth_loss), the patch batches of the device batcher (snerf_zip_ray_patch_batch /
zipnerf.PatchRayBatcher) and ZipTrainer.step(n_patch=...), eager and captured.  The two terms are restated below in torch, parametrised by
dtype; the kernel is held against the reference's own values (golden g32_smooth_zip, tools/gen_golden_zip_smooth.py) and against the
float64 evaluation of that restatement, with gradient bounds made from the fp32 evaluation's own error."""
import os

import numpy as np
import pytest
import torch

from snerf_amd import _lib
from test_device_batcher import np_bounded            # the numpy restatement of the batchers' bounded Philox draw

gpu = pytest.mark.gpu
D_MULT = S_MULT = float(np.float32(0.001))             # the ABI takes the multipliers as floats: the same numbers on both sides


# ---- the two terms, restated ----------------------------------------------------------------------------------------------------------
def smooth_terms(rgb, depth, sem, mask, d_mult, s_mult, dtype):
    """rgb [P,p,p,3], depth [P,p,p], sem [P,p,p,C] or None, mask [P,p,p] (> 0 = masked out) or None, evaluated in `dtype` on the CPU
    -> (d_smo, s_smo, d (d_smo + s_smo) / d depth, d / d sem or None, Nx, Ny).  Each channel is divided by its patch mean (+ eps), the
    absolute differences of horizontal / vertical neighbours are weighted by exp(-mean |colour difference|), and each direction is
    averaged over the edges of the whole batch whose two pixels are unmasked; no such edge in either direction: the terms are 0."""
    rgb = rgb.detach().cpu().to(dtype)
    depth = depth.detach().cpu().to(dtype).clone().requires_grad_(True)
    sem = None if sem is None else sem.detach().cpu().to(dtype).clone().requires_grad_(True)
    ok = torch.ones(depth.shape, dtype=torch.bool) if mask is None else ~(mask.detach().cpu() > 0)
    ok_x, ok_y = ok[:, :, :-1] & ok[:, :, 1:], ok[:, :-1] & ok[:, 1:]
    nx, ny = int(ok_x.sum()), int(ok_y.sum())
    w_x = torch.exp(-(rgb[:, :, :-1] - rgb[:, :, 1:]).abs().mean(-1))
    w_y = torch.exp(-(rgb[:, :-1] - rgb[:, 1:]).abs().mean(-1))

    def term(z, eps):                                  # z [P,p,p,K]
        if nx == 0 or ny == 0:
            return z.sum() * 0
        z = z / (z.mean((1, 2), keepdim=True) + eps)
        e_x = (z[:, :, :-1] - z[:, :, 1:]).abs().sum(-1) * w_x
        e_y = (z[:, :-1] - z[:, 1:]).abs().sum(-1) * w_y
        return e_x[ok_x].sum() / nx + e_y[ok_y].sum() / ny

    d_smo = d_mult * term((1 / (depth + 1e-5))[..., None], 1e-7)
    s_smo = s_mult * term(sem, 1e-5) if sem is not None else torch.zeros((), dtype=dtype)
    leaves = [depth] + ([sem] if sem is not None else [])
    grads = torch.autograd.grad(d_smo + s_smo, leaves)
    return d_smo.detach(), s_smo.detach(), grads[0], (grads[1] if sem is not None else None), nx, ny


def bounds(rgb, depth, sem, mask, d_mult=D_MULT, s_mult=S_MULT):
    """-> float64 results and, per gradient, the bound the issue sets: 4 x the largest deviation of the fp32 torch evaluation from the
    float64 one plus 4 fp32 ulp of max |g| -- from the references alone"""
    r64 = smooth_terms(rgb, depth, sem, mask, d_mult, s_mult, torch.float64)
    r32 = smooth_terms(rgb, depth, sem, mask, d_mult, s_mult, torch.float32)
    out = []
    for g64, g32 in zip(r64[2:4], r32[2:4]):
        if g64 is None:
            out.append(None)
            continue
        gmax, dev32 = float(g64.abs().max()), float((g32.double() - g64).abs().max())
        out.append((4 * dev32 + 4 * float(np.spacing(np.float32(gmax))), dev32, gmax))
    return r64, out


def run_kernel(rgb, depth, sem, mask, P, p, **kw):
    from snerf_amd import ops
    cu = lambda t: None if t is None else t.cuda()
    s = None if sem is None else cu(sem).reshape(P * p * p, -1)
    return ops.zip_smooth_loss(cu(rgb), cu(depth), s, cu(mask), P, p, **{"d_mult": D_MULT, "s_mult": S_MULT, **kw})


def check_against_f64(tag, got, rgb, depth, sem, mask, P, p):
    out, gd, gs = got
    r64, (bd, bs) = bounds(rgb, depth, sem, mask)
    d64, s64, gd64, gs64, nx, ny = r64
    assert (float(out[2]), float(out[3])) == (nx, ny), (tag, out.tolist(), nx, ny)
    for name, k, v in (("d_smo", 0, float(d64)), ("s_smo", 1, float(s64))):
        rel = abs(float(out[k]) - v) / max(abs(v), 1e-30)
        print(f"{tag} {name}: kernel {float(out[k]):.9e}, float64 {v:.9e}, rel {rel:.2e}")
        assert abs(float(out[k]) - v) <= 1e-6 * abs(v), (tag, name)
    err = float((gd.cpu().double().reshape(-1) - gd64.reshape(-1)).abs().max())
    print(f"{tag} g_depth: max |g| {bd[2]:.3e}, fp32 torch deviation {bd[1]:.3e}, bound {bd[0]:.3e}, kernel error {err:.3e}")
    assert err <= bd[0], (tag, "g_depth")
    if sem is not None:
        err = float((gs.cpu().double().reshape(-1) - gs64.reshape(-1)).abs().max())
        print(f"{tag} g_sem: max |g| {bs[2]:.3e}, fp32 torch deviation {bs[1]:.3e}, bound {bs[0]:.3e}, kernel error {err:.3e}")
        assert err <= bs[0], (tag, "g_sem")
    return r64


def test_restatement_matches_the_recorded_reference(golden):
    """the float64 restatement against the reference's fp32 values and autograd gradients of g32_smooth_zip: no GPU involved"""
    g = golden("g32_smooth_zip")
    (d64, s64, gd64, gs64, nx, ny), (bd, bs) = bounds(g["rgb"], g["depth"], g["sem"], g["mask"], float(g["mults"][0]), float(g["mults"][1]))
    assert [nx, ny] == g["n_edges"].tolist() and nx > 0 and ny > 0
    # the recorded values are fp32 sums of ~80 like-signed edge values per direction: a few ulp each from the per-edge arithmetic
    # (16 x 2^-24 ~ 1e-6); the recorded gradients are an fp32 evaluation, held to the bound made from this file's own fp32 evaluation
    assert abs(float(d64) - float(g["d_smo"])) <= 1e-6 * float(d64) and abs(float(s64) - float(g["s_smo"])) <= 1e-6 * float(s64)
    print(f"recorded gradients vs float64: depth {float((gd64 - g['g_depth'].double()).abs().max()):.3e} (bound {bd[0]:.3e}), "
          f"sem {float((gs64 - g['g_sem'].double()).abs().max()):.3e} (bound {bs[0]:.3e})")
    assert float((gd64 - g["g_depth"].double()).abs().max()) <= bd[0] and float((gs64 - g["g_sem"].double()).abs().max()) <= bs[0]


# ---- statuses: host-only, no launch ------------------------------------------------------------------------------------------------------
def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")


def _smooth_args(**kw):
    a = dict(rgb=64, depth=64, sem=64, ld_sem=19, C=19, mask=64, P=3, p=6, d_mult=0.001, s_mult=0.001, grad_mult=1.0, ws=64, ws_doubles=14,
             out=64, total=None, g_depth=64, g_sem=64, accumulate=0, stream=None)
    a.update(kw)
    return list(a.values())


def _patch_args(**kw):
    a = dict(images=64, images_u8=0, depths=None, semantics=None, masks=None, pixtocams=64, camtoworlds=64, local2global=None, N=3, H=24, W=40,
             near=0.1, far=10.0, border=0, patch_size=2, single_image=0, seed=0, counter=64, n=32, k0=0, k1=2, i0=8, i1=32, origins=64,
             directions=64, viewdirs=64, radii=64, imageplane=None, base_x=64, base_y=64, lossmult=64, near_out=64, far_out=64, cam_idx=64,
             glo_idx=None, rgb=64, depth=None, semantic=None, mask=None, pix_x=64, pix_y=64, stream=None)
    a.update(kw)
    return list(a.values())


def test_new_entries_reject_bad_arguments_without_a_gpu():
    """argument validation happens before any launch (the pointers here are never dereferenced)"""
    _lib_or_skip()
    bad_smooth = [dict(rgb=None), dict(depth=None), dict(out=None), dict(g_depth=None), dict(ws=None), dict(g_sem=None), dict(ws_doubles=13),
                  dict(p=1), dict(p=0), dict(p=33), dict(p=-6), dict(P=-1), dict(C=0), dict(C=33, ld_sem=33), dict(C=-1), dict(ld_sem=18),
                  dict(accumulate=2), dict(accumulate=-1)]
    for kw in bad_smooth:
        with pytest.raises(_lib.SnerfHipError, match="bad argument"):
            _lib.call("snerf_zip_smooth_loss", *_smooth_args(**kw))
    bad_patch = [dict(patch_size=1), dict(patch_size=0), dict(patch_size=33), dict(n=33, i1=33), dict(n=40, i1=40), dict(border=12),
                 dict(H=5, border=2), dict(W=1), dict(border=-1), dict(k0=-1), dict(k0=2, k1=1), dict(k1=3), dict(i0=7), dict(i0=20, i1=19),
                 dict(i1=33), dict(images=None), dict(N=0), dict(pixtocams=None), dict(counter=None), dict(glo_idx=64), dict(depth=64),
                 dict(semantic=64), dict(mask=64), dict(pix_x=None), dict(images_u8=2), dict(single_image=2)]
    for kw in bad_patch:
        with pytest.raises(_lib.SnerfHipError, match="bad argument"):
            _lib.call("snerf_zip_ray_patch_batch", *_patch_args(**kw))
    # no patches to smooth, and an empty batch, are no-ops whatever the rest
    none_smooth = [None if isinstance(v, int) and v == 64 else v for v in _smooth_args(P=0, ws_doubles=0, p=99, C=-5)]
    none_patch = [None if isinstance(v, int) and v == 64 else v for v in _patch_args(n=0, i0=0, i1=0, k1=0)]
    assert _lib.call("snerf_zip_smooth_loss", *none_smooth) is None
    assert _lib.call("snerf_zip_ray_patch_batch", *none_patch) is None
    assert [_lib.query("snerf_zip_smooth_loss_ws", P) for P in (-3, 0)] == [0, 0] and _lib.query("snerf_zip_smooth_loss_ws", 70) >= 2 + 4 * 70
    # the old entry keeps refusing patches
    from test_device_batcher import _zip_args
    with pytest.raises(_lib.SnerfHipError, match="bad argument"):
        _lib.call("snerf_zip_ray_batch", *_zip_args(patch_size=2))


def test_patch_batcher_constructor_rejects_what_it_cannot_draw():
    """checked before anything touches a device"""
    from snerf_amd import zipnerf
    img = np.zeros((2, 8, 8, 3), np.float32)
    pose, K = np.tile(np.eye(4, dtype=np.float32)[:3], (2, 1, 1)), np.tile(np.eye(3, dtype=np.float32), (2, 1, 1))
    for kw in (dict(patch_size=2, batch_size=24), dict(patch_size=2, batch_size=0), dict(patch_size=1, batch_size=16), dict(patch_size=33, batch_size=4 * 33 * 33),
               dict(patch_size=6, batch_size=4 * 36, border=2), dict(patch_size=2, batch_size=16, border=4), dict(patch_size=2, batch_size=16, batching="patches")):
        with pytest.raises(ValueError):
            zipnerf.PatchRayBatcher(img, K, pose, 0.1, 10.0, **kw)


# ---- GPU: the kernel ------------------------------------------------------------------------------------------------------------------
@gpu
def test_smooth_kernel_on_the_reference_golden(golden):
    g = golden("g32_smooth_zip")
    P, p, C = g["sem"].shape[0], g["sem"].shape[1], g["sem"].shape[3]
    assert (P, p, C) == (5, 6, 19) and g["mults"].tolist() == [D_MULT, S_MULT]
    got = run_kernel(g["rgb"], g["depth"], g["sem"], g["mask"], P, p)
    again = run_kernel(g["rgb"], g["depth"], g["sem"], g["mask"], P, p)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    out = got[0]
    for name, k in (("d_smo", 0), ("s_smo", 1)):
        want = float(g[name])
        print(f"g32_smooth_zip {name}: kernel {float(out[k]):.9e}, recorded {want:.9e}, rel {abs(float(out[k]) - want) / want:.2e}")
        assert abs(float(out[k]) - want) <= 1e-6 * abs(want) and want > 0
    assert [float(out[2]), float(out[3])] == g["n_edges"].tolist()
    r64 = check_against_f64("g32_smooth_zip", got, g["rgb"], g["depth"], g["sem"], g["mask"], P, p)
    # the recorded autograd gradients are fp32 evaluations themselves: within the same bound of the float64 ones, hence of the kernel's
    _, (bd, bs) = bounds(g["rgb"], g["depth"], g["sem"], g["mask"])
    assert float((g["g_depth"].double() - r64[2]).abs().max()) <= bd[0] and float((g["g_sem"].double() - r64[3]).abs().max()) <= bs[0]


def _masks(P, p, gen):
    col = torch.ones(P, p, p)
    col[:, :, p // 2] = 0                                                               # one valid column: no x-edge, (p - 1) y-edges a patch
    rnd = (torch.rand(P, p, p, generator=gen) < 0.3).float() * 2.5                      # about 30 % masked; any value > 0 masks
    if P * p * p <= 8:                                                                  # (four pixels: one masked, one valid edge each way)
        rnd = torch.zeros(P, p, p)
        rnd[0, 0, 0] = 2.5
    return {"none": None, "random": rnd, "all": torch.ones(P, p, p), "column": col}


@gpu
@pytest.mark.parametrize("p,P,C,ld", [(2, 1, 1, 1), (2, 70, 19, 19), (8, 1, 32, 32), (8, 3, 19, 24), (8, 70, 1, 1), (32, 1, 19, 19), (32, 3, 32, 32),
                                      (32, 70, 19, 19)])
def test_smooth_kernel_edges(p, P, C, ld):
    from snerf_amd import ops
    gen = torch.Generator().manual_seed(1000 * p + 10 * P + C)
    pp = p * p
    rgb = torch.rand(P, p, p, 3, generator=gen)
    depth = torch.rand(P, p, p, generator=gen) * 39.5 + 0.5
    const = P - 1 if P >= 3 else None                                                   # a patch of constant depth
    if const is not None:
        depth[const] = 7.25
    sem_store = torch.zeros(P, p, p, ld)
    # (a softmax over one class is the constant 1, which has no edges: one class gets plain probabilities)
    sem_store[..., :C] = torch.softmax(torch.randn(P, p, p, C, generator=gen) * 2.0, -1) if C > 1 else torch.rand(P, p, p, 1, generator=gen) * 0.8 + 0.1
    sem = sem_store[..., :C]                                                            # row stride ld >= C
    for name, mask in _masks(P, p, gen).items():
        tag = f"p={p} P={P} C={C} ld={ld} mask={name}"
        got = run_kernel(rgb, depth, sem_store.cuda().reshape(P * pp, ld)[:, :C], mask, P, p)
        out, gd, gs = got
        assert tuple(gs.shape) == (P * pp, C) and (gs.stride(0) == ld or P * pp == 1)
        d64, s64, gd64, gs64, nx, ny = smooth_terms(rgb, depth, sem, mask, D_MULT, S_MULT, torch.float64)
        if name in ("all", "column"):                                                   # an empty edge set in one direction: exact zeros
            assert (nx, ny) == ((0, 0) if name == "all" else (0, P * (p - 1)))
            assert float(out[0]) == 0 and float(out[1]) == 0 and (float(out[2]), float(out[3])) == (nx, ny)
            assert float(gd.abs().max()) == 0 and float(gs.abs().max()) == 0
            assert float(d64) == 0 and float(s64) == 0 and float(gd64.abs().max()) == 0 and float(gs64.abs().max()) == 0
            pre_d, pre_s = torch.rand(P * pp, generator=gen).cuda(), torch.rand(P * pp, ld, generator=gen).cuda()
            acc_d, acc_s, total = pre_d.clone(), pre_s.clone(), torch.full((1,), 1.5, device="cuda")
            ops.zip_smooth_loss(rgb.cuda(), depth.cuda(), sem_store.cuda().reshape(P * pp, ld)[:, :C], mask.cuda(), P, p, total=total, g_depth=acc_d,
                                g_sem=acc_s[:, :C], accumulate=True)
            assert torch.equal(acc_d, pre_d) and torch.equal(acc_s, pre_s) and float(total) == 1.5
            continue
        assert nx > 0 and ny > 0
        if name == "none":
            assert nx == ny == P * p * (p - 1)
        check_against_f64(tag, got, rgb, depth, sem, mask, P, p)
        assert bool(torch.isfinite(gd).all()) and bool(torch.isfinite(gs).all())
        gdh = gd.cpu().view(P, pp)
        if const is not None:                                                           # equal neighbours: sign(0) = 0, and nothing through the mean
            assert float(gdh[const].abs().max()) == 0 and float(gd64.view(P, pp)[const].abs().max()) == 0
            assert float(gs.cpu().view(P, pp, C)[const].abs().max()) > 0
        if name == "random":                                                            # a masked pixel still feels its patch mean
            m = mask.view(P, pp) > 0
            with_edges = (gd64.view(P, pp).abs() * (~m)).amax(1) > 0
            pick = m & with_edges[:, None]
            if const is not None:
                pick[const] = False
            assert bool(pick.any()), "no masked pixel beside valid edges"
            assert bool((gdh[pick] != 0).all()) and bool((gd64.view(P, pp)[pick] != 0).all())
            assert bool((gs.cpu().view(P, pp, C)[pick] != 0).all())
        # two identical calls; accumulate and total; the loss scale; zero multipliers; no semantic input
        again = run_kernel(rgb, depth, sem_store.cuda().reshape(P * pp, ld)[:, :C], mask, P, p)
        assert all(torch.equal(a, b) for a, b in zip(got, again))
        pre_d, pre_s = torch.rand(P * pp, generator=gen).cuda() - 0.5, torch.rand(P * pp, ld, generator=gen).cuda() - 0.5
        acc_d, acc_s, total = pre_d.clone(), pre_s.clone(), torch.full((1,), 1.5, device="cuda")
        cu = lambda t: None if t is None else t.cuda()
        sem_dev = sem_store.cuda().reshape(P * pp, ld)[:, :C]
        out3, g3, s3 = ops.zip_smooth_loss(rgb.cuda(), depth.cuda(), sem_dev, cu(mask), P, p, d_mult=D_MULT, s_mult=S_MULT, total=total, g_depth=acc_d,
                                           g_sem=acc_s[:, :C], accumulate=True)
        assert g3 is acc_d and torch.equal(acc_d, pre_d + gd) and torch.equal(acc_s[:, :C], pre_s[:, :C] + gs) and torch.equal(out3, out)
        assert torch.equal(acc_s[:, C:], pre_s[:, C:])                                   # the padding columns of a wide row are not written
        assert torch.equal(total, (torch.full((1,), 1.5, device="cuda") + out[0]) + out[1])
        over_d, over_s = pre_d.clone(), pre_s.clone()
        ops.zip_smooth_loss(rgb.cuda(), depth.cuda(), sem_dev, cu(mask), P, p, d_mult=D_MULT, s_mult=S_MULT, g_depth=over_d, g_sem=over_s[:, :C])
        assert torch.equal(over_d, gd) and torch.equal(over_s[:, :C], gs) and torch.equal(over_s[:, C:], pre_s[:, C:])
        out_s, gd_s, gs_s = run_kernel(rgb, depth, sem_dev, mask, P, p, grad_mult=4096.0)
        assert torch.equal(out_s, out) and torch.equal(gd_s, gd * 4096) and torch.equal(gs_s, gs * 4096)
        out0, gd0, gs0 = run_kernel(rgb, depth, sem_dev, mask, P, p, d_mult=0.0, s_mult=0.0)
        assert float(out0[0]) == 0 and float(out0[1]) == 0 and float(gd0.abs().max()) == 0 and float(gs0.abs().max()) == 0
        assert torch.equal(out0[2:], out[2:])
        # sem = NULL through the C entry itself: s_smo = 0 and the g_sem it is handed stays as it was
        keep = pre_s.clone()
        out_n, gd_n = torch.zeros(4, device="cuda"), torch.empty(P * pp, device="cuda")
        ws = torch.empty(ops.zip_smooth_loss_ws(P), dtype=torch.float64, device="cuda")
        rgb_dev, depth_dev, m_dev = rgb.cuda(), depth.cuda(), cu(mask)                  # (named: alive while the launches run)
        _lib.call("snerf_zip_smooth_loss", rgb_dev.data_ptr(), depth_dev.data_ptr(), None, 0, 0, None if m_dev is None else m_dev.data_ptr(), P, p,
                  D_MULT, S_MULT, 1.0, ws.data_ptr(), ws.numel(), out_n.data_ptr(), None, gd_n.data_ptr(), keep.data_ptr(), 0, ops._stream())
        r64n, (bdn, _) = bounds(rgb, depth, None, mask)
        assert float(out_n[1]) == 0 and torch.equal(keep, pre_s) and float(out_n[0]) == float(out[0])
        assert float((gd_n.cpu().double() - r64n[2].reshape(-1)).abs().max()) <= bdn[0]
        out_n2, gd_n2, gs_n2 = run_kernel(rgb, depth, None, mask, P, p)
        assert gs_n2 is None and torch.equal(out_n2, out_n) and torch.equal(gd_n2, gd_n)


@gpu
def test_smooth_op_without_patches_launches_nothing():
    from snerf_amd import ops
    e = torch.empty(0, device="cuda")
    total = torch.full((1,), 2.0, device="cuda")
    out, gd, gs = ops.zip_smooth_loss(e.view(0, 3), e, e.view(0, 19), None, 0, 6, total=total)
    assert float(out.abs().max()) == 0 and gd.numel() == 0 and gs.numel() == 0 and float(total) == 2.0


# ---- GPU: the batcher -----------------------------------------------------------------------------------------------------------------
H_, W_, N_ = 24, 40, 3


def _scene(u8, seed=0):
    from test_device_batcher import _zip_scene
    return _zip_scene(N=N_, H=H_, W=W_, u8=u8, seed=seed)


def _batcher(sc, p, batch_size, border, seed=5, rank=0, world=1, batching="all_images"):
    from snerf_amd import zipnerf
    kw = dict(depths=sc["depths"], semantics=sc["semantics"], masks=sc["masks"], local2global=sc["local2global"], batch_size=batch_size, border=border,
              batching=batching, seed=seed, rank=rank, world=world, device="cuda")
    if p == 1:
        return zipnerf.RayBatcher(sc["images"], sc["pixtocams"], sc["camtoworlds"], 0.02, 100.0, **kw)
    return zipnerf.PatchRayBatcher(sc["images"], sc["pixtocams"], sc["camtoworlds"], 0.02, 100.0, p, **kw)


@gpu
@pytest.mark.parametrize("p,k,border,u8", [(2, 5, 0, True), (2, 3, 3, False), (6, 2, 0, False), (6, 3, 3, True)])
def test_patch_batcher_rows_are_the_documented_patches_then_the_pixel_batch(p, k, border, u8):
    from snerf_amd import ops
    sc = _scene(u8)
    n, pp, seed = 4 * p * p * k, p * p, 5
    b, plain = _batcher(sc, p, n, border), _batcher(sc, 1, n, border)
    assert (b.n_patch, b.n_patch_local, b.n_patch_rows, b.rows) == (k, k, k * pp, n) and b.patch_size == p
    buf = b.buffers()
    assert all(v.shape[0] == n for v in buf.values())
    prev = None
    for s in range(3):
        bt, pl = b.next(), plain.next()
        x, y, cam = (bt[key].cpu().numpy() for key in ("pix_x_int", "pix_y_int", "cam_idx"))
        cam = cam[:, 0].astype(np.int64)
        # the patch corners: the bounded draw of the patch's first row
        first = np.arange(k) * pp
        x0, y0 = border + np_bounded(first, 1, s, W_ - 2 * border - p + 1, seed), border + np_bounded(first, 2, s, H_ - 2 * border - p + 1, seed)
        c0 = np_bounded(first, 0, s, N_, seed)
        dy, dx = np.divmod(np.arange(pp), p)
        assert np.array_equal(x[:k * pp].reshape(k, pp), x0[:, None] + dx[None]) and np.array_equal(y[:k * pp].reshape(k, pp), y0[:, None] + dy[None])
        assert np.array_equal(cam[:k * pp].reshape(k, pp), np.broadcast_to(c0[:, None], (k, pp)))
        assert x[:k * pp].min() >= border and x[:k * pp].max() < W_ - border and y[:k * pp].min() >= border and y[:k * pp].max() < H_ - border
        # the pixel rows: those of the single-pixel batcher, bit for bit
        for key, v in pl.items():
            assert torch.equal(bt[key][k * pp:], v[k * pp:]), (s, key)
        # every row: the rays of its pixel, the targets gathered
        want = ops.zip_pixels_to_rays(bt["pix_x_int"], bt["pix_y_int"], bt["cam_idx"][:, 0].int().contiguous(), torch.from_numpy(sc["pixtocams"]).cuda(),
                                      torch.from_numpy(sc["camtoworlds"]).cuda(), want_imageplane=True)
        for key, v in want.items():
            assert torch.equal(bt[key], v), (s, key)
        ref = sc["images"][cam, y, x]
        assert np.array_equal(bt["rgb"].cpu().numpy(), (ref / 255.).astype(np.float32) if u8 else ref)
        assert np.array_equal(bt["depth"].cpu().numpy(), sc["depths"][cam, y, x]) and np.array_equal(bt["mask"].cpu().numpy(), sc["masks"][cam, y, x])
        assert np.array_equal(bt["semantic"].cpu().numpy(), sc["semantics"][cam, y, x]) and bt["semantic"].dtype == torch.int32
        assert np.array_equal(bt["glo_idx"][:, 0].cpu().numpy(), sc["local2global"][cam].astype(np.float32))
        assert float(bt["lossmult"].min()) == 1.0 == float(bt["lossmult"].max())
        assert prev is None or not torch.equal(prev, bt["pix_x_int"])                    # two draws differ
        prev = bt["pix_x_int"]
    assert b.step == 3 and b.counter.tolist() == [3, 0]
    one = _batcher(sc, p, n, border, batching="single_image")
    for s in range(2):
        cam = one.next()["cam_idx"]
        assert torch.equal(cam, torch.full_like(cam, float(np_bounded([0], 0, s, N_, seed)[0])))


@gpu
@pytest.mark.parametrize("p,k", [(2, 5), (6, 3)])
def test_patch_batcher_ranks_make_the_single_gpu_batch(p, k):
    sc = _scene(False)
    n, pp = 4 * p * p * k, p * p
    full = _batcher(sc, p, n, 3)
    parts = [_batcher(sc, p, n, 3, rank=r, world=2) for r in range(2)]
    assert sum(q.n_patch_local for q in parts) == k and sum(q.rows for q in parts) == n and all(q.n_patch == k for q in parts)
    for _ in range(2):
        want, got = full.next(), [q.next() for q in parts]
        for key, v in want.items():
            patches = torch.cat([g[key][:q.n_patch_rows] for g, q in zip(got, parts)])
            pixels = torch.cat([g[key][q.n_patch_rows:] for g, q in zip(got, parts)])
            assert torch.equal(torch.cat([patches, pixels]), v), key


# ---- GPU: the trainer -----------------------------------------------------------------------------------------------------------------
P_SZ, N_PATCH, N_PIX = 4, 2, 24
ROWS = N_PATCH * P_SZ * P_SZ
R_ALL = ROWS + N_PIX
LR, EPS = 1e-2, 1.0      # eps far above the gradients: Adam's first step is then lr * g / (|g| + eps), proportional to the gradient -- an
#                          update that shows a gradient's size and not only its sign (with a tiny eps it is lr * sign(g))


@pytest.fixture(scope="module")
def scene():
    """the small model's parameters, a batch of R_ALL rays whose first ROWS rows stand for the patches, targets, a patch mask, draws"""
    from test_zip_paths import zip_setup
    specs, p = zip_setup()
    g = torch.Generator().manual_seed(9)
    R = R_ALL
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    bx = torch.nn.functional.normalize(torch.cross(d, torch.randn(R, 3, generator=g), dim=-1), dim=-1)
    batch = dict(origins=torch.randn(R, 3, generator=g) * 0.1, directions=d, viewdirs=d, radii=2e-3 + 2e-3 * torch.rand(R, 1, generator=g),
                 near=torch.full((R, 1), 0.1), far=torch.full((R, 1), 10.0), base_x=bx, base_y=torch.nn.functional.normalize(torch.cross(d, bx, dim=-1), dim=-1))
    lm = (torch.rand(R, generator=g) < 0.8).float()
    tg = dict(lossmult=lm, depth=torch.rand(R, generator=g) * 5 + 0.5, depth_mask=lm * (torch.rand(R, generator=g) < 0.6), complete_mask=(1 - lm) * 1.0,
              semantic=torch.randint(0, 19, (R,), generator=g).int(), semantic_mask=lm.clone())
    assert all(float(tg[k][ROWS:].sum()) > 0 for k in ("lossmult", "depth_mask", "complete_mask", "semantic_mask"))    # every term has pixel rows
    return dict(p=p, batch=batch, target=torch.rand(R, 3, generator=g), targets=tg, patch_mask=(torch.rand(ROWS, generator=g) < 0.3).float())


def _setup(scene, semantic=True, deterministic=False, **trainer_kw):
    import test_zip_paths
    from snerf_amd.trainer import ZipTrainer
    test_zip_paths.DEV = "cuda"
    torch.manual_seed(3)                               # (the semantic head is not among the formula parameters: the same initial values every time)
    m = test_zip_paths.make_model("f32", "f32", scene["p"], use_semantic=semantic)
    if deterministic:                                  # the networks' weight gradients folded in a fixed order instead of by fp32 atomics
        m.set_deterministic(True)
    tr = ZipTrainer(m, lr=LR, eps=EPS, **trainer_kw)
    cu = lambda d: {k: v.cuda() for k, v in d.items()}
    draws = m._draws(R_ALL, False, m.arena.flat.device, 7)
    return m, tr, cu(scene["batch"]), scene["target"].cuda(), cu(scene["targets"]), scene["patch_mask"].cuda(), draws


def _total(last_losses):
    return last_losses[0] + last_losses[2:].sum()      # ops.ZIP_LOSS_NAMES + hash_decay, without the mse that is reported only


@gpu
def test_trainer_patch_terms_join_the_loss(scene):
    """(a) last_smooth_losses is the float64 restatement on that step's NeRF-level depth and semantic outputs; the loss is the sum"""
    m, tr, batch, target, tg, pm, draws = _setup(scene)
    before = {k: v.clone() for k, v in tg.items()}
    loss, levels = tr.step(batch, target, rand=False, draws=draws, targets=tg, n_patch=N_PATCH, patch_size=P_SZ, patch_mask=pm)
    fin = levels[2]
    shape = (N_PATCH, P_SZ, P_SZ)
    d64, s64, _, _, nx, ny = smooth_terms(target[:ROWS].reshape(*shape, 3), fin["depth"][:ROWS].reshape(shape), fin["semantic"][:ROWS].reshape(*shape, -1),
                                          pm.reshape(shape), D_MULT, S_MULT, torch.float64)
    got = tr.last_smooth_losses.cpu().tolist()
    print(f"trainer: d_smo {got[0]:.9e} (float64 {float(d64):.9e}), s_smo {got[1]:.9e} (float64 {float(s64):.9e}), Nx {nx} Ny {ny}")
    assert nx > 0 and ny > 0 and float(d64) > 0 and float(s64) > 0
    assert abs(got[0] - float(d64)) <= 2e-5 * float(d64) and abs(got[1] - float(s64)) <= 2e-5 * float(s64)
    assert tr.last_losses.numel() == 8
    want = float(_total(tr.last_losses)) + got[0] + got[1]
    assert abs(float(loss) - want) <= 4 * float(np.spacing(np.float32(want)))
    assert all(torch.equal(tg[k], before[k]) for k in tg)                                # the caller's targets are not written


@gpu
def test_trainer_patch_rows_leave_the_per_ray_terms(scene):
    """(b) with both multipliers 0 the step is the step without patches whose targets were masked on the patch rows by hand: `loss` and
    `last_losses` have equal bits (the hash decay, whose value is a sum by atomics in no fixed order, is switched off; the tail's terms
    are sums inside one workgroup at this size).  Three sets of targets: all of them; without lossmult; labels alone -- the loss tail
    reads an absent lossmult, and an absent semantic_mask beside labels, as 1 on every row, so the trainer has to make both.  The
    parameter update is held to the deviation of the hand-masked step from its own repetition (existing code only), x 2; the steps
    run with set_deterministic (weight gradients folded in a fixed order), so that deviation is expected to be 0."""
    ones = lambda: torch.ones(R_ALL, device="cuda")
    cases = {"all": lambda tg: (tg, tg),
             "no lossmult": lambda tg: ({k: v for k, v in tg.items() if k != "lossmult"}, dict(tg, lossmult=ones())),
             "labels alone": lambda tg: (dict(semantic=tg["semantic"]), dict(semantic=tg["semantic"], semantic_mask=ones(), lossmult=ones()))}
    first = None
    for name, pick in cases.items():
        res = {}
        for mode in ("patch", "hand", "hand again"):
            m, tr, batch, target, tg, pm, draws = _setup(scene, deterministic=True, loss_cfg=dict(d_smo_mult=0.0, s_smo_mult=0.0, hash_decay_mult=0.0))
            given, by_hand = pick(tg)
            start = m.arena.flat.clone()
            if mode == "patch":
                loss, _ = tr.step(batch, target, rand=False, draws=draws, targets=given, n_patch=N_PATCH, patch_size=P_SZ, patch_mask=pm)
                assert tr.last_smooth_losses.tolist() == [0.0, 0.0]
            else:
                hand = {k: v.clone() for k, v in by_hand.items()}
                for k in ("lossmult", "depth_mask", "complete_mask", "semantic_mask"):
                    if k in hand:
                        hand[k][:ROWS] = 0
                loss, _ = tr.step(batch, target, rand=False, draws=draws, targets=hand)
            res[mode] = (loss.clone(), tr.last_losses.clone(), (m.arena.flat - start).clone())
        (la, ta, ua), (lb, tb, ub), (lc, tc, uc) = res["patch"], res["hand"], res["hand again"]
        own = float((ub - uc).abs().max())
        print(f"targets {name}: the hand-masked step differs from its repetition by {own:.3e} in the update, the patch step from it by "
              f"{float((ua - ub).abs().max()):.3e}; largest update {float(ub.abs().max()):.3e}")
        assert torch.equal(la, lb) and torch.equal(ta, tb), (name, ta.tolist(), tb.tolist())
        assert float((ua - ub).abs().max()) <= 2 * own and float(ub.abs().max()) > 0
        first = first or res["patch"]
        if name == "labels alone":
            assert float(ta[4]) > 0                                                      # the semantic term is on
    # and the patch rows did carry targets: the unmasked step differs
    m, tr, batch, target, tg, pm, draws = _setup(scene, loss_cfg=dict(hash_decay_mult=0.0))
    tr.step(batch, target, rand=False, draws=draws, targets=tg)
    assert all(float(tr.last_losses[i]) != float(first[1][i]) for i in (0, 2, 4))
    m, tr, batch, target, tg, pm, draws = _setup(scene, loss_cfg=dict(hash_decay_mult=0.0))
    tr.step(batch, target, rand=False, draws=draws, targets=dict(semantic=tg["semantic"]))
    assert float(tr.last_losses[4]) != float(ta[4])                                     # labels alone: every row counts without patches


def _autograd_step(scene, patch, semantic=True):
    """one step through the model's autograd path: Model under grad mode, every term of the step in torch, loss.backward(),
    torch.optim.Adam -> the parameter update"""
    from oracle import callers as ocl
    m, _, batch, target, tg, pm, draws = _setup(scene, semantic=semantic)
    start = m.arena.flat.clone()
    opt = torch.optim.Adam(m.parameters(), lr=LR, betas=(0.9, 0.99), eps=EPS)
    rend, hist = m(False, batch, 1.0, False, draws=draws)
    fin = rend[-1]
    lm = tg["lossmult"].clone()
    masks = {k: tg[k].clone() for k in ("depth_mask", "complete_mask", "semantic_mask")}
    if patch:
        lm[:ROWS] = 0
        for v in masks.values():
            v[:ROWS] = 0
    loss = (lm[:, None] * torch.sqrt((fin["rgb"] - target) ** 2 + 0.001 ** 2)).sum() / (3 * lm.sum())
    e = (1 / (fin["depth"] + 1e-5) - 1 / (1e-5 + tg["depth"])).abs()
    loss = loss + 0.5 * (masks["depth_mask"] * e).sum() / masks["depth_mask"].sum() + 0.5 * 0.2 * (masks["complete_mask"] * e).sum() / masks["complete_mask"].sum()
    if semantic:
        pick = fin["semantic"][torch.arange(R_ALL, device="cuda"), tg["semantic"].long()]
        loss = loss - 0.04 * (masks["semantic_mask"] * torch.log(pick + 1e-6)).sum() / masks["semantic_mask"].sum()
    # anti-interlevel: the resampled NeRF histogram is a constant (float64 numpy, the oracle's); the gradient reaches the proposal weights only
    n = lambda t: t.detach().cpu().numpy()
    c, w = n(hist[2]["sdist"]).astype(np.float64), n(hist[2]["weights"]).astype(np.float64)
    wn = w / (c[..., 1:] - c[..., :-1])
    for i, r in enumerate((0.03, 0.003)):
        c_, w_ = ocl.blur_stepfun(n(hist[2]["sdist"]), wn, r)
        area = 0.5 * (w_[..., 1:] + w_[..., :-1]) * (c_[..., 1:] - c_[..., :-1])
        cdf = np.concatenate([np.zeros_like(area[..., :1]), np.cumsum(area, -1)], -1)
        ws = torch.from_numpy(np.diff(ocl.sorted_interp_quad(n(hist[i]["sdist"]).astype(np.float64), c_, w_, cdf), axis=-1)).float().cuda()
        wp = hist[i]["weights"]
        loss = loss + 0.01 * (torch.clamp(ws - wp, min=0) ** 2 / (wp + 1e-5)).mean()
    t, w2 = hist[2]["sdist"].detach(), hist[2]["weights"]
    ut = (t[:, 1:] + t[:, :-1]) / 2
    inter = (w2 * (w2[:, None, :] * (ut[:, :, None] - ut[:, None, :]).abs()).sum(-1)).sum(-1)
    loss = loss + 0.005 * (inter + (w2 ** 2 * (t[:, 1:] - t[:, :-1])).sum(-1) / 3).mean()
    named = dict(m.named_parameters())
    for i, pre in enumerate(m.names):                                                   # hash decay: mean over (level, channel) of the level's mean square
        tab, off = named[pre + "encoder.embeddings"], m.encs[i].offsets
        loss = loss + 0.1 * torch.stack([(tab[off[l]:off[l + 1]] ** 2).mean(0) for l in range(len(off) - 1)]).mean()
    if patch:
        shape = (N_PATCH, P_SZ, P_SZ)
        ok = ~(pm.reshape(shape) > 0)
        ok_x, ok_y = ok[:, :, :-1] & ok[:, :, 1:], ok[:, :-1] & ok[:, 1:]
        rgb = target[:ROWS].reshape(*shape, 3)
        w_x, w_y = torch.exp(-(rgb[:, :, :-1] - rgb[:, :, 1:]).abs().mean(-1)), torch.exp(-(rgb[:, :-1] - rgb[:, 1:]).abs().mean(-1))

        def term(z, eps):
            z = z / (z.mean((1, 2), keepdim=True) + eps)
            return ((z[:, :, :-1] - z[:, :, 1:]).abs().sum(-1) * w_x)[ok_x].mean() + ((z[:, :-1] - z[:, 1:]).abs().sum(-1) * w_y)[ok_y].mean()
        loss = loss + D_MULT * term((1 / (fin["depth"][:ROWS].reshape(*shape, 1) + 1e-5)), 1e-7)
        if semantic:
            loss = loss + S_MULT * term(fin["semantic"][:ROWS].reshape(*shape, -1), 1e-5)
    loss.backward()
    opt.step()
    return float(loss.detach()), (m.arena.flat.detach() - start).clone()


def _fused_step(scene, patch, semantic=True, **trainer_kw):
    m, tr, batch, target, tg, pm, draws = _setup(scene, semantic=semantic, **trainer_kw)
    start = m.arena.flat.clone()
    kw = dict(n_patch=N_PATCH, patch_size=P_SZ, patch_mask=pm) if patch else {}
    loss, _ = tr.step(batch, target, rand=False, draws=draws, targets=tg, **kw)
    return float(loss), (m.arena.flat - start).clone(), tr


@gpu
def test_trainer_patch_gradients_follow_the_autograd_route(scene):
    """(c) one fused step with the patch terms against the same step through Model + torch autograd + torch.optim.Adam.  The allowed
    deviation is measured: the same comparison with the patch terms off (existing code only), x 2, + 4 fp32 ulp of the largest update"""
    dev = {}
    for patch in (False, True):
        la, ua = _autograd_step(scene, patch)
        lf, uf, _ = _fused_step(scene, patch)
        dev[patch] = (float((ua - uf).abs().max()), float(ua.abs().max()), la, lf)
        assert abs(la - lf) <= 2e-5 * abs(la), (patch, la, lf)
    _, u_off, _ = _fused_step(scene, True, loss_cfg=dict(d_smo_mult=0.0, s_smo_mult=0.0))
    _, u_on, _ = _fused_step(scene, True)
    moved = float((u_on - u_off).abs().max())
    allowed = 2 * dev[False][0] + 4 * float(np.spacing(np.float32(dev[True][1])))
    print(f"autograd route: deviation without the patch terms {dev[False][0]:.3e}, with them {dev[True][0]:.3e}, allowed {allowed:.3e}; largest update "
          f"{dev[True][1]:.3e}; the two patch terms move the update by {moved:.3e}")
    assert dev[True][0] <= allowed
    assert moved > 10 * allowed                        # the comparison can see the terms


@gpu
def test_trainer_patch_terms_without_a_semantic_head(scene):
    """(d) no semantic head: s_smo = 0, the depth term as it is"""
    m, tr, batch, target, tg, pm, draws = _setup(scene, semantic=False)
    loss, levels = tr.step(batch, target, rand=False, draws=draws, targets=tg, n_patch=N_PATCH, patch_size=P_SZ, patch_mask=pm)
    shape = (N_PATCH, P_SZ, P_SZ)
    d64 = smooth_terms(target[:ROWS].reshape(*shape, 3), levels[2]["depth"][:ROWS].reshape(shape), None, pm.reshape(shape), D_MULT, S_MULT, torch.float64)[0]
    got = tr.last_smooth_losses.cpu().tolist()
    assert got[1] == 0.0 and abs(got[0] - float(d64)) <= 2e-5 * float(d64) and float(d64) > 0 and np.isfinite(float(loss))
    # without depth targets the tail has no depth gradient: the term brings its own buffer
    m, tr, batch, target, tg, pm, draws = _setup(scene, semantic=True)
    start = m.arena.flat.clone()
    loss, _ = tr.step(batch, target, rand=False, draws=draws, n_patch=N_PATCH, patch_size=P_SZ)
    assert np.isfinite(float(loss)) and float(tr.last_smooth_losses[0]) > 0 < float(tr.last_smooth_losses[1])
    m2, tr2, *_ = _setup(scene, semantic=True, loss_cfg=dict(d_smo_mult=0.0, s_smo_mult=0.0))
    start2 = m2.arena.flat.clone()
    tr2.step(batch, target, rand=False, draws=draws, n_patch=N_PATCH, patch_size=P_SZ)
    assert float(((m.arena.flat - start) - (m2.arena.flat - start2)).abs().max()) > 0


@gpu
def test_trainer_patch_terms_carry_the_loss_scale(scene):
    """(e) loss_scale = 4096 moves the parameters like loss_scale = 1: within twice the deviation of the same pair without the terms.
    Both pairs run with set_deterministic: the fp32 atomics of the networks' weight gradients otherwise add in an order that varies
    from run to run, and a pair without the terms that happens to agree to the bit then leaves no room for a pair with them that does
    not.  A factor of 4096 is exact in every fixed-order sum, so both deviations are expected to be 0."""
    dev = {}
    for patch in (False, True):
        l1, u1, _ = _fused_step(scene, patch, deterministic=True, loss_scale=1.0)
        l2, u2, tr = _fused_step(scene, patch, deterministic=True, loss_scale=4096.0)
        assert tr.loss_scale == 4096.0 and abs(l1 - l2) <= 1e-6 * abs(l1)
        dev[patch] = (float((u1 - u2).abs().max()), float(u1.abs().max()))
    print(f"loss scale 4096 vs 1: deviation without the patch terms {dev[False][0]:.3e}, with them {dev[True][0]:.3e}; largest update {dev[True][1]:.3e}")
    assert dev[True][0] <= 2 * dev[False][0]


@gpu
def test_trainer_refuses_inconsistent_patch_arguments(scene):
    """(f)"""
    m, tr, batch, target, tg, pm, draws = _setup(scene)
    start = m.arena.flat.clone()
    step = lambda **kw: tr.step(batch, target, rand=False, draws=draws, targets=tg, **kw)
    for kw in (dict(n_patch=N_PATCH), dict(n_patch=N_PATCH, patch_size=P_SZ, patch_mask=pm[:-1]), dict(n_patch=4, patch_size=P_SZ),
               dict(n_patch=1, patch_size=8), dict(n_patch=-1, patch_size=P_SZ), dict(n_patch=N_PATCH, patch_size=1), dict(n_patch=1, patch_size=33),
               dict(patch_mask=pm), dict(n_patch=0, patch_size=P_SZ, patch_mask=pm)):
        with pytest.raises(ValueError):
            step(**kw)
    assert torch.equal(m.arena.flat, start) and tr.t == 0
    step(n_patch=0, patch_size=P_SZ)                                                     # no patches: the plain step
    assert tr.last_smooth_losses is None and tr.t == 1
    step(n_patch=N_PATCH, patch_size=P_SZ, patch_mask=pm)
    assert tr.last_smooth_losses is not None and tr.t == 2
    step(n_patch=0, patch_size=P_SZ, patch_mask=pm[:0])                                  # a rank without patches: its mask slice is empty
    assert tr.last_smooth_losses is None and tr.t == 3                                   # nothing stale left for a logger
    step(n_patch=N_PATCH, patch_size=P_SZ, patch_mask=pm)
    step()
    assert tr.last_smooth_losses is None and tr.t == 5


# ---- GPU: captured ----------------------------------------------------------------------------------------------------------------------
@gpu
def test_captured_draw_and_patch_terms_replay_the_eager_ones():
    """one capture of PatchRayBatcher.next_into + ops.zip_smooth_loss on the drawn patches, replayed twice: the batches advance and every
    result has the eager bits"""
    from snerf_amd import ops
    sc = _scene(False)
    sc["masks"] = 1 - sc["masks"]                                                        # about 30 % of the pixels masked out
    p, k, C = 6, 2, 19
    n, rows = 4 * p * p * k, p * p * k
    cap, eager = _batcher(sc, p, n, 3), _batcher(sc, p, n, 3)
    gen = torch.Generator().manual_seed(4)
    depth = (torch.rand(rows, generator=gen) * 39.5 + 0.5).cuda()
    sem = torch.softmax(torch.randn(rows, C, generator=gen), -1).cuda()
    buf, out, total = cap.buffers(), torch.zeros(4, device="cuda"), torch.zeros(1, device="cuda")
    gd, gs = torch.zeros(rows, device="cuda"), torch.zeros(rows, C, device="cuda")
    ws = torch.empty(ops.zip_smooth_loss_ws(k), dtype=torch.float64, device="cuda")

    def work(b, bf):
        b.next_into(bf)
        ops.zip_smooth_loss(bf["rgb"][:rows], depth, sem, bf["mask"][:rows], k, p, out=out, total=total, g_depth=gd, g_sem=gs, accumulate=True, ws=ws)
    work(cap, buf)                                                                       # (loads the kernels outside the capture)
    cap.load_state_dict({"seed": 5, "step": 0})
    for t in (total, gd, gs):
        t.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        work(cap, buf)
    want_total, want_gd, want_gs = torch.zeros(1, device="cuda"), torch.zeros(rows, device="cuda"), torch.zeros(rows, C, device="cuda")
    seen = []
    for s in range(2):
        g.replay()
        bt = eager.next()
        w_out, _, _ = ops.zip_smooth_loss(bt["rgb"][:rows], depth, sem, bt["mask"][:rows], k, p, total=want_total, g_depth=want_gd, g_sem=want_gs, accumulate=True)
        assert all(torch.equal(buf[key], bt[key]) for key in bt), s
        assert torch.equal(out, w_out) and torch.equal(total, want_total) and torch.equal(gd, want_gd) and torch.equal(gs, want_gs), s
        assert float(out[0]) > 0 and float(out[1]) > 0 and float(out[2]) > 0 and float(out[3]) > 0
        seen.append(bt["pix_x_int"].clone())
    assert not torch.equal(seen[0], seen[1]) and cap.counter.tolist() == [2, 0]
