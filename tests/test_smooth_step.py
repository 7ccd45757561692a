"""The edge-aware smooth loss inside the fused mip step: the patch draw of the device batcher (snerf_mip_image_patch_batch /
sample_utils.PatchRayBatcher), the loss kernel (snerf_smooth_loss / ops.smooth_loss) and MipTrainer's smooth term, eager and captured.
The draw is restated here in numpy from the algorithm documented in csrc/callers.hip; the loss and its gradient are held against
sample_utils.smooth_loss (the torch form the reference's golden g32 pins) evaluated in float64."""
import os
import types

import numpy as np
import pytest
import torch

from snerf_amd import _lib

gpu = pytest.mark.gpu
M32 = np.uint64(0xFFFFFFFF)


# ---- numpy restatement of the bounded draw --------------------------------------------------------------------------------------------
def np_philox(c0, c1, c2, c3, seed):
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, dtype=np.uint64) & M32 for c in (c0, c1, c2, c3)))
    c0, c1, c2, c3 = (c.copy() for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = c0 * np.uint64(0xD2511F53), c2 * np.uint64(0xCD9E8D57)
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0


def np_centres(s, seed, H, W, p, n_patch):
    """centre k of step s: Lemire's bounded integer over the (H - 2p - 1)(W - 2p - 1) interior pixels on the counter
    (k, 3 << 16 | 3 << 8 | attempt, lo32(s), hi32(s)), row-major in that window"""
    hr, wc = H - 2 * p - 1, W - 2 * p - 1
    rng = hr * wc
    thresh = (2 ** 32 - rng) % rng
    idx = []
    for k in range(n_patch):
        for a in range(256):
            m = int(np_philox(k, (3 << 16) | (3 << 8) | a, s & 0xFFFFFFFF, s >> 32, seed)) * rng
            if (m & 0xFFFFFFFF) >= thresh or a == 255:
                break
        idx.append(m >> 32)
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    return np.stack([p + 1 + idx // wc, p + 1 + idx % wc], -1)


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,seed,H,W,p", [(0, 0, 24, 40, 6), (7, 3, 24, 40, 8), (123456789012, 99, 37, 53, 6), (5, (1 << 63) - 1, 9, 70, 2),
                                          (19, 11, 200, 67, 32)])
def test_patch_centres_follow_the_documented_draw(s, seed, H, W, p):
    from snerf_amd import sample_utils as su
    n_patch = 9
    c = su.patch_centres_of_step(s, seed, H, W, p, n_patch)
    assert c.dtype == np.int64 and c.shape == (n_patch, 2)
    assert np.array_equal(c, np_centres(s, seed, H, W, p, n_patch))
    assert ((c[:, 0] > p) & (c[:, 0] < H - p) & (c[:, 1] > p) & (c[:, 1] < W - p)).all()
    # the layout half of sample_patches: np.random.randint made to return these centres
    px = su.patch_pixels(c, p)
    hr, wc = H - 2 * p - 1, W - 2 * p - 1
    idx = (c[:, 0] - p - 1) * wc + (c[:, 1] - p - 1)
    real = np.random.randint
    np.random.randint = lambda hi, size=None: idx.copy() if (hi, size) == (hr * wc, n_patch) else real(hi, size=size)
    try:
        want = su.sample_patches(H, W, p, n_patch)
    finally:
        np.random.randint = real
    assert np.array_equal(px, want) and px.shape == (n_patch * p * p, 2)
    assert px[:, 0].min() >= 0 and px[:, 0].max() < H and px[:, 1].min() >= 0 and px[:, 1].max() < W
    # a centre, its first and its last pixel
    assert tuple(px[0]) == (c[0, 0] - p // 2, c[0, 1] - p // 2) and tuple(px[p * p - 1]) == (c[0, 0] + p // 2 - 1, c[0, 1] + p // 2 - 1)
    assert tuple(px[1]) == (c[0, 0] - p // 2, c[0, 1] - p // 2 + 1)                       # rows outer


def test_patch_centres_depend_on_step_and_seed_only():
    from snerf_amd import sample_utils as su
    a = su.patch_centres_of_step(4, 3, 24, 40, 6, 50)
    assert np.array_equal(a[:7], su.patch_centres_of_step(4, 3, 24, 40, 6, 7))           # centre k does not depend on n_patch
    assert not np.array_equal(a, su.patch_centres_of_step(5, 3, 24, 40, 6, 50))
    assert not np.array_equal(a, su.patch_centres_of_step(4, 4, 24, 40, 6, 50))
    assert len({tuple(x) for x in a}) > 25                                              # drawn over the window, with replacement


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")


def _patch_args(**kw):
    a = dict(images=64, images_u8=0, depths=64, poses=64, intrinsics=64, near=64, far=64, app=64, extras=None, n_extra=0, i_train=64,
             n_train=2, N=3, H=24, W=40, seed=0, counter=64, n=16, i0=0, i1=16, origins=64, directions=64, viewdirs=64, radii=64,
             lossmult=64, near_out=64, far_out=64, app_out=64, rgb=64, depth=64, extras_out=None, sel_coords=64, img_out=64, n_patch=4,
             patch_sz=6, k0=0, k1=4, stream=None)
    a.update(kw)
    return list(a.values())


def _smooth_args(**kw):
    a = dict(rgb=64, dist=64, sky=None, P=3, p=6, weight=0.1, ws=64, ws_doubles=6, out=64, total=None, g_dist=64, accumulate=0, stream=None)
    a.update(kw)
    return list(a.values())


def test_new_entries_reject_bad_arguments_without_a_gpu():
    """argument validation happens before any launch (the pointers here are never dereferenced)"""
    _lib_or_skip()
    bad_patch = [dict(patch_sz=5), dict(patch_sz=7), dict(patch_sz=0), dict(patch_sz=1), dict(patch_sz=34), dict(patch_sz=-2),
                 dict(H=13), dict(W=13), dict(patch_sz=12, H=24), dict(H=70000, W=70000, patch_sz=2, n=16),       # range < 1, >= 2^32
                 dict(n_patch=-1, k0=0, k1=0), dict(k0=-1), dict(k0=3, k1=2), dict(k1=5), dict(n_patch=0, k0=0, k1=1),
                 # and what snerf_mip_image_batch refuses
                 dict(images=None), dict(N=0), dict(n_train=0), dict(i1=17), dict(i0=5, i1=4), dict(n=-1), dict(counter=None), dict(origins=None),
                 dict(n_extra=1), dict(images_u8=2), dict(depths=None), dict(n_patch=0, k0=0, k1=0, images=None)]
    for kw in bad_patch:
        with pytest.raises(_lib.SnerfHipError, match="bad argument"):
            _lib.call("snerf_mip_image_patch_batch", *_patch_args(**kw))
    bad_smooth = [dict(ws_doubles=5), dict(ws=None), dict(rgb=None), dict(dist=None), dict(out=None), dict(g_dist=None), dict(p=1), dict(p=0),
                  dict(p=33), dict(p=-6), dict(P=-1), dict(accumulate=2)]
    for kw in bad_smooth:
        with pytest.raises(_lib.SnerfHipError, match="bad argument"):
            _lib.call("snerf_smooth_loss", *_smooth_args(**kw))
    # no patches and no pixels, and no patches to smooth, are no-ops whatever the rest
    none_patch = [None if isinstance(v, int) and v == 64 else v for v in _patch_args(n=0, i1=0, n_patch=0, k1=0)]
    none_smooth = [None if isinstance(v, int) and v == 64 else v for v in _smooth_args(P=0, ws_doubles=0)]
    assert _lib.call("snerf_mip_image_patch_batch", *none_patch) is None
    assert _lib.call("snerf_smooth_loss", *none_smooth) is None
    assert [_lib.query("snerf_smooth_loss_ws", P) >= 0 for P in (-3, 0)] == [True, True] and _lib.query("snerf_smooth_loss_ws", 0) == 0
    assert _lib.query("snerf_smooth_loss_ws", 70) >= 2 * 70


def test_patch_batcher_constructor_rejects_what_it_cannot_draw():
    """checked before anything touches a device"""
    from snerf_amd import sample_utils as su
    args = types.SimpleNamespace(no_ndc=True, smooth_loss=True, near_far=False, N_rgb=16, N_patch=3, patch_sz=6)
    img, dep = np.zeros((2, 24, 40, 3), np.float32), np.ones((2, 24, 40), np.float32)
    pose, K = np.tile(np.eye(4, dtype=np.float32)[:3], (2, 1, 1)), np.tile(np.eye(3, dtype=np.float32), (2, 1, 1))
    mk = lambda a=args, images=img, **kw: su.PatchRayBatcher(a, images, dep, pose, K, [0, 1], 1.0, 10.0, device="cuda", **kw)
    for kw in (dict(patch_sz=5), dict(patch_sz=0), dict(patch_sz=34), dict(n_patch=0), dict(n_patch=-2), dict(patch_sz=12),
               dict(images=np.zeros((2, 13, 40, 3), np.float32))):
        with pytest.raises(ValueError):
            mk(**kw)
    with pytest.raises(ValueError):
        mk(types.SimpleNamespace(no_ndc=True, smooth_loss=True, near_far=False, N_rgb=16, N_patch=3, patch_sz=7))
    with pytest.raises(NotImplementedError):
        mk(types.SimpleNamespace(no_ndc=False, smooth_loss=True, near_far=False, N_rgb=16, N_patch=3, patch_sz=6), images=img)
    assert issubclass(su.PatchRayBatcher, su.ImageRayBatcher)


# ---- GPU: the batcher -------------------------------------------------------------------------------------------------------------------
N_SC, H_SC, W_SC, I_TRAIN = 5, 24, 40, (0, 1, 3, 4)


def _scene(u8=False, seed=0):
    rng = np.random.default_rng(seed)
    images = rng.integers(0, 256, size=(N_SC, H_SC, W_SC, 3), dtype=np.uint8) if u8 else rng.random((N_SC, H_SC, W_SC, 3), dtype=np.float32)
    depths = (rng.random((N_SC, H_SC, W_SC)) * 4 + 2).astype(np.float32)
    depths[rng.random((N_SC, H_SC, W_SC)) < 0.4] = 0
    poses = np.zeros((N_SC, 3, 4), np.float32)
    for i in range(N_SC):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        poses[i, :, :3], poses[i, :, 3] = q, rng.normal(size=3) * 0.1
    K = np.zeros((N_SC, 3, 3), np.float32)
    K[:, 0, 0], K[:, 1, 1] = rng.uniform(20, 30, N_SC), rng.uniform(20, 30, N_SC)
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = W_SC * rng.uniform(0.4, 0.6, N_SC), H_SC * rng.uniform(0.4, 0.6, N_SC), 1
    extras = [(rng.random((N_SC, H_SC, W_SC)) < 0.3).astype(np.float32), rng.random((N_SC, H_SC, W_SC), dtype=np.float32)]   # sky, a confidence
    return images, depths, poses, K, extras


def _batchers(n_patch, p, u8=False, n=300, seed=3, rank=0, world=1, plain=True):
    """-> (PatchRayBatcher, an ImageRayBatcher of the same seed or None, the scene)"""
    from snerf_amd import sample_utils as su
    sc = images, depths, poses, K, ex = _scene(u8)
    mk = lambda cls, smooth, **kw: cls(types.SimpleNamespace(no_ndc=True, smooth_loss=smooth, near_far=False, N_rgb=n, N_patch=n_patch, patch_sz=p),
                                       images, depths, poses, K, list(I_TRAIN), 2.0, 6.0, camera_index=np.arange(N_SC) * 10.0, extras=ex, seed=seed,
                                       rank=rank, world=world, device="cuda", **kw)
    return mk(su.PatchRayBatcher, True), (mk(su.ImageRayBatcher, False) if plain else None), sc


@gpu
@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("n_patch,p", [(5, 6), (3, 8)])
def test_patch_batcher_rows_are_the_image_batcher_plus_the_documented_patches(n_patch, p, u8):
    from snerf_amd import sample_utils as su
    b, plain, (images, depths, poses, K, ex) = _batchers(n_patch, p, u8)
    n = 300
    assert b.n_rgb_rows == n and b.n_patch_rows == n_patch * p * p and b.n_rows == n + n_patch * p * p
    seen = set()
    for s in range(20):
        rays, trgb, tdep, sel, img_t, extras = b.next()
        w_rays, w_rgb, w_dep, w_sel, w_img, w_ex = plain.next()
        img = int(img_t)
        seen.add(img)
        # the image and the pixel rows: turning patches on does not move them
        assert img == int(w_img) == b.image_of_step(s)
        for k in range(8):
            assert rays[k].shape[0] == b.n_rows and torch.equal(rays[k][:n], w_rays[k]), (s, k)
        assert torch.equal(trgb[:n], w_rgb) and torch.equal(tdep[:n], w_dep) and torch.equal(sel[:n], w_sel)
        assert all(torch.equal(a[:n], w) for a, w in zip(extras, w_ex)) and len(extras) == 2
        # the patch rows
        centres = su.patch_centres_of_step(s, 3, H_SC, W_SC, p, n_patch)
        assert np.array_equal(centres, np_centres(s, 3, H_SC, W_SC, p, n_patch)) and np.array_equal(centres, b.patch_centres_of_step(s))
        px = su.patch_pixels(centres, p)
        assert np.array_equal(sel[n:].cpu().numpy(), px), s
        want = su.rays_of_pixels(px, poses[img], K[img], H_SC, W_SC, 2.0 * 0.9, 6.0 * 1.1, training=True)
        for k in ("origins", "directions", "viewdirs", "radii", "lossmult", "near", "far"):
            assert torch.equal(getattr(rays, k)[n:], getattr(want, k)), (s, k)
        assert torch.equal(rays.app, torch.full_like(rays.app, img * 10.0))
        r, c = px[:, 0], px[:, 1]
        ref_rgb = images[img] if not u8 else (images[img] / 255.).astype(np.float32)
        assert np.array_equal(trgb[n:].cpu().numpy(), ref_rgb[r, c]) and np.array_equal(tdep[n:].cpu().numpy(), depths[img][r, c])
        for e_got, e_map in zip(extras, ex):
            assert np.array_equal(e_got[n:].cpu().numpy(), e_map[img][r, c])
    assert seen == set(I_TRAIN)


@gpu
def test_patch_entry_without_patches_is_the_image_batch_bit_for_bit():
    from snerf_amd import ops
    _, plain, _ = _batchers(3, 6)
    a, b = plain.buffers(), plain.buffers()
    for s in (0, 1, 9):
        plain.load_state_dict({"seed": 3, "step": s})
        plain.next_into(a)
        plain.load_state_dict({"seed": 3, "step": s})
        ops.mip_image_patch_batch(plain.images, plain.depths, plain.poses, plain.intrinsics, plain.near, plain.far, plain.app, plain.extras,
                                  plain.i_train, plain.seed, plain.counter, plain.batch_n, plain.i0, plain.i1, 0, 0, 0, 0, b)
        assert int(plain.counter[0]) == s + 1 and int(plain.counter[1]) == 0
        for k in a:
            assert torch.equal(a[k], b[k]), (s, k)


@gpu
@pytest.mark.parametrize("n_patch", [5, 2])
def test_patch_batcher_ranks_make_the_single_gpu_batch(n_patch):
    world, p, n = 3, 6, 300
    full = _batchers(n_patch, p, plain=False)[0]
    parts = [_batchers(n_patch, p, rank=r, world=world, plain=False)[0] for r in range(world)]
    assert sum(q.n_rgb_rows for q in parts) == n and sum(q.n_patch_rows for q in parts) == n_patch * p * p
    if n_patch == 2:
        assert parts[2].n_patch_rows == 0 and parts[2].n_rows == parts[2].n_rgb_rows == 100
    for _ in range(3):
        want = full.next()
        got = [q.next() for q in parts]
        for q, g in zip(parts, got):
            assert g[1].shape[0] == q.n_rows and g[3].shape[0] == q.n_rows
        cat = lambda f, w: (torch.equal(torch.cat([f(g)[:q.n_rgb_rows] for q, g in zip(parts, got)]), f(w)[:n]) and
                            torch.equal(torch.cat([f(g)[q.n_rgb_rows:] for q, g in zip(parts, got)]), f(w)[n:]))
        for k in range(8):
            assert cat(lambda g: g[0][k], want), k
        for j in (1, 2, 3):
            assert cat(lambda g: g[j], want), j
        for e in range(2):
            assert cat(lambda g: g[5][e], want), e
        assert all(int(g[4]) == int(want[4]) for g in got)


@gpu
def test_patch_batcher_counter_advances_once_per_draw_and_resumes():
    from snerf_amd import sample_utils as su
    b = _batchers(5, 6, plain=False)[0]
    px = lambda s: su.patch_pixels(su.patch_centres_of_step(s, 3, H_SC, W_SC, 6, 5), 6)
    b.next(); b.next()
    s = b.step
    assert s == 2 and int(b.counter[0]) == 2 and int(b.counter[1]) == 0
    x, y = b.next(), b.next()
    assert np.array_equal(x[3][300:].cpu().numpy(), px(s)) and np.array_equal(y[3][300:].cpu().numpy(), px(s + 1))
    assert int(b.counter[0]) == s + 2 and b.step == s + 2 and b.state_dict() == {"seed": 3, "step": s + 2}
    d = _batchers(5, 6, seed=99, plain=False)[0]
    d.load_state_dict({"seed": 3, "step": s})
    z = d.next()
    assert torch.equal(z[3], x[3]) and torch.equal(z[0].directions, x[0].directions) and torch.equal(z[1], x[1]) and int(z[4]) == int(x[4])


# ---- GPU: the kernel --------------------------------------------------------------------------------------------------------------------
def _yardstick(rgb, dist, sky, P, p, weight, dtype):
    """sample_utils.smooth_loss (the torch form) on patches given as arrays: the patches stacked into a (P p) x p image -> (loss, gradient)"""
    from snerf_amd import sample_utils as su
    img = rgb.detach().cpu().reshape(P * p, p, 3).to(dtype)
    sk = None if sky is None else sky.detach().cpu().reshape(P * p, p).to(dtype)
    rr, cc = torch.meshgrid(torch.arange(P * p), torch.arange(p), indexing="ij")
    d = dist.detach().cpu().reshape(-1).to(dtype).clone().requires_grad_(True)
    loss = su.smooth_loss(img, sk, torch.stack([rr, cc], -1).reshape(-1, 2), d, P, p, weight, use_skymask=sky is not None)
    loss.backward()
    return loss.detach(), d.grad


def _grad_bound(rgb, dist, sky, P, p, weight):
    """-> (float64 loss, float64 gradient, bound): 4 x the largest deviation of the fp32 torch evaluation from the float64 one plus 4 fp32
    ulp of max |g| -- computed from the references alone"""
    l64, g64 = _yardstick(rgb, dist, sky, P, p, weight, torch.float64)
    _, g32 = _yardstick(rgb, dist, sky, P, p, weight, torch.float32)
    gmax = float(g64.abs().max())
    dev32 = float((g32.double() - g64).abs().max())
    return l64, g64, 4 * dev32 + 4 * float(np.spacing(np.float32(gmax))), dev32, gmax


@gpu
def test_smooth_kernel_on_the_reference_golden(golden):
    from snerf_amd import ops
    g = golden("g32_smooth_patches")
    n_rgb, p, P = (int(g[k]) for k in ("N_rgb", "patch_sz", "N_patch"))
    sel = g["sel_coords"][n_rgb:]
    rgb, sky = g["image"][sel[:, 0], sel[:, 1]], g["skymask"][sel[:, 0], sel[:, 1]]
    assert torch.equal(rgb, g["target_rgb"][n_rgb:]) and (P, p) == (5, 6)
    dist, w = g["patch_distance"], float(g["smooth_lambda"])
    out, gd = ops.smooth_loss(rgb.cuda(), dist.cuda(), sky.cuda(), P, p, w)
    out2, gd2 = ops.smooth_loss(rgb.cuda(), dist.cuda(), sky.cuda(), P, p, w)
    assert torch.equal(out, out2) and torch.equal(gd, gd2)
    want = float(g["smooth_loss"])
    print(f"g32 loss: kernel {float(out[0]):.9e}, golden {want:.9e}, rel {abs(float(out[0]) - want) / want:.2e}")
    assert abs(float(out[0]) - want) <= 1e-6 * abs(want)
    l64, g64, bound, dev32, gmax = _grad_bound(rgb, dist, sky, P, p, w)
    err = float((gd.cpu().double() - g64).abs().max())
    print(f"g32 gradient: max |g| {gmax:.3e}, fp32 torch deviation {dev32:.3e}, bound {bound:.3e}, kernel error {err:.3e}")
    assert err <= bound and gmax > 0
    assert abs(float(out[0]) - float(l64)) <= 1e-6 * float(l64)
    assert abs(float(out[0]) - w * (float(out[1]) + float(out[2]))) <= 4 * float(np.spacing(np.float32(float(out[0])))) and float(out[1]) > 0 < float(out[2])


W_EDGE = float(np.float32(0.1))                       # the ABI takes the weight as a float: the same number on both sides


@gpu
@pytest.mark.parametrize("P", [1, 3, 70])
@pytest.mark.parametrize("p", [2, 8, 16, 32])
def test_smooth_kernel_edges(p, P):
    from snerf_amd import ops
    gen = torch.Generator().manual_seed(100 * p + P)
    pp = p * p
    rgb = torch.rand(P, p, p, 3, generator=gen)
    base = torch.rand(P, p, p, generator=gen) * 40 + 3                                   # distances in [3, 43]
    skies = {"none": None, "ones": torch.ones(P, p, p), "random": (torch.rand(P, p, p, generator=gen) < 0.4).float()}
    const = P - 1 if P >= 3 else None                                                    # a constant patch
    tiny, zero = (0, 1), ((1 if P >= 2 else 0), pp - 1)                                  # (patch, pixel) of the distances 1e-6 and 0
    for name, sky in skies.items():
        dist = base.clone()
        if const is not None:
            dist[const] = 7.25
        plain = dist.clone()                                                             # the same batch without the two tiny distances
        dist.view(P, pp)[tiny[0], tiny[1]] = 1e-6
        dist.view(P, pp)[zero[0], zero[1]] = 0.0
        cu = lambda t: None if t is None else t.cuda()
        out, g = ops.smooth_loss(cu(rgb), cu(dist), cu(sky), P, p, W_EDGE)
        l64, g64, bound, dev32, gmax = _grad_bound(rgb, dist, sky, P, p, W_EDGE)
        gh = g.cpu().view(P, pp)
        err = float((gh.double().view(-1) - g64).abs().max())
        print(f"p={p} P={P} sky={name}: max |g| {gmax:.3e}, fp32 torch deviation {dev32:.3e}, bound {bound:.3e}, kernel error {err:.3e}, "
              f"loss rel {abs(float(out[0]) - float(l64)) / float(l64):.2e}")
        assert bool(torch.isfinite(gh).all()) and bool(torch.isfinite(out).all())
        assert err <= bound and gmax > 0
        assert abs(float(out[0]) - float(l64)) <= 1e-6 * float(l64)                      # a float64 evaluation rounded once
        # torch's rules: nothing through the clamp, nothing from equal neighbours
        assert float(gh[tiny]) == 0 and float(gh[zero]) == 0 and float(g64.view(P, pp)[tiny]) == 0 and float(g64.view(P, pp)[zero]) == 0
        if const is not None:
            assert float(gh[const].abs().max()) == 0 and float(g64.view(P, pp)[const].abs().max()) == 0
        # the clamped pixels still enter their patch mean: the other pixels of those patches feel them
        out_plain, g_plain = ops.smooth_loss(cu(rgb), cu(plain), cu(sky), P, p, W_EDGE)
        gp = g_plain.cpu().view(P, pp)
        lp64, gp64, bound_p, dev_p, gmax_p = _grad_bound(rgb, plain, sky, P, p, W_EDGE)   # (ordinary distances everywhere: the same yardstick)
        err_p = float((gp.double().view(-1) - gp64).abs().max())
        print(f"    without the tiny distances: max |g| {gmax_p:.3e}, fp32 torch deviation {dev_p:.3e}, bound {bound_p:.3e}, kernel error {err_p:.3e}")
        assert err_p <= bound_p and abs(float(out_plain[0]) - float(lp64)) <= 1e-6 * float(lp64)
        for k, j in (tiny, zero):
            others = [i for i in range(pp) if i != j and not (k == tiny[0] == zero[0] and i in (tiny[1], zero[1]))]
            assert float((gh[k, others] - gp[k, others]).abs().max()) > 0
            assert float(gh[k, others].abs().max()) < float(gp[k, others].abs().max())   # a mean of ~1e5 / p^2 flattens the patch
        # two identical calls, accumulate, total, weight 0
        out2, g2 = ops.smooth_loss(cu(rgb), cu(dist), cu(sky), P, p, W_EDGE)
        assert torch.equal(out, out2) and torch.equal(g, g2)
        pre = torch.rand(P * pp, generator=gen).cuda() - 0.5
        acc, total = pre.clone(), torch.full((1,), 1.5, device="cuda")
        out3, g3 = ops.smooth_loss(cu(rgb), cu(dist), cu(sky), P, p, W_EDGE, total=total, g_dist=acc, accumulate=True)
        assert g3 is acc and torch.equal(acc, pre + g) and torch.equal(out3, out)
        assert torch.equal(total, torch.full((1,), 1.5, device="cuda") + out[0])
        over = pre.clone()
        ops.smooth_loss(cu(rgb), cu(dist), cu(sky), P, p, W_EDGE, g_dist=over, accumulate=False)
        assert torch.equal(over, g)
        out0, g0 = ops.smooth_loss(cu(rgb), cu(dist), cu(sky), P, p, 0.0)
        assert float(g0.abs().max()) == 0 and float(out0[0]) == 0 and torch.equal(out0[1:], out[1:])


@gpu
def test_smooth_op_without_patches_launches_nothing():
    from snerf_amd import ops
    e = torch.empty(0, device="cuda")
    total = torch.full((1,), 2.0, device="cuda")
    out, g = ops.smooth_loss(e.view(0, 3), e, None, 0, 6, 0.1, total=total)
    assert float(out.abs().max()) == 0 and g.numel() == 0 and float(total) == 2.0


# ---- GPU: the trainer -------------------------------------------------------------------------------------------------------------------
N_RGB, N_PATCH, P_SZ = 65, 2, 6
N_ALL = N_RGB + N_PATCH * P_SZ * P_SZ


def _model(semantic=False):
    """the small model of tests/test_confidence_step.py, in deterministic mode: two routes that feed the step the same bits leave the same
    bits in the arena"""
    from snerf_amd import mipnerf
    torch.manual_seed(0)
    kw = dict(semantic=True, semantic_class_num=5) if semantic else {}
    m = mipnerf.MipNerfModel(n_samples=16, N_fine=17, no_warp_sample=0, ray_shape="cone", fn=1, radius=3., transform_idx=0, real=True,
                             rgb_layer=3, hidden_layer=64, density_noise=0., max_deg_point=16, proposal_hidden_layer=64, proposal_loss=True,
                             compute="f32", **kw)
    return m.set_deterministic(True)


def _trainer(smooth=True, lam=0.1, semantic=False, sky=True):
    from snerf_amd.trainer import MipTrainer
    kw = dict(smooth_patch_sz=P_SZ, smooth_lambda=lam, smooth_skymask=sky) if smooth else {}
    return MipTrainer(_model(semantic), lr=5e-4, proposal_loss=True, **kw)


def _patch_batch(step=0):
    """batch `step` of a PatchRayBatcher: 65 pixel rows + 2 patches of 6 x 6, with depth targets and the sky extra"""
    b = _batchers(N_PATCH, P_SZ, n=N_RGB, plain=False)[0]
    for _ in range(step):
        b.next()
    rays, trgb, tdep, sel, img, ex = b.next()
    assert trgb.shape[0] == N_ALL == b.n_rows and b.n_rgb_rows == N_RGB
    assert 0 < int((tdep[N_RGB:] != 0).sum()) and 0 < int((tdep[:N_RGB] != 0).sum())       # LiDAR targets on both kinds of rows
    return rays, trgb, tdep, ex[0]


def _state(tr):
    return tr.model.arena.flat.clone(), tr.m.clone(), tr.v.clone()


@gpu
def test_trainer_smooth_term_joins_loss_and_gradient():
    from snerf_amd import ops
    rays, trgb, tdep, sky = _patch_batch()
    tdep0 = tdep.clone()
    tdep0[N_RGB:] = 0
    kept = tdep.clone()
    # the baseline: a trainer without the term on the same rays, patch-row depth targets set to 0; two of them leave the same bits
    base, base2 = _trainer(smooth=False), _trainer(smooth=False)
    loss_b, outs_b = base.step(rays, trgb, tdep0, randomized=False)
    base2.step(rays, trgb, tdep0, randomized=False)
    assert all(torch.equal(x, y) for x, y in zip(_state(base), _state(base2)))
    assert not torch.equal(base.model.arena.flat, _model().arena.flat)
    out, _ = ops.smooth_loss(trgb[N_RGB:], outs_b[5].reshape(-1)[N_RGB:].contiguous(), sky[N_RGB:], N_PATCH, P_SZ, 0.1)
    # (a) the loss
    tr = _trainer()
    loss, outs = tr.step(rays, trgb, tdep, randomized=False, n_rgb=N_RGB, smooth_sky=sky[N_RGB:])
    assert torch.equal(outs[5], outs_b[5])
    want = float(loss_b) + float(out[0])
    print(f"loss {float(loss):.9e} = baseline {float(loss_b):.9e} + smooth {float(out[0]):.9e} (sum {want:.9e})")
    assert abs(float(loss) - want) <= 2 * float(np.spacing(np.float32(want))) and float(out[0]) > 0
    assert torch.equal(tr.last_smooth_loss, out[0]) and tr.last_smooth_loss.is_cuda and tr.last_losses.numel() == 4
    # (d) the caller's targets are only read
    assert torch.equal(tdep, kept) and 0 < int((tdep[N_RGB:] != 0).sum())
    # (c) the term trains
    assert not torch.equal(tr.model.arena.flat, base.model.arena.flat)
    # (b) weight 0: the baseline's bits
    tr0 = _trainer(lam=0.0)
    loss0, _ = tr0.step(rays, trgb, tdep, randomized=False, n_rgb=N_RGB, smooth_sky=sky[N_RGB:])
    for name, x, y in zip(("arena", "m", "v"), _state(tr0), _state(base)):
        assert torch.equal(x, y), name
    assert float(tr0.last_smooth_loss) == 0 and abs(float(loss0) - float(loss_b)) <= 2 * float(np.spacing(np.float32(float(loss_b))))
    # without the sky weighting
    trn = _trainer(sky=False)
    trn.step(rays, trgb, tdep, randomized=False, n_rgb=N_RGB)
    outn, _ = ops.smooth_loss(trgb[N_RGB:], outs_b[5].reshape(-1)[N_RGB:].contiguous(), None, N_PATCH, P_SZ, 0.1)
    assert torch.equal(trn.last_smooth_loss, outn[0]) and float(outn[0]) < float(out[0])


@gpu
def test_trainer_batch_without_patch_rows_is_the_baseline():
    rays, trgb, tdep, sky = _patch_batch()
    cut = lambda t: t[:N_RGB].contiguous()
    r65 = type(rays)(*[cut(f) for f in rays])
    base, tr = _trainer(smooth=False), _trainer()
    loss_b, _ = base.step(r65, cut(trgb), cut(tdep), randomized=False)
    loss, _ = tr.step(r65, cut(trgb), cut(tdep), randomized=False, n_rgb=N_RGB, smooth_sky=sky[N_RGB:N_RGB])
    for name, x, y in zip(("arena", "m", "v"), _state(tr), _state(base)):
        assert torch.equal(x, y), name
    assert float(tr.last_smooth_loss) == 0 and abs(float(loss) - float(loss_b)) <= 2 * float(np.spacing(np.float32(float(loss_b))))


@gpu
def test_trainer_labels_leave_the_patch_rows_out_and_stay_untouched():
    """the semantic term counts the first n_rgb rays only; the caller's labels are read, never written"""
    rays, trgb, tdep, sky = _patch_batch()
    gen = torch.Generator().manual_seed(5)
    labels = torch.randint(0, 5, (N_ALL,), generator=gen).float()
    labels[torch.rand(N_ALL, generator=gen) < 0.2] = -100
    labels = labels.cuda()
    kept_l, kept_d = labels.clone(), tdep.clone()
    tr = _trainer(semantic=True)
    tr.step(rays, trgb, tdep, randomized=False, target_semantic=labels, n_rgb=N_RGB, smooth_sky=sky[N_RGB:])
    assert torch.equal(labels, kept_l) and torch.equal(tdep, kept_d)
    n_dep, _, n_sem = (int(c) for c in tr.last_counts)
    assert n_sem == int((kept_l[:N_RGB] != -100).sum()) < int((kept_l != -100).sum())
    assert n_dep == int((kept_d[:N_RGB] != 0).sum()) < int((kept_d != 0).sum())
    assert float(tr.last_smooth_loss) > 0 and float(tr.last_semantic_loss) > 0


@gpu
def test_trainer_refuses_inconsistent_smooth_arguments():
    rays, trgb, tdep, sky = _patch_batch()
    tr = _trainer()
    before = tr.model.arena.flat.clone()
    with pytest.raises(ValueError):
        tr.step(rays, trgb, tdep, randomized=False, smooth_sky=sky[N_RGB:])                               # no n_rgb
    with pytest.raises(ValueError):
        tr.step(rays, trgb, tdep, randomized=False, n_rgb=N_RGB + 1, smooth_sky=sky[N_RGB + 1:])          # 71 rows: not whole patches
    with pytest.raises(ValueError):
        tr.step(rays, trgb, tdep, randomized=False, n_rgb=N_RGB)                                          # no sky
    with pytest.raises(ValueError):
        tr.step(rays, trgb, tdep, randomized=False, n_rgb=N_RGB, smooth_sky=sky[N_RGB + 1:])              # a short sky
    with pytest.raises(ValueError):
        _trainer(sky=False).step(rays, trgb, tdep, randomized=False, n_rgb=N_RGB, smooth_sky=sky[N_RGB:])
    with pytest.raises(ValueError):
        _trainer(smooth=False).step(rays, trgb, tdep, randomized=False, n_rgb=N_RGB)
    assert torch.equal(tr.model.arena.flat, before) and tr.t == 0


@gpu
def test_capture_with_patch_batcher_replays_the_eager_steps():
    """three replays with a PatchRayBatcher against three eager steps from the same state (deterministic model, no random draws)"""
    steps = 3
    b, tr = _batchers(N_PATCH, P_SZ, n=N_RGB, plain=False)[0], _trainer()
    smooth = []
    for _ in range(steps):
        rays, trgb, tdep, sel, img, ex = b.next()
        tr.step(rays, trgb, tdep, randomized=False, n_rgb=b.n_rgb_rows, smooth_sky=ex[0][b.n_rgb_rows:])
        smooth.append(tr.last_smooth_loss.clone())
    eager = _state(tr)
    b, tr = _batchers(N_PATCH, P_SZ, n=N_RGB, plain=False)[0], _trainer()
    init = tr.model.arena.flat.clone()
    tr.capture(None, None, randomized=False, warmup=2, batcher=b, smooth_sky_extra=0)
    torch.cuda.synchronize()
    assert tr.t == 0 and torch.equal(tr.model.arena.flat, init) and b.step == 0 and int(b.counter[0]) == 0
    for k in range(steps):
        loss, _ = tr.replay()
        assert np.isfinite(float(loss)) and torch.equal(tr.last_smooth_loss, smooth[k]) and float(smooth[k]) > 0
    assert tr.t == steps and b.step == steps and int(b.counter[0]) == steps
    for name, got, want in zip(("arena", "m", "v"), _state(tr), eager):
        print(f"captured vs eager {name}: max |diff| = {float((got - want).abs().max()):.3e}")
        assert torch.equal(got, want), name
    with pytest.raises(ValueError):
        _trainer().capture(None, None, randomized=False, batcher=_batchers(N_PATCH, P_SZ, n=N_RGB)[1], smooth_sky_extra=0)
    with pytest.raises(ValueError):
        _trainer().capture(None, None, randomized=False, batcher=_batchers(N_PATCH, P_SZ, n=N_RGB, plain=False)[0])
