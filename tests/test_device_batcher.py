"""Device-resident training batchers (snerf_mip_image_batch / sample_utils.ImageRayBatcher for path A, snerf_zip_ray_batch /
zipnerf.RayBatcher for path C).  Given the drawn pixels, rays and targets must equal the existing mirrors bit for bit; the draws
themselves are restated here in numpy from the algorithm documented in csrc/callers.hip (Philox4x32-10, keyed Feistel permutation with
cycle walking, Lemire's bounded integers)."""
import os
import types

import numpy as np
import pytest
import torch

from snerf_amd import _lib

gpu = pytest.mark.gpu
M32 = np.uint64(0xFFFFFFFF)


# ---- numpy restatement of the generator ---------------------------------------------------------------------------------------------
def np_philox(c0, c1, c2, c3, seed):
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, dtype=np.uint64) & M32 for c in (c0, c1, c2, c3)))
    c0, c1, c2, c3 = (c.copy() for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = c0 * np.uint64(0xD2511F53), c2 * np.uint64(0xCD9E8D57)
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0


def np_perm(v, M, tag, t, seed):
    b = max(2, int(M - 1).bit_length())
    b += b & 1
    h = np.uint64(b >> 1)
    mask = np.uint64((1 << int(h)) - 1)
    t0, t1 = t & 0xFFFFFFFF, (t >> 32) & 0xFFFFFFFF
    v = np.asarray(v, dtype=np.uint64).copy()
    todo = np.ones(v.shape, dtype=bool)
    while todo.any():
        x = v[todo]
        for j in range(4):
            L, R = x >> h, x & mask
            x = (R << h) | (L ^ (np_philox(R, (tag << 16) | j, t0, t1, seed) & mask))
        v[todo] = x
        todo = v >= np.uint64(M)
    return v.astype(np.int64)


def np_bounded(i, v, s, rng, seed):
    i = np.asarray(i, dtype=np.uint64)
    thresh = np.uint64((2 ** 32 - rng) % rng)
    out = np.zeros(i.shape, dtype=np.int64)
    todo = np.ones(i.shape, dtype=bool)
    for a in range(256):
        m = np_philox(i[todo], (3 << 16) | (v << 8) | a, s & 0xFFFFFFFF, s >> 32, seed) * np.uint64(rng)
        ok = ((m & M32) >= thresh) | (a == 255)
        idx = np.nonzero(todo)[0]
        out[idx[ok]] = (m[ok] >> np.uint64(32)).astype(np.int64)
        todo[idx[ok]] = False
        if not todo.any():
            break
    return out


def np_image_of_step(i_train, seed, s):
    nt = len(i_train)
    return int(np.asarray(i_train)[np_perm([s % nt], nt, 1, s // nt, seed)[0]])


# ---- CPU: generator, schedule, argument checks --------------------------------------------------------------------------------------
def test_philox_known_answers_and_numpy_restatement():
    """the host generator is Philox4x32-10 (Random123's known-answer vectors) and the numpy restatement agrees with it"""
    from snerf_amd import sample_utils as su
    assert su.philox((0, 0, 0, 0), 0) == 0x6627E8D5
    assert su.philox((0xFFFFFFFF,) * 4, (1 << 64) - 1) == 0x408F276D
    assert su.philox((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), 0x299F31D0 << 32 | 0xA4093822) == 0xD16CFE09
    c = np.arange(50)
    want = [su.philox((int(x), 7, 11, 13), 12345) for x in c]
    assert np.array_equal(np_philox(c, 7, 11, 13, 12345), np.asarray(want, dtype=np.uint64))
    for M in (1, 2, 5, 64, 1000):
        got = np_perm(np.arange(M), M, 2, 3, 99)
        assert sorted(got.tolist()) == list(range(M))
        assert got.tolist() == [su.keyed_perm(v, M, 2, 3, 99) for v in range(M)]


def test_image_schedule_visits_every_training_image_once_per_epoch():
    from snerf_amd import sample_utils as su
    i_train = [0, 2, 3, 5, 8, 9, 13]
    nt = len(i_train)
    orders = []
    for e in range(6):
        order = [su.image_of_step(i_train, 5, e * nt + p) for p in range(nt)]
        assert sorted(order) == i_train, (e, order)
        assert order == [np_image_of_step(i_train, 5, e * nt + p) for p in range(nt)]
        orders.append(order)
    assert len({tuple(o) for o in orders}) > 1                                   # a new order every epoch
    assert [su.image_of_step(i_train, 5, s) for s in range(40)] == [su.image_of_step(i_train, 5, s) for s in range(40)]
    assert [su.image_of_step(i_train, 5, s) for s in range(40)] != [su.image_of_step(i_train, 6, s) for s in range(40)]
    assert all(su.image_of_step([4], 1, s) == 4 for s in range(5))


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")


def _mip_args(**kw):
    a = dict(images=64, images_u8=0, depths=64, poses=64, intrinsics=64, near=64, far=64, app=64, extras=None, n_extra=0, i_train=64,
             n_train=2, N=3, H=8, W=8, seed=0, counter=64, n=16, i0=0, i1=16, origins=64, directions=64, viewdirs=64, radii=64,
             lossmult=64, near_out=64, far_out=64, app_out=64, rgb=64, depth=64, extras_out=None, sel_coords=64, img_out=64, stream=None)
    a.update(kw)
    return list(a.values())


def _zip_args(**kw):
    a = dict(images=64, images_u8=0, depths=None, semantics=None, masks=None, pixtocams=64, camtoworlds=64, local2global=None, N=3, H=8, W=8,
             near=0.1, far=10.0, border=0, patch_size=1, single_image=0, seed=0, counter=64, n=16, i0=0, i1=16, origins=64, directions=64,
             viewdirs=64, radii=64, imageplane=None, base_x=64, base_y=64, lossmult=64, near_out=64, far_out=64, cam_idx=64, glo_idx=None,
             rgb=64, depth=None, semantic=None, mask=None, pix_x=64, pix_y=64, stream=None)
    a.update(kw)
    return list(a.values())


def test_batch_entries_reject_bad_arguments_without_a_gpu():
    """argument validation happens before any launch (the pointers here are never dereferenced)"""
    _lib_or_skip()
    bad_mip = [dict(n=65, i1=65), dict(H=2), dict(images=None), dict(N=0), dict(n_train=0), dict(i1=17), dict(i0=5, i1=4), dict(n=-1),
               dict(counter=None), dict(origins=None), dict(n_extra=1), dict(images_u8=2), dict(depths=None)]
    for kw in bad_mip:
        with pytest.raises(_lib.SnerfHipError, match="bad argument"):
            _lib.call("snerf_mip_image_batch", *_mip_args(**kw))
    bad_zip = [dict(border=4), dict(border=-1), dict(patch_size=2), dict(images=None), dict(N=0), dict(pixtocams=None), dict(i1=17),
               dict(counter=None), dict(glo_idx=64), dict(depth=64), dict(semantic=64), dict(mask=64), dict(pix_x=None)]
    for kw in bad_zip:
        with pytest.raises(_lib.SnerfHipError, match="bad argument"):
            _lib.call("snerf_zip_ray_batch", *_zip_args(**kw))
    # an empty batch is a no-op, whatever the rest
    none_mip = [None if isinstance(v, int) and v == 64 else v for v in _mip_args(n=0, i1=0)]
    none_zip = [None if isinstance(v, int) and v == 64 else v for v in _zip_args(n=0, i1=0)]
    assert _lib.call("snerf_mip_image_batch", *none_mip) is None
    assert _lib.call("snerf_zip_ray_batch", *none_zip) is None


def test_batcher_constructors_reject_what_they_do_not_cover():
    from snerf_amd import sample_utils as su, zipnerf
    args = types.SimpleNamespace(no_ndc=True, smooth_loss=False, near_far=False, N_rgb=64)
    img, dep = np.zeros((2, 8, 8, 3), np.float32), np.ones((2, 8, 8), np.float32)
    pose, K = np.tile(np.eye(4, dtype=np.float32)[:3], (2, 1, 1)), np.tile(np.eye(3, dtype=np.float32), (2, 1, 1))
    mk = lambda a=args, **kw: su.ImageRayBatcher(a, kw.pop("images", img), dep, pose, K, kw.pop("i_train", [0, 1]), 1.0, 10.0, **kw)
    with pytest.raises(NotImplementedError):
        mk(types.SimpleNamespace(no_ndc=False, smooth_loss=False, near_far=False, N_rgb=64))
    with pytest.raises(NotImplementedError):
        mk(types.SimpleNamespace(no_ndc=True, smooth_loss=True, near_far=False, N_rgb=64))
    with pytest.raises(ValueError):
        mk(batch_n=65)
    with pytest.raises(ValueError):
        mk(images=np.zeros((0, 8, 8, 3), np.float32))
    with pytest.raises(ValueError):
        mk(i_train=[])
    with pytest.raises(NotImplementedError):
        zipnerf.RayBatcher(img, K, pose, 0.1, 10.0, patch_size=2)
    with pytest.raises(ValueError):
        zipnerf.RayBatcher(np.zeros((0, 8, 8, 3), np.float32), K[:0], pose[:0], 0.1, 10.0)
    with pytest.raises(ValueError):
        zipnerf.RayBatcher(img, K, pose, 0.1, 10.0, border=4)
    with pytest.raises(ValueError):
        zipnerf.RayBatcher(img, K, pose, 0.1, 10.0, batching="patches")


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def _scene(N=5, H=24, W=40, u8=False, seed=0):
    rng = np.random.default_rng(seed)
    if u8:
        images = rng.integers(0, 256, size=(N, H, W, 3), dtype=np.uint8)
    else:
        images = rng.random((N, H, W, 3), dtype=np.float32)
    depths = (rng.random((N, H, W)) * 60 + 2).astype(np.float32)
    depths[rng.random((N, H, W)) < 0.5] = 0
    poses = np.zeros((N, 3, 4), np.float32)
    for i in range(N):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        poses[i, :, :3], poses[i, :, 3] = q, rng.normal(size=3)
    K = np.zeros((N, 3, 3), np.float32)
    K[:, 0, 0], K[:, 1, 1] = rng.uniform(20, 80, N), rng.uniform(20, 80, N)
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = W * rng.uniform(0.4, 0.6, N), H * rng.uniform(0.4, 0.6, N), 1
    extras = [rng.random((N, H, W), dtype=np.float32) for _ in range(2)]
    return images, depths, poses, K, extras


def _image_batcher(near_far=False, u8=False, n=300, seed=3, rank=0, world=1, N=5, H=24, W=40, i_train=(0, 1, 3, 4), extras=True):
    from snerf_amd import sample_utils as su
    images, depths, poses, K, ex = _scene(N, H, W, u8)
    args = types.SimpleNamespace(no_ndc=True, smooth_loss=False, near_far=near_far, N_rgb=n)
    b = su.ImageRayBatcher(args, images, depths, poses, K, list(i_train), 2.0, 80.0, camera_index=np.arange(N) * 10.0, batch_n=n,
                           extras=ex if extras else None, seed=seed, rank=rank, world=world, device="cuda")
    return b, (images, depths, poses, K, ex)


@gpu
@pytest.mark.parametrize("near_far", [False, True])
@pytest.mark.parametrize("u8", [False, True])
def test_image_batcher_equals_rays_of_pixels_bit_for_bit(near_far, u8):
    from snerf_amd import sample_utils as su
    b, (images, depths, poses, K, ex) = _image_batcher(near_far, u8)
    H, W = images.shape[1:3]
    seen = set()
    for s in range(20):
        rays, trgb, tdep, sel, img_t, extras = b.next()
        img = int(img_t)
        assert img == b.image_of_step(s) == np_image_of_step([0, 1, 3, 4], 3, s)
        seen.add(img)
        if near_far:
            nz = depths[img][depths[img] != 0]
            near, far = float(nz.min()) * 0.9, float(nz.max()) * 1.1
        else:
            near, far = 2.0 * 0.9, 80.0 * 1.1
        want = su.rays_of_pixels(sel, poses[img], K[img], H, W, near, far, training=True)
        for k in ("origins", "directions", "viewdirs", "radii", "lossmult", "near", "far"):
            assert torch.equal(getattr(rays, k), getattr(want, k)), (s, k)
        assert torch.equal(rays.app, torch.full_like(rays.app, img * 10.0))
        r, c = sel[:, 0].cpu().numpy(), sel[:, 1].cpu().numpy()
        ref_rgb = images[img] if not u8 else (images[img] / 255.).astype(np.float32)
        assert np.array_equal(trgb.cpu().numpy(), ref_rgb[r, c])
        assert np.array_equal(tdep.cpu().numpy(), depths[img][r, c])
        for e_got, e_map in zip(extras, ex):
            assert np.array_equal(e_got.cpu().numpy(), e_map[img][r, c])
        q = np_perm(np.arange(300), H * W, 2, s, 3)
        assert np.array_equal(r, q // W) and np.array_equal(c, q % W)            # the documented draw
        assert len(set((r * W + c).tolist())) == 300                             # without replacement
    assert seen == {0, 1, 3, 4}


@gpu
def test_image_batcher_full_permutation_and_uniformity():
    b, _ = _image_batcher(n=24 * 40, extras=False)
    for _ in range(3):
        sel = b.next()[3].cpu().numpy()
        assert sorted((sel[:, 0] * 40 + sel[:, 1]).tolist()) == list(range(24 * 40))
    H, W, n, steps = 50, 64, 2048, 500                                          # 1.02 M draws
    b, _ = _image_batcher(n=n, H=H, W=W, N=2, i_train=(0, 1), extras=False, seed=11)
    rows = torch.zeros(H, dtype=torch.int64, device="cuda")
    cols = torch.zeros(W, dtype=torch.int64, device="cuda")
    for _ in range(steps):
        sel = b.next()[3]
        rows += torch.bincount(sel[:, 0], minlength=H)
        cols += torch.bincount(sel[:, 1], minlength=W)
    for cnt, k in ((rows, H), (cols, W)):
        e = n * steps / k
        chi2 = float(((cnt.double() - e) ** 2 / e).sum())
        assert chi2 < (k - 1) + 6 * np.sqrt(2 * (k - 1)), (k, chi2)


@gpu
@pytest.mark.parametrize("world", [2, 4, 8])
def test_image_batcher_rank_slices_make_the_single_gpu_batch(world):
    full, _ = _image_batcher(n=301)
    parts = [_image_batcher(n=301, rank=r, world=world)[0] for r in range(world)]
    for _ in range(3):
        want = full.next()
        got = [p.next() for p in parts]
        for k in range(8):
            assert torch.equal(torch.cat([g[0][k] for g in got]), want[0][k])
        for j in (1, 2, 3):
            assert torch.equal(torch.cat([g[j] for g in got]), want[j])
        assert all(int(g[4]) == int(want[4]) for g in got)
        for e in range(2):
            assert torch.equal(torch.cat([g[5][e] for g in got]), want[5][e])


@gpu
def test_image_batcher_determinism_and_resume():
    a, b, c = _image_batcher()[0], _image_batcher()[0], _image_batcher(seed=4)[0]
    for _ in range(4):
        x, y, z = a.next(), b.next(), c.next()
        assert torch.equal(x[3], y[3]) and torch.equal(x[0].directions, y[0].directions)
        assert not torch.equal(x[3], z[3])
    keep = a.next()                                                              # eager results stay valid after later calls
    kept = keep[3].clone()
    sd = a.state_dict()
    later = [a.next()[3] for _ in range(3)]
    assert torch.equal(keep[3], kept)
    d = _image_batcher(seed=99)[0]
    d.load_state_dict(sd)
    assert d.step == 5 and d.seed == 3
    for w in later:
        assert torch.equal(d.next()[3], w)


@gpu
def test_image_batcher_captured_draw_replays_the_eager_stream():
    eager = _image_batcher()[0]
    cap = _image_batcher()[0]
    buf = cap.buffers()
    cap.next_into(buf)                                                           # (load the kernel before capturing)
    cap.load_state_dict({"seed": 3, "step": 0})
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        view = cap.next_into(buf)
    torch.cuda.synchronize()
    assert int(cap.counter[0]) == 0
    for s in range(4):
        g.replay()
        want = eager.next()
        assert torch.equal(view[3], want[3]) and torch.equal(view[0].radii, want[0].radii) and int(view[4]) == int(want[4]), s
        assert torch.equal(view[1], want[1]) and torch.equal(view[5][1], want[5][1])
    torch.cuda.synchronize()
    assert int(cap.counter[0]) == 4


def _mip_model():
    from snerf_amd import mipnerf
    torch.manual_seed(0)
    return mipnerf.MipNerfModel(n_samples=16, N_fine=17, no_warp_sample=0, ray_shape="cone", fn=1, radius=3., transform_idx=0, real=True,
                                rgb_layer=3, hidden_layer=64, density_noise=0., max_deg_point=16, proposal_hidden_layer=64, proposal_loss=True,
                                compute="f32")


@gpu
def test_mip_trainer_capture_with_batcher_trains_on_a_fresh_draw_every_replay():
    from snerf_amd.trainer import MipTrainer
    b, _ = _image_batcher(n=256)
    eager, _ = _image_batcher(n=256)
    draws = [eager.next() for _ in range(6)]
    b.next(); b.next()
    s0 = b.step
    tr = MipTrainer(_mip_model(), lr=5e-4)
    init = tr.model.arena.flat.clone()
    tr.capture(None, None, randomized=True, warmup=2, batcher=b, conf_extra=0)
    torch.cuda.synchronize()
    assert b.step == s0 and int(b.counter[0]) == s0 and tr.t == 0 and torch.equal(tr.model.arena.flat, init)
    prev = None
    for k in range(4):
        loss, _ = tr.replay()
        rays, trgb, tdep, sel, img, ex = tr.batch
        want = draws[s0 + k]
        assert torch.equal(sel, want[3]) and torch.equal(rays.directions, want[0].directions) and torch.equal(trgb, want[1]), k
        assert torch.equal(tdep, want[2]) and torch.equal(ex[0], want[5][0]) and int(img) == int(want[4])
        assert prev is None or not torch.equal(sel, prev)
        prev = sel.clone()
        assert np.isfinite(float(loss))
    assert b.step == s0 + 4 and int(b.counter[0]) == s0 + 4 and tr.t == 4
    assert not torch.equal(tr.model.arena.flat, init)


@gpu
def test_mip_trainer_steps_on_batcher_output():
    from snerf_amd.trainer import MipTrainer
    b, _ = _image_batcher(n=256, near_far=True, u8=True)
    tr = MipTrainer(_mip_model(), lr=5e-4)
    for _ in range(20):
        rays, trgb, tdep, _, _, ex = b.next()
        loss, _ = tr.step(rays, trgb, tdep, ex[0])
        assert np.isfinite(float(loss))


# ---- path C -------------------------------------------------------------------------------------------------------------------------
def _zip_scene(N=7, H=30, W=50, u8=True, seed=0):
    rng = np.random.default_rng(seed)
    images = rng.integers(0, 256, size=(N, H, W, 3), dtype=np.uint8) if u8 else rng.random((N, H, W, 3), dtype=np.float32)
    depths = (rng.random((N, H, W)) * 0.8).astype(np.float32)
    sem = rng.integers(0, 19, size=(N, H, W)).astype(np.int32)
    masks = (rng.random((N, H, W)) < 0.7).astype(np.float32)
    K = np.zeros((N, 3, 3), np.float64)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = rng.uniform(40, 60, N), rng.uniform(40, 60, N), W / 2, H / 2, 1
    pixtocams = np.linalg.inv(K).astype(np.float32)
    c2w = np.zeros((N, 3, 4), np.float32)
    for i in range(N):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        c2w[i, :, :3], c2w[i, :, 3] = q, rng.normal(size=3) * 0.05
    l2g = (np.arange(N) * 3 + 1).astype(np.int32)
    return dict(images=images, pixtocams=pixtocams, camtoworlds=c2w, depths=depths, semantics=sem, masks=masks, local2global=l2g)


def _zip_batcher(batch_size=1000, border=2, seed=5, rank=0, world=1, batching="all_images", u8=True, **kw):
    from snerf_amd import zipnerf
    sc = _zip_scene(u8=u8, **kw)
    b = zipnerf.RayBatcher(sc["images"], sc["pixtocams"], sc["camtoworlds"], 0.02, 100.0, depths=sc["depths"], semantics=sc["semantics"],
                           masks=sc["masks"], local2global=sc["local2global"], batch_size=batch_size, border=border, batching=batching,
                           seed=seed, rank=rank, world=world, device="cuda")
    return b, sc


@gpu
@pytest.mark.parametrize("u8", [True, False])
def test_zip_batcher_equals_pixels_to_rays_bit_for_bit(u8):
    from snerf_amd import ops
    b, sc = _zip_batcher(u8=u8)
    N, H, W = sc["images"].shape[:3]
    for s in range(20):
        bt = b.next()
        x, y, cam = bt["pix_x_int"], bt["pix_y_int"], bt["cam_idx"][:, 0].int()
        i = np.arange(1000)
        assert np.array_equal(cam.cpu().numpy(), np_bounded(i, 0, s, N, 5))
        assert np.array_equal(x.cpu().numpy(), 2 + np_bounded(i, 1, s, W - 4, 5))
        assert np.array_equal(y.cpu().numpy(), 2 + np_bounded(i, 2, s, H - 4, 5))
        want = ops.zip_pixels_to_rays(x, y, cam.contiguous(), torch.from_numpy(sc["pixtocams"]).cuda(), torch.from_numpy(sc["camtoworlds"]).cuda(),
                                      want_imageplane=True)
        for k, v in want.items():
            assert torch.equal(bt[k], v), (s, k)
        xs, ys, cs = x.cpu().numpy(), y.cpu().numpy(), cam.cpu().numpy()
        ref = sc["images"][cs, ys, xs]
        ref = (ref / 255.).astype(np.float32) if u8 else ref
        assert np.array_equal(bt["rgb"].cpu().numpy(), ref)
        assert np.array_equal(bt["depth"].cpu().numpy(), sc["depths"][cs, ys, xs])
        assert np.array_equal(bt["semantic"].cpu().numpy(), sc["semantics"][cs, ys, xs]) and bt["semantic"].dtype == torch.int32
        assert np.array_equal(bt["mask"].cpu().numpy(), sc["masks"][cs, ys, xs])
        assert np.array_equal(bt["glo_idx"][:, 0].cpu().numpy(), sc["local2global"][cs].astype(np.float32))
        assert xs.min() >= 2 and xs.max() < W - 2 and ys.min() >= 2 and ys.max() < H - 2
        assert float(bt["lossmult"].min()) == 1.0 == float(bt["lossmult"].max())
        assert torch.equal(bt["near"], torch.full_like(bt["near"], 0.02)) and torch.equal(bt["far"], torch.full_like(bt["far"], 100.0))
    one, _ = _zip_batcher(batching="single_image")
    for s in range(5):
        cam = one.next()["cam_idx"]
        assert torch.equal(cam, torch.full_like(cam, float(np_bounded([0], 0, s, 7, 5)[0])))


@gpu
def test_zip_batcher_uniformity():
    b, sc = _zip_batcher(batch_size=65536, seed=21)
    N, H, W = sc["images"].shape[:3]
    cnt = {k: torch.zeros(r, dtype=torch.int64, device="cuda") for k, r in (("x", W), ("y", H), ("c", N))}
    steps = 16                                                                   # 1.05 M draws
    for _ in range(steps):
        bt = b.next()
        cnt["x"] += torch.bincount(bt["pix_x_int"].long(), minlength=W)
        cnt["y"] += torch.bincount(bt["pix_y_int"].long(), minlength=H)
        cnt["c"] += torch.bincount(bt["cam_idx"][:, 0].long(), minlength=N)
    for k, lo, hi in (("x", 2, W - 2), ("y", 2, H - 2), ("c", 0, N)):
        c = cnt[k].double()
        assert float(c[:lo].sum() + c[hi:].sum()) == 0
        c = c[lo:hi]
        e = 65536 * steps / c.numel()
        chi2 = float(((c - e) ** 2 / e).sum())
        dof = c.numel() - 1
        assert chi2 < dof + 6 * np.sqrt(2 * dof), (k, chi2)


@gpu
@pytest.mark.parametrize("world", [2, 4, 8])
def test_zip_batcher_rank_slices_make_the_single_gpu_batch(world):
    full, _ = _zip_batcher(batch_size=1001)
    parts = [_zip_batcher(batch_size=1001, rank=r, world=world)[0] for r in range(world)]
    for _ in range(3):
        want = full.next()
        got = [p.next() for p in parts]
        for k, v in want.items():
            assert torch.equal(torch.cat([g[k] for g in got]), v), k


@gpu
def test_zip_batcher_determinism_resume_and_graph():
    a, b, c = _zip_batcher()[0], _zip_batcher()[0], _zip_batcher(seed=6)[0]
    for _ in range(3):
        x, y, z = a.next(), b.next(), c.next()
        assert all(torch.equal(x[k], y[k]) for k in x)
        assert not torch.equal(x["pix_x_int"], z["pix_x_int"])
    sd = a.state_dict()
    later = [a.next() for _ in range(2)]
    d = _zip_batcher(seed=1)[0]
    d.load_state_dict(sd)
    for w in later:
        assert torch.equal(d.next()["origins"], w["origins"])
    cap = _zip_batcher()[0]
    buf = cap.buffers()
    cap.next_into(buf)
    cap.load_state_dict({"seed": 5, "step": 0})
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap.next_into(buf)
    eager = _zip_batcher()[0]
    for s in range(4):
        g.replay()
        want = eager.next()
        assert all(torch.equal(buf[k], want[k]) for k in want), s


@gpu
def test_zip_trainer_steps_on_batcher_output():
    from snerf_amd import zipnerf
    from snerf_amd.trainer import ZipTrainer
    torch.manual_seed(0)
    m = zipnerf.Model(config=None, raydist_fn='power_transformation', opaque_background=True, compute="bf16", table_dtype="ref",
                      grid_log2_hashmap_size=16, init_std=0.1, device="cuda")
    tr = ZipTrainer(m, lr=1e-2)
    b, _ = _zip_batcher(batch_size=4096)
    for _ in range(20):
        bt = b.next()
        loss, _ = tr.step(bt, bt["rgb"], train_frac=0.5, rand=True, targets=dict(depth=bt["depth"], depth_mask=bt["mask"]))
        assert np.isfinite(float(loss))
