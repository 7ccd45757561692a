"""The fused train step of the classic render_rays path (path B): the loss-tail kernel (snerf_classic_loss_tail / ops.classic_loss_tail),
the device ray batcher (snerf_classic_train_batch / classic.RayBatcher) and trainer.ClassicTrainer, eager and captured.

The reference has no loss loop of its own for this path; the oracles are stated here:
  * the loss tail: float64 torch autograd of img2mse(rgb, t) + img2mse(rgb0, t) and mse2psnr (run_nerf_helpers.py:16-17), and a numpy
    fp32 restatement of the gradient expression the header documents;
  * the batch: the schedule restated on the host (sample_utils.classic_rays_of_step) and, for the rows, classic.render's own ray rows
    (ops.classic_ray_batch) of the same camera, one camera at a time;
  * the step: the autograd route over classic.render_rays seeded with the tail's own gradients -- the same kernels on the same inputs,
    so every difference is a wiring bug -- followed by ops.adam_step, and torch.optim.Adam inside the bound test_optimizer_tail.py
    uses for the fused Adam."""
import os

import numpy as np
import pytest
import torch

from snerf_amd import _lib
from snerf_amd import sample_utils as su

gpu = pytest.mark.gpu
DEV = "cuda"


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")


def ulp32(x):
    """spacing of fp32 at |x| (float64 in, float64 out)"""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


# ---- the loss tail: host model and float64 oracle -----------------------------------------------------------------------------------
def tail_model(rgb, rgb0, tgt):
    """numpy restatement of snerf_classic_loss_tail: fp32 gradients inv * (2 * (x - t)) with inv = 1.0f / (float)(3 N); double sums of
    the double differences' squares, each scalar rounded to fp32 once -> (out[4], g_rgb, g_rgb0 or None)"""
    N = rgb.shape[0]
    inv = np.float32(1.0) / np.float32(3 * N)
    grad = lambda x: (inv * (np.float32(2.0) * (x - tgt))).astype(np.float32)
    mse = lambda x: float(((x.astype(np.float64) - tgt.astype(np.float64)) ** 2).sum() / (3.0 * N))
    l1, l0 = mse(rgb), (mse(rgb0) if rgb0 is not None else 0.0)
    out = np.asarray([l1 + l0, l1, l0, -10.0 * np.log(l1) / np.log(10.0)], dtype=np.float64).astype(np.float32)
    return out, grad(rgb), (grad(rgb0) if rgb0 is not None else None)


def tail_f64(rgb, rgb0, tgt):
    """float64 torch autograd of the stock loss -> (out[4] float64, g_rgb, g_rgb0 or None float64)"""
    img2mse = lambda x, y: torch.mean((x - y) ** 2)
    mse2psnr = lambda x: -10. * torch.log(x) / torch.log(torch.tensor([10.], dtype=torch.float64))
    t = torch.from_numpy(tgt).double()
    x = torch.from_numpy(rgb).double().requires_grad_(True)
    x0 = None if rgb0 is None else torch.from_numpy(rgb0).double().requires_grad_(True)
    l1 = img2mse(x, t)
    l0 = img2mse(x0, t) if x0 is not None else torch.zeros((), dtype=torch.float64)
    (l1 + l0).backward()
    out = np.asarray([float((l1 + l0).detach()), float(l1.detach()), float(l0.detach()), float(mse2psnr(l1.detach()))])
    return out, x.grad.numpy(), (None if x0 is None else x0.grad.numpy())


def _tail_inputs(N, seed=0):
    rng = np.random.default_rng(seed + N)
    return rng.random((N, 3), dtype=np.float32), rng.random((N, 3), dtype=np.float32), rng.random((N, 3), dtype=np.float32)


TAIL_N = (1, 63, 64, 65, 257, 1000, 5000)


@pytest.mark.parametrize("with0", [True, False])
@pytest.mark.parametrize("N", TAIL_N)
def test_loss_tail_host_model_against_float64_autograd(N, with0):
    rgb, rgb0, tgt = _tail_inputs(N)
    rgb0 = rgb0 if with0 else None
    out, g, g0 = tail_model(rgb, rgb0, tgt)
    ref, gr, gr0 = tail_f64(rgb, rgb0, tgt)
    assert (np.abs(out.astype(np.float64) - ref) <= ulp32(ref)).all(), (out, ref)
    for a, b in ((g, gr), (g0, gr0)):
        if b is None:
            assert a is None
            continue
        # (1 ulp of the float64 value; an element whose difference is exactly 0 has gradient exactly 0 on both sides)
        assert (np.abs(a.astype(np.float64) - b) <= ulp32(b)).all()
    assert out[2] == 0.0 or with0


# ---- the batch schedule on the host --------------------------------------------------------------------------------------------------
SCENES = {70: (2, 5, 7), 162: (3, 9, 6)}                  # T -> (training images, H, W)


@pytest.mark.parametrize("T", sorted(SCENES))
@pytest.mark.parametrize("n_rand", [1, 16, "T", "T+30"])
def test_batch_schedule_visits_every_ray_once_per_epoch(T, n_rand):
    n_rand = {"T": T, "T+30": T + 30}.get(n_rand, n_rand)
    seed = 11
    epochs = 3
    steps = -(-epochs * T // n_rand)
    stream = np.concatenate([su.classic_rays_of_step(s, n_rand, T, seed) for s in range(steps)])
    assert stream.dtype == np.int64 and stream.shape == (steps * n_rand,)
    orders = []
    for e in range(epochs):
        ep = stream[e * T:(e + 1) * T]
        assert np.array_equal(np.sort(ep), np.arange(T)), (T, n_rand, e)            # a permutation of [0, T)
        assert np.array_equal(ep, [su.keyed_perm(p, T, su.CLASSIC_BATCH_TAG, e, seed) for p in range(T)])
        orders.append(ep)
    assert not np.array_equal(orders[0], orders[1]) and not np.array_equal(orders[1], orders[2])
    # a batch that straddles an epoch boundary: the tail of one epoch's order, then the head of the next one's
    for s in range(steps):
        lo, hi = s * n_rand, (s + 1) * n_rand
        if lo // T != (hi - 1) // T and hi <= epochs * T:
            e = lo // T
            cut = (e + 1) * T - lo
            b = su.classic_rays_of_step(s, n_rand, T, seed)
            assert np.array_equal(b[:cut], orders[e][T - cut:]) and np.array_equal(b[cut:cut + T], orders[e + 1][:min(T, n_rand - cut)])
    # ranks 0..2 of world 3 together hold the one global batch
    for s in (0, steps - 1):
        parts = [su.classic_rays_of_step(s, n_rand, T, seed, r, 3) for r in range(3)]
        assert np.array_equal(np.concatenate(parts), su.classic_rays_of_step(s, n_rand, T, seed))
        assert [len(p) for p in parts] == [n_rand // 3 + (1 if r < n_rand % 3 else 0) for r in range(3)]
    assert not np.array_equal(su.classic_rays_of_step(0, n_rand, T, seed), su.classic_rays_of_step(0, n_rand, T, seed + 1)) or T == n_rand == 1


def test_lrate_decay_is_the_stock_schedule():
    from snerf_amd import classic
    assert classic.lrate_decay(5e-4, 250, 0) == 5e-4
    assert classic.lrate_decay(5e-4, 250, 250000) == 5e-4 * 0.1 ** 1.0
    assert classic.lrate_decay(5e-4, 500, 1234) == 5e-4 * 0.1 ** (1234 / 500000)


# ---- the entries' argument checks ---------------------------------------------------------------------------------------------------
def _tail_args(**kw):
    a = dict(rgb=64, rgb0=128, tgt=192, N=5, ws=256, out=320, g_rgb=384, g_rgb0=448, stream=None)
    a.update(kw)
    return list(a.values())


def _batch_args(**kw):
    a = dict(images=64, images_u8=1, c2w=128, intrinsics=192, i_train=256, n_train=2, n_images=3, H=5, W=7, seed=0, counter=320, n=16, i0=0,
             i1=16, ndc=0, near=2.0, far=6.0, use_viewdirs=1, rows=384, ld=11, rgb=448, stream=None)
    a.update(kw)
    return list(a.values())


def test_new_entries_reject_bad_arguments_without_a_gpu():
    """argument validation happens before any launch (the pointers here are never dereferenced)"""
    _lib_or_skip()
    names = lambda e: [n for _, n in _lib.parse_header()[e]]
    assert names("snerf_classic_loss_tail") == ["rgb", "rgb0", "tgt", "N", "ws", "out", "g_rgb", "g_rgb0", "stream"]
    assert names("snerf_classic_train_batch") == ["images", "images_u8", "c2w", "intrinsics", "i_train", "n_train", "n_images", "H", "W", "seed",
                                                   "counter", "n", "i0", "i1", "ndc", "near", "far", "use_viewdirs", "rows", "ld", "rgb", "stream"]
    bad_tail = [dict(N=0), dict(N=-3), dict(rgb=None), dict(tgt=None), dict(ws=None), dict(out=None), dict(g_rgb=None),
                dict(rgb0=None), dict(g_rgb0=None),                                          # rgb0 and g_rgb0: both or neither
                dict(rgb=66), dict(rgb0=129), dict(tgt=195), dict(out=322), dict(g_rgb=385), dict(g_rgb0=450), dict(ws=258), dict(ws=260)]
    for kw in bad_tail:
        with pytest.raises(_lib.SnerfHipError, match="bad argument"):
            _lib.call("snerf_classic_loss_tail", *_tail_args(**kw))
    ws = lambda n: _lib.query("snerf_classic_loss_tail_ws", n)
    assert [ws(n) for n in (0, -4, 1, 256, 257, 5000, 65536, 1 << 30)] == [0, 0, 16, 16, 32, 16 * 20, 16 * 256, 16 * 256]
    bad_batch = [dict(n=0), dict(n=-1), dict(n_images=0), dict(n_train=0), dict(H=0), dict(W=0), dict(i0=-1), dict(i0=9, i1=8), dict(i1=17),
                 dict(seed=-1), dict(images=None), dict(c2w=None), dict(intrinsics=None), dict(i_train=None), dict(counter=None), dict(rows=None),
                 dict(rgb=None), dict(images_u8=2), dict(images_u8=-1), dict(ld=10), dict(ld=7, use_viewdirs=0), dict(c2w=130), dict(intrinsics=196),
                 dict(counter=324), dict(rows=386), dict(rgb=449), dict(i_train=257), dict(images=65, images_u8=0)]
    for kw in bad_batch:
        with pytest.raises(_lib.SnerfHipError, match="bad argument"):
            _lib.call("snerf_classic_train_batch", *_batch_args(**kw))


def test_ray_batcher_constructor_rejects_what_it_cannot_draw():
    """checked before anything touches a device"""
    from snerf_amd import classic
    img = np.zeros((3, 5, 7, 3), np.uint8)
    pose = np.tile(np.eye(4, dtype=np.float32)[:3], (3, 1, 1))
    mk = lambda images=img, poses=pose, focal=10.0, i_train=(0, 2), N_rand=16, **kw: classic.RayBatcher(images, poses, focal, i_train, N_rand, device="cuda", **kw)
    for kw in (dict(i_train=[]), dict(i_train=[0, 3]), dict(i_train=[-1]), dict(images=np.zeros((3, 5, 7, 4), np.uint8)), dict(poses=pose[:2]),
               dict(focal=[1.0, 2.0]), dict(ori_points=[(1.0, 2.0)]), dict(seed=-1), dict(seed=1 << 63), dict(rank=2, world=2), dict(N_rand=1, world=2),
               dict(N_rand=0)):
        with pytest.raises(ValueError):
            mk(**kw)


# ---- the optimiser state ------------------------------------------------------------------------------------------------------------
def _nets(D=3, W=64, use_viewdirs=True, compute="f32", device="cpu", seed=0, n=2, scale=None):
    from snerf_amd import classic
    torch.manual_seed(seed)
    out = []
    for _ in range(n):
        net = classic.NeRF(D=D, W=W, input_ch=63, input_ch_views=27 if use_viewdirs else 0, output_ch=5, skips=[1] if D < 5 else [4],
                           use_viewdirs=use_viewdirs, compute=compute, device=device)
        with torch.no_grad():
            if scale is not None:
                net.arena.flat.mul_(scale)
                if use_viewdirs:                         # (small weights leave the raw density around its bias: keep it positive, so that rays composite)
                    net.arena.p["alpha_linear.bias"][0] = 0.1
            if not use_viewdirs:                         # a density the default initialisation leaves at relu(< 0) = 0 everywhere has no gradient
                net.arena.p["output_linear.bias"][3] = 0.3
        net.arena.bump()
        out.append(net)
    return out


def test_optimizer_state_round_trips_through_torch_adam():
    from snerf_amd import classic
    from snerf_amd.trainer import ClassicTrainer
    coarse, fine = _nets()                               # (host arenas: nothing here launches a kernel)
    tr = ClassicTrainer(coarse, None, 8, 8, fine, lr=3e-4, betas=(0.8, 0.99), eps=1e-7)
    g = torch.Generator().manual_seed(3)
    tr.m.copy_(torch.randn(tr.m.shape, generator=g)); tr.v.copy_(torch.rand(tr.v.shape, generator=g)); tr.t = 17
    params = list(coarse.parameters()) + list(fine.parameters())
    sd = tr.state_dict()
    assert sd["param_names"] == ["network_fn." + n for n, _ in coarse.named_parameters()] + ["network_fine." + n for n, _ in fine.named_parameters()]
    opt = torch.optim.Adam(params, lr=1.0)
    opt.load_state_dict({k: v for k, v in sd.items() if k != "param_names"})
    assert opt.param_groups[0]["lr"] == 3e-4 and tuple(opt.param_groups[0]["betas"]) == (0.8, 0.99) and opt.param_groups[0]["eps"] == 1e-7
    layout = tr._layout()
    for p, (name, lo, cnt, shape) in zip(params, layout):
        st = opt.state[p]
        assert tuple(p.shape) == tuple(shape) and float(st["step"]) == 17.0
        assert torch.equal(st["exp_avg"].reshape(-1), tr.m[lo:lo + cnt]) and torch.equal(st["exp_avg_sq"].reshape(-1), tr.v[lo:lo + cnt])
    # the fine network's moments sit behind the coarse network's
    assert layout[len(list(coarse.parameters()))][1] == coarse.arena.numel
    # and back: torch's own state_dict (what create_nerf's optimizer saves as optimizer_state_dict) into a fresh trainer
    tr2 = ClassicTrainer(coarse, None, 8, 8, fine)
    tr2.load_state_dict(opt.state_dict())
    used = torch.zeros(tr.m.numel(), dtype=torch.bool)
    for _, lo, cnt, _ in layout:
        used[lo:lo + cnt] = True
    assert torch.equal(tr2.m[used], tr.m[used]) and torch.equal(tr2.v[used], tr.v[used]) and tr2.t == 17
    assert (tr2.lr, tr2.betas, tr2.eps) == (3e-4, (0.8, 0.99), 1e-7)
    # refused loads leave the trainer untouched
    before = (tr2.m.clone(), tr2.v.clone(), tr2.t, tr2.lr, tr2.betas, tr2.eps)
    other = dict(sd, param_names=list(reversed(sd["param_names"])))
    short = torch.optim.Adam(list(coarse.parameters()), lr=1e-3).state_dict()
    wrong = {k: v for k, v in sd.items() if k != "param_names"}
    wrong = dict(wrong, state={i: dict(s, exp_avg=s["exp_avg"].reshape(-1)[:-1]) if i == len(layout) - 1 else s for i, s in wrong["state"].items()})
    steps = {k: v for k, v in sd.items() if k != "param_names"}
    steps = dict(steps, state={i: dict(s, step=torch.tensor(3.0)) if i == 0 else s for i, s in steps["state"].items()})
    for bad in (other, short, wrong, steps):
        with pytest.raises(ValueError):
            tr2.load_state_dict(bad)
        assert torch.equal(tr2.m, before[0]) and torch.equal(tr2.v, before[1]) and (tr2.t, tr2.lr, tr2.betas, tr2.eps) == before[2:]
    # one network for both passes: its parameters once
    shared = ClassicTrainer(coarse, None, 8, 8, None)
    assert len(shared.state_dict()["param_groups"][0]["params"]) == len(list(coarse.parameters())) and shared.m.numel() == coarse.arena.numel


def test_trainer_refuses_what_it_does_not_offer():
    from snerf_amd import classic
    from snerf_amd.trainer import ClassicTrainer
    coarse, fine = _nets()
    rgb_net = classic.NeRF_RGB(D=3, W=64, input_ch=63, input_ch_views=27, output_ch=5, skips=[1], use_viewdirs=True, alpha_model=coarse, compute="f32",
                               device="cpu")
    for args, kw in (((rgb_net, None, 8, 8, fine), {}), ((coarse, None, 8, 8, rgb_net), {}), ((None, None, 8, 8, fine), {}),
                     ((coarse, None, 8, 0, fine), {}), ((coarse, None, 8, 8, coarse), {}), ((coarse, None, 1, 8, fine), {}),
                     ((coarse, None, 8, 8, fine), dict(loss_scale=0.0))):
        with pytest.raises(ValueError):
            ClassicTrainer(*args, **kw)
    with pytest.raises(TypeError):
        ClassicTrainer(coarse, None, 8, 8, fine, ert=(1e-4, 16))
    # create_nerf's render_kwargs_train, as it stands
    kw = {'network_query_fn': None, 'perturb': 1.0, 'N_importance': 8, 'network_fine': fine, 'N_samples': 8, 'network_fn': coarse,
          'use_viewdirs': True, 'white_bkgd': False, 'raw_noise_std': 0.0, 'ndc': False, 'lindisp': False}
    tr = ClassicTrainer(**kw)
    assert tr.N_samples == 8 and tr.network_fine is fine and tr.lr == 5e-4


# ---- GPU: the loss-tail kernel -------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32)


@gpu
@pytest.mark.parametrize("with0", [True, False])
@pytest.mark.parametrize("N", TAIL_N)
def test_loss_tail_kernel_equals_the_host_model(N, with0):
    from snerf_amd import ops
    rgb, rgb0, tgt = _tail_inputs(N)
    rgb0 = rgb0 if with0 else None
    want_out, want_g, want_g0 = tail_model(rgb, rgb0, tgt)
    ref, _, _ = tail_f64(rgb, rgb0, tgt)
    d = lambda a: None if a is None else torch.from_numpy(a).to(DEV)
    need = ops.classic_loss_tail_ws(N)
    assert need == 16 * min(256, -(-N // 256))
    guard = 64
    runs = []
    for _ in range(2):
        ws = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device=DEV)
        out, g, g0 = ops.classic_loss_tail(d(rgb), d(rgb0), d(tgt), ws=ws)
        torch.cuda.synchronize()
        assert bool((ws[need:] == 0xA5).all()), "scratch past snerf_classic_loss_tail_ws(N) bytes was written"
        runs.append((out.cpu(), g.cpu(), None if g0 is None else g0.cpu()))
    (out, g, g0), (out2, g2, g02) = runs
    assert torch.equal(_bits(out), _bits(out2)) and torch.equal(_bits(g), _bits(g2)) and (g0 is None or torch.equal(_bits(g0), _bits(g02)))
    assert np.array_equal(g.numpy().view(np.int32), want_g.view(np.int32))
    assert (g0 is None) == (want_g0 is None) and (g0 is None or np.array_equal(g0.numpy().view(np.int32), want_g0.view(np.int32)))
    err = np.abs(out.numpy().astype(np.float64) - ref)
    print(f"MEASURED classic loss tail N={N} rgb0={with0}: out {out.numpy()} float64 {ref} |err| / ulp {err / ulp32(ref)}")
    assert (err <= ulp32(ref)).all(), (out, ref)
    assert with0 or float(out[2]) == 0.0


# ---- GPU: the batch kernel -----------------------------------------------------------------------------------------------------------
def _scene(T, u8, seed=0):
    n_train, H, W = SCENES[T]
    n = n_train + 1                                       # one image that is never trained on
    rng = np.random.default_rng(seed + T)
    images = rng.integers(0, 256, size=(n, H, W, 3), dtype=np.uint8) if u8 else rng.random((n, H, W, 3), dtype=np.float32)
    poses = np.tile(np.eye(4, dtype=np.float32)[:3], (n, 1, 1))
    poses[:, :, :3] += rng.normal(size=(n, 3, 3)).astype(np.float32) * 0.2
    poses[:, :, 3] = rng.normal(size=(n, 3)).astype(np.float32)
    focal = 8.0 + rng.random(n) * 4
    ori = [(W * 0.5 + float(rng.normal()) * 0.3, H * 0.5 + float(rng.normal()) * 0.3) for _ in range(n)]
    i_train = [2, 0] if n_train == 2 else [3, 0, 1]
    return images, poses, focal, ori, i_train, H, W


@gpu
@pytest.mark.parametrize("u8,use_viewdirs,ndc", [(True, True, False), (False, False, True), (True, False, False), (False, True, True)])
@pytest.mark.parametrize("T", sorted(SCENES))
def test_train_batch_rows_are_render_s_rows_of_the_scheduled_pixels(T, u8, use_viewdirs, ndc):
    from snerf_amd import classic, ops
    images, poses, focal, ori, i_train, H, W = _scene(T, u8)
    near, far, seed = 0.25, 5.5, 5
    # classic.render's own rows, one camera at a time
    cam_rows = [ops.classic_ray_batch(H, W, float(focal[i]), float(ori[i][0]), float(ori[i][1]), poses[i], None, None, None, H * W, ndc, near, far, None,
                                      use_viewdirs, torch.device(DEV)).cpu() for i in range(len(images))]
    decoded = (images / 255.).astype(np.float32) if u8 else images
    for n_rand in (1, 16, T, T + 30):
        mk = lambda **kw: classic.RayBatcher(images, poses, focal, i_train, n_rand, near=near, far=far, ndc=ndc, use_viewdirs=use_viewdirs,
                                             ori_points=ori, seed=seed, device=DEV, **kw)
        b = mk()
        shards = [mk(rank=r, world=3) for r in range(3)] if n_rand >= 3 else []
        steps = -(-2 * T // n_rand) + 1 if n_rand > 1 else 5
        for s in range(steps):
            rays, rgb = b.next()
            px = b.pixels_of_step(s)
            assert tuple(rays.shape) == (n_rand, 11 if use_viewdirs else 8) and tuple(rgb.shape) == (n_rand, 3) and px.shape == (n_rand, 3)
            want = torch.stack([cam_rows[i][r * W + c] for i, r, c in px])
            assert torch.equal(_bits(rays.cpu()), _bits(want)), (T, n_rand, s)
            assert np.array_equal(rgb.cpu().numpy(), decoded[px[:, 0], px[:, 1], px[:, 2]]), (T, n_rand, s)
            assert set(px[:, 0].tolist()) <= set(i_train)
            if shards:
                parts = [sh.next() for sh in shards]
                assert torch.equal(torch.cat([p[0] for p in parts]), rays) and torch.equal(torch.cat([p[1] for p in parts]), rgb)
        torch.cuda.synchronize()
        assert b.step == steps and int(b.counter[0]) == steps and int(b.counter[1]) == 0
    # state: a batcher resumed at step 3 draws step 3
    twin = mk()
    twin.load_state_dict({"seed": seed, "step": 3})
    assert np.array_equal(twin.pixels_of_step(3), b.pixels_of_step(3))
    b2 = mk()
    for _ in range(3):
        b2.next()
    assert b2.state_dict() == {"seed": seed, "step": 3} and torch.equal(twin.next()[0], b2.next()[0])


# ---- GPU: the chain -------------------------------------------------------------------------------------------------------------------
N_RAYS, N_S = 96, 8


def _rays(n, use_viewdirs, seed=1):
    g = torch.Generator().manual_seed(seed)
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    o = torch.randn(n, 3, generator=g) * 0.1 + torch.tensor([0.0, 0.0, 4.0])
    cols = [o, -d, torch.full((n, 1), 2.0), torch.full((n, 1), 6.0)] + ([-d] if use_viewdirs else [])
    return torch.cat(cols, -1).to(DEV), torch.rand(n, 3, generator=g).to(DEV)


def _query_fn(use_viewdirs):
    from snerf_amd import classic
    return classic.make_network_query_fn(classic.get_embedder(10, 0)[0], classic.get_embedder(4, 0)[0] if use_viewdirs else None)


def _pair(big, compute, use_viewdirs=True, seed=0, scale=None):
    """two NeRF 8 x 256 (the fused kernels), or two of 4 layers on the per-layer route: 64 wide in f32, 128 wide in bf16 (the 16-bit tiles
    take W / 2 in multiples of 64: the network refuses a narrower one)"""
    nets = _nets(D=8 if big else 4, W=256 if big else (64 if compute == "f32" else 128), use_viewdirs=use_viewdirs, compute=compute, device=DEV, seed=seed, scale=scale)
    for n in nets:
        n.set_deterministic(True)
    return nets


def _draws(n, ni, seed=2):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, N_S, generator=g).to(DEV), (torch.rand(n, ni, generator=g).to(DEV) if ni else None)


def _autograd_grads(coarse, fine, shared, rays, ni, t_rand, u, g_rgb, g_rgb0, seed, **kw):
    """the autograd route over classic.render_rays, seeded with the tail's own gradients -> {network: {name: .grad}}"""
    from snerf_amd import classic
    nets = [coarse] + ([] if shared or ni == 0 else [fine])
    for net in nets:
        for p in net.parameters():
            p.grad = None
    torch.manual_seed(seed)
    r = classic.render_rays(rays, coarse, _query_fn(rays.shape[1] > 9), N_S, perturb=1.0, N_importance=ni, network_fine=None if shared or ni == 0 else fine,
                            t_rand=t_rand, u=u, **kw)
    if ni > 0:
        torch.autograd.backward([r["rgb_map"], r["rgb0"]], [g_rgb, g_rgb0])
    else:
        torch.autograd.backward([r["rgb_map"]], [g_rgb0])
    return r, [{n: p.grad.clone() for n, p in net.named_parameters()} for net in nets]


def _check_chain(big, compute, ni, shared=False, use_viewdirs=True, **kw):
    from snerf_amd.trainer import ClassicTrainer
    coarse, fine = _pair(big, compute, use_viewdirs)
    rays, tgt = _rays(N_RAYS, use_viewdirs)
    rays0, tgt0 = rays.clone(), tgt.clone()
    t_rand, u = _draws(N_RAYS, ni)
    tr = ClassicTrainer(coarse, None, N_S, ni, None if shared or ni == 0 else fine, perturb=1.0, **kw)
    torch.manual_seed(9)
    loss, out = tr.loss_and_grads(rays, tgt, t_rand=t_rand, u=u)
    got = [x.net.arena.grad.clone() for x in tr.nets]
    g_rgb, g_rgb0 = tr.last_grads
    for x in tr.nets:
        x.net.arena.grad.zero_()
    r, want = _autograd_grads(coarse, fine, shared, rays, ni, t_rand, u, g_rgb, g_rgb0, 9, **kw)
    assert torch.equal(rays, rays0) and torch.equal(tgt, tgt0)
    for k in ("rgb_map", "disp_map", "acc_map", "depth_map", "z_vals_map", "weights") + (("rgb0", "disp0", "acc0", "z_std") if ni else ()):
        assert torch.equal(_bits(out[k]), _bits(r[k].detach())), k
    assert float(loss) == float(out["losses"][0]) and np.isfinite(float(loss))
    for x, g, w in zip(tr.nets, got, want):
        a = x.net.arena
        live = 0
        for n in a.names:
            lo, cnt = a._offs[n]
            assert torch.equal(_bits(g[lo:lo + cnt]), _bits(w[n].reshape(-1))), (n, float((g[lo:lo + cnt] - w[n].reshape(-1)).abs().max()))
            live += int((w[n] != 0).sum())
        assert live > 0.2 * a.numel, "dead gradient"
    assert len(tr.nets) == (1 if shared or ni == 0 else 2)


@gpu
@pytest.mark.parametrize("ni", [0, 8])
@pytest.mark.parametrize("compute", ["bf16", "f32"])
@pytest.mark.parametrize("big", [True, False], ids=["fused_8x256", "per_layer_4x64"])
def test_arena_gradients_equal_the_autograd_route_seeded_with_the_tail_s_gradients(big, compute, ni):
    _check_chain(big, compute, ni)


@gpu
@pytest.mark.parametrize("variant", ["shared_network", "white_bkgd", "raw_noise", "lindisp", "no_viewdirs"])
def test_arena_gradients_of_the_variants(variant):
    kw = dict(shared_network=dict(shared=True), white_bkgd=dict(white_bkgd=True), raw_noise=dict(raw_noise_std=0.5), lindisp=dict(lindisp=True),
              no_viewdirs=dict(use_viewdirs=False))[variant]
    for big in ((True, False) if variant != "no_viewdirs" else (False,)):
        _check_chain(big, "bf16", 8, **kw)


@gpu
def test_given_noise_is_used_as_it_is():
    """noise=(coarse, fine): the values raw2outputs would have drawn from the same generator state give the same bits"""
    from snerf_amd.trainer import ClassicTrainer
    coarse, fine = _pair(False, "f32")
    rays, tgt = _rays(N_RAYS, True)
    t_rand, u = _draws(N_RAYS, 8)
    tr = ClassicTrainer(coarse, None, N_S, 8, fine, raw_noise_std=0.5)
    torch.manual_seed(4)
    _, a = tr.loss_and_grads(rays, tgt, t_rand=t_rand, u=u)
    ga = [x.net.arena.grad.clone() for x in tr.nets]
    for x in tr.nets:
        x.net.arena.grad.zero_()
    torch.manual_seed(4)
    n0 = torch.randn(N_RAYS, N_S, device=DEV) * 0.5
    n1 = torch.randn(N_RAYS, N_S + 8, device=DEV) * 0.5
    torch.manual_seed(77)
    _, b = tr.loss_and_grads(rays, tgt, t_rand=t_rand, u=u, noise=(n0, n1))
    assert torch.equal(a["rgb_map"], b["rgb_map"]) and torch.equal(a["rgb0"], b["rgb0"])
    assert all(torch.equal(g, x.net.arena.grad) for g, x in zip(ga, tr.nets))


# ---- GPU: steps -----------------------------------------------------------------------------------------------------------------------
def _twin(src, big, compute):
    nets = _pair(big, compute)
    for a, b in zip(nets, src):
        a.load_state_dict(b.state_dict())
        a.arena.bump()
    return nets


@gpu
@pytest.mark.parametrize("big", [True, False], ids=["fused_8x256", "per_layer_4x64"])
def test_three_steps_equal_the_autograd_route_followed_by_adam(big):
    """Parameters after 3 steps == the autograd-seeded route + ops.adam_step on each arena, bit for bit; and against torch.optim.Adam on
    the same gradients inside the bound of test_optimizer_tail.py (4 x torch's own fp32 error against float64, in units of lr, times
    the number of steps), under that test's conditions: weights scaled by 1 / 16 at lr = 1e-2, so that one ulp of a stored parameter
    stays inside the bound on the updates."""
    from snerf_amd import ops
    from snerf_amd.trainer import ClassicTrainer
    from test_optimizer_tail import MIP_HP, TRAINER_LR, TRAINER_WEIGHT_SCALE, torch_adam_error
    _, b1, b2, eps = MIP_HP
    lr, ni = TRAINER_LR, 8
    A = _pair(big, "bf16", scale=TRAINER_WEIGHT_SCALE)
    B = _twin(A, big, "bf16")
    rays, tgt = _rays(N_RAYS, True)
    rays0, tgt0 = rays.clone(), tgt.clone()
    tr = ClassicTrainer(A[0], None, N_S, ni, A[1], lr=lr, betas=(b1, b2), eps=eps, perturb=1.0)
    params = [p.detach().clone().requires_grad_(True) for net in B for p in net.parameters()]
    opt = torch.optim.Adam(params, lr=lr, betas=(b1, b2), eps=eps)
    mom = [(torch.zeros_like(net.arena.flat), torch.zeros_like(net.arena.flat)) for net in B]
    per_step = 4 * torch_adam_error(b1, b2, eps, lr, 300)
    worst = 0.0
    for k in range(1, 4):
        t_rand, u = _draws(N_RAYS, ni, seed=10 + k)
        loss, out = tr.step(rays, tgt, t_rand=t_rand, u=u)
        assert tr.t == k and all(float(x.net.arena.grad.abs().max()) == 0.0 for x in tr.nets)
        # the other route on the twin networks
        r = _autograd_tail_step(B, rays, tgt, ni, t_rand, u)
        assert torch.equal(_bits(out["rgb_map"]), _bits(r["rgb_map"].detach())) and torch.equal(_bits(out["losses"]), _bits(r["losses"]))
        grads = [p.grad.clone() for net in B for p in net.parameters()]
        assert sum(int((g != 0).sum()) for g in grads) > 0.2 * sum(g.numel() for g in grads), "dead gradient"
        for net, (m, v) in zip(B, mom):
            for n, p in net.named_parameters():
                net.arena.g[n].copy_(p.grad)
                p.grad = None
            ops.adam_step(net.arena.flat, net.arena.grad, m, v, lr, b1, b2, eps, k, grad_scale=1.0, zero_grad=True, nonfinite="zero")
            net.arena.bump()
        for q, g in zip(params, grads):
            q.grad = g
        opt.step()
        for a, b in zip(A, B):
            assert torch.equal(_bits(a.arena.flat), _bits(b.arena.flat)), k
        got = torch.cat([p.detach().reshape(-1) for net in A for p in net.parameters()]).double()
        want = torch.cat([q.detach().reshape(-1) for q in params]).double()
        assert float(got.abs().max()) < 0.125
        err = float((got - want).abs().max()) / lr
        worst = max(worst, err / k)
        print(f"MEASURED classic trainer step {k}: max |p - p_torch| / lr {err:.3e} (bound {per_step * k:.3e})")
        assert err <= per_step * k, (k, err, per_step * k)
    assert torch.equal(rays, rays0) and torch.equal(tgt, tgt0)
    sd = tr.state_dict()
    assert float(sd["state"][0]["step"]) == 3.0 and torch.equal(sd["state"][0]["exp_avg"].reshape(-1), mom[0][0][:sd["state"][0]["exp_avg"].numel()])


def _autograd_tail_step(nets, rays, tgt, ni, t_rand, u, **kw):
    """render_rays with autograd, the tail kernel on its colour maps, autograd.backward seeded with the tail's gradients: .grad of the
    networks' parameters hold the step's gradients afterwards -> render_rays' dict plus `losses`"""
    from snerf_amd import classic, ops
    for net in nets:
        for p in net.parameters():
            p.grad = None
    r = classic.render_rays(rays, nets[0], _query_fn(True), N_S, perturb=1.0, N_importance=ni, network_fine=nets[1], t_rand=t_rand, u=u, **kw)
    out, g_rgb, g_rgb0 = ops.classic_loss_tail(r["rgb_map"].detach(), r["rgb0"].detach(), tgt)
    torch.autograd.backward([r["rgb_map"], r["rgb0"]], [g_rgb, g_rgb0])
    r["losses"] = out
    return r


@gpu
def test_single_rank_exchange_lands_on_the_plain_step_s_bits(tmp_path):
    import torch.distributed as dist
    from snerf_amd.trainer import ClassicTrainer
    if dist.is_initialized():
        pytest.skip("a process group is already up in this process")
    rays, tgt = _rays(N_RAYS, True)
    A = _pair(False, "bf16")
    B = _twin(A, False, "bf16")
    plain = ClassicTrainer(A[0], None, N_S, 8, A[1], perturb=1.0)
    dist.init_process_group("gloo", init_method=f"file://{tmp_path / 'pg'}", rank=0, world_size=1)
    try:
        coll = ClassicTrainer(B[0], None, N_S, 8, B[1], perturb=1.0, exchange_when_single=True)
        assert coll.single_rank_exchange and coll.world == 1
        coll.broadcast_parameters()
        for k in range(2):
            t_rand, u = _draws(N_RAYS, 8, seed=20 + k)
            la, _ = plain.step(rays, tgt, t_rand=t_rand, u=u)
            lb, _ = coll.step(rays, tgt, t_rand=t_rand, u=u)
            assert float(la) == float(lb)
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    for a, b in zip(A, B):
        assert torch.equal(_bits(a.arena.flat), _bits(b.arena.flat))
    assert torch.equal(plain.m, coll.m) and torch.equal(plain.v, coll.v) and plain.t == coll.t == 2


# ---- GPU: the captured step ---------------------------------------------------------------------------------------------------------
@gpu
def test_replays_equal_eager_steps_on_the_batcher_s_draws():
    from snerf_amd import classic
    from snerf_amd.trainer import ClassicTrainer
    images, poses, focal, ori, i_train, H, W = _scene(162, True)
    mk = lambda: classic.RayBatcher(images, poses, focal, i_train, 50, near=2.0, far=6.0, ndc=False, use_viewdirs=True, ori_points=ori, seed=3, device=DEV)
    A = _pair(False, "bf16")
    B = _twin(A, False, "bf16")
    ba, bb = mk(), mk()
    ba.next(); bb.next()
    s0 = ba.step
    cap = ClassicTrainer(A[0], None, N_S, 8, A[1], lr=1e-3, perturb=1.0)
    eager = ClassicTrainer(B[0], None, N_S, 8, B[1], lr=1e-3, perturb=1.0)
    init = [n.arena.flat.clone() for n in A]
    cap.capture(batcher=ba, warmup=2)
    torch.cuda.synchronize()
    assert ba.step == s0 and int(ba.counter[0]) == s0 and cap.t == 0 and all(torch.equal(n.arena.flat, i) for n, i in zip(A, init))
    assert float(cap.m.abs().max()) == 0.0 and float(cap.v.abs().max()) == 0.0
    k = 3
    torch.manual_seed(5)
    for i in range(k):
        if i == 2:
            cap.lr = 2.5e-4                              # the next replay must use it
        loss_c, out_c = cap.replay()
        losses_c = out_c["losses"].clone()
    torch.manual_seed(5)
    for i in range(k):
        if i == 2:
            eager.lr = 2.5e-4
        rays, tgt = bb.next()
        assert i < k - 1 or (torch.equal(cap.batch[0], rays) and torch.equal(cap.batch[1], tgt))
        loss_e, out_e = eager.step(rays, tgt)
    torch.cuda.synchronize()
    assert torch.equal(_bits(losses_c), _bits(out_e["losses"])) and torch.equal(_bits(out_c["rgb_map"]), _bits(out_e["rgb_map"]))
    for a, b in zip(A, B):
        assert torch.equal(_bits(a.arena.flat), _bits(b.arena.flat))
    assert torch.equal(_bits(cap.m), _bits(eager.m)) and torch.equal(_bits(cap.v), _bits(eager.v))
    assert cap.t == eager.t == k and all(int(x.step_dev) == k for x in cap.nets)
    assert ba.step == bb.step == s0 + k and int(ba.counter[0]) == int(bb.counter[0]) == s0 + k
    assert not any(torch.equal(n.arena.flat, i) for n, i in zip(A, init))
    # the lr change counted: a twin that kept the old rate is elsewhere
    assert float(cap.nets[0].lr_dev) == np.float32(2.5e-4)
