"""Pose refinement on the device: poses.LearnPose, the kernels snerf_pose_apply / snerf_pose_grad, and the learned pose inside
MipTrainer.step and the captured step.

The yardstick is the reference's formula (utils/lie_group_helper.py:47-81), restated once below in torch and evaluated in float64:
R = I + (sin th / th) K + ((1 - cos th) / th^2) K K with K the cross-product matrix of the axis-angle row and th = |r| + 1e-15, the
rays' directions and viewdirs rotated by R and the origins shifted by t."""
import os
import types

import numpy as np
import pytest
import torch

from snerf_amd import _lib, poses

gpu = pytest.mark.gpu
EPS = 2.0 ** -24                                        # half an ulp of 1 in fp32: the relative error of one rounding
NCAM = 3


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def ref_cross_matrix(a):
    o = torch.zeros((), dtype=a.dtype)
    return torch.stack([torch.stack([o, -a[2], a[1]]), torch.stack([a[2], o, -a[0]]), torch.stack([-a[1], a[0], o])])


def ref_rotation(a):
    a = a.to(torch.float64)
    K = ref_cross_matrix(a)
    th = a.norm() + 1e-15
    return torch.eye(3, dtype=torch.float64) + (torch.sin(th) / th) * K + ((1 - torch.cos(th)) / th ** 2) * (K @ K)


def axis(size, seed=0):
    """an axis-angle row of the given length (fp32-representable)"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(3, generator=g, dtype=torch.float64)
    return (a / a.norm() * size).to(torch.float32)


# ---- without a GPU ------------------------------------------------------------------------------------------------------------------
def test_learn_pose_state_dict_and_switches():
    init = torch.eye(4).repeat(5, 1, 1)
    init[:, :3, 3] = torch.arange(15.).view(5, 3)
    p = poses.LearnPose(5, True, False, init)
    sd = p.state_dict()
    assert list(sd) == ["init_c2w", "r", "t"]
    assert tuple(sd["r"].shape) == (5, 3) == tuple(sd["t"].shape) and tuple(sd["init_c2w"].shape) == (5, 4, 4)
    assert sd["r"].dtype == torch.float32 and not p.init_c2w.requires_grad
    assert p.r.requires_grad and not p.t.requires_grad
    q = poses.LearnPose(5, False, True)
    assert not q.r.requires_grad and q.t.requires_grad and list(q.state_dict()) == ["r", "t"]
    # a dict in the layout of the reference's pose/NNNNNN.tar 'model_param' entry
    saved = {"init_c2w": init.clone() * 2, "r": torch.randn(5, 3), "t": torch.randn(5, 3)}
    p.load_state_dict(saved)
    for k, v in saved.items():
        assert torch.equal(p.state_dict()[k], v)


@pytest.mark.parametrize("size", [0.0, 2e-4, 3e-2, 1.0])
def test_learn_pose_forward_against_the_float64_restatement(size):
    init = torch.eye(4).repeat(NCAM, 1, 1)
    init[:, :3, :3] = torch.linalg.qr(torch.randn(NCAM, 3, 3, generator=torch.Generator().manual_seed(5)))[0]
    init[:, :3, 3] = torch.randn(NCAM, 3, generator=torch.Generator().manual_seed(6))
    p = poses.LearnPose(NCAM, True, True, init)
    with torch.no_grad():
        p.r[1] = axis(size, 1) if size else torch.zeros(3)
        p.t[1] = torch.tensor([0.25, -1.5, 3.0])
    only = p(1, transform_only=True).detach()
    want = ref_rotation(p.r[1].detach())
    assert tuple(only.shape) == (4, 4) and only.dtype == torch.float32
    assert (only[:3, :3].double() - want).abs().max() <= 4 * EPS
    assert torch.equal(only[:3, 3], p.t[1].detach()) and torch.equal(only[3], torch.tensor([0., 0., 0., 1.]))
    full = p(1).detach()
    assert torch.equal(full, only @ init[1])
    want_full = want @ init[1, :3, :3].double()
    # each entry of the product: three products of entries within 4 eps of the float64 ones with |init| <= 1 (12 eps), their three
    # roundings (3 eps) and the roundings of two partial sums below 2 (4 eps)
    assert (full[:3, :3].double() - want_full).abs().max() <= (12 + 3 + 4) * EPS
    if size == 0.0:
        assert torch.equal(only[:3], torch.cat([torch.eye(3), p.t[1].detach()[:, None]], 1))      # exactly [I | t]
    q = poses.LearnPose(NCAM, True, True)                                                       # no initial poses: the transform itself
    assert torch.equal(q(2), q(2, transform_only=True)) and torch.equal(q(2), torch.eye(4))


@pytest.mark.parametrize("size", [0.0, 2e-4, 3e-2, 1.0])
def test_gradient_chain_host_model_against_float64_autograd(size):
    g = torch.Generator().manual_seed(11)
    G = torch.randn(3, 3, generator=g, dtype=torch.float64)
    r = (axis(size, 2).double() if size else torch.zeros(3, dtype=torch.float64)).requires_grad_(True)
    (ref_rotation(r) * G).sum().backward()
    got = poses.pose_grad_chain(r.detach(), G)
    assert (got - r.grad).abs().max() <= 1e-12 * G.abs().max(), (got, r.grad)
    if size == 0.0:                                                                             # A = 1 times the skew part of G
        want = torch.stack([G[2, 1] - G[1, 2], G[0, 2] - G[2, 0], G[1, 0] - G[0, 1]])
        assert torch.equal(got, want)


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")


_P = lambda k: 1 << 20 | k << 12                       # distinct fake device addresses, 4096 bytes apart: never dereferenced


def _apply_args(**kw):
    a = dict(r=_P(1), t=_P(2), n_cams=3, cam_dev=None, cam_host=1, origins=_P(3), directions=_P(4), viewdirs=_P(5), n=16, origins_out=_P(6),
             directions_out=_P(7), viewdirs_out=_P(8), pose_out=_P(9), stream=None)
    a.update(kw)
    return list(a.values())


def _grad_args(**kw):
    a = dict(r=_P(1), n_cams=3, cam_dev=None, cam_host=1, g_o=_P(2), g_d=_P(3), g_v=_P(4), directions=_P(5), viewdirs=_P(6), n=1000, ws=_P(7),
             ws_doubles=48, grad_r=_P(8), grad_t=_P(9), stream=None)
    a.update(kw)
    return list(a.values())


def test_pose_entries_reject_bad_arguments_without_a_gpu():
    """argument validation happens before any launch (the pointers here are never dereferenced)"""
    _lib_or_skip()
    assert [n for _, n in _lib.parse_header()["snerf_pose_apply"]] == list(
        dict(r=0, t=0, n_cams=0, cam_dev=0, cam_host=0, origins=0, directions=0, viewdirs=0, n=0, origins_out=0, directions_out=0,
             viewdirs_out=0, pose_out=0, stream=0))
    assert [n for _, n in _lib.parse_header()["snerf_pose_grad"]] == list(
        dict(r=0, n_cams=0, cam_dev=0, cam_host=0, g_o=0, g_d=0, g_v=0, directions=0, viewdirs=0, n=0, ws=0, ws_doubles=0, grad_r=0, grad_t=0,
             stream=0))
    bad_apply = [dict(r=None), dict(origins=None), dict(directions=None), dict(viewdirs=None), dict(origins_out=None),
                 dict(directions_out=None), dict(viewdirs_out=None), dict(n=-1), dict(n_cams=0), dict(cam_host=3), dict(cam_host=-1),
                 dict(directions_out=_P(4)), dict(viewdirs_out=_P(5)), dict(origins_out=_P(3)), dict(directions_out=_P(4) + 12 * 15),
                 dict(viewdirs_out=_P(4)), dict(viewdirs_out=_P(7)), dict(origins_out=_P(8) + 12), dict(pose_out=_P(6) + 180),
                 dict(pose_out=_P(8))]
    for kw in bad_apply:
        with pytest.raises(_lib.SnerfHipError, match="bad argument"):
            _lib.call("snerf_pose_apply", *_apply_args(**kw))
    assert _lib.query("snerf_pose_grad_ws", 1000) == 48 and _lib.query("snerf_pose_grad_ws", 0) == 0
    assert [_lib.query("snerf_pose_grad_ws", n) for n in (1, 256, 257, 5000, 1 << 30)] == [12, 12, 24, 240, 12 * 256]
    bad_grad = [dict(r=None), dict(g_d=None), dict(g_v=None), dict(directions=None), dict(viewdirs=None), dict(ws=None), dict(g_o=None),
                dict(grad_r=None, grad_t=None), dict(n=-1), dict(n_cams=0), dict(cam_host=3), dict(cam_host=-1), dict(ws_doubles=47),
                dict(ws_doubles=0)]
    for kw in bad_grad:
        with pytest.raises(_lib.SnerfHipError, match="bad argument"):
            _lib.call("snerf_pose_grad", *_grad_args(**kw))
    # an empty batch is a no-op, whatever the rest
    none = lambda args: [None if isinstance(v, int) and v >= (1 << 20) else v for v in args]
    assert _lib.call("snerf_pose_apply", *none(_apply_args(n=0))) is None
    assert _lib.call("snerf_pose_grad", *none(_grad_args(n=0, ws_doubles=0))) is None


# ---- GPU: the kernels ---------------------------------------------------------------------------------------------------------------
def _table(size, seed=0):
    """three rows of the given rotation size and a nonzero translation table"""
    r = torch.stack([axis(size, seed + i) if size else torch.zeros(3) for i in range(NCAM)])
    t = torch.randn(NCAM, 3, generator=torch.Generator().manual_seed(seed + 9))
    return r, t


def _rays(n, seed=0):
    g = torch.Generator().manual_seed(100 + seed)
    o, d = torch.randn(n, 3, generator=g), torch.randn(n, 3, generator=g)
    return o, d, d / d.norm(dim=-1, keepdim=True)


@gpu
@pytest.mark.parametrize("cam", [0, 2])
@pytest.mark.parametrize("n", [1, 63, 65, 1000])
def test_pose_apply(n, cam):
    from snerf_amd import ops
    o, d, v = (x.cuda() for x in _rays(n))
    keep = [x.clone() for x in (o, d, v)]
    cam_dev = torch.tensor([cam], dtype=torch.int64, device="cuda")
    zero = torch.zeros(NCAM, 3, device="cuda")
    # (i) the identity, bit for bit
    for got, want in zip(ops.pose_apply(zero, zero, cam, o, d, v), (o, d, v)):
        assert torch.equal(got, want)
    for size in (3e-2, 1.0):
        r, t = (x.cuda() for x in _table(size))
        out = torch.full((3, 4), float("nan"), device="cuda")
        o2, d2, v2 = ops.pose_apply(r, t, cam, o, d, v, pose_out=out)
        # (ii) one fp32 add for the origins; three rounded products, summed with two more roundings, of R rounded once
        assert torch.equal(o2, o + t[cam])
        R = ref_rotation(r[cam].cpu())
        for got, x in ((d2, d), (v2, v)):
            want = x.cpu().double() @ R.T
            err = (got.cpu().double() - want).abs()
            bound = 4 * EPS * x.cpu().double().abs().sum(-1, keepdim=True)
            print(f"pose_apply n={n} cam={cam} |r|={size}: max err / bound = {float((err / bound).max()):.3f}")
            assert bool((err <= bound).all())
        # (iii) device index = host index
        for a, b in zip(ops.pose_apply(r, t, cam_dev, o, d, v), (o2, d2, v2)):
            assert torch.equal(a, b)
        # (iv) no translation
        o3, d3, v3 = ops.pose_apply(r, None, cam, o, d, v)
        assert torch.equal(o3, o) and torch.equal(d3, d2) and torch.equal(v3, v2)
        # (v) the applied transform is the module's
        net = poses.LearnPose(NCAM, True, True)
        net.load_state_dict({"r": r.cpu(), "t": t.cpu()})
        assert (out[:, :3].cpu().double() - R).abs().max() <= 4 * EPS
        assert (out[:, :3].cpu() - net(cam, transform_only=True)[:3, :3].detach()).abs().max() <= 4 * EPS
        assert torch.equal(out[:, 3], t[cam])
        # an index outside the table: nothing is written
        mark = [torch.full_like(x, 7.0) for x in (o, d, v)]
        outside = torch.tensor([NCAM], dtype=torch.int64, device="cuda")
        _lib.call("snerf_pose_apply", r.data_ptr(), t.data_ptr(), NCAM, outside.data_ptr(), 0, o.data_ptr(), d.data_ptr(), v.data_ptr(), n,
                  mark[0].data_ptr(), mark[1].data_ptr(), mark[2].data_ptr(), None, torch.cuda.current_stream().cuda_stream)
        assert all(bool((x == 7.0).all()) for x in mark)
    assert all(torch.equal(a, b) for a, b in zip((o, d, v), keep))                             # the inputs stay as they were
    with pytest.raises(_lib.SnerfHipError, match="bad argument"):                              # outputs may not alias inputs
        _lib.call("snerf_pose_apply", zero.data_ptr(), None, NCAM, None, 0, o.data_ptr(), d.data_ptr(), v.data_ptr(), n, o.data_ptr(),
                  d.data_ptr(), v.data_ptr(), None, torch.cuda.current_stream().cuda_stream)


def _grad_case(n, seed=0):
    g = torch.Generator().manual_seed(200 + seed)
    return tuple(torch.randn(n, 3, generator=g) for _ in range(5))          # g_o, g_d, g_v, d, v


def _grad_bound(G, g_t):
    """36 * 2^-24 * max(|G|, |g_t|): an output is at most 18 products of a G entry with a coefficient of magnitude <= 2, formed in
    double and rounded once"""
    return 36 * EPS * float(max(G.abs().max(), g_t.abs().max()))


@gpu
@pytest.mark.parametrize("n", [1, 63, 65, 1000, 5000])
def test_pose_grad(n):
    from snerf_amd import ops
    from snerf_amd.trainer import shard_bounds
    host = _grad_case(n)
    dev = [x.cuda() for x in host]
    G, g_t = poses.pose_sums(*host)
    bound = _grad_bound(G, g_t)
    for size in (0.0, 2e-4, 3e-2, 1.0):
        r, _ = _table(size, seed=3)
        rd = r.cuda()
        for cam in (0, 2):
            want_r = poses.pose_grad_chain(r[cam], G)
            gr, gt = torch.zeros(NCAM, 3, device="cuda"), torch.zeros(NCAM, 3, device="cuda")
            ops.pose_grad(rd, cam, *dev, gr, gt)
            err_r, err_t = float((gr[cam].cpu().double() - want_r).abs().max()), float((gt[cam].cpu().double() - g_t).abs().max())
            print(f"pose_grad n={n} |r|={size} cam={cam}: err_r / bound = {err_r / bound:.3f}, err_t / bound = {err_t / bound:.3f}")
            assert err_r <= bound and err_t <= bound
            other = [c for c in range(NCAM) if c != cam]
            assert float(gr[other].abs().max()) == 0 and float(gt[other].abs().max()) == 0
            if size == 0.0:                                                                     # A = 1 times the skew part of G
                skew = torch.stack([G[2, 1] - G[1, 2], G[0, 2] - G[2, 0], G[1, 0] - G[0, 1]])
                assert float((gr[cam].cpu().double() - skew).abs().max()) <= bound
            # run-to-run reproducible; the device index gives the same bits
            gr2, gt2 = torch.zeros_like(gr), torch.zeros_like(gt)
            ops.pose_grad(rd, torch.tensor([cam], dtype=torch.int64, device="cuda"), *dev, gr2, gt2)
            assert torch.equal(gr, gr2) and torch.equal(gt, gt2)
            # accumulates into row cam of a pre-filled buffer, the other rows keep their bits
            fr, ft = torch.full((NCAM, 3), 0.5, device="cuda"), torch.full((NCAM, 3), -2.0, device="cuda")
            ops.pose_grad(rd, cam, *dev, fr, ft)
            assert torch.equal(fr[cam], 0.5 + gr[cam]) and torch.equal(ft[cam], -2.0 + gt[cam])
            assert bool((fr[other] == 0.5).all()) and bool((ft[other] == -2.0).all())
            # without a translation gradient
            only = torch.zeros_like(gr)
            ops.pose_grad(rd, cam, None, *dev[1:], only, None)
            assert torch.equal(only, gr)
        # an index outside the table writes nothing
        fr, ft = torch.full((NCAM, 3), 0.5, device="cuda"), torch.full((NCAM, 3), -2.0, device="cuda")
        for outside in (NCAM, -1):
            ops.pose_grad(rd, torch.tensor([outside], dtype=torch.int64, device="cuda"), *dev, fr, ft)
        assert bool((fr == 0.5).all()) and bool((ft == -2.0).all())
        # rank slices add up to the whole batch
        whole_r, whole_t = torch.zeros(NCAM, 3, device="cuda"), torch.zeros(NCAM, 3, device="cuda")
        ops.pose_grad(rd, 1, *dev, whole_r, whole_t)
        for world in (2, 4):
            sr, st = torch.zeros(NCAM, 3, dtype=torch.float64), torch.zeros(NCAM, 3, dtype=torch.float64)
            for rank in range(world):
                a, b = shard_bounds(n, rank, world)
                pr, pt = torch.zeros(NCAM, 3, device="cuda"), torch.zeros(NCAM, 3, device="cuda")
                ops.pose_grad(rd, 1, *[x[a:b].contiguous() for x in dev], pr, pt)
                sr += pr.cpu().double(); st += pt.cpu().double()
            assert float((sr - whole_r.cpu().double()).abs().max()) <= (world + 1) * bound
            assert float((st - whole_t.cpu().double()).abs().max()) <= (world + 1) * bound


# ---- GPU: the trainer ---------------------------------------------------------------------------------------------------------------
def _scene(N=5, H=24, W=40, seed=0):
    rng = np.random.default_rng(seed)
    images = rng.random((N, H, W, 3), dtype=np.float32)
    depths = (rng.random((N, H, W)) * 60 + 2).astype(np.float32)
    depths[rng.random((N, H, W)) < 0.5] = 0
    cams = np.zeros((N, 3, 4), np.float32)
    for i in range(N):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        cams[i, :, :3], cams[i, :, 3] = q, rng.normal(size=3)
    K = np.zeros((N, 3, 3), np.float32)
    K[:, 0, 0], K[:, 1, 1] = rng.uniform(20, 80, N), rng.uniform(20, 80, N)
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = W * rng.uniform(0.4, 0.6, N), H * rng.uniform(0.4, 0.6, N), 1
    conf = rng.random((N, H, W), dtype=np.float32)
    return images, depths, cams, K, conf


N_IMG, I_TRAIN = 5, (0, 1, 3, 4)


def _batcher(n=256, seed=3):
    from snerf_amd import sample_utils as su
    images, depths, cams, K, conf = _scene(N_IMG)
    args = types.SimpleNamespace(no_ndc=True, smooth_loss=False, near_far=False, N_rgb=n)
    return su.ImageRayBatcher(args, images, depths, cams, K, list(I_TRAIN), 2.0, 80.0, camera_index=np.arange(N_IMG) * 10.0, batch_n=n,
                              extras=[conf], seed=seed, device="cuda")


def _model():
    """the small model of tests/test_device_batcher.py, in deterministic mode (weight-gradient partials folded in a fixed order instead of
    fp32 atomics): two routes that feed the step the same bits must then leave the same bits in the arena"""
    from snerf_amd import mipnerf
    torch.manual_seed(0)
    m = mipnerf.MipNerfModel(n_samples=16, N_fine=17, no_warp_sample=0, ray_shape="cone", fn=1, radius=3., transform_idx=0, real=True,
                             rgb_layer=3, hidden_layer=64, density_noise=0., max_deg_point=16, proposal_hidden_layer=64, proposal_loss=True,
                             compute="f32")
    return m.set_deterministic(True)


POSE_LR = 1e-4
POSE_TOL = 1e-3 * POSE_LR * 3          # three Adam steps of about lr each; the routes differ in the rounding of one gradient


def _glue_route(steps, learn_t):
    """today's route: apply_pose_transform in torch, step(ray_grads=True), autograd into a torch LearnPose, torch.optim.Adam"""
    from snerf_amd import sample_utils as su
    from snerf_amd.trainer import MipTrainer
    b, tr = _batcher(), MipTrainer(_model(), lr=5e-4)
    net = poses.LearnPose(N_IMG, True, learn_t).cuda()
    opt = torch.optim.Adam([{"params": [p for p in net.parameters() if p.requires_grad], "lr": POSE_LR}])
    arenas, imgs = [], []
    for s in range(steps):
        rays, trgb, tdep, _, img, ex = b.next()
        imgs.append(int(img))
        moved = su.apply_pose_transform(rays, net(imgs[-1], transform_only=True))
        tr.step(moved, trgb, tdep, ex[0], randomized=False, ray_grads=True)      # (no random draws: both routes run the same step)
        opt.zero_grad()
        leaves = [moved.origins, moved.directions, moved.viewdirs] if learn_t else [moved.directions, moved.viewdirs]
        torch.autograd.backward(leaves, list(tr.last_ray_grads)[-len(leaves):])
        opt.step()
        arenas.append(tr.model.arena.flat.clone())
    return net, opt, arenas, imgs


def _fused_route(steps, learn_t, device_index=True):
    from snerf_amd.trainer import MipTrainer
    net = poses.LearnPose(N_IMG, True, learn_t)
    b, tr = _batcher(), MipTrainer(_model(), lr=5e-4, pose_net=net, pose_lr=POSE_LR)
    arenas = []
    for s in range(steps):
        rays, trgb, tdep, _, img, ex = b.next()
        tr.step(rays, trgb, tdep, ex[0], randomized=False, img_i=img if device_index else int(img))
        assert len(tr.last_ray_grads) == 3 and tuple(tr.last_ray_grads[1].shape) == (256, 3)
        arenas.append(tr.model.arena.flat.clone())
    return net, tr, arenas


@gpu
@pytest.mark.parametrize("learn_t", [True, False])
def test_trainer_fused_pose_step_against_the_glue_route(learn_t):
    ref_net, ref_opt, ref_arenas, imgs = _glue_route(3, learn_t)
    net, tr, arenas = _fused_route(3, learn_t)
    assert torch.equal(arenas[0], ref_arenas[0])                  # step 1: r = 0, the rays are bit-identical
    assert len(set(imgs)) == 3
    for name in ("r", "t"):
        got, want = getattr(net, name).detach(), getattr(ref_net, name).detach()
        diff = float((got - want).abs().max())
        print(f"learn_t={learn_t} {name}: max |fused - glue| = {diff:.3e} (bound {POSE_TOL:.1e}), max |{name}| = {float(want.abs().max()):.3e}")
        assert diff <= POSE_TOL
        unvisited = [i for i in range(N_IMG) if i not in imgs]
        assert float(got[unvisited].abs().max()) == 0              # never visited: exactly where they started
    assert float(net.r.detach()[imgs].abs().min()) > 0.1 * POSE_LR  # the visited rows moved
    if not learn_t:
        assert float(net.t.detach().abs().max()) == 0 and not net.t.requires_grad
    # a python int as the index trains the same bits as the device tensor
    net_i, tr_i, _ = _fused_route(3, learn_t, device_index=False)
    assert torch.equal(net_i.r.detach(), net.r.detach()) and torch.equal(net_i.t.detach(), net.t.detach())
    # the optimiser state: round trip, and into a real torch.optim.Adam over a torch LearnPose
    sd = tr.pose_state_dict()
    assert len(sd["state"]) == (2 if learn_t else 1) and float(sd["state"][0]["step"]) == 3 and sd["param_groups"][0]["lr"] == POSE_LR
    net2 = poses.LearnPose(N_IMG, True, learn_t)
    net2.load_state_dict(net.state_dict())
    from snerf_amd.trainer import MipTrainer
    tr2 = MipTrainer(_model(), lr=5e-4, pose_net=net2, pose_lr=7.0)
    tr2.load_pose_state_dict(sd)
    assert tr2.pose.t == 3 and tr2.pose.lr == POSE_LR and torch.equal(tr2.pose.m, tr.pose.m) and torch.equal(tr2.pose.v, tr.pose.v)
    torch_net = poses.LearnPose(N_IMG, True, learn_t).cuda()
    opt = torch.optim.Adam([{"params": [p for p in torch_net.parameters() if p.requires_grad], "lr": 1.0}])
    opt.load_state_dict(sd)
    assert opt.param_groups[0]["lr"] == POSE_LR and torch.equal(opt.state[torch_net.r]["exp_avg"], tr.pose.m[:3 * N_IMG].view(-1, 3))
    # ... and the other way round: what the glue route's torch.optim.Adam saved loads here, with its moments within the routes' difference
    tr2.load_pose_state_dict(ref_opt.state_dict())
    assert tr2.pose.t == 3 and torch.equal(tr2.pose.m[:3 * N_IMG].view(-1, 3), ref_opt.state[ref_net.r]["exp_avg"])


@gpu
def test_trainer_pose_step_needs_the_image_index():
    from snerf_amd.trainer import MipTrainer
    b = _batcher()
    rays, trgb, tdep, _, img, ex = b.next()
    with pytest.raises(ValueError, match="img_i"):
        MipTrainer(_model(), pose_net=poses.LearnPose(N_IMG, True, True)).step(rays, trgb, tdep, ex[0])
    with pytest.raises(ValueError, match="pose_net"):
        MipTrainer(_model()).step(rays, trgb, tdep, ex[0], img_i=img)
    with pytest.raises(ValueError, match="neither"):
        MipTrainer(_model(), pose_net=poses.LearnPose(N_IMG, False, False))
    # a module whose parameters were reallocated after the trainer took it is refused, not trained past
    net = poses.LearnPose(N_IMG, True, True)
    tr = MipTrainer(_model(), pose_net=net)
    tr.step(rays, trgb, tdep, ex[0], img_i=img)
    net.double()
    with pytest.raises(RuntimeError, match="flat pose buffer"):
        tr.step(rays, trgb, tdep, ex[0], img_i=img)


@gpu
def test_capture_with_pose_net_trains_the_table_inside_the_graph():
    from snerf_amd.trainer import MipTrainer
    torch.manual_seed(1)
    eager_b = _batcher()
    imgs = [int(eager_b.next()[4]) for _ in range(3)]
    b = _batcher()
    net = poses.LearnPose(N_IMG, True, True)
    tr = MipTrainer(_model(), lr=5e-4, pose_net=net, pose_lr=POSE_LR)
    init = tr.model.arena.flat.clone()
    tr.capture(None, None, randomized=True, warmup=2, batcher=b, conf_extra=0)
    torch.cuda.synchronize()
    # capturing trains nothing
    assert torch.equal(tr.model.arena.flat, init) and float(tr.m.abs().max()) == 0 and float(tr.v.abs().max()) == 0 and tr.t == 0
    assert float(tr.pose.flat.abs().max()) == 0 and float(tr.pose.m.abs().max()) == 0 and float(tr.pose.v.abs().max()) == 0
    assert float(tr.pose.grad.abs().max()) == 0 and tr.pose.t == 0 and int(tr.pose.step_dev) == 0
    assert b.step == 0 and int(b.counter[0]) == 0
    for k in range(3):
        loss, _ = tr.replay()
        assert int(tr.batch[4]) == imgs[k] and np.isfinite(float(loss))
    assert tr.t == 3 and tr.pose.t == 3 and int(tr.pose.step_dev) == 3 and b.step == 3
    r, t = net.r.detach(), net.t.detach()
    assert float(r[imgs].abs().min()) > 0.1 * POSE_LR and float(t[imgs].abs().max()) > 0.1 * POSE_LR
    unvisited = [i for i in range(N_IMG) if i not in imgs]
    assert float(r[unvisited].abs().max()) == 0 and float(t[unvisited].abs().max()) == 0
    # the table after three replays against three eager fused steps from the same state (without random draws, so that both run the same steps)
    def run(captured):
        torch.manual_seed(7)
        bb, nn_ = _batcher(), poses.LearnPose(N_IMG, True, True)
        tt = MipTrainer(_model(), lr=5e-4, pose_net=nn_, pose_lr=POSE_LR)
        if captured:
            tt.capture(None, None, randomized=False, warmup=2, batcher=bb, conf_extra=0)
            for _ in range(3):
                tt.replay()
        else:
            for _ in range(3):
                rays, trgb, tdep, _, img, ex = bb.next()
                tt.step(rays, trgb, tdep, ex[0], randomized=False, img_i=img)
        return nn_.r.detach().clone(), nn_.t.detach().clone(), tt.model.arena.flat.clone()
    (r_g, t_g, a_g), (r_e, t_e, a_e) = run(True), run(False)
    print(f"captured vs eager: max |r| diff {float((r_g - r_e).abs().max()):.3e}, max |t| diff {float((t_g - t_e).abs().max()):.3e} (bound {POSE_TOL:.1e})")
    assert float((r_g - r_e).abs().max()) <= POSE_TOL and float((t_g - t_e).abs().max()) <= POSE_TOL
    assert float(r_g[imgs].abs().min()) > 0.1 * POSE_LR
