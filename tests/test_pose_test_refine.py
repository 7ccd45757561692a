"""Test-time pose refinement (s-nerf/eval.py:77-114, --test_refine_iter): the composed pose kernels snerf_pose_compose_apply /
snerf_pose_compose_grad, the backward pass without weight gradients, and MipTrainer(freeze_model=True, pose_compose=True).

The yardstick is the reference's procedure restated in float64 torch: the learned transform make_c2w(r, t) = [R(r) | t] (R as in
tests/test_pose_refine.py: lie_group_helper.py:47-81) times the image's initial pose, and pinhole rays generated from that matrix
(origin = its translation column, direction = its rotation times the camera-frame direction, viewdir = the normalised direction).
On the rays of the INITIAL pose that is o' = R o + t, d' = R d, v' = R v: the identity the feature rests on, checked first."""
import numpy as np
import pytest
import torch

from snerf_amd import _lib, poses

from test_pose_refine import (EPS, N_IMG, NCAM, POSE_LR, POSE_TOL, _batcher, _grad_bound, _lib_or_skip, _model, _P, _rays, _table, axis,
                              ref_rotation)

gpu = pytest.mark.gpu
SIZES = (0.0, 2e-4, 3e-2, 1.0)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def ref_rays(c2w, cam_dirs):
    """pinhole rays of a [3,4] camera-to-world matrix for camera-frame directions [n,3] -> (origins, directions, viewdirs), float64"""
    d = cam_dirs @ c2w[:, :3].T
    return c2w[:, 3].expand_as(d), d, d / d.norm(dim=-1, keepdim=True)


def ref_composed(r, t, init):
    """make_c2w(r, t) @ init_c2w (eval.py:88-89), its top three rows"""
    top = torch.cat([ref_rotation(r), t[:, None]], 1)
    return top @ init


def _init_pose(seed=4):
    g = torch.Generator().manual_seed(seed)
    q = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))[0]
    init = torch.eye(4, dtype=torch.float64)
    init[:3, :3], init[:3, 3] = q, torch.randn(3, generator=g, dtype=torch.float64) * 3
    return init


# ---- without a GPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
def test_composed_host_model_against_float64_autograd_of_the_reference_procedure(size):
    n = 50
    g = torch.Generator().manual_seed(21)
    init = _init_pose()
    cam_dirs = torch.cat([torch.randn(n, 2, generator=g, dtype=torch.float64), -torch.ones(n, 1, dtype=torch.float64)], 1)
    w_o, w_d, w_v = (torch.randn(n, 3, generator=g, dtype=torch.float64) for _ in range(3))      # d loss / d (o', d', v') of a linear loss
    r = (axis(size, 2).double() if size else torch.zeros(3, dtype=torch.float64)).requires_grad_(True)
    t = torch.tensor([0.25, -1.5, 3.0], dtype=torch.float64, requires_grad=True)
    o2, d2, v2 = ref_rays(ref_composed(r, t, init), cam_dirs)
    ((w_o * o2).sum() + (w_d * d2).sum() + (w_v * v2).sum()).backward()
    o, d, v = ref_rays(init[:3], cam_dirs)                                                       # the rays of the initial pose
    # the identity: composing the poses = applying the delta to the initial pose's rays, centre included
    R = ref_rotation(r.detach())
    for got, want in ((o2, o @ R.T + t.detach()), (d2, d @ R.T), (v2, v @ R.T)):
        assert (got.detach() - want).abs().max() <= 1e-13 * max(1.0, float(want.abs().max()))
    G, g_t = poses.pose_sums(w_o, w_d, w_v, d, v, origins=o)
    got = poses.pose_grad_chain(r.detach(), G)
    bound = 1e-12 * float(G.abs().max())
    assert (got - r.grad).abs().max() <= bound, (got, r.grad)
    assert (g_t - t.grad).abs().max() <= bound
    # the origin term is there: without it the sums are those of the training-time route, whose five-argument call keeps working
    G5, g_t5 = poses.pose_sums(w_o, w_d, w_v, d, v)
    assert torch.equal(g_t5, g_t) and torch.equal(G, G5 + w_o.T @ o)
    assert (poses.pose_grad_chain(r.detach(), G5) - r.grad).abs().max() > 1e3 * bound


def _apply_args(**kw):
    a = dict(r=_P(1), t=_P(2), n_cams=3, cam_dev=None, cam_host=1, origins=_P(3), directions=_P(4), viewdirs=_P(5), n=16, origins_out=_P(6),
             directions_out=_P(7), viewdirs_out=_P(8), pose_out=_P(9), stream=None)
    a.update(kw)
    return list(a.values())


def _grad_args(**kw):
    a = dict(r=_P(1), n_cams=3, cam_dev=None, cam_host=1, g_o=_P(2), g_d=_P(3), g_v=_P(4), origins=_P(10), directions=_P(5), viewdirs=_P(6), n=1000,
             ws=_P(7), ws_doubles=48, grad_r=_P(8), grad_t=_P(9), stream=None)
    a.update(kw)
    return list(a.values())


def test_composed_pose_entries_reject_bad_arguments_without_a_gpu():
    """argument validation happens before any launch (the pointers here are never dereferenced)"""
    _lib_or_skip()
    hdr = _lib.parse_header()
    assert [n for _, n in hdr["snerf_pose_compose_apply"]] == list(
        dict(r=0, t=0, n_cams=0, cam_dev=0, cam_host=0, origins=0, directions=0, viewdirs=0, n=0, origins_out=0, directions_out=0,
             viewdirs_out=0, pose_out=0, stream=0))
    assert [n for _, n in hdr["snerf_pose_compose_grad"]] == list(
        dict(r=0, n_cams=0, cam_dev=0, cam_host=0, g_o=0, g_d=0, g_v=0, origins=0, directions=0, viewdirs=0, n=0, ws=0, ws_doubles=0, grad_r=0,
             grad_t=0, stream=0))
    assert hdr["snerf_pose_compose_apply"] == hdr["snerf_pose_apply"]                            # the same signature, type for type
    bad_apply = [dict(r=None), dict(origins=None), dict(directions=None), dict(viewdirs=None), dict(origins_out=None),
                 dict(directions_out=None), dict(viewdirs_out=None), dict(n=-1), dict(n_cams=0), dict(cam_host=3), dict(cam_host=-1),
                 dict(directions_out=_P(4)), dict(viewdirs_out=_P(5)), dict(origins_out=_P(3)), dict(directions_out=_P(4) + 12 * 15),
                 dict(viewdirs_out=_P(4)), dict(viewdirs_out=_P(7)), dict(origins_out=_P(8) + 12), dict(pose_out=_P(6) + 180),
                 dict(pose_out=_P(8))]
    for kw in bad_apply:
        with pytest.raises(_lib.SnerfHipError, match="bad argument"):
            _lib.call("snerf_pose_compose_apply", *_apply_args(**kw))
    bad_grad = [dict(r=None), dict(g_o=None), dict(g_d=None), dict(g_v=None), dict(origins=None), dict(directions=None), dict(viewdirs=None),
                dict(ws=None), dict(g_o=None, grad_t=None), dict(grad_r=None, grad_t=None), dict(n=-1), dict(n_cams=0), dict(cam_host=3),
                dict(cam_host=-1), dict(ws_doubles=47), dict(ws_doubles=0)]
    for kw in bad_grad:
        with pytest.raises(_lib.SnerfHipError, match="bad argument"):
            _lib.call("snerf_pose_compose_grad", *_grad_args(**kw))
    # an empty batch is a no-op, whatever the rest
    none = lambda args: [None if isinstance(v, int) and v >= (1 << 20) else v for v in args]
    assert _lib.call("snerf_pose_compose_apply", *none(_apply_args(n=0))) is None
    assert _lib.call("snerf_pose_compose_grad", *none(_grad_args(n=0, ws_doubles=0))) is None


# ---- GPU: the kernels ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cam", [0, 2])
@pytest.mark.parametrize("n", [1, 63, 65, 1000])
def test_pose_compose_apply(n, cam):
    from snerf_amd import ops
    o, d, v = (x.cuda() for x in _rays(n))
    keep = [x.clone() for x in (o, d, v)]
    cam_dev = torch.tensor([cam], dtype=torch.int64, device="cuda")
    zero = torch.zeros(NCAM, 3, device="cuda")
    # (i) the identity, bit for bit, with a zero and with no translation
    for t in (zero, None):
        for got, want in zip(ops.pose_compose_apply(zero, t, cam, o, d, v), (o, d, v)):
            assert torch.equal(got, want)
    for size in SIZES:
        r, t = (x.cuda() for x in _table(size))
        out = torch.full((3, 4), float("nan"), device="cuda")
        o2, d2, v2 = ops.pose_compose_apply(r, t, cam, o, d, v, pose_out=out)
        R = ref_rotation(r[cam].cpu())
        # (ii) a rotated vector: three rounded products, summed with two more roundings, of R rounded once (test_pose_apply's bound); the
        # origins: that bound on o, and the one rounding of the sum with t
        rot_bound = lambda x: 4 * EPS * x.cpu().double().abs().sum(-1, keepdim=True)
        for name, got, x in (("d", d2, d), ("v", v2, v)):
            err = (got.cpu().double() - x.cpu().double() @ R.T).abs()
            print(f"pose_compose_apply n={n} cam={cam} |r|={size} {name}: max err / bound = {float((err / rot_bound(x)).max()):.3f}")
            assert bool((err <= rot_bound(x)).all())
        want_o = o.cpu().double() @ R.T + t[cam].cpu().double()
        err, bound = (o2.cpu().double() - want_o).abs(), rot_bound(o) + EPS * want_o.abs()
        print(f"pose_compose_apply n={n} cam={cam} |r|={size} o: max err / bound = {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all())
        # (iii) no translation: R o alone, and the translated origins are that plus t in one fp32 add
        o3, d3, v3 = ops.pose_compose_apply(r, None, cam, o, d, v)
        assert bool(((o3.cpu().double() - o.cpu().double() @ R.T).abs() <= rot_bound(o)).all())
        assert torch.equal(o2, o3 + t[cam]) and torch.equal(d3, d2) and torch.equal(v3, v2)
        # (iv) directions and viewdirs are the training-time route's, bit for bit; the origins are not (unless R = I)
        o1, d1, v1 = ops.pose_apply(r, t, cam, o, d, v)
        assert torch.equal(d1, d2) and torch.equal(v1, v2) and (size == 0.0) == torch.equal(o1, o2)
        # (v) device index = host index
        for a, b in zip(ops.pose_compose_apply(r, t, cam_dev, o, d, v), (o2, d2, v2)):
            assert torch.equal(a, b)
        # (vi) the applied transform is the module's
        net = poses.LearnPose(NCAM, True, True)
        net.load_state_dict({"r": r.cpu(), "t": t.cpu()})
        assert (out[:, :3].cpu().double() - R).abs().max() <= 4 * EPS
        assert (out[:, :3].cpu() - net(cam, transform_only=True)[:3, :3].detach()).abs().max() <= 4 * EPS
        assert torch.equal(out[:, 3], t[cam])
        # an index outside the table: nothing is written
        mark = [torch.full_like(x, 7.0) for x in (o, d, v)]
        outside = torch.tensor([NCAM], dtype=torch.int64, device="cuda")
        _lib.call("snerf_pose_compose_apply", r.data_ptr(), t.data_ptr(), NCAM, outside.data_ptr(), 0, o.data_ptr(), d.data_ptr(), v.data_ptr(), n,
                  mark[0].data_ptr(), mark[1].data_ptr(), mark[2].data_ptr(), None, torch.cuda.current_stream().cuda_stream)
        assert all(bool((x == 7.0).all()) for x in mark)
    assert all(torch.equal(a, b) for a, b in zip((o, d, v), keep))                             # the inputs stay as they were
    with pytest.raises(_lib.SnerfHipError, match="bad argument"):                              # outputs may not alias inputs
        _lib.call("snerf_pose_compose_apply", zero.data_ptr(), None, NCAM, None, 0, o.data_ptr(), d.data_ptr(), v.data_ptr(), n, o.data_ptr(),
                  d.data_ptr(), v.data_ptr(), None, torch.cuda.current_stream().cuda_stream)


def _grad_case(n, seed=0):
    g = torch.Generator().manual_seed(300 + seed)
    return tuple(torch.randn(n, 3, generator=g) for _ in range(6))          # g_o, g_d, g_v, o, d, v


@gpu
@pytest.mark.parametrize("n", [1, 63, 65, 1000, 5000])
def test_pose_compose_grad(n):
    from snerf_amd import ops
    from snerf_amd.trainer import shard_bounds
    host = _grad_case(n)
    dev = [x.cuda() for x in host]
    g_o, g_d, g_v, o, d, v = host
    G, g_t = poses.pose_sums(g_o, g_d, g_v, d, v, origins=o)
    bound = _grad_bound(G, g_t)
    if n == 5000:
        assert ops.pose_grad_ws(n) > 12                                                         # more than one workgroup partial
    for size in SIZES:
        r, _ = _table(size, seed=3)
        rd = r.cuda()
        for cam in (0, 2):
            want_r = poses.pose_grad_chain(r[cam], G)
            gr, gt = torch.zeros(NCAM, 3, device="cuda"), torch.zeros(NCAM, 3, device="cuda")
            ops.pose_compose_grad(rd, cam, *dev, gr, gt)
            err_r, err_t = float((gr[cam].cpu().double() - want_r).abs().max()), float((gt[cam].cpu().double() - g_t).abs().max())
            print(f"pose_compose_grad n={n} |r|={size} cam={cam}: err_r / bound = {err_r / bound:.3f}, err_t / bound = {err_t / bound:.3f}")
            assert err_r <= bound and err_t <= bound
            other = [c for c in range(NCAM) if c != cam]
            assert float(gr[other].abs().max()) == 0 and float(gt[other].abs().max()) == 0
            # two calls give equal bits; the device index gives the same bits
            gr2, gt2 = torch.zeros_like(gr), torch.zeros_like(gt)
            ops.pose_compose_grad(rd, torch.tensor([cam], dtype=torch.int64, device="cuda"), *dev, gr2, gt2)
            assert torch.equal(gr, gr2) and torch.equal(gt, gt2)
            # accumulates into row cam of a pre-filled buffer, the other rows keep their bits
            fr, ft = torch.full((NCAM, 3), 0.5, device="cuda"), torch.full((NCAM, 3), -2.0, device="cuda")
            ops.pose_compose_grad(rd, cam, *dev, fr, ft)
            assert torch.equal(fr[cam], 0.5 + gr[cam]) and torch.equal(ft[cam], -2.0 + gt[cam])
            assert bool((fr[other] == 0.5).all()) and bool((ft[other] == -2.0).all())
            # without a translation gradient: the origin term of the rotation's gradient stays
            only = torch.zeros_like(gr)
            ops.pose_compose_grad(rd, cam, *dev, only, None)
            assert torch.equal(only, gr)
        # an index outside the table writes nothing
        fr, ft = torch.full((NCAM, 3), 0.5, device="cuda"), torch.full((NCAM, 3), -2.0, device="cuda")
        for outside in (NCAM, -1):
            ops.pose_compose_grad(rd, torch.tensor([outside], dtype=torch.int64, device="cuda"), *dev, fr, ft)
        assert bool((fr == 0.5).all()) and bool((ft == -2.0).all())
        # rank slices add up to the whole batch
        whole_r, whole_t = torch.zeros(NCAM, 3, device="cuda"), torch.zeros(NCAM, 3, device="cuda")
        ops.pose_compose_grad(rd, 1, *dev, whole_r, whole_t)
        for world in (2, 4):
            sr, st = torch.zeros(NCAM, 3, dtype=torch.float64), torch.zeros(NCAM, 3, dtype=torch.float64)
            for rank in range(world):
                a, b = shard_bounds(n, rank, world)
                pr, pt = torch.zeros(NCAM, 3, device="cuda"), torch.zeros(NCAM, 3, device="cuda")
                ops.pose_compose_grad(rd, 1, *[x[a:b].contiguous() for x in dev], pr, pt)
                sr += pr.cpu().double(); st += pt.cpu().double()
            assert float((sr - whole_r.cpu().double()).abs().max()) <= (world + 1) * bound
            assert float((st - whole_t.cpu().double()).abs().max()) <= (world + 1) * bound


# ---- GPU: the backward pass without weight gradients ----------------------------------------------------------------------------------
def _wide_model(compute):
    """the shipped widths (hidden 1024: the fused colour head's shape) on the small sample counts, deterministic"""
    from snerf_amd import mipnerf
    torch.manual_seed(0)
    m = mipnerf.MipNerfModel(n_samples=16, N_fine=17, no_warp_sample=0, ray_shape="cone", fn=1, radius=3., transform_idx=0, real=True,
                             rgb_layer=3, hidden_layer=1024, density_noise=0., max_deg_point=16, proposal_loss=True, compute=compute)
    return m.set_deterministic(True)


MODELS = {"f32_64": _model, "bf16_1024": lambda: _wide_model("bf16"), "f16f8_1024": lambda: _wide_model("f16f8")}


def _no_wgrad(monkeypatch):
    from snerf_amd import ops

    def refuse(*a, **k):
        raise AssertionError("a weight-gradient GEMM was launched in a pass without weight gradients")
    monkeypatch.setattr(ops, "linear_wgrad", refuse)


@gpu
@pytest.mark.parametrize("depth", [True, False])
@pytest.mark.parametrize("model", list(MODELS))
def test_frozen_backward_equals_the_full_backward_on_the_data_path(model, depth, monkeypatch):
    """The fused colour head takes any batch (its conditions are on the widths: hidden 1024, 27 view columns, 3 x 128), so the file's 256
    rays (4096 fine rows, 16 row tiles) are the batch; the bf16 case asserts that both of its launches ran."""
    from snerf_amd import ops
    from snerf_amd.trainer import MipTrainer
    rays, trgb, tdep, _, img, ex = _batcher().next()
    tail = (tdep, ex[0]) if depth else (None, None)
    calls = {"fwd": 0, "bwd": 0}

    def counted(key, real):
        def call(*a, **k):
            calls[key] += 1
            return real(*a, **k)
        return call
    for key, name in (("fwd", "fcolour_fwd"), ("bwd", "fcolour_bwd")):
        monkeypatch.setattr(ops, name, counted(key, getattr(ops, name)))
    full = MipTrainer(MODELS[model](), lr=5e-4, pose_net=poses.LearnPose(N_IMG, True, True), pose_lr=POSE_LR)
    full.step(rays, trgb, *tail, randomized=False, img_i=img)
    assert float(full.model.arena.flat.abs().max()) > 0 and full.t == 1
    n_full = dict(calls)
    frozen = MipTrainer(MODELS[model](), lr=5e-4, pose_net=poses.LearnPose(N_IMG, True, True), pose_lr=POSE_LR, freeze_model=True)
    _no_wgrad(monkeypatch)
    frozen.step(rays, trgb, *tail, randomized=False, img_i=img)
    if model == "bf16_1024":
        assert n_full == {"fwd": 1, "bwd": 1} and calls == {"fwd": 2, "bwd": 2}                  # the fused colour head ran, both ways, in both passes
    for name, a, b in zip("odv", frozen.last_ray_grads, full.last_ray_grads):
        assert float(b.abs().max()) > 0 and bool(torch.isfinite(b).all()), name
        assert torch.equal(a, b), (model, depth, name, float((a - b).abs().max()))
    assert float(frozen.model.arena.grad.abs().max()) == 0 and frozen.t == 0
    assert torch.equal(frozen.pose.flat, full.pose.flat)                                         # the same pose gradient, the same pose Adam


def _frozen_route(steps, learn_t=True, **kw):
    from snerf_amd.trainer import MipTrainer
    net = poses.LearnPose(N_IMG, True, learn_t)
    b, tr = _batcher(), MipTrainer(_model(), lr=5e-4, pose_net=net, pose_lr=POSE_LR, **kw)
    imgs = []
    for s in range(steps):
        rays, trgb, tdep, _, img, ex = b.next()
        imgs.append(int(img))
        tr.step(rays, trgb, tdep, ex[0], randomized=False, img_i=img)
    return net, tr, imgs


@gpu
def test_frozen_steps_leave_the_network_where_it_was(monkeypatch):
    from snerf_amd.trainer import MipTrainer
    with pytest.raises(ValueError, match="pose_net"):
        MipTrainer(_model(), freeze_model=True)
    with pytest.raises(ValueError, match="pose_net"):
        MipTrainer(_model(), pose_compose=True)
    _no_wgrad(monkeypatch)
    bumps = []
    net, tr, imgs = _frozen_route(0, freeze_model=True)
    before = tr.model.arena.flat.clone()
    monkeypatch.setattr(tr.model.arena, "bump", lambda: bumps.append(1))
    b = _batcher()
    for _ in range(3):
        rays, trgb, tdep, _, img, ex = b.next()
        imgs.append(int(img))
        loss, _ = tr.step(rays, trgb, tdep, ex[0], randomized=False, img_i=img)
        assert np.isfinite(float(loss))
    a = tr.model.arena
    assert torch.equal(a.flat, before) and float(a.grad.abs().max()) == 0 and not bumps
    assert float(tr.m.abs().max()) == 0 and float(tr.v.abs().max()) == 0 and tr.t == 0
    assert tr.pose.t == 3 and len(set(imgs)) == 3
    r, t = net.r.detach(), net.t.detach()
    assert float(r[imgs].abs().min()) > 0.1 * POSE_LR and float(t[imgs].abs().max()) > 0.1 * POSE_LR
    unvisited = [i for i in range(N_IMG) if i not in imgs]
    assert float(r[unvisited].abs().max()) == 0 and float(t[unvisited].abs().max()) == 0


@gpu
def test_frozen_step_trains_the_table_like_the_full_step_at_model_lr_zero():
    from snerf_amd.trainer import MipTrainer
    net, tr, imgs = _frozen_route(3, freeze_model=True)
    ref_net = poses.LearnPose(N_IMG, True, True)
    b, ref = _batcher(), MipTrainer(_model(), lr=0.0, pose_net=ref_net, pose_lr=POSE_LR)
    init = ref.model.arena.flat.clone()
    for s in range(3):
        rays, trgb, tdep, _, img, ex = b.next()
        ref.step(rays, trgb, tdep, ex[0], randomized=False, img_i=img)
    assert torch.equal(ref.model.arena.flat, init) and ref.t == 3                                # (lr = 0: the full step's network stayed put too)
    assert torch.equal(net.r.detach(), ref_net.r.detach()) and torch.equal(net.t.detach(), ref_net.t.detach())
    assert torch.equal(tr.pose.m, ref.pose.m) and torch.equal(tr.pose.v, ref.pose.v)
    assert float(net.r.detach()[imgs].abs().min()) > 0.1 * POSE_LR


# ---- GPU: the composed pose in the step ---------------------------------------------------------------------------------------------
def _composed_glue_route(steps, learn_t):
    """the caller-side route: R o + t, R d, R v in torch on a torch LearnPose, step(ray_grads=True), autograd, torch.optim.Adam"""
    from snerf_amd.trainer import MipTrainer
    b, tr = _batcher(), MipTrainer(_model(), lr=5e-4)
    net = poses.LearnPose(N_IMG, True, learn_t).cuda()
    opt = torch.optim.Adam([{"params": [p for p in net.parameters() if p.requires_grad], "lr": POSE_LR}])
    arenas, imgs = [], []
    for s in range(steps):
        rays, trgb, tdep, _, img, ex = b.next()
        imgs.append(int(img))
        pose = net(imgs[-1], transform_only=True)
        R, t = pose[:3, :3], pose[:3, 3]
        rot = lambda x: (x[..., None, :] * R).sum(-1)
        moved = rays._replace(origins=rot(rays.origins) + t, directions=rot(rays.directions), viewdirs=rot(rays.viewdirs))
        tr.step(moved, trgb, tdep, ex[0], randomized=False, ray_grads=True)
        opt.zero_grad()
        torch.autograd.backward([moved.origins, moved.directions, moved.viewdirs], list(tr.last_ray_grads))
        opt.step()
        arenas.append(tr.model.arena.flat.clone())
    return net, arenas, imgs


@gpu
@pytest.mark.parametrize("learn_t", [True, False])
def test_trainer_composed_pose_step_against_the_glue_route(learn_t):
    from snerf_amd.trainer import MipTrainer
    ref_net, ref_arenas, imgs = _composed_glue_route(3, learn_t)
    net = poses.LearnPose(N_IMG, True, learn_t)
    b, tr = _batcher(), MipTrainer(_model(), lr=5e-4, pose_net=net, pose_lr=POSE_LR, pose_compose=True)
    arenas = []
    for s in range(3):
        rays, trgb, tdep, _, img, ex = b.next()
        tr.step(rays, trgb, tdep, ex[0], randomized=False, img_i=img)
        arenas.append(tr.model.arena.flat.clone())
    assert torch.equal(arenas[0], ref_arenas[0])                  # step 1: r = 0, the rays are bit-identical
    assert len(set(imgs)) == 3
    for name in ("r", "t"):
        got, want = getattr(net, name).detach(), getattr(ref_net, name).detach()
        diff = float((got - want).abs().max())
        print(f"composed, learn_t={learn_t} {name}: max |fused - glue| = {diff:.3e} (bound {POSE_TOL:.1e}), max |{name}| = {float(want.abs().max()):.3e}")
        assert diff <= POSE_TOL
        unvisited = [i for i in range(N_IMG) if i not in imgs]
        assert float(got[unvisited].abs().max()) == 0
    assert float(net.r.detach()[imgs].abs().min()) > 0.1 * POSE_LR
    if not learn_t:
        assert float(net.t.detach().abs().max()) == 0 and not net.t.requires_grad


# ---- GPU: the drop-in route -----------------------------------------------------------------------------------------------------------
@gpu
def test_drop_in_forward_with_frozen_parameters_returns_ray_gradients_only(monkeypatch):
    rays = _batcher().next()[0]

    def run(freeze):
        m = _model()
        if freeze:
            for p in m.parameters():
                p.requires_grad_(False)
        leaves = [x.detach().clone().requires_grad_(True) for x in (rays.origins, rays.directions, rays.viewdirs)]
        ret = m(rays._replace(origins=leaves[0], directions=leaves[1], viewdirs=leaves[2]), False, False)
        ((ret[1][0] ** 2).mean() + 0.1 * ret[1][1].mean() + 0.05 * ret[0][1].mean()).backward()      # reaches both levels
        return m, [x.grad for x in leaves]
    m_full, want = run(False)
    assert all(p.grad is not None for p in m_full.parameters())
    _no_wgrad(monkeypatch)
    m, got = run(True)
    for a, b in zip(got, want):
        assert float(b.abs().max()) > 0 and torch.equal(a, b)
    assert all(p.grad is None for p in m.parameters())
    assert float(m.arena.grad.abs().max()) == 0


# ---- GPU: the captured step -----------------------------------------------------------------------------------------------------------
@gpu
def test_capture_of_the_frozen_composed_step(monkeypatch):
    from snerf_amd.trainer import MipTrainer
    _no_wgrad(monkeypatch)

    def run(captured):
        torch.manual_seed(7)
        b, net = _batcher(), poses.LearnPose(N_IMG, True, True)
        tr = MipTrainer(_model(), lr=5e-4, pose_net=net, pose_lr=POSE_LR, freeze_model=True, pose_compose=True)
        before = tr.model.arena.flat.clone()
        if captured:
            tr.capture(None, None, randomized=False, warmup=2, batcher=b, conf_extra=0)
            torch.cuda.synchronize()
            # capturing trains nothing
            assert float(tr.pose.flat.abs().max()) == 0 and float(tr.pose.m.abs().max()) == 0 and tr.pose.t == 0 and int(tr.pose.step_dev) == 0
            assert tr.step_dev is None and b.step == 0 and int(b.counter[0]) == 0
            for _ in range(3):
                loss, _ = tr.replay()
                assert np.isfinite(float(loss))
            assert int(tr.pose.step_dev) == 3 and b.step == 3
        else:
            for _ in range(3):
                rays, trgb, tdep, _, img, ex = b.next()
                tr.step(rays, trgb, tdep, ex[0], randomized=False, img_i=img)
        a = tr.model.arena
        assert torch.equal(a.flat, before) and float(a.grad.abs().max()) == 0
        assert float(tr.m.abs().max()) == 0 and float(tr.v.abs().max()) == 0 and tr.t == 0 and tr.pose.t == 3
        return net.r.detach().clone(), net.t.detach().clone()
    (r_g, t_g), (r_e, t_e) = run(True), run(False)
    print(f"captured vs eager (frozen, composed): max |r| diff {float((r_g - r_e).abs().max()):.3e}, max |t| diff {float((t_g - t_e).abs().max()):.3e} "
          f"(bound {POSE_TOL:.1e})")
    assert float((r_g - r_e).abs().max()) <= POSE_TOL and float((t_g - t_e).abs().max()) <= POSE_TOL
    assert float(r_g.abs().max()) > 0.1 * POSE_LR and float(t_g.abs().max()) > 0.1 * POSE_LR
