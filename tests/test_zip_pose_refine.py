"""Path C pose refinement (s-nerfpp/zipnerf/train.py:177-213, 256, 338-344; internal/posenet_v2.py): poses.LearnPoseV2,
zipnerf.apply_pose, the kernels snerf_pose_table / snerf_pose_rays_apply / snerf_pose_rays_grad / snerf_sgd_step, and the per-ray
learned poses inside ZipTrainer.step.

The yardstick is the reference's formula, restated once below in torch and evaluated in float64: row c of the table gives
R_c = I + (sin th / th) K + ((1 - cos th) / th^2) K K (K the cross-product matrix of r_c, th = |r_c| + 1e-15) and t_c * t_ratio; a ray of
camera c gets o + t_c t_ratio and R_c x for x in (directions, viewdirs, base_x, base_y)."""
import importlib.util
import os

import pytest
import torch

from snerf_amd import _lib, poses

gpu = pytest.mark.gpu
EPS = 2.0 ** -24                                        # half an ulp of 1 in fp32: the relative error of one rounding
SIZES = (0.0, 2e-4, 3e-2, 1.0)
KEYS = ("origins", "directions", "viewdirs", "base_x", "base_y")
REFERENCE = os.environ.get("SNERF_REFERENCE", "/root/reference")      # the reference tree of the build container, where there is one


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def ref_rotations(r):
    """[N,3] -> [N,3,3], in the dtype of r"""
    z = torch.zeros_like(r[:, 0])
    K = torch.stack([torch.stack([z, -r[:, 2], r[:, 1]], 1), torch.stack([r[:, 2], z, -r[:, 0]], 1), torch.stack([-r[:, 1], r[:, 0], z], 1)], 1)
    th = r.norm(dim=-1)[:, None, None] + 1e-15
    return torch.eye(3, dtype=r.dtype)[None] + (torch.sin(th) / th) * K + ((1 - torch.cos(th)) / th ** 2) * (K @ K)


def ref_pose(r, t, t_ratio, cam, init=None):
    """float64 [B,4,4]: make_c2w(r, t * t_ratio)[cam] (@ init[cam])"""
    top = torch.cat([ref_rotations(r), (t * t_ratio)[:, :, None]], 2)
    c2w = torch.cat([top, torch.tensor([0., 0., 0., 1.], dtype=r.dtype).expand(r.shape[0], 1, 4)], 1)[cam]
    return c2w if init is None else c2w @ init[cam]


def axis(size, seed=0):
    """an axis-angle row of the given length (fp32-representable)"""
    a = torch.randn(3, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    return (a / a.norm() * size).to(torch.float32)


def table(n_cams, size=None, seed=0):
    """r [n_cams,3] with rows of length `size` (None: the four SIZES in turn) and t [n_cams,3] in [-1, 1]"""
    r = torch.stack([axis(SIZES[i % 4] if size is None else size, seed + i) for i in range(n_cams)])
    t = torch.rand(n_cams, 3, generator=torch.Generator().manual_seed(seed + 99)) * 2 - 1
    return r, t


def rot_grad_bound(size, gmax):
    """What fp32 autograd through the formula can be held to against float64, per component of d loss / d r, for |G| <= gmax:
    dL/dr_k = A <G,E_k> + B <G,E_k K + K E_k> + (A' <G,K> + B' <G,K K>) r_k / |r|.  In fp32, 1 - cos th carries an absolute error of up to
    EPS, so B is off by EPS / th^2 and B' (two terms of size 1 / th and 2 (1 - cos th) / th^3) by 2 EPS / th^3, and A' (cos th / th - sin th
    / th^2, each rounded) by 2 EPS / th; the factors they meet are |<G,E_k K + K E_k>| <= 6 th gmax, |<G,K K>| <= 9 th^2 gmax,
    |<G,K>| <= 6 th gmax: (6 + 18) EPS gmax / th + 12 EPS gmax, and 6 EPS gmax for A <G,E_k> with A good to 3 EPS; the remaining roundings
    of at most 18 products are inside the 36 EPS gmax that tests/test_pose_refine.py::_grad_bound allows the double-precision chain.
    At r = 0 the terms through th vanish (K = 0, torch's subgradient of the norm is 0)."""
    return (36 + (24 / size if size else 0)) * EPS * gmax


# ---- without a GPU --------------------------------------------------------------------------------------------------------------------
CAM = torch.tensor([1, 1, 3, 0, 1, 4])                  # batched, with repeats; row 2 is never asked for


def _net(size, t_ratio, init=None, seed=0):
    net = poses.LearnPoseV2(5, True, True, init, t_ratio=t_ratio)
    r, t = table(5, size, seed)
    with torch.no_grad():
        net.r.copy_(r); net.t.copy_(t)
    return net


def _init(seed=5):
    init = torch.eye(4).repeat(5, 1, 1)
    init[:, :3, :3] = torch.linalg.qr(torch.randn(5, 3, 3, generator=torch.Generator().manual_seed(seed)))[0]
    init[:, :3, 3] = torch.rand(5, 3, generator=torch.Generator().manual_seed(seed + 1)) * 2 - 1
    return init


@pytest.mark.parametrize("t_ratio", [1, 0.25])
@pytest.mark.parametrize("size", SIZES)
def test_learn_pose_v2_against_the_float64_restatement(size, t_ratio):
    net = _net(size, t_ratio)
    r64, t64 = net.r.detach().double().requires_grad_(True), net.t.detach().double().requires_grad_(True)
    got = net(CAM)
    want = ref_pose(r64, t64, t_ratio, CAM)
    assert tuple(got.shape) == (6, 4, 4) and got.dtype == torch.float32
    assert (got[:, :3, :3].detach().double() - want[:, :3, :3].detach()).abs().max() <= 4 * EPS
    assert torch.equal(got[:, :3, 3].detach(), (net.t.detach() * t_ratio)[CAM])                 # one fp32 product, as posenet_v2.py:99
    assert torch.equal(got[:, 3].detach(), torch.tensor([0., 0., 0., 1.]).expand(6, 4))
    if size == 0.0:
        assert torch.equal(got[:, :3, :3].detach(), torch.eye(3).expand(6, 3, 3))               # exactly I
    assert torch.equal(net(CAM, transform_only=True), got)                                      # no init_c2w: the transform itself
    assert torch.equal(net(CAM.int()), got) and torch.equal(net(CAM.float().reshape(-1, 1)), got)
    one = net(CAM[2:], one_img=True)
    assert tuple(one.shape) == (1, 4, 4) and torch.equal(one[0], got[2])                        # the row of cam_id[0] alone
    # autograd, against float64 autograd through the restatement
    W = torch.randn(6, 3, 4, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    (got[:, :3] * W.float()).sum().backward()
    (want[:, :3] * W).sum().backward()
    for c in range(5):
        rows = W[CAM == c]
        if rows.shape[0] == 0:
            assert float(net.r.grad[c].abs().max()) == 0 and float(net.t.grad[c].abs().max()) == 0
            continue
        gmax = float(rows[:, :, :3].sum(0).abs().max()) + 3 * EPS * float(rows[:, :, :3].abs().sum(0).max())    # (the repeats add in fp32)
        err = float((net.r.grad[c].double() - r64.grad[c]).abs().max())
        assert err <= rot_grad_bound(size, gmax), (c, err, rot_grad_bound(size, gmax))
        assert float((net.t.grad[c].double() - t64.grad[c]).abs().max()) <= 4 * EPS * float(rows[:, :, 3].abs().sum(0).max())


@pytest.mark.parametrize("size", SIZES)
def test_learn_pose_v2_with_initial_poses(size):
    init = _init()
    net = _net(size, 0.25, init)
    got = net(CAM).detach()
    want = ref_pose(net.r.detach().double(), net.t.detach().double(), 0.25, CAM, init.double())
    # rotation part: three products of entries within 4 eps of the float64 ones with |init| <= 1 (12 eps), their three roundings
    # (3 eps) and the roundings of two partial sums below 2 (4 eps); the translation column adds t * t_ratio, |.| <= 1: one more
    # term (its rounding and a partial sum below 4: 1 + 4 eps more, the earlier partial sums below 4 instead of 2: 4 eps more)
    assert (got[:, :3, :3].double() - want[:, :3, :3]).abs().max() <= (12 + 3 + 4) * EPS
    assert (got[:, :3, 3].double() - want[:, :3, 3]).abs().max() <= (12 + 3 + 4 + 1 + 4 + 4) * EPS
    assert torch.equal(got[:, 3], torch.tensor([0., 0., 0., 1.]).expand(6, 4))
    only = net(CAM, transform_only=True).detach()
    assert (only[:, :3, :3].double() - ref_pose(net.r.detach().double(), net.t.detach().double(), 0.25, CAM)[:, :3, :3]).abs().max() <= 4 * EPS
    assert torch.equal(net(CAM[2:], one_img=True)[0], only[2])                                  # one_img: the bare transform, posenet_v2.py:87-91
    assert list(net.state_dict()) == ["init_c2w", "r", "t"] and not net.init_c2w.requires_grad


def test_learn_pose_v2_state_dict_round_trip():
    net = _net(3e-2, 0.25)
    sd = net.state_dict()
    assert list(sd) == ["r", "t"] and tuple(sd["r"].shape) == (5, 3) == tuple(sd["t"].shape) and sd["r"].dtype == torch.float32
    other = poses.LearnPoseV2(5, True, False, t_ratio=0.25)
    assert other.r.requires_grad and not other.t.requires_grad
    other.load_state_dict(sd)                                                                   # a posenet_ckpt_* dict: the names r, t
    assert torch.equal(other.r, net.r) and torch.equal(other.t, net.t)
    assert torch.equal(other(CAM), net(CAM))


def _reference_class():
    path = os.path.join(REFERENCE, "s-nerfpp", "zipnerf", "internal", "posenet_v2.py")
    if not os.path.exists(path):
        pytest.skip("no reference tree on this machine")
    spec = importlib.util.spec_from_file_location("reference_posenet_v2", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.LearnPose


@pytest.mark.parametrize("t_ratio", [1, 0.25])
@pytest.mark.parametrize("size", SIZES)
def test_learn_pose_v2_against_the_reference_class(size, t_ratio):
    RefPose = _reference_class()
    for init in (None, _init()):
        net = _net(size, t_ratio, init)
        ref = RefPose(5, True, True, None if init is None else init.numpy(), t_ratio=t_ratio)
        ref.load_state_dict(net.state_dict())                                                   # the same names, both ways
        net.load_state_dict(ref.state_dict())
        W = torch.randn(6, 4, 4, generator=torch.Generator().manual_seed(4))
        for only in (False, True):
            net.zero_grad(); ref.zero_grad()
            got, want = net(CAM, transform_only=only), ref(CAM, transform_only=only)
            assert got.shape == want.shape
            scale = 1.0 if (init is None or only) else 4.0                                      # (entries of the product with init_c2w: below 4)
            assert float((got - want).detach().abs().max()) <= 4 * EPS * scale
            (got * W).sum().backward(); (want * W).sum().backward()
            gmax = max(float(ref.r.grad.abs().max()), float(ref.t.grad.abs().max()), float(W.abs().max()))
            assert float((net.r.grad - ref.r.grad).abs().max()) <= 36 * EPS * gmax
            assert float((net.t.grad - ref.t.grad).abs().max()) <= 36 * EPS * gmax


def _grad_case(n, n_cams, assign="random", seed=0):
    """cam fp32 [n] and the nine [n,3] operands of the reduction (g_o, g_d, g_v, g_bx, g_by, d, v, bx, by)"""
    g = torch.Generator().manual_seed(200 + seed + n + 7 * n_cams)
    cam = torch.randint(0, n_cams, (n,), generator=g).float()
    if assign == "one":
        cam.fill_(float(n_cams - 1))
    elif assign == "absent" and n_cams > 1:
        cam[cam == 1] = 0.0
    elif assign == "outside":
        cam += torch.rand(n, generator=g) * 0.75                                                # fractions truncate toward zero
        bad = torch.tensor([-1.0, float(n_cams), float("nan"), -0.5, n_cams + 3.5, -7.0])       # (-0.5 truncates to row 0: inside)
        where = torch.randperm(n, generator=g)[:min(n, 6)]
        cam[where] = bad[:where.shape[0]]
    return cam, [torch.randn(n, 3, generator=g) for _ in range(9)]


@pytest.mark.parametrize("assign", ["random", "absent", "outside"])
def test_host_model_of_the_reduction_against_float64_autograd(assign):
    from snerf_amd import zipnerf
    n, n_cams, t_ratio = 157, 5, 0.25
    cam, ops9 = _grad_case(n, n_cams, assign)
    grads, rays = [x.double() for x in ops9[:5]], [x.double() for x in ops9[5:]]
    net = _net(None, t_ratio).double()
    origins = torch.randn(n, 3, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    batch = dict(zip(KEYS, [origins] + rays), radii=torch.ones(n, 1))
    inside = (torch.trunc(cam) >= 0) & (torch.trunc(cam) < n_cams)
    rows = torch.where(inside, torch.trunc(cam), torch.zeros(())).long()
    moved = zipnerf.apply_pose(batch, net(rows))
    assert moved is not batch and moved["radii"] is batch["radii"] and batch["origins"] is origins      # a new dict, the rest passed on
    loss = sum((moved[k] * g * inside[:, None]).sum() for k, g in zip(KEYS, grads))             # rays outside the table take no part
    loss.backward()
    G, g_t, count = poses.pose_rays_sums(cam, n_cams, *grads, *rays, t_ratio=t_ratio)
    assert torch.equal(count, torch.bincount(rows[inside], minlength=n_cams).double())
    for c in range(n_cams):
        got = poses.pose_grad_chain(net.r[c].detach(), G[c])
        assert float((got - net.r.grad[c]).abs().max()) <= 1e-12 * max(1.0, float(G[c].abs().max())), c
        assert float((g_t[c] - net.t.grad[c]).abs().max()) <= 1e-12 * max(1.0, float(g_t[c].abs().max())), c
        if count[c] == 0:
            assert float(G[c].abs().max()) == 0 and float(g_t[c].abs().max()) == 0
    if assign == "absent":
        assert count[1] == 0
    # the moved rays themselves, against the restatement
    R = ref_rotations(net.r.detach())[rows]
    assert torch.allclose(moved["origins"], origins + (net.t.detach() * t_ratio)[rows], rtol=0, atol=1e-15)
    for k in KEYS[1:]:
        assert torch.allclose(moved[k].detach(), (R @ batch[k][:, :, None])[:, :, 0], rtol=0, atol=1e-14)


def test_pose_sgd_state_round_trips_into_torch_sgd():
    from snerf_amd.trainer import _PoseSGD
    net = poses.LearnPoseV2(5, True, True, t_ratio=0.25)
    ps = _PoseSGD(net, "cpu", 1e-2)
    ps.check_views()
    assert ps.names == ["r", "t"] and ps.flat.numel() == 30 and ps.g["t"].data_ptr() == ps.grad.data_ptr() + 60
    sd = ps.state_dict()
    assert sd == torch.optim.SGD(list(net.parameters()), lr=1e-2).state_dict()
    opt = torch.optim.SGD(list(net.parameters()), lr=0.5)
    opt.load_state_dict(sd)
    assert opt.param_groups[0]["lr"] == 1e-2 and opt.param_groups[0]["momentum"] == 0
    opt.param_groups[0]["lr"] = 3e-3
    net.r.grad = torch.ones_like(net.r); net.t.grad = torch.ones_like(net.t)
    opt.step()                                                                                  # (fills torch's per-parameter state)
    ps.load_state_dict(opt.state_dict())
    assert ps.lr == 3e-3
    ps.lr = 7e-4                                                                                # a plain attribute: the caller's schedule
    assert ps.state_dict()["param_groups"][0]["lr"] == 7e-4
    for bad in (dict(momentum=0.9), dict(weight_decay=1e-4), dict(nesterov=True), dict(maximize=True)):
        sd = ps.state_dict()
        sd["param_groups"][0].update(bad)
        with pytest.raises(ValueError, match="plain SGD"):
            ps.load_state_dict(sd)
    sd = ps.state_dict()
    sd["param_groups"][0]["params"] = [0]
    with pytest.raises(ValueError, match="1 parameters, 2 expected"):
        ps.load_state_dict(sd)
    assert ps.lr == 7e-4
    only_r = _PoseSGD(poses.LearnPoseV2(5, True, False), "cpu", 1e-2)
    assert only_r.names == ["r"] and only_r.flat.numel() == 15 and "t" not in only_r.g
    with pytest.raises(ValueError, match="neither r nor t"):
        _PoseSGD(poses.LearnPoseV2(5, False, False), "cpu", 1e-2)


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")


_P = lambda k: 1 << 20 | k << 12                        # distinct fake device addresses, 4096 bytes apart: never dereferenced


def _args(name, **kw):
    a = {n: None for _, n in _lib.parse_header()[name]}
    a.update(kw)
    return list(a.values())


def _table_args(**kw):
    return _args("snerf_pose_table", **{**dict(r=_P(1), t=_P(2), n_cams=5, t_ratio=0.25, table_out=_P(3)), **kw})


def _apply_args(**kw):
    return _args("snerf_pose_rays_apply", **{**dict(table=_P(1), n_cams=5, cam=_P(2), origins=_P(3), directions=_P(4), viewdirs=_P(5), base_x=_P(6),
                                                    base_y=_P(7), n=16, origins_out=_P(8), directions_out=_P(9), viewdirs_out=_P(10),
                                                    base_x_out=_P(11), base_y_out=_P(12)), **kw})


def _grad_args(**kw):
    return _args("snerf_pose_rays_grad", **{**dict(r=_P(1), n_cams=5, t_ratio=0.25, cam=_P(2), g_o=_P(3), g_d=_P(4), g_v=_P(5), g_bx=_P(6),
                                                   g_by=_P(7), directions=_P(8), viewdirs=_P(9), base_x=_P(10), base_y=_P(11), n=1000, ws=_P(12),
                                                   ws_doubles=13 * 5 * 4, grad_r=_P(13), grad_t=_P(14)), **kw})


def _sgd_args(**kw):
    return _args("snerf_sgd_step", **{**dict(p=_P(1), g=_P(2), count=30, lr=1e-2, grad_scale=1.0, grad_max_val=0.0, nonfinite=1), **kw})


def test_new_entries_reject_bad_arguments_without_a_gpu():
    """argument validation happens before any launch (the pointers here are never dereferenced)"""
    _lib_or_skip()
    names = lambda e: [n for _, n in _lib.parse_header()[e]]
    assert names("snerf_pose_table") == ["r", "t", "n_cams", "t_ratio", "table_out", "stream"]
    assert names("snerf_pose_rays_apply") == ["table", "n_cams", "cam", "origins", "directions", "viewdirs", "base_x", "base_y", "n", "origins_out",
                                              "directions_out", "viewdirs_out", "base_x_out", "base_y_out", "stream"]
    assert names("snerf_pose_rays_grad") == ["r", "n_cams", "t_ratio", "cam", "g_o", "g_d", "g_v", "g_bx", "g_by", "directions", "viewdirs", "base_x",
                                             "base_y", "n", "ws", "ws_doubles", "grad_r", "grad_t", "stream"]
    assert names("snerf_sgd_step") == ["p", "g", "count", "lr", "grad_scale", "grad_max_val", "clip_coef", "nonfinite", "dropped", "stream"]
    for kw in (dict(r=None), dict(table_out=None), dict(n_cams=0), dict(n_cams=-3), dict(table_out=_P(1)), dict(table_out=_P(2)), dict(table_out=_P(1) - 200)):
        with pytest.raises(_lib.SnerfHipError, match="bad argument"):
            _lib.call("snerf_pose_table", *_table_args(**kw))
    ins, outs = ["origins", "directions", "viewdirs", "base_x", "base_y"], ["origins_out", "directions_out", "viewdirs_out", "base_x_out", "base_y_out"]
    bad_apply = [dict(table=None), dict(cam=None), dict(n=-1), dict(n_cams=0), dict(table=_P(1) + 4)] + [{k: None} for k in ins + outs]
    bad_apply += [{o: _P(3 + i)} for o in outs for i in range(5)]                               # an output on an input
    bad_apply += [{o: _P(8 + j)} for i, o in enumerate(outs) for j in range(5) if j != i]       # an output on another output
    bad_apply += [dict(origins_out=_P(4) + 12 * 15), dict(base_y_out=_P(11) + 12), dict(viewdirs_out=_P(1) + 200), dict(base_x_out=_P(2) + 60)]
    for kw in bad_apply:
        with pytest.raises(_lib.SnerfHipError, match="bad argument"):
            _lib.call("snerf_pose_rays_apply", *_apply_args(**kw))
    # the workspace: 13 doubles per camera and slice; slices = min(ceil(n / 256), 256, ceil(2048 / n_cams))
    ws = lambda n, c: _lib.query("snerf_pose_rays_grad_ws", n, c)
    assert [ws(n, 1) for n in (0, -4, 1, 256, 257, 5000, 1 << 30)] == [0, 0, 13, 13, 26, 13 * 20, 13 * 256]
    assert [ws(1000, c) for c in (0, 5, 70, 1000, 4000)] == [0, 13 * 5 * 4, 13 * 70 * 4, 13 * 1000 * 3, 13 * 4000]
    assert ws(65536, 1000) == 13 * 1000 * 3 and ws(65536, 200) == 13 * 200 * 11
    bad_grad = [dict(n=-1), dict(n_cams=0), dict(ws_doubles=13 * 5 * 4 - 1), dict(ws_doubles=0), dict(grad_r=None, grad_t=None), dict(g_o=None)]
    bad_grad += [{k: None} for k in ("r", "cam", "g_d", "g_v", "g_bx", "g_by", "directions", "viewdirs", "base_x", "base_y", "ws")]
    for kw in bad_grad:
        with pytest.raises(_lib.SnerfHipError, match="bad argument"):
            _lib.call("snerf_pose_rays_grad", *_grad_args(**kw))
    for kw in (dict(p=None), dict(g=None), dict(count=-1), dict(nonfinite=3), dict(nonfinite=-1), dict(p=_P(1) + 2), dict(dropped=_P(3) + 4)):
        with pytest.raises(_lib.SnerfHipError, match="bad argument"):
            _lib.call("snerf_sgd_step", *_sgd_args(**kw))
    # an empty batch / buffer is a no-op, whatever the rest
    none = lambda args: [None if isinstance(v, int) and v >= (1 << 20) else v for v in args]
    assert _lib.call("snerf_pose_rays_apply", *none(_apply_args(n=0))) is None
    assert _lib.call("snerf_pose_rays_grad", *none(_grad_args(n=0, ws_doubles=0))) is None
    assert _lib.call("snerf_sgd_step", *none(_sgd_args(count=0))) is None


# ---- GPU: the kernels -----------------------------------------------------------------------------------------------------------------
def _rays(n, seed=0):
    g = torch.Generator().manual_seed(100 + seed + n)
    o, d, bx, by = (torch.randn(n, 3, generator=g) for _ in range(4))
    return [o, d, d / d.norm(dim=-1, keepdim=True), bx, by]


@gpu
@pytest.mark.parametrize("n_cams", [1, 5, 70])
@pytest.mark.parametrize("n", [1, 63, 65, 257, 1000])
def test_pose_table_and_rays_apply(n, n_cams):
    from snerf_amd import ops
    t_ratio = 0.25
    r, t = table(n_cams)
    rays = _rays(n)
    cam, _ = _grad_case(n, n_cams, "outside")
    dev = [x.cuda() for x in rays]
    keep = [x.clone() for x in dev]
    camd = cam.cuda()
    # a zero table returns all five inputs bit for bit
    zero = ops.pose_table(torch.zeros(n_cams, 3, device="cuda"), torch.zeros(n_cams, 3, device="cuda"), t_ratio)
    assert torch.equal(zero, torch.cat([torch.eye(3), torch.zeros(3, 1)], 1).cuda().expand(n_cams, 3, 4))
    for got, x in zip(ops.pose_rays_apply(zero, camd, *dev), dev):
        assert torch.equal(got, x) and got.data_ptr() != x.data_ptr()
    assert torch.equal(ops.pose_table(torch.zeros(n_cams, 3, device="cuda"), None, t_ratio), zero)     # no translation: zeros
    # the table: the rotation within 4 eps of float64, column 3 = fp32(t * t_ratio)
    tab = ops.pose_table(r.cuda(), t.cuda(), t_ratio)
    R64 = ref_rotations(r.double())
    assert float((tab[:, :, :3].cpu().double() - R64).abs().max()) <= 4 * EPS
    assert torch.equal(tab[:, :, 3].cpu(), t * t_ratio)
    for c in range(n_cams):
        if SIZES[c % 4] == 0.0:
            assert torch.equal(tab[c, :, :3].cpu(), torch.eye(3))                               # a row with r = 0: R = I exactly
    # the rays
    out = [x.cpu() for x in ops.pose_rays_apply(tab, camd, *dev)]
    for x, k in zip(dev, keep):
        assert torch.equal(x, k)                                                                # the inputs are never written
    ct = torch.trunc(cam)
    inside = (ct >= 0) & (ct < n_cams)
    rows = torch.where(inside, ct, torch.zeros(())).long()
    assert torch.equal(out[0][inside], (rays[0] + (t * t_ratio)[rows])[inside])
    for got, x in zip(out[1:], rays[1:]):
        # against the float64 product: with |R_ij| <= 1, the rounding of R, of the three products and of the two sums is each at
        # most eps * sum |x|
        want = (R64[rows] @ x.double()[:, :, None])[:, :, 0]
        assert bool(((got.double() - want).abs()[inside] <= 4 * EPS * x.double().abs().sum(-1, keepdim=True)[inside]).all())
    for got, x in zip(out, rays):
        assert torch.equal(got[~inside], x[~inside])                                            # outside the table (-1, n_cams, NaN): passed through
    # aliased outputs are refused
    outs = [torch.empty_like(x) for x in dev]
    call = lambda ins, outs_: _lib.call("snerf_pose_rays_apply", tab.data_ptr(), n_cams, camd.data_ptr(), *[x.data_ptr() for x in ins], n,
                                        *[x.data_ptr() for x in outs_], torch.cuda.current_stream().cuda_stream)
    for i in range(5):
        for bad in (dev[i], dev[(i + 1) % 5], outs[(i + 2) % 5]):
            with pytest.raises(_lib.SnerfHipError, match="bad argument"):
                call(dev, outs[:i] + [bad] + outs[i + 1:])
    call(dev, outs)
    for got, want in zip(outs, out):
        assert torch.equal(got.cpu(), want)


def _row_bounds(G, g_t):
    """per table row, tests/test_pose_refine.py::_grad_bound: 36 * 2^-24 * max(|G_c|, |g_t,c|) -- an output is at most 18 products of a G
    entry with a coefficient of magnitude <= 2, formed in double and rounded once"""
    return 36 * EPS * torch.maximum(G.abs().amax((1, 2)), g_t.abs().amax(1))


def _host_grads(r, cam, n_cams, nine, t_ratio):
    G, g_t, count = poses.pose_rays_sums(cam, n_cams, *nine, t_ratio=t_ratio)
    want_r = torch.stack([poses.pose_grad_chain(r[c], G[c]) if count[c] > 0 else torch.zeros(3, dtype=torch.float64) for c in range(n_cams)])
    return want_r, g_t, count, _row_bounds(G, g_t)


@gpu
@pytest.mark.parametrize("n_cams", [1, 5, 70])
@pytest.mark.parametrize("n", [1, 63, 65, 257, 1000, 5000])
def test_pose_rays_grad(n, n_cams):
    from snerf_amd import ops
    from snerf_amd.trainer import shard_bounds
    t_ratio = 0.25
    r, _ = table(n_cams, 3e-2 if n_cams == 1 else None, seed=3)
    rd = r.cuda()
    worst = 0.0
    for assign in ("random", "one", "absent", "outside"):
        cam, nine = _grad_case(n, n_cams, assign)
        camd, dev = cam.cuda(), [x.cuda() for x in nine]
        want_r, want_t, count, bound = _host_grads(r, cam, n_cams, nine, t_ratio)
        present = count > 0
        gr, gt = torch.zeros(n_cams, 3, device="cuda"), torch.zeros(n_cams, 3, device="cuda")
        ops.pose_rays_grad(rd, t_ratio, camd, *dev, gr, gt)
        err_r, err_t = (gr.cpu().double() - want_r).abs().amax(1), (gt.cpu().double() - want_t).abs().amax(1)
        ratio = float(torch.maximum(err_r, err_t)[present].div(bound[present].clamp_min(1e-300)).max()) if bool(present.any()) else 0.0
        worst = max(worst, ratio)
        assert bool((err_r <= bound).all()) and bool((err_t <= bound).all()), (assign, ratio)
        assert float(gr[~present.cuda()].abs().sum()) == 0 and float(gt[~present.cuda()].abs().sum()) == 0
        if assign == "one":
            assert int(present.sum()) == 1 and bool(present[n_cams - 1])
        if assign == "absent" and n_cams > 1:
            assert not bool(present[1])
        # two runs give the same bits
        gr2, gt2 = torch.zeros_like(gr), torch.zeros_like(gt)
        ops.pose_rays_grad(rd, t_ratio, camd, *dev, gr2, gt2, ws=torch.full((ops.pose_rays_grad_ws(n, n_cams),), float("nan"), dtype=torch.float64, device="cuda"))
        assert torch.equal(gr, gr2) and torch.equal(gt, gt2)
        # pre-filled buffers: absent rows keep their bits (a NaN pattern would not survive a store of x + 0), present rows accumulate
        fr, ft = torch.full((n_cams, 3), 0.5, device="cuda"), torch.full((n_cams, 3), -2.0, device="cuda")
        fr[~present.cuda()] = float("nan"); ft[~present.cuda()] = float("-inf")
        ops.pose_rays_grad(rd, t_ratio, camd, *dev, fr, ft)
        pc = present.cuda()
        assert torch.equal(fr[pc], 0.5 + gr[pc]) and torch.equal(ft[pc], -2.0 + gt[pc])
        assert bool(torch.isnan(fr[~pc]).all()) and bool((ft[~pc] == float("-inf")).all())
        # either gradient alone (g_o is not needed without grad_t)
        only_r, only_t = torch.zeros_like(gr), torch.zeros_like(gt)
        ops.pose_rays_grad(rd, t_ratio, camd, None, *dev[1:], only_r, None)
        ops.pose_rays_grad(rd, t_ratio, camd, *dev, None, only_t)
        assert torch.equal(only_r, gr) and torch.equal(only_t, gt)
        # the rank slices of shard_bounds add up to the whole batch
        for world in (2, 3):
            sr, st = torch.zeros_like(gr), torch.zeros_like(gt)
            for rank in range(world):
                a, b = shard_bounds(n, rank, world)
                if b > a:
                    ops.pose_rays_grad(rd, t_ratio, camd[a:b].contiguous(), *[x[a:b].contiguous() for x in dev], sr, st)
            lim = (world + 1) * bound
            assert bool(((sr.cpu().double() - want_r).abs().amax(1) <= lim).all()) and bool(((st.cpu().double() - want_t).abs().amax(1) <= lim).all())
    print(f"pose_rays_grad n={n} n_cams={n_cams}: worst err / bound = {worst:.3f}")
    if n_cams == 1:
        # one camera, base_x / base_y gradients zero, t_ratio 1: the reduction of ops.pose_grad
        cam, nine = _grad_case(n, 1, "random")
        nine[3].zero_(); nine[4].zero_()
        dev = [x.cuda() for x in nine]
        want_r, want_t, _, bound = _host_grads(r, cam, 1, nine, 1.0)
        gr, gt, pr, pt = (torch.zeros(1, 3, device="cuda") for _ in range(4))
        ops.pose_rays_grad(rd, 1.0, cam.cuda(), *dev, gr, gt)
        ops.pose_grad(rd, 0, dev[0], dev[1], dev[2], dev[5], dev[6], pr, pt)
        for got in (gr, pr):
            assert float((got.cpu().double() - want_r).abs().max()) <= float(bound[0])
        for got in (gt, pt):
            assert float((got.cpu().double() - want_t).abs().max()) <= float(bound[0])
        assert float((gr - pr).abs().max()) <= float(bound[0]) and float((gt - pt).abs().max()) <= float(bound[0])


@gpu
@pytest.mark.parametrize("policy,max_val", [("nan_to_num", 0.5), ("nan_to_num", 0.0), ("zero", 0.5), ("zero", 0.0), ("keep", 0.0)])
def test_sgd_step_against_torch_sgd(policy, max_val):
    from snerf_amd import ops
    n, lr, scale = 1000, 1e-2, 1.0 / 4096
    g = torch.Generator().manual_seed(12)
    p0 = torch.randn(n, generator=g)
    g0 = torch.randn(n, generator=g) * 4096
    g0[::7] *= 50                                                                               # beyond the clip once scaled
    special = [float("nan"), float("inf"), float("-inf"), float("nan"), float("inf")]
    if policy != "keep":
        g0[torch.tensor([3, 250, 251, 777, 999])] = torch.tensor(special)
    # the reference: train_utils.clip_gradients' order (clip_grad_value_, then nan_to_num_) and torch.optim.SGD, on the host
    par = torch.nn.Parameter(p0.clone())
    par.grad = g0 * scale
    if max_val > 0:
        torch.nn.utils.clip_grad_value_([par], max_val)
    if policy == "nan_to_num":
        par.grad.nan_to_num_()
    elif policy == "zero":
        par.grad.nan_to_num_(0.0, 0.0, 0.0)
    clean = par.grad.clone()
    torch.optim.SGD([par], lr=lr).step()
    pd, gd = p0.cuda(), g0.cuda()
    dropped = torch.full((1,), 5, dtype=torch.int64, device="cuda")
    ops.sgd_step(pd, gd, lr, grad_scale=scale, nonfinite=policy, grad_max_val=max_val, dropped=dropped)
    assert float(gd.abs().sum()) == 0 and not bool(torch.isnan(gd).any())                       # gradients come back zeroed
    assert int(dropped) == 5 + (5 if policy != "keep" else 0)
    got = pd.cpu()
    # the same single fp32 multiply and subtract, each rounded on its own: equal bits
    assert torch.equal(got, p0 - clean * torch.tensor(lr, dtype=torch.float32))
    # torch's own step (add_ with alpha: it may fuse the multiply into the add): one ulp of the largest operand
    step = (clean * lr).abs()
    ulp = 2 * EPS * torch.maximum(torch.maximum(p0.abs(), step), got.abs())
    assert bool(((got - par.detach()).abs() <= ulp).all())
    print(f"sgd_step {policy} max_val={max_val}: {int((got != par.detach()).sum())} of {n} differ from torch.optim.SGD (<= 1 ulp)")
    # the global-norm coefficient rides in the same launch
    coef = torch.tensor([0.25], device="cuda")
    p1, g1 = p0.cuda(), torch.ones(n, device="cuda")
    ops.sgd_step(p1, g1, lr, grad_scale=2.0, clip_coef=coef)
    assert torch.equal(p1.cpu(), p0 - torch.full((n,), 0.5) * torch.tensor(lr, dtype=torch.float32))


# ---- GPU: the trainer -----------------------------------------------------------------------------------------------------------------
N_RAYS, N_CAMS, ABSENT, T_RATIO, POSE_LR = 96, 5, 2, 0.25, 1e-2


@pytest.fixture(scope="module")
def scene():
    """the small model's parameters and 96 rays spread over 4 of 5 cameras (row ABSENT owns none), with targets"""
    from test_zip_paths import zip_setup
    specs, p = zip_setup()
    g = torch.Generator().manual_seed(21)
    R = N_RAYS
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    bx = torch.nn.functional.normalize(torch.cross(d, torch.randn(R, 3, generator=g), dim=-1), dim=-1)
    cam = torch.tensor([c for c in range(N_CAMS) if c != ABSENT])[torch.randint(0, N_CAMS - 1, (R,), generator=g)]
    batch = dict(origins=torch.randn(R, 3, generator=g) * 0.1, directions=d, viewdirs=d, radii=2e-3 + 2e-3 * torch.rand(R, 1, generator=g),
                 near=torch.full((R, 1), 0.1), far=torch.full((R, 1), 10.0), base_x=bx,
                 base_y=torch.nn.functional.normalize(torch.cross(d, bx, dim=-1), dim=-1), glo_idx=cam.float()[:, None])
    lm = (torch.rand(R, generator=g) < 0.8).float()
    tg = dict(lossmult=lm, depth=torch.rand(R, generator=g) * 5 + 0.5, depth_mask=lm * (torch.rand(R, generator=g) < 0.6), complete_mask=(1 - lm) * 1.0)
    assert all(float(tg[k].sum()) > 0 for k in tg) and set(cam.tolist()) == set(range(N_CAMS)) - {ABSENT}
    return dict(p=p, batch=batch, target=torch.rand(R, 3, generator=g), targets=tg)


def _setup(scene, pose=False, learn_t=True, **trainer_kw):
    import test_zip_paths
    from snerf_amd.trainer import ZipTrainer
    test_zip_paths.DEV = "cuda"
    m = test_zip_paths.make_model("f32", "f32", scene["p"])
    m.set_deterministic(True)                           # the networks' weight gradients folded in a fixed order: arenas can be compared bit for bit
    if pose:
        trainer_kw.update(pose_net=poses.LearnPoseV2(N_CAMS, True, learn_t, t_ratio=T_RATIO), pose_lr=POSE_LR)
    tr = ZipTrainer(m, lr=1e-2, eps=1.0, nonfinite="nan_to_num", **trainer_kw)
    cu = lambda d: {k: v.cuda() for k, v in d.items()}
    return m, tr, cu(scene["batch"]), scene["target"].cuda(), cu(scene["targets"]), m._draws(N_RAYS, False, m.arena.flat.device, 7)


@gpu
def test_trainer_fused_pose_step_follows_the_glue_route(scene):
    """Three steps of the refinement window, fused (step(pose="train")) against glue: LearnPoseV2 in torch -> apply_pose ->
    step(ray_grads=True) with depth_lambda 0 (train.py:256) -> torch.autograd.backward(moved rays, last_ray_grads) -> nan_to_num_ ->
    torch.optim.SGD.  After step 1 (the table is zero: both routes feed the model the same bits) the arenas are equal bit for bit.
    After three steps r and t agree within 3 lr bound_c, bound_c = n_c 2^-24 sum |products| the fp32 summation bound of the glue
    route's per-camera sums, in float64 from that route's own ray gradients: for r the products g_x[i] x[j] of all nine entries of
    G_c and all four turned tensors (a component of d loss / d r combines the nine sums with coefficients 1 + O(|r|) on two of them
    and O(|r|) on the rest; |r| < 0.1 here, asserted), for t the products t_ratio g_o[i], the largest of the three components.
    The bound is one of summation order only, so it presupposes that both routes feed the model the same rays: apply_pose forms
    R x in the kernel's order.  (With torch's own reduction order, (x * R).sum(-1), 46 of 288 components of the moved directions
    differed in their last bit at step 2; hash-grid gradients jump where a sample crosses a cell face, the ray gradients then
    differed by up to 1.3 % of their largest entry and r by 1e-8 against limits of 0.8 - 2.8e-10.  Measured as it stands: r within
    0.9 - 2.2e-11 of the glue route, t within 3.4e-13, limits 0.8 - 2.8e-10 and 0.5 - 2.4e-11.)"""
    from snerf_amd import zipnerf
    m_f, tr_f, batch, target, tg, draws = _setup(scene, pose=True)
    m_g, tr_g, _, _, _, _ = _setup(scene, loss_cfg=dict(depth_lambda=0.0))
    net_g = poses.LearnPoseV2(N_CAMS, True, True, t_ratio=T_RATIO).cuda()
    opt = torch.optim.SGD(net_g.parameters(), lr=POSE_LR)
    assert torch.equal(m_f.arena.flat, m_g.arena.flat)
    cam = batch["glo_idx"].reshape(-1).long()
    n_c = torch.bincount(cam, minlength=N_CAMS).double().cpu()
    bound_r, bound_t = torch.zeros(N_CAMS, dtype=torch.float64), torch.zeros(N_CAMS, dtype=torch.float64)
    for step in range(3):
        tr_f.step(batch, target, rand=False, draws=draws, targets=tg, pose="train")
        moved = zipnerf.apply_pose(batch, net_g(batch["glo_idx"].reshape(-1).int()))
        tr_g.step(moved, target, rand=False, draws=draws, targets=tg, ray_grads=True)
        rg = tr_g.last_ray_grads
        opt.zero_grad()
        torch.autograd.backward([moved[k] for k in KEYS], rg)
        for p in net_g.parameters():
            p.grad.nan_to_num_()
        opt.step()
        if step == 0:
            assert torch.equal(m_f.arena.flat, m_g.arena.flat)
        prod_r = sum(g.double().abs().sum(-1) * batch[k].double().abs().sum(-1) for g, k in zip(rg[1:], KEYS[1:])).cpu()       # sum_ij |g_i x_j| per ray
        prod_t = T_RATIO * rg[0].double().abs().cpu()
        s_r = torch.zeros(N_CAMS, dtype=torch.float64).index_add_(0, cam.cpu(), prod_r)
        s_t = torch.zeros(N_CAMS, 3, dtype=torch.float64).index_add_(0, cam.cpu(), prod_t).amax(1)
        bound_r, bound_t = torch.maximum(bound_r, n_c * EPS * s_r), torch.maximum(bound_t, n_c * EPS * s_t)
    rf, tf, rgl, tgl = tr_f.pose.net.r.detach().cpu().double(), tr_f.pose.net.t.detach().cpu().double(), net_g.r.detach().cpu().double(), net_g.t.detach().cpu().double()
    lim_r, lim_t = 3 * POSE_LR * bound_r, 3 * POSE_LR * bound_t
    dr, dt = (rf - rgl).abs().amax(1), (tf - tgl).abs().amax(1)
    print(f"fused vs glue after 3 steps: |r| max {float(rf.abs().max()):.3e}, |t| max {float(tf.abs().max()):.3e}")
    for c in range(N_CAMS):
        print(f"  camera {c} ({int(n_c[c])} rays): r differs by {float(dr[c]):.3e} (limit {float(lim_r[c]):.3e}, moved {float(rf[c].abs().max()):.3e}), "
              f"t by {float(dt[c]):.3e} (limit {float(lim_t[c]):.3e}, moved {float(tf[c].abs().max()):.3e})")
    assert float(rf.norm(dim=1).max()) < 0.1
    assert float(rf[ABSENT].abs().max()) == 0 and float(tf[ABSENT].abs().max()) == 0              # exactly zero: no store, SGD of a zero gradient
    assert float(rgl[ABSENT].abs().max()) == 0 and float(tgl[ABSENT].abs().max()) == 0
    visited = [c for c in range(N_CAMS) if c != ABSENT]
    assert bool((rf[visited].abs().amax(1) > 10 * lim_r[visited]).all()) and bool((tf[visited].abs().amax(1) > 10 * lim_t[visited]).all())
    assert bool((dr <= lim_r).all()) and bool((dt <= lim_t).all())
    assert float(tr_f.pose.grad.abs().max()) == 0                                                 # zeroed by the SGD launch
    assert tr_f.last_ray_grads is None


@gpu
def test_trainer_pose_losses_and_modes(scene, monkeypatch):
    from snerf_amd import ops, zipnerf
    from snerf_amd.trainer import LossScaler
    names = ops.ZIP_LOSS_NAMES
    step = lambda tr, b, **kw: tr.step(b, target, rand=False, draws=draws, targets=tg, **kw)
    # a ZipTrainer without pose_net: the reference for "nothing changed"
    m_a, tr_a, batch, target, tg, draws = _setup(scene)
    step(tr_a, batch)
    plain_losses = tr_a.last_losses.cpu()
    assert tr_a.pose is None and tr_a.last_ray_grads is None
    assert float(plain_losses[names.index("depth")]) > 0 and float(plain_losses[names.index("d_complete")]) > 0
    # "train": depth and d_complete vanish
    m_p, tr_p, _, _, _, _ = _setup(scene, pose=True)
    step(tr_p, batch, pose="train", ray_grads=True)
    got = tr_p.last_losses.cpu()
    assert float(got[names.index("depth")]) == 0 and float(got[names.index("d_complete")]) == 0 and float(got[names.index("data")]) > 0
    assert len(tr_p.last_ray_grads) == 5 and all(tuple(g.shape) == (N_RAYS, 3) for g in tr_p.last_ray_grads)
    assert float(tr_p.pose.net.r.detach().abs().max()) > 0 and float(tr_p.pose.net.t.detach().abs().max()) > 0
    # "apply": the table's bits stay, the step is the plain step on moved rays.  Rows with r = 0 and t != 0 move the rays by the same
    # bits in the kernel and in apply_pose (R = I, t * 0.25 exact): the arenas are equal bit for bit
    net = tr_p.pose.net
    with torch.no_grad():
        net.r.zero_()
        net.t.copy_(torch.randn(N_CAMS, 3, generator=torch.Generator().manual_seed(2)) * 0.05)
    tr_p.pose.check_views()
    m_q, tr_q, _, _, _, _ = _setup(scene)
    m_q.arena.flat.copy_(m_p.arena.flat); m_q.arena.bump()
    tr_q.m.copy_(tr_p.m); tr_q.v.copy_(tr_p.v); tr_q.t = tr_p.t
    before = tr_p.pose.flat.clone()
    step(tr_p, batch, pose="apply")
    with torch.no_grad():
        step(tr_q, zipnerf.apply_pose(batch, net(batch["glo_idx"].reshape(-1).int())))
    assert torch.equal(tr_p.pose.flat, before) and float(tr_p.pose.grad.abs().max()) == 0 and tr_p.last_ray_grads is None
    assert torch.equal(m_p.arena.flat, m_q.arena.flat)
    assert float(tr_p.last_losses[names.index("depth")]) > 0                                      # depth supervision is back after the window
    with torch.no_grad():
        net.r.copy_(table(N_CAMS, 3e-2)[0])
    before = tr_p.pose.flat.clone()
    step(tr_p, batch, pose="apply")                                                             # a turned table: still not touched
    assert torch.equal(tr_p.pose.flat, before)
    # cam_idx stands in for an absent glo_idx; a learn_t=False table has no t gradient and leaves t alone
    m_r, tr_r, _, _, _, _ = _setup(scene, pose=True, learn_t=False)
    b2 = {k: v for k, v in batch.items() if k != "glo_idx"}
    b2["cam_idx"] = batch["glo_idx"]
    step(tr_r, b2, pose="train")
    assert tr_r.pose.names == ["r"] and float(tr_r.pose.net.r.detach().abs().max()) > 0 and float(tr_r.pose.net.t.detach().abs().max()) == 0
    assert torch.equal(tr_r.pose.net.r[ABSENT], torch.zeros(3, device="cuda"))
    # the optimiser state round-trips into a real torch.optim.SGD
    sd = tr_p.pose_state_dict()
    opt = torch.optim.SGD(list(tr_p.pose.net.parameters()), lr=0.5)
    opt.load_state_dict(sd)
    assert opt.param_groups[0]["lr"] == POSE_LR
    opt.param_groups[0]["lr"] = 2e-3
    tr_p.load_pose_state_dict(opt.state_dict())
    assert tr_p.pose.lr == 2e-3
    # a dynamic loss scale whose step overflows (a NaN target poisons that step's gradients) skips the table's update too and zeroes
    # its gradient
    m_s, tr_s, _, _, _, _ = _setup(scene, pose=True, loss_scale=LossScaler(init_scale=1024.0))
    arena0 = m_s.arena.flat.clone()
    poisoned = target.clone()
    poisoned[0, 0] = float("nan")
    tr_s.step(batch, poisoned, rand=False, draws=draws, targets=tg, pose="train")
    assert tr_s.scaler.skipped_steps == 1 and tr_s.scaler.scale == 512.0 and tr_s.t == 0 and torch.equal(m_s.arena.flat, arena0)
    assert float(tr_s.pose.flat.abs().max()) == 0 and float(tr_s.pose.grad.abs().max()) == 0 and not bool(torch.isnan(tr_s.pose.grad).any())
    # refused before any launch
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    with pytest.raises(ValueError, match="pose_net"):
        step(tr_a, batch, pose="train")
    with pytest.raises(ValueError, match="pose_net"):
        step(tr_a, batch, pose="apply")
    with pytest.raises(ValueError, match="neither"):
        step(tr_p, {k: v for k, v in batch.items() if k != "glo_idx"}, pose="train")
    with pytest.raises(ValueError, match="'train' or 'apply'"):
        step(tr_p, batch, pose="refine")
    with pytest.raises(ValueError, match="one table row per ray"):
        step(tr_p, dict(batch, glo_idx=batch["glo_idx"][:-1]), pose="apply")
    assert calls == []
    monkeypatch.setattr(_lib, "call", real)
    # a ZipTrainer without pose_net, built after the pose trainers have run: the same bits as the first one
    m_b, tr_b, _, _, _, _ = _setup(scene)
    step(tr_b, batch)
    assert torch.equal(m_b.arena.flat, m_a.arena.flat)
    step(tr_a, batch, ray_grads=True)                                                             # ray_grads without a pose_net
    step(tr_b, batch)
    assert len(tr_a.last_ray_grads) == 5 and torch.equal(m_b.arena.flat, m_a.arena.flat)
