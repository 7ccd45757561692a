"""Learned depth confidence on the device: confidence.Confidence / ConfidenceMaps, the kernels snerf_conf_apply / snerf_conf_grad, the
g_conf route of the masked loss tail (snerf_mip_loss_tail_gconf), and the learned table inside MipTrainer.step and the captured step.

The yardstick is the reference's own text, restated once below in torch and evaluated in float64: the precomputed branch of
calc_final_confidence (s-nerf/model/confidence.py:193-206), DepthLoss (model/loss_factory.py:26-37, disparity form) times that
confidence, and the masked mean of calc_depth_loss (confidence.py:209-224) times depth_lambda (train.py).  The per-ray term is
computed on the masked subset, as the reference does: 1 / 0 under a mask would give NaN gradients."""
import os
import types

import numpy as np
import pytest
import torch

from snerf_amd import _lib, confidence

gpu = pytest.mark.gpu
EPS = 2.0 ** -24                                        # half an ulp of 1 in fp32: the relative error of one rounding
EPS64 = 2.0 ** -53
H, W, N_IMG = 13, 17, 5
I_TRAIN = (3, 0, 4, 2)                                  # positions 0..3: image 1 has no maps, and no image sits at its own position
MODES = ["rgb", "ssim", "depth", "vgg"]
# depth_lambda and coarse_depth_mult (arg_parser defaults 0.2 / 0.2) as the fp32 values the kernels receive
LAM_D = CM = float(torch.tensor(0.2, dtype=torch.float32))


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def ref_final_confidence(lambdas, modes, all_conf_maps, i_train, img_i, sel_coords, skymask=None):
    """confidence.py:193-206, float64: lambdas [M, n_images] (differentiable), all_conf_maps = the list precompute_conf_map returns
    -> the confidence of every ray of the batch, [n]"""
    conf_maps = all_conf_maps[np.where(np.asarray(i_train) == img_i)[0].item()]                # :193
    final_conf_map = torch.zeros((H, W), dtype=torch.float64)                                  # :195
    weights = torch.sigmoid(lambdas[:, img_i].to(torch.float64))                               # :196
    for idx, mode in enumerate(modes):                                                         # :197-198
        final_conf_map = final_conf_map + weights[idx] * conf_maps[mode].to(torch.float64).reshape(H, W)
    final_conf_map = final_conf_map / weights.sum()                                            # :199
    if skymask is not None:                                                                    # :202-203
        final_conf_map = torch.where(skymask[img_i], torch.ones((), dtype=torch.float64), final_conf_map)
    return final_conf_map[sel_coords[:, 0], sel_coords[:, 1]]                                  # :205


def ref_depth_loss(d1, d0, td, conf, keep=None, lam=LAM_D, cm=CM):
    """calc_depth_loss (confidence.py:209-224) with DepthLoss in its disparity form (loss_factory.py:26-37), float64, times depth_lambda:
    the per-ray term on the rays with a target only, times their confidence, the back-camera style mask `keep` (bool [n], :222-223),
    the mean"""
    f = lambda x: x.to(torch.float64)
    target_mask = td != 0                                                                      # :211
    fn = lambda x, y: torch.abs(1 / x - 1 / y)                                                 # loss_factory.py:31
    depth_loss = fn(f(d1)[target_mask], f(td)[target_mask]) + cm * fn(f(d0)[target_mask], f(td)[target_mask])     # :36
    depth_loss = depth_loss * f(conf)[target_mask]                                             # :219-220
    if keep is not None:
        depth_loss = depth_loss[keep[target_mask]]                                             # :223
    return depth_loss.mean() * lam if depth_loss.numel() else torch.zeros((), dtype=torch.float64)


# ---- the scene of every test: maps as precompute_conf_map returns them ----------------------------------------------------------------
def _scene(M, seed=0):
    """-> (modes, all_conf_maps [list per i_train position of {mode: [H*W]}], skymask bool [N_IMG,H,W], lambdas fp32 [M,N_IMG])"""
    g = torch.Generator().manual_seed(40 + 7 * M + seed)
    modes = MODES[:M]
    all_maps = [{m: torch.rand(H * W, generator=g) for m in modes} for _ in I_TRAIN]
    sky = torch.rand(N_IMG, H, W, generator=g) < 0.3
    lambdas = (torch.rand(M, N_IMG, generator=g) * 4 - 2)
    return modes, all_maps, sky, lambdas


def _coords(n, seed=0):
    g = torch.Generator().manual_seed(500 + n + seed)
    return torch.stack([torch.randint(0, H, (n,), generator=g), torch.randint(0, W, (n,), generator=g)], -1)


def _device_maps(all_maps, sky, with_sky):
    return confidence.ConfidenceMaps(all_maps, I_TRAIN, N_IMG, H, W, skymask=sky if with_sky else None, device="cuda")


# ---- without a GPU ------------------------------------------------------------------------------------------------------------------
def test_confidence_state_dict_and_reference_checkpoint():
    c = confidence.Confidence(["rgb", "ssim", "depth"], 5)
    assert list(c.state_dict()) == ["lambdas"] and [n for n, _ in c.named_parameters()] == ["lambdas"]
    assert tuple(c.lambdas.shape) == (3, 5) and c.lambdas.dtype == torch.float32 and float(c.lambdas.detach().abs().max()) == 0 and c.lambdas.requires_grad
    assert c.tau == 0.2 and c.modes == ["rgb", "ssim", "depth"]
    # the `confidence` entry of a reference checkpoint written with vgg_loss = True carries the frozen VGG network
    saved = {"lambdas": torch.randn(3, 5), "vgg_loss.vgg.slice1.0.weight": torch.randn(4, 3, 3, 3), "vgg_loss.vgg.slice1.0.bias": torch.randn(4)}
    c.load_state_dict(saved)
    assert torch.equal(c.state_dict()["lambdas"], saved["lambdas"]) and list(c.state_dict()) == ["lambdas"]
    with pytest.raises(RuntimeError):                                                           # anything else unknown is still refused
        c.load_state_dict({"lambdas": torch.zeros(3, 5), "other": torch.zeros(1)})
    # build_confidence_model: the mode list of confidence.py:171-185 and the table's own Adam
    for kw, want in ((dict(no_reproj=False, no_geometry=False, vgg_loss=False), ["rgb", "ssim", "depth"]),
                     (dict(no_reproj=True, no_geometry=False, vgg_loss=True), ["depth", "vgg"]),
                     (dict(no_reproj=False, no_geometry=True, vgg_loss=False), ["rgb", "ssim"])):
        net, opt = confidence.build_confidence_model(types.SimpleNamespace(tau=0.3, **kw), 7, "cpu")
        assert net.modes == want and tuple(net.lambdas.shape) == (len(want), 7) and net.tau == 0.3
        assert isinstance(opt, torch.optim.Adam) and opt.param_groups[0]["lr"] == 1e-3 and opt.param_groups[0]["params"][0] is net.lambdas
    with pytest.raises(ValueError, match="modes"):
        confidence.Confidence([], 5)


@pytest.mark.parametrize("M", [1, 3, 4])
def test_gradient_chain_host_model_against_float64_autograd(M):
    modes, all_maps, sky, lambdas = _scene(M)
    n = 96
    sel = _coords(n)
    g = torch.randn(n, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    for img in I_TRAIN:
        for skymask in (None, sky):
            lam = lambdas.double().clone().requires_grad_(True)
            (ref_final_confidence(lam, modes, all_maps, I_TRAIN, img, sel, skymask) * g).sum().backward()
            at = torch.stack([all_maps[I_TRAIN.index(img)][m].reshape(H, W)[sel[:, 0], sel[:, 1]] for m in modes])
            A = confidence.conf_sums(at, None if skymask is None else skymask[img][sel[:, 0], sel[:, 1]], g)
            got = confidence.conf_grad_chain(lambdas[:, img], A)
            scale = float((at.double().abs() * g.abs()).sum(-1).max())
            assert float((got - lam.grad[:, img]).abs().max()) <= 1e-13 * scale, (got, lam.grad[:, img])
            other = [i for i in range(N_IMG) if i != img]
            assert float(lam.grad[:, other].abs().max()) == 0
            if M > 1:
                assert float(got.abs().max()) > 1e-3 * scale / n                                 # the case has a gradient to get wrong
            else:
                assert float(got.abs().max()) <= 1e-13 * scale                                  # one mode: conf is the map, whatever lambda


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")


_P = lambda k: 1 << 20 | k << 12                       # distinct fake device addresses, 4096 bytes apart: never dereferenced


def _apply_args(**kw):
    a = dict(maps=_P(1), M=3, P=4, H=H, W=W, slot_of_image=_P(2), lambdas=_P(3), n_images=5, sky=_P(4), img_dev=None, img_host=1, coords=_P(5),
             n=16, conf=_P(6), stream=None)
    a.update(kw)
    return a


def _grad_args(**kw):
    a = dict(maps=_P(1), M=3, P=4, H=H, W=W, slot_of_image=_P(2), lambdas=_P(3), n_images=5, sky=_P(4), img_dev=None, img_host=1, coords=_P(5),
             g_conf=_P(6), n=1000, ws=_P(7), ws_doubles=32, grad_lambdas=_P(8), stream=None)
    a.update(kw)
    return a


def _gconf_tail_args(**kw):
    a = dict(rgb=_P(1), tgt=_P(2), dist1=_P(3), dist0=_P(4), tdepth=_P(5), conf=_P(6), s_f=_P(7), w_f=_P(8), s_c=_P(9), w_c=_P(10), sem=_P(11),
             labels=_P(12), labels_f32=0, C=7, rows=_P(13), img_i=_P(14), rgb_row_limit=_P(15), depth_row_limit=_P(16), sem_valid=_P(17),
             n_images=3, depth_keep=_P(18), N=24, Pf=17, Sc=16, disparity=1, depth_lambda=0.2, coarse_mult=0.2, prop_lambda=0.05,
             semantic_lambda=0.1, out=_P(19), g_rgb=_P(20), g_dist1=_P(21), g_dist0=_P(22), g_wc=_P(23), g_sem=_P(24), g_conf=_P(25), stream=None)
    a.update(kw)
    return a


def test_confidence_entries_reject_bad_arguments_without_a_gpu():
    """argument validation happens before any launch (the pointers here are never dereferenced)"""
    _lib_or_skip()
    protos = _lib.parse_header()
    assert [n for _, n in protos["snerf_conf_apply"]] == list(_apply_args())
    assert [n for _, n in protos["snerf_conf_grad"]] == list(_grad_args())
    assert [n for _, n in protos["snerf_mip_loss_tail_gconf"]] == list(_gconf_tail_args())
    assert [n for _, n in protos["snerf_mip_loss_tail_gconf"]][:-2] == [n for _, n in protos["snerf_mip_loss_tail_masked"]][:-1]
    common = [dict(maps=None), dict(slot_of_image=None), dict(lambdas=None), dict(coords=None), dict(M=0), dict(M=9), dict(M=-1), dict(n=-1),
              dict(img_host=5), dict(img_host=-1), dict(P=0), dict(H=0), dict(W=0), dict(n_images=0)]
    for kw in common + [dict(conf=None)]:
        with pytest.raises(_lib.SnerfHipError, match="bad argument"):
            _lib.call("snerf_conf_apply", *_apply_args(**kw).values())
    assert [_lib.query("snerf_conf_grad_ws", n) for n in (0, -3, 1, 256, 257, 1000, 5000, 1 << 30)] == [0, 0, 8, 8, 16, 32, 160, 8 * 256]
    for kw in common + [dict(g_conf=None), dict(grad_lambdas=None), dict(ws=None), dict(ws_doubles=31), dict(ws_doubles=0)]:
        with pytest.raises(_lib.SnerfHipError, match="bad argument"):
            _lib.call("snerf_conf_grad", *_grad_args(**kw).values())
    for kw in (dict(tdepth=None, depth_keep=None), dict(rgb=None), dict(g_dist1=None), dict(C=33), dict(rows=None), dict(g_sem=None)):
        with pytest.raises(_lib.SnerfHipError, match="bad argument"):
            _lib.call("snerf_mip_loss_tail_gconf", *_gconf_tail_args(**kw).values())
    # an empty batch is a no-op, whatever the rest
    none = lambda a: [None if isinstance(v, int) and v >= (1 << 20) else v for v in a.values()]
    assert _lib.call("snerf_conf_apply", *none(_apply_args(n=0))) is None
    assert _lib.call("snerf_conf_grad", *none(_grad_args(n=0, ws_doubles=0))) is None
    assert _lib.call("snerf_mip_loss_tail_gconf", *none(_gconf_tail_args(N=0))) is None


def test_confidence_maps_argument_errors():
    modes, all_maps, sky, _ = _scene(3)
    m = confidence.ConfidenceMaps(all_maps, I_TRAIN, N_IMG, H, W, skymask=sky)
    assert tuple(m.maps.shape) == (3, 4, H, W) and m.maps.dtype == torch.float32 and m.modes == modes
    assert m.slot_of_image.tolist() == [1, -1, 3, 0, 2] and m.slot_of_image.dtype == torch.int32
    assert m.sky.dtype == torch.uint8 and torch.equal(m.sky.bool(), sky)
    for p, img in enumerate(I_TRAIN):
        for k, mode in enumerate(modes):
            assert torch.equal(m.maps[k, m.slot_of_image[img]], all_maps[p][mode].reshape(H, W))
    assert confidence.ConfidenceMaps(all_maps, np.asarray(I_TRAIN), N_IMG, H, W).sky is None
    broken = [dict(d) for d in all_maps]
    del broken[2]["ssim"]
    with pytest.raises(ValueError, match="'ssim' map"):
        confidence.ConfidenceMaps(broken, I_TRAIN, N_IMG, H, W)
    with pytest.raises(ValueError, match="per i_train position"):
        confidence.ConfidenceMaps(all_maps[:3], I_TRAIN, N_IMG, H, W)
    with pytest.raises(ValueError, match="i_train"):
        confidence.ConfidenceMaps(all_maps, (0, 1, 2, 5), N_IMG, H, W)
    with pytest.raises(ValueError, match="H \\* W"):
        confidence.ConfidenceMaps(all_maps, I_TRAIN, N_IMG, H, W + 1)
    with pytest.raises(ValueError, match="skymask"):
        confidence.ConfidenceMaps(all_maps, I_TRAIN, N_IMG, H, W, skymask=sky[:4])
    # against the model: a missing mode and a table of another width are refused; another order is followed
    with pytest.raises(ValueError, match="no mode"):
        m.for_model(confidence.Confidence(["rgb", "ssim", "depth", "vgg"], N_IMG))
    with pytest.raises(ValueError, match="columns"):
        m.for_model(confidence.Confidence(modes, N_IMG + 1))
    m2 = confidence.ConfidenceMaps(all_maps, I_TRAIN, N_IMG, H, W).for_model(confidence.Confidence(["depth", "rgb"], N_IMG))
    assert m2.modes == ["depth", "rgb"] and torch.equal(m2.maps[0], m.maps[2]) and torch.equal(m2.maps[1], m.maps[0])


def test_trainer_argument_errors_with_a_confidence_table():
    from cpu_ops_emulation import emulate_ops
    from oracle import common
    from snerf_amd import mipnerf
    from snerf_amd.trainer import MipTrainer
    modes, all_maps, sky, _ = _scene(3)
    with emulate_ops():
        model = mipnerf.MipNerfModel(n_samples=8, N_fine=9, no_warp_sample=0, ray_shape="cone", fn=1, radius=3., transform_idx=0, real=True,
                                     rgb_layer=3, hidden_layer=64, density_noise=0., max_deg_point=16, proposal_hidden_layer=64,
                                     proposal_loss=True, compute="f32", device="cpu")
        maps = lambda: confidence.ConfidenceMaps(all_maps, I_TRAIN, N_IMG, H, W, skymask=sky)
        with pytest.raises(ValueError, match="go together"):
            MipTrainer(model, conf_net=confidence.Confidence(modes, N_IMG))
        with pytest.raises(ValueError, match="go together"):
            MipTrainer(model, conf_maps=maps())
        with pytest.raises(ValueError, match="no mode"):
            MipTrainer(model, conf_net=confidence.Confidence(MODES, N_IMG), conf_maps=maps())
        frozen = confidence.Confidence(modes, N_IMG)
        frozen.lambdas.requires_grad_(False)
        with pytest.raises(ValueError, match="trained fp32"):
            MipTrainer(model, conf_net=frozen, conf_maps=maps())
        net = confidence.Confidence(modes, N_IMG)
        tr = MipTrainer(model, conf_net=net, conf_maps=maps(), conf_lr=2e-3)
        assert tr.conf.lr == 2e-3 and tr.conf.flat.data_ptr() == net.lambdas.data_ptr() and tuple(tr.conf.g.shape) == (3, N_IMG)
        n = 16
        rays = mipnerf.Rays(**common.synthetic_rays(n, seed=2))
        tgt, td, sel = torch.rand(n, 3), torch.rand(n) + 2, _coords(n)
        with pytest.raises(ValueError, match="conf= cannot be given"):
            tr.step(rays, tgt, td, torch.rand(n), sel_coords=sel, img_i=0)
        for kw in (dict(target_depth=None, sel_coords=sel, img_i=0), dict(target_depth=td, sel_coords=None, img_i=0),
                   dict(target_depth=td, sel_coords=sel, img_i=None)):
            with pytest.raises(ValueError, match="needs target_depth=, sel_coords= and img_i="):
                tr.step(rays, tgt, **kw)
        with pytest.raises(ValueError, match="batcher"):                 # the table is captured with a batcher only
            tr.capture(rays, tgt, td, img_i=torch.zeros(1, dtype=torch.int64))
        assert tr._step_dev is None and tr.conf.step_dev is None         # a refused capture arms nothing: later eager steps count on the host
        # the optimiser state has torch.optim.Adam's layout before the first step as well
        sd = tr.conf_state_dict()
        assert sd["param_groups"][0]["lr"] == 2e-3 and sd["param_groups"][0]["params"] == [0] and float(sd["state"][0]["step"]) == 0
        opt = torch.optim.Adam([{"params": [confidence.Confidence(modes, N_IMG).lambdas], "lr": 1.0}])
        opt.load_state_dict(sd)
        assert opt.param_groups[0]["lr"] == 2e-3
        # a refused optimiser state writes nothing: the table holds the moments of an accepted load, then refuses a wrong shape ...
        from snerf_amd import poses
        g = torch.Generator().manual_seed(4)
        sd["state"][0] = {"step": torch.tensor(5.), "exp_avg": torch.randn(3, N_IMG, generator=g), "exp_avg_sq": torch.rand(3, N_IMG, generator=g)}
        tr.load_conf_state_dict(sd)
        assert tr.conf.t == 5 and torch.equal(tr.conf.m.view(3, N_IMG), sd["state"][0]["exp_avg"])
        assert torch.equal(tr.conf.v.view(3, N_IMG), sd["state"][0]["exp_avg_sq"])
        bad = tr.conf_state_dict()
        bad["state"][0]["exp_avg"] = torch.zeros(N_IMG, 3)
        bad["state"][0]["step"] = torch.tensor(9.)
        with pytest.raises(ValueError):
            tr.load_conf_state_dict(bad)
        assert tr.conf.t == 5 and torch.equal(tr.conf.m.view(3, N_IMG), sd["state"][0]["exp_avg"])
        assert torch.equal(tr.conf.v.view(3, N_IMG), sd["state"][0]["exp_avg_sq"])
        # ... and the pose table (two entries) one whose entries disagree on the step count
        tp = MipTrainer(model, pose_net=poses.LearnPose(N_IMG, True, True))
        ok = tp.pose_state_dict()
        for i in (0, 1):
            ok["state"][i] = {"step": torch.tensor(3.), "exp_avg": torch.randn(N_IMG, 3, generator=g), "exp_avg_sq": torch.rand(N_IMG, 3, generator=g)}
        tp.load_pose_state_dict(ok)
        kept = (tp.pose.m.clone(), tp.pose.v.clone())
        assert tp.pose.t == 3 and torch.equal(kept[0][3 * N_IMG:].view(N_IMG, 3), ok["state"][1]["exp_avg"]) and bool(kept[1].any())
        split = tp.pose_state_dict()
        split["state"][0]["exp_avg"] = torch.ones(N_IMG, 3)
        split["state"][1]["step"] = torch.tensor(4.)
        with pytest.raises(ValueError):
            tp.load_pose_state_dict(split)
        assert tp.pose.t == 3 and torch.equal(tp.pose.m, kept[0]) and torch.equal(tp.pose.v, kept[1])
        # a module whose parameter was reallocated after the trainer took it is refused, not trained past
        net.double()
        with pytest.raises(RuntimeError, match="no longer lives"):
            tr.step(rays, tgt, td, sel_coords=sel, img_i=0)


# ---- GPU: snerf_conf_apply ----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("with_sky", [False, True])
@pytest.mark.parametrize("n", [1, 63, 65, 1000])
def test_conf_apply(n, with_sky):
    """Bound, relative to conf (every term is non-negative, so relative errors do not grow): with u = 2^-24, the kernel rounds each
    sigmoid once (u), each product w_k map_k once (u) and each of the M - 1 additions of the numerator once, so the numerator is
    within (1 + u)^(M+1) - 1; the denominator's terms carry their sigmoid's rounding and M - 1 additions, (1 + u)^M - 1; the division is
    rounded once.  Together (1 + u)^(2M+2) - 1 = (2M + 2) u + O(u^2); one more u covers the second-order terms and the float64
    evaluations (the kernel's own double sigmoid and the yardstick): (2M + 3) u."""
    from snerf_amd import ops
    sel = _coords(n)
    sel_d = sel.cuda()
    for M in (1, 3, 4):
        modes, all_maps, sky, lambdas = _scene(M)
        dm = _device_maps(all_maps, sky, with_sky)
        lam_d = lambdas.cuda()
        for img in I_TRAIN:
            want = ref_final_confidence(lambdas, modes, all_maps, I_TRAIN, img, sel, sky if with_sky else None)
            got = ops.conf_apply(dm.maps, dm.slot_of_image, lam_d, dm.sky, img, sel_d)
            assert got.dtype == torch.float32 and tuple(got.shape) == (n,)
            err = (got.cpu().double() - want).abs()
            bound = (2 * M + 3) * EPS * want
            print(f"conf_apply n={n} M={M} img={img} sky={with_sky}: max err / bound = {float((err / bound).max()):.3f}")
            assert bool((err <= bound).all())
            if with_sky:
                on_sky = sky[img][sel[:, 0], sel[:, 1]]
                assert bool((got.cpu()[on_sky] == 1.0).all())
                if n >= 63:
                    assert 0 < int(on_sky.sum()) < n
            # the device index gives the same bits
            assert torch.equal(ops.conf_apply(dm.maps, dm.slot_of_image, lam_d, dm.sky, torch.tensor([img], dtype=torch.int64, device="cuda"), sel_d), got)
        # an image without maps, and a device index outside the table: all ones
        for img in (1, torch.tensor([1], dtype=torch.int64, device="cuda"), torch.tensor([N_IMG], dtype=torch.int64, device="cuda"),
                    torch.tensor([-1], dtype=torch.int64, device="cuda")):
            assert bool((ops.conf_apply(dm.maps, dm.slot_of_image, lam_d, dm.sky, img, sel_d) == 1.0).all())
        # lambdas = 0 (where training starts): the plain mean of the maps
        got = ops.conf_apply(dm.maps, dm.slot_of_image, torch.zeros_like(lam_d), None, 3, sel_d).cpu().double()
        mean = torch.stack([all_maps[0][m].reshape(H, W)[sel[:, 0], sel[:, 1]] for m in modes]).double().mean(0)
        assert bool(((got - mean).abs() <= (2 * M + 3) * EPS * mean).all())


# ---- GPU: snerf_conf_grad -----------------------------------------------------------------------------------------------------------
def _grad_bound(want, g, at, n):
    """per entry of the column: one fp32 rounding of the result, u |want_k|, plus the double sums.  A_k is a sum of n exact products
    (24-bit x 24-bit in a 53-bit format) and is within (n - 1) 2^-53 sum_r |g_r map_kr| of the true sum; d lambda_k =
    c_k (A_k - sum_j p_j A_j) with c_k = s_k (1 - s_k) / S <= 1 and sum_j p_j = 1, so the errors of the A reach the result at most
    twice, and the dozen double operations of the chain stay below 16 more units of the same size.  The float64 autograd of the
    restatement sums the same n terms in its own order with the same bound: twice that.
    -> [M] = u |want| + 4 (n + 16) 2^-53 max_k sum_r |g_r| map_kr"""
    return EPS * want.abs() + 4 * (n + 16) * EPS64 * float((at.double() * g.double().abs()).sum(-1).max())


@gpu
@pytest.mark.parametrize("with_sky", [False, True])
@pytest.mark.parametrize("n", [1, 63, 65, 1000, 5000])
def test_conf_grad(n, with_sky):
    """n = 5000: 20 workgroups of the partial pass (1000: 4)"""
    from snerf_amd import ops
    from snerf_amd.trainer import shard_bounds
    sel = _coords(n)
    sel_d = sel.cuda()
    g = torch.randn(n, generator=torch.Generator().manual_seed(77 + n))
    g_d = g.cuda()
    for M in (1, 3, 4):
        modes, all_maps, sky, lambdas = _scene(M)
        dm = _device_maps(all_maps, sky, with_sky)
        lam_d = lambdas.cuda()
        run = lambda img, buf, a=0, b=n: ops.conf_grad(dm.maps, dm.slot_of_image, lam_d, dm.sky, img, sel_d[a:b].contiguous(), g_d[a:b].contiguous(), buf)
        for img in (3, 2):
            lam = lambdas.double().clone().requires_grad_(True)
            (ref_final_confidence(lam, modes, all_maps, I_TRAIN, img, sel, sky if with_sky else None) * g.double()).sum().backward()
            want = lam.grad[:, img]
            at = torch.stack([all_maps[I_TRAIN.index(img)][m].reshape(H, W)[sel[:, 0], sel[:, 1]] for m in modes])
            bound = _grad_bound(want, g, at, n)
            buf = torch.zeros(M, N_IMG, device="cuda")
            run(img, buf)
            err = (buf[:, img].cpu().double() - want).abs()
            print(f"conf_grad n={n} M={M} img={img} sky={with_sky}: max err / bound = {float((err / bound).max()):.3f}, max |want| = {float(want.abs().max()):.3e}")
            assert bool((err <= bound).all())
            if M > 1 and n > 1:
                assert float(want.abs().max()) > 100 * float(bound.max())                       # the bound is far below the gradient
            other = [i for i in range(N_IMG) if i != img]
            assert float(buf[:, other].abs().max()) == 0                                        # only column img
            # run-to-run reproducible; the device index gives the same bits
            again = torch.zeros_like(buf)
            run(torch.tensor([img], dtype=torch.int64, device="cuda"), again)
            assert torch.equal(buf, again)
            # accumulates into column img of a pre-filled buffer, the other columns keep their bits
            filled = torch.full((M, N_IMG), 0.5, device="cuda")
            run(img, filled)
            assert torch.equal(filled[:, img], 0.5 + buf[:, img]) and bool((filled[:, other] == 0.5).all())
            # two half-batches add up to the whole: the true values do, and each of the three results is within its own bound of its
            # true value -- a half's rounding is relative to the half, which may be larger than the whole (the halves can cancel),
            # and its double-sum term is at most the whole batch's
            halves, tol = torch.zeros(M, dtype=torch.float64), bound.clone()
            if n > 1:
                for rank in range(2):
                    a, b = shard_bounds(n, rank, 2)
                    part = torch.zeros(M, N_IMG, device="cuda")
                    run(img, part, a, b)
                    halves += part[:, img].cpu().double()
                    tol += EPS * part[:, img].cpu().double().abs() * (1 + 2 * EPS) + (bound - EPS * want.abs())
                assert bool(((halves - buf[:, img].cpu().double()).abs() <= tol).all())
        # an image without maps (slot -1) and an index outside the table leave the buffer untouched
        filled = torch.full((M, N_IMG), 0.5, device="cuda")
        for img in (1, torch.tensor([N_IMG], dtype=torch.int64, device="cuda"), torch.tensor([-1], dtype=torch.int64, device="cuda")):
            run(img, filled)
        assert bool((filled == 0.5).all())
        # so does a batch that is all sky
        all_sky = confidence.ConfidenceMaps(all_maps, I_TRAIN, N_IMG, H, W, skymask=torch.ones(N_IMG, H, W, dtype=torch.bool), device="cuda")
        ops.conf_grad(all_sky.maps, all_sky.slot_of_image, lam_d, all_sky.sky, 3, sel_d, g_d, filled)
        assert bool((filled == 0.5).all())


@gpu
def test_calc_final_confidence_under_autograd():
    """the two kernels as one differentiable function: forward = conf_apply, backward = conf_grad into lambdas.grad"""
    from snerf_amd import ops
    n, M = 65, 3
    modes, all_maps, sky, lambdas = _scene(M)
    dm = _device_maps(all_maps, sky, True)
    net = confidence.Confidence(modes, N_IMG).cuda()
    net.load_state_dict({"lambdas": lambdas})
    sel, g = _coords(n), torch.randn(n, generator=torch.Generator().manual_seed(4))
    conf = confidence.calc_final_confidence(net, dm, sel.cuda(), 4)
    assert torch.equal(conf, ops.conf_apply(dm.maps, dm.slot_of_image, net.lambdas.data, dm.sky, 4, sel.cuda())) and conf.requires_grad
    (conf * g.cuda()).sum().backward()
    buf = torch.zeros(M, N_IMG, device="cuda")
    ops.conf_grad(dm.maps, dm.slot_of_image, net.lambdas.data, dm.sky, 4, sel.cuda(), g.cuda(), buf)
    assert torch.equal(net.lambdas.grad, buf) and float(buf[:, 4].abs().max()) > 0


# ---- GPU: the g_conf route of the masked tail ---------------------------------------------------------------------------------------
LAM_P, LAM_S, H_RULE = 0.05, 0.1, 8
RGB_LIM, DEP_LIM, SEM_VALID = [H_RULE, 5, 0], [H_RULE, 4, 0], [1, 1, 1]


def _tail_inputs(N, C=7, Sc=16, Pf=17, seed=0):
    g = torch.Generator().manual_seed(3000 + N + seed)
    r = lambda *s: torch.rand(*s, generator=g)

    def fence(P):
        s = torch.sort(r(N, P), dim=-1).values
        s[:, 0], s[:, -1] = 0.0, 1.0
        return s
    w_c, w_f = r(N, Sc) ** 2, r(N, Pf - 1) ** 3
    td = r(N) * 20 + 2
    td[r(N) < 0.3] = 0
    labels = torch.randint(0, C, (N,), generator=g).to(torch.int32)
    labels[r(N) < 0.2] = -100
    rows = torch.randint(0, H_RULE, (N,), generator=g)
    return dict(rgb=r(N, 3), tgt=r(N, 3), d1=r(N) * 30 + 1, d0=r(N) * 30 + 1, td=td, conf=r(N), keep=(r(N) < 0.3).float(),
                s_f=fence(Pf), w_f=w_f / w_f.sum(-1, keepdim=True), s_c=fence(Sc + 1), w_c=w_c / w_c.sum(-1, keepdim=True) * r(N, 1),
                sem=(r(N, C) * 2 - 1) * 10, labels=labels, sel=torch.stack([rows, torch.randint(0, 11, (N,), generator=g)], -1))


@gpu
@pytest.mark.parametrize("case", ["plain", "keep", "rules", "all"])
@pytest.mark.parametrize("N", [1, 64, 65, 130])
def test_g_conf_tail(N, case):
    """g_conf against the float64 derivative of the restatement, and every other output against snerf_mip_loss_tail_masked.
    Bound of g_conf_r = (|e1| + cm |e0|) (lam / #depth), e = 1/d - 1/t, with u = 2^-24: the two reciprocals of an e are rounded (u each,
    relative to themselves) and so is their difference, so |e| is within u (1/d + 1/t) (1 + u) + u |e| of the true value -- the
    difference may cancel, hence the absolute term; then cm |e0|, the sum, lam / #depth and the final product are rounded once each
    (4 u relative), the whole within k u ((1/d1 + 1/t) + cm (1/d0 + 1/t)) + 5 u |g_conf_r| with k = lam / #depth, and one more
    u |g_conf_r| for the second-order terms."""
    from snerf_amd import ops
    c = _tail_inputs(N)
    d = {k: v.cuda().contiguous() for k, v in c.items()}
    keep = case in ("keep", "all")
    for img in ((0, 1, 2) if case in ("rules", "all") else (None,)):
        kw = dict(depth_keep=d["keep"] if keep else None)
        if case == "all":
            kw.update(sem=d["sem"], labels=d["labels"], semantic_lambda=LAM_S)
        if img is not None:
            tables = [torch.tensor(v, dtype=torch.int32, device="cuda") for v in (RGB_LIM, DEP_LIM, SEM_VALID)]
            kw.update(rows=d["sel"], img_i=torch.tensor([img], dtype=torch.int64, device="cuda"), rgb_row_limit=tables[0],
                      depth_row_limit=tables[1], sem_valid=tables[2])
        run = lambda **more: ops.mip_loss_tail_masked(d["rgb"], d["tgt"], d["d1"], d["d0"], d["td"], d["conf"], d["s_f"], d["w_f"], d["s_c"], d["w_c"],
                                                      True, LAM_D, CM, LAM_P, **kw, **more)
        old, new = run(), run(want_g_conf=True)
        assert len(old) == 6 and len(new) == 7
        # ---- g_conf
        mask = torch.ones(N, dtype=torch.bool)
        if img is not None:
            mask &= c["sel"][:, 0] < DEP_LIM[img]
        if keep:
            mask &= c["keep"] == 0
        conf = c["conf"].double().clone().requires_grad_(True)
        loss = ref_depth_loss(c["d1"], c["d0"], c["td"], conf, mask)
        want = torch.autograd.grad(loss, conf)[0] if loss.requires_grad else torch.zeros(N, dtype=torch.float64)
        counted = mask & (c["td"] != 0)
        n_dep = int(counted.sum())
        assert float(new[0][0]) == n_dep
        got = new[6].cpu()
        assert bool((got[~counted] == 0).all()) and bool((want[~counted] == 0).all())           # written in full, 0 outside the mean
        if n_dep:
            t, d1, d0 = (c[k].double()[counted] for k in ("td", "d1", "d0"))
            bound = (LAM_D / n_dep) * EPS * ((1 / d1 + 1 / t) + CM * (1 / d0 + 1 / t)) + 6 * EPS * want[counted].abs()
            err = (got.double()[counted] - want[counted]).abs()
            print(f"g_conf N={N} case={case} img={img}: {n_dep} rays, max err / bound = {float((err / bound).max()):.3f}")
            assert bool((err <= bound).all()) and float(want.abs().max()) > 0
        # ---- every other output: the gradients and the counts bit for bit; the loss sums are fp32 atomic adds of one value per wave, so
        # with one wave (N <= 64) they are the same bits too, and with w waves two launches may add in another order, each addition
        # rounding the running sum once (<= w 2^-24 relative, tests/test_mip_semantic_step.py)
        for a, b in zip(old[1:], new[1:6]):
            assert (a is None and b is None) or torch.equal(a, b)
        oa, ob = old[0].cpu(), new[0].cpu()
        assert all(float(oa[k]) == float(ob[k]) for k in (0, 6, 7))
        waves = (N + 63) // 64
        for k in (1, 2, 3, 4, 5):
            diff = abs(float(oa[k]) - float(ob[k]))
            assert diff == 0 if waves == 1 else diff <= waves * EPS * abs(float(oa[k])), (k, diff)
    # without a confidence the factor is 1 and g_conf is the same expression
    if case == "plain":
        a = ops.mip_loss_tail_masked(d["rgb"], d["tgt"], d["d1"], d["d0"], d["td"], None, None, None, None, None, True, LAM_D, CM, LAM_P, want_g_conf=True)
        assert torch.equal(a[6], new[6])


# ---- GPU: the trainer ---------------------------------------------------------------------------------------------------------------
N_RAYS, STEP_IMGS = 65, [2, 2, 4, 0, 2, 4]
CONF_LR, B1, B2, ADAM_EPS = 1e-3, float(torch.tensor(0.9, dtype=torch.float32)), float(torch.tensor(0.999, dtype=torch.float32)), 1e-8


def _model():
    """the small model of tests/test_pose_refine.py, in deterministic mode (weight-gradient partials folded in a fixed order instead of
    fp32 atomics): two routes that feed the step the same bits must then leave the same bits in the arena"""
    from snerf_amd import mipnerf
    torch.manual_seed(0)
    m = mipnerf.MipNerfModel(n_samples=16, N_fine=17, no_warp_sample=0, ray_shape="cone", fn=1, radius=3., transform_idx=0, real=True,
                             rgb_layer=3, hidden_layer=64, density_noise=0., max_deg_point=16, proposal_hidden_layer=64, proposal_loss=True,
                             compute="f32")
    return m.set_deterministic(True)


def _step_batch(step):
    """65 hand-made rays of image STEP_IMGS[step] with their targets, pixels and the sampler's draws"""
    from oracle import common, mip as om
    from snerf_amd import mipnerf
    g = torch.Generator().manual_seed(900 + step)
    n = N_RAYS
    rays = mipnerf.Rays(**{k: v.cuda() for k, v in common.synthetic_rays(n, seed=20 + step).items()})
    td = torch.rand(n, generator=g) * 4 + 2
    td[torch.rand(n, generator=g) < 0.3] = 0
    s_rand = torch.rand(n, 17, generator=g)
    u = om.rand_u(17, torch.empty(n, 17).uniform_(0, 1 / 17 - om.EPS32, generator=g))
    return dict(rays=rays, tgt=torch.rand(n, 3, generator=g).cuda(), td=td.cuda(), sel=_coords(n, seed=step).cuda(), s_rand=s_rand.cuda(), u=u.cuda(),
                img=torch.tensor([STEP_IMGS[step]], dtype=torch.int64, device="cuda"))


def _conf_trainer(M=3, with_sky=True, conf_lr=CONF_LR):
    from snerf_amd.trainer import MipTrainer
    modes, all_maps, sky, lambdas = _scene(M)
    net = confidence.Confidence(modes, N_IMG)
    net.load_state_dict({"lambdas": lambdas * 0.25})
    maps = confidence.ConfidenceMaps(all_maps, I_TRAIN, N_IMG, H, W, skymask=sky if with_sky else None)
    return MipTrainer(_model(), lr=5e-4, proposal_loss=True, conf_net=net, conf_maps=maps, conf_lr=conf_lr), (modes, all_maps, sky)


@gpu
def test_trainer_conf_step_updates_the_model_like_a_given_confidence():
    """one step with the table against one step from the same state that is handed conf = ops.conf_apply(...): the same bits in the arena"""
    from snerf_amd import ops
    from snerf_amd.trainer import MipTrainer
    b = _step_batch(0)
    tr, _ = _conf_trainer()
    start = tr.conf.flat.clone()
    cf = tr.conf
    conf = ops.conf_apply(cf.maps.maps, cf.maps.slot_of_image, cf.net.lambdas.data.clone(), cf.maps.sky, b["img"], b["sel"])
    tr.step(b["rays"], b["tgt"], b["td"], randomized=True, s_rand=b["s_rand"], u=b["u"], img_i=b["img"], sel_coords=b["sel"])
    assert torch.equal(tr.last_conf, conf) and 0 < int((conf == 1).sum()) < N_RAYS
    ref = MipTrainer(_model(), lr=5e-4, proposal_loss=True)
    ref.step(b["rays"], b["tgt"], b["td"], conf, randomized=True, s_rand=b["s_rand"], u=b["u"])
    assert torch.equal(tr.model.arena.flat, ref.model.arena.flat) and torch.equal(tr.m, ref.m) and torch.equal(tr.v, ref.v)
    assert float((tr.model.arena.flat - _model().arena.flat).abs().max()) > 0
    assert not torch.equal(tr.conf.flat, start) and tr.conf.t == 1 and float(tr.conf.grad.abs().max()) == 0
    # a python int as the image trains the same bits
    tr2, _ = _conf_trainer()
    tr2.step(b["rays"], b["tgt"], b["td"], randomized=True, s_rand=b["s_rand"], u=b["u"], img_i=int(b["img"]), sel_coords=b["sel"])
    assert torch.equal(tr2.conf.flat, tr.conf.flat) and torch.equal(tr2.model.arena.flat, tr.model.arena.flat)


def _adam64(p, m, v, g, t):
    """torch.optim.Adam's step in float64 with the fp32 betas the kernel receives -> (p, m, v)"""
    m = B1 * m + (1 - B1) * g
    v = B2 * v + (1 - B2) * g * g
    bc1, bc2 = 1 - B1 ** t, 1 - B2 ** t
    return p - (CONF_LR / bc1) * m / (v.sqrt() / bc2 ** 0.5 + ADAM_EPS), m, v


@gpu
def test_trainer_trains_the_table_like_float64_adam_over_six_steps():
    """After each step the table against a float64 Adam step from the trainer's previous state (table and moments), fed the float64
    gradient of the restatement at the distances the step returned.
    Margin per entry, from reference quantities only.  (a) The gradient the kernels form is within
        dg_k = u |g_k| + sum_r b_r + 4 (n + 16) 2^-53 sum_r |g_conf_r|
    of the float64 one: test_conf_grad's bound, plus the error b_r of the fp32 g_conf_r (test_g_conf_tail's bound) passed through
    |d lambda_k / d g_conf_r| = c_k |map_kr - conf_r| <= 1.  Its effect on the update: the float64 Adam step evaluated at g +- dg,
    twice the larger deviation (the step is smooth in g on that scale: |g| >> eps here, asserted).  (b) The fp32 Adam kernel:
    1 - b^t is formed from powf(b, t), good to 2 ulp of a number below 1 (4 u absolute), i.e. 4 u / (1 - b1^t) relative for the step
    size and half of 4 u / (1 - b2^t) for sqrt(1 - b2^t); eight more roundings in m, v, the quotient and the product (8 u); all relative
    to the update |dp|; and the final subtraction rounds the table entry (u |p|)."""
    tr, (modes, all_maps, sky) = _conf_trainer()
    cf = tr.conf
    worst = 0.0
    for step, img in enumerate(STEP_IMGS):
        b = _step_batch(step)
        p0, m0, v0 = (x.detach().cpu().double().view(3, N_IMG).clone() for x in (cf.flat, cf.m, cf.v))
        _, outs = tr.step(b["rays"], b["tgt"], b["td"], randomized=True, s_rand=b["s_rand"], u=b["u"], img_i=b["img"], sel_coords=b["sel"])
        d0, d1, td, sel = outs[0].detach().cpu(), outs[5].detach().cpu(), b["td"].cpu(), b["sel"].cpu()
        lam = p0.clone().requires_grad_(True)
        conf = ref_final_confidence(lam, modes, all_maps, I_TRAIN, img, sel, sky)
        ref_depth_loss(d1, d0, td, conf).backward()
        g = lam.grad.clone()
        # (a)
        counted = td != 0
        n_dep = int(counted.sum())
        gc = torch.autograd.grad(ref_depth_loss(d1, d0, td, cc := conf.detach().clone().requires_grad_(True)), cc)[0]
        t_, a1, a0 = (x.double()[counted] for x in (td, d1, d0))
        b_r = (LAM_D / n_dep) * EPS * ((1 / a1 + 1 / t_) + CM * (1 / a0 + 1 / t_)) + 6 * EPS * gc[counted].abs()
        dg = torch.zeros_like(g)
        dg[:, img] = EPS * g[:, img].abs() + float(b_r.sum()) + 4 * (N_RAYS + 16) * EPS64 * float(gc.abs().sum())
        t = step + 1
        want, m1, v1 = _adam64(p0, m0, v0, g, t)
        dev = torch.maximum((_adam64(p0, m0, v0, g + dg, t)[0] - want).abs(), (_adam64(p0, m0, v0, g - dg, t)[0] - want).abs())
        # (b)
        dp = (want - p0).abs()
        margin = 2 * dev + dp * (4 * EPS / (1 - B1 ** t) + 2 * EPS / (1 - B2 ** t) + 8 * EPS) + EPS * want.abs()
        got = cf.flat.detach().cpu().double().view(3, N_IMG)
        err = (got - want).abs()
        worst = max(worst, float((err / margin.clamp_min(1e-300)).max()))
        print(f"step {step} img {img}: max |lambda - float64 Adam| = {float(err.max()):.3e}, max err / margin = {float((err / margin.clamp_min(1e-300)).max()):.3f}, "
              f"max |g| = {float(g.abs().max()):.3e}, max |update| = {float(dp.max()):.3e}")
        assert float(g[:, img].abs().min()) > 100 * ADAM_EPS and float(g[:, [i for i in range(N_IMG) if i != img]].abs().max()) == 0
        assert bool((err <= margin).all()), (step, err, margin)
        assert float(margin.max()) <= 1e-2 * CONF_LR                                            # the margin is a small part of one update
        # a column with history and no gradient this step still moves on its momentum; a column never visited stays put exactly
        seen = set(STEP_IMGS[:step + 1])
        for i in range(N_IMG):
            if i not in seen:
                assert torch.equal(got[:, i], p0[:, i]) and float(cf.m.view(3, N_IMG)[:, i].abs().max()) == 0
            elif i != img:
                assert float((got[:, i] - p0[:, i]).abs().min()) > 0.01 * CONF_LR
    assert cf.t == 6 and tr.t == 6
    # the optimiser state: round trip, and through a real torch.optim.Adam over a torch Confidence
    from snerf_amd.trainer import MipTrainer
    sd = tr.conf_state_dict()
    assert list(sd["state"]) == [0] and float(sd["state"][0]["step"]) == 6 and sd["param_groups"][0]["lr"] == CONF_LR
    assert tuple(sd["state"][0]["exp_avg"].shape) == (3, N_IMG)
    torch_net = confidence.Confidence(modes, N_IMG).cuda()
    opt = torch.optim.Adam([{"params": [p for p in torch_net.parameters() if p.requires_grad], "lr": 1.0}])
    opt.load_state_dict(sd)
    assert opt.param_groups[0]["lr"] == CONF_LR and torch.equal(opt.state[torch_net.lambdas]["exp_avg"], cf.m.view(3, N_IMG))
    assert torch.equal(opt.state[torch_net.lambdas]["exp_avg_sq"], cf.v.view(3, N_IMG))
    tr2, _ = _conf_trainer(conf_lr=7.0)
    tr2.load_conf_state_dict(opt.state_dict())
    assert tr2.conf.t == 6 and tr2.conf.lr == CONF_LR and torch.equal(tr2.conf.m, cf.m) and torch.equal(tr2.conf.v, cf.v)


# ---- GPU: the captured step ---------------------------------------------------------------------------------------------------------
def _batcher(n=N_RAYS, seed=3):
    from snerf_amd import sample_utils as su
    rng = np.random.default_rng(1)
    images = rng.random((N_IMG, H, W, 3), dtype=np.float32)
    depths = (rng.random((N_IMG, H, W)) * 4 + 2).astype(np.float32)
    depths[rng.random((N_IMG, H, W)) < 0.4] = 0
    cams = np.zeros((N_IMG, 3, 4), np.float32)
    for i in range(N_IMG):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        cams[i, :, :3], cams[i, :, 3] = q, rng.normal(size=3) * 0.1
    K = np.zeros((N_IMG, 3, 3), np.float32)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = 20.0, 20.0, W / 2, H / 2, 1
    args = types.SimpleNamespace(no_ndc=True, smooth_loss=False, near_far=False, N_rgb=n)
    return su.ImageRayBatcher(args, images, depths, cams, K, list(I_TRAIN), 2.0, 6.0, camera_index=np.arange(N_IMG) * 1.0, batch_n=n, seed=seed,
                              device="cuda")


@gpu
def test_capture_with_conf_net_trains_the_table_inside_the_graph():
    """three replays with a batcher against three eager steps from the same state (deterministic model, no random draws: the same
    bits), and a warm-up that leaves the table where it was"""
    steps = 3
    # eager
    b, (tr, _) = _batcher(), _conf_trainer()
    start = tr.conf.flat.clone()
    imgs = []
    for _ in range(steps):
        rays, trgb, tdep, sel, img, _ = b.next()
        imgs.append(int(img))
        tr.step(rays, trgb, tdep, randomized=False, img_i=img, sel_coords=sel)
    eager = (tr.conf.flat.clone(), tr.conf.m.clone(), tr.conf.v.clone(), tr.model.arena.flat.clone())
    assert tr.conf.t == steps and len(set(imgs)) >= 2
    # captured
    b, (tr, _) = _batcher(), _conf_trainer()
    init = tr.model.arena.flat.clone()
    tr.capture(None, None, randomized=False, warmup=2, batcher=b)
    torch.cuda.synchronize()
    cf = tr.conf
    assert torch.equal(cf.flat, start) and float(cf.m.abs().max()) == 0 and float(cf.v.abs().max()) == 0 and float(cf.grad.abs().max()) == 0
    assert cf.t == 0 and int(cf.step_dev) == 0 and tr.t == 0 and torch.equal(tr.model.arena.flat, init) and b.step == 0 and int(b.counter[0]) == 0
    for k in range(steps):
        loss, _ = tr.replay()
        assert int(tr.batch[4]) == imgs[k] and np.isfinite(float(loss))
    assert cf.t == steps and int(cf.step_dev) == steps and tr.t == steps and b.step == steps
    for name, got, want in zip(("lambdas", "exp_avg", "exp_avg_sq", "arena"), (cf.flat, cf.m, cf.v, tr.model.arena.flat), eager):
        print(f"captured vs eager {name}: max |diff| = {float((got - want).abs().max()):.3e}")
        assert torch.equal(got, want), name
    moved = (cf.flat - start).view(3, N_IMG).abs()
    assert float(moved[:, sorted(set(imgs))].min()) > 0.1 * CONF_LR
    assert float(moved[:, [i for i in range(N_IMG) if i not in imgs]].max()) == 0
