"""Semantic cross-entropy and per-image ray masks in the fused mip step: the kernel pair behind snerf_mip_loss_tail_masked,
ops.mip_loss_tail_masked, trainer.MipLossRules and the new arguments of MipTrainer.step / capture.

The yardstick is the reference's loss block (s-nerf/train.py:131-209, model/loss_factory.py, model/loss.py:330-346) restated once
below in torch and evaluated in float64 on the CPU: the Waymo side-camera mask on the RGB and semantic means, the back-camera mask
(with seg_mask == 0) on the depth mean only, nn.CrossEntropyLoss (ignore_index -100) times semantic_lambda for images with labels.
The one stated deviation: a mean over no ray is 0 with zero gradients here, NaN in the reference."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import callers as oc
from oracle import common
from snerf_amd import _lib

gpu = pytest.mark.gpu
EPS = 2.0 ** -24                                        # half an ulp of 1 in fp32: the relative error of one rounding
LAM_D, CM, LAM_P, LAM_S = 0.2, 0.2, 0.05, 0.1           # depth_lambda, coarse_depth_mult, proposal_lambda, semantic_lambda (arg_parser.py:166)
H_IMG = 8


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def restated_terms(t, dtype, rgb_lim=None, dep_lim=None, sem_on=True, disparity=True, lam_s=LAM_S):
    """t: rgb, tgt [n,3]; d1, d0, td, conf, keep [n] (td None = no depth term; conf / keep optional); s_f, w_f, s_c, w_c (s_c None = no
    proposal term); sem [n,C], labels [n] (sem None = no semantic term); rows [n] int64.  rgb_lim / dep_lim: the image's row limits
    (None = no rule); sem_on: the image has labels.  -> ({rgb, depth, proposal, semantic, total}, {depth, rgb, semantic} counts);
    differentiable w.r.t. whatever in `t` requires grad."""
    f = lambda k: None if t.get(k) is None else t[k].to(dtype)
    n = t["rgb"].shape[0]
    everyone = torch.ones(n, dtype=torch.bool)
    zero = torch.zeros((), dtype=dtype)
    rows = t.get("rows")
    # train.py:137-149: the side-camera mask, then RgbLoss
    rgb_mask = rows < rgb_lim if rgb_lim is not None else everyone
    n_rgb = int(rgb_mask.sum())
    l_rgb = torch.mean((f("rgb")[rgb_mask] - f("tgt")[rgb_mask]) ** 2) if n_rgb else zero
    # train.py:165-170 + loss.py:330-346: DepthLoss on the rays with a target, times the confidence, then the back-camera mask
    l_dep, n_dep = zero, 0
    if t.get("td") is not None:
        backcam = rows < dep_lim if dep_lim is not None else everyone
        if t.get("keep") is not None:
            backcam = backcam & (t["keep"] == 0)
        tm = t["td"] != 0
        fn = (lambda x, y: torch.abs(1 / x - 1 / y)) if disparity else (lambda x, y: torch.abs(x - y))
        dl = fn(f("d1")[tm], f("td")[tm]) + CM * fn(f("d0")[tm], f("td")[tm])
        if t.get("conf") is not None:
            dl = dl * f("conf")[tm]
        dl = dl[backcam[tm]]
        n_dep = dl.numel()
        l_dep = dl.mean() * LAM_D if n_dep else zero
    # train.py:180-182: every ray
    l_prop = oc.proposal_loss(f("s_f"), f("w_f"), f("s_c"), f("w_c"), LAM_P) if t.get("s_c") is not None else zero
    # train.py:131-134,142-144,185-191: SemanticLoss on the rays inside the side-camera mask
    l_sem, n_sem = zero, 0
    if t.get("sem") is not None and sem_on:
        lab = t["labels"].long()[rgb_mask]
        n_sem = int((lab != -100).sum())
        if n_sem:
            l_sem = F.cross_entropy(f("sem")[rgb_mask], lab) * lam_s
    terms = dict(rgb=l_rgb, depth=l_dep, proposal=l_prop, semantic=l_sem, total=((l_rgb + l_dep) + l_prop) + l_sem)
    return terms, dict(depth=n_dep, rgb=n_rgb, semantic=n_sem)


LEAVES = ("rgb", "d1", "d0", "w_c", "sem")


def restated(c, dtype, **kw):
    """-> (terms, counts, gradients of the total w.r.t. rgb, d1, d0, w_c, sem) on detached copies of `c`"""
    t = dict(c)
    for k in LEAVES:
        if c.get(k) is not None:
            t[k] = c[k].detach().to(dtype).clone().requires_grad_(True)
    terms, counts = restated_terms(t, dtype, **kw)
    leaves = [k for k in LEAVES if c.get(k) is not None]
    gs = torch.autograd.grad(terms["total"], [t[k] for k in leaves], allow_unused=True) if terms["total"].requires_grad else [None] * len(leaves)
    grads = {k: (torch.zeros_like(t[k]) if g is None else g).detach() for k, g in zip(leaves, gs)}
    return {k: v.detach() for k, v in terms.items()}, counts, grads


def tail_inputs(N, C, Sc=8, Pf=9, seed=0, scale=40.0):
    """one batch of loss-tail inputs on the CPU: logits in +-scale, a fifth of the labels -100, rows in [0, H_IMG)"""
    g = torch.Generator().manual_seed(1000 * N + C + seed)
    r = lambda *s: torch.rand(*s, generator=g)

    def fence(P):
        s = torch.sort(r(N, P), dim=-1).values
        s[:, 0], s[:, -1] = 0.0, 1.0
        return s
    w_c, w_f = r(N, Sc) ** 2, r(N, Pf - 1) ** 3
    td = r(N) * 20 + 2
    td[r(N) < 0.3] = 0
    labels = torch.randint(0, C, (N,), generator=g)
    labels[r(N) < 0.2] = -100
    return dict(rgb=r(N, 3), tgt=r(N, 3), d1=r(N) + 1, d0=r(N) + 1, td=td, conf=r(N), keep=(r(N) < 0.3).float(),
                s_f=fence(Pf), w_f=w_f / w_f.sum(-1, keepdim=True), s_c=fence(Sc + 1), w_c=w_c / w_c.sum(-1, keepdim=True) * r(N, 1),
                sem=(r(N, C) * 2 - 1) * scale, labels=labels, rows=torch.randint(0, H_IMG, (N,), generator=g))


def emulated_masked_tail(rgb, tgt, dist1, dist0, tdepth, conf, s_f, w_f, s_c, w_c, disparity, depth_lambda, coarse_mult, prop_lambda,
                         sem=None, labels=None, semantic_lambda=0.1, rows=None, img_i=None, rgb_row_limit=None, depth_row_limit=None,
                         sem_valid=None, depth_keep=None):
    """ops.mip_loss_tail_masked for the CPU emulation: the restatement in float32"""
    assert (depth_lambda, coarse_mult, prop_lambda) == (LAM_D, CM, LAM_P)
    c = dict(rgb=rgb, tgt=tgt, d1=dist1, d0=dist0, td=tdepth, conf=conf, keep=depth_keep, s_f=s_f, w_f=w_f, s_c=s_c, w_c=w_c, sem=sem,
             labels=labels, rows=None if rows is None else rows[:, 0])
    kw = {}
    if rows is not None:
        i = int(img_i)
        kw = dict(rgb_lim=int(rgb_row_limit[i]), dep_lim=int(depth_row_limit[i]), sem_on=bool(sem_valid[i]))
    terms, counts, g = restated(c, torch.float32, disparity=bool(disparity), lam_s=semantic_lambda, **kw)
    out = torch.tensor([counts["depth"], terms["rgb"], terms["depth"], terms["proposal"], terms["total"], terms["semantic"], counts["rgb"],
                        counts["semantic"]], dtype=torch.float32)
    return out, g["rgb"], g.get("d1"), g.get("d0"), g.get("w_c"), g.get("sem")


# ---- without a GPU: the C entry's refusals ------------------------------------------------------------------------------------------
_P = lambda k: 1 << 20 | k << 12                        # distinct fake device addresses, 4096 bytes apart: never dereferenced


def _tail_args(**kw):
    a = dict(rgb=_P(1), tgt=_P(2), dist1=_P(3), dist0=_P(4), tdepth=_P(5), conf=_P(6), s_f=_P(7), w_f=_P(8), s_c=_P(9), w_c=_P(10), sem=_P(11),
             labels=_P(12), labels_f32=0, C=7, rows=_P(13), img_i=_P(14), rgb_row_limit=_P(15), depth_row_limit=_P(16), sem_valid=_P(17),
             n_images=3, depth_keep=_P(18), N=24, Pf=17, Sc=16, disparity=1, depth_lambda=0.2, coarse_mult=0.2, prop_lambda=0.05,
             semantic_lambda=0.1, out=_P(19), g_rgb=_P(20), g_dist1=_P(21), g_dist0=_P(22), g_wc=_P(23), g_sem=_P(24), stream=None)
    a.update(kw)
    return a


def test_masked_tail_rejects_bad_arguments_without_a_gpu():
    """argument validation happens before any launch (the pointers here are never dereferenced)"""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    assert [n for _, n in _lib.parse_header()["snerf_mip_loss_tail_masked"]] == list(_tail_args())
    bad = [dict(rgb=None), dict(tgt=None), dict(out=None), dict(g_rgb=None), dict(dist1=None), dict(dist0=None), dict(g_dist1=None),
           dict(g_dist0=None), dict(s_f=None), dict(w_f=None), dict(w_c=None), dict(g_wc=None), dict(Pf=1), dict(Sc=0),
           dict(C=0), dict(C=33), dict(C=-1), dict(sem=None), dict(labels=None), dict(g_sem=None), dict(labels_f32=2), dict(labels_f32=-1),
           dict(rows=None), dict(img_i=None), dict(rgb_row_limit=None), dict(depth_row_limit=None), dict(sem_valid=None), dict(n_images=0),
           dict(tdepth=None)]                                      # (the last: depth_keep without a depth term)
    for kw in bad:
        with pytest.raises(_lib.SnerfHipError, match="bad argument"):
            _lib.call("snerf_mip_loss_tail_masked", *_tail_args(**kw).values())
    # an empty batch is a no-op, whatever the rest
    none = {k: None for k, v in _tail_args().items() if isinstance(v, int) and v >= (1 << 20)}
    for n in (0, -1):
        assert _lib.call("snerf_mip_loss_tail_masked", *_tail_args(N=n, C=0, **none).values()) is None


# ---- without a GPU: the rule tables -------------------------------------------------------------------------------------------------
def test_mip_loss_rules_tables():
    from snerf_amd.trainer import MipLossRules
    cams = [0, 3, 1, 4, 0, 2]
    lst = lambda t: t.tolist()
    r = MipLossRules(6, 900, cams)
    assert lst(r.rgb_row_limit) == [900] * 6 and lst(r.depth_row_limit) == [900] * 6 and lst(r.sem_valid) == [0] * 6
    assert all(t.dtype == torch.int32 for t in (r.rgb_row_limit, r.depth_row_limit, r.sem_valid))
    r = MipLossRules(6, 900, cams, waymo=True)
    assert lst(r.rgb_row_limit) == [900, 886, 900, 886, 900, 900] and lst(r.depth_row_limit) == [900] * 6
    r = MipLossRules(6, 900, np.asarray(cams, np.float64), backcam=True)
    assert lst(r.rgb_row_limit) == [900] * 6 and lst(r.depth_row_limit) == [750, 900, 900, 900, 750, 900]
    r = MipLossRules(6, 8, torch.tensor(cams), semantic_index=[1, 4, 5], waymo=True, backcam=True, waymo_cams=(1, 2), waymo_row_limit=5,
                     backcam_cam=3, backcam_row_limit=4)
    assert lst(r.rgb_row_limit) == [8, 8, 5, 8, 8, 5] and lst(r.depth_row_limit) == [8, 4, 8, 8, 8, 8] and lst(r.sem_valid) == [0, 1, 0, 0, 1, 1]
    assert all(torch.equal(a, b) for a, b in zip(r.on("cpu"), (r.rgb_row_limit, r.depth_row_limit, r.sem_valid))) and r.on("cpu") is r.on("cpu")
    with pytest.raises(ValueError, match="one entry per image"):
        MipLossRules(5, 8, cams)
    with pytest.raises(ValueError, match="semantic_index"):
        MipLossRules(6, 8, cams, semantic_index=[6])


# ---- the fused step against autograd (CPU emulation and GPU share the case) ---------------------------------------------------------
N_STEP, C_STEP = 24, 7


def _semantic_model(device):
    """the model of golden g14 (tests/test_paths.py::test_mipnerf_semantic_head_vs_reference_golden)"""
    from snerf_amd import mipnerf
    m = mipnerf.MipNerfModel(n_samples=16, N_fine=17, no_warp_sample=0, ray_shape="cone", fn=1, radius=3., transform_idx=0, real=True,
                             rgb_layer=3, hidden_layer=64, density_noise=0., max_deg_point=16, proposal_hidden_layer=64,
                             proposal_loss=True, semantic=True, semantic_class_num=C_STEP, compute="f32", device=device)
    m.load_state_dict(common.fill_state_dict_({k: torch.empty(v.shape) for k, v in m.state_dict().items()}))
    return m


def _step_rules():
    """three images 8 rows high; image 0 has both row limits (5 for RGB / semantic, 4 for depth) and labels"""
    from snerf_amd.trainer import MipLossRules
    return MipLossRules(3, H_IMG, [0, 3, 1], semantic_index=[0, 1], waymo=True, backcam=True, waymo_cams=(0, 3), waymo_row_limit=5,
                        backcam_cam=0, backcam_row_limit=4)


def _step_case():
    g = torch.Generator().manual_seed(3)
    n = N_STEP
    rc = common.synthetic_rays(n, seed=2)
    td = torch.rand(n, generator=g) * 20 + 2
    td[::5] = 0
    labels = torch.randint(0, C_STEP, (n,), generator=g).float()
    labels[1::6] = -100
    rows = torch.arange(n) % H_IMG
    sel = torch.stack([rows, torch.arange(n) % 11], -1)
    keep = (torch.arange(n) % 7 == 3).float()
    return rc, dict(tgt=torch.rand(n, 3, generator=g), td=td, conf=torch.rand(n, generator=g), labels=labels, sel=sel, keep=keep)


def _fused_step_against_autograd(dev, ray_grads):
    """-> (trainer, {name: (fused gradient, autograd gradient)}, [(fused, autograd) ray gradients])"""
    from snerf_amd import mipnerf
    from snerf_amd.trainer import MipTrainer
    m = _semantic_model(dev)
    rc, x = _step_case()
    to = lambda v: v.to(dev)
    rays = {k: to(v) for k, v in rc.items()}
    leaves = {k: rays[k].clone().requires_grad_(True) for k in ("origins", "directions", "viewdirs")} if ray_grads else {}
    ret = m(mipnerf.Rays(**{**rays, **leaves}), False, False, 0.)
    # the restated loss on the model's differentiable outputs (float64 on the CPU; autograd carries it back into the model)
    t = dict(rgb=ret[1][0], d1=ret[1][1], d0=ret[0][1], s_f=ret[1][4], w_f=ret[1][5], s_c=ret[0][3], w_c=ret[0][4], sem=ret[1][3])
    t = {k: v.cpu() for k, v in t.items()}
    t.update(tgt=x["tgt"], td=x["td"], conf=x["conf"], keep=x["keep"], labels=x["labels"], rows=x["sel"][:, 0])
    terms, counts = restated_terms(t, torch.float64, rgb_lim=5, dep_lim=4, sem_on=True)
    terms["total"].backward()
    ref = {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters()}
    ref_rays = [leaves[k].grad.detach().cpu().clone() for k in leaves]
    tr = MipTrainer(m, lr=5e-4, depth_lambda=LAM_D, coarse_depth_mult=CM, proposal_loss=True, proposal_lambda=LAM_P, semantic_lambda=LAM_S,
                    loss_rules=_step_rules())
    m.arena.grad.zero_()
    tr._forward_backward(mipnerf.Rays(**rays), to(x["tgt"]), to(x["td"]), to(x["conf"]), False, None, None, ray_grads, None, 0,
                         target_semantic=to(x["labels"]), sel_coords=to(x["sel"]), depth_keep=to(x["keep"]))
    got = {k: m.arena.g[k].detach().cpu().clone() for k in ref}
    m.arena.grad.zero_()
    assert [int(v) for v in tr.last_counts] == [counts["depth"], counts["rgb"], counts["semantic"]]
    assert all(int(v) > 0 for v in tr.last_counts) and counts["rgb"] < N_STEP and counts["depth"] < int((x["td"] != 0).sum())
    for k, name in ((1, "rgb"), (2, "depth"), (3, "proposal")):
        assert abs(float(tr.last_losses[k]) - float(terms[name].detach())) <= 1e-4 * abs(float(terms[name].detach())), name
    sem_ref = float(terms["semantic"].detach())
    assert abs(float(tr.last_semantic_loss) - sem_ref) <= 1e-4 * sem_ref and sem_ref > 0
    rg = [] if not ray_grads else [(a.cpu(), b) for a, b in zip(tr.last_ray_grads, ref_rays)]
    return tr, {k: (got[k], ref[k]) for k in ref}, rg


def _check_step_gradients(pairs, rays):
    """per parameter tensor within 1e-4 max|ref| (the bound of tests/test_callers.py for the fused step against autograd)"""
    head = [k for k in pairs if "semantic" in k]
    assert head and all(float(pairs[k][0].norm()) > 0 and float(pairs[k][1].norm()) > 0 for k in head), head
    worst = 0.0
    for k, (got, ref) in pairs.items():
        scale = float(ref.abs().max())
        assert scale > 0, k
        worst = max(worst, float((got - ref).abs().max()) / scale)
        assert float((got - ref).abs().max()) <= 1e-4 * scale, (k, float((got - ref).abs().max()), scale)
    for got, ref in rays:
        scale = float(ref.abs().max())
        worst = max(worst, float((got - ref).abs().max()) / scale)
        assert scale > 0 and float((got - ref).abs().max()) <= 1e-4 * scale
    print(f"MEASURED fused step vs autograd: worst max|diff| / max|ref| = {worst:.3e} (bound 1e-4)")


def test_fused_step_trains_the_semantic_head_like_autograd_on_the_cpu_emulation(monkeypatch):
    """host logic of the step (labels, rules, confidence, depth_keep) on the CPU emulation: the gradient arena after
    _forward_backward against autograd through model(rays) with the restated loss.  Gradients, not parameters after Adam: Adam's
    update is scale-invariant and would hide a wrong semantic_lambda on the head-only parameters."""
    from cpu_ops_emulation import emulate_ops
    with emulate_ops() as ops:
        monkeypatch.setattr(ops, "mip_loss_tail_masked", emulated_masked_tail)
        _, pairs, _ = _fused_step_against_autograd("cpu", False)
    _check_step_gradients(pairs, [])


def test_step_without_the_new_arguments_calls_the_plain_tail(monkeypatch):
    from cpu_ops_emulation import emulate_ops
    from snerf_amd import mipnerf
    from snerf_amd.trainer import MipTrainer
    calls = {"plain": 0, "masked": 0}
    with emulate_ops() as ops:
        plain = ops.mip_loss_tail

        def count_plain(*a, **k):
            calls["plain"] += 1
            return plain(*a, **k)

        def count_masked(*a, **k):
            calls["masked"] += 1
            return emulated_masked_tail(*a, **k)
        monkeypatch.setattr(ops, "mip_loss_tail", count_plain)
        monkeypatch.setattr(ops, "mip_loss_tail_masked", count_masked)
        m = _semantic_model("cpu")
        rc, x = _step_case()
        tr = MipTrainer(m, lr=5e-4, proposal_loss=True)
        tr.step(mipnerf.Rays(**rc), x["tgt"], x["td"], x["conf"], randomized=False)
        assert calls == {"plain": 1, "masked": 0} and tuple(tr.last_losses.shape) == (4,)
        assert tr.last_semantic_loss is None and tr.last_counts is None
        # labels alone (no rules) take the masked tail; last_losses stays the four entries it is
        tr.step(mipnerf.Rays(**rc), x["tgt"], x["td"], x["conf"], randomized=False, target_semantic=x["labels"])
        assert calls == {"plain": 1, "masked": 1} and tuple(tr.last_losses.shape) == (4,)
        assert [int(v) for v in tr.last_counts] == [int((x["td"] != 0).sum()), N_STEP, int((x["labels"] != -100).sum())]
        # refusals of the host layer
        plain_model = mipnerf.MipNerfModel(n_samples=8, N_fine=9, no_warp_sample=0, ray_shape="cone", fn=1, radius=3., transform_idx=0, real=True,
                                           rgb_layer=3, hidden_layer=64, density_noise=0., max_deg_point=16, proposal_hidden_layer=64,
                                           proposal_loss=True, compute="f32", device="cpu")
        with pytest.raises(ValueError, match="semantic head"):
            MipTrainer(plain_model, proposal_loss=True).step(mipnerf.Rays(**rc), x["tgt"], target_semantic=x["labels"])
        ruled = MipTrainer(m, proposal_loss=True, loss_rules=_step_rules())
        with pytest.raises(ValueError, match="sel_coords"):
            ruled.step(mipnerf.Rays(**rc), x["tgt"], img_i=0)
        with pytest.raises(ValueError, match="sel_coords"):
            ruled.step(mipnerf.Rays(**rc), x["tgt"], sel_coords=x["sel"])
        with pytest.raises(ValueError, match="batcher"):                 # rules are captured with a batcher only
            ruled.capture(mipnerf.Rays(**rc), x["tgt"], img_i=torch.zeros(1, dtype=torch.int64))
        assert ruled._step_dev is None                                   # a refused capture arms nothing: the steps below count on the host
        # a python int as the image is wrapped once per value
        ruled.step(mipnerf.Rays(**rc), x["tgt"], randomized=False, img_i=1, sel_coords=x["sel"])
        first = ruled._img_dev[1]
        ruled.step(mipnerf.Rays(**rc), x["tgt"], randomized=False, img_i=1, sel_coords=x["sel"])
        assert ruled._img_dev[1] is first and int(first) == 1
        ruled.step(mipnerf.Rays(**rc), x["tgt"], randomized=False, img_i=2, sel_coords=x["sel"])
        assert ruled._img_dev[1] is not first and int(ruled._img_dev[1]) == 2
        calls["masked"] -= 3
        with pytest.raises(ValueError, match="target_depth"):
            tr.step(mipnerf.Rays(**rc), x["tgt"], depth_keep=x["keep"])
        with pytest.raises(ValueError, match="pose_net or loss_rules"):
            tr.step(mipnerf.Rays(**rc), x["tgt"], img_i=0)
        assert calls == {"plain": 1, "masked": 1}


# ---- GPU: the kernel against the float64 restatement --------------------------------------------------------------------------------
# per-image tables of the kernel test: 0 no rule, 1 RGB / semantic row limit, 2 depth row limit, 3 no labels, 4 both limits 0
RGB_LIM, DEP_LIM, SEM_VALID = [H_IMG, 5, H_IMG, H_IMG, 0], [H_IMG, H_IMG, 4, H_IMG, 0], [1, 1, 1, 0, 1]


def _tol(ref64, ref32):
    """4 x the distance of torch's own float32 CPU evaluation from the float64 one (summation and atomic order), with a floor of
    16 * 2^-24 relative to the largest reference magnitude"""
    d32 = float((ref32.double() - ref64).abs().max())
    return max(4 * d32, 16 * EPS * float(ref64.abs().max())), d32


def _run_masked(ops, d, img=None, labels=None, proposal=True, semantic=True, keep=True):
    tables = [torch.tensor(v, dtype=torch.int32, device="cuda") for v in (RGB_LIM, DEP_LIM, SEM_VALID)]
    kw = {}
    if img is not None:
        kw = dict(rows=d["sel"], img_i=torch.tensor([img], dtype=torch.int64, device="cuda"), rgb_row_limit=tables[0], depth_row_limit=tables[1],
                  sem_valid=tables[2])
    p = (lambda k: d[k]) if proposal else (lambda k: None)
    return ops.mip_loss_tail_masked(d["rgb"], d["tgt"], d["d1"], d["d0"], d["td"], d["conf"], p("s_f"), p("w_f"), p("s_c"), p("w_c"), True, LAM_D, CM,
                                    LAM_P, sem=d["sem"] if semantic else None, labels=labels if semantic else None, semantic_lambda=LAM_S,
                                    depth_keep=d["keep"] if keep else None, **kw)


# Measured on the MI355X, worst over the 16 (N, C) cases, the 5 images and both label forms, in units of 2^-24 relative to the largest
# reference magnitude of the output (kernel vs float64 / torch float32 on the CPU vs float64):
#   rgb 1.86 / 1.85, depth 1.71 / 1.71, proposal 1.31 / 1.98, semantic 1.40 / 2^24, total 1.76 / 2.66,
#   g_rgb 1.36 / 1.36, g_d1 2.24 / 2.53, g_d0 3.10 / 2.80, g_w_c 606 / 606, g_sem 1.22 / 2^24.
# semantic / g_sem: at N = 1, C = 2 the ray's loss is log(1 + e^-d) with d between 17 and 36 -- below float32's resolution of 1 + x, so
# torch's float32 evaluation returns 0 (distance = the whole value) while the kernel's float64 log-sum-exp keeps it.  g_w_c: `w + 1e-8` of
# ProposalLoss rounds to w in float32, in torch and in the kernel alike (the same 606 units for both).  Everything else sits under the
# floor of 16 units.
@gpu
@pytest.mark.parametrize("C", [1, 2, 29, 32])
@pytest.mark.parametrize("N", [1, 64, 65, 130])
def test_masked_tail_kernel_against_the_float64_restatement(N, C):
    """Every output of snerf_mip_loss_tail_masked, for each image of the tables above and both label forms, against the restatement in
    float64; the tolerance is 4 x the distance of torch's float32 CPU evaluation of the same expression from the float64 one, floor
    16 * 2^-24 relative (measured figures: the comment above)."""
    from snerf_amd import ops
    c = tail_inputs(N, C)
    d = {k: v.cuda().contiguous() for k, v in c.items() if k not in ("labels", "rows")}
    d["sel"] = torch.stack([c["rows"], torch.zeros_like(c["rows"])], -1).cuda()
    forms = dict(int32=c["labels"].to(torch.int32).cuda(), fp32=c["labels"].float().cuda())
    worst = {}
    for img in range(5):
        kw = dict(rgb_lim=RGB_LIM[img], dep_lim=DEP_LIM[img], sem_on=bool(SEM_VALID[img]))
        t64, counts, g64 = restated(c, torch.float64, **kw)
        t32, counts32, g32 = restated(c, torch.float32, **kw)
        assert counts == counts32
        for form, labels in forms.items():
            out, g_rgb, g_d1, g_d0, g_wc, g_sem = _run_masked(ops, d, img, labels)
            torch.cuda.synchronize()
            out = out.cpu()
            assert [int(out[0]), int(out[6]), int(out[7])] == [counts["depth"], counts["rgb"], counts["semantic"]], (img, form)
            got = dict(rgb=out[1], depth=out[2], proposal=out[3], total=out[4], semantic=out[5], g_rgb=g_rgb, g_d1=g_d1, g_d0=g_d0, g_w_c=g_wc,
                       g_sem=g_sem)
            for name, val in got.items():
                r64, r32 = (t64[name], t32[name]) if name in t64 else (g64[name[2:]], g32[name[2:]])
                tol, d32 = _tol(r64, r32)
                val = val.detach().cpu().double().reshape(r64.shape)
                assert bool(torch.isfinite(val).all()), (img, form, name)
                err = float((val - r64).abs().max())
                scale = float(r64.abs().max())
                if scale > 0:
                    w = worst.setdefault(name, [0.0, 0.0])
                    w[0], w[1] = max(w[0], err / scale), max(w[1], d32 / scale)
                assert err <= tol, (img, form, name, err, tol)
            if not SEM_VALID[img] or RGB_LIM[img] == 0:                   # no labels / nothing inside the mask: exactly nothing
                assert float(out[5]) == 0 and float(g_sem.abs().max()) == 0
            if RGB_LIM[img] == 0:
                assert float(out[1]) == 0 and float(out[2]) == 0 and float(g_rgb.abs().max()) == 0
                assert float(g_d1.abs().max()) == 0 and float(g_d0.abs().max()) == 0
    # every count zero and no proposal term: loss 0, gradients 0, no NaN anywhere
    out, g_rgb, g_d1, g_d0, g_wc, g_sem = _run_masked(ops, d, 4, forms["fp32"], proposal=False)
    assert g_wc is None and torch.equal(out.cpu(), torch.zeros(8))
    assert all(bool((g == 0).all()) for g in (g_rgb, g_d1, g_d0, g_sem))
    # an image index outside the tables counts no ray either
    out = _run_masked(ops, d, 5, forms["int32"], proposal=False)[0]
    assert torch.equal(out.cpu(), torch.zeros(8))
    for name, (e, d32) in worst.items():
        print(f"MEASURED N={N} C={C} {name}: kernel vs float64 {e / EPS:.2f} x 2^-24, torch float32 vs float64 {d32 / EPS:.2f} x 2^-24 (relative to max|ref|)")


@gpu
@pytest.mark.parametrize("form", ["int32", "fp32"])
def test_masked_tail_semantic_term_without_rules_ignores_labels_outside_the_classes(form):
    """the semantic term alone (no rows / img_i / tables: every ray, always active), and the documented deviation: a label outside
    [0, C) other than -100 -- C, -1, far off, and in the fp32 form a non-integer or non-finite value -- is left out like -100 (the
    reference raises on one); reference = the restatement with those labels set to -100"""
    from snerf_amd import ops
    N, C = 65, 7
    c = tail_inputs(N, C)
    bad = [C, -1, 1000, -101, C + 25] + ([3.5, 0.5, -0.5, float("nan"), float("inf")] if form == "fp32" else [])
    labels = c["labels"].double()
    where = torch.arange(len(bad)) * 6 + 1
    where[-1] = N - 1                                                    # one of them in the second wave
    labels[where] = torch.tensor(bad, dtype=torch.float64)
    dev_labels = labels.float().cuda() if form == "fp32" else labels.to(torch.int32).cuda()
    c["labels"][where] = -100
    assert int((c["labels"] != -100).sum()) > 0
    d = {k: v.cuda().contiguous() for k, v in c.items() if k not in ("labels", "rows")}
    t64, counts, g64 = restated(c, torch.float64)
    t32, _, g32 = restated(c, torch.float32)
    out, g_rgb, g_d1, g_d0, g_wc, g_sem = _run_masked(ops, d, None, dev_labels)
    out = out.cpu()
    assert [int(out[0]), int(out[6]), int(out[7])] == [counts["depth"], N, counts["semantic"]]
    assert float(g_sem[where.cuda()].abs().max()) == 0 and bool(torch.isfinite(g_sem).all())
    for name, val, r64, r32 in (("semantic", out[5], t64["semantic"], t32["semantic"]), ("total", out[4], t64["total"], t32["total"]),
                                ("g_sem", g_sem, g64["sem"], g32["sem"]), ("g_rgb", g_rgb, g64["rgb"], g32["rgb"])):
        tol, d32 = _tol(r64, r32)
        err = float((val.detach().cpu().double().reshape(r64.shape) - r64).abs().max())
        print(f"MEASURED no rules, {form} labels, {name}: kernel vs float64 {err / float(r64.abs().max()) / EPS:.2f} x 2^-24, "
              f"torch float32 vs float64 {d32 / float(r64.abs().max()) / EPS:.2f} x 2^-24")
        assert err <= tol, (name, err, tol)


@gpu
@pytest.mark.parametrize("N", [1, 64, 65, 130])
def test_masked_tail_without_the_new_pointers_is_the_plain_tail(N):
    """gradients bit for bit; loss values within the atomic-order noise of the plain entry against itself: one wave (N <= 64) adds once
    into a zeroed word, so the values are equal; with w waves the w atomic adds of a term may land in another order, each rounding
    the running sum once (<= w * 2^-24 relative).  The bound is the largest distance between four calls of the plain entry, or that
    analytic figure where it is larger: an addition to the measured noise, which came out 0 in every run (so did masked vs plain), so
    that a first reordering of the atomics on some later day does not fail the test."""
    from snerf_amd import ops
    c = tail_inputs(N, 7, Sc=16, Pf=17)
    d = {k: v.cuda().contiguous() for k, v in c.items() if k not in ("labels", "rows")}
    plain = lambda: ops.mip_loss_tail(d["rgb"], d["tgt"], d["d1"], d["d0"], d["td"], d["conf"], d["s_f"], d["w_f"], d["s_c"], d["w_c"], True, LAM_D, CM, LAM_P)
    a, b, more = plain(), plain(), [plain()[0].cpu() for _ in range(2)]
    new = _run_masked(ops, d, semantic=False, keep=False)
    assert new[5] is None
    for x, y, z in zip(a[1:], b[1:], new[1:5]):
        assert torch.equal(x, y) and torch.equal(x, z)
    oa, ob, on = a[0].cpu(), b[0].cpu(), new[0].cpu()
    assert float(on[0]) == float(oa[0]) == float((c["td"] != 0).sum()) and float(on[6]) == N and float(on[5]) == 0 and float(on[7]) == 0
    waves = (N + 63) // 64
    for k in range(1, 5):
        noise = max(abs(float(o[k]) - float(oa[k])) for o in [ob] + more)
        diff = abs(float(on[k]) - float(oa[k]))
        print(f"MEASURED N={N} out[{k}]: plain vs plain {noise:.3e}, masked vs plain {diff:.3e}")
        if waves == 1:
            assert noise == 0 and diff == 0
        else:
            assert diff <= max(noise, waves * EPS * abs(float(oa[k])))
    # the depth-free, proposal-free form as well
    a = ops.mip_loss_tail(d["rgb"], d["tgt"], None, None, None, None, None, None, None, None, True, LAM_D, CM, LAM_P)
    new = ops.mip_loss_tail_masked(d["rgb"], d["tgt"], None, None, None, None, None, None, None, None, True, LAM_D, CM, LAM_P)
    assert torch.equal(a[1], new[1]) and all(g is None for g in new[2:])
    if waves == 1:
        assert torch.equal(a[0].cpu(), new[0].cpu()[:5])


# ---- GPU: the fused step ------------------------------------------------------------------------------------------------------------
@gpu
def test_fused_step_trains_the_semantic_head_like_autograd_on_the_device():
    """the emulated test above on the device, with the ray gradients (the semantic term reaches the rays through the weights)"""
    tr, pairs, rays = _fused_step_against_autograd("cuda", True)
    assert len(rays) == 3
    _check_step_gradients(pairs, rays)
    assert all(torch.is_tensor(v) and v.is_cuda for v in tr.last_counts) and tr.last_semantic_loss.is_cuda


# ---- GPU: the captured step ---------------------------------------------------------------------------------------------------------
CAP_SEED, CAP_STEPS, CAP_LR = 3, 3, 5e-4
CAP_CAMS = [0, 3, 1]                    # image 0: back camera (depth limit 4), image 1: side camera (RGB limit 5), image 2: no rule, no labels


def _cap_rules():
    from snerf_amd.trainer import MipLossRules
    return MipLossRules(3, H_IMG, CAP_CAMS, semantic_index=[0, 1], waymo=True, backcam=True, waymo_row_limit=5, backcam_row_limit=4)


def test_the_captured_steps_visit_images_with_different_rules():
    from snerf_amd import sample_utils as su
    imgs = [su.image_of_step(np.arange(3), CAP_SEED, s) for s in range(CAP_STEPS)]
    r = _cap_rules()
    rules = {(int(r.rgb_row_limit[i]), int(r.depth_row_limit[i]), int(r.sem_valid[i])) for i in imgs}
    assert len(rules) >= 2, (imgs, rules)


def _cap_batcher(n=64):
    from snerf_amd import sample_utils as su
    rng = np.random.default_rng(5)
    N, H, W = 3, H_IMG, 24
    images = rng.random((N, H, W, 3), dtype=np.float32)
    depths = (rng.random((N, H, W)) * 60 + 2).astype(np.float32)
    depths[rng.random((N, H, W)) < 0.4] = 0
    cams = np.zeros((N, 3, 4), np.float32)
    for i in range(N):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        cams[i, :, :3], cams[i, :, 3] = q, rng.normal(size=3)
    K = np.zeros((N, 3, 3), np.float32)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = 30.0, 30.0, W / 2, H / 2, 1
    labels = rng.integers(0, C_STEP, (N, H, W)).astype(np.float32)
    labels[rng.random((N, H, W)) < 0.2] = -100
    seg = (rng.random((N, H, W)) < 0.3).astype(np.float32)
    args = types.SimpleNamespace(no_ndc=True, smooth_loss=False, near_far=False, N_rgb=n)
    return su.ImageRayBatcher(args, images, depths, cams, K, [0, 1, 2], 2.0, 80.0, camera_index=np.asarray(CAP_CAMS, np.float64), batch_n=n,
                              extras=[labels, seg], seed=CAP_SEED, device="cuda")


@gpu
def test_captured_step_applies_the_rules_of_the_image_it_drew():
    from snerf_amd.trainer import MipTrainer
    rules = _cap_rules()

    def trainer():
        return MipTrainer(_semantic_model("cuda").set_deterministic(True), lr=CAP_LR, proposal_loss=True, semantic_lambda=LAM_S, loss_rules=rules)
    # eager: CAP_STEPS fused steps on the batcher's draws
    b, tr = _cap_batcher(), trainer()
    eager = []
    for s in range(CAP_STEPS):
        rays, trgb, tdep, sel, img, ex = b.next()
        tr.step(rays, trgb, tdep, randomized=False, img_i=img, target_semantic=ex[0], sel_coords=sel, depth_keep=ex[1])
        eager.append(tr.model.arena.flat.clone())
    # captured: the same steps as replays of one graph
    b, tr = _cap_batcher(), trainer()
    init = tr.model.arena.flat.clone()
    head = {k: v.clone() for k, v in tr.model.arena.p.items() if "semantic" in k}
    tr.capture(None, None, randomized=False, warmup=2, batcher=b, sem_extra=0, depth_keep_extra=1)
    torch.cuda.synchronize()
    assert torch.equal(tr.model.arena.flat, init) and tr.t == 0 and b.step == 0 and int(b.counter[0]) == 0          # capturing trains nothing
    seen = set()
    for s in range(CAP_STEPS):
        tr.replay()
        rays, trgb, tdep, sel, img, ex = tr.batch
        i = int(img)
        assert i == b.image_of_step(s)
        rgb_lim, dep_lim, valid = int(rules.rgb_row_limit[i]), int(rules.depth_row_limit[i]), int(rules.sem_valid[i])
        seen.add((rgb_lim, dep_lim, valid))
        rows = sel[:, 0]
        want = [int(((tdep != 0) & (rows < dep_lim) & (ex[1] == 0)).sum()), int((rows < rgb_lim).sum()),
                valid * int(((rows < rgb_lim) & (ex[0] != -100)).sum())]
        assert [int(v) for v in tr.last_counts] == want, (s, i, want)
        assert (float(tr.last_semantic_loss) > 0) == (want[2] > 0)
        # deterministic model, no random draws: the replay lands on the eager step's bits (as tests/test_optimizer_tail.py gets)
        assert torch.equal(tr.model.arena.flat, eager[s]), (s, float((tr.model.arena.flat - eager[s]).abs().max()))
    assert len(seen) >= 2 and tr.t == CAP_STEPS and b.step == CAP_STEPS
    moved = max(float((tr.model.arena.p[k] - v).abs().max()) for k, v in head.items())
    assert head and moved > 0.1 * CAP_LR                                    # the captured steps trained the semantic head
