"""The fp16 flavour of the fused 256-wide networks (csrc/fmlp.hip: fmlp_kernel<.., F16>, fchain_bwd_kernel<.., F16>): compute="fp16" runs the
classic NeRF 8 x 256 and the mip proposal MLP 4 x 256 as ONE launch per network (inference, training forward, data-gradient chain) like
compute="bf16" does.  "hip": the real kernels; "emulated": the host logic on the CPU models (tests/cpu_ops_emulation.py).
The per-layer fp16 route (`fused = False`) is the behaviour before these kernels and the partner of every comparison; the bounds are
the ones the bf16 tests of tests/test_mlp.py hold the bf16 flavour to."""
import os

import numpy as np
import pytest
import torch

import test_paths
from cpu_ops_emulation import emulate_ops
from oracle import classic as oc
from oracle import common
from oracle import mip as om

DEV = "cuda"


@pytest.fixture(params=[pytest.param("hip", marks=pytest.mark.gpu), "emulated"])
def backend(request):
    global DEV
    if request.param == "hip":
        DEV = test_paths.DEV = "cuda"
        yield "hip"
    else:
        DEV = test_paths.DEV = "cpu"
        with emulate_ops():
            yield "emulated"
    DEV = test_paths.DEV = "cuda"


def rnd_params(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    return {k: (torch.randn(s, generator=g) * (1.4 / s[1] ** 0.5) if len(s) == 2 else torch.randn(s, generator=g) * 0.1) for k, s in shapes}


def _rand_sd(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    return {k: (torch.randn(s, generator=g) * (1.4 / s[-1] ** 0.5) if len(s) == 2 else torch.randn(s, generator=g) * 0.1) for k, s in shapes}


def rel(a, b):
    a = a.detach().float().cpu(); b = b.detach().float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


def q16(t):
    return t.half().float()


class _Calls:
    """counts the launches of a block: every ops.linear_fwd (with its activation code), every ops.fmlp_* and ops.fchain_bwd"""

    def __init__(self):
        from snerf_amd import ops
        self.ops, self.linear, self.fmlp, self.chain = ops, [], [], 0
        self.names = ["linear_fwd", "fchain_bwd"] + [n for n in dir(ops) if n.startswith("fmlp_") and callable(getattr(ops, n))]

    def __enter__(self):
        self.saved = {n: getattr(self.ops, n) for n in self.names}

        def wrap(n, f):
            def g(*a, **k):
                if n == "linear_fwd":
                    self.linear.append(k["act"] if "act" in k else a[6])
                elif n == "fchain_bwd":
                    self.chain += 1
                else:
                    self.fmlp.append(n)
                return f(*a, **k)
            return g
        for n, f in self.saved.items():
            setattr(self.ops, n, wrap(n, f))
        return self

    def __exit__(self, *exc):
        for n, f in self.saved.items():
            setattr(self.ops, n, f)

    def masked(self):
        return sum(1 for a in self.linear if a in (self.ops.ACT_MASK, self.ops.ACT_MASK_BITS))


def _classic_net(dt, sd=None, seed=31):
    from snerf_amd.mlp import ClassicNeRFNet, ParamArena
    shapes = ClassicNeRFNet.param_shapes(8, 256, 63, 27, (4,))
    arena = ParamArena(shapes, torch.device(DEV))
    arena.load(sd if sd is not None else _rand_sd(shapes, seed))
    return ClassicNeRFNet(arena, "", dt, 8, 256), arena


def _proposal_net(dt, sd=None, seed=33):
    from snerf_amd.mlp import MipProposalNet, ParamArena
    shapes = MipProposalNet.param_shapes(256, 4, 96)
    arena = ParamArena(shapes, torch.device(DEV))
    arena.load(sd if sd is not None else _rand_sd(shapes, seed))
    return MipProposalNet(arena, "", dt, 256, 4, 96), arena


def _classic_inputs(M, S, seed, span=4.0):
    g = torch.Generator().manual_seed(seed)
    pts = torch.rand(M, 3, generator=g) * span - span / 2
    vd = torch.nn.functional.normalize(torch.randn(M // S, 3, generator=g), dim=-1)
    return pts, vd, g


def _prop_E(net, enc):
    from snerf_amd import ops
    E = torch.zeros(enc.shape[0], net.Ew, dtype=ops.torch_dtype(net.dt), device=DEV)
    E[:, :96] = enc.to(DEV)
    return E


# ---- 1. gate and launch count ------------------------------------------------------------------------------------------------------
def test_fp16_gate_is_open_and_each_network_is_one_launch(backend):
    """(1: gate and launch count; fails before the fp16 flavour existed.)  In ops.F16 both 256-wide networks pass fused_ok() / chain_ok();
    an inference forward makes no linear_fwd call and exactly one fmlp_* call; a training forward + backward makes one fchain_bwd call and no
    masked data-gradient GEMM.  `fused = False` gives the per-layer counts (12 / 5 GEMMs forward, 9 / 4 masked data-gradient GEMMs), and the
    gate stays closed for F16F8, BF16X3 and F32."""
    from snerf_amd import ops
    M, S = 512, 8
    pts, vd, g = _classic_inputs(M, S, 5)
    d_raw, d_den = torch.randn(M, 4, generator=g).to(DEV), torch.randn(M, 1, generator=g).to(DEV)
    enc = torch.randn(M, 96, generator=g) * 0.5
    for dt in (ops.F16F8, ops.BF16X3, ops.F32):
        assert not _classic_net(dt)[0].fused_ok() and not _classic_net(dt)[0].chain_ok()
        assert not _proposal_net(dt)[0].fused_ok() and not _proposal_net(dt)[0].chain_ok()

    net, arena = _classic_net(ops.F16)
    assert net.fused_ok() and net.chain_ok()
    with torch.no_grad(), _Calls() as c:
        net.forward(pts.to(DEV), vd.to(DEV), S, False)
    assert c.linear == [] and len(c.fmlp) == 1, (c.linear, c.fmlp)
    with _Calls() as c:
        raw, saved = net.forward(pts.to(DEV), vd.to(DEV), S, True)
        net.backward(d_raw, saved)
    assert c.chain == 1 and c.masked() == 0 and len(c.fmlp) == 1, (c.chain, c.masked(), c.fmlp)
    net.fused = False
    with torch.no_grad(), _Calls() as c:
        net.forward(pts.to(DEV), vd.to(DEV), S, False)
    assert len(c.linear) == 12 and c.fmlp == []
    with _Calls() as c:
        raw, saved = net.forward(pts.to(DEV), vd.to(DEV), S, True)
        net.backward(d_raw, saved)
    assert c.chain == 0 and c.masked() == 9 and c.fmlp == [], (c.chain, c.masked(), c.fmlp)
    net.fused, net.deterministic = True, True                    # the deterministic mode keeps the per-layer data gradients
    assert net.fused_ok() and not net.chain_ok()

    prop, arena = _proposal_net(ops.F16)
    assert prop.fused_ok() and prop.chain_ok()
    E = _prop_E(prop, enc)
    with torch.no_grad(), _Calls() as c:
        prop.forward(E, False)
    assert c.linear == [] and c.fmlp == ["fmlp_proposal_fwd"], (c.linear, c.fmlp)
    with _Calls() as c:
        out, acts = prop.forward(E, True)
        prop.backward(d_den, acts)
    assert c.chain == 1 and c.masked() == 0 and c.fmlp == ["fmlp_proposal_train_fwd"], (c.chain, c.masked(), c.fmlp)
    prop.fused = False
    with torch.no_grad(), _Calls() as c:
        prop.forward(E, False)
    assert len(c.linear) == 5 and c.fmlp == []
    with _Calls() as c:
        out, acts = prop.forward(E, True)
        prop.backward(d_den, acts)
    assert c.chain == 0 and c.masked() == 4 and c.fmlp == []
    prop.fused, prop.fused_chain = True, False
    assert prop.fused_ok() and not prop.chain_ok()


# ---- 2. forward against the per-layer route and the fp32 oracle ----------------------------------------------------------------------
@pytest.mark.parametrize("M", [700, 1024])
def test_fp16_fused_forward_matches_per_layer_route_and_oracle(backend, M):
    """(2: forward.)  The fused fp16 launch of both networks against the fp32 oracle (reference) and the per-layer fp16 route (partner), on
    the inputs of the bf16 tests of tests/test_mlp.py: err_fused < 2 err_layered + 1e-3 (max error / max |ref|) and fused vs per-layer rel L2
    < 5e-3.  M = 700: ragged last tile."""
    from snerf_amd import classic, ops
    sd = _rand_sd(oc.nerf_param_shapes(W=256), 31)
    net = classic.NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=4, skips=[4], use_viewdirs=True, compute="fp16", device=DEV)
    net.load_state_dict(sd)
    assert net.net.fused_ok() and net.net.dt == ops.F16
    g = torch.Generator().manual_seed(32)
    S = 4
    pts = (torch.rand(M // S, S, 3, generator=g) * 4 - 2)
    vd = torch.nn.functional.normalize(torch.randn(M // S, 3, generator=g), dim=-1)
    e, ev = classic.get_embedder(10, 0)[0], classic.get_embedder(4, 0)[0]
    with torch.no_grad():
        fused = classic.run_network(pts.to(DEV), vd.to(DEV), net, e, ev).cpu()
        net.net.fused = False
        layered = classic.run_network(pts.to(DEV), vd.to(DEV), net, e, ev).cpu()
        net.net.fused = True
    ref = oc.run_network(pts, vd, sd)
    scale = float(ref.abs().max())
    err_f, err_l = float((fused - ref).abs().max()) / scale, float((layered - ref).abs().max()) / scale
    r = float((fused - layered).norm() / layered.norm())
    print(f"MEASURED fp16 fused classic MLP vs fp32 oracle (M {M}): fused {err_f:.3e}, per-layer {err_l:.3e}; fused vs per-layer rel L2 {r:.3e}")
    assert err_f < 2.0 * err_l + 1e-3
    assert r < 5e-3

    sd_p = _rand_sd(_proposal_net(ops.F16)[0].param_shapes(256, 4, 96), 33)
    prop, _ = _proposal_net(ops.F16, sd_p)
    g = torch.Generator().manual_seed(34)
    E = _prop_E(prop, torch.randn(M, 96, generator=g) * 0.5)
    assert E.dtype == torch.float16
    with torch.no_grad():
        fused, _ = prop.forward(E, False)
        prop.fused = False
        layered, _ = prop.forward(E, False)
    ref = om.proposal_mlp({"proposal." + k: v for k, v in sd_p.items()}, E[:, :96].float().cpu()[None]).reshape(-1)
    scale = float(ref.abs().max())
    err_f = float((fused.cpu().reshape(-1) - ref).abs().max()) / scale
    err_l = float((layered.cpu().reshape(-1) - ref).abs().max()) / scale
    r = float((fused - layered).norm() / layered.norm())
    print(f"MEASURED fp16 fused proposal MLP vs fp32 oracle (M {M}): fused {err_f:.3e}, per-layer {err_l:.3e}; fused vs per-layer rel L2 {r:.3e}")
    assert err_f < 2.0 * err_l + 1e-3
    assert r < 5e-3


def test_fp16_fused_forward_is_fp16_arithmetic_not_bf16(backend):
    """(2: the differential assertion.)  Same weights, same fp32 inputs (those of test_fused_gradient_chains_*, M = 1000): the fused fp16
    network's rel L2 error against the fp32 oracle is at most HALF the fused bf16 network's -- three more mantissa bits make it about 1/8; a
    launch that ran the bf16 kernel on fp16 bit patterns, or rounded through bf16 anywhere, could not get there."""
    from snerf_amd import ops
    from snerf_amd.mlp import ClassicNeRFNet, MipProposalNet
    M, S = 1000, 8
    g = torch.Generator().manual_seed(61)
    sd = rnd_params(ClassicNeRFNet.param_shapes(8, 256, 63, 27, (4,)), 62)
    pts = torch.rand(M, 3, generator=g) * 2 - 1
    vd = torch.nn.functional.normalize(torch.randn(M // S, 3, generator=g), dim=-1)
    ref = oc.nerf_mlp(sd, torch.cat([oc.embed(pts, 10), oc.embed(vd[:, None].expand(M // S, S, 3).reshape(M, 3), 4)], -1))
    errs = {}
    for dt in (ops.F16, ops.BF16):
        net, _ = _classic_net(dt, sd)
        assert net.fused_ok()
        with torch.no_grad(), _Calls() as c:
            raw, _ = net.forward(pts.to(DEV), vd.to(DEV), S, False)
        assert c.linear == [] and len(c.fmlp) == 1
        errs[dt] = rel(raw, ref)
    print(f"MEASURED classic fused vs fp32 oracle, rel L2: fp16 {errs[ops.F16]:.3e}, bf16 {errs[ops.BF16]:.3e}, ratio {errs[ops.F16] / errs[ops.BF16]:.3f}")
    assert errs[ops.F16] <= 0.5 * errs[ops.BF16]

    sd_p = rnd_params(MipProposalNet.param_shapes(256, 4, 96), 63)
    enc = torch.rand(M, 96, generator=g) * 2 - 1
    ref = om.proposal_mlp({"proposal." + k: v for k, v in sd_p.items()}, enc[None]).reshape(-1)
    for dt in (ops.F16, ops.BF16):
        prop, _ = _proposal_net(dt, sd_p)
        with torch.no_grad():
            out, _ = prop.forward(_prop_E(prop, enc), False)
        errs[dt] = rel(out.reshape(-1), ref)
    print(f"MEASURED proposal fused vs fp32 oracle, rel L2: fp16 {errs[ops.F16]:.3e}, bf16 {errs[ops.BF16]:.3e}, ratio {errs[ops.F16] / errs[ops.BF16]:.3f}")
    assert errs[ops.F16] <= 0.5 * errs[ops.BF16]


# ---- 3. bit-exact properties -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1000, 768])
def test_fp16_inference_launch_reproduces_training_launch_and_stored_activations(backend, M):
    """(3a, 3d.)  The inference launch (no stores) gives the `raw` of the training launch bit for bit -- classic network behind the
    embedding kernel (`fused_embed = False`: the same fp16 operand rows) and proposal MLP; the stored activations are torch.float16 and agree
    with the per-layer route's to 1e-2 rel L2."""
    from snerf_amd import ops
    S = 8
    pts, vd, g = _classic_inputs(M, S, 42)
    net, _ = _classic_net(ops.F16, seed=41)
    net.fused_embed = False
    with torch.no_grad():
        raw_i, _ = net.forward(pts.to(DEV), vd.to(DEV), S, False)
        raw_t, saved = net.forward(pts.to(DEV), vd.to(DEV), S, True)
        assert torch.equal(raw_i, raw_t), "inference launch (no stores) must reproduce the training launch"
        net.fused = False
        raw_l, saved_l = net.forward(pts.to(DEV), vd.to(DEV), S, True)
    worst = 0.0
    for (x, k, y), (_, _, yl) in zip(saved[0], saved_l[0]):
        assert y.dtype == torch.float16 and yl.dtype == torch.float16
        worst = max(worst, rel(y, yl))
    assert saved[1].dtype == torch.float16 and saved[2].dtype == torch.float16
    worst = max(worst, rel(saved[1], saved_l[1]), rel(saved[2], saved_l[2]))
    print(f"MEASURED fp16 classic stored activations, fused vs per-layer (M {M}): worst rel L2 {worst:.3e}; raw {rel(raw_t, raw_l):.3e}")
    assert worst < 1e-2 and rel(raw_t, raw_l) < 5e-3

    prop, _ = _proposal_net(ops.F16, seed=43)
    E = _prop_E(prop, torch.randn(M, 96, generator=g) * 0.5)
    with torch.no_grad():
        out_i, _ = prop.forward(E, False)
        out_t, acts = prop.forward(E, True)
        assert torch.equal(out_i, out_t)
        prop.fused = False
        out_l, acts_l = prop.forward(E, True)
    worst = 0.0
    for (x, k, y), (_, _, yl) in zip(acts, acts_l):
        assert y.dtype == torch.float16
        worst = max(worst, rel(y, yl))
    print(f"MEASURED fp16 proposal stored activations, fused vs per-layer (M {M}): worst rel L2 {worst:.3e}; raw {rel(out_t, out_l):.3e}")
    assert worst < 1e-2 and rel(out_t, out_l) < 5e-3


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1000, 768])
def test_fp16_x_flavour_equals_cast_pad_plus_rows_flavour_bit_for_bit(M):
    """(3b.)  snerf_fmlp_classic_x_fwd_dt on fp32 rows == snerf_cast_pad(.., F16) into E / VE followed by the rows flavour, bit for bit
    (the in-register conversion is the round-to-nearest-even one cast_pad applies; values beyond fp16's range and on rounding ties are
    among the inputs); the training launch's xin copies are the cast_pad outputs; its raw is the inference launch's."""
    from snerf_amd import ops
    net, _ = _classic_net(ops.F16, seed=41)
    net._fused_ready()
    g = torch.Generator().manual_seed(44)
    x = (torch.rand(M, 90, generator=g) * 2 - 1)
    x[::7, 5] = 1.0 + 2.0 ** -11                                  # a tie between two fp16 neighbours (-> even)
    x[::11, 70] = 1.0 + 3 * 2.0 ** -11                            # the other tie (-> up)
    x[3, 10], x[4, 80] = 1e-6, -3e-8                              # fp16 subnormal / below half the smallest subnormal
    wide = torch.zeros(M, 96)
    wide[:, 3:93] = x
    xd = wide.to(DEV)[:, 3:93]                                    # a column slice of a wider tensor: 4-byte aligned rows only
    E, VE = torch.zeros(M, 64, dtype=torch.float16, device=DEV), torch.zeros(M, 32, dtype=torch.float16, device=DEV)
    ops.cast_pad(xd[:, :63], 63, E, 64, ops.F16)
    ops.cast_pad(xd[:, 63:90], 27, VE, 32, ops.F16)
    raw_x, raw_r = torch.empty(M, 4, device=DEV), torch.empty(M, 4, device=DEV)
    ops.fmlp_classic_x_fwd(xd, net.fstream, net.fbias, raw_x)
    ops.fmlp_classic_fwd(E, VE, net.fstream, net.fbias, raw_r)
    assert torch.equal(raw_x, raw_r)
    with torch.no_grad():
        raw_t, saved = net.forward_embedded(xd, True)
    acts, V, HV, SK, Eb = saved[:5]
    assert torch.equal(raw_t, raw_x)
    assert Eb.dtype == torch.float16 and torch.equal(Eb[:, :64], E) and torch.equal(SK[:, :64], E) and torch.equal(V[:, 256:288], VE)


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1000, 768])
def test_fp16_relu_bit_masks_are_exactly_the_sign_of_the_stored_activations(M):
    """(3c.)  Every ReLU bit mask the fp16 training launches write -- decoded from the documented layout as
    test_fused_training_forward_stores_activations_and_relu_bits does -- is exactly y > 0 of the fp16 activation the same launch stored."""
    from snerf_amd import ops

    def decode(words, Mr, N):
        w = words.cpu().numpy().view("uint8").reshape(-1, N // 64, 64, 4)                     # [rb, cg, word, byte]
        bits = ((w[..., None] >> np.arange(8, dtype="uint8")) & 1).astype(bool)               # [rb, cg, word, byte, e]
        rb, cg, ln, it, e = np.meshgrid(*[np.arange(n) for n in bits.shape], indexing="ij")
        out = np.zeros((bits.shape[0] * 32, N), bool)
        out[rb * 32 + 8 * it + (ln >> 3), cg * 64 + 8 * (ln & 7) + e] = bits
        return out[:Mr]
    S = 8
    pts, vd, g = _classic_inputs(M, S, 42)
    net, _ = _classic_net(ops.F16, seed=41)
    raw, saved = net.forward(pts.to(DEV), vd.to(DEV), S, True)
    assert len(net._bits) == 8
    for (x, k, y) in saved[0]:
        words, N = net._bits[(y.data_ptr(), M)]
        assert y.dtype == torch.float16 and np.array_equal(decode(words, M, N), (y.float() > 0).cpu().numpy())
    assert np.array_equal(decode(saved[5][8], M, 128), (saved[2].float() > 0).cpu().numpy())      # views_linears.0 (2 column groups)
    prop, _ = _proposal_net(ops.F16, seed=43)
    out, acts = prop.forward(_prop_E(prop, torch.randn(M, 96, generator=g) * 0.5), True)
    for (x, k, y) in acts:
        words, N = prop._bits[(y.data_ptr(), M)]
        assert y.dtype == torch.float16 and np.array_equal(decode(words, M, N), (y.float() > 0).cpu().numpy())


# ---- 4. gradients ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1000, 768])
def test_fp16_fused_gradient_chains_match_per_layer_kernels_and_oracle(backend, M):
    """(4: gradients.)  Every parameter gradient of both networks through backward() (the scaled fp16 backward) and the proposal network's
    input gradient: the fused chain against torch autograd of the oracle and against `fused_chain = False`, with the bounds of
    test_fused_gradient_chains_match_per_layer_kernels_and_oracle as they stand (e_c < 0.25, e_c < 2 e_l + 2e-2, chain vs per-layer < 3e-2)."""
    from snerf_amd import ops
    from snerf_amd.mlp import ClassicNeRFNet, MipProposalNet
    g = torch.Generator().manual_seed(61)
    S = 8
    shapes = ClassicNeRFNet.param_shapes(8, 256, 63, 27, (4,))
    sd = rnd_params(shapes, 62)
    pts = torch.rand(M, 3, generator=g) * 2 - 1
    vd = torch.nn.functional.normalize(torch.randn(M // S, 3, generator=g), dim=-1)
    d_raw = torch.randn(M, 4, generator=g)
    pr = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    e = torch.cat([q16(oc.embed(pts, 10)), q16(oc.embed(vd[:, None].expand(M // S, S, 3).reshape(M, 3), 4))], -1)
    (oc.nerf_mlp(pr, e) * d_raw).sum().backward()

    def run_classic(chain):
        net, arena = _classic_net(ops.F16, sd)
        net.fused_chain = chain
        assert net.fused_ok() and net.chain_ok() == chain
        with _Calls() as c:
            raw, saved = net.forward(pts.to(DEV), vd.to(DEV), S, True)
            arena.grad.zero_()
            net.backward(d_raw.to(DEV), saved)
        assert c.chain == (1 if chain else 0)
        return {k: arena.g[k].clone() for k in sd}
    g_c, g_l = run_classic(True), run_classic(False)
    worst = [0.0, 0.0, 0.0]
    for k in sd:
        e_c, e_l, e_cl = rel(g_c[k], pr[k].grad), rel(g_l[k], pr[k].grad), rel(g_c[k], g_l[k])
        worst = [max(worst[0], e_c), max(worst[1], e_l), max(worst[2], e_cl)]
    print(f"MEASURED fp16 classic gradients (M {M}), worst rel L2: chain vs autograd {worst[0]:.3e}, per-layer vs autograd {worst[1]:.3e}, "
          f"chain vs per-layer {worst[2]:.3e}")
    for k in sd:
        e_c, e_l = rel(g_c[k], pr[k].grad), rel(g_l[k], pr[k].grad)
        assert torch.isfinite(g_c[k]).all()
        assert e_c < 0.25 and e_c < 2.0 * e_l + 2e-2, (k, e_c, e_l)
        assert rel(g_c[k], g_l[k]) < 3e-2, (k, rel(g_c[k], g_l[k]))

    shapes_p = MipProposalNet.param_shapes(256, 4, 96)
    sd_p = rnd_params(shapes_p, 63)
    enc = q16(torch.rand(M, 96, generator=g) * 2 - 1)
    d_den = torch.randn(M, 1, generator=g)
    pp = {"proposal." + k: v.clone().requires_grad_(True) for k, v in sd_p.items()}
    (om.proposal_mlp(pp, enc[:, None]).reshape(M, 1) * d_den).sum().backward()

    def run_prop(chain):
        net, arena = _proposal_net(ops.F16, sd_p)
        net.fused_chain = chain
        assert net.fused_ok() and net.chain_ok() == chain
        out, acts = net.forward(_prop_E(net, enc), True)
        arena.grad.zero_()
        ig = net.backward(d_den.to(DEV), acts, want_input_grad=True)
        return {k: arena.g[k].clone() for k in sd_p}, ig
    (g_c, ig_c), (g_l, ig_l) = run_prop(True), run_prop(False)
    worst = [0.0, 0.0, 0.0]
    for k in sd_p:
        e_c, e_l, e_cl = rel(g_c[k], pp["proposal." + k].grad), rel(g_l[k], pp["proposal." + k].grad), rel(g_c[k], g_l[k])
        worst = [max(worst[0], e_c), max(worst[1], e_l), max(worst[2], e_cl)]
    print(f"MEASURED fp16 proposal gradients (M {M}), worst rel L2: chain vs autograd {worst[0]:.3e}, per-layer vs autograd {worst[1]:.3e}, "
          f"chain vs per-layer {worst[2]:.3e}; input gradient chain vs per-layer {rel(ig_c, ig_l):.3e}")
    assert rel(ig_c, ig_l) < 3e-2, rel(ig_c, ig_l)
    for k in sd_p:
        e_c, e_l = rel(g_c[k], pp["proposal." + k].grad), rel(g_l[k], pp["proposal." + k].grad)
        assert e_c < 0.25 and e_c < 2.0 * e_l + 2e-2, (k, e_c, e_l)
        assert rel(g_c[k], g_l[k]) < 3e-2, (k, rel(g_c[k], g_l[k]))


# ---- 5. in-kernel embedding ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1000, 768])
def test_fp16_in_kernel_embedding_matches_embedding_kernel(backend, M):
    """(5: in-kernel embedding.)  `fused_embed = True` (positional encodings computed in the fused launch, rounded to fp16) against `False`
    (the bit-exact embedding kernel writing fp16 rows): rel L2 below the bf16 test's 3e-3 -- only features that land on the other side of an
    fp16 rounding boundary differ."""
    from snerf_amd import ops
    S = 8
    pts, vd, g = _classic_inputs(M, S, 32)
    net, _ = _classic_net(ops.F16, seed=31)
    with torch.no_grad():
        with _Calls() as c:
            a, _ = net.forward(pts.to(DEV), vd.to(DEV), S, False)
        assert c.fmlp == ["fmlp_classic_pts_fwd"]
        net.fused_embed = False
        with _Calls() as c:
            b, _ = net.forward(pts.to(DEV), vd.to(DEV), S, False)
        assert c.fmlp == ["fmlp_classic_fwd"]
    r = rel(a, b)
    print(f"MEASURED fp16 in-kernel embedding vs embedding kernel (M {M}): rel L2 {r:.3e}")
    assert r < 3e-3


# ---- 6. public interface -----------------------------------------------------------------------------------------------------------------
def test_fp16_classic_render_rays_vs_oracle_on_the_fused_route(backend):
    """(6: public interface, path B.)  classic.NeRF(compute="fp16"), D = 8, W = 256, through run_network / render_rays against oracle.classic:
    the body and the tolerance (3e-2) of the ("bf16", 256, 3e-2) row of test_classic_render_rays_vs_oracle, and every network evaluation of
    it is one fused launch."""
    with _Calls() as c:
        test_paths.test_classic_render_rays_vs_oracle(backend, "fp16", 256, 3e-2)
    assert c.linear == [] and len(c.fmlp) >= 2 and set(c.fmlp) <= {"fmlp_classic_pts_fwd"}, (len(c.linear), c.fmlp)


def test_fp16_mipnerf_forward_vs_oracle_on_the_fused_route(backend):
    """(6: public interface, path A.)  MipNerfModel(compute="fp16", hidden_layer=1024) forward against the oracle at the existing fp16 row's
    1e-2 (the body of test_mipnerf_forward_vs_oracle); its proposal network is one fused launch."""
    with _Calls() as c:
        test_paths.test_mipnerf_forward_vs_oracle(backend, "fp16", 1024, 64, 129, 96, 1e-2)
    assert c.fmlp == ["fmlp_proposal_fwd"], c.fmlp


def test_fp16_trainer_step_on_the_fused_route_matches_the_per_layer_route(backend):
    """(6: public interface, training.)  One MipTrainer.step in fp16 (proposal MLP 4 x 256 fused: training forward + gradient chain): the
    gradient the optimiser receives is finite and equals the `fused = False` step's within the gradient bound of (4) (rel L2 < 3e-2 per
    parameter), and the parameters it leaves are finite and within one Adam step (2 lr: a sign flip of a near-zero gradient) of that run's."""
    from snerf_amd import mipnerf, ops
    from snerf_amd.trainer import MipTrainer
    S0, P1, n, hidden, lr = 24, 25, 64, 128, 5e-4
    sd = test_paths.random_params(om.mipnerf_param_shapes(hidden=hidden, prop_hidden=256), 21, ("mlp.density_layer.bias", "proposal.density_layer.bias"))
    rays_c = common.synthetic_rays(n, seed=7)
    gg = torch.Generator().manual_seed(8)
    target, tdepth = torch.rand(n, 3, generator=gg), torch.rand(n, generator=gg) * 50 + 5

    def run(fused):
        m = test_paths.make_mip(hidden, 256, S0, P1, "fp16", sd)
        m.prop.fused = fused
        assert m.prop.fused_ok() == fused and m.prop.chain_ok() == fused
        tr = MipTrainer(m, lr=lr, proposal_loss=True)
        grads = []
        real = ops.adam_step

        def spy(p, g, *a, **k):
            grads.append(g.clone())
            return real(p, g, *a, **k)
        ops.adam_step = spy
        try:
            with _Calls() as c:
                tr.step(mipnerf.Rays(**{k: v.to(DEV) for k, v in rays_c.items()}), target.to(DEV), tdepth.to(DEV), None, randomized=False)
        finally:
            ops.adam_step = real
        assert c.chain == (1 if fused else 0) and (c.fmlp == ["fmlp_proposal_train_fwd"]) == fused, (c.chain, c.fmlp)
        assert len(grads) == 1
        return m, grads[0]
    (m_f, g_f), (m_l, g_l) = run(True), run(False)
    assert torch.isfinite(m_f.arena.flat).all() and torch.isfinite(g_f).all()
    worst = 0.0
    for name, (o, cnt) in m_f.arena._offs.items():
        r = rel(g_f[o:o + cnt], g_l[o:o + cnt])
        worst = max(worst, r)
        assert r < 3e-2, (name, r)
    print(f"MEASURED fp16 trainer step, fused vs per-layer proposal network: worst per-parameter gradient rel L2 {worst:.3e}")
    assert float((m_f.arena.flat - m_l.arena.flat).abs().max()) <= 2 * lr + 1e-7


# ---- 7. argument checks without a GPU ---------------------------------------------------------------------------------------------------------
def test_fp16_dt_entries_reject_bad_arguments_without_a_gpu():
    """(7: argument checks.)  Every `_dt` entry returns "bad argument" for dtype SNERF_DT_F32 and for a misaligned pointer, before anything
    touches a device; the entries without the suffix keep their argument lists (an empty batch is accepted, a misaligned pointer is not)."""
    import ctypes
    from snerf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    assert _lib.load().snerf_version() >= 2
    F32, BF16, F16 = 0, 1, 2
    buf = (ctypes.c_char * 4096)()
    A = (ctypes.addressof(buf) + 15) & ~15                        # a 16-byte aligned host address: never dereferenced by the checks
    arr = (ctypes.c_void_p * 10)(*([A] * 10))
    lds = (ctypes.c_long * 10)(*([256] * 10))
    pa, pl = ctypes.addressof(arr), ctypes.addressof(lds)
    entries = {
        # name -> (arguments in front of dtype with a hole `P` for the pointer to misalign)
        "snerf_fmlp_classic_fwd": lambda P, M: (A, 64, P, 32, A, 1184, A, 78, A, M),
        "snerf_fmlp_classic_train_fwd": lambda P, M: (A, 64, P, 32, A, 1184, A, 78, A, pa, pl, pa, M),
        "snerf_fmlp_classic_pts_fwd": lambda P, M: (A, A, 3, 8, A, 1184, A, 78, P, M),
        "snerf_fmlp_classic_x_fwd": lambda P, M: (A, 90, A, 1184, A, 78, P, M),
        "snerf_fmlp_classic_x_train_fwd": lambda P, M: (A, 90, A, 1184, A, 78, P, pa, pl, pa, pl, pa, M),
        "snerf_fmlp_proposal_fwd": lambda P, M: (P, 96, P, 448, A, 33, A, M),
        "snerf_fmlp_proposal_train_fwd": lambda P, M: (P, 96, P, 448, A, 33, A, pa, pl, pa, M),
        "snerf_fchain_bwd": lambda P, M: (1, A, P, 400, pa, pa, pl, pa, A, 1 << 20, M),
    }
    for name, args in entries.items():
        for dt in (BF16, F16):
            with pytest.raises(_lib.SnerfHipError, match="bad argument"):
                _lib.call(name + "_dt", *args(A + 4, 256), dt, None)        # misaligned pointer
        with pytest.raises(_lib.SnerfHipError, match="bad argument"):
            _lib.call(name + "_dt", *args(A, 256), F32, None)               # a dtype the fused kernels do not have
        with pytest.raises(_lib.SnerfHipError, match="bad argument"):
            _lib.call(name + "_dt", *args(A, 0), F32, None)                 # ... refused even for an empty batch
        with pytest.raises(_lib.SnerfHipError, match="bad argument"):
            _lib.call(name + "_dt", *args(A, 256), 5, None)                 # SNERF_DT_F16F8
        assert _lib.call(name + "_dt", *args(A, 0), F16, None) is None      # an empty batch is not an error
        assert _lib.call(name, *args(A, 0), None) is None                   # the old entry, its old argument list
        with pytest.raises(_lib.SnerfHipError, match="bad argument"):
            _lib.call(name, *args(A + 4, 256), None)


# ---- 8. determinism ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_fp16_fused_training_forward_and_chains_are_bit_reproducible():
    """(8: determinism; the chain block of tests/test_determinism.py in fp16.)  200 repeats of the fp16 training forward and of the fp16
    gradient chains, with a vendor GEMM and other LDS content in between, store bit-identical raw, activations, masks and dz; the chains'
    bias gradients (LDS atomics in arrival order) stay within 1e-5 relative."""
    from snerf_amd import ops
    from test_determinism import _repeat
    torch.manual_seed(2)
    dev = torch.device("cuda")
    big = torch.randn(2048, 2048, device="cuda").bfloat16()
    for kind in ("classic", "proposal"):
        M = 3000
        if kind == "classic":
            nn_, ar = _classic_net(ops.F16, seed=71)
            pts = torch.rand(M, 3, device=dev) * 2 - 1
            vd = torch.nn.functional.normalize(torch.randn(M // 8, 3, device=dev), dim=-1)

            def train_fwd():
                raw, saved = nn_.forward(pts, vd, 8, True)
                return [raw] + [y for _, _, y in saved[0]] + [saved[1], saved[2]] + list(saved[5])
            raw, saved = nn_.forward(pts, vd, 8, True)
            d_raw = torch.randn(M, 4, device=dev)
            widths, bits, net_id = [128] + [256] * 9, saved[5], ops.CHAIN_CLASSIC
        else:
            nn_, ar = _proposal_net(ops.F16, seed=72)
            E = torch.zeros(M, nn_.Ew, dtype=torch.float16, device=dev)
            E[:, :96] = (torch.rand(M, 96, device=dev) * 2 - 1).half()

            def train_fwd():
                out, acts = nn_.forward(E, True)
                return [out] + [y for _, _, y in acts] + list(nn_._chain_bits[1])
            out, acts = nn_.forward(E, True)
            d_raw = torch.randn(M, 1, device=dev)
            widths, bits, net_id = [256] * 4, nn_._chain_bits[1], ops.CHAIN_PROPOSAL
        stream = nn_._chain_stream()
        assert stream.dtype == torch.float16
        gb0 = None

        def chain():
            dz = [torch.empty(M, w, dtype=torch.float16, device=dev) for w in widths]
            gb = [torch.zeros(w, device=dev) for w in widths]
            ops.fchain_bwd(net_id, d_raw, stream, bits, dz, gb)
            nonlocal gb0
            if gb0 is None:
                gb0 = [g.clone() for g in gb]
            for g, g0 in zip(gb, gb0):                             # bias gradients: same sums, arrival order of the LDS atomics varies
                assert float((g - g0).abs().max()) <= 1e-5 * float(g0.abs().max()) + 1e-12
            return dz
        assert _repeat(chain, 200, big) == 0, kind
        with torch.no_grad():
            assert _repeat(train_fwd, 200, big) == 0, kind
