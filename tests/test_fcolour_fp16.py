"""The fp16 flavour of the fused colour head (csrc/fmlp.hip: fcolour_fwd_kernel<.., F16>, fcolour_bwd_kernel<F16>): compute="fp16" runs
cat([bottleneck 1024, view encoding 27]) -> 128 -> 128 -> 128 -> 3 of the mip path's NeRF MLP as ONE launch each way, like compute="bf16".
"hip": the real kernels; "emulated": the host logic on the CPU models (tests/cpu_ops_emulation.py).
The per-layer fp16 route (`fused_colour = False`) is the behaviour before these kernels and the partner of every comparison; the bounds are
the ones tests/test_mlp.py::test_fused_colour_head_matches_per_layer_kernels_and_oracle holds the bf16 flavour to, on its inputs and seeds."""
import os

import numpy as np
import pytest
import torch

import test_paths
from cpu_ops_emulation import emulate_ops
from oracle import common
from oracle import mip as om

DEV = "cuda"
H = 1024
COLOUR_KEYS = {"cond_layers.0.layers.0", "cond_layers.1.layers.0", "cond_layers.2.layers.0", "rgb"}


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


def rel(a, b):
    a = a.detach().float().cpu(); b = b.detach().float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


def q16(t):
    return t.half().float()


def _shapes():
    from snerf_amd.mlp import MipNerfNet
    return [("mlp." + n, s) for n, s in MipNerfNet.param_shapes(H, 8, 4, 96, 27, 3, 128)]


def _net(dt, sd, fused=True):
    from snerf_amd.mlp import MipNerfNet, ParamArena
    arena = ParamArena(_shapes(), torch.device(DEV))
    arena.load(sd)
    net = MipNerfNet(arena, "mlp.", dt, H)
    net.fused_colour = fused
    return net, arena


def _inputs(net, enc, cond):
    M = enc.shape[0]
    SKIP, CB = net.alloc_inputs(M)
    SKIP[:, H:] = 0; CB[:, H:] = 0
    SKIP[:, H:H + 96] = enc.to(DEV, net.tdt)
    CB[:, H:H + 27] = cond.to(DEV, net.tdt)
    return SKIP, CB


def _case(M):
    """inputs and seeds of test_fused_colour_head_matches_per_layer_kernels_and_oracle, the encodings on fp16's grid instead of bf16's"""
    sd = rnd_params(_shapes(), 51)
    g = torch.Generator().manual_seed(52)
    enc = q16(torch.rand(M, 96, generator=g) * 2 - 1)
    cond = q16(torch.rand(M, 27, generator=g) * 2 - 1)
    d_rgb, d_den = torch.randn(M, 3, generator=g), torch.randn(M, 1, generator=g)
    return sd, enc, cond, d_rgb, d_den


class _Calls:
    """counts the launches of a block: ops.fcolour_fwd / ops.fcolour_bwd, and -- for the networks handed in -- every per-layer forward
    GEMM (`fwd`) and data-gradient GEMM (`dgrad`) by the key of its packed weights"""

    def __init__(self, *nets):
        from snerf_amd import ops
        self.ops, self.nets, self.cf, self.cb, self.fwd, self.dgrad = ops, nets, 0, 0, [], []

    def __enter__(self):
        self.saved = (self.ops.fcolour_fwd, self.ops.fcolour_bwd)
        f0, b0 = self.saved

        def f(*a, **k):
            self.cf += 1
            return f0(*a, **k)

        def b(*a, **k):
            self.cb += 1
            return b0(*a, **k)
        self.ops.fcolour_fwd, self.ops.fcolour_bwd = f, b
        for net in self.nets:
            fw, dg = net.fwd, net.dgrad

            def fwd(key, *a, _fw=fw, **k):
                self.fwd.append(key)
                return _fw(key, *a, **k)

            def dgrad(key, *a, _dg=dg, **k):
                self.dgrad.append((key, k.get("mask") is not None))
                return _dg(key, *a, **k)
            net.fwd, net.dgrad = fwd, dgrad
        return self

    def __exit__(self, *exc):
        self.ops.fcolour_fwd, self.ops.fcolour_bwd = self.saved
        for net in self.nets:
            del net.fwd, net.dgrad

    def colour_fwd(self):
        return [k for k in self.fwd if k in COLOUR_KEYS]

    def colour_dgrad(self):
        return [k for k, masked in self.dgrad if k in COLOUR_KEYS and masked]


# ---- 1. gate and launch count ------------------------------------------------------------------------------------------------------
def test_fp16_colour_gate_is_open_and_the_head_is_one_launch_each_way(backend):
    """(1: gate and launch count; fails before the fp16 flavour existed.)  In ops.F16 colour_fused_ok() is true; an inference forward makes
    exactly one fcolour_fwd call and no per-layer GEMM for cond_layers.* / rgb; a training forward + backward makes one fcolour_fwd, one
    fcolour_bwd and no masked data-gradient GEMM for the colour head.  `fused_colour = False`: 4 + 4 per-layer launches and no fcolour_*
    call.  The gate is closed for F16F8, BF16X3, F32, and inside a plain backward."""
    from snerf_amd import ops
    M = 700
    sd, enc, cond, d_rgb, d_den = _case(M)
    for dt in (ops.F16F8, ops.BF16X3, ops.F32):
        assert not _net(dt, sd)[0].colour_fused_ok()
    net, arena = _net(ops.F16, sd)
    assert net.colour_fused_ok()
    net._in_plain_bwd = True
    assert not net.colour_fused_ok()
    net._in_plain_bwd = False
    SKIP, CB = _inputs(net, enc, cond)
    with torch.no_grad(), _Calls(net) as c:
        net.forward(SKIP.clone(), CB.clone(), False)
    assert c.cf == 1 and c.cb == 0 and c.colour_fwd() == [], (c.cf, c.cb, c.fwd)
    with _Calls(net) as c:
        raw_rgb, raw_d, saved = net.forward(SKIP, CB, True)
        arena.grad.zero_()
        net.backward(d_rgb.to(DEV), d_den.to(DEV), saved)
    assert saved[1][-1][0] == "fused"
    assert c.cf == 1 and c.cb == 1 and c.colour_fwd() == [] and c.colour_dgrad() == [], (c.cf, c.cb, c.fwd, c.dgrad)

    net, arena = _net(ops.F16, sd, fused=False)
    assert not net.colour_fused_ok()
    SKIP, CB = _inputs(net, enc, cond)
    with torch.no_grad(), _Calls(net) as c:
        net.forward(SKIP.clone(), CB.clone(), False)
    assert c.cf == 0 and len(c.colour_fwd()) == 4, (c.cf, c.fwd)
    with _Calls(net) as c:
        raw_rgb, raw_d, saved = net.forward(SKIP, CB, True)
        arena.grad.zero_()
        net.backward(d_rgb.to(DEV), d_den.to(DEV), saved)
    assert len(saved[1]) == 3
    assert c.cf == 0 and c.cb == 0 and len(c.colour_fwd()) == 4 and len(c.colour_dgrad()) == 4, (c.cf, c.cb, c.fwd, c.dgrad)
    print(f"MEASURED fp16 colour head launches: fused 1 forward + 1 backward; per-layer {len(c.colour_fwd())} + {len(c.colour_dgrad())}")


# ---- 2. forward against the per-layer route and the fp32 oracle ----------------------------------------------------------------------
@pytest.mark.parametrize("M", [700, 1024])
def test_fp16_fused_colour_forward_matches_per_layer_route_and_oracle(backend, M):
    """(2: forward.)  raw_rgb of the fused fp16 launch against the fp32 oracle (om.nerf_mlp) and the per-layer fp16 route: err_fused <
    2 err_layered + 1e-3 (max error / max |ref|), fused vs per-layer rel L2 < 5e-3; the stored activations are torch.float16 and within 1e-2
    rel L2 of the per-layer route's.  M = 700: ragged 256-row tile."""
    from snerf_amd import ops
    sd, enc, cond, _, _ = _case(M)
    with torch.no_grad():
        rr, _, _ = om.nerf_mlp(sd, enc[:, None], cond)
    ref = rr.reshape(M, 3)

    def run(fused):
        net, _ = _net(ops.F16, sd, fused)
        assert net.colour_fused_ok() == fused
        SKIP, CB = _inputs(net, enc, cond)
        with torch.no_grad():
            raw_rgb, _, saved = net.forward(SKIP, CB, True)
        return raw_rgb.cpu(), saved
    rgb_f, saved_f = run(True)
    rgb_l, saved_l = run(False)
    assert saved_f[1][-1][0] == "fused" and len(saved_l[1]) == 3
    scale = float(ref.abs().max())
    err_f, err_l = float((rgb_f - ref).abs().max()) / scale, float((rgb_l - ref).abs().max()) / scale
    r = rel(rgb_f, rgb_l)
    worst = 0.0
    for j in range(3):
        yf, yl = saved_f[1][j][2], saved_l[1][j][2]
        assert yf.dtype == torch.float16 and yl.dtype == torch.float16
        worst = max(worst, rel(yf, yl))
    print(f"MEASURED fp16 fused colour head vs fp32 oracle (M {M}): fused {err_f:.3e}, per-layer {err_l:.3e}; fused vs per-layer rel L2 {r:.3e}; "
          f"stored activations fused vs per-layer worst rel L2 {worst:.3e}")
    assert err_f < 2.0 * err_l + 1e-3
    assert r < 5e-3
    assert worst < 1e-2


# ---- 3. differential: fp16 arithmetic, not bf16 ---------------------------------------------------------------------------------------------
def test_fp16_fused_colour_forward_is_fp16_arithmetic_not_bf16(backend):
    """(3: the differential assertion; a mis-instantiated kernel cannot pass.)  ops.fcolour_fwd called directly on weights, post-ReLU
    bottleneck rows and view encodings that bf16 AND fp16 hold exactly, against the four layers in float64: the only error left is the
    rounding of the hidden activations, and fp16's three more mantissa bits predict a ratio of 1/8 between the flavours.  Required:
    rel(fp16) <= 0.25 rel(bf16), twice the prediction (a kernel rounding the hidden layers through bf16 gives 0.58 on the CPU models)."""
    from snerf_amd import ops
    M = 1000
    shapes = _shapes()
    g = torch.Generator().manual_seed(71)
    both = lambda t: t.bfloat16().float().half().float()
    sd = {k: both(torch.randn(s, generator=g) * (1.4 / s[1] ** 0.5) if len(s) == 2 else torch.randn(s, generator=g) * 0.1) for k, s in shapes}
    cb = both(torch.relu(torch.randn(M, H, generator=g)))          # a post-ReLU bottleneck
    vd = both(torch.rand(M, 27, generator=g) * 2 - 1)
    for v in list(sd.values()) + [cb, vd]:
        assert torch.equal(v.bfloat16().float(), v) and torch.equal(v.half().float(), v), "both round trips must be the identity"
    W = lambda n: sd["mlp." + n + ".weight"].double()
    B = lambda n: sd["mlp." + n + ".bias"].double()
    h = torch.cat([cb, vd], 1).double()
    for j in range(3):
        h = torch.relu(h @ W(f"cond_layers.{j}.layers.0").t() + B(f"cond_layers.{j}.layers.0"))
    ref = (h @ W("rgb_layer").t() + B("rgb_layer")).float()
    err = {}
    for dt in (ops.F16, ops.BF16):
        net, _ = _net(dt, sd)
        assert net.colour_fused_ok()
        net.ensure_packed(False)
        net._colour_streams(False)
        assert net._cfwd[0].dtype == net.tdt
        _, CB = net.alloc_inputs(M)
        CB.zero_()
        CB[:, :H] = cb.to(DEV, net.tdt)
        CB[:, H:H + 27] = vd.to(DEV, net.tdt)
        raw = torch.empty(M, 3, device=DEV)
        ops.fcolour_fwd(CB, net._cfwd[0], net._cfwd[1], raw)
        err[dt] = rel(raw, ref)
    ratio = err[ops.F16] / err[ops.BF16]
    print(f"MEASURED fused colour head vs float64 layers on exactly representable operands, rel L2: fp16 {err[ops.F16]:.3e}, bf16 {err[ops.BF16]:.3e}, "
          f"ratio {ratio:.3f}")
    assert err[ops.F16] <= 0.25 * err[ops.BF16]


# ---- 4. bit-exact properties -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [700, 1024])
def test_fp16_colour_inference_launch_reproduces_training_launch(backend, M):
    """(4a.)  The inference launch (no stores) gives the raw_rgb of the training launch bit for bit."""
    from snerf_amd import ops
    sd, enc, cond, _, _ = _case(M)
    net, _ = _net(ops.F16, sd)
    SKIP, CB = _inputs(net, enc, cond)
    with torch.no_grad(), _Calls(net) as c:
        raw_t, _, saved = net.forward(SKIP, CB, True)
        raw_i, _, _ = net.forward(SKIP.clone(), CB.clone(), False)
    assert c.cf == 2 and saved[1][-1][0] == "fused"
    n_diff = int((raw_t != raw_i).sum())
    print(f"MEASURED fp16 colour head, inference vs training launch (M {M}): {n_diff} differing raw_rgb values")
    assert torch.equal(raw_i, raw_t), "inference launch (no stores) must reproduce the training launch"


@pytest.mark.gpu
@pytest.mark.parametrize("M", [700, 1024])
def test_fp16_colour_relu_bit_masks_are_exactly_the_sign_of_the_stored_activations(M):
    """(4b.)  Each of the three ReLU bit masks the fp16 training launch writes -- decoded from the documented layout as
    test_fp16_relu_bit_masks_are_exactly_the_sign_of_the_stored_activations does -- is exactly y > 0 of the fp16 activation it stored."""
    from snerf_amd import ops

    def decode(words, Mr, N):
        w = words.cpu().numpy().view("uint8").reshape(-1, N // 64, 64, 4)                     # [rb, cg, word, byte]
        bits = ((w[..., None] >> np.arange(8, dtype="uint8")) & 1).astype(bool)               # [rb, cg, word, byte, e]
        rb, cg, ln, it, e = np.meshgrid(*[np.arange(n) for n in bits.shape], indexing="ij")
        out = np.zeros((bits.shape[0] * 32, N), bool)
        out[rb * 32 + 8 * it + (ln >> 3), cg * 64 + 8 * (ln & 7) + e] = bits
        return out[:Mr]
    sd, enc, cond, _, _ = _case(M)
    net, _ = _net(ops.F16, sd)
    SKIP, CB = _inputs(net, enc, cond)
    with torch.no_grad():
        _, _, saved = net.forward(SKIP, CB, True)
    tag, cbits, _ = saved[1][-1]
    assert tag == "fused" and len(cbits) == 3
    bad = []
    for j in range(3):
        y = saved[1][j][2]
        assert y.dtype == torch.float16
        bad.append(int((decode(cbits[j], M, 128) != (y[:, :128].float() > 0).cpu().numpy()).sum()))
    print(f"MEASURED fp16 colour head ReLU bit masks vs stored activations (M {M}): mismatching bits per layer {bad}")
    assert bad == [0, 0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("M", [700, 1024])
def test_fp16_colour_read_ahead_depth_does_not_change_the_result(M):
    """(4c.)  variant = 1 (input read-ahead of five lines) gives the raw_rgb and the stored activations of variant = 0: the depth of the
    read-ahead does not change the order of the k-steps."""
    from snerf_amd import ops
    sd, enc, cond, _, _ = _case(M)
    net, _ = _net(ops.F16, sd)
    SKIP, CB = _inputs(net, enc, cond)
    with torch.no_grad():
        net.forward(SKIP, CB, True)                                  # fills CB[:, :H]
    net._colour_streams(True)
    out = []
    for variant in (0, 1):
        raw = torch.empty(M, 3, device=DEV)
        cys = [net.buf(M, 128) for _ in range(3)]
        cbits = [torch.empty(ops.mask_bits_words(M, 128), dtype=torch.int32, device=DEV) for _ in range(3)]
        ops.fcolour_fwd(CB, net._cfwd[0], net._cfwd[1], raw, cys, cbits, variant=variant)
        raw_i = torch.empty(M, 3, device=DEV)
        ops.fcolour_fwd(CB, net._cfwd[0], net._cfwd[1], raw_i, variant=variant)
        assert torch.equal(raw, raw_i)
        out.append([raw] + cys)
    n_diff = [int((a != b).sum()) for a, b in zip(*out)]
    print(f"MEASURED fp16 colour head, read-ahead 5 lines vs 3 (M {M}): differing values in raw_rgb / activations {n_diff}")
    assert n_diff == [0, 0, 0, 0]


# ---- 5. gradients ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [700, 1024])
def test_fp16_fused_colour_gradients_match_per_layer_kernels_and_oracle(backend, M):
    """(5: gradients.)  Every parameter gradient of the whole MipNerfNet through backward() (the scaled fp16 backward): fused against torch
    autograd of the oracle and against `fused_colour = False`, with the bounds of test_fused_colour_head_matches_per_layer_kernels_and_oracle
    as they stand (e_f < 0.25, e_f < 2 e_l + 2e-2, fused vs per-layer < 3e-2 for the six parameters it lists); all finite; with
    want_cond_grad the view-encoding gradient dV fused vs per-layer < 3e-2."""
    from snerf_amd import ops
    sd, enc, cond, d_rgb, d_den = _case(M)
    pr = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    rr, rd, _ = om.nerf_mlp(pr, enc[:, None], cond)               # one "ray" per row: every row carries its own view encoding
    ((rr.reshape(M, 3) * d_rgb).sum() + (rd.reshape(M, 1) * d_den).sum()).backward()

    def run(fused):
        net, arena = _net(ops.F16, sd, fused)
        assert net.colour_fused_ok() == fused
        SKIP, CB = _inputs(net, enc, cond)
        with _Calls(net) as c:
            raw_rgb, raw_d, saved = net.forward(SKIP, CB, True)
            arena.grad.zero_()
            dV = net.backward(d_rgb.to(DEV), d_den.to(DEV), saved, want_cond_grad=True)
        assert (c.cf, c.cb) == ((1, 1) if fused else (0, 0))
        return {k: arena.g[k].clone() for k in sd}, dV
    (g_f, dV_f), (g_l, dV_l) = run(True), run(False)
    worst = [0.0, 0.0, 0.0]
    for k in sd:
        e_f, e_l, e_fl = rel(g_f[k], pr[k].grad), rel(g_l[k], pr[k].grad), rel(g_f[k], g_l[k])
        worst = [max(worst[0], e_f), max(worst[1], e_l), max(worst[2], e_fl)]
    r_dv = rel(dV_f[:, :27], dV_l[:, :27])
    print(f"MEASURED fp16 colour head gradients (M {M}), worst rel L2: fused vs autograd {worst[0]:.3e}, per-layer vs autograd {worst[1]:.3e}, "
          f"fused vs per-layer {worst[2]:.3e}; dV fused vs per-layer {r_dv:.3e}")
    for k in sd:
        e_f, e_l = rel(g_f[k], pr[k].grad), rel(g_l[k], pr[k].grad)
        assert torch.isfinite(g_f[k]).all(), k
        assert e_f < 0.25 and e_f < 2.0 * e_l + 2e-2, (k, e_f, e_l)
    for k in ("mlp.cond_layers.0.layers.0.weight", "mlp.cond_layers.1.layers.0.bias", "mlp.cond_layers.2.layers.0.bias", "mlp.bottleneck_layer.layers.0.bias",
              "mlp.bottleneck_layer.layers.0.weight", "mlp.layers.3.layers.0.weight"):
        assert rel(g_f[k], g_l[k]) < 3e-2, (k, rel(g_f[k], g_l[k]))
    assert torch.isfinite(dV_f).all() and r_dv < 3e-2, r_dv


# ---- 6. public interface -----------------------------------------------------------------------------------------------------------------
def test_fp16_mipnerf_forward_vs_oracle_with_the_fused_colour_head(backend):
    """(6: public interface, inference.)  MipNerfModel(compute="fp16", hidden_layer=1024) forward against the oracle at the existing fp16
    row's 1e-2 (the body of test_mipnerf_forward_vs_oracle); its colour head is exactly one fused launch."""
    with _Calls() as c:
        test_paths.test_mipnerf_forward_vs_oracle(backend, "fp16", 1024, 64, 129, 96, 1e-2)
    print(f"MEASURED fp16 MipNerfModel forward: {c.cf} fcolour_fwd, {c.cb} fcolour_bwd calls")
    assert c.cf == 1 and c.cb == 0, (c.cf, c.cb)


def test_fp16_trainer_step_with_the_fused_colour_head_matches_the_per_layer_route(backend):
    """(6: public interface, training.)  One MipTrainer.step in fp16 at hidden 1024: one fcolour_fwd and one fcolour_bwd; the gradient the
    optimiser receives is finite and equals the `fused_colour = False` step's within the gradient bound of (5) (rel L2 < 3e-2 per parameter),
    and the parameters it leaves are finite and within one Adam step (2 lr: a sign flip of a near-zero gradient) of that run's."""
    from snerf_amd import mipnerf, ops
    from snerf_amd.trainer import MipTrainer
    S0, P1, n, hidden, lr = 24, 25, 16, 1024, 5e-4
    sd = test_paths.random_params(om.mipnerf_param_shapes(hidden=hidden, prop_hidden=256), 21, ("mlp.density_layer.bias", "proposal.density_layer.bias"))
    rays_c = common.synthetic_rays(n, seed=7)
    gg = torch.Generator().manual_seed(8)
    target, tdepth = torch.rand(n, 3, generator=gg), torch.rand(n, generator=gg) * 50 + 5

    def run(fused):
        m = test_paths.make_mip(hidden, 256, S0, P1, "fp16", sd)
        m.nerf.fused_colour = fused
        assert m.nerf.colour_fused_ok() == fused
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
        assert (c.cf, c.cb) == ((1, 1) if fused else (0, 0)), (c.cf, c.cb)
        assert len(grads) == 1
        return m, grads[0]
    (m_f, g_f), (m_l, g_l) = run(True), run(False)
    assert torch.isfinite(m_f.arena.flat).all() and torch.isfinite(g_f).all()
    worst = 0.0
    for name, (o, cnt) in m_f.arena._offs.items():
        worst = max(worst, rel(g_f[o:o + cnt], g_l[o:o + cnt]))
    dp = float((m_f.arena.flat - m_l.arena.flat).abs().max())
    print(f"MEASURED fp16 trainer step, fused vs per-layer colour head: worst per-parameter gradient rel L2 {worst:.3e}, max parameter difference {dp:.3e}")
    for name, (o, cnt) in m_f.arena._offs.items():
        r = rel(g_f[o:o + cnt], g_l[o:o + cnt])
        assert r < 3e-2, (name, r)
    assert dp <= 2 * lr + 1e-7


# ---- 7. argument checks without a GPU ---------------------------------------------------------------------------------------------------------
def test_fp16_colour_dt_entries_reject_bad_arguments_without_a_gpu():
    """(7: argument checks.)  Both `_dt` entries return "bad argument" for dtype SNERF_DT_F32, for dtype 5, for a misaligned pointer in either
    16-bit dtype and for F32 with an empty batch, before anything touches a device; an empty batch in F16 is accepted; the entries without the
    suffix keep their argument lists (an empty batch is accepted, a misaligned pointer is not).  The library says version >= 3."""
    import ctypes
    from snerf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    version = _lib.load().snerf_version()
    print(f"MEASURED snerf_version() = {version}")
    assert version >= 3
    F32, BF16, F16 = 0, 1, 2
    buf = (ctypes.c_char * 4096)()
    A = (ctypes.addressof(buf) + 15) & ~15                        # a 16-byte aligned host address: never dereferenced by the checks
    arr = (ctypes.c_void_p * 4)(*([A] * 4))
    lds = (ctypes.c_long * 4)(*([128] * 4))
    pa, pl = ctypes.addressof(arr), ctypes.addressof(lds)
    entries = {
        # name -> (arguments in front of dtype with a hole `P` for the pointer to misalign)
        "snerf_fcolour_fwd": lambda P, M: (P, 1056, A, 336, A, 13, A, pa, pl, pa, M, 0),
        "snerf_fcolour_bwd": lambda P, M: (A, P, 336, pa, pa, pl, A, 1024, pa, A, 1 << 24, M),
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
def test_fp16_fused_colour_head_is_bit_reproducible():
    """(8: determinism; the colour block of tests/test_determinism.py in fp16.)  150 repeats of the fp16 training forward + backward in the
    deterministic mode, with a vendor GEMM and other LDS content in between: raw_rgb and the four bias gradients of the fused chain are
    bit-identical run to run (the screen for a miscounted s_waitcnt)."""
    from snerf_amd import ops
    from snerf_amd.mlp import MipNerfNet, ParamArena
    from test_determinism import _repeat
    torch.manual_seed(2)
    dev = torch.device("cuda")
    big = torch.randn(2048, 2048, device="cuda").bfloat16()

    def rnd(shapes):
        return {k: (torch.randn(s) * (1.4 / s[-1] ** 0.5) if len(s) == 2 else torch.randn(s) * 0.1) for k, s in shapes}
    M = 5000                                                        # not a multiple of the 256-row tile
    shapes = _shapes()
    arena = ParamArena(shapes, dev); arena.load(rnd(shapes))
    net = MipNerfNet(arena, "mlp.", ops.F16, H)
    assert net.colour_fused_ok()
    SKIP, CB = net.alloc_inputs(M)
    SKIP.zero_(); CB.zero_()
    SKIP[:, H:H + 96] = (torch.rand(M, 96, device=dev) * 2 - 1).half()
    CB[:, H:H + 27] = (torch.rand(M, 27, device=dev) * 2 - 1).half()
    d_rgb, d_den = torch.randn(M, 3, device=dev), torch.randn(M, 1, device=dev)
    calls = _Calls()

    def colour():
        raw_rgb, raw_d, saved = net.forward(SKIP, CB, True)
        arena.grad.zero_()
        net.backward(d_rgb, d_den, saved)
        names = ["mlp.cond_layers.0.layers.0.bias", "mlp.cond_layers.1.layers.0.bias", "mlp.cond_layers.2.layers.0.bias", "mlp.bottleneck_layer.layers.0.bias"]
        return [raw_rgb] + [arena.g[k].clone() for k in names]
    net.deterministic = True                                       # fixed-order weight-gradient folds: every stored value is reproducible
    with calls:
        bad = _repeat(colour, 150, big)
    print(f"MEASURED fp16 fused colour head, 150 repeats: {bad} differing from the first ({calls.cf} fcolour_fwd, {calls.cb} fcolour_bwd launches)")
    assert calls.cf == 150 and calls.cb == 150
    assert bad == 0
