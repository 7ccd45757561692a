"""NeRF.forward(x) / NeRF_RGB.forward(x) on pre-embedded rows (s-nerf/model/run_nerf_helpers.py:103-126, 188-212), the entry point the
reference's own run_network reaches through batchify(fn, netchunk)(embedded) (:450-474).  Three layers, as in tests/test_classic_drivers.py:
the oracle against the reference's goldens (CPU), the product's host logic on the oracle-based emulation of the kernels (CPU), the HIP
kernels through the C-ABI (-m gpu) -- among them the fused-x launches (snerf_fmlp_classic_x_fwd / _x_train_fwd), bit for bit against
snerf_cast_pad followed by the buffer-reading launches."""
import contextlib

import pytest
import torch

import cpu_ops_emulation as emu
from oracle import classic as oc
from oracle import common

from cpu_ops_emulation import emulate_ops
from test_paths import close, nerf_params, random_params

DEV = "cuda"


# ---- CPU emulation of the entry points this feature adds (built from the emulated fused launches and cast_pad) ----
def _emu_x_fwd(x, stream, bias, raw):
    M = x.shape[0]
    E, VE = torch.zeros(M, 64, dtype=torch.bfloat16), torch.zeros(M, 32, dtype=torch.bfloat16)
    emu.cast_pad(x[:, :63], 63, E, 64, 1)
    emu.cast_pad(x[:, 63:90], 27, VE, 32, 1)
    emu.fmlp_classic_fwd(E, VE, stream, bias, raw)


def _emu_x_train_fwd(x, stream, bias, raw, xin, acts, bits):
    emu.cast_pad(x[:, :63], 63, xin[0], 64, 1)
    emu.cast_pad(x[:, :63], 63, xin[1], 64, 1)
    emu.cast_pad(x[:, 63:90], 27, xin[2], 32, 1)
    emu.fmlp_classic_train_fwd(xin[0], xin[2], stream, bias, raw, acts, bits)


def _emu_x_grad(g0, g5, gv, ic, icv, dx):
    dx[:, :ic] = g0[:, :ic] + g5[:, :ic]
    if icv:
        dx[:, ic:ic + icv] = gv[:, :icv]


@contextlib.contextmanager
def _emulated():
    from snerf_amd import ops
    new = {"fmlp_classic_x_fwd": _emu_x_fwd, "fmlp_classic_x_train_fwd": _emu_x_train_fwd, "classic_x_grad": _emu_x_grad}
    saved = {n: getattr(ops, n) for n in new}
    with emulate_ops():
        try:
            for n, f in new.items():
                setattr(ops, n, f)
            yield
        finally:
            for n, f in saved.items():
                setattr(ops, n, f)


@pytest.fixture(params=[pytest.param("hip", marks=pytest.mark.gpu), "emulated"])
def backend(request):
    global DEV
    if request.param == "hip":
        DEV = "cuda"
        yield "hip"
    else:
        DEV = "cpu"
        with _emulated():
            yield "emulated"
    DEV = "cuda"


def batchify(fn, chunk):
    """run_nerf_helpers.py:450-457"""
    return lambda inputs: torch.cat([fn(inputs[i:i + chunk]) for i in range(0, inputs.shape[0], chunk)], 0)


def _embedded(pts, viewdirs, multires=10, multires_views=4, identity=False):
    """x as the reference's run_network builds it (:460-470): embed(points) | embed(view directions broadcast over the samples)"""
    from snerf_amd import classic
    e, _ = classic.get_embedder(multires, -1 if identity else 0)
    x = e(pts.reshape(-1, 3))
    if viewdirs is not None:
        ed, _ = classic.get_embedder(multires_views, -1 if identity else 0)
        x = torch.cat([x, ed(viewdirs[:, None].expand(pts.shape).reshape(-1, 3))], -1)
    return x


def _fill(net, flip=False):
    sd = common.fill_state_dict_({k: torch.empty_like(v) for k, v in net.state_dict().items()})
    net.load_state_dict({k: v.flip(0) for k, v in sd.items()} if flip else sd)
    return net


def _oracle_dx(fn, x):
    xr = x.detach().cpu().clone().requires_grad_(True)
    return xr, fn(xr)


# ------------------------------------------------------------------------------------------------ oracle vs reference goldens
def test_oracle_batchified_forward_vs_reference_golden(golden):
    """the oracle's network, called the way batchify calls NeRF.forward (strided row chunks), reproduces the reference's run_network"""
    g = golden("g28_identity_embed")
    sd = common.fill_state_dict_({k: torch.empty(s) for k, s in oc.nerf_param_shapes(W=64, input_ch=3, input_ch_views=3)})
    pts, vd = g["pts"], g["viewdirs"]
    x = torch.cat([pts.reshape(-1, 3), vd[:, None].expand(pts.shape).reshape(-1, 3)], -1)
    out = batchify(lambda t: oc.nerf_mlp(sd, t, 3, 3), 7)(x).reshape(pts.shape[0], pts.shape[1], 4)
    close(out, g["run_network_out"], 1e-5, 1e-5, "oracle NeRF.forward, batchified")


# ------------------------------------------------------------------------------------------------ product vs reference goldens
def test_nerf_rgb_forward_on_embedded_rows_vs_golden(backend, golden):
    """NeRF_RGB(x) over batchify's row chunks (chunk 7 does not divide M): outputs and every parameter gradient against the reference's
    run_network (g20), the frozen alpha model gets none, d loss / d x against autograd of the oracle on the same x"""
    from snerf_amd import classic
    g = golden("g20_nerf_rgb")
    alpha_sd = {k: (v.flip(1) if v.dim() == 2 else v) for k, v in nerf_params(64).items()}
    alpha = classic.NeRF(D=8, W=64, input_ch=63, input_ch_views=27, output_ch=4, skips=[4], use_viewdirs=True, compute="f32", device=DEV)
    alpha.load_state_dict(alpha_sd)
    shapes = [(k, s) for k, s in oc.nerf_param_shapes(W=64) if not k.startswith("alpha_linear")]
    own = common.fill_state_dict_({k: torch.empty(s) for k, s in shapes})
    m = classic.NeRF_RGB(D=8, W=64, input_ch=63, input_ch_views=27, output_ch=4, skips=[4], use_viewdirs=True, alpha_model=alpha,
                         compute="f32", device=DEV)
    m.load_state_dict({**own, **{"alpha_model." + k: v for k, v in alpha.state_dict().items()}})
    pts, vd = g["pts"].to(DEV), g["viewdirs"].to(DEV)
    x = _embedded(pts, vd).detach().requires_grad_(True)
    out = batchify(m, 7)(x).reshape(pts.shape[0], pts.shape[1], 4)
    close(out, g["run_network_out"], 1e-4, 1e-4, "NeRF_RGB.forward(x)")
    ((out - g["target"].to(DEV)) ** 2).sum().backward()
    named = dict(m.named_parameters())
    for k in own:
        close(named[k].grad, g["grad_" + k], 1e-3, 1e-3 * float(g["grad_" + k].abs().max()), "NeRF_RGB grad " + k)
    assert all(p.grad is None for k, p in named.items() if k.startswith("alpha_model.")), "the alpha model is frozen"
    xr, ref = _oracle_dx(lambda t: oc.nerf_rgb_mlp({k: v for k, v in own.items()}, alpha_sd, t), x)
    ((ref.reshape(out.shape) - g["target"]) ** 2).sum().backward()
    scale = float(xr.grad.abs().max())
    close(x.grad / scale, xr.grad / scale, 0, 5e-4, "NeRF_RGB d loss / d x")


def test_no_viewdirs_forward_on_embedded_rows_vs_golden(backend, golden):
    """NeRF(use_viewdirs=False, output_ch=5)(x): x = embedded points only (input_ch_views = 0), outputs / gradients against g27"""
    from snerf_amd import classic
    g = golden("g27_no_viewdirs")
    m = _fill(classic.NeRF(D=8, W=64, input_ch=63, input_ch_views=0, output_ch=5, skips=[4], use_viewdirs=False, compute="f32", device=DEV))
    pts = g["pts"].to(DEV)
    x = _embedded(pts, None).detach().requires_grad_(True)
    out = batchify(m, 13)(x).reshape(pts.shape[0], pts.shape[1], 5)
    close(out, g["run_network_out"], 1e-4, 1e-4, "NeRF.forward(x), no viewdirs")
    ((out - g["target"].to(DEV)) ** 2).sum().backward()
    named = dict(m.named_parameters())
    for k in named:
        if "grad_" + k in g:
            ref = g["grad_" + k]
            close(named[k].grad / (ref.abs().max() + 1e-12), ref / (ref.abs().max() + 1e-12), 0, 5e-4, "grad " + k)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    xr, ref = _oracle_dx(lambda t: oc.nerf_mlp(sd, t, 63, 0, use_viewdirs=False), x)
    ((ref.reshape(out.shape) - g["target"]) ** 2).sum().backward()
    scale = float(xr.grad.abs().max())
    close(x.grad / scale, xr.grad / scale, 0, 5e-4, "d loss / d x, no viewdirs")


def test_identity_embedding_forward_on_embedded_rows_vs_golden(backend, golden):
    """get_embedder(., i=-1): x = [points | directions] (6 columns), against g28"""
    from snerf_amd import classic
    g = golden("g28_identity_embed")
    m = _fill(classic.NeRF(D=8, W=64, input_ch=3, input_ch_views=3, output_ch=4, skips=[4], use_viewdirs=True, compute="f32", device=DEV))
    pts, vd = g["pts"].to(DEV), g["viewdirs"].to(DEV)
    x = _embedded(pts, vd, identity=True).detach().requires_grad_(True)
    assert x.shape[-1] == 6
    out = batchify(m, 11)(x).reshape(pts.shape[0], pts.shape[1], 4)
    close(out, g["run_network_out"], 1e-4, 1e-4, "NeRF.forward(x), identity embedding")
    ((out - g["target"].to(DEV)) ** 2).sum().backward()
    for k, p in m.named_parameters():
        ref = g["grad_" + k]
        close(p.grad / (ref.abs().max() + 1e-12), ref / (ref.abs().max() + 1e-12), 0, 5e-4, "grad " + k)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    xr, ref = _oracle_dx(lambda t: oc.nerf_mlp(sd, t, 3, 3), x)
    ((ref.reshape(out.shape) - g["target"]) ** 2).sum().backward()
    scale = float(xr.grad.abs().max())
    close(x.grad / scale, xr.grad / scale, 0, 5e-4, "d loss / d x, identity embedding")


def test_forward_on_embedded_rows_rejects_bad_inputs(backend):
    from snerf_amd import classic
    m = classic.NeRF(D=8, W=64, input_ch=63, input_ch_views=27, output_ch=4, skips=[4], use_viewdirs=True, compute="f32", device=DEV)
    with pytest.raises(RuntimeError, match="last dimension"):
        m(torch.zeros(5, 89, device=DEV))
    with pytest.raises(RuntimeError, match="last dimension"):
        m(torch.zeros(5, 93, device=DEV))
    rgb = classic.NeRF_RGB(D=8, W=64, input_ch=63, input_ch_views=27, output_ch=4, skips=[4], use_viewdirs=True, compute="f32", device=DEV)
    with pytest.raises(RuntimeError, match="alpha_model"):
        rgb(torch.zeros(5, 90, device=DEV))
    assert m(torch.zeros(0, 90, device=DEV)).shape == (0, 4)


# ------------------------------------------------------------------------------------------------ the fused bf16 network, W = 256
def _bf16_net(seed=41):
    from snerf_amd import classic
    sd = random_params(oc.nerf_param_shapes(W=256), seed, ("alpha_linear.bias",))
    m = classic.NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=4, skips=[4], use_viewdirs=True, compute="bf16", device=DEV)
    m.load_state_dict(sd)
    assert m.net.fused_ok()
    return m, sd


def _points(n, S, seed):
    g = torch.Generator().manual_seed(seed)
    pts = torch.rand(n, S, 3, generator=g) * 4 - 2
    vd = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    return pts.to(DEV), vd.to(DEV)


def _both_routes(m, fn):
    m.net.fused_x = True
    try:
        a = fn()
        m.net.fused_x = False
        b = fn()
    finally:
        m.net.fused_x = True
    return a, b


def _train_step(m, x, w):
    for p in m.parameters():
        p.grad = None
    xx = x.detach().clone().requires_grad_(True)
    out = m(xx)
    (out * w).sum().backward()
    return out.detach(), {k: p.grad.clone() for k, p in m.named_parameters()}, xx.grad


def test_fused_x_training_route_matches_the_two_launch_route(backend):
    """training (deterministic mode): the fused-x train launch and snerf_cast_pad -> snerf_fmlp_classic_train_fwd give the same raw
    outputs, parameter gradients and input gradient bit for bit; the input gradient also against the oracle's autograd"""
    m, sd = _bf16_net()
    m.set_deterministic(True)
    pts, vd = _points(37, 9, 43)
    x = _embedded(pts, vd).detach()
    w = torch.randn(x.shape[0], 4, generator=torch.Generator().manual_seed(44)).to(DEV)
    (oa, ga, da), (ob, gb, db) = _both_routes(m, lambda: _train_step(m, x, w))
    assert torch.equal(oa, ob)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
    assert torch.equal(da, db)
    xr = x.cpu().clone().requires_grad_(True)
    (oc.nerf_mlp(sd, xr) * w.cpu()).sum().backward()
    rel = float((da.cpu() - xr.grad).norm() / xr.grad.norm())
    print(f"MEASURED bf16 d loss / d x vs fp32 oracle: rel L2 {rel:.3e}")
    # (a sanity bound: eight bf16 layers of data gradient on a random W = 256 network, measured 0.146 on the emulation; the bit-for-bit
    # comparison above and the mode test below are the real checks)
    assert rel < 0.25


@pytest.mark.gpu
def test_fused_x_inference_is_bit_identical_to_the_two_launch_route():
    """no_grad: model(x) through snerf_fmlp_classic_x_fwd == snerf_cast_pad -> snerf_fmlp_classic_fwd, for ragged and empty batches,
    a column slice of a wider tensor (row stride 97), leading dimensions, and batchify's row views"""
    m, _ = _bf16_net()
    pts, vd = _points(257, 256, 45)
    full = _embedded(pts, vd).detach()                                       # 65 792 rows
    with torch.no_grad():
        for M in (0, 1, 255, 257, 65536 + 3):
            x = full[:M]
            a, b = _both_routes(m, lambda: m(x))
            assert a.shape == (M, 4) and torch.equal(a, b), M
        wide = torch.zeros(4099, 97, device=DEV)
        wide[:, 5:95] = full[:4099]
        xs = wide[:, 5:95]
        assert xs.stride(0) == 97
        a, b = _both_routes(m, lambda: m(xs))
        assert torch.equal(a, b) and torch.equal(a, m(full[:4099]))
        a, b = _both_routes(m, lambda: m(full[:257 * 30].reshape(257, 30, 90)))
        assert a.shape == (257, 30, 4) and torch.equal(a, b)
        a, b = _both_routes(m, lambda: batchify(m, 1000)(full[:4099]))
        assert torch.equal(a, b) and torch.equal(a, m(full[:4099]))


@pytest.mark.gpu
def test_fused_x_matches_run_network_on_the_same_points():
    """model(Embedder(pts) | Embedder(viewdirs)) vs run_network(pts, viewdirs): the same network, but the pts launch evaluates sin in
    revolutions, so a few features round to the neighbouring bf16 -- the fused-embedding tests' bound"""
    from snerf_amd import classic
    m, _ = _bf16_net()
    pts, vd = _points(125, 16, 46)
    e, ev = classic.get_embedder(10, 0)[0], classic.get_embedder(4, 0)[0]
    with torch.no_grad():
        a = m(_embedded(pts, vd)).reshape(125, 16, 4)
        b = classic.run_network(pts, vd, m, e, ev)
    rel = float((a - b).norm() / b.norm())
    print(f"MEASURED NeRF.forward(x) vs run_network: rel L2 {rel:.3e}")
    assert rel < 3e-3


@pytest.mark.gpu
def test_fused_x_training_on_strided_views_and_input_gradient_only():
    """training through the fused-x launch on a column slice of a wider tensor, a frozen network whose only gradient is the input's,
    and batchify's chunks against the whole batch"""
    m, _ = _bf16_net()
    m.set_deterministic(True)
    pts, vd = _points(41, 25, 47)
    x = _embedded(pts, vd).detach()
    w = torch.randn(x.shape[0], 4, generator=torch.Generator().manual_seed(48)).to(DEV)
    o1, g1, d1 = _train_step(m, x, w)
    wide = torch.zeros(x.shape[0], 97, device=DEV)
    wide[:, 7:97] = x
    wide.requires_grad_(True)
    for p in m.parameters():
        p.grad = None
    out = m(wide[:, 7:97])
    assert torch.equal(out.detach(), o1)
    (out * w).sum().backward()
    assert torch.equal(wide.grad[:, 7:97], d1) and float(wide.grad[:, :7].abs().max()) == 0.0
    for k, p in m.named_parameters():
        assert torch.equal(p.grad, g1[k]), k
    for p in m.parameters():
        p.requires_grad_(False)
    try:
        xx = x.clone().requires_grad_(True)
        (m(xx) * w).sum().backward()
        assert torch.equal(xx.grad, d1)
    finally:
        for p in m.parameters():
            p.requires_grad_(True)


# ------------------------------------------------------------------------------------------------ every compute mode
@pytest.mark.parametrize("compute,tol_out,tol_grad", [("f32", 1e-4, 1e-3), ("bf16x3", 1e-4, 6e-3), ("f16f8", 1e-4, 3e-2),
                                                      ("bf16x3_fwd", 1e-4, 3e-2), ("bf16", 3e-1, 0.113), ("fp16", 5e-2, 0.16)])
def test_every_compute_mode_vs_oracle(backend, compute, tol_out, tol_grad):
    """model(x) and its parameter / input gradients against the fp32 oracle (W = 128: the per-layer launches on cast_pad'ed operands, the
    widths of tests/test_paths.py::test_classic_backward_vs_autograd).  Outputs element-wise relative to their largest value (the modes of
    the 1e-4 contract at 1e-4), gradients norm-wise per parameter at the bounds the run_network tests use"""
    from snerf_amd import classic
    W = 128
    sd = random_params(oc.nerf_param_shapes(W=W), 49, ("alpha_linear.bias",))
    m = classic.NeRF(D=8, W=W, input_ch=63, input_ch_views=27, output_ch=4, skips=[4], use_viewdirs=True, compute=compute, device=DEV)
    m.load_state_dict(sd)
    pts, vd = _points(30, 24, 50)
    x = _embedded(pts, vd).detach()
    t = torch.rand(x.shape[0], 3, generator=torch.Generator().manual_seed(51))
    loss = lambda o, t: ((torch.sigmoid(o[:, :3]) - t) ** 2).mean() + 0.1 * torch.relu(o[:, 3]).mean()      # (a render-like loss)
    xx = x.clone().requires_grad_(True)
    out = m(xx)
    loss(out, t.to(DEV)).backward()
    pr = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    xr = x.cpu().clone().requires_grad_(True)
    ref = oc.nerf_mlp(pr, xr)
    loss(ref, t).backward()
    err = float((out - ref.to(DEV)).abs().max())
    print(f"MEASURED {compute} NeRF.forward(x) vs fp32 oracle: max abs err {err:.3e} (max |ref| {float(ref.abs().max()):.2e})")
    scale = float(ref.abs().max())
    close(out / scale, ref / scale, 0, tol_out, f"{compute} NeRF.forward(x)")
    named = dict(m.named_parameters())
    for k in sd:
        rel = float((named[k].grad.cpu() - pr[k].grad).norm() / (pr[k].grad.norm() + 1e-12))
        assert rel < tol_grad, f"{compute} grad {k}: rel L2 {rel:.3e}"
    rel = float((xx.grad.cpu() - xr.grad).norm() / xr.grad.norm())
    print(f"MEASURED {compute} d loss / d x: rel L2 {rel:.3e}")
    assert rel < 2 * tol_grad            # (one data-gradient GEMM more than the first layer's weight gradient, and two paths summed)
