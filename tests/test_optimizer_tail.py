"""The optimizer tail (csrc/elementwise.hip: snerf_adam_step*, snerf_grad_clip_coef) against torch, part by part.

1. the Adam arithmetic against a float64 restatement, bounded by torch.optim.Adam's own fp32 error on the same gradients;
2. the gradient hygiene folded into the launch (unscale, global-norm clip, value clip, non-finite policy) as an exact function: the fused
   launch == torch's sequence on the gradient followed by a plain launch, bit for bit, at every alignment and grid-stride edge;
3. the `dropped` counter; 4. the clip coefficient against a float64 norm, NaN / Inf gradients included; 5. the C-ABI entries and their
   argument checks; 6. the trainers' wiring of all of it against a torch replay (both backends); 7. the captured step.

THE PINNED ORDER (train_utils.clip_gradients of the zipnerf reference, then torch.optim.Adam):
    g *= grad_scale * coef                       (GradScaler's unscale and clip_grad_norm_'s factor, one fp32 product)
    g = clamp(g, -grad_max_val, +grad_max_val)   (clip_grad_value_: torch.clamp -- +-Inf becomes +-grad_max_val, a NaN stays a NaN)
    policy: "keep" nothing | "zero" NaN, +-Inf -> 0 | "nan_to_num" NaN -> 0, +-Inf -> +-FLT_MAX
so with a value clip an Inf gradient reaches Adam as +-grad_max_val under EVERY policy ("zero" drops an Inf only when no value clip
is set), and a NaN in the arena makes the clip coefficient NaN, i.e. every gradient of that step NaN: "zero" / "nan_to_num" then apply
an all-zero gradient (m and v decay, p moves by momentum), "keep" poisons the arena as torch does."""
import functools
import math

import pytest
import torch

import test_paths
import test_zip_paths
from oracle import common
from oracle import mip as om
from test_gpu_kernels import ops  # noqa: F401  (fixture)
from test_paths import backend  # noqa: F401  (fixture: "hip" on the GPU box, "emulated" on the CPU emulation of snerf_amd.ops)

FLT_MAX = 3.4028234663852886e38
NAN, INF = float("nan"), float("inf")
POLICIES = ("keep", "zero", "nan_to_num")
ZIP_HP = (1e-2, 0.9, 0.99, 1e-15)            # lr, b1, b2, eps of the zipnerf reference
MIP_HP = (5e-4, 0.9, 0.999, 1e-8)


def f32(x):
    return torch.tensor(float(x), dtype=torch.float32)


def same(a, b):
    """bit-identical, any NaN equal to any NaN (+0 and -0 differ)"""
    if a.shape != b.shape:
        return False
    ia, ib = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    if torch.equal(ia, ib):
        return True
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(torch.where(na, 0, ia), torch.where(nb, 0, ib))


# ------------------------------------------------------------------------------------------------ 1. the Adam arithmetic ----
NZ, NZERO = 1024, 261                        # random-gradient elements, then a block whose gradient is always zero (n & 3 == 1)
ADAM_CONFIGS = {                             # b1, b2, eps, lr, steps
    "mip_b2_0.999_eps_1e-8_lr_5e-4": (0.9, 0.999, 1e-8, 5e-4, 6000),
    "zip_b2_0.99_eps_1e-15_lr_1e-2": (0.9, 0.99, 1e-15, 1e-2, 1500),
    "zip_b2_0.99_eps_1e-15_lr_1e-10": (0.9, 0.99, 1e-15, 1e-10, 1500),
}


def _trajectory(T, seed=1):
    """[T, NZ + NZERO] fp32 gradients: one magnitude per element, 1e-12 .. 1e2; the last NZERO columns are zero on every step"""
    g = torch.Generator().manual_seed(seed)
    scale = 10.0 ** (torch.rand(NZ, generator=g, dtype=torch.float64) * 14 - 12)
    G = torch.zeros(T, NZ + NZERO, dtype=torch.float32)
    G[:, :NZ] = (torch.randn(T, NZ, generator=g, dtype=torch.float64) * scale).float()
    return G


def _adam_f64(G, b1, b2, eps, lr):
    """the update of every step in float64 with python-double hyperparameters, from zero state: [T, n] float64"""
    m = torch.zeros(G.shape[1], dtype=torch.float64); v = torch.zeros_like(m)
    U = torch.empty(G.shape, dtype=torch.float64)
    for t in range(1, G.shape[0] + 1):
        g = G[t - 1].double()
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        U[t - 1] = -(lr / (1 - b1 ** t)) * m / (v.sqrt() / math.sqrt(1 - b2 ** t) + eps)
    return U


def _adam_torch_f32(G, b1, b2, eps, lr):
    """torch.optim.Adam in fp32 on the same gradients (what the reference runs); the parameter is zeroed before every step, so that the
    parameter after the step is the update: [T, n] fp32"""
    p = torch.zeros(G.shape[1], dtype=torch.float32, requires_grad=True)
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps)
    U = torch.empty(G.shape, dtype=torch.float32)
    for t in range(G.shape[0]):
        p.data.zero_()
        p.grad = G[t].clone()
        opt.step()
        U[t] = p.detach()
    return U


@functools.lru_cache(maxsize=None)
def torch_adam_error(b1, b2, eps, lr, T):
    """max |u_torch_fp32 - u_f64| / lr over the elements and steps of the trajectory: torch's own error, the yardstick of parts 1 and 6"""
    G = _trajectory(T)
    return float((_adam_torch_f32(G, b1, b2, eps, lr).double() - _adam_f64(G, b1, b2, eps, lr)).abs().max()) / lr


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", list(ADAM_CONFIGS))
def test_adam_update_against_float64_within_torchs_own_error(ops, cfg):
    """The UPDATE (p is zeroed before every launch) of T launches from zero state against the float64 restatement, each side carrying its
    own m and v.  Bound: 4 x the error torch.optim.Adam (fp32) shows on the same gradients -- the kernel makes the same number of
    roundings per element; the factor covers few-ulp differences of the device's powf / sqrtf / division.  The host step, the device
    step counter and the device learning rate give the same bits.  Zero-gradient elements: p untouched, m = v = 0 for good."""
    b1, b2, eps, lr, T = ADAM_CONFIGS[cfg]
    G = _trajectory(T)
    U64 = _adam_f64(G, b1, b2, eps, lr)
    e_torch = torch_adam_error(b1, b2, eps, lr, T)
    Gd, U64d = G.cuda(), U64[:, :NZ].cuda()
    n = NZ + NZERO
    p0 = torch.zeros(n)
    p0[NZ:] = torch.randn(NZERO, generator=torch.Generator().manual_seed(2))
    runs = {}
    for way in ("host", "step_dev", "lr_dev"):
        p, m, v, g = p0.cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), torch.empty(n, device="cuda")
        step_dev = torch.zeros(1, dtype=torch.int32, device="cuda")
        lr_dev = torch.tensor([lr], dtype=torch.float32, device="cuda")
        U = torch.empty(T, NZ, dtype=torch.float32, device="cuda")
        for t in range(1, T + 1):
            g.copy_(Gd[t - 1])
            p[:NZ].zero_()
            if way == "host":
                ops.adam_step(p, g, m, v, lr, b1, b2, eps, t)
            elif way == "step_dev":
                ops.adam_step_dev(p, g, m, v, lr, b1, b2, eps, step_dev)
            else:
                ops.adam_step(p, g, m, v, 7.0 * lr, b1, b2, eps, t, lr_dev=lr_dev)      # the host scalar must be ignored
            U[t - 1].copy_(p[:NZ])
        assert float(g.abs().max()) == 0.0
        assert int(step_dev) == (T if way == "step_dev" else 0), "the device step counter must read T after T launches"
        assert same(p[NZ:], p0[NZ:].cuda()), f"{way}: a parameter with an always-zero gradient moved"
        assert float(m[NZ:].abs().max()) == 0.0 and float(v[NZ:].abs().max()) == 0.0, f"{way}: m / v of zero-gradient elements"
        runs[way] = U
    err = (runs["host"].double() - U64d).abs() / lr
    e_kernel = float(err.max())
    worst_step = int(err.max(dim=1).values.argmax()) + 1
    print(f"MEASURED adam update {cfg} ({T} steps): max |u - u_f64| / lr: torch fp32 {e_torch:.3e}, kernel {e_kernel:.3e} "
          f"(ratio {e_kernel / e_torch:.2f}, worst at step {worst_step})")
    assert same(runs["step_dev"], runs["host"]), "step_dev gives other bits than the host step"
    assert same(runs["lr_dev"], runs["host"]), "lr_dev gives other bits than the host learning rate"
    assert e_kernel <= 4 * e_torch, (cfg, e_kernel, e_torch)


# ------------------------------------------------------------------------------------------- 2. hygiene as an exact function ----
GMV = 0.1
HYGIENE_SIZES = [1, 2, 3, 4, 5, 255, 256, 257, 1025, 2097151, 2097152, 2097153, 6606952]


def _specials(s):
    """the values a clean-up goes wrong on.  `s` = the factor the launch multiplies with: the second half is laid out so that the PRODUCT
    lands exactly on +-grad_max_val, its one-ulp neighbours and the denormals (s a power of two: the division is exact).  Denormals have
    short mantissas or sit far enough from underflow that g * grad_scale * coef rounds once in either association."""
    v = f32(GMV)
    up, dn = torch.nextafter(v, f32(1.0)), torch.nextafter(v, f32(0.0))
    edge = [float(x) for x in (v, up, dn)]
    den = [2.0 ** -149, 2.0 ** -127, 2.0 ** -126, float(torch.tensor(0x007fffff, dtype=torch.int32).view(torch.float32))]
    pre = [NAN, INF, -INF, FLT_MAX, -FLT_MAX, 0.0, -0.0] + [sg * x for x in edge + den for sg in (1.0, -1.0)]
    post = [sg * x / s for x in edge + den[:3] for sg in (1.0, -1.0)]
    return torch.tensor(pre + post, dtype=torch.float64).float()


def _hygiene_body(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(n, generator=g, device="cuda") * 10.0 ** (torch.rand(n, generator=g, device="cuda") * 9 - 6)   # 1e-6 .. 1e3: around the value clip


def _hygiene_grads(body, seed, s):
    """the random body with the special values planted in the head, in the n & 3 tail and across the body (small n: every element is
    special, and which one rotates with the seed)"""
    n = body.numel()
    g = torch.Generator().manual_seed(seed)
    sp = _specials(s)
    L = sp.numel()
    pos = torch.cat([torch.arange(min(n, L)), torch.arange(max(n - L, 0), n), torch.randint(0, n, (4 * L,), generator=g)]).unique()
    x = body.clone()
    x[pos.cuda()] = sp[(torch.arange(pos.numel()) + seed) % L].cuda()
    return x


def _clean_torch(g, grad_scale, coef, gmv, policy):
    """the reference's sequence on the gradient, in torch fp32: GradScaler's unscale, clip_grad_norm_'s product, clip_grad_value_,
    then the policy (train_utils.clip_gradients ends in nan_to_num_)"""
    x = g * f32(grad_scale).to(g.device)
    if coef is not None:
        x = x * coef[0]
    if gmv > 0:
        x = torch.clamp(x, -gmv, gmv)
    if policy == "zero":
        x = torch.where(torch.isfinite(x), x, torch.zeros_like(x))
    elif policy == "nan_to_num":
        x = torch.nan_to_num(x)
    return x


def _clean_f64(g, grad_scale, coef, gmv, policy):
    """the same in float64, with the launch's single fp32 factor grad_scale * coef"""
    fac = f32(grad_scale).to(g.device) * (coef[0] if coef is not None else 1.0)
    x = g.double() * fac.double()
    if gmv > 0:
        x = torch.clamp(x, -float(f32(gmv)), float(f32(gmv)))
    if policy == "zero":
        x = torch.where(torch.isfinite(x), x, torch.zeros_like(x))
    elif policy == "nan_to_num":
        x = torch.nan_to_num(x, nan=0.0, posinf=FLT_MAX, neginf=-FLT_MAX)
    return x


def _cleaned_by_kernel(ops, g, **opts):
    """what adam_clean_grad hands to the update: with b1 = 0 and m = 0 the launch leaves m = 0 * 0 + (1 - 0) * g_clean"""
    n = g.numel()
    p, m, v = (torch.zeros(n, device="cuda") for _ in range(3))
    ops.adam_step(p, g.clone(), m, v, 1e-2, 0.0, 0.99, 1e-15, 1, **opts)
    return m


@pytest.mark.gpu
def test_hygiene_order_inf_is_value_clipped_under_every_policy_and_nan_survives_the_clamp(ops):
    """the reference order, pinned: clamp BEFORE the policy.  With a value clip +-Inf -> +-grad_max_val under all three policies (also under
    "zero", which drops an Inf only without a value clip); a NaN passes torch.clamp and meets the policy."""
    g = torch.tensor([INF, -INF, NAN, 5.0, -5.0, 0.05, FLT_MAX, -FLT_MAX], device="cuda")
    v = float(f32(GMV))
    want = {("keep", GMV): [v, -v, NAN, v, -v, 0.05, v, -v], ("zero", GMV): [v, -v, 0.0, v, -v, 0.05, v, -v],
            ("nan_to_num", GMV): [v, -v, 0.0, v, -v, 0.05, v, -v],
            ("keep", 0.0): [INF, -INF, NAN, 5.0, -5.0, 0.05, FLT_MAX, -FLT_MAX], ("zero", 0.0): [0.0, 0.0, 0.0, 5.0, -5.0, 0.05, FLT_MAX, -FLT_MAX],
            ("nan_to_num", 0.0): [FLT_MAX, -FLT_MAX, 0.0, 5.0, -5.0, 0.05, FLT_MAX, -FLT_MAX]}
    for (policy, gmv), w in want.items():
        got = _cleaned_by_kernel(ops, g, nonfinite=policy, grad_max_val=gmv)
        assert same(got, torch.tensor(w, dtype=torch.float64).float().cuda()), (policy, gmv, got.tolist())
        assert same(got, _clean_torch(g, 1.0, None, gmv, policy)), (policy, gmv)


@pytest.mark.gpu
@pytest.mark.parametrize("n", HYGIENE_SIZES)
def test_hygiene_is_torchs_sequence_then_a_plain_launch(ops, n):
    """For every option set, ops.adam_step(g, options) == torch's sequence on g (fp32) followed by ops.adam_step(nonfinite="keep",
    grad_scale=1): p, m, v bit-identical (NaN-aware), g zeroed.  Part 1 pins the arithmetic, so this isolates adam_clean_grad.  Power-of-two
    grad_scale: the fused product grad_scale * coef is exact, the comparison is on bits; grad_scale = 1/3: the cleaned gradient within one
    ulp of the float64 restatement.  Every case on a 16-byte aligned buffer (vector flavour) and on slices offset by 1, 2, 3 floats (scalar
    flavour), which agree bit for bit; sizes around the grid-stride caps of both flavours (2048 x 256 x 4 = 8192 x 256 = 2 097 152) and a
    shipped table (6 606 952)."""
    lr, b1, b2, eps = ZIP_HP
    gen = torch.Generator().manual_seed(n)
    p0, m0, v0 = torch.randn(n, generator=gen).cuda(), (torch.randn(n, generator=gen) * 0.1).cuda(), (torch.rand(n, generator=gen) * 0.01).cuda()
    bufs = [torch.empty(n + 8, device="cuda") for _ in range(4)]
    body = _hygiene_body(n, n)
    case = 0
    for gs in (1.0, 1.0 / 8, 2.0 ** -15, 1.0 / 3):
        for cval in (None, 0.25, 1.0, 0.0, NAN):
            coef = None if cval is None else torch.tensor([cval, 0.0], dtype=torch.float32, device="cuda")
            s = float(f32(gs)) * (cval if cval in (0.25, 1.0) else 1.0)
            for gmv in (0.0, GMV):
                for policy in POLICIES:
                    case += 1
                    what = (n, gs, cval, gmv, policy)
                    g0 = _hygiene_grads(body, 1000 * case + 7, s)
                    if gs != 1.0 / 3:
                        x = _clean_torch(g0, gs, coef, gmv, policy)
                        # (the inputs are such that the two associations of g * grad_scale * coef round alike: see _specials)
                        if cval in (0.25, 1.0):
                            assert same(g0 * (f32(gs).cuda() * coef[0]), (g0 * f32(gs).cuda()) * coef[0]), what
                        ref = [p0.clone(), x, m0.clone(), v0.clone()]
                        ops.adam_step(*ref, lr, b1, b2, eps, 3, grad_scale=1.0, nonfinite="keep")
                    else:
                        x64 = _clean_f64(g0, gs, coef, gmv, policy)
                        x32 = x64.float()
                        got = _cleaned_by_kernel(ops, g0, grad_scale=gs, nonfinite=policy, grad_max_val=gmv, clip_coef=coef)
                        lo, hi = torch.nextafter(x32, torch.full_like(x32, -INF)), torch.nextafter(x32, torch.full_like(x32, INF))
                        ok = (got == x32) | ((got >= lo) & (got <= hi)) | (torch.isnan(got) & torch.isnan(x32))
                        assert bool(ok.all()), (what, "cleaned gradient more than 1 ulp from the float64 restatement", int((~ok).sum()))
                        ref = None
                    for off in range(4):
                        for b in bufs:
                            b.fill_(7.0)
                        views = [b[off:off + n] for b in bufs]
                        for vw, src in zip(views, (p0, g0, m0, v0)):
                            vw.copy_(src)
                        ops.adam_step(*views, lr, b1, b2, eps, 3, grad_scale=gs, nonfinite=policy, grad_max_val=gmv, clip_coef=coef)
                        if ref is None:                       # 1/3: the aligned launch is the partner of the offset ones
                            ref = [vw.clone() for vw in views]
                        for k, name in ((0, "p"), (2, "m"), (3, "v")):
                            assert same(views[k], ref[k]), (what, off, name)
                        assert float(views[1].abs().max()) == 0.0, (what, off, "g not zeroed")
                        for b in bufs:
                            assert bool((b[:off] == 7.0).all()) and bool((b[off + n:] == 7.0).all()), (what, off, "wrote outside its slice")
    assert case == 120


# --------------------------------------------------------------------------------------------------- 3. the dropped counter ----
@pytest.mark.gpu
def test_dropped_counts_every_nonfinite_element_whatever_the_options(ops):
    """~10 000 NaN / +-Inf at random positions -- the first element, the vector body, the n & 3 tail -- : the counter grows by exactly
    (~isfinite(g)).sum() per launch under all three policies, with and without clipping, in both flavours, and is never reset."""
    lr, b1, b2, eps = ZIP_HP
    n = 1000003
    gen = torch.Generator().manual_seed(3)
    base = torch.randn(n, generator=gen)
    base[torch.randint(0, n, (500,), generator=gen)] = FLT_MAX          # finite: not counted (it overflows only after the scale)
    bad = torch.cat([torch.tensor([0, n - 3, n - 2, n - 1]), torch.randint(0, n, (10000,), generator=gen)]).unique()
    base[bad] = torch.tensor([NAN, INF, -INF])[torch.randint(0, 3, (bad.numel(),), generator=gen)]
    expect = int((~torch.isfinite(base)).sum())
    assert expect == bad.numel() and 9900 < expect <= 10004
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    total = 0
    bufs = [torch.zeros(n + 8, device="cuda") for _ in range(4)]
    for off in (0, 1, 2, 3):
        views = [b[off:off + n] for b in bufs]
        for policy in POLICIES:
            for gmv, cval in ((0.0, None), (GMV, None), (0.0, 0.25), (GMV, 0.25), (GMV, NAN)):
                views[1].copy_(base)
                coef = None if cval is None else torch.tensor([cval, 0.0], dtype=torch.float32, device="cuda")
                ops.adam_step(*views, lr, b1, b2, eps, 1, grad_scale=2.0, nonfinite=policy, grad_max_val=gmv, clip_coef=coef, dropped=cnt)
                total += expect
                assert int(cnt) == total, (off, policy, gmv, cval, int(cnt), total)
    views[1].copy_(torch.randn(n, generator=gen))                        # a clean gradient adds nothing
    ops.adam_step(*views, lr, b1, b2, eps, 1, dropped=cnt)
    assert int(cnt) == total


# ------------------------------------------------------------------------------------------------------ 4. grad_clip_coef ----
CLIP_SIZES = [1, 255, 256, 257, 262143, 262144, 262145, 10000019]
CLIP_TOL = 1e-6          # relative: five fp32 roundings (grad_scale, the norm, their product, + 1e-6, the division) after the double sum


def _coef64(norm64, grad_scale, max_norm):
    c = float(f32(max_norm)) / (abs(float(f32(grad_scale))) * norm64 + 1e-6)
    return min(c, 1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("n", CLIP_SIZES)
def test_grad_clip_coef_against_a_float64_norm(ops, n):
    """coefficient and norm vs a float64 norm at 1e-6 relative, around the 1024-block cap (262 144 = 1024 x 256), on offset slices, for an
    input whose sum of squares overflows fp32 (1e-20 .. 1e18), with either sign of grad_scale; exactly 1.0 below max_norm; run-to-run
    bit-identical."""
    gen = torch.Generator().manual_seed(n)
    buf = torch.empty(n + 3, device="cuda")
    worst = {"coef": 0.0, "norm": 0.0}
    for kind in ("unit", "wide"):
        x = torch.randn(n, generator=gen)
        if kind == "wide":
            x = x.sign() * 10.0 ** (torch.rand(n, generator=gen) * 38 - 20)
            x[torch.randint(0, n, (1,), generator=gen)] = 1e18           # (so that n = 1 .. 257 reach the top of the range too)
        for off in (0, 1, 2, 3):
            g = buf[off:off + n]
            g.copy_(x)
            norm64 = float(g.double().pow(2).sum().sqrt())
            if kind == "wide" and n >= 262143:                          # (it takes a few hundred elements near 1e18)
                assert not math.isfinite(float(g.pow(2).sum())), "the fp32 sum of squares was meant to overflow"
            for gs in (0.125, -0.125, 1.0 / 3):
                for frac in (0.37, 2.0):                                 # clip active / the norm below max_norm
                    max_norm = frac * abs(gs) * norm64
                    out = ops.grad_clip_coef(g, gs, max_norm)
                    c, nm = float(out[0]), float(out[1])
                    assert math.isfinite(c) and math.isfinite(nm), (n, kind, off, gs, frac, c, nm)
                    want_n = abs(float(f32(gs))) * norm64
                    worst["norm"] = max(worst["norm"], abs(nm - want_n) / want_n)
                    assert abs(nm - want_n) <= CLIP_TOL * want_n, (n, kind, off, gs, nm, want_n)
                    if frac > 1:
                        assert c == 1.0, (n, kind, off, gs, c)
                    else:
                        want_c = _coef64(norm64, gs, max_norm)
                        worst["coef"] = max(worst["coef"], abs(c - want_c) / want_c)
                        assert abs(c - want_c) <= CLIP_TOL * want_c, (n, kind, off, gs, c, want_c)
                    assert same(ops.grad_clip_coef(g, gs, max_norm), out), "two runs differ"
                    if gs < 0:
                        assert same(out, ops.grad_clip_coef(g, -gs, max_norm)), "the sign of grad_scale reached the coefficient"
    print(f"MEASURED grad_clip_coef n = {n}: max rel error vs float64: coefficient {worst['coef']:.3e}, norm {worst['norm']:.3e}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 4099, 262145])
def test_grad_clip_coef_of_poisoned_gradients_and_what_adam_does_with_it(ops, n):
    """+-Inf in g: coefficient 0 (max_norm / Inf).  NaN in g: coefficient NaN, as torch.nn.utils.clip_grad_norm_ multiplies every gradient
    by NaN.  adam_step with that coefficient: "zero" / "nan_to_num" apply an all-zero gradient (m, v decay, p moves by momentum only),
    "keep" poisons p, m, v as torch does."""
    lr, b1, b2, eps = ZIP_HP
    gen = torch.Generator().manual_seed(n)
    g0 = torch.randn(n, generator=gen).cuda()
    for bad, pos in ((INF, 0), (-INF, n - 1), (INF, n // 2)):
        g = g0.clone(); g[pos] = bad
        out = ops.grad_clip_coef(g, 0.5, 1e-3)
        assert float(out[0]) == 0.0 and float(out[1]) == INF, (bad, pos, out.tolist())
    p0, m0, v0 = torch.randn(n, generator=gen).cuda(), (torch.randn(n, generator=gen) * 0.1).cuda(), (torch.rand(n, generator=gen) * 0.01).cuda()
    for pos in (0, n - 1, n // 2):
        g = g0.clone(); g[pos] = NAN
        out = ops.grad_clip_coef(g, 0.5, 1e-3)
        assert math.isnan(float(out[0])) and math.isnan(float(out[1])), ("NaN gradient", pos, out.tolist())
        # torch: the same arena as one parameter
        t = g.clone(); pt = torch.nn.Parameter(torch.zeros(n, device="cuda")); pt.grad = t
        torch.nn.utils.clip_grad_norm_([pt], 1e-3)
        assert bool(torch.isnan(t).all())
        zero = [p0.clone(), torch.zeros(n, device="cuda"), m0.clone(), v0.clone()]
        ops.adam_step(*zero, lr, b1, b2, eps, 3, nonfinite="keep")
        assert same(zero[2], m0 * f32(b1).cuda()) and not same(zero[0], p0)
        for policy in POLICIES:
            for gmv in (0.0, GMV):
                st = [p0.clone(), g.clone(), m0.clone(), v0.clone()]
                ops.adam_step(*st, lr, b1, b2, eps, 3, grad_scale=0.5, nonfinite=policy, grad_max_val=gmv, clip_coef=out)
                if policy == "keep":
                    assert all(bool(torch.isnan(st[k]).all()) for k in (0, 2, 3)), (policy, gmv)
                else:
                    assert all(same(st[k], zero[k]) for k in (0, 2, 3)), (policy, gmv, "not the all-zero-gradient step")


# ------------------------------------------------------------------------------------------------------- 5. the ABI surface ----
@pytest.mark.gpu
def test_plain_abi_entries_equal_the_counting_entry_and_bad_arguments_are_refused(ops):
    from snerf_amd import _lib
    from snerf_amd._lib import SnerfHipError
    lr, b1, b2, eps = ZIP_HP
    n = 4099
    gen = torch.Generator().manual_seed(5)
    p0, g0, m0, v0 = torch.randn(n, generator=gen).cuda(), torch.randn(n, generator=gen).cuda(), (torch.randn(n, generator=gen) * 0.1).cuda(), \
        (torch.rand(n, generator=gen) * 0.01).cuda()
    g0[7], g0[n - 1] = NAN, INF                    # the plain entries are plain torch.optim.Adam: nonfinite = 0 (keep)
    P, S = ops._p, ops._stream
    fresh = lambda: [p0.clone(), g0.clone(), m0.clone(), v0.clone()]
    ptrs = lambda st: [P(t) for t in st]

    def cnt(st, step, step_dev=None, lr_dev=None, gs=0.5, zg=1, nf=0, gmv=0.0, coef=None, dropped=None):
        _lib.call("snerf_adam_step_cnt", *ptrs(st), n, lr, b1, b2, eps, step, P(step_dev), P(lr_dev), gs, zg, nf, gmv, P(coef), P(dropped), S())
    eq = lambda a, b: all(same(x, y) for x, y in zip(a, b))
    # snerf_adam_step
    a, b = fresh(), fresh()
    _lib.call("snerf_adam_step", *ptrs(a), n, lr, b1, b2, eps, 3, 0.5, 1, S()); cnt(b, 3)
    assert eq(a, b) and float(a[1].abs().max()) == 0.0 and bool(torch.isnan(a[0][7]))
    a, b = fresh(), fresh()
    _lib.call("snerf_adam_step", *ptrs(a), n, lr, b1, b2, eps, 2, 0.5, 0, S()); cnt(b, 2, zg=0)
    assert eq(a, b) and same(a[1], g0), "zero_grad = 0 must leave g"
    # snerf_adam_step_dev
    a, b = fresh(), fresh()
    sa, sb = torch.full((1,), 2, dtype=torch.int32, device="cuda"), torch.full((1,), 2, dtype=torch.int32, device="cuda")
    _lib.call("snerf_adam_step_dev", *ptrs(a), n, lr, b1, b2, eps, P(sa), 0.5, 1, S()); cnt(b, 0, step_dev=sb)
    c = fresh(); cnt(c, 3)
    assert eq(a, b) and eq(a, c) and int(sa) == 3 and int(sb) == 3
    # snerf_adam_step_ex, every option
    coef = torch.tensor([0.25, 0.0], device="cuda"); lr_dev = torch.tensor([3e-3], device="cuda")
    for nf in (0, 1, 2):
        a, b = fresh(), fresh()
        sa.fill_(4); sb.fill_(4)
        _lib.call("snerf_adam_step_ex", *ptrs(a), n, lr, b1, b2, eps, 0, P(sa), P(lr_dev), 0.5, 1, nf, GMV, P(coef), S())
        cnt(b, 0, step_dev=sb, lr_dev=lr_dev, nf=nf, gmv=GMV, coef=coef)
        assert eq(a, b) and int(sa) == 5 and int(sb) == 5, nf
    # refused arguments: nothing is launched, nothing moves, and the next valid launch works
    dropped = torch.zeros(2, dtype=torch.int64, device="cuda")
    bad_calls = [
        ("step < 1", lambda st: _lib.call("snerf_adam_step", *ptrs(st), n, lr, b1, b2, eps, 0, 0.5, 1, S())),
        ("step < 1 (ex)", lambda st: _lib.call("snerf_adam_step_ex", *ptrs(st), n, lr, b1, b2, eps, 0, None, None, 0.5, 1, 1, 0.0, None, S())),
        ("step < 1 (cnt)", lambda st: cnt(st, 0)),
        ("step < 0 (cnt)", lambda st: cnt(st, -1)),
        ("nonfinite = 3", lambda st: cnt(st, 3, nf=3)),
        ("nonfinite = 3 with a device counter", lambda st: cnt(st, 0, step_dev=sa, nf=3)),
        ("nonfinite = -1 (ex)", lambda st: _lib.call("snerf_adam_step_ex", *ptrs(st), n, lr, b1, b2, eps, 3, None, None, 0.5, 1, -1, 0.0, None, S())),
        ("dropped not 8-byte aligned", lambda st: _lib.call("snerf_adam_step_cnt", *ptrs(st), n, lr, b1, b2, eps, 3, None, None, 0.5, 1, 1, 0.0, None,
                                                           P(dropped) + 4, S())),
        ("step_dev = NULL (dev)", lambda st: _lib.call("snerf_adam_step_dev", *ptrs(st), n, lr, b1, b2, eps, None, 0.5, 1, S())),
    ]
    sa.fill_(9)
    for what, f in bad_calls:
        st = fresh()
        with pytest.raises(SnerfHipError):
            f(st)
        torch.cuda.synchronize()
        assert eq(st, fresh()) and int(sa) == 9 and int(dropped.sum()) == 0, (what, "a refused call touched memory")
        a, b = fresh(), fresh()
        ops.adam_step(*a, lr, b1, b2, eps, 3, grad_scale=0.5, nonfinite="keep"); cnt(b, 3)
        assert eq(a, b), (what, "the launch after a refused call")
    for mn in (0.0, -1.0):
        with pytest.raises(SnerfHipError):
            ops.grad_clip_coef(g0, 1.0, mn)
    out = ops.grad_clip_coef(torch.ones(16, device="cuda"), 1.0, 1.0)
    assert abs(float(out[1]) - 4.0) < 1e-6 and abs(float(out[0]) - 0.25) < 1e-6
    # n == 0: a no-op (no launch, the device counter stays)
    st = fresh()
    for name, args in (("snerf_adam_step", (3, 0.5, 1)), ("snerf_adam_step_dev", (P(sa), 0.5, 1)),
                       ("snerf_adam_step_ex", (0, P(sa), None, 0.5, 1, 1, 0.0, None)), ("snerf_adam_step_cnt", (0, P(sa), None, 0.5, 1, 1, 0.0, None, P(dropped)))):
        _lib.call(name, *ptrs(st), 0, lr, b1, b2, eps, *args, S())
    torch.cuda.synchronize()
    assert eq(st, fresh()) and int(sa) == 9 and int(dropped.sum()) == 0


# ------------------------------------------------------------------------------------------------------ 6. trainer wiring ----
TRAINER_LR, TRAINER_WEIGHT_SCALE = 1e-2, 1.0 / 16     # see the test's docstring: the bound is on updates, and fl(p - u) must not drown it
TRAINER_OPTIONS = {
    "nan_to_num_both_clips": dict(nonfinite="nan_to_num", grad_max_norm=1e-3, grad_max_val=0.1),
    "zero_both_clips": dict(grad_max_norm=1e-3, grad_max_val=0.1),                 # the default policy
    "zero_value_clip_only": dict(grad_max_val=0.1),                                # an Inf is value-clipped, not dropped
    "no_hygiene": dict(nonfinite="keep"),
}


def _small_mip(opts):
    from snerf_amd import mipnerf
    from snerf_amd.trainer import MipTrainer
    dev = test_paths.DEV
    _, b1, b2, eps = MIP_HP
    lr = TRAINER_LR
    sd = test_paths.random_params(om.mipnerf_param_shapes(hidden=64, prop_hidden=64), 21, ("mlp.density_layer.bias", "proposal.density_layer.bias"))
    m = test_paths.make_mip(64, 64, 16, 17, "f32", {k: v * TRAINER_WEIGHT_SCALE for k, v in sd.items()})
    tr = MipTrainer(m, lr=lr, betas=(b1, b2), eps=eps, proposal_loss=True, **opts)
    n = 48
    rays = mipnerf.Rays(**{k: v.to(dev) for k, v in common.synthetic_rays(n, seed=7).items()})
    gg = torch.Generator().manual_seed(8)
    target, tdepth = torch.rand(n, 3, generator=gg).to(dev), (torch.rand(n, generator=gg) * 50 + 5).to(dev)
    return m, tr, (lambda: tr.step(rays, target, tdepth, None, randomized=False)), 1.0


def _small_zip(opts):
    from snerf_amd.trainer import ZipTrainer
    dev = test_paths.DEV
    _, b1, b2, eps = ZIP_HP
    lr = TRAINER_LR
    _, p = test_zip_paths.zip_setup()
    saved, test_zip_paths.DEV = test_zip_paths.DEV, dev
    try:
        m = test_zip_paths.make_model("f32", "f32", {k: v * TRAINER_WEIGHT_SCALE for k, v in p.items()})
    finally:
        test_zip_paths.DEV = saved
    loss_scale = 256.0
    tr = ZipTrainer(m, lr=lr, betas=(b1, b2), eps=eps, loss_scale=loss_scale, table_exchange="sharded", **opts)
    assert tr.shards is None and tr.loss_scale == loss_scale
    R = 16
    g = torch.Generator().manual_seed(5)
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    bx = torch.nn.functional.normalize(torch.cross(d, torch.randn(R, 3, generator=g), dim=-1), dim=-1)
    batch = {k: v.to(dev) for k, v in dict(origins=torch.randn(R, 3, generator=g) * 0.1, directions=d, viewdirs=d, radii=2e-3 + 2e-3 * torch.rand(R, 1, generator=g),
                                           near=torch.full((R, 1), 0.1), far=torch.full((R, 1), 10.0), base_x=bx,
                                           base_y=torch.nn.functional.normalize(torch.cross(d, bx, dim=-1), dim=-1)).items()}
    target = torch.rand(R, 3, generator=g).to(dev)
    draws = m._draws(R, False, m.arena.flat.device, 7)
    return m, tr, (lambda: tr.step(batch, target, rand=False, draws=draws)), 1.0 / loss_scale


@pytest.mark.parametrize("options", list(TRAINER_OPTIONS))
@pytest.mark.parametrize("which", ["mip", "zip"])
def test_trainers_hand_the_hygiene_options_to_the_launches_like_the_reference_loop(backend, which, options):
    """Five steps of a small MipTrainer / ZipTrainer (static power-of-two loss scale, eps = 1e-15) against a torch replay of the reference
    loop on a copy of the parameters: .grad = the trainer's gradient arena times 1 / (world x loss_scale), clip_grad_norm_,
    clip_grad_value_, the policy (nan_to_num_ in the reference), torch.optim.Adam.step().  One NaN and, on another step, one Inf are planted
    in the gradient arena in front of the launches.  Bound on arena.flat after step k: (the per-step bound of part 1 = 4 x torch's own
    error vs float64, in units of lr) x lr x k.  Catches a wrong scale handed to grad_clip_coef, a wrong order, arena padding leaking
    into the norm.  "zero": the documented deviation from the reference's nan_to_num_ -- an Inf is dropped unless value-clipped.
    Small weights (1/16 of the usual initialisation, |p| < 0.125 throughout) at lr = 1e-2: the bound is one on UPDATES (2e-6 .. 4e-6 lr
    per step), the comparison one on stored parameters, and p - u is rounded to fp32 -- two correct implementations whose updates differ in
    the last bit can land one ulp(p) apart.  With |p| in [0.25, 0.5) at the mip reference's 5e-4 that ulp (3e-8 = 6e-5 lr) is 15 x the
    bound, for torch against itself as well; here it (7.5e-9 = 7.5e-7 lr) is inside it, and nothing else about the update depends on |p|
    or lr.  Every step must see a live gradient (a larger lr kills the small mip model after one step, and a zero gradient tests nothing)."""
    from snerf_amd import ops
    opts = TRAINER_OPTIONS[options]
    policy, max_norm, max_val = opts.get("nonfinite", "zero"), opts.get("grad_max_norm", 0.0), opts.get("grad_max_val", 0.0)
    m, tr, step, grad_scale = (_small_mip if which == "mip" else _small_zip)(opts)
    _, b1, b2, eps = MIP_HP if which == "mip" else ZIP_HP
    lr = TRAINER_LR
    a = m.arena
    offs = dict(a._offs)
    first, last = a.names[0], a.names[-1]
    # "keep": a poisoned parameter makes the next forward NaN everywhere, so its plants come on the last step
    plants = {5: [(offs[first][0] + 1, NAN), (offs[last][0] + offs[last][1] - 1, INF)]} if policy == "keep" else \
        {2: [(offs[first][0] + 1, NAN)], 4: [(offs[last][0] + offs[last][1] - 1, -INF)]}
    snaps, planted = [], set()

    def plant():
        if tr.t not in planted:
            planted.add(tr.t)
            for pos, val in plants.get(tr.t, ()):
                a.grad[pos] = val
    real_adam, real_coef = ops.adam_step, ops.grad_clip_coef

    def adam_spy(p, g, *args, **kw):
        assert g.data_ptr() == a.grad.data_ptr() and g.numel() == a.numel
        plant()
        snaps.append(a.grad.clone())
        return real_adam(p, g, *args, **kw)

    def coef_spy(g, *args, **kw):
        plant()
        return real_coef(g, *args, **kw)
    params = {k: a.flat[o:o + c].detach().clone().requires_grad_(True) for k, (o, c) in offs.items()}
    pad = torch.ones(a.numel, dtype=torch.bool)
    for o, c in offs.values():
        pad[o:o + c] = False
    opt = torch.optim.Adam(list(params.values()), lr=lr, betas=(b1, b2), eps=eps)
    per_step = 4 * torch_adam_error(b1, b2, eps, lr, 300)
    worst = 0.0
    ops.adam_step, ops.grad_clip_coef = adam_spy, coef_spy
    try:
        for k in range(1, 6):
            step()
            assert len(snaps) == k and tr.t == k
            snap = snaps[-1]
            assert float(a.grad.abs().max()) == 0.0
            assert float((snap != 0).float().mean()) > 0.3 and float(a.flat.abs().nan_to_num(0.0).max()) < 0.125, (k, "dead gradient / large parameters")
            for name, (o, c) in offs.items():
                params[name].grad = snap[o:o + c].clone() * grad_scale
            if max_norm > 0:
                torch.nn.utils.clip_grad_norm_(list(params.values()), max_norm)
            if max_val > 0:
                torch.nn.utils.clip_grad_value_(list(params.values()), max_val)
            for q in params.values():
                if policy == "nan_to_num":
                    q.grad.nan_to_num_()
                elif policy == "zero":
                    q.grad = torch.where(torch.isfinite(q.grad), q.grad, torch.zeros_like(q.grad))
            opt.step()
            for name, (o, c) in offs.items():
                got, want = a.flat[o:o + c].detach().double().cpu(), params[name].detach().double().cpu()
                assert torch.equal(torch.isnan(got), torch.isnan(want)), (name, k, "NaN pattern")
                if policy != "keep" or k < 5:
                    assert bool(torch.isfinite(got).all()), (name, k)
                err = float(torch.nan_to_num(got - want, nan=0.0).abs().max()) / lr
                worst = max(worst, err / k)
                assert err <= per_step * k, (which, options, name, k, err, per_step * k)
            assert float(a.flat[pad.to(a.flat.device)].abs().max() if bool(pad.any()) else 0.0) == 0.0, "arena padding moved"
    finally:
        ops.adam_step, ops.grad_clip_coef = real_adam, real_coef
    assert planted >= set(plants)
    if policy == "keep":
        assert bool(torch.isnan(a.flat[offs[first][0] + 1]))
    print(f"MEASURED {which} trainer, {options}, {backend}: max |p - p_torch| / (lr k) over 5 steps {worst:.3e} (bound {per_step:.3e})")


# -------------------------------------------------------------------------------------------------------- 7. captured step ----
@pytest.mark.gpu
def test_captured_step_with_clipping_replays_like_the_eager_step(ops):
    """MipTrainer(grad_max_norm, grad_max_val).capture(): the clip-coefficient launches and the Adam launch that reads the coefficient
    from the device are part of the hipGraph.  Deterministic weight gradients, hidden width 64: three replays land on the bits of three
    eager steps of a twin trainer."""
    from snerf_amd import mipnerf
    from snerf_amd.trainer import MipTrainer
    n = 256

    def fresh():
        torch.manual_seed(0)
        m = mipnerf.MipNerfModel(n_samples=16, N_fine=17, no_warp_sample=0, ray_shape="cone", fn=1, radius=3., transform_idx=0, real=True, rgb_layer=3,
                                 hidden_layer=64, density_noise=0., max_deg_point=16, proposal_hidden_layer=64, proposal_loss=True, compute="bf16")
        m.set_deterministic(True)
        return m, MipTrainer(m, lr=5e-4, grad_max_norm=1e-3, grad_max_val=0.1)
    rays = mipnerf.Rays(**{k: v.cuda() for k, v in common.synthetic_rays(n, seed=3).items()})
    g = torch.Generator().manual_seed(4)
    tgt, td = torch.rand(n, 3, generator=g).cuda(), (torch.rand(n, generator=g) * 50 + 2).cuda()

    def eager():
        m, t = fresh()
        init = m.arena.flat.clone()
        for _ in range(3):
            t.step(rays, tgt, td, None, randomized=False)
        return m, t, init
    m1, t1, init = eager()
    m1b, _, _ = eager()
    assert same(m1.arena.flat, m1b.arena.flat), "two eager runs differ: the step is not deterministic"
    m2, t2 = fresh()
    t2.capture(rays, tgt, td, None, randomized=False, warmup=2)
    assert t2.t == 0 and int(t2._step_dev) == 0 and same(m2.arena.flat, init)
    for _ in range(3):
        t2.replay()
    assert t2.t == 3 and int(t2._step_dev) == 3
    assert not same(m1.arena.flat, init) and bool(torch.isfinite(m2.arena.flat).all())
    assert same(m2.arena.flat, m1.arena.flat) and same(t2.m, t1.m) and same(t2.v, t1.v), \
        float((m2.arena.flat - m1.arena.flat).abs().max())
    # the clip was active (otherwise this would not test the coefficient's way through the graph)
    unclipped, tu = fresh()
    tu.grad_max_norm = 0.0
    tu.step(rays, tgt, td, None, randomized=False)
    clipped, tc = fresh()
    tc.step(rays, tgt, td, None, randomized=False)
    assert not same(unclipped.arena.flat, clipped.arena.flat)
