"""zip_composite_fwd / _bwd and semantic_composite_kernel (end of csrc/zip.hip) against float64, stage-isolated.

The references are the eager oracle of tests/cpu_ops_emulation.py run twice on the same inputs: in float64 (the truth) and in
float32 (what a careful fp32 implementation achieves).  No fixed tolerance is both tight on well-conditioned rays and passable on
sparse non-opaque ones (1 - exp(-dd) cancels: the fp32 oracle itself is off by up to 2 % in g_dirs there), so every output of the
kernel is bounded by the fp32 oracle's own distance from float64 on the same case:

    e_hip <= K[output] * e_ref + FLOOR_EPS * eps32 * scale      (max-abs errors against float64)

scale: 1 for weights / acc / rgb, max td[S] for depth, max |float64 result| for gradients and semantic outputs.

The inputs keep clear of the three kinks of the function (test_inputs_keep_clear_of_the_kinks checks it for every ray of every
case): the depth clip (exp(E) at least 1e-3 relative inside [td[0], td[S]] on non-empty rays; the last interval is widened so that
an opaque ray that puts all its weight there is still inside), the background clamp (1 - acc > 0 in float64 for non-opaque rays:
directions of norm 0.15 .. 0.4 keep the optical depth of a 50-unit ray near 20 at most) and the softplus switch at 20.

Measured on an MI355X (e = max over the regime's cases of max-abs error / scale; ratio = largest per-case (e_hip - floor) / e_ref,
0 where e_hip is under the floor; `python tests/test_zip_composite_f64.py` prints this table):

    regime                    output              e_ref     e_hip  ratio   ratio with 1 - expf(-dd)
    mixed                     rgb               2.9e-07   1.4e-07   0.00      3.17
    mixed                     depth             8.5e-08   1.7e-07   0.00      0.00
    mixed                     acc               4.8e-07   1.2e-07   0.00      9.00
    mixed                     weights           7.6e-08   7.6e-08   0.00      0.00
    mixed                     d_raw_rgb         4.4e-07   2.4e-07   0.00      0.17
    mixed                     d_raw_density     4.2e-07   3.4e-07   0.00      1.03
    mixed                     g_dirs            1.1e-06   5.6e-07   0.11      2.14
    dense                     rgb               4.9e-07   6.2e-07   0.61      9.08
    dense                     depth             2.7e-06   9.5e-07   0.37      5.31
    dense                     acc               9.3e-07   7.2e-07   0.80      9.02
    dense                     weights           7.8e-08   6.9e-07   2.80      2.80
    dense                     d_raw_rgb         2.8e-07   5.1e-07   0.37      0.37
    dense                     d_raw_density     1.4e-05   1.8e-06   1.46      4.16
    dense                     g_dirs            1.4e-05   2.3e-06   1.19      8.74
    sparse                    rgb               5.7e-07   2.0e-07   0.00      4.03
    sparse                    depth             3.4e-04   7.4e-07   0.40      4.86
    sparse                    acc               1.1e-06   1.2e-07   0.00     53.36
    sparse                    weights           3.2e-08   3.5e-08   0.00      0.00
    sparse                    d_raw_rgb         6.9e-04   4.7e-07   0.00      1.29
    sparse                    d_raw_density     6.9e-04   1.5e-05   0.03      8.11
    sparse                    g_dirs            4.0e-01   1.3e-04   2.28      7.65
    semantic f32 softmax      sem               2.7e-07   2.2e-07   0.00      0.00
    semantic f32 softmax      d_logits          3.8e-06   3.8e-06   0.99      0.99
    semantic f32 identity     sem               1.0e-05   2.0e-06   0.15      0.15
    semantic f32 identity     d_logits          5.2e-08   5.2e-08   0.00      0.00
    semantic f32 identity     g_w               1.7e-07   2.4e-07   0.00      0.00
    semantic bf16 softmax     sem               1.7e-07   1.8e-07   0.00      0.00
    semantic bf16 softmax     d_logits          4.5e-07   9.2e-07   1.15      1.15
    semantic bf16 identity    sem               8.9e-06   4.1e-06   0.40      0.40
    semantic bf16 identity    d_logits          5.2e-08   5.2e-08   0.00      0.00
    semantic bf16 identity    g_w               1.4e-07   1.9e-07   0.00      0.00
    semantic f16 softmax      sem               1.4e-07   1.5e-07   0.00      0.00
    semantic f16 softmax      d_logits          5.5e-07   1.2e-06   1.25      1.25
    semantic f16 identity     sem               1.1e-06   1.1e-06   0.58      0.58
    semantic f16 identity     d_logits          5.2e-08   5.2e-08   0.00      0.00
    semantic f16 identity     g_w               1.6e-07   2.1e-07   0.00      0.00
    largest ratio per output: rgb 0.61, depth 0.40, acc 0.80, weights 2.80, d_raw_rgb 0.37, d_raw_density 1.46, g_dirs 2.28, sem 0.58, d_logits 1.25, g_w 0.00
    with 1 - expf(-dd):       rgb 9.08, depth 5.31, acc 53.36, weights 2.80, d_raw_rgb 1.29, d_raw_density 8.11, g_dirs 8.74, sem 0.58, d_logits 1.25, g_w 0.00
"""
import collections
import functools

import pytest
import torch

import cpu_ops_emulation as E

EPS32 = 1.1920929e-07
FLOOR_EPS = 4                     # "a few fp32 epsilons" of the output's natural scale
RGB_PADDING, DENSITY_BIAS = 0.001, -1.0
SENTINEL = -777.25
OUTPUTS = ("rgb", "depth", "acc", "weights", "d_raw_rgb", "d_raw_density", "g_dirs")
# one K per output: the smallest power of two >= twice the largest ratio of the table above (at least 1, never above 16).  With
# alpha = 1 - expf(-dd) in the forward kernel acc needed 128 and rgb 32: the rounding of expf near 1 has one sign over a ray's thin
# intervals and adds up; the kernel now takes -expm1f(-dd) (last column of the table: the ratios before that).
K = dict(rgb=2, depth=1, acc=2, weights=8, d_raw_rgb=1, d_raw_density=4, g_dirs=8, sem=2, d_logits=4, g_w=1)

Case = collections.namedtuple("Case", "S R opaque bg rgb regime grads g_dirs")
ALL = ("rgb", "depth", "acc", "w")


def _c(S, R, opaque, bg, rgb, regime, grads=ALL, g_dirs=True):
    return Case(S, R, bool(opaque), float(bg), bool(rgb), regime, tuple(grads) if rgb else ("w",), bool(g_dirs))


def _block(S):
    """every value of every axis at one S (the issue asks for it at S = 65 and S = 512)"""
    return [
        _c(S, 37, 1, 1, 1, "mixed"), _c(S, 37, 0, 1, 1, "mixed"), _c(S, 5, 0, 0, 1, "mixed", ("rgb", "depth"), False),
        _c(S, 1, 1, 0, 0, "mixed", g_dirs=False), _c(S, 5, 1, 1, 1, "mixed", ("depth",)),
        _c(S, 37, 1, 1, 1, "dense"), _c(S, 37, 0, 0, 1, "dense"), _c(S, 5, 0, 1, 0, "dense"),
        _c(S, 37, 1, 0, 1, "sparse"), _c(S, 37, 0, 1, 1, "sparse"), _c(S, 1, 0, 0, 0, "sparse", g_dirs=False),
        _c(S, 5, 0, 1, 1, "sparse", ("acc", "w"), False),
        _c(S, 37, 1, 1, 1, "empty"), _c(S, 37, 0, 1, 1, "empty"), _c(S, 5, 0, 0, 0, "empty"),
    ]


CASES = _block(65) + _block(512) + [
    _c(1, 37, 1, 1, 1, "mixed"), _c(1, 5, 0, 1, 1, "sparse"), _c(1, 1, 0, 0, 1, "empty"),
    _c(63, 37, 0, 1, 1, "mixed"), _c(63, 5, 1, 0, 1, "dense", ("rgb",)),
    _c(64, 37, 1, 1, 1, "mixed"), _c(64, 5, 0, 0, 1, "dense"), _c(64, 1, 0, 1, 0, "sparse"),
    _c(128, 37, 0, 0, 1, "mixed"), _c(128, 5, 1, 1, 0, "dense"),
    _c(129, 37, 0, 1, 1, "dense"), _c(129, 5, 1, 0, 1, "sparse", ("rgb", "depth")),
]
S513 = _c(513, 5, 1, 1, 1, "mixed")


def _id(c):
    return f"S{c.S}-R{c.R}-{'opq' if c.opaque else 'air'}-bg{c.bg:g}-{'rgb' if c.rgb else 'prop'}-{c.regime}-g{'+'.join(c.grads)}-{'gd' if c.g_dirs else 'nogd'}"


assert len({_id(c) for c in CASES}) == len(CASES)


@functools.lru_cache(maxsize=None)
def inputs(c):
    """fp32 inputs of a case.  buf4: the model's [P,4] buffer (raw rgb | raw density)."""
    g = torch.Generator().manual_seed(CASES.index(c) if c in CASES else 999)
    R, S = c.R, c.S
    near, far = 1.5 + torch.rand(R, generator=g), 5 + 50 * torch.rand(R, generator=g)
    u = 0.5 + torch.rand(R, S, generator=g).double()
    u[:, -1] += 4 if S > 1 else 0           # a wide last interval: an opaque ray with all its weight there stays 1e-3 inside td[S]
    cs = torch.cat([torch.zeros(R, 1, dtype=torch.float64), torch.cumsum(u, -1) / u.sum(-1, keepdim=True)], -1)
    td = (near[:, None].double() + (far - near)[:, None].double() * cs).float().contiguous()
    assert bool((td[:, 1:] > td[:, :-1]).all())
    dirs = torch.randn(R, 3, generator=g)
    dirs = (dirs / dirs.norm(dim=-1, keepdim=True) * (0.15 + 0.25 * torch.rand(R, 1, generator=g))).contiguous()
    buf4 = torch.randn(R * S, 4, generator=g)
    z = buf4[:, 3].clone().view(R, S)
    if c.regime == "mixed":
        z = z * 3
    elif c.regime == "dense":
        z = z - 6
        z[torch.arange(R), torch.randint(0, S, (R,), generator=g)] = 18.0
    elif c.regime == "sparse":
        z = z - 8
    else:
        z = torch.full_like(z, -30.0)
    buf4[:, 3] = z.reshape(-1)
    gs = dict(rgb=torch.randn(R, 3, generator=g), depth=torch.randn(R, generator=g) * 0.05, acc=torch.randn(R, generator=g),
              w=torch.randn(R, S, generator=g))
    return dict(td=td, dirs=dirs, buf4=buf4, g={k: (gs[k] if k in c.grads else None) for k in ALL})


@functools.lru_cache(maxsize=None)
def reference(c, dtype):
    """the oracle in `dtype` on the case's inputs: the seven outputs, computed once and shared (read-only)"""
    x = inputs(c)
    cv = lambda t: None if t is None else t.to(dtype)
    P = c.R * c.S
    raw_rgb = cv(x["buf4"][:, :3].contiguous()) if c.rgb else None
    raw_d, td, dirs = cv(x["buf4"][:, 3:4].contiguous()), cv(x["td"]), cv(x["dirs"])
    rgb, depth, acc, w = E.zip_composite_fwd(raw_rgb, raw_d, td, dirs, c.opaque, c.bg, RGB_PADDING, DENSITY_BIAS)
    d_rgb, d_den, g_dirs = torch.zeros(P, 3, dtype=dtype), torch.zeros(P, 1, dtype=dtype), torch.zeros(c.R, 3, dtype=dtype)
    E.zip_composite_bwd(raw_rgb, raw_d, td, dirs, c.opaque, c.bg, RGB_PADDING, DENSITY_BIAS, w, acc, depth, *[cv(x["g"][k]) for k in ALL],
                        d_rgb if c.rgb else None, d_den, g_dirs)
    out = dict(rgb=rgb, depth=depth, acc=acc, weights=w, d_raw_rgb=d_rgb if c.rgb else None, d_raw_density=d_den,
               g_dirs=g_dirs if c.g_dirs else None)
    for k, v in out.items():
        assert v is None or (v.dtype == dtype and bool(torch.isfinite(v).all())), (k, _id(c))
    return {k: (None if v is None else v.detach()) for k, v in out.items()}


def raw_depth(c, weights, dtype):
    """exp(E) before the clip, from a reference's own weights, and the clip ends"""
    td = inputs(c)["td"].to(dtype)
    Em = (weights * torch.log(0.5 * (td[:, :-1] + td[:, 1:]))).sum(-1) / weights.sum(-1).clamp_min(EPS32)
    return torch.exp(Em), td[:, 0], td[:, -1]


# ------------------------------------------------------------------ CPU: the inputs keep clear of the kinks ----
@pytest.mark.parametrize("c", CASES + [S513], ids=_id)
def test_inputs_keep_clear_of_the_kinks(c):
    r64, r32 = reference(c, torch.float64), reference(c, torch.float32)
    raw, lo, hi = raw_depth(c, r64["weights"], torch.float64)
    raw32, lo32, hi32 = raw_depth(c, r32["weights"], torch.float32)
    clipped = (raw < lo) | (raw > hi)
    if c.regime != "empty":
        assert bool(((raw >= lo * (1 + 1e-3)) & (raw <= hi * (1 - 1e-3))).all()), "a non-empty ray is within 1e-3 of the depth clip"
    elif not c.opaque:
        assert bool((raw < lo).all()) and bool((r64["depth"] == lo).all()), "an empty ray in air is clipped at td[0] (near > 1)"
    else:
        assert not bool(clipped.any())
    assert torch.equal(clipped, (raw32 < lo32) | (raw32 > hi32)), "fp32 and float64 disagree on which rays are clipped"
    if not c.opaque:
        assert bool((1 - r64["acc"] > 0).all()), "background clamp reached in float64"
    x = inputs(c)["buf4"][:, 3].double() + DENSITY_BIAS
    assert bool(((x - 20).abs() > 1e-3).all()), "a density sits on the softplus switch"


def test_case_table_covers_every_axis():
    assert 35 <= len(CASES) <= 45
    for S in (65, 512):
        at = [c for c in CASES if c.S == S]
        assert {c.R for c in at} == {1, 5, 37} and {c.opaque for c in at} == {True, False} and {c.bg for c in at} == {0.0, 1.0}
        assert {c.rgb for c in at} == {True, False} and {c.regime for c in at} == {"mixed", "dense", "sparse", "empty"}
        assert {c.g_dirs for c in at} == {True, False} and ALL in {c.grads for c in at} and len({c.grads for c in at}) >= 4
    assert {c.S for c in CASES} == {1, 63, 64, 65, 128, 129, 512} and all(c.R * c.S <= 37 * 512 for c in CASES)


# ------------------------------------------------------------------ GPU ----
@pytest.fixture(scope="module")
def ops():
    from snerf_amd import ops as _ops
    return _ops


def run_hip(ops, c, strided, backward=True):
    """forward, then the backward on the forward's own weights / acc / depth, as the model does.  strided: raw rgb / density are
    columns of one [P,4] buffer (the model's layout) and the gradients columns 0:3 / 3 of a sentinel-filled [P,5] one (a fifth
    column nobody owns, and a row stride that differs from the input's)."""
    x = inputs(c)
    P = c.R * c.S
    cu = lambda t: None if t is None else t.cuda().contiguous()
    buf4 = x["buf4"].cuda()
    if strided:
        raw_rgb, raw_d = (buf4[:, :3] if c.rgb else None), buf4[:, 3:4]
        dbuf = torch.full((P, 5), SENTINEL, device="cuda")
        d_rgb, d_den = (dbuf[:, :3] if c.rgb else None), dbuf[:, 3:4]
    else:
        raw_rgb, raw_d = (buf4[:, :3].contiguous() if c.rgb else None), buf4[:, 3:4].contiguous()
        dbuf = None
        d_rgb, d_den = (torch.full((P, 3), SENTINEL, device="cuda") if c.rgb else None), torch.full((P, 1), SENTINEL, device="cuda")
    td, dirs = cu(x["td"]), cu(x["dirs"])
    rgb, depth, acc, w = ops.zip_composite_fwd(raw_rgb, raw_d, td, dirs, c.opaque, c.bg, RGB_PADDING, DENSITY_BIAS)
    out = dict(rgb=rgb, depth=depth, acc=acc, weights=w, d_raw_rgb=None, d_raw_density=None, g_dirs=None)
    if backward:
        g_dirs = torch.full((c.R, 3), SENTINEL, device="cuda") if c.g_dirs else None
        ops.zip_composite_bwd(raw_rgb, raw_d, td, dirs, c.opaque, c.bg, RGB_PADDING, DENSITY_BIAS, w, acc, depth, *[cu(x["g"][k]) for k in ALL],
                              d_rgb, d_den, g_dirs=g_dirs)
        out.update(d_raw_rgb=d_rgb, d_raw_density=d_den, g_dirs=g_dirs)
    torch.cuda.synchronize()
    if dbuf is not None and backward:
        keep = dbuf[:, 4:] if c.rgb else torch.cat([dbuf[:, :3], dbuf[:, 4:]], 1)
        assert bool((keep == SENTINEL).all()), "the backward wrote a column it does not own"
    assert bool(torch.equal(buf4.cpu(), x["buf4"])), "the kernels changed their inputs"
    return {k: (None if v is None else v.cpu().contiguous()) for k, v in out.items()}


def errors(c, got):
    """per output: (e_ref, e_hip, floor, scale), max-abs errors against float64"""
    r64, r32 = reference(c, torch.float64), reference(c, torch.float32)
    rec = {}
    for k in OUTPUTS:
        if got[k] is None:
            continue
        scale = 1.0 if k in ("rgb", "acc", "weights") else float(inputs(c)["td"][:, -1].max()) if k == "depth" else float(r64[k].abs().max())
        assert got[k].shape == r64[k].shape and bool(torch.isfinite(got[k]).all()), f"{k}: shape or non-finite values"
        e_ref, e_hip = float((r32[k].double() - r64[k]).abs().max()), float((got[k].double() - r64[k]).abs().max())
        rec[k] = (e_ref, e_hip, FLOOR_EPS * EPS32 * scale, scale)
    return rec


def check_bound(rec, what):
    bad = [f"{k}: e_hip {h:.3e} > {K[k]} * e_ref {r:.3e} + floor {f:.3e}" for k, (r, h, f, _) in rec.items() if not h <= K[k] * r + f]
    for k, (r, h, f, s) in rec.items():
        print(f"{what} {k}: e_ref {r:.3e} e_hip {h:.3e} floor {f:.3e} ratio {max(h - f, 0) / r if r > 0 else 0.0:.2f}")
    assert not bad, f"{what}: " + "; ".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=_id)
def test_zip_composite_against_float64(ops, c):
    got = run_hip(ops, c, strided=True)
    same = run_hip(ops, c, strided=False)
    for k in OUTPUTS:
        assert (got[k] is None) == (same[k] is None) and (got[k] is None or torch.equal(got[k], same[k])), f"{k}: strided and contiguous runs differ in bits"
    if c.opaque:
        assert bool((got["d_raw_density"].view(c.R, c.S)[:, -1] == 0).all()), "the opaque last interval has alpha == 1 whatever its density"
    if c.regime != "empty":
        check_bound(errors(c, got), _id(c))
        return
    gmax = max(float(g.abs().max()) for g in inputs(c)["g"].values() if g is not None)
    grads = [got[k] for k in ("d_raw_rgb", "d_raw_density", "g_dirs") if got[k] is not None]
    assert all(bool(torch.isfinite(g).all()) for g in grads)
    if c.opaque:
        assert bool(((got["weights"][:, -1] - 1).abs() <= 1e-6).all()) and bool((got["weights"][:, :-1].abs() < 1e-10).all())
    else:
        assert bool((got["weights"].abs() < 1e-10).all()) and bool((got["acc"].abs() < 1e-10).all())
        assert bool(((got["rgb"] - c.bg).abs() <= 1e-6).all())
        assert torch.equal(got["depth"], inputs(c)["td"][:, 0]), "depth of an empty ray is td[0] exactly"
        assert all(float(g.abs().max()) < 1e-6 * gmax for g in grads)


@pytest.mark.gpu
def test_zip_composite_513_intervals(ops):
    """past 64 * ZMAXSEG: the backward refuses with the library's argument error and writes nothing; the forward has no such limit"""
    from snerf_amd import _lib
    c, x = S513, inputs(S513)
    got = run_hip(ops, c, strided=True, backward=False)
    check_bound(errors(c, got), _id(c))
    P = c.R * c.S
    cu = lambda t: None if t is None else t.cuda().contiguous()
    buf4, dbuf, g_dirs = x["buf4"].cuda(), torch.full((P, 5), SENTINEL, device="cuda"), torch.full((c.R, 3), SENTINEL, device="cuda")
    with pytest.raises(_lib.SnerfHipError, match="bad argument"):
        ops.zip_composite_bwd(buf4[:, :3], buf4[:, 3:4], cu(x["td"]), cu(x["dirs"]), c.opaque, c.bg, RGB_PADDING, DENSITY_BIAS, cu(got["weights"]),
                              cu(got["acc"]), cu(got["depth"]), *[cu(x["g"][k]) for k in ALL], dbuf[:, :3], dbuf[:, 3:4], g_dirs=g_dirs)
    torch.cuda.synchronize()
    assert bool((dbuf == SENTINEL).all()) and bool((g_dirs == SENTINEL).all()), "a refused call wrote to its outputs"


# ------------------------------------------------------------------ semantic compositing ----
SEM_LD, SEM_LD_D = 48, 40
SEM_SHAPES = [(C, S, R) for C in (1, 19, 32) for S in (1, 65, 200) for R in (1, 37)]
SEM_DTYPES = dict(f32=torch.float32, bf16=torch.bfloat16, f16=torch.float16)


@functools.lru_cache(maxsize=None)
def sem_inputs(C, S, R, dtype, softmax):
    g = torch.Generator().manual_seed(C * 1000 + S * 10 + R)
    P = R * S
    w = torch.rand(R, S, generator=g) ** 2
    buf = torch.full((P, SEM_LD), 3.0e4)                  # columns >= C: large finite junk a kernel must not read
    buf[:, :C] = torch.randn(P, C, generator=g) * 3
    if softmax:
        buf[0, C // 2] = buf[0, :C].max() + 80            # one logit 80 above the rest: exp underflows for the others
    buf = buf.to(dtype)
    g_sem = torch.randn(R, C, generator=g)
    # compacted evaluation: sample p reads row ri[p] of a permuted buffer, a fifth of the samples are skipped (-1)
    perm = torch.randperm(P, generator=g)
    ri = perm.clone().int()
    ri[torch.rand(P, generator=g) < 0.2] = -1
    pbuf = torch.empty_like(buf)
    pbuf[perm] = buf
    return dict(w=w, buf=buf, g_sem=g_sem, ri=ri.view(R, S), pbuf=pbuf)


def sem_reference(C, S, R, dtype, softmax, hp):
    x = sem_inputs(C, S, R, dtype, softmax)
    cv = (lambda t: t.double()) if hp else (lambda t: t)
    lg = x["buf"].double() if hp else x["buf"]            # float64 from the upcast 16-bit values; the fp32 oracle upcasts itself
    out = dict(sem=E.semantic_composite_fwd(cv(x["w"]), lg, C, softmax),
               sem_ri=E.semantic_composite_fwd(cv(x["w"]), x["pbuf"].double() if hp else x["pbuf"], C, softmax, row_index=x["ri"]))
    d = torch.zeros(R * S, C, dtype=torch.float64 if hp else torch.float32)
    out["g_w"] = E.semantic_composite_bwd(cv(x["w"]), lg, cv(x["g_sem"]), C, softmax, d, want_g_w=True)
    out["d_logits"] = d
    assert all(out[k].dtype == d.dtype for k in ("sem", "sem_ri", "d_logits"))
    return out


def sem_errors(ref64, ref32, got, keys):
    rec = {}
    for k in keys:
        kk = "sem" if k == "sem_ri" else k
        scale = float(ref64[k].abs().max())
        assert bool(torch.isfinite(got[k]).all())
        rec[k] = (kk, float((ref32[k].double() - ref64[k]).abs().max()), float((got[k].double() - ref64[k]).abs().max()), FLOOR_EPS * EPS32 * scale)
    return rec


def run_sem(ops, C, S, R, dtype, softmax):
    x = sem_inputs(C, S, R, dtype, softmax)
    P = R * S
    w, buf, g_sem = x["w"].cuda(), x["buf"].cuda(), x["g_sem"].cuda()
    got = dict(sem=ops.semantic_composite_fwd(w, buf, C, softmax), sem_ri=ops.semantic_composite_fwd(w, x["pbuf"].cuda(), C, softmax, row_index=x["ri"].cuda()))
    # d_logits: a [P, 40] view at the head of a [P, 48] allocation -- a row stride of its own, with room behind it
    alloc, alloc2 = torch.full((P * SEM_LD,), SENTINEL, device="cuda"), torch.full((P * SEM_LD,), SENTINEL, device="cuda")
    d_logits = alloc[:P * SEM_LD_D].view(P, SEM_LD_D)
    got["g_w"] = ops.semantic_composite_bwd(w, buf, g_sem, C, softmax, d_logits, want_g_w=True)
    assert ops.semantic_composite_bwd(w, buf, g_sem, C, softmax, alloc2[:P * SEM_LD_D].view(P, SEM_LD_D), want_g_w=False) is None
    torch.cuda.synchronize()
    assert torch.equal(alloc, alloc2), "d_logits depends on whether the weights' gradient is asked for"
    assert bool((d_logits[:, C:] == SENTINEL).all()) and bool((alloc[P * SEM_LD_D:] == SENTINEL).all()), "d_logits written outside its C columns"
    got["d_logits"] = d_logits[:, :C]
    return {k: v.cpu() for k, v in got.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("softmax", [1, 0], ids=["softmax", "identity"])
@pytest.mark.parametrize("dt", list(SEM_DTYPES))
def test_semantic_composite_against_float64(ops, dt, softmax):
    bad = []
    for C, S, R in SEM_SHAPES:
        args = (C, S, R, SEM_DTYPES[dt], softmax)
        got, r64, r32 = run_sem(ops, *args), sem_reference(*args, hp=True), sem_reference(*args, hp=False)
        keys = ["sem", "sem_ri", "d_logits"] + ([] if softmax else ["g_w"])
        if softmax:
            assert bool((got["g_w"] == 0).all()) and got["g_w"].shape == (R, S), "softmax flavour: no gradient to the weights"
        for k, (kk, r, h, f) in sem_errors(r64, r32, got, keys).items():
            print(f"sem {dt} softmax={softmax} C={C} S={S} R={R} {k}: e_ref {r:.3e} e_hip {h:.3e} floor {f:.3e} ratio {max(h - f, 0) / r if r > 0 else 0.0:.2f}")
            if not h <= K[kk] * r + f:
                bad.append(f"C={C} S={S} R={R} {k}: e_hip {h:.3e} > {K[kk]} * e_ref {r:.3e} + floor {f:.3e}")
    assert not bad, "; ".join(bad)


# ------------------------------------------------------------------ the table of the docstring ----
def measure():
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from snerf_amd import ops as _ops
    worst = collections.defaultdict(lambda: [0.0, 0.0, 0.0])
    for c in CASES + [S513]:
        if c.regime == "empty":
            continue
        for k, (r, h, f, s) in errors(c, run_hip(_ops, c, True, backward=c.S <= 512)).items():
            print(f"{_id(c)} {k}: e_ref {r:.3e} e_hip {h:.3e} floor {f:.3e} ratio {max(h - f, 0) / r if r > 0 else 0.0:.2f}")
            m = worst[(c.regime, k)]
            m[0], m[1], m[2] = max(m[0], r / (s or 1.0)), max(m[1], h / (s or 1.0)), max(m[2], max(h - f, 0) / r if r > 0 else 0.0)
    for dt in SEM_DTYPES:
        for softmax in (1, 0):
            for C, S, R in SEM_SHAPES:
                args = (C, S, R, SEM_DTYPES[dt], softmax)
                got, r64, r32 = run_sem(_ops, *args), sem_reference(*args, hp=True), sem_reference(*args, hp=False)
                for k, (kk, r, h, f) in sem_errors(r64, r32, got, ["sem", "sem_ri", "d_logits"] + ([] if softmax else ["g_w"])).items():
                    s = f / (FLOOR_EPS * EPS32) or 1.0
                    m = worst[(f"semantic {dt} {'softmax' if softmax else 'identity'}", kk)]
                    m[0], m[1], m[2] = max(m[0], r / s), max(m[1], h / s), max(m[2], max(h - f, 0) / r if r > 0 else 0.0)
    print(f"    {'regime':<26}{'output':<15}{'e_ref':>10}{'e_hip':>10}{'ratio':>7}")
    for (reg, k), (r, h, q) in worst.items():
        print(f"    {reg:<26}{k:<15}{r:>10.1e}{h:>10.1e}{q:>7.2f}")
    need = collections.defaultdict(float)
    for (reg, k), (r, h, q) in worst.items():
        need[k] = max(need[k], q)
    print("    largest ratio per output:", ", ".join(f"{k} {v:.2f}" for k, v in need.items()))


if __name__ == "__main__":
    measure()
