"""mip_composite_fwd / _bwd and classic_composite_fwd / _bwd (csrc/composite.hip) against float64, stage-isolated.

Same structure and bound as tests/test_zip_composite_f64.py.  The references are the eager oracle of tests/cpu_ops_emulation.py run
twice on the same fp32 inputs: in float64 (the truth) and in float32 (what a careful fp32 implementation reaches).  Every output of
a kernel is bounded per case by the fp32 oracle's own distance from float64:

    e_hip <= K[output] * e_ref + FLOOR_EPS * eps32 * scale      (max-abs errors against float64)

scale: 1 for weights / acc / rgb, max t[S] (mip) or max z (classic) for distance / depth, max |float64 result| for disp and all
gradients.  The backward kernels get the float64 reference's weights / distance / acc / depth rounded to fp32, never the forward
kernel's outputs.  raw_* / d_raw_* are column views of wider buffers, as the models pass them.

The inputs keep clear of the kinks of the two functions (test_inputs_keep_clear_of_the_kinks checks every ray of every case): the
mip distance clip (the unclipped sum w t_mid is 1e-3 relative away from t[0] and t[S] and both references agree on which side it is;
mixed rays are inside, sparse and empty rays are clipped low -- those cases test the gate that drops g_dist), the softplus switch
at 20, the relu of the classic density and the classic disparity clamp.

Measured on an MI355X (e = max over the regime's cases of max-abs error / scale; ratio = largest per-case (e_hip - floor) / e_ref,
0 where e_hip is under the floor; `python tests/test_mip_classic_composite_f64.py` prints the first five columns).  The last two
columns are the ratios of the kernels as they were before this file existed, and of those kernels with nothing but
alpha = -expm1f(-x) (and, classic, q = expf(-x) + 1e-10f) in place of 1 - expf(-x):

    regime            output              e_ref     e_hip  ratio   before  expm1f only
    mip mixed         rgb               2.0e-06   2.1e-06   0.78     0.89         0.78
    mip mixed         distance          2.0e-07   1.2e-07   0.00     0.00         0.00
    mip mixed         acc               4.4e-07   3.2e-07   0.00     2.91         0.00
    mip mixed         weights           1.7e-06   1.7e-06   0.74     0.78         0.74
    mip mixed         d_raw_rgb         5.0e-05   2.8e-07   0.00     0.00         0.00
    mip mixed         d_raw_density     6.3e-05   6.4e-05   1.13     1.33         1.33
    mip mixed         g_dirs            1.3e-05   3.2e-05   7.01     7.01         7.01
    mip dense         rgb               1.8e-05   1.7e-05   1.03     1.17         1.03
    mip dense         distance          2.1e-05   2.1e-05   0.96    10.94         8.05
    mip dense         acc               3.2e-05   3.2e-05   0.96     2.28         1.10
    mip dense         weights           3.2e-05   3.2e-05   0.99     1.70         1.70
    mip dense         d_raw_rgb         1.7e-05   1.5e-07   0.00     0.00         0.00
    mip dense         d_raw_density     2.7e-05   2.6e-05   2.43    10.74        10.74
    mip dense         g_dirs            2.9e-05   2.7e-05   2.47     8.24         8.24
    mip sparse        rgb               7.0e-07   5.9e-08   0.00     4.95         0.00
    mip sparse        distance          2.3e-09   2.3e-09   0.00     0.00         0.00
    mip sparse        acc               1.3e-06   2.4e-08   0.00    10.89         0.00
    mip sparse        weights           3.6e-08   1.6e-08   0.00     0.00         0.00
    mip sparse        d_raw_rgb         1.5e-04   2.5e-07   0.00     0.00         0.00
    mip sparse        d_raw_density     1.9e-05   1.9e-05   3.51     3.51         3.51
    mip sparse        g_dirs            1.1e-06   1.3e-06   0.83     0.83         0.83
    mip empty         rgb               9.8e-13   9.8e-13   0.00     0.00         0.00
    mip empty         distance          2.4e-09   2.4e-09   0.00     0.00         0.00
    mip empty         acc               2.0e-12   1.3e-15   0.00     0.00         0.00
    mip empty         weights           1.6e-12   5.6e-17   0.00     0.00         0.00
    mip empty         d_raw_rgb         1.0e+00   1.8e-07   0.00     0.00         0.00
    mip empty         d_raw_density     3.6e-05   2.5e-05   0.71     0.71         0.71
    mip empty         g_dirs            4.8e-06   4.8e-06   0.90     0.90         0.90
    classic mixed     rgb               1.8e-07   1.4e-07   0.00     0.00         0.00
    classic mixed     disp              2.0e-07   1.8e-07   0.00     0.00         0.00
    classic mixed     acc               1.3e-07   1.5e-07   0.00     0.00         0.00
    classic mixed     weights           6.2e-08   4.9e-08   0.00     0.00         0.00
    classic mixed     depth             4.9e-08   3.8e-08   0.00     0.00         0.00
    classic mixed     d_rgb             6.5e-07   4.5e-07   0.00     0.00         0.00
    classic mixed     d_sigma           2.6e-07   4.5e-07   0.00     0.00         0.00
    classic dense     rgb               2.1e-07   1.2e-07   0.00     0.00         0.00
    classic dense     disp              1.7e-07   1.4e-07   0.00     0.00         0.00
    classic dense     acc               1.2e-07   1.2e-07   0.00     0.00         0.00
    classic dense     weights           6.2e-08   6.2e-08   0.00     0.00         0.00
    classic dense     depth             2.8e-08   3.3e-08   0.00     0.00         0.00
    classic dense     d_rgb             1.9e-07   1.4e-07   0.00     0.00         0.00
    classic dense     d_sigma           5.0e-07   4.6e-07   0.00     0.00         0.00
    classic sparse    rgb               7.0e-08   1.1e-07   0.00     0.00         0.00
    classic sparse    disp              5.6e-06   7.8e-08   0.00     0.91         0.00
    classic sparse    acc               5.1e-08   5.1e-08   0.00     0.00         0.00
    classic sparse    weights           7.9e-08   3.0e-08   0.00     0.00         0.00
    classic sparse    depth             7.3e-08   7.3e-08   0.00     0.00         0.00
    classic sparse    d_rgb             5.2e-06   1.0e-07   0.00     0.00         0.00
    classic sparse    d_sigma           4.5e-05   1.2e-06   1.01     1.01         1.01
    classic thin      rgb               6.8e-07   1.5e-07   0.00     6.35        12.20
    classic thin      disp              3.0e-06   1.8e-07   0.00     1.00         0.00
    classic thin      acc               9.9e-07   1.3e-07   0.00     9.10        45.26
    classic thin      weights           7.5e-07   3.3e-08   0.00     6.61         6.61
    classic thin      depth             8.0e-07   1.7e-07   0.00     8.18        29.06
    classic thin      d_rgb             3.2e-04   2.2e-07   0.00     0.00         0.00
    classic thin      d_sigma           1.4e-04   1.1e-05   0.26     9.12         9.12
    classic empty     rgb               0.0e+00   0.0e+00   0.00     0.00         0.00
    classic empty     disp              0.0e+00   0.0e+00   0.00     0.00         0.00
    classic empty     acc               0.0e+00   0.0e+00   0.00     0.00         0.00
    classic empty     weights           0.0e+00   0.0e+00   0.00     0.00         0.00
    classic empty     depth             0.0e+00   0.0e+00   0.00     0.00         0.00
    classic empty     d_rgb             0.0e+00   0.0e+00   0.00     0.00         0.00
    classic empty     d_sigma           0.0e+00   0.0e+00   0.00     0.00         0.00
    largest ratio per output, mip:     rgb 1.03, distance 0.96, acc 0.96, weights 0.99, d_raw_rgb 0.00, d_raw_density 3.51, g_dirs 7.01
    before:                            rgb 4.95, distance 10.94, acc 10.89, weights 1.70, d_raw_rgb 0.00, d_raw_density 10.74, g_dirs 8.24
    largest ratio per output, classic: rgb 0.00, disp 0.00, acc 0.00, weights 0.00, depth 0.00, d_rgb 0.00, d_sigma 1.01
    before:                            rgb 6.35, disp 1.00, acc 9.10, weights 6.61, depth 8.18, d_rgb 0.00, d_sigma 9.12
    expm1f only:                       rgb 12.20, disp 0.00, acc 45.26, weights 6.61, depth 29.06, d_rgb 0.00, d_sigma 9.12

Three things were behind the ratios above 8 (a K above 16), all fixed in csrc/composite.hip:
  * 1 - expf(-dd) in the mip forward: acc and rgb of sparse rays (10.89, 4.95), as in the zip kernel.
  * exclusive scans taken as inclusive - own value, in the mip forward (transmittance) and both backwards (suffix sum of g w): behind
    a dense sample the small sum keeps an error of eps * that sample's value.  distance 10.94, d_raw_density 10.74, g_dirs 8.24 of
    the dense regime; the kernels now take the neighbour lane's inclusive value.
  * the classic transmittance as a running product of q = 1 - alpha + 1e-10: every q just under 1 rounds by 3e-8 of the product, and
    the opaque last sample of a ray of 512 thin intervals had a weight off by 5e-6.  With 1 - expf the sum of the weights still
    telescoped (acc 9.10); with an exact alpha it no longer did (acc 45.26, column "expm1f only").  Both classic kernels now take
    exp of a running sum of log q.
g_dirs of one mixed case (S = 512, disparity spacing, g_dist alone) stays at 7.01 and has not been explained (g T_next and the suffix
sum nearly cancel on such a ray); it is inside the cap, K = 16.
"""
import collections
import functools
import os
import sys
import zlib

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pytest
import torch

import cpu_ops_emulation as E

EPS32 = 1.1920929e-07
FLOOR_EPS = 4                     # "a few fp32 epsilons" of the output's natural scale
RGB_PADDING, DENSITY_BIAS = 0.001, -1.0
SENTINEL = -777.25
OUTPUTS = dict(mip=("rgb", "distance", "acc", "weights", "d_raw_rgb", "d_raw_density", "g_dirs"),
               classic=("rgb", "disp", "acc", "weights", "depth", "d_rgb", "d_sigma"))      # d_rgb = d_raw[:, :3], d_sigma = d_raw[:, 3]
UNIT_SCALE, T_SCALE = ("rgb", "acc", "weights"), ("distance", "depth")
# one K per output: the smallest power of two >= twice the largest ratio of the table above (at least 1, never above 16)
K = dict(mip=dict(rgb=4, distance=2, acc=2, weights=2, d_raw_rgb=1, d_raw_density=8, g_dirs=16),
         classic=dict(rgb=1, disp=1, acc=1, weights=1, depth=1, d_rgb=1, d_sigma=4))

# one table for both families.  mip: tf = transform_idx, rgb = NeRF level (False: proposal level, no colour), g_dirs = wanted;
# classic: last = "open" (sigma < 0 at the last sample) or "closed" (sigma > 0: the 1e10 interval makes the ray opaque)
Case = collections.namedtuple("Case", "kind S R tf white rgb noise g_dirs grads last regime seed")
MIP_ALL, CLASSIC_ALL = ("rgb", "dist", "acc", "w"), ("rgb", "disp", "acc", "depth", "w")
MIP_REGIMES, CLASSIC_REGIMES = ("mixed", "dense", "sparse", "empty"), ("mixed", "dense", "sparse", "thin", "empty")


def _m(S, R, tf, white, rgb, noise, g_dirs, regime, grads=MIP_ALL, seed=0):
    grads = tuple(k for k in grads if rgb or k != "rgb")
    return Case("mip", S, R, tf, bool(white), bool(rgb), bool(noise), bool(g_dirs), grads, None, regime, seed)


def _k(S, R, white, noise, last, regime, grads=CLASSIC_ALL, seed=0):
    return Case("classic", S, R, None, bool(white), True, bool(noise), False, tuple(grads), last, regime, seed)


def _mip_block(S):
    """every value of every mip axis at one S"""
    return [
        _m(S, 37, 0, 1, 1, 1, 1, "mixed"), _m(S, 37, 1, 0, 1, 0, 1, "mixed"), _m(S, 5, 2, 1, 1, 1, 0, "mixed", ("rgb", "dist")),
        _m(S, 1, 0, 0, 0, 0, 0, "mixed", ("w",)), _m(S, 5, 1, 1, 1, 1, 1, "mixed", ("dist",)),
        _m(S, 37, 0, 1, 1, 0, 1, "dense"), _m(S, 37, 2, 0, 1, 1, 1, "dense"), _m(S, 5, 1, 1, 0, 1, 1, "dense", ("dist", "w")),
        _m(S, 37, 0, 0, 1, 1, 1, "sparse"), _m(S, 37, 1, 1, 1, 0, 1, "sparse"), _m(S, 37, 2, 1, 1, 1, 1, "sparse", ("dist",)),
        _m(S, 1, 0, 0, 0, 0, 0, "sparse", ("dist", "acc", "w")), _m(S, 5, 2, 1, 1, 1, 0, "sparse", ("acc", "w")),
        _m(S, 37, 0, 1, 1, 1, 1, "empty"), _m(S, 5, 1, 0, 0, 0, 1, "empty", ("dist", "w")),
    ]


def _classic_block(S):
    """every value of every classic axis at one S"""
    return [
        _k(S, 37, 1, 1, "open", "mixed"), _k(S, 37, 0, 0, "closed", "mixed"), _k(S, 5, 1, 0, "open", "mixed", ("rgb", "disp")),
        _k(S, 1, 0, 1, "closed", "mixed", ("depth", "w")),
        _k(S, 37, 1, 1, "closed", "dense"), _k(S, 5, 0, 0, "open", "dense", ("disp",)),
        _k(S, 37, 0, 1, "open", "sparse"), _k(S, 5, 1, 0, "closed", "sparse", ("acc", "w")),
        _k(S, 37, 1, 0, "open", "thin"), _k(S, 37, 0, 1, "closed", "thin"), _k(S, 5, 1, 1, "open", "thin", ("disp", "depth")),
        _k(S, 37, 1, 1, "open", "empty", ("rgb", "acc", "depth", "w")), _k(S, 1, 0, 0, "open", "empty", ("rgb", "w")),
    ]


CASES = _mip_block(65) + _mip_block(512) + [
    _m(1, 5, 2, 1, 1, 1, 1, "mixed"), _m(1, 37, 0, 1, 1, 0, 1, "dense"), _m(1, 37, 1, 0, 1, 1, 1, "sparse"), _m(1, 1, 0, 1, 1, 0, 0, "empty"),
    _m(63, 37, 0, 1, 1, 1, 1, "mixed"), _m(63, 5, 1, 0, 1, 0, 1, "dense", ("rgb",)),
    _m(64, 37, 2, 1, 1, 1, 1, "mixed"), _m(64, 5, 0, 0, 0, 1, 0, "sparse", ("dist", "w")),
    _m(128, 37, 1, 0, 1, 1, 1, "mixed"), _m(128, 5, 2, 1, 0, 0, 1, "dense"),
    _m(129, 37, 0, 1, 1, 1, 1, "dense"), _m(129, 5, 1, 0, 1, 1, 1, "sparse", ("rgb", "dist")),
] + _classic_block(65) + _classic_block(512) + [
    _k(1, 37, 1, 1, "closed", "mixed"), _k(1, 5, 0, 0, "open", "empty", ("rgb", "acc")),      # S = 1: an open ray is an empty one
    _k(63, 37, 0, 1, "open", "mixed"),
    _k(64, 37, 1, 1, "open", "thin"), _k(64, 5, 0, 0, "closed", "dense"),
    _k(128, 37, 1, 0, "open", "mixed"),
    _k(129, 37, 0, 1, "closed", "thin"), _k(129, 5, 1, 1, "open", "sparse", ("disp", "acc")),
]
S513 = [_m(513, 5, 0, 1, 1, 1, 1, "mixed"), _k(513, 5, 1, 1, "open", "mixed")]
ROW_INDEX = [_m(65, 37, 0, 1, 1, 1, 0, "mixed", seed=7), _m(129, 37, 2, 0, 1, 0, 0, "mixed", seed=7)]   # forward only, compacted rows


def _id(c):
    tail = f"g{'+'.join(c.grads)}-{c.regime}" + (f"-s{c.seed}" if c.seed else "")
    if c.kind == "mip":
        return (f"mip-S{c.S}-R{c.R}-tf{c.tf}-{'white' if c.white else 'black'}-{'rgb' if c.rgb else 'prop'}-{'noise' if c.noise else 'quiet'}-"
                f"{'gd' if c.g_dirs else 'nogd'}-{tail}")
    return f"classic-S{c.S}-R{c.R}-{'white' if c.white else 'black'}-{'noise' if c.noise else 'quiet'}-{c.last}-{tail}"


assert len({_id(c) for c in CASES + S513 + ROW_INDEX}) == len(CASES + S513 + ROW_INDEX)


def _gen(c):
    return torch.Generator().manual_seed(zlib.crc32(_id(c).encode()))


def _fence(g, R, n):
    """[R, n + 1] float64 fence posts in [0, 1] from a cumulative sum of 0.5 + U"""
    u = 0.5 + torch.rand(R, n, generator=g).double()
    cs = torch.cat([torch.zeros(R, 1, dtype=torch.float64), torch.cumsum(u, -1) / u.sum(-1, keepdim=True)], -1)
    cs[:, -1] = 1
    return cs


def _dirs(g, R):
    d = torch.randn(R, 3, generator=g)
    return (d / d.norm(dim=-1, keepdim=True) * (0.8 + 0.4 * torch.rand(R, 1, generator=g))).contiguous()


@functools.lru_cache(maxsize=None)
def inputs(c):
    """fp32 inputs of a case.  mip: buf4 is the model's [P,4] buffer (raw rgb | raw density); classic: raw is [P,5] (rgb | sigma |
    a column nobody reads, the width create_nerf uses with importance sampling)."""
    g = _gen(c)
    R, S = c.R, c.S
    if c.kind == "mip":
        near, far = 1.5 + torch.rand(R, generator=g), 5 + 50 * torch.rand(R, generator=g)
        s_vals = _fence(g, R, S).float().contiguous()
        assert bool((s_vals[:, 1:] > s_vals[:, :-1]).all())
        dirs = _dirs(g, R)
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
        noise = 0.1 * torch.randn(R, S, generator=g) if c.noise else None
        gs = dict(rgb=torch.randn(R, 3, generator=g), dist=torch.randn(R, generator=g) * 0.05, acc=torch.randn(R, generator=g),
                  w=torch.randn(R, S, generator=g))
        return dict(s_vals=s_vals, near=near, far=far, dirs=dirs, buf4=buf4, noise=noise, g={k: (gs[k] if k in c.grads else None) for k in MIP_ALL})
    near = 1.5 + torch.rand(R, generator=g).double()
    span = torch.full((R,), 1e-3 * S, dtype=torch.float64) if c.regime == "thin" else 3.5 + 5 * torch.rand(R, generator=g).double()
    z_vals = (near[:, None] + span[:, None] * (_fence(g, R, S - 1) if S > 1 else torch.zeros(R, 1, dtype=torch.float64))).float().contiguous()
    assert S == 1 or bool((z_vals[:, 1:] > z_vals[:, :-1]).all())
    rays_d = _dirs(g, R)
    raw = torch.randn(R * S, 5, generator=g)
    raw[:, 4] = 3.0e4
    n01, u01 = raw[:, 3].clone().view(R, S), torch.rand(R, S, generator=g)
    if c.regime == "thin":                                          # sigma * dist around 1e-6 .. 1e-4 per interval: 1 - exp cancels
        noise = 1e-3 * torch.rand(R, S, generator=g) if c.noise else None
        sig = 4e-3 * 20 ** u01
    else:
        noise = 0.1 * torch.randn(R, S, generator=g) if c.noise else None
        sig = dict(mixed=3 * n01, dense=2 + 8 * u01, sparse=n01 - 3, empty=-1 - u01)[c.regime]
    nz = noise if noise is not None else torch.zeros(R, S)
    if c.regime == "sparse" and S > 1:                              # one faint hit per ray: no ray of a non-empty regime is empty
        rows, hit = torch.arange(R), torch.randint(0, S - 1, (R,), generator=g)
        sig[rows, hit] = 0.05 + 0.2 * torch.rand(R, generator=g) - nz[rows, hit]
    if c.regime != "empty":
        sig[:, -1] = (0.5 + u01[:, -1]) * (1 if c.last == "closed" else -1) - nz[:, -1]
    near0 = (sig + nz).abs() < 2e-3                                 # off the relu kink
    sig[near0] += 0.01
    raw[:, 3] = sig.reshape(-1)
    gs = dict(rgb=torch.randn(R, 3, generator=g), disp=torch.randn(R, generator=g), acc=torch.randn(R, generator=g),
              depth=torch.randn(R, generator=g) * 0.1, w=torch.randn(R, S, generator=g))
    return dict(z_vals=z_vals, rays_d=rays_d, raw=raw, noise=noise, g={k: (gs[k] if k in c.grads else None) for k in CLASSIC_ALL})


@functools.lru_cache(maxsize=None)
def compaction(c):
    """row_index of a ROW_INDEX case and its compacted [M,4] buffer: about 40 % of the samples dropped, two whole rays among them, one
    ray that keeps only its last sample; the kept samples' rows are a random permutation"""
    g = torch.Generator().manual_seed(c.S)
    keep = torch.rand(c.R, c.S, generator=g) > 0.4
    keep[3], keep[11], keep[5] = False, False, False
    keep[5, -1] = True
    M = int(keep.sum())
    rows = torch.randperm(M, generator=g)
    ri = torch.full((c.R, c.S), -1, dtype=torch.int32)
    ri[keep] = rows.int()
    buf = torch.empty(M, 4)
    buf[rows] = inputs(c)["buf4"][keep.reshape(-1)]
    return ri, buf


@functools.lru_cache(maxsize=None)
def reference(c, dtype):
    """the oracle in `dtype` on the case's inputs, computed once and shared (read-only).  Keys with a leading underscore are not
    kernel outputs: _tmax (the scale of distance / depth) and, for mip, the unclipped distance and the clip ends."""
    x = inputs(c)
    cv = lambda t: None if t is None else t.to(dtype)
    P = c.R * c.S
    if c.kind == "mip":
        buf4, ri = x["buf4"], None
        if c in ROW_INDEX:
            ri, buf4 = compaction(c)
        raw_rgb, raw_d = (cv(buf4[:, :3].contiguous()) if c.rgb else None), cv(buf4[:, 3:4].contiguous())
        args = (cv(x["noise"]), cv(x["s_vals"]), cv(x["dirs"]), cv(x["near"]), cv(x["far"]), c.tf, c.white, RGB_PADDING, DENSITY_BIAS)
        rgb, dist, acc, w = E.mip_composite_fwd(raw_rgb, raw_d, *args, row_index=ri)
        t = E.om.transform(args[1], args[3][:, None], args[4][:, None], c.tf)
        out = dict(rgb=rgb, distance=dist, acc=acc, weights=w, _tmax=t[:, -1].max(), _raw=(w * 0.5 * (t[:, :-1] + t[:, 1:])).sum(-1),
                   _lo=t[:, 0], _hi=t[:, -1])
        if ri is None:
            d_rgb, d_den, g_dirs = torch.zeros(P, 3, dtype=dtype), torch.zeros(P, 1, dtype=dtype), torch.zeros(c.R, 3, dtype=dtype)
            E.mip_composite_bwd(raw_rgb, raw_d, *args, w, dist, *[cv(x["g"][k]) for k in MIP_ALL], d_rgb if c.rgb else None, d_den, g_dirs)
            out.update(d_raw_rgb=d_rgb if c.rgb else None, d_raw_density=d_den, g_dirs=g_dirs if c.g_dirs else None)
    else:
        args = (cv(x["raw"]), cv(x["noise"]), cv(x["z_vals"]), cv(x["rays_d"]), c.white)
        rgb, disp, acc, w, depth = E.classic_composite_fwd(*args)
        d_raw = torch.zeros(P, 5, dtype=dtype)
        E.classic_composite_bwd(*args, w, acc, depth, *[cv(x["g"][k]) for k in CLASSIC_ALL], d_raw)
        assert bool((d_raw[:, 4] == 0).all())
        out = dict(rgb=rgb, disp=disp, acc=acc, weights=w, depth=depth, d_rgb=d_raw[:, :3], d_sigma=d_raw[:, 3], _tmax=args[2].max())
    for k, v in out.items():
        assert v is None or v.dtype == dtype, (k, _id(c))
        assert v is None or bool(torch.isfinite(v).all()) or (k == "disp" and c.regime == "empty"), (k, _id(c))
    return {k: (None if v is None else v.detach()) for k, v in out.items()}


# ------------------------------------------------------------------ CPU: the inputs keep clear of the kinks ----
@pytest.mark.parametrize("c", CASES + S513 + ROW_INDEX, ids=_id)
def test_inputs_keep_clear_of_the_kinks(c):
    r64, r32, x = reference(c, torch.float64), reference(c, torch.float32), inputs(c)
    if c.kind == "mip":
        side = lambda r: (r["_raw"] > r["_hi"]).long() - (r["_raw"] < r["_lo"]).long()
        raw, lo, hi = r64["_raw"], r64["_lo"], r64["_hi"]
        assert bool(((raw - lo).abs() >= 1e-3 * lo).all()) and bool(((raw - hi).abs() >= 1e-3 * hi).all()), "a ray is within 1e-3 of the distance clip"
        assert torch.equal(side(r64), side(r32)), "fp32 and float64 disagree on which rays are clipped"
        inside = side(r64) == 0
        if c not in ROW_INDEX:
            if c.regime == "mixed":
                assert bool(inside.all()), "a ray of the mixed regime is clipped"
            elif c.regime == "dense":
                assert float(inside.double().mean()) >= 0.25, "fewer than a quarter of a dense case's rays are inside the clip"
            else:
                assert bool((side(r64) == -1).all()), "a sparse or empty ray is not clipped low"
        z = x["buf4"][:, 3].double() + (0 if x["noise"] is None else x["noise"].reshape(-1).double()) + DENSITY_BIAS
        assert bool(((z - 20).abs() > 1e-3).all()), "a density sits on the softplus switch"
        return
    sig = x["raw"][:, 3].view(c.R, c.S).double() + (0 if x["noise"] is None else x["noise"].double())
    assert bool((sig.abs() > 1e-3).all()), "a density sits on the relu kink"
    if c.regime == "empty":
        assert bool((sig < 0).all()) and "disp" not in c.grads and c.last == "open"
        for r in (r64, r32):
            assert bool((r["acc"] == 0).all()) and bool(torch.isnan(r["disp"]).all())
        return
    assert bool((sig[:, -1] > 0).all() if c.last == "closed" else (sig[:, -1] < 0).all())
    assert bool((sig > 0).any(-1).all()), "a ray of a non-empty regime is empty"
    for r in (r64, r32):
        assert bool((r["acc"] > 0).all()) and bool((r["depth"] / r["acc"] > 1e-3).all()), "disparity clamp"
    if c.last == "closed":
        assert bool(((r64["acc"] - 1).abs() < 1e-6).all()), "a closed last sample makes the ray opaque"
    if c.regime == "thin" and c.S > 1:
        dist = (x["z_vals"][:, 1:] - x["z_vals"][:, :-1]).double() * x["rays_d"].double().norm(dim=-1, keepdim=True)
        xx = sig[:, :-1] * dist
        assert bool((xx > 5e-7).all()) and bool((xx < 3e-4).all()), "thin: sigma * dist around 1e-6 .. 1e-4"


def test_case_table_covers_every_axis():
    mip, classic = [c for c in CASES if c.kind == "mip"], [c for c in CASES if c.kind == "classic"]
    assert 35 <= len(mip) <= 45 and 25 <= len(classic) <= 35
    for S in (65, 512):
        at = [c for c in mip if c.S == S]
        assert {c.R for c in at} == {1, 5, 37} and {c.tf for c in at} == {0, 1, 2} and {c.white for c in at} == {True, False}
        assert {c.rgb for c in at} == {True, False} and {c.noise for c in at} == {True, False} and {c.g_dirs for c in at} == {True, False}
        assert {c.regime for c in at} == set(MIP_REGIMES) and MIP_ALL in {c.grads for c in at} and len({c.grads for c in at}) >= 4
        assert any("dist" in c.grads for c in at if c.regime == "sparse") and any("dist" in c.grads for c in at if c.regime == "empty")
        at = [c for c in classic if c.S == S]
        assert {c.R for c in at} == {1, 5, 37} and {c.white for c in at} == {True, False} and {c.noise for c in at} == {True, False}
        assert {c.last for c in at} == {"open", "closed"} and {c.regime for c in at} == set(CLASSIC_REGIMES)
        assert CLASSIC_ALL in {c.grads for c in at} and len({c.grads for c in at}) >= 4
    for cs in (mip, classic):
        assert {c.S for c in cs} == {1, 63, 64, 65, 128, 129, 512}
    assert all(c.R * c.S <= 37 * 512 and c.grads for c in CASES)


# ------------------------------------------------------------------ GPU ----
@pytest.fixture(scope="module")
def ops():
    from snerf_amd import ops as _ops
    return _ops


def _cu(t):
    return None if t is None else t.cuda().contiguous()


def mip_args(c):
    """device arguments of both mip entries: raw rgb / density are columns of one [P,4] buffer (the model's layout)"""
    x = inputs(c)
    buf4 = (compaction(c)[1] if c in ROW_INDEX else x["buf4"]).cuda()
    return buf4, ((buf4[:, :3] if c.rgb else None), buf4[:, 3:4], _cu(x["noise"]), _cu(x["s_vals"]), _cu(x["dirs"]), _cu(x["near"]), _cu(x["far"]),
                  c.tf, c.white, RGB_PADDING, DENSITY_BIAS)


def mip_bwd_buffers(c):
    """the gradients are columns 1:4 / 6 of a sentinel-filled [P,8] buffer: a row stride that differs from the input's"""
    dbuf = torch.full((c.R * c.S, 8), SENTINEL, device="cuda")
    return dbuf, (dbuf[:, 1:4] if c.rgb else None), dbuf[:, 6:7], (torch.full((c.R, 3), SENTINEL, device="cuda") if c.g_dirs else None)


def run_mip(ops, c, backward=True):
    x, r64 = inputs(c), reference(c, torch.float64)
    buf4, args = mip_args(c)
    before = buf4.clone()
    ri = _cu(compaction(c)[0]) if c in ROW_INDEX else None
    rgb, dist, acc, w = ops.mip_composite_fwd(*args, row_index=ri)
    out = dict(rgb=rgb, distance=dist, acc=acc, weights=w, d_raw_rgb=None, d_raw_density=None, g_dirs=None)
    if backward:
        dbuf, d_rgb, d_den, g_dirs = mip_bwd_buffers(c)
        ops.mip_composite_bwd(*args, _cu(r64["weights"].float()), _cu(r64["distance"].float()), *[_cu(x["g"][k]) for k in MIP_ALL],
                              d_rgb, d_den, g_dirs=g_dirs)
        out.update(d_raw_rgb=d_rgb, d_raw_density=d_den, g_dirs=g_dirs)
        own = torch.zeros(8, dtype=torch.bool)
        own[6] = True
        own[1:4] = c.rgb
        assert bool((dbuf[:, ~own.cuda()] == SENTINEL).all()), "the backward wrote a column it does not own"
    torch.cuda.synchronize()
    assert torch.equal(buf4, before), "the kernels changed their inputs"
    return {k: (None if v is None else v.cpu().contiguous()) for k, v in out.items()}


def classic_args(c):
    x = inputs(c)
    return _cu(x["raw"]), _cu(x["noise"]), _cu(x["z_vals"]), _cu(x["rays_d"]), c.white


def run_classic(ops, c, backward=True):
    x, r64 = inputs(c), reference(c, torch.float64)
    args = classic_args(c)
    before = args[0].clone()
    rgb, disp, acc, w, depth = ops.classic_composite_fwd(*args)
    out = dict(rgb=rgb, disp=disp, acc=acc, weights=w, depth=depth, d_rgb=None, d_sigma=None)
    if backward:
        d_raw = torch.full((c.R * c.S, 5), SENTINEL, device="cuda")
        ops.classic_composite_bwd(*args, *[_cu(r64[k].float()) for k in ("weights", "acc", "depth")], *[_cu(x["g"][k]) for k in CLASSIC_ALL], d_raw)
        assert bool((d_raw[:, 4] == SENTINEL).all()), "the backward wrote a column it does not own"
        out.update(d_rgb=d_raw[:, :3], d_sigma=d_raw[:, 3])
    torch.cuda.synchronize()
    assert torch.equal(args[0], before), "the kernels changed their inputs"
    return {k: (None if v is None else v.cpu().contiguous()) for k, v in out.items()}


def run_hip(ops, c, backward=True):
    return (run_mip if c.kind == "mip" else run_classic)(ops, c, backward)


def errors(c, got):
    """per output: (e_ref, e_hip, floor, scale), max-abs errors against float64.  NaN (disp of an empty classic ray) must sit at the same
    positions in both references and the kernel's output; the rest is compared."""
    r64, r32 = reference(c, torch.float64), reference(c, torch.float32)
    rec = {}
    for k in OUTPUTS[c.kind]:
        if got[k] is None:
            continue
        a64, a32, h = r64[k], r32[k].double(), got[k].double()
        assert h.shape == a64.shape, f"{k}: shape"
        nan = torch.isnan(a64)
        assert torch.equal(nan, torch.isnan(a32)) and torch.equal(nan, torch.isnan(h)), f"{k}: NaN at other positions than the reference's"
        a64, a32, h = a64[~nan], a32[~nan], h[~nan]
        assert bool(torch.isfinite(h).all()), f"{k}: non-finite values"
        if a64.numel() == 0:
            rec[k] = (0.0, 0.0, 0.0, 0.0)
            continue
        scale = 1.0 if k in UNIT_SCALE else float(r64["_tmax"]) if k in T_SCALE else float(a64.abs().max())
        rec[k] = (float((a32 - a64).abs().max()), float((h - a64).abs().max()), FLOOR_EPS * EPS32 * scale, scale)
    return rec


def _ratio(r, h, f):
    return max(h - f, 0) / r if r > 0 else (0.0 if h <= f else float("inf"))


def check_bound(c, rec, what):
    Kc = K[c.kind]
    bad = [f"{k}: e_hip {h:.3e} > {Kc[k]} * e_ref {r:.3e} + floor {f:.3e}" for k, (r, h, f, _) in rec.items() if not h <= Kc[k] * r + f]
    for k, (r, h, f, s) in rec.items():
        print(f"{what} {k}: e_ref {r:.3e} e_hip {h:.3e} floor {f:.3e} ratio {_ratio(r, h, f):.2f}")
    assert not bad, f"{what}: " + "; ".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=_id)
def test_composite_against_float64(ops, c):
    check_bound(c, errors(c, run_hip(ops, c)), _id(c))


@pytest.mark.gpu
@pytest.mark.parametrize("c", ROW_INDEX, ids=_id)
def test_mip_composite_fwd_row_index(ops, c):
    """compacted rows: a sample with row -1 has density 0 and no colour, every other sample reads its row of the compacted arrays"""
    ri = compaction(c)[0]
    assert 0.3 < float((ri < 0).float().mean()) < 0.5 and bool((ri[3] < 0).all()) and int((ri[5] >= 0).sum()) == 1 and int(ri[5, -1]) >= 0
    got = run_hip(ops, c, backward=False)
    assert bool((got["weights"][ri < 0] == 0).all()), "a sample that was not evaluated has weight"
    check_bound(c, errors(c, got), _id(c))


@pytest.mark.gpu
@pytest.mark.parametrize("c", S513, ids=_id)
def test_composite_513_samples(ops, c):
    """past 64 * MAXSEG: the backward refuses with the library's argument error and writes nothing; the forward has no such limit"""
    from snerf_amd import _lib
    x = inputs(c)
    got = run_hip(ops, c, backward=False)
    check_bound(c, errors(c, got), _id(c))
    with pytest.raises(_lib.SnerfHipError, match="bad argument"):
        if c.kind == "mip":
            dbuf, d_rgb, d_den, g_dirs = outs = mip_bwd_buffers(c)
            ops.mip_composite_bwd(*mip_args(c)[1], _cu(got["weights"]), _cu(got["distance"]), *[_cu(x["g"][k]) for k in MIP_ALL], d_rgb, d_den, g_dirs=g_dirs)
        else:
            outs = [torch.full((c.R * c.S, 5), SENTINEL, device="cuda")]
            ops.classic_composite_bwd(*classic_args(c), *[_cu(got[k]) for k in ("weights", "acc", "depth")], *[_cu(x["g"][k]) for k in CLASSIC_ALL], outs[0])
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in outs if t is not None), "a refused call wrote to its outputs"


@pytest.mark.gpu
def test_classic_empty_rays_with_g_disp_get_zero_gradients(ops):
    """The kernel's contract where the reference has none of its own: on a ray with acc == 0 disp is NaN (0 / 0), and with g_disp given
    NaN enters the reference's backward pass (what comes out depends on how autograd masks the relu: this torch gives zeros).  The
    backward kernel skips the disparity term there and writes exact zeros, so that the trainer never receives NaN from an empty ray;
    the other rays of the batch are not affected."""
    c = _k(65, 5, 1, 1, "open", "mixed", seed=3)
    x = inputs(c)
    raw = x["raw"].clone()
    nz = x["noise"]
    empty = torch.tensor([True, False, True, False, False])
    raw.view(c.R, c.S, 5)[empty, :, 3] = -1.0 - nz[empty].abs()
    args64 = (raw.double(), nz.double(), x["z_vals"].double(), x["rays_d"].double(), c.white)
    r64 = E.classic_composite_fwd(*args64)
    d64 = torch.zeros(c.R * c.S, 5, dtype=torch.float64)
    E.classic_composite_bwd(*args64, r64[3], r64[2], r64[4], *[x["g"][k].double() for k in CLASSIC_ALL], d64)
    d64 = d64.view(c.R, c.S, 5)
    assert bool(torch.isnan(r64[1][empty]).all()) and bool(torch.isfinite(d64[~empty]).all()) and not bool((d64[empty] != 0).any())
    args = (_cu(raw), _cu(nz), _cu(x["z_vals"]), _cu(x["rays_d"]), c.white)
    rgb, disp, acc, w, depth = ops.classic_composite_fwd(*args)
    assert torch.equal(torch.isnan(disp).cpu(), empty) and bool((acc.cpu()[empty] == 0).all())
    d_raw = torch.full((c.R * c.S, 5), SENTINEL, device="cuda")
    ops.classic_composite_bwd(*args, w, acc, depth, *[_cu(x["g"][k]) for k in CLASSIC_ALL], d_raw)
    torch.cuda.synchronize()
    d = d_raw.cpu().view(c.R, c.S, 5)
    assert bool((d[empty][..., :4] == 0).all()), "an empty ray gets exact zeros"
    assert bool((d[..., 4] == SENTINEL).all())
    # rays are independent: the other rays' gradients are what the kernel gives for a batch without the empty ones
    keep = (~empty).cuda()
    sub = lambda t: t[keep].contiguous()                                    # per-ray tensors, [R, ...]
    d_sub = torch.full((int(keep.sum()) * c.S, 5), SENTINEL, device="cuda")
    ops.classic_composite_bwd(sub(args[0].view(c.R, c.S, 5)).view(-1, 5), sub(args[1]), sub(args[2]), sub(args[3]), c.white, sub(w), sub(acc), sub(depth),
                              *[sub(_cu(x["g"][k])) for k in CLASSIC_ALL], d_sub)
    assert torch.equal(d_sub.cpu().view(-1, c.S, 5), d[~empty]), "an empty ray in the batch changed another ray's gradient"
    assert bool(torch.isfinite(d[~empty][..., :4]).all()) and float(d[~empty][..., 3].abs().max()) > 0


# ------------------------------------------------------------------ the table of the docstring ----
def measure():
    from snerf_amd import ops as _ops
    worst = collections.defaultdict(lambda: [0.0, 0.0, 0.0])
    for c in CASES + S513 + ROW_INDEX:
        for k, (r, h, f, s) in errors(c, run_hip(_ops, c, backward=c.S <= 512 and c not in ROW_INDEX)).items():
            print(f"{_id(c)} {k}: e_ref {r:.3e} e_hip {h:.3e} floor {f:.3e} ratio {_ratio(r, h, f):.2f}")
            m = worst[(f"{c.kind} {c.regime}", k)]
            m[0], m[1], m[2] = max(m[0], r / (s or 1.0)), max(m[1], h / (s or 1.0)), max(m[2], _ratio(r, h, f))
    print(f"    {'regime':<18}{'output':<15}{'e_ref':>10}{'e_hip':>10}{'ratio':>7}")
    for (reg, k), (r, h, q) in worst.items():
        print(f"    {reg:<18}{k:<15}{r:>10.1e}{h:>10.1e}{q:>7.2f}")
    for kind in OUTPUTS:
        need = collections.defaultdict(float)
        for (reg, k), (r, h, q) in worst.items():
            if reg.startswith(kind):
                need[k] = max(need[k], q)
        print(f"    largest ratio per output, {kind}:", ", ".join(f"{k} {v:.2f}" for k, v in need.items()))


if __name__ == "__main__":
    measure()
