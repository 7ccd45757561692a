"""The mesh ray tracer (snerf_amd.meshtrace, csrc/meshtrace.hip: snerf_mesh_prepare / snerf_mesh_trace / snerf_mesh_trace_pinhole) and its
callers in snerf_amd.foreground (mesh_depth, mask_from_mesh, composite_frame with mesh=).

The reference is an all-pairs Moeller-Trumbore in float64 numpy (nearest t > 0 wins, no tolerance) on the fp32 vertices and rays the
kernels get.  Fixture F: an icosphere subdivided 4 times (2562 vertices, 5120 faces), scaled by (2.2, 0.8, 0.9), rotated 0.6 rad about
y, moved to (0.4, -0.3, -9), plus a two-triangle quad with corners (+-3, +-2, -14) behind it: 5122 faces = two groups, a ragged last
chunk, a second surface.  Camera 48 x 64, fx = fy = 80, cx = 31.3, cy = 24.7.

A ray is AMBIGUOUS when min(|u|, |v|, |1 - u - v|) over all triangles with a non-zero determinant is below 1e-4 in float64: it passes
within rounding of an edge line, where hit or miss is a coin toss in any fp32 code.  Ambiguous rays are left out of the parity
comparisons and every comparison asserts that it left out at most 3 %.

Depth bounds: 1e-5 relative on the pinhole routes (an fp32 numpy restatement of another formulation is 3.4e-7 off), 1e-4 on the general
route (the project's parity bound; the restatement: 9.2e-6)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from snerf_amd import _lib

gpu = pytest.mark.gpu
f32 = np.float32
H, W, FX, FY, CX, CY = 48, 64, 80., 80., 31.3, 24.7
SCALE, ANGLE, CENTRE = np.array([2.2, 0.8, 0.9]), 0.6, np.array([0.4, -0.3, -9.])
AMBIGUOUS, CAP = 1e-4, 0.03
T_MAX = 100.
built = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libsnerf_hip.so not built (run __graft_entry__.build())")


# ---- fixture and float64 reference ------------------------------------------------------------------------------------------------------
def icosphere(n):
    """the unit icosphere: the icosahedron on (0, +-1, +-phi) and its cyclic shifts, every edge split n times, vertices normalised"""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(n):
        cache, nf = {}, []

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                cache[k] = len(v) - 1
            return cache[k]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v), np.array(f, dtype=np.int64)


def placement(scale=SCALE, angle=ANGLE, centre=CENTRE):
    """the 3 x 4 map x -> R_y(angle) diag(scale) x + centre, float64"""
    c, s = np.cos(angle), np.sin(angle)
    rot = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return np.concatenate([rot @ np.diag(scale), np.asarray(centre, dtype=np.float64)[:, None]], 1)


QUAD = np.array([[-3, -2, -14], [3, -2, -14], [3, 2, -14], [-3, 2, -14.]])


def reference(o, d, V, F, chunk=256):
    """all-pairs Moeller-Trumbore in float64 -> (t of the nearest hit with t > 0 or inf, its face or -1, ambiguous, the unit normal of that
    face)"""
    o, d, V = np.asarray(o, np.float64), np.asarray(d, np.float64), np.asarray(V, np.float64)
    a, e1, e2 = V[F[:, 0]], V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]]
    R = len(d)
    tb, fb, amb = np.full(R, np.inf), np.full(R, -1), np.zeros(R, bool)
    for s in range(0, R, chunk):
        oo, dd = o[s:s + chunk, None], d[s:s + chunk, None]
        p = np.cross(dd, e2[None])
        det = (e1[None] * p).sum(-1)
        with np.errstate(all="ignore"):
            tv = oo - a[None]
            u = (tv * p).sum(-1) / det
            q = np.cross(tv, e1[None])
            v = (dd * q).sum(-1) / det
            t = (e2[None] * q).sum(-1) / det
        nz = det != 0
        m = np.minimum(np.minimum(np.abs(u), np.abs(v)), np.abs(1 - u - v))
        amb[s:s + chunk] = np.where(nz, m, np.inf).min(1) < AMBIGUOUS
        tt = np.where(nz & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0), t, np.inf)
        k = tt.argmin(1)
        tb[s:s + chunk] = tt[np.arange(len(k)), k]
        fb[s:s + chunk] = np.where(np.isfinite(tb[s:s + chunk]), k, -1)
    n = np.cross(e1, e2)
    n = n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-300)
    return dict(t=tb, face=fb, ambiguous=amb, normal=np.where(fb[:, None] >= 0, n[np.maximum(fb, 0)], 0.))


def pinhole_rays(centre, h=H, w=W):
    """the kernel's rays, operation by operation in fp32: d = (((x + c) - cx) / fx, -(((y + c) - cy) / fy), -1)"""
    x, y = np.meshgrid(np.arange(w, dtype=f32), np.arange(h, dtype=f32), indexing="xy")
    off = f32(0.5 if centre else 0.)
    dx = ((x + off) - f32(CX)) / f32(FX)
    dy = -(((y + off) - f32(CY)) / f32(FY))
    return np.stack([dx, dy, -np.ones_like(dx)], -1).reshape(-1, 3)


def general_rays():
    rng = np.random.default_rng(7)
    o = rng.normal(size=(2048, 3))
    o = CENTRE + 6 * o / np.linalg.norm(o, axis=1, keepdims=True)
    d = CENTRE + rng.uniform(-1, 1, (2048, 3)) * np.array([2.6, 1.2, 1.6]) - o
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 2, (2048, 1))
    return o.astype(f32), d.astype(f32)


@pytest.fixture(scope="module")
def scene():
    """fixture F, the three ray sets and their float64 answers, computed once and only read by the tests"""
    sv, sf = icosphere(4)
    P = placement()
    ev = sv @ P[:, :3].T + P[:, 3]
    V = np.concatenate([ev, QUAD]).astype(f32)
    F = np.concatenate([sf, [[2562, 2563, 2564], [2562, 2564, 2565]]])
    s = dict(sphere_v=sv, sphere_f=sf, V=V, F=F, P=P)
    for name, (o, d) in dict(integer=(None, pinhole_rays(False)), centre=(None, pinhole_rays(True)), general=general_rays()).items():
        o = np.zeros_like(d) if o is None else o
        s[name] = dict(o=o, d=d, **reference(o, d, V, F))
        for a in s[name].values():
            a.setflags(write=False)
    for a in (sv, sf, V, F, P):
        a.setflags(write=False)
    return s


# ---- 1. reference and fixture self-checks (no GPU) --------------------------------------------------------------------------------------------
def test_fixture_hit_counts_and_ambiguous_shares(scene):
    assert scene["sphere_v"].shape == (2562, 3) and scene["F"].shape == (5122, 3)
    assert int((scene["integer"]["face"] >= 0).sum()) == 786 and int((scene["centre"]["face"] >= 0).sum()) == 790
    for name in ("integer", "centre", "general"):
        share = scene[name]["ambiguous"].mean()
        print(f"ambiguous share of the {name} rays: {share:.4f}")
        assert share <= CAP, (name, share)
    assert 500 < int((scene["general"]["face"] >= 0).sum()) < 1500              # the general rays hit and miss


def test_reference_on_an_axis_aligned_quad():
    """a quad at z = -5 whose edges fall between pixel columns / rows: exactly the pixel rectangle, t = 5"""
    X = lambda c: 5 * (c - CX) / FX
    Y = lambda r: -5 * (r - CY) / FY
    V = np.array([[X(10.5), Y(5.5), -5], [X(20.5), Y(5.5), -5], [X(20.5), Y(15.5), -5], [X(10.5), Y(15.5), -5]])
    ref = reference(np.zeros((H * W, 3)), pinhole_rays(False), V, np.array([[0, 1, 2], [0, 2, 3]]))
    hit = (ref["face"] >= 0).reshape(H, W)
    want = np.zeros((H, W), bool)
    want[6:16, 11:21] = True
    assert np.array_equal(hit, want)
    assert np.abs(ref["t"][hit.reshape(-1)] - 5).max() < 1e-12


# ---- status checks without a GPU ------------------------------------------------------------------------------------------------------------
_HOST = (ctypes.c_char * 64)()
_A = (ctypes.addressof(_HOST) + 15) & ~15           # a 16-byte aligned host address: the checks never dereference it


def _status(name, **values):
    base = dict(vertices=_A, V=8, faces=_A, face_ids=None, F=100, transform=None, ws=_A, ws_bytes=1 << 30, stream=None, rays_o=_A, rays_d=_A,
                R=64, t_max=100., flags=0, depth=_A, face_id=_A, positions=None, normals=None, fx=80., fy=80., cx=31.3, cy=24.7, pixel_center=0,
                H=48, W=64, mask=None, miss_value=.1, hit=None)
    base.update(values)
    return getattr(_lib.load(), name)(*[base[arg] for _, arg in _lib.parse_header()[name]])


@built
def test_mesh_entries_refuse_bad_arguments_without_a_gpu():
    """every refusal is SNERF_ERR_ARG before any launch; F = 0 and R = 0 are SNERF_OK"""
    q = lambda F: _lib.query("snerf_mesh_ws_bytes", F)
    assert [q(F) for F in (-1, 0, 1, 64, 65, 5122)] == [0, 0, 5376, 5376, 8448, 253184]
    for bad in (dict(faces=None), dict(vertices=None), dict(ws=None), dict(ws=_A + 4), dict(F=-1), dict(V=-1), dict(ws_bytes=q(100) - 1), dict(ws_bytes=0)):
        assert _status("snerf_mesh_prepare", **bad) == 1, bad
    assert _status("snerf_mesh_prepare", F=0) == 0 and _status("snerf_mesh_prepare", F=0, faces=None, vertices=None, ws=None, ws_bytes=0) == 0
    for bad in (dict(rays_o=None), dict(rays_d=None), dict(depth=None), dict(ws=None), dict(ws=_A + 8), dict(R=-1), dict(F=-1), dict(t_max=0.),
                dict(t_max=-1.), dict(t_max=float("nan")), dict(t_max=float("inf")), dict(flags=4), dict(flags=-1)):
        assert _status("snerf_mesh_trace", **bad) == 1, bad
    assert _status("snerf_mesh_trace", R=0) == 0 and _status("snerf_mesh_trace", R=0, F=0, ws=None, rays_o=None, rays_d=None, depth=None) == 0
    for bad in (dict(depth=None), dict(ws=None), dict(ws=_A + 4), dict(H=-1), dict(W=-1), dict(F=-1), dict(H=65536, W=65536), dict(H=1 << 16, W=1 << 15),
                dict(t_max=0.), dict(t_max=-2.), dict(t_max=float("nan")), dict(fx=0.), dict(fy=float("inf")), dict(cx=float("nan")), dict(flags=8)):
        assert _status("snerf_mesh_trace_pinhole", **bad) == 1, bad
    assert _status("snerf_mesh_trace_pinhole", H=0) == 0 and _status("snerf_mesh_trace_pinhole", W=0, F=0, ws=None, depth=None) == 0


def test_construction_refuses_a_face_index_out_of_range():
    """the Python check runs before anything touches the device"""
    from snerf_amd import meshtrace
    order = meshtrace.morton_order(torch.tensor([[0., 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5], [6, 5, 5], [5, 6, 5]]), torch.tensor([[3, 4, 5], [0, 1, 2]]))
    assert order.tolist() == [1, 0]                                             # sorted along the diagonal
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="outside"):
            meshtrace.RayTracer(np.zeros((3, 3), f32), np.array([[0, 1, 3]]))
        with pytest.raises(ValueError, match="outside"):
            meshtrace.RayTracer(np.zeros((3, 3), f32), np.array([[0, -1, 2]]))


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def traced(scene):
    """fixture F through the three routes, once: the pinhole entry (integer pixels, pixel centres), the general entry on the same rays given
    explicitly, and the 2048 general rays; numpy copies, only read by the tests"""
    from snerf_amd import meshtrace
    rt = meshtrace.RayTracer(scene["V"], scene["F"])
    out = dict(tracer=rt)
    for name, centre in (("integer", False), ("centre", True)):
        depth, hit = rt.trace_pinhole(FX, FY, CX, CY, H, W, centre, want_hit=True)
        out[name + "_pinhole"] = dict(depth=depth.cpu().numpy().reshape(-1), hit=hit.cpu().numpy())
    for name in ("integer", "centre", "general"):
        pos, nrm, depth, face = rt.trace_ids(scene[name]["o"], scene[name]["d"])
        out[name] = dict(depth=depth.cpu().numpy(), face=face.cpu().numpy().astype(np.int64), pos=pos.cpu().numpy(), normal=nrm.cpu().numpy())
    torch.cuda.synchronize()
    return out


def _parity(ref, depth, face, bound, miss=T_MAX, what=""):
    """hit / miss, face id and depth against float64 on the unambiguous rays -> the largest relative depth error"""
    keep = ~ref["ambiguous"]
    assert 1 - keep.mean() <= CAP, (what, 1 - keep.mean())
    hit64 = ref["face"] >= 0
    hit = depth != f32(miss)
    assert np.array_equal(hit[keep], hit64[keep]), (what, int((hit != hit64)[keep].sum()))
    if face is not None:
        assert np.array_equal(face[keep], ref["face"][keep]), (what, int((face != ref["face"])[keep].sum()))
        assert np.array_equal(face >= 0, hit), what                             # face id and depth tell the same story on every ray
    sel = keep & hit64
    err = float((np.abs(depth[sel].astype(np.float64) - ref["t"][sel]) / ref["t"][sel]).max())
    print(f"{what}: {int(sel.sum())} hits compared, {int((~keep).sum())} ambiguous rays left out, max relative depth error {err:.3e}")
    assert err <= bound, (what, err)
    return err


@gpu
def test_parity_with_float64_on_fixture_f(scene, traced):
    """Measured on an MI355X, largest relative depth error on the unambiguous hits: pinhole entry 2.0e-7 (integer pixels, 772 hits, 37
    rays left out as ambiguous) and 4.9e-7 (pixel centres, 773 hits, 40 left out); the general entry on the same rays: the same figures
    (the same bits); the 2048 general rays 1.0e-6 (968 hits, 41 left out).  No hit / miss or face id differs from float64."""
    _parity(scene["integer"], traced["integer_pinhole"]["depth"], None, 1e-5, what="pinhole, integer pixels")
    _parity(scene["centre"], traced["centre_pinhole"]["depth"], None, 1e-5, what="pinhole, pixel centres")
    _parity(scene["integer"], traced["integer"]["depth"], traced["integer"]["face"], 1e-5, what="general entry, integer-pixel rays")
    _parity(scene["centre"], traced["centre"]["depth"], traced["centre"]["face"], 1e-5, what="general entry, pixel-centre rays")
    _parity(scene["general"], traced["general"]["depth"], traced["general"]["face"], 1e-4, what="general entry, 2048 rays")
    for name in ("integer", "centre", "general"):                              # positions and normals: o + t d, the face's unit normal; zero on a miss
        r, g = scene[name], traced[name]
        hit = g["face"] >= 0
        assert not g["pos"][~hit].any() and not g["normal"][~hit].any()
        want = r["o"].astype(np.float64) + g["depth"][:, None].astype(np.float64) * r["d"]
        assert np.abs(g["pos"][hit] - want[hit]).max() <= 4 * np.finfo(f32).eps * 16            # three fp32 operations on magnitudes < 16
        same = hit & (g["face"] == r["face"])
        assert np.abs(g["normal"][same] - r["normal"][same]).max() <= 1e-4      # fp32 cross product of edges ~0.1 long: cancellation ~1e-5


@gpu
def test_no_ray_leaks_through_vertices_and_edges(scene):
    """rays through every front-facing vertex and edge midpoint of the ellipsoid (2993; plain fp32 Moeller-Trumbore with u, v, w >= 0 lets
    300 of them through): every one hits, within 1e-3 of the point's depth.  Measured on an MI355X: no miss, largest error 1.9e-7."""
    from snerf_amd import meshtrace
    sv, sf, P = scene["sphere_v"], scene["sphere_f"], scene["P"]
    rot = P[:, :3] @ np.diag(1 / SCALE)
    n = (sv / SCALE) @ rot.T                                                    # the ellipsoid's normal at a vertex
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    ev = scene["V"][:2562].astype(np.float64)
    E = np.unique(np.sort(np.concatenate([sf[:, [0, 1]], sf[:, [1, 2]], sf[:, [2, 0]]]), 1), axis=0)
    nm = n[E[:, 0]] + n[E[:, 1]]
    nm /= np.linalg.norm(nm, axis=1, keepdims=True)
    p, nn = np.concatenate([ev, (ev[E[:, 0]] + ev[E[:, 1]]) / 2]), np.concatenate([n, nm])
    p = p[(nn * p).sum(1) / np.linalg.norm(p, axis=1) < -0.3]
    assert len(p) == 2993
    d = (p / -p[:, 2:3]).astype(f32)
    d[:, 2] = -1
    for rt in (meshtrace.RayTracer(scene["V"], scene["F"]), meshtrace.RayTracer(scene["V"][:2562], sf)):
        _, _, depth, face = rt.trace_ids(np.zeros_like(d), d)
        depth, face = depth.cpu().numpy().astype(np.float64), face.cpu().numpy()
        err = np.abs(depth - (-p[:, 2])) / (-p[:, 2])
        print(f"no-leak rays: {int((face < 0).sum())} misses, {int((err > 1e-3).sum())} leaks, max relative depth error {err.max():.3e}")
        assert (face >= 0).all() and (face < 5120).all()
        assert err.max() <= 1e-3


def _transform_bound(ref):
    """Baked vertices are the float64 placement rounded once (half an ulp); the kernel's placement is three products and three sums on
    magnitudes below 16: at most 3.5 ulp(16) = 3.5 * 2^-20 more per coordinate, 4 ulp in all, so a vertex moves by at most
    sqrt(3) * 4 * 2^-20 and the face's plane by no more along its normal: t moves by at most that over |n . d|, on top of the pinhole
    route's own 1e-5 t."""
    nd = np.abs((ref["normal"] * ref["d"].astype(np.float64)).sum(1))
    return 1e-5 * ref["t"] + np.sqrt(3) * 4 * 2. ** -20 / np.maximum(nd, 1e-300)


@gpu
def test_transform_is_applied_per_call(scene):
    """the unit icosphere (and the quad's pre-image) traced with the placement as `transform` = fixture F with baked vertices; a second
    transform on the same RayTracer gives that transform's answer.  Measured on an MI355X: depth errors up to 3.1e-6 absolute, at most
    0.019 of the bound of _transform_bound."""
    from snerf_amd import meshtrace
    P = scene["P"]
    inv = np.linalg.inv(P[:, :3])
    V0 = np.concatenate([scene["sphere_v"], (QUAD - P[:, 3]) @ inv.T]).astype(f32)
    rt = meshtrace.RayTracer(V0, scene["F"])
    P2 = placement(scale=(1.5, 1.1, 0.7), angle=-0.4, centre=(-0.8, 0.5, -7.))
    V2 = (V0.astype(np.float64) @ P2[:, :3].T + P2[:, 3]).astype(f32)
    d = scene["integer"]["d"]
    idx = np.arange(0, H * W, 3)                                                # every third ray: a third of the float64 work for the second placement
    ref1 = {k: v[idx] for k, v in scene["integer"].items()}
    ref2 = dict(d=d[idx], **reference(np.zeros_like(d[idx]), d[idx], V2, scene["F"]))
    assert ref2["ambiguous"].mean() <= CAP and 100 < (ref2["face"] >= 0).sum() < 1000
    assert (ref2["face"] != ref1["face"]).mean() > 0.1                          # the two placements really differ
    for ref, T in ((ref1, P), (ref2, P2), (ref1, torch.tensor(P).cuda())):
        pos, nrm, depth, face = rt.trace_ids(np.zeros_like(d), d, transform=T)
        depth, face = depth.cpu().numpy(), face.cpu().numpy()
        dp = rt.trace_pinhole(FX, FY, CX, CY, H, W, False, transform=T)[0].cpu().numpy().reshape(-1)
        assert np.array_equal(dp, depth)
        depth, face = depth[idx], face[idx]
        # a ray within 1e-4 of an edge line in barycentric terms is ambiguous; the vertices move by 1e-5 of an edge at most
        keep = ~ref["ambiguous"]
        hit64 = ref["face"] >= 0
        assert np.array_equal((face >= 0)[keep], hit64[keep]) and np.array_equal(face[keep], ref["face"][keep])
        assert (depth[face < 0] == f32(T_MAX)).all()
        sel = keep & hit64
        err = np.abs(depth[sel].astype(np.float64) - ref["t"][sel])
        print(f"transform: max depth error {err.max():.3e}, {(err / _transform_bound(ref)[sel]).max():.3f} of its bound")
        assert (err <= _transform_bound(ref)[sel]).all()


@gpu
def test_stage_semantics_mesh_depth_mask_and_composite(scene, traced):
    from snerf_amd import foreground as fgm, meshtrace
    K = np.array([[FX, 0, CX], [0, FY, CY], [0, 0, 1]])
    flip = np.array([1, -1, -1], f32)
    rt_flipped = meshtrace.RayTracer(scene["V"] * flip, scene["F"])              # mesh_in_cam_coord: the flip inside mesh_depth gives fixture F
    yy, xx = np.mgrid[:H, :W]
    m = (((yy - 22) / 14.) ** 2 + ((xx - 24) / 18.) ** 2 <= 1) | ((yy < 4) & (xx > 50))     # 837 pixels: 545 hits, 292 misses; 241 hits outside
    mask = (m[..., None].repeat(3, -1) * 255).astype(np.uint8)
    mask_c0 = mask.copy()
    mask_c0[..., 1:] = 255                                                      # only channel 0 decides
    fg = fgm.mesh_depth(rt_flipped, K, H, W, _dev(mask_c0)).cpu().numpy()
    want = traced["integer_pinhole"]["depth"].reshape(H, W)
    hit = want != f32(T_MAX)
    assert (m & hit).sum() > 300 and (m & ~hit).sum() > 100 and (~m & hit).sum() > 100
    assert (fg[~m] == 0).all() and (fg[m & ~hit] == f32(.1)).all() and np.array_equal(fg[m & hit], want[m & hit])
    # the same through `transform`: the unflipped fixture with the flip handed in (the flip is its own inverse)
    fg2 = fgm.mesh_depth(traced["tracer"], K, H, W, _dev(mask), transform=np.diag([1., -1, -1, 1])).cpu().numpy()
    assert np.array_equal(fg2, fg)
    # stage 0: pixel centres, the mesh as given, 255 where the ray hits
    mm = fgm.mask_from_mesh(traced["tracer"], (W, H), K).cpu().numpy()
    assert mm.shape == (H, W, 3) and mm.dtype == np.uint8 and set(np.unique(mm)) == {0, 255}
    keep = ~scene["centre"]["ambiguous"].reshape(H, W)
    assert np.array_equal((mm[..., 0] == 255)[keep], (scene["centre"]["face"] >= 0).reshape(H, W)[keep])
    assert np.array_equal(mm[..., 0], mm[..., 1]) and np.array_equal(mm[..., 0], mm[..., 2])
    assert np.array_equal(mm, traced["centre_pinhole"]["hit"])
    # composite_frame: mesh= and fg_depth=mesh_depth(...) give the same bits
    rng = np.random.default_rng(3)
    bg = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    depth = (rng.integers(256, 20 * 256, (H, W)) / 256.).astype(f32)            # in front of and behind the ellipsoid at z = 8 .. 10
    sem = rng.integers(0, 19, (H, W)).astype(np.uint8)
    image = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    mask2 = np.roll(mask, 5, axis=1)
    frames = []
    for with_mesh in (True, False):
        inst = []
        for mk in (mask, mask2):
            i = dict(image=_dev(image), mask=_dev(mk), category="vehicle", r=2)
            if with_mesh:
                i.update(mesh=(rt_flipped, None), intrinsic=K)
            else:
                i.update(fg_depth=fgm.mesh_depth(rt_flipped, K, H, W, _dev(mk)))
            inst.append(i)
        frames.append(fgm.composite_frame(_dev(bg), _dev(depth), _dev(sem), inst))
    for k in ("fuse", "mask", "bound", "occluded_mask", "depth", "semantic"):
        assert torch.equal(frames[0][k], frames[1][k]), k
    assert [float(o) for o in frames[0]["occlusion"]] == [float(o) for o in frames[1]["occlusion"]]
    assert 0.05 < float(frames[0]["occlusion"][0]) < 0.95                       # the depth test went both ways


@gpu
def test_degenerate_faces_and_rays_hit_nothing(scene, traced):
    """a zero-area face, a face with a NaN vertex, a face with an index out of range (past the Python check: the ops layer directly), a NaN
    ray and a zero-direction ray: none reports a hit, every other ray keeps its bits, the calls return SNERF_OK"""
    from snerf_amd import ops
    V = np.concatenate([scene["V"], [[np.nan, 0, -5]], [[-50, -50, -4], [50, -50, -4], [0, 60, -4]]]).astype(f32)   # 5126: NaN; 5127..9: a wall in front
    nV = len(V)
    extra = [[10, 10, 11], [10, 20, 10], [5127, 5128, 5126], [5127, 5128, nV + 7], [5127, -1, 5129], [5127, 5128, 5128]]
    F = np.concatenate([scene["F"], extra]).astype(np.int32)
    d = np.concatenate([scene["integer"]["d"], [[np.nan, 0, -1]], [[0, 0, 0]], [[0, np.inf, -1]]]).astype(f32)
    o = np.zeros_like(d)
    ws = ops.mesh_prepare(_dev(V), _dev(F))                                     # identity order: face ids are positions
    depth, face, pos, nrm = ops.mesh_trace(ws, len(F), _dev(o), _dev(d))
    depth, face = depth.cpu().numpy(), face.cpu().numpy()
    assert (face < 5122).all()                                                  # none of the six extra faces is ever hit
    assert (face[-3:] == -1).all() and (depth[-3:] == f32(T_MAX)).all() and not pos[-3:].any() and not nrm[-3:].any()
    assert np.array_equal(depth[:-3], traced["integer"]["depth"])               # the bits of the clean mesh in Morton order
    keep = ~scene["integer"]["ambiguous"]
    assert np.array_equal(face[:-3][keep], traced["integer"]["face"][keep])
    dp, _ = ops.mesh_trace_pinhole(ws, len(F), FX, FY, CX, CY, False, H, W)
    assert np.array_equal(dp.cpu().numpy().reshape(-1), traced["integer_pinhole"]["depth"])
    # a mesh of degenerate faces only, and no mesh at all: everything misses
    ws3 = ops.mesh_prepare(_dev(V), _dev(np.array(extra, np.int32)))
    for w, n in ((ws3, len(extra)), (None, 0)):
        assert (ops.mesh_trace(w, n, _dev(o), _dev(d))[1] == -1).all()
        assert (ops.mesh_trace_pinhole(w, n, FX, FY, CX, CY, True, H, W, miss_value=7., device="cuda")[0] == 7.).all()
    from snerf_amd import meshtrace
    empty = meshtrace.RayTracer(np.zeros((0, 3), f32), np.zeros((0, 3), np.int64))
    assert (empty.trace(o, d)[2] == T_MAX).all() and empty.trace(np.zeros((0, 3), f32), np.zeros((0, 3), f32))[2].shape == (0,)


@gpu
def test_runs_are_bit_identical_and_the_entries_share_their_routine(scene, traced):
    """two runs give the same bits; the pinhole entry and the general entry run ONE intersection routine (mt_hit), so on the same rays they
    agree bit for bit -- as do the flavour without LDS staging and the flavour without box culling"""
    from snerf_amd import ops
    rt = traced["tracer"]
    for name in ("integer", "centre"):
        assert np.array_equal(traced[name + "_pinhole"]["depth"], traced[name]["depth"]), name
    for name in ("integer", "general"):
        o, d = scene[name]["o"], scene[name]["d"]
        for flags in (0, ops.MESH_UNIFORM, ops.MESH_NO_CULL, ops.MESH_UNIFORM | ops.MESH_NO_CULL):
            pos, nrm, depth, face = rt.trace_ids(o, d, flags=flags)
            assert np.array_equal(depth.cpu().numpy(), traced[name]["depth"]) and np.array_equal(face.cpu().numpy(), traced[name]["face"]), (name, flags)
            assert np.array_equal(pos.cpu().numpy(), traced[name]["pos"]) and np.array_equal(nrm.cpu().numpy(), traced[name]["normal"])
    for flags in (ops.MESH_UNIFORM, ops.MESH_NO_CULL):
        dp = rt.trace_pinhole(FX, FY, CX, CY, H, W, True, flags=flags)[0].cpu().numpy().reshape(-1)
        assert np.array_equal(dp, traced["centre_pinhole"]["depth"]), flags
    # a ray's answer does not depend on its neighbours in the wave: the general rays in another order
    perm = np.random.default_rng(1).permutation(2048)
    _, _, depth, face = rt.trace_ids(scene["general"]["o"][perm], scene["general"]["d"][perm])
    assert np.array_equal(depth.cpu().numpy(), traced["general"]["depth"][perm]) and np.array_equal(face.cpu().numpy(), traced["general"]["face"][perm])
