"""The mesh renderer (snerf_amd.meshrender, csrc/meshtrace.hip: snerf_mesh_render_pinhole / snerf_mesh_render_scratch_bytes) and
foreground.composite_frame with render= instances.

Fixture: the mesh of test_mesh_trace.py (icosphere subdivided 4 times, scaled, rotated, placed at (0.4, -0.3, -9), plus the quad at
z = -14: 5122 faces), camera fx = fy = 80, cx = 31.3, cy = 24.7, pixel-centre rays, frames 48 x 64 and 45 x 61 (ragged tiles).
Vertex colours 0.5 + 0.5 sin(0.37 i), sin(1.13 i + 1), sin(2.71 i + 2); uvs default_rng(3).uniform(-2, 3) (so `% 1` matters) with some
face_uvs_idx at -1; three materials (a random 37 x 53 8-bit map / 255, a 1 x 1 constant, a random 16 x 9 float map) and a
face_material_idx that also holds the value 3 >= M.

Oracle: that file's all-pairs float64 Moeller-Trumbore for the nearest face, float64 barycentrics of that face, float64 interpolation,
and `torch.nn.functional.grid_sample` in float64 on the CPU called exactly as s-nerfpp/api_code/mesh_renderer.py:76-85 calls it.  A
pixel is AMBIGUOUS under that file's definition (within 1e-4 of an edge line); ambiguous pixels are left out of value comparisons and
every comparison asserts that it left out at most 3 %.

Bound on image_f: 5e-4 absolute.  An fp32 numpy restatement of the kernel's edge-function barycentrics, run on the CPU, is 5.0e-5
(vertex colours) and 3.2e-4 (this fixture's three materials) off the oracle.  Both are the 5.2e-5 of barycentric cancellation on these
pixel-sized triangles: a colour differs by at most 1 across a triangle, while the uvs of a triangle's corners are independent random
numbers here, about half the 53-texel map apart, over texels of full 8-bit contrast.  The bound is far below any convention error (a
half-texel shift, a flipped v or a permuted vertex move a random texture by more than 1e-2)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from snerf_amd import _lib, meshrender
from test_mesh_trace import CAP, CX, CY, FX, FY, QUAD, icosphere, pinhole_rays, placement, reference

gpu = pytest.mark.gpu
f32 = np.float32
built = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libsnerf_hip.so not built (run __graft_entry__.build())")
FRAMES = ((48, 64), (45, 61))
BOUND = 5e-4
MISS = 77.


# ---- fixture and float64 oracle -----------------------------------------------------------------------------------------------------------
def bary64(d, V, F, face):
    """float64 barycentrics [n,3] of vertices (a, b, c) of `face` [n] where the rays d [n,3] from the origin meet its plane"""
    d, V = np.asarray(d, np.float64), np.asarray(V, np.float64)
    a, e1, e2 = V[F[face, 0]], V[F[face, 1]] - V[F[face, 0]], V[F[face, 2]] - V[F[face, 0]]
    p = np.cross(d, e2)
    det = (e1 * p).sum(-1)
    tv = -a
    u = (tv * p).sum(-1) / det
    v = (d * np.cross(tv, e1)).sum(-1) / det
    return np.stack([1 - u - v, u, v], -1)


def shade_colours(b, F, face, colours):
    """sum_j b_j colour[F[face, j]] in float64, clamped to [0, 1]"""
    return np.clip(np.einsum("nj,njc->nc", b, np.asarray(colours, np.float64)[F[face]]), 0, 1)


def shade_textures(b, face, uvs, face_uvs_idx, materials, face_material_idx):
    """mesh_renderer.py:65-87 in float64: uvs [U,2] (already % 1) with a zero row appended for index -1, the interpolated uv, then for every
    material i `grid_sample(materials[i], (2u - 1, -(2v - 1)), mode='bilinear', align_corners=False, padding_mode='border')` on the
    pixels whose face has material i; pixels whose face matches no material stay 0"""
    uvz = np.concatenate([np.asarray(uvs, np.float64), np.zeros((1, 2))])
    fu = np.where(face_uvs_idx < 0, len(uvz) - 1, face_uvs_idx)
    uv = np.einsum("nj,njc->nc", b, uvz[fu[face]])
    img = np.zeros((len(face), 3))
    mat = face_material_idx[face]
    for i, m in enumerate(materials):
        sel = mat == i
        if sel.any():
            tc = torch.from_numpy(uv[sel] * 2. - 1.)
            tc[:, 1] = -tc[:, 1]
            val = torch.nn.functional.grid_sample(m.double(), tc.reshape(1, 1, -1, 2), mode="bilinear", align_corners=False, padding_mode="border")
            img[sel] = val[0, :, 0].permute(1, 0).numpy()
    return np.clip(img, 0, 1)


def to_u8(x):
    """torchvision's save_image: floor(255 x + 0.5)"""
    return np.floor(255. * x + 0.5).astype(np.uint8)


def attributes(nV, nF, F):
    i = np.arange(nV, dtype=np.float64)
    colours = np.stack([0.5 + 0.5 * np.sin(0.37 * i), 0.5 + 0.5 * np.sin(1.13 * i + 1), 0.5 + 0.5 * np.sin(2.71 * i + 2)], 1).astype(f32)
    uvs = np.random.default_rng(3).uniform(-2, 3, (nV, 2)).astype(f32)
    fu = F.copy()
    fu[::19, 1] = -1                                                            # one corner without a uv
    fu[5::23] = -1                                                             # whole faces without uvs: the constant sample at uv (0, 0)
    rng = np.random.default_rng(11)
    materials = [torch.from_numpy(rng.integers(0, 256, (1, 3, 37, 53)).astype(f32) / f32(255.)),
                 torch.tensor([0.3137, 0.77123, 0.05551]).reshape(1, 3, 1, 1),
                 torch.from_numpy(rng.uniform(0, 1, (3, 16, 9)).astype(f32))]
    g = (np.arange(nF) // 40) % 8
    fm = np.where(g == 1, 1, np.where(g == 2, 2, np.where(g == 3, 3, 0)))       # 3 >= M = 3: no material matches
    return colours, uvs, fu, materials, fm


def materials4(materials):
    return [m if m.dim() == 4 else m[None] for m in materials]


@pytest.fixture(scope="module")
def scene():
    """the mesh, its attributes and the float64 answers of both frames, computed once and only read by the tests"""
    sv, sf = icosphere(4)
    P = placement()
    V = np.concatenate([sv @ P[:, :3].T + P[:, 3], QUAD]).astype(f32)
    F = np.concatenate([sf, [[2562, 2563, 2564], [2562, 2564, 2565]]])
    colours, uvs, fu, materials, fm = attributes(len(V), len(F), F)
    uvs1 = (torch.from_numpy(uvs) % 1.).numpy()                                 # the reference takes % 1 in fp32 at load time
    s = dict(V=V, F=F, colours=colours, uvs=uvs, uvs1=uvs1, fu=fu, materials=materials, fm=fm, sphere_v=sv)
    for h, w in FRAMES:
        d = pinhole_rays(True, h, w)
        ref = reference(np.zeros_like(d), d, V, F)
        hit = ref["face"] >= 0
        face = ref["face"][hit]
        b = bary64(d[hit], V, F, face)
        col, tex = np.zeros((h * w, 3)), np.zeros((h * w, 3))
        col[hit] = shade_colours(b, F, face, colours)
        tex[hit] = shade_textures(b, face, uvs1, fu, materials4(materials), fm)
        s[(h, w)] = dict(d=d, t=ref["t"], face=ref["face"], ambiguous=ref["ambiguous"], hit=hit, colour=col, texture=tex)
    return s


# ---- 1. oracle self-checks (no GPU) -----------------------------------------------------------------------------------------------------------
def test_fixture_hit_counts_and_ambiguous_shares(scene):
    assert scene["F"].shape == (5122, 3)
    for h, w in FRAMES:
        r = scene[(h, w)]
        share = r["ambiguous"].mean()
        print(f"{h} x {w}: {int(r['hit'].sum())} hits, ambiguous share {share:.4f}")
        assert int(r["hit"].sum()) == 790 and share <= CAP
        mat = scene["fm"][r["face"][r["hit"]]]
        assert all((mat == i).sum() > 20 for i in range(4)), [(mat == i).sum() for i in range(4)]       # every material and the value >= M are seen
        nouv = (scene["fu"][r["face"][r["hit"]]] < 0)
        assert nouv.all(1).sum() >= 5 and (nouv.any(1) & ~nouv.all(1)).sum() >= 5                       # faces without uvs, faces with one corner without


def test_oracle_on_a_quad_with_affine_attributes():
    """a quad at z = -5 with colours and uvs affine in (x, y): every covered pixel has a closed-form value.  Bilinear sampling of a ramp
    texture (r = x / (Wm - 1), g = y / (Hm - 1)) is the unnormalised coordinate itself: ix = u Wm - 0.5, iy = (1 - v) Hm - 0.5, clipped"""
    h, w = 48, 64
    X = lambda c: 5 * (c - CX) / FX
    Y = lambda r: -5 * (r - CY) / FY
    V = np.array([[X(10), Y(5), -5], [X(20), Y(5), -5], [X(20), Y(15), -5], [X(10), Y(15), -5]])
    F = np.array([[0, 1, 2], [0, 2, 3]])
    d = pinhole_rays(True, h, w)
    ref = reference(np.zeros_like(d), d, V, F)
    hit = ref["face"] >= 0
    want = np.zeros((h, w), bool)
    want[5:15, 10:20] = True                                                    # pixel centres x + .5 between the edges at 10 and 20
    assert np.array_equal(hit.reshape(h, w), want)
    b = bary64(d[hit], V, F, ref["face"][hit])
    assert np.abs(b.sum(1) - 1).max() < 1e-12 and b.min() > -1e-12
    px, py = 5 * d[hit, 0].astype(np.float64), 5 * d[hit, 1].astype(np.float64)           # the hit point
    A = np.array([[0.11, -0.07, 0.5], [0.05, 0.09, 0.4], [-0.08, 0.02, 0.6]])               # colour = A (x, y, 1)
    colours = np.stack([V[:, 0], V[:, 1], np.ones(4)], 1) @ A.T
    got = shade_colours(b, F, ref["face"][hit], colours)
    assert np.abs(got - np.stack([px, py, np.ones_like(px)], 1) @ A.T).max() < 1e-12
    s, t = (V[:, 0] - V[0, 0]) / (V[1, 0] - V[0, 0]), (V[:, 1] - V[3, 1]) / (V[0, 1] - V[3, 1])      # uv = (s, t) in [0, 1]^2 across the quad
    Hm, Wm = 7, 12
    yy, xx = np.mgrid[:Hm, :Wm]
    ramp = torch.from_numpy(np.stack([xx / (Wm - 1), yy / (Hm - 1), np.full((Hm, Wm), 0.25)])[None])
    fu = np.array([[0, 1, 2], [0, -1, 3]])                                      # the -1 is vertex 2 (uv (1, 0)) of the second face: uv (0, 0) there
    uvs = np.stack([s, t], 1)
    got = shade_textures(b, ref["face"][hit], uvs, F, [ramp], np.zeros(2, np.int64))
    u, v = (px - V[0, 0]) / (V[1, 0] - V[0, 0]), (py - V[3, 1]) / (V[0, 1] - V[3, 1])
    ix, iy = np.clip(u * Wm - 0.5, 0, Wm - 1), np.clip((1 - v) * Hm - 0.5, 0, Hm - 1)
    assert np.abs(got - np.stack([ix / (Wm - 1), iy / (Hm - 1), np.full_like(ix, 0.25)], 1)).max() < 1e-12
    got_z = shade_textures(b, ref["face"][hit], uvs, fu, [ramp], np.array([0, 0]))          # the appended zero row, and a material nobody has
    second = ref["face"][hit] == 1
    assert np.array_equal(got_z[~second], got[~second]) and np.abs(got_z[second] - got[second]).max() > 1e-2
    assert not shade_textures(b, ref["face"][hit], uvs, F, [ramp], np.array([1, -1])).any()
    assert np.array_equal(to_u8(np.array([0., 0.5 / 255 - 1e-9, 0.5 / 255, 1.])), [0, 0, 1, 255])


# ---- 2. statuses without a GPU ---------------------------------------------------------------------------------------------------------------
_HOST = (ctypes.c_char * 64)()
_A = (ctypes.addressof(_HOST) + 15) & ~15           # a 16-byte aligned host address: the checks never dereference it


def _status(**values):
    base = dict(ws=_A, F=100, fx=80., fy=80., cx=31.3, cy=24.7, H=48, W=64, t_max=100., miss_value=100., flags=0, faces=_A, vertex_color=_A, V=8,
                uvs=None, U=0, face_uvs_idx=None, face_material_idx=None, texels=None, n_texels=0, materials=None, M=0, validate=1, scratch=_A,
                scratch_bytes=1 << 30, image=_A, image_f=None, mask=None, depth=None, face_id=None, stream=None)
    base.update(values)
    return _lib.load().snerf_mesh_render_pinhole(*[base[arg] for _, arg in _lib.parse_header()["snerf_mesh_render_pinhole"]])


TEXTURED = dict(faces=None, vertex_color=None, V=0, uvs=_A, U=8, face_uvs_idx=_A, face_material_idx=_A, texels=_A, n_texels=64, materials=_A, M=2)


@built
def test_render_entries_refuse_bad_arguments_without_a_gpu():
    """every refusal is SNERF_ERR_ARG before any launch; H = 0, W = 0 are SNERF_OK"""
    q = lambda h, w: _lib.query("snerf_mesh_render_scratch_bytes", h, w)
    assert [q(*s) for s in ((0, 5), (5, 0), (-1, 8), (1, 1), (8, 8), (9, 8), (48, 64), (45, 61))] == [0, 0, 0, 24, 24, 32, 16 + 8 * 48, 16 + 8 * 48]
    for bad in (dict(F=-1), dict(H=-1), dict(W=-1), dict(V=-1), dict(U=-1), dict(n_texels=-1), dict(H=65536, W=65536), dict(H=1 << 16, W=1 << 15),
                dict(fx=0.), dict(fy=0.), dict(fx=float("nan")), dict(fy=float("inf")), dict(cx=float("nan")), dict(cy=float("inf")),
                dict(t_max=0.), dict(t_max=-2.), dict(t_max=float("nan")), dict(t_max=float("inf")), dict(flags=4), dict(flags=-1), dict(image=None),
                dict(ws=None), dict(ws=_A + 4), dict(vertex_color=None), dict(faces=None), dict(face_uvs_idx=_A, face_material_idx=_A, materials=_A, M=1),
                dict(scratch=None), dict(scratch=_A + 4), dict(scratch_bytes=q(48, 64) - 1), dict(scratch_bytes=0)):
        assert _status(**bad) == 1, bad
    for bad in (dict(M=0), dict(M=-1), dict(materials=None), dict(materials=_A + 8), dict(face_material_idx=None), dict(texels=None), dict(texels=_A + 4),
                dict(uvs=None), dict(vertex_color=_A, faces=_A), dict(ws=None), dict(image=None)):
        assert _status(**{**TEXTURED, **bad}) == 1, bad
    # valid without a launch: an empty frame (nothing is looked at but the numbers), in either mode
    assert _status(H=0) == 0 and _status(W=0, image=None, ws=None, scratch=None) == 0 and _status(**TEXTURED, H=0, image=None) == 0
    assert _status(F=0, H=0, ws=None, faces=None, vertex_color=None) == 0      # no mesh: the attribute arguments are not looked at
    assert _status(F=0, H=0, ws=None, faces=None, vertex_color=None, flags=8) == 1 and _status(H=0, fx=0.) == 1 and _status(H=0, vertex_color=None) == 1


# ---- 3. MeshRenderer's checks and reorder logic on the CPU ------------------------------------------------------------------------------------
@built
def test_constructor_checks_and_reorders_on_the_cpu(scene):
    V, F = scene["V"], scene["F"]
    kw = dict(uvs=scene["uvs"], face_uvs_idx=scene["fu"], materials=scene["materials"], face_material_idx=scene["fm"], device="cpu")
    r = meshrender.MeshRenderer(V, F, **kw)
    order = r.tracer.face_ids.long().numpy()
    assert sorted(order.tolist()) == list(range(len(F))) and not np.array_equal(order, np.arange(len(F)))
    assert np.array_equal(r.tracer.faces.numpy(), F[order]) and np.array_equal(r.face_uvs_idx.numpy(), scene["fu"][order])
    assert np.array_equal(r.face_material_idx.numpy(), scene["fm"][order]) and r.face_uvs_idx.dtype == torch.int32
    assert np.array_equal(r.uvs.numpy(), scene["uvs1"]) and 0 <= r.uvs.min() and r.uvs.max() < 1 and not np.array_equal(scene["uvs"], scene["uvs1"])
    assert r.materials.tolist() == [[0, 37, 53, 0], [37 * 53, 1, 1, 0], [37 * 53 + 1, 16, 9, 0]] and tuple(r.texels.shape) == (37 * 53 + 1 + 144, 4)
    m0 = scene["materials"][0][0]
    assert torch.equal(r.texels[5 * 53 + 7, :3], m0[:, 5, 7]) and torch.equal(r.texels[37 * 53, :3], scene["materials"][1].reshape(3))
    assert torch.equal(r.texels[37 * 53 + 1 + 3 * 9 + 2, :3], scene["materials"][2][:, 3, 2]) and not r.texels[:, 3].any()
    r0 = meshrender.MeshRenderer(V, F, uvs=scene["uvs"], face_uvs_idx=scene["fu"], materials=scene["materials"], device="cpu")
    assert not r0.face_material_idx.any()                                       # mesh_renderer.py:159
    rc = meshrender.MeshRenderer(V, F, vertex_color=scene["colours"], device="cpu")
    assert rc.uvs is None and torch.equal(rc.vertex_color, torch.from_numpy(scene["colours"]))
    for bad in (dict(), dict(vertex_color=scene["colours"], uvs=scene["uvs"]), dict(vertex_color=scene["colours"][:-1]), dict(vertex_color=scene["colours"][:, :2]),
                dict(uvs=scene["uvs"]), dict(uvs=scene["uvs"], face_uvs_idx=scene["fu"]), {**kw, "uvs": np.zeros((4, 3), f32)}, {**kw, "face_uvs_idx": scene["fu"][:-1]},
                {**kw, "face_material_idx": scene["fm"][:-1]}, {**kw, "materials": []}, {**kw, "materials": [torch.zeros(1, 4, 2, 2)]},
                {**kw, "materials": [torch.zeros(3, 0, 2)]}):
        with pytest.raises(ValueError):
            meshrender.MeshRenderer(V, F, **{"device": "cpu", **bad})
    with pytest.raises(ValueError, match="outside"):
        meshrender.MeshRenderer(V, np.array([[0, 1, len(V)]]), vertex_color=scene["colours"], device="cpu")


def _check_center_mesh_bottom(scene, device):
    """mesh_renderer.py:14-34 restated in float64 torch on the CPU; 1e-6 of the result's size"""
    v = (scene["sphere_v"] * np.array([2.2, 0.8, 0.9]) + np.array([0.3, 0.2, -0.5])).astype(f32)
    for category, length, want_l in (("vehicle", None, 4.5), ("vehicle", 4.43, 4.43), ("person", None, 1.7), ("bicycle", None, 1.6), ("motorcycle", None, 2.),
                                     ("object", None, None)):
        x = torch.from_numpy(v).double()
        lo, hi = x.min(dim=0, keepdim=True)[0], x.max(dim=0, keepdim=True)[0]
        x = x - (hi + lo) / 2.
        l0 = (hi - lo).max()
        x[:, 1] = x[:, 1] - x[:, 1].min()
        x = x * ((l0 if want_l is None else want_l) / l0)
        src = torch.from_numpy(v).to(device)
        got = meshrender.center_mesh_bottom(src, category, length)
        assert got.device == src.device and got.dtype == torch.float32 and torch.equal(src.cpu(), torch.from_numpy(v))      # the input is left alone
        got = got.cpu().double()
        err = float((got - x).abs().max() / x.abs().max())
        print(f"center_mesh_bottom {category} {length}: relative error {err:.2e}")
        assert err <= 1e-6
        assert float(got[:, 1].min()) == 0. and abs(float(got[:, 0].max() + got[:, 0].min())) <= 1e-6 * float(x.abs().max())
        if want_l is not None:
            assert abs(float((got.max(0)[0] - got.min(0)[0]).max()) - want_l) <= 1e-6 * want_l * 4


def test_center_mesh_bottom_on_the_cpu(scene):
    _check_center_mesh_bottom(scene, "cpu")


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


WANT = ("image_f", "depth", "face_id")


@pytest.fixture(scope="module")
def rendered(scene):
    """both renderers, both frames, once: numpy copies that the tests only read"""
    rc = meshrender.MeshRenderer(scene["V"], scene["F"], vertex_color=scene["colours"])
    rt = meshrender.MeshRenderer(scene["V"], scene["F"], uvs=scene["uvs"], face_uvs_idx=scene["fu"], materials=scene["materials"], face_material_idx=scene["fm"])
    out = dict(colour_renderer=rc, texture_renderer=rt)
    for mode, r in (("colour", rc), ("texture", rt)):
        for h, w in FRAMES:
            image, mask, extra = r.render(FX, FY, CX, CY, h, w, miss_value=MISS, want=WANT)
            out[(mode, h, w)] = dict(image=image.cpu().numpy(), mask=mask.cpu().numpy(), **{k: v.cpu().numpy() for k, v in extra.items()})
    torch.cuda.synchronize()
    return out


@gpu
def test_visibility_is_the_tracers_bit_for_bit(scene, rendered):
    """hit mask, face id and depth equal trace_pinhole's / trace_ids' for the same inputs; both modes give the same visibility"""
    tracer = rendered["colour_renderer"].tracer
    for h, w in FRAMES:
        depth, hit = tracer.trace_pinhole(FX, FY, CX, CY, h, w, True, miss_value=MISS, want_hit=True)
        d = scene[(h, w)]["d"]
        _, _, _, face = tracer.trace_ids(np.zeros_like(d), d)
        for mode in ("colour", "texture"):
            g = rendered[(mode, h, w)]
            assert g["mask"].dtype == np.uint8 and g["mask"].shape == (h, w, 3) and g["depth"].shape == (h, w) and g["face_id"].dtype == np.int32
            assert np.array_equal(g["mask"], hit.cpu().numpy()), (mode, h, w)
            assert np.array_equal(g["depth"].view(np.uint32), depth.cpu().numpy().view(np.uint32)), (mode, h, w)
            assert np.array_equal(g["face_id"].reshape(-1), face.cpu().numpy()), (mode, h, w)
        assert (rendered[("colour", h, w)]["face_id"] >= 0).sum() > 700


def _unambiguous_hits(scene, rendered, mode, h, w):
    r, g = scene[(h, w)], rendered[(mode, h, w)]
    keep = ~r["ambiguous"]
    assert 1 - keep.mean() <= CAP
    assert np.array_equal((g["face_id"].reshape(-1) >= 0)[keep], r["hit"][keep]) and np.array_equal(g["face_id"].reshape(-1)[keep], r["face"][keep])
    return keep & r["hit"]


@gpu
def test_image_f_against_the_float64_oracle(scene, rendered):
    """Bound 5e-4 absolute (module docstring).  Measured on an MI355X, largest |image_f - oracle| on the 773 unambiguous hit pixels of
    either frame: 4.974e-5 with vertex colours, 3.229e-4 with the textures (the CPU restatement's figures to the digit)."""
    for mode in ("colour", "texture"):
        for h, w in FRAMES:
            sel = _unambiguous_hits(scene, rendered, mode, h, w)
            got = rendered[(mode, h, w)]["image_f"].reshape(-1, 3).astype(np.float64)
            assert got.min() >= 0 and got.max() <= 1
            err = float(np.abs(got[sel] - scene[(h, w)][mode][sel]).max())
            print(f"image_f {mode} {h} x {w}: {int(sel.sum())} pixels compared, max abs error {err:.3e}")
            assert err <= BOUND, (mode, h, w, err)
    assert rendered[("texture", 48, 64)]["image_f"].std() > 0.2                 # the texture really has contrast


@gpu
def test_uint8_image_is_the_rounded_float_image(scene, rendered):
    """image == floor(255 image_f + 0.5) of the kernel's own float output exactly; within one level of the oracle's uint8"""
    for mode in ("colour", "texture"):
        for h, w in FRAMES:
            g = rendered[(mode, h, w)]
            assert g["image"].dtype == np.uint8 and g["image"].shape == (h, w, 3)
            assert np.array_equal(g["image"], np.floor(f32(255.) * g["image_f"] + f32(0.5)).astype(np.uint8)), (mode, h, w)
            sel = _unambiguous_hits(scene, rendered, mode, h, w)
            diff = np.abs(g["image"].reshape(-1, 3)[sel].astype(np.int64) - to_u8(scene[(h, w)][mode][sel]).astype(np.int64))
            print(f"image {mode} {h} x {w}: {int((diff > 0).sum())} of {diff.size} values differ from the oracle's level, by at most {int(diff.max())}")
            assert diff.max() <= 1, (mode, h, w)


@gpu
def test_misses_missing_materials_and_missing_uvs(scene, rendered):
    """misses are 0 / 0 / miss_value / -1; a material index >= M gives colour 0 with mask 255; uv index -1 samples uv (0, 0)"""
    for mode in ("colour", "texture"):
        for h, w in FRAMES:
            g = rendered[(mode, h, w)]
            miss = g["face_id"] < 0
            assert miss.sum() > 1500 and not g["image"][miss].any() and not g["image_f"][miss].any() and not g["mask"][miss].any()
            assert (g["depth"][miss] == f32(MISS)).all() and (g["mask"][~miss] == 255).all() and (g["depth"][~miss] < 20).all()
    for h, w in FRAMES:
        g = rendered[("texture", h, w)]
        face = g["face_id"].reshape(-1)
        mat = np.where(face >= 0, scene["fm"][np.maximum(face, 0)], -1)
        none = mat == 3
        assert none.sum() > 20 and not g["image_f"].reshape(-1, 3)[none].any() and not g["image"].reshape(-1, 3)[none].any()
        assert (g["mask"].reshape(-1, 3)[none] == 255).all()
        const = mat == 1                                                        # the 1 x 1 map keeps its float values
        assert const.sum() > 20 and np.abs(g["image_f"].reshape(-1, 3)[const] - scene["materials"][1].reshape(3).numpy()).max() <= 1e-6
        nouv = (face >= 0) & (scene["fu"][np.maximum(face, 0)] < 0).all(1)
        for i, m in enumerate(materials4(scene["materials"])):
            sel = nouv & (mat == i)
            if sel.any():                                                       # uv (0, 0) is grid (-1, 1): the map's bottom-left texel (border padding)
                want = torch.nn.functional.grid_sample(m.double(), torch.tensor([[[[-1., 1.]]]], dtype=torch.float64), mode="bilinear", align_corners=False,
                                                       padding_mode="border").reshape(3).numpy()
                assert np.abs(want - m[0, :, -1, 0].double().numpy()).max() == 0
                assert np.abs(g["image_f"].reshape(-1, 3)[sel] - want).max() <= 1e-6, i
        assert nouv.sum() >= 5


def _quad_renderer(rows, cols, fx=20., cx=12., cy=8.):
    """one quad at z = -5 whose edges lie on the pixel boundaries rows[0] / rows[1] and cols[0] / cols[1] of a 16 x 24 frame"""
    X = lambda c: 5 * (c - cx) / fx
    Y = lambda r: -5 * (r - cy) / fx
    V = np.array([[X(cols[0]), Y(rows[0]), -5], [X(cols[1]), Y(rows[0]), -5], [X(cols[1]), Y(rows[1]), -5], [X(cols[0]), Y(rows[1]), -5]], f32)
    return meshrender.MeshRenderer(V, np.array([[0, 1, 2], [0, 2, 3]]), vertex_color=np.full((4, 3), 0.6, f32))


@gpu
def test_frame_validity_runs_on_the_device():
    """mesh_renderer.py:44-53 on a 16 x 24 frame; and no host read inside render"""
    H, W = 16, 24
    cases = (("rows 0 and 15", (-1, 17), (10, 14), False), ("columns 0 and 23", (6, 8), (-1, 25), False), ("308 of 384, no border", (1, 15), (1, 23), False),
             ("195 of 384, no border", (1, 14), (1, 16), False), ("exactly 192 of 384", (1, 13), (1, 17), True), ("top and left only", (-1, 5), (-1, 7), True),
             ("top and left, one column short of the right", (0, 3), (0, 23), True))
    for what, rows, cols, kept in cases:
        r = _quad_renderer(rows, cols)
        n = (min(rows[1], H) - max(rows[0], 0)) * (min(cols[1], W) - max(cols[0], 0))
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            image, mask, extra = r.render(20., 20., 12., 8., H, W, miss_value=MISS, want=WANT)
            image0, mask0, extra0 = r.render(20., 20., 12., 8., H, W, miss_value=MISS, want=WANT, validate=False)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert int((mask0[..., 0] == 255).sum()) == n and int((extra0["face_id"] >= 0).sum()) == n, (what, n)      # validate=False never clears
        assert (image0[mask0 > 0] == 153).all() and ((extra0["depth"][mask0[..., 0] > 0] - 5.).abs() <= 1e-5).all()
        if kept:
            assert torch.equal(image, image0) and torch.equal(mask, mask0), what
            assert all(torch.equal(extra[k], extra0[k]) for k in WANT), what
        else:
            assert not image.any() and not mask.any() and not extra["image_f"].any(), what
            assert (extra["depth"] == MISS).all() and (extra["face_id"] == -1).all(), what
    empty = meshrender.MeshRenderer(np.zeros((0, 3), f32), np.zeros((0, 3), np.int64), vertex_color=np.zeros((0, 3), f32))
    image, mask, extra = empty.render(20., 20., 12., 8., H, W, miss_value=MISS, want=WANT)               # no mesh: everything misses, the frame is valid
    assert not image.any() and not mask.any() and (extra["depth"] == MISS).all() and (extra["face_id"] == -1).all()
    assert tuple(empty.render(20., 20., 12., 8., 0, W)[0].shape) == (0, W, 3)


@gpu
def test_renders_are_bit_identical_across_runs_and_flavours(scene, rendered):
    from snerf_amd import ops
    for mode in ("colour", "texture"):
        r = rendered[mode + "_renderer"]
        for h, w in FRAMES:
            for flags in (0, ops.MESH_UNIFORM, ops.MESH_NO_CULL, ops.MESH_UNIFORM | ops.MESH_NO_CULL):
                image, mask, extra = r.render(FX, FY, CX, CY, h, w, miss_value=MISS, want=WANT, flags=flags)
                g = rendered[(mode, h, w)]
                assert np.array_equal(image.cpu().numpy(), g["image"]) and np.array_equal(mask.cpu().numpy(), g["mask"]), (mode, h, w, flags)
                assert all(np.array_equal(extra[k].cpu().numpy().view(np.uint32), g[k].view(np.uint32)) for k in WANT), (mode, h, w, flags)


@gpu
def test_transform_is_the_tracers(scene, rendered):
    """the unplaced mesh rendered through `transform` sees what the tracer sees through it; where it sees the oracle's face its colours
    stay inside the image bound of the baked mesh: the kernel's placement moves a vertex by at most 4 ulp(16) = 4e-6 (test_mesh_trace's
    _transform_bound), 4e-5 of these 0.1-long edges in barycentric terms, on top of the 5e-5 measured without a transform"""
    P = placement()
    V0 = np.concatenate([scene["sphere_v"], (QUAD - P[:, 3]) @ np.linalg.inv(P[:, :3]).T]).astype(f32)
    r = meshrender.MeshRenderer(V0, scene["F"], vertex_color=scene["colours"])
    h, w = FRAMES[0]
    for T in (P, torch.tensor(P).cuda()):
        image, mask, extra = r.render(FX, FY, CX, CY, h, w, transform=T, want=WANT)
        depth, hit = r.tracer.trace_pinhole(FX, FY, CX, CY, h, w, True, transform=T, want_hit=True)
        assert torch.equal(mask, hit) and torch.equal(extra["depth"], depth)
        sel = _unambiguous_hits(scene, rendered, "colour", h, w) & (extra["face_id"].cpu().numpy().reshape(-1) == scene[(h, w)]["face"])
        assert sel.sum() > 700
        assert np.abs(extra["image_f"].cpu().numpy().reshape(-1, 3)[sel] - scene[(h, w)]["colour"][sel]).max() <= BOUND


@gpu
def test_composite_frame_renders_its_instances(scene, rendered):
    """an instance with render= gives the frame that the same instance gives with its image and mask rendered beforehand"""
    from snerf_amd import foreground as fgm
    h, w = FRAMES[0]
    K = np.array([[FX, 0, CX], [0, FY, CY], [0, 0, 1]])
    shift = np.array([[1., 0, 0, -1.5], [0, 1, 0, 0.4], [0, 0, 1, 1.], [0, 0, 0, 1]])
    rng = np.random.default_rng(5)
    bg = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    depth = (rng.integers(256, 20 * 256, (h, w)) / 256.).astype(f32)
    sem = rng.integers(0, 19, (h, w)).astype(np.uint8)
    plan = ((rendered["texture_renderer"], None, "vehicle"), (rendered["colour_renderer"], shift, "person"))
    frames = []
    for on_the_fly in (True, False):
        inst = []
        for r, T, cat in plan:
            image, mask, extra = r.render(FX, FY, CX, CY, h, w, transform=T, want=("depth",), miss_value=.1)
            i = dict(category=cat, r=2, fg_depth=None if cat == "person" else extra["depth"])
            i.update(dict(render=(r, T), intrinsic=K) if on_the_fly else dict(image=image, mask=mask))
            inst.append(i)
        frames.append(fgm.composite_frame(_dev(bg), _dev(depth), _dev(sem), inst))
    for k in ("fuse", "mask", "bound", "occluded_mask", "depth", "semantic"):
        assert torch.equal(frames[0][k], frames[1][k]), k
    assert [float(o) for o in frames[0]["occlusion"]] == [float(o) for o in frames[1]["occlusion"]]
    assert 0.05 < float(frames[0]["occlusion"][0]) < 0.95 and int((frames[0]["mask"] > 0).sum()) > 3 * 600          # both instances are in the frame
    assert not torch.equal(frames[0]["fuse"], _dev(bg))


@gpu
def test_center_mesh_bottom_on_the_device(scene):
    _check_center_mesh_bottom(scene, "cuda")
