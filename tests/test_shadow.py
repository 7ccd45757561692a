"""The projected mesh shadow (snerf_amd.shadow, csrc/shadow.hip: snerf_shadow_project / snerf_shadow_close / snerf_shadow_fuse) against
tests/shadow_cpu_model.py, and that model against the reference's own functions.

Pinned by the reference (tests/golden/g18_foreground_shadow.npz, written by tools/gen_golden_shadow.py from s-nerfpp/stage3_code/utils.py):
process_mesh, project_to_ground (with its `if not ground_height` quirk), project, points_to_mask (strict `> 0` clip), check_the_occlusion
and the fuse expression of mesh_shadow.py:100-105 -- the model reproduces every recorded output bit for bit.  NOT pinned (cv2 is absent):
the closing and the box filter; they are checked against OpenCV's published definitions, restated here as per-pixel window loops, and
against known answers.

Every device comparison is bit-equal: mask, closed mask, kw / kh, counts, image.  The splat can be compared that way because every
test asserts that no projected coordinate of its inputs lies within 1e-7 of an integer (device and numpy float64 differ by ~1e-13
through the order of the products); the hand-made points sit on half-integers."""
import ctypes
import os

import numpy as np
import pytest
import torch

import shadow_cpu_model as model
from snerf_amd import _lib

gpu = pytest.mark.gpu
built = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libsnerf_hip.so not built (run __graft_entry__.build())")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g18_foreground_shadow.npz")
MARGIN = 1e-7
N_CASES = 3


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN, allow_pickle=False))


def _case(g, k):
    """the inputs of fixture case k as the keyword arguments of the model's / the device's entry points"""
    p = f"c{k}_"
    H, W = (int(v) for v in g[p + "hw"])
    ground = None if bool(g[p + "ground_none"]) else float(g[p + "ground"])
    return dict(vertices=np.ascontiguousarray(g[p + "mesh_points"].T), bbox_center=g[p + "bbox_center"], theta=float(g[p + "theta"]), mesh_bias=g[p + "mesh_bias"],
                pitch_angle=float(g[p + "pitch"]), yaw_angle=float(g[p + "yaw"]), c2w=g[p + "c2w"], P=g[p + "P"], ground_height=ground), H, W


# ---- the model against the reference's recorded outputs -----------------------------------------------------------------------------
def test_model_reproduces_every_recorded_reference_output(golden):
    g = golden
    grounds = []
    for k in range(N_CASES):
        kw, H, W = _case(g, k)
        p = f"c{k}_"
        grounds.append(kw["ground_height"])
        placed = model.process_mesh(g[p + "mesh_points"], kw["bbox_center"], kw["theta"], kw["mesh_bias"])
        assert np.array_equal(placed, g[p + "placed"]), (k, "process_mesh")
        grounded = model.project_to_ground(g[p + "placed"], kw["pitch_angle"], kw["yaw_angle"], kw["ground_height"])
        assert np.array_equal(grounded, g[p + "grounded"]), (k, "project_to_ground")
        projected = model.project(g[p + "grounded"], kw["c2w"], kw["P"])
        assert np.array_equal(projected, g[p + "projected"]), (k, "project")
        want = np.unpackbits(g[p + "mask"], axis=1)[:, :W].astype(bool)
        assert bool(g[p + "mask_channels_equal"])
        mask = model.points_to_mask(g[p + "projected"], H, W)
        assert np.array_equal(mask, np.repeat(want[..., None], 3, 2).astype(np.uint8) * 255), (k, "points_to_mask")
        assert not mask[0].any() and not mask[:, 0].any() and mask.any()                       # strict: row 0 and column 0 never set
        x, y = model.pixel_coordinates(g[p + "projected"])
        q = np.concatenate([x, y])
        assert np.abs(q - np.round(q)).min() > MARGIN and np.abs(q).max() < 6e4                 # what the generator promises
        assert ((x < 0) | (x >= W) | (y < 0) | (y >= H)).any()                                  # the clip is exercised
        # the whole chain from the raw inputs, as the device tests use the model
        assert np.array_equal(model.shadow_mask(H=H, W=W, **kw)[0], mask)
    assert grounds[0] is None and grounds[1] == 0.0 and grounds[2] not in (None, 0.0)
    # the quirk: 0.0 means "the smallest z", so case 1's ground is NOT z = 0
    z = g["c1_placed"][2]
    assert np.array_equal(g["c1_grounded"][2], z - model.light_vector(float(g["c1_pitch"]), float(g["c1_yaw"]))[2] * ((z - z.min()) / model.light_vector(
        float(g["c1_pitch"]), float(g["c1_yaw"]))[2]))
    assert abs(g["c1_grounded"][2] - z.min()).max() < 1e-12 and abs(z.min()) > 0.01
    blurred = np.repeat(g["f_blurred"][..., None], 3, 2)
    assert np.array_equal(model.check_the_occlusion(g["f_total"], blurred), g["f_occ"])
    assert np.array_equal(model.fuse(g["f_im"], g["f_total"], blurred, float(g["f_light_scale"])), g["f_fused"])
    assert (g["f_fused"] != g["f_im"]).any()


def test_host_placement_and_light_agree_with_the_model(golden):
    """snerf_amd.shadow's host matrices: Rz from cos / sin (scipy's goes through a quaternion: an ulp apart) and P c2w^-1 composed"""
    from snerf_amd import shadow
    for k in range(N_CASES):
        kw, H, W = _case(golden, k)
        A = shadow.process_placement(kw["bbox_center"], kw["theta"], kw["mesh_bias"])
        pts = golden[f"c{k}_mesh_points"]
        assert np.abs(A[:, :3] @ pts + A[:, 3:] - golden[f"c{k}_placed"]).max() < 1e-14
        assert np.array_equal(shadow.light_vector(kw["pitch_angle"], kw["yaw_angle"]), model.light_vector(kw["pitch_angle"], kw["yaw_angle"]))
        M = shadow.world_to_pixel(kw["c2w"], kw["P"])
        gr = golden[f"c{k}_grounded"]
        assert np.abs(M[:, :3] @ gr + M[:, 3:] - golden[f"c{k}_projected"]).max() < 1e-10


# ---- OpenCV's definitions, per pixel -------------------------------------------------------------------------------------------------
def _window_by_definition(img, r, erode):
    """dst(x, y) = max / min over 0 <= x', y' < r of src(x + x' - r // 2, y + y' - r // 2), pixels outside never win"""
    H, W = img.shape
    a = r // 2
    out = np.zeros_like(img)
    for y in range(H):
        for x in range(W):
            win = img[max(0, y - a):max(0, min(H, y - a + r)), max(0, x - a):max(0, min(W, x - a + r))]
            out[y, x] = win.min() if erode else win.max()
    return out


def _close_by_definition(mask2d, r, iter):
    h, w = mask2d.shape
    img = np.pad(mask2d, ((h, h), (w, w)))
    for _ in range(iter):
        img = _window_by_definition(img, r, False)
    for _ in range(iter):
        img = _window_by_definition(img, r, True)
    return img[h:2 * h, w:2 * w]


def _close(mask2d, r, iter):
    """the model's closing of a 2-D bool mask -> 2-D bool"""
    return model.interpolate(np.repeat(mask2d[..., None], 3, 2).astype(np.uint8) * 255, r, iter)[..., 0] > 0


def _single(shape, y, x):
    m = np.zeros(shape, bool)
    m[y, x] = True
    return m


@pytest.mark.parametrize("r,iter,want", [(20, 3, (13, 20)), (2, 1, (11, 18)), (3, 1, (10, 17)), (5, 2, (10, 17))])
def test_closing_of_a_single_pixel(r, iter, want):
    """an even r shifts the result by iter * (r // 2 - (r - 1 - r // 2)) = iter pixels; both routes agree"""
    m = _single((24, 40), 10, 17)
    for got in (_close(m, r, iter), _close_by_definition(m, r, iter)):
        assert np.array_equal(got, _single((24, 40), *want)), (r, iter, np.argwhere(got).tolist())


def test_closing_known_answers():
    # a pixel whose shifted image leaves the frame
    m = _single((24, 40), 22, 38)
    assert not _close(m, 20, 3).any() and not _close_by_definition(m, 20, 3).any()
    # two pixels 47 apart in a row are bridged (3 dilations reach 27 + 30): one 48-pixel run, shifted by (+3, +3)
    m = np.zeros((24, 65), bool)
    m[8, 3] = m[8, 50] = True
    want = np.zeros((24, 65), bool)
    want[11, 6:54] = True
    for got in (_close(m, 20, 3), _close_by_definition(m, 20, 3)):
        assert np.array_equal(got, want), np.argwhere(got).tolist()
    # a full mask loses its three left columns; its rows survive because the pad (24) is smaller than the reach (30): the dilation fills
    # the padded rows, and outside the padded image nothing wins
    full = np.ones((24, 40), bool)
    want = full.copy()
    want[:, :3] = False
    for got in (_close(full, 20, 3), _close_by_definition(full, 20, 3)):
        assert np.array_equal(got, want) and got.sum() == 888
    # iter = 0 copies; r = 1 is the identity
    rng = np.random.default_rng(5)
    m = rng.random((9, 70)) < 0.3
    assert np.array_equal(_close(m, 20, 0), m) and np.array_equal(_close(m, 1, 2), m)
    for r, it in ((7, 2), (4, 1), (2, 3)):
        assert np.array_equal(_close(m, r, it), _close_by_definition(m, r, it)), (r, it)


def _counts_by_definition(m, kw, kh):
    H, W = m.shape
    refl = lambda i, n: -i if i < 0 else (2 * (n - 1) - i if i >= n else i)
    out = np.zeros((H, W), np.int64)
    for y in range(H):
        for x in range(W):
            out[y, x] = sum(int(m[refl(y - kh // 2 + j, H), refl(x - kw // 2 + i, W)]) for j in range(kh) for i in range(kw))
    return out


def test_box_counts_reflect_101():
    rng = np.random.default_rng(11)
    m = rng.random((9, 14)) < 0.4
    m[0, 0] = m[8, 13] = True
    m[0, 13] = m[8, 0] = False
    for kw, kh in ((2, 3), (3, 2), (4, 1), (1, 4), (5, 3), (2, 2)):
        assert np.array_equal(model.box_counts(m, kw, kh), _counts_by_definition(m, kw, kh)), (kw, kh)
    assert np.array_equal(model.box_counts(m, 1, 1), m.astype(np.int64))
    # hand-checked: a lone corner pixel under a 3 x 3 window is seen once from (0, 0), (0, 1), (1, 0) and (1, 1): the reflection does not repeat
    # the edge row, it mirrors about it -- so (1, 1) sees (0, 0) once and (0, 0) sees it once
    c = model.box_counts(_single((5, 6), 0, 0), 3, 3)
    assert c[:2, :2].tolist() == [[1, 1], [1, 1]] and c.sum() == 4
    # an even kernel reaches one further to the left / up (anchor k // 2)
    c = model.box_counts(_single((5, 6), 2, 3), 2, 2)
    assert np.argwhere(c).tolist() == [[2, 3], [2, 4], [3, 3], [3, 4]]
    assert model.blur_kernel(np.zeros((5, 6, 3), np.uint8)) == (False, 1, 1)
    m3 = np.zeros((40, 60, 3), np.uint8)
    m3[4:31, 7:50] = 255                                     # box 42 x 26 -> 8 x 5
    assert model.blur_kernel(m3) == (True, 8, 5)
    m3[:] = 0
    m3[3:7, 2:6] = 255                                       # box 3 x 3 -> max(1, 0)
    assert model.blur_kernel(m3) == (True, 1, 1)


# ---- host statuses, without a device -------------------------------------------------------------------------------------------------
H0, W0 = 48, 64
_IMG = 3 * H0 * W0


def _host_block():
    """one host allocation carved into non-overlapping [H,W,3] images and a scratch buffer: the checks never dereference them"""
    ws_bytes = _lib.query("snerf_shadow_ws_bytes", H0, W0, 100, 20, 3)
    buf = (ctypes.c_char * (ws_bytes + 4 * _IMG + 1024))()
    a = (ctypes.addressof(buf) + 255) & ~255
    return buf, dict(ws=a, ws_bytes=ws_bytes, im=a + ws_bytes + 256, total_mask=a + ws_bytes + 256 + _IMG, shadow_mask=a + ws_bytes + 256 + 2 * _IMG,
                     vertices=a + ws_bytes + 256 + 3 * _IMG)


def _status(name, ptrs, **values):
    xf = (ctypes.c_double * 28)(*([1.] * 28))
    base = dict(ptrs, vertices_f64=0, N=100, xf=ctypes.addressof(xf), ground_mode=1, H=H0, W=W0, mask_out=ptrs["shadow_mask"], mask_in=ptrs["total_mask"],
                r=20, iter=3, light_scale=.55, check=0, stream=None)
    base.update(values)
    return getattr(_lib.load(), name)(*[base[arg] for _, arg in _lib.parse_header()[name]])


@built
def test_shadow_entries_refuse_bad_arguments_without_a_gpu():
    """every refusal is SNERF_ERR_ARG before any launch"""
    q = lambda *a: _lib.query("snerf_shadow_ws_bytes", *a)
    off = lambda *a: _lib.query("snerf_shadow_ws_offset", *a)
    assert q(H0, W0, 100, 20, 3) > q(H0, W0, 100, 1, 0) > 4 * H0 * W0 * 2 and q(H0, W0, 0, 20, 3) == q(H0, W0, 100, 20, 3)
    for bad in ((0, W0, 1, 20, 3), (H0, 0, 1, 20, 3), (H0, W0, -1, 20, 3), (H0, W0, 1 << 31, 20, 3), (H0, W0, 1, 0, 3), (H0, W0, 1, 20, -1), (1 << 16, 1 << 15, 1, 20, 3),
                (1 << 30, 1, 1, 20, 1 << 27)):
        assert q(*bad) == 0, bad                                   # the last one: H W fits, the rows of the extended bit plane (3 H) do not
    assert q(1 << 15, 1 << 15, 1, 20, 3) > 0 and q(1 << 30, 1, 1, 20, 3) > 0
    assert off(H0, W0, 0) == 0 and off(H0, W0, 1) > 0 and off(H0, W0, 1) % 256 == 0 and off(H0, W0, 1) + 4 * H0 * W0 <= q(H0, W0, 0, 1, 0)
    assert off(0, W0, 0) == -1 and off(H0, W0, 2) == -1 and off(H0, W0, -1) == -1
    buf, p = _host_block()
    small = q(H0, W0, 100, 1, 0)
    for bad in (dict(vertices=None), dict(xf=None), dict(ws=None), dict(ws=p["ws"] + 4), dict(H=0), dict(W=-1), dict(N=-1), dict(N=1 << 31), dict(ws_bytes=small - 1),
                dict(ws_bytes=0), dict(vertices_f64=2), dict(ground_mode=3), dict(ground_mode=-1), dict(H=1 << 16, W=1 << 15),
                dict(mask_out=p["ws"] + 512), dict(mask_out=p["vertices"] + 4)):
        assert _status("snerf_shadow_project", p, **bad) == 1, bad
    for bad in (dict(ws=None), dict(ws=p["ws"] + 2), dict(H=0), dict(W=0), dict(r=0), dict(r=-3), dict(iter=-1), dict(ws_bytes=p["ws_bytes"] - 1), dict(ws_bytes=small),
                dict(mask_out=p["total_mask"] + 3), dict(mask_out=p["total_mask"] - _IMG + 1), dict(mask_out=p["ws"]), dict(mask_in=p["ws"] + p["ws_bytes"] - 1),
                dict(H=1 << 30, W=1, iter=1 << 27, ws_bytes=1 << 40)):
        assert _status("snerf_shadow_close", p, **bad) == 1, bad
    for bad in (dict(im=None), dict(total_mask=None), dict(ws=None), dict(ws=p["ws"] + 1), dict(H=-1), dict(W=0), dict(ws_bytes=small - 1), dict(check=2),
                dict(light_scale=-0.1), dict(light_scale=1.5), dict(light_scale=float("nan")), dict(total_mask=p["im"] + 1), dict(shadow_mask=p["im"]),
                dict(shadow_mask=p["im"] + _IMG - 1), dict(im=p["ws"] + 1024), dict(total_mask=p["ws"]), dict(H=1 << 16, W=1 << 15)):
        assert _status("snerf_shadow_fuse", p, **bad) == 1, bad
    del buf


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _m3(mask2d):
    return np.repeat(np.asarray(mask2d, bool)[..., None], 3, 2).astype(np.uint8) * 255


def _assert_margin(x, y):
    q = np.concatenate([x, y])
    q = q[np.isfinite(q) & (np.abs(q) < 1e5)]
    assert q.size == 0 or np.abs(q - np.round(q)).min() > MARGIN, "a projected coordinate of this test's input is too close to an integer"


def _project_both(kw, H, W, dtype, check=False):
    """-> (device mask, model mask) for vertices of `dtype`; the model gets the values the device gets"""
    from snerf_amd import shadow
    v = np.ascontiguousarray(np.asarray(kw["vertices"]).reshape(-1, 3).astype(dtype))
    with np.errstate(all="ignore"):
        want, (x, y) = model.shadow_mask(H=H, W=W, check=check, **dict(kw, vertices=v.astype(np.float64)))
    _assert_margin(x, y)
    got = shadow.project_shadow_mask(H=H, W=W, check=check, **dict(kw, vertices=_dev(v))).cpu().numpy()
    return got, want


@gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_project_fixture_cases(golden, dtype):
    for k in range(N_CASES):
        kw, H, W = _case(golden, k)
        for ground in (kw["ground_height"], None, 0.0, -0.37):
            got, want = _project_both(dict(kw, ground_height=ground), H, W, dtype)
            assert want.any() and np.array_equal(got, want), (k, ground, int((got != want).sum()))
        got, want = _project_both(kw, H, W, dtype, check=True)                      # no ground projection
        assert np.array_equal(got, want), (k, "check")
    if dtype is np.float64:                                                          # on fp64 vertices the device reproduces the REFERENCE's recorded splat
        for k in range(N_CASES):
            kw, H, W = _case(golden, k)
            got, _ = _project_both(kw, H, W, dtype)
            assert np.array_equal(got[..., 0] > 0, np.unpackbits(golden[f"c{k}_mask"], axis=1)[:, :W].astype(bool)), k


@gpu
def test_project_block_tails_and_empty(golden):
    kw, H, W = _case(golden, 0)
    rng = np.random.default_rng(3)
    for n in (0, 1, 65, 4097):
        d = rng.normal(size=(n, 3))
        d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-9)
        v = d * np.array([2.1, 0.9, 0.75]) + np.array([0., 0., 0.75])
        for dtype in (np.float32, np.float64):
            got, want = _project_both(dict(kw, vertices=v), H, W, dtype)
            assert np.array_equal(got, want) and want.any() == (n > 0), (n, dtype)


@gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_project_drops_what_the_reference_clips_or_wraps(dtype):
    """hand-made points on the ground plane z = g (so the ground projection leaves them where they are), seen by a camera at the origin
    that looks along world +x: pixel (u, v) comes from (wx, wy, g) with wx = -fy g / (v - cy), wy = -(u - cx) wx / fx"""
    H, W, fx, fy, cx, cy, g = 24, 40, 32., 32., 20.25, 4.25, -1.
    c2w = np.array([[0., 0, 1, 0], [-1, 0, 0, 0], [0, -1, 0, 0], [0, 0, 0, 1]])
    P = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.]])
    targets = [(1.5, 1.5), (12.5, 7.5), (39.5, 10.5), (10.5, 23.5),                  # kept: first and last valid column / row
               (0.5, 10.5), (10.5, 0.5), (40.5, 10.5), (10.5, 24.5),                 # column 0, row 0, x >= W, y >= H
               (-3.5, 10.5), (-0.5, 10.5), (10.5, -2.5),                             # negative quotients
               (65546.5, 10.5), (-65525.5, 10.5), (10.5, 65546.5)]                   # the reference's uint16 cast would wrap these to 10
    pts = []
    for u, v in targets:
        wx = -fy * g / (v - cy)
        pts.append([wx, -(u - cx) * wx / fx, g])
    pts += [[0., 1., g], [np.nan, 1., g], [3., np.nan, g], [np.inf, 1., g]]         # third coordinate 0 (division by zero), NaN, inf
    kw = dict(vertices=np.array(pts), bbox_center=(0., 0., 0.), theta=0., mesh_bias=(0., 0., 0.), pitch_angle=30., yaw_angle=20., c2w=c2w, P=P)
    want_set = [[1, 1], [7, 12], [10, 39], [23, 10]]
    for ground in (g, None):                                                          # the smallest z of the placed points is g too (the NaN never wins)
        got, want = _project_both(dict(kw, ground_height=ground), H, W, dtype)
        assert np.array_equal(got, want)
        assert sorted(np.argwhere(got[..., 0]).tolist()) == want_set and np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 0], got[..., 2])


def _masks(H, W, rng):
    edges = np.zeros((H, W), bool)
    edges[0, W // 3] = edges[H - 1, W // 2] = edges[H // 2, 0] = edges[H // 3, W - 1] = edges[0, 0] = edges[H - 1, W - 1] = True
    edges[H // 2, W // 2:W // 2 + 5] = True
    return dict(sparse=rng.random((H, W)) < 0.01, dense=rng.random((H, W)) < 0.30, edges=edges, empty=np.zeros((H, W), bool), full=np.ones((H, W), bool))


def _close_both(m2d, r, it):
    from snerf_amd import shadow
    m = _m3(m2d)
    return shadow.interpolate(_dev(m), r, it).cpu().numpy(), model.interpolate(m, r, it)


@gpu
@pytest.mark.parametrize("H,W", [(24, 40), (24, 65), (96, 160), (70, 129)])
def test_close_matches_the_model(H, W):
    """24 x 40 and 24 x 65: the pad is smaller than the reach of r = 20, iter = 3, and 65 leaves a one-bit word tail; 70 x 129 likewise"""
    rng = np.random.default_rng(H * 1000 + W)
    for name, m in _masks(H, W, rng).items():
        for r, it in ((1, 1), (2, 1), (3, 1), (20, 3), (7, 2), (20, 0)):
            got, want = _close_both(m, r, it)
            assert np.array_equal(got, want), (name, r, it, int((got != want).sum()))


@gpu
def test_close_wide_windows_and_both_kernel_routes():
    """windows wider than a word (two halo words per side) and windows whose tile no longer fits in LDS, which take the row / column
    kernels through global memory: r = 900 on 70 x 129 is clamped to the extended image (387 wide), 141 KB of tile"""
    rng = np.random.default_rng(9)
    for (H, W), params in (((70, 129), ((60, 1), (130, 1), (131, 2), (900, 1), (901, 2))), ((5, 300), ((64, 2), (65, 1), (700, 1))), ((200, 3), ((33, 2), (1000, 1)))):
        for name, m in _masks(H, W, rng).items():
            if name in ("sparse", "edges", "full"):
                for r, it in params:
                    got, want = _close_both(m, r, it)
                    assert np.array_equal(got, want), ((H, W), name, r, it, int((got != want).sum()))


@gpu
def test_close_known_answers_on_the_device():
    from snerf_amd import shadow
    got, _ = _close_both(_single((24, 40), 10, 17), 20, 3)
    assert np.argwhere(got[..., 0]).tolist() == [[13, 20]]
    m = _dev(_m3(np.ones((24, 40), bool)))
    out = shadow.interpolate(m, 20, 3)
    assert int((out[..., 0] > 0).sum()) == 888 and not bool(out[:, :3].any())
    # in place is allowed: the input is packed before anything is written
    from snerf_amd import ops
    ws = torch.empty(ops.shadow_ws_bytes(24, 40, 0, 20, 3), dtype=torch.uint8, device="cuda")
    ops.shadow_close(m, 24, 40, 20, 3, ws, m)
    assert torch.equal(m, out)


FH, FW = 48, 80


def _fuse_inputs():
    rng = np.random.default_rng(21)
    im = rng.integers(0, 256, (FH, FW, 3)).astype(np.uint8)
    im[32:36, 52:78], im[36:40, 52:78], im[40:44, 52:78], im[44:48, 52:78] = 0, 20, 200, 255        # multiples of 20: on truncation boundaries at full coverage
    total = np.zeros((FH, FW, 3), np.uint8)
    total[28:40, 60:70, 0] = 255
    total[10:45, 40:58, 1] = 1
    total[:, 75:, 2] = 200
    corner = np.zeros((FH, FW), bool)
    corner[30:, 50:] = True                                       # touches the right and the bottom edge: box 29 x 17 -> 5 x 3, the window reflects
    ragged = np.zeros((FH, FW), bool)
    ragged[5:41, 10:71] = rng.random((36, 61)) < 0.6              # box ~60 x 35 -> 12 x 7: an even and an odd kernel, kw != kh
    ragged[5, 10] = ragged[40, 70] = True
    tiny = np.zeros((FH, FW), bool)
    tiny[20:24, 33:38] = True                                     # box 4 x 3 -> 1 x 1
    whole = np.ones((FH, FW), bool)                               # box 79 x 47 -> 15 x 9, reflects on every side
    col0 = np.zeros((FH, FW), bool)
    col0[:, 0] = True                                             # box 0 x 47 -> 1 x 9
    return im, total, dict(corner=corner, ragged=ragged, tiny=tiny, whole=whole, col0=col0)


@gpu
def test_fuse_matches_the_model():
    from snerf_amd import ops, shadow
    im, total, masks = _fuse_inputs()
    ws = torch.empty(ops.shadow_ws_bytes(FH, FW, 0, 1, 0), dtype=torch.uint8, device="cuda")
    info, counts = ops.shadow_ws_views(ws, FH, FW)
    seen = set()
    for name, m in masks.items():
        for ls in (.55, 1.0, 0.3):
            want, rec = model.blur_shadow(im, total, _m3(m), ls)
            d_im = _dev(im)
            shadow.blur_shadow(d_im, _dev(total), _dev(_m3(m)), ls, ws=ws)
            assert info[:3].tolist() == [1, rec["kw"], rec["kh"]], (name, info.tolist(), rec["kw"], rec["kh"])
            assert np.array_equal(counts.cpu().numpy(), rec["counts"]), name
            got = d_im.cpu().numpy()
            assert np.array_equal(got, want), (name, ls, int((got != want).sum()))
            assert (want != im).any()
            # the call made twice: shadows multiply
            want2 = model.blur_shadow(want, total, _m3(m), ls)[0]
            shadow.blur_shadow(d_im, _dev(total), _dev(_m3(m)), ls, ws=ws)
            assert np.array_equal(d_im.cpu().numpy(), want2), (name, ls, "twice")
        seen.add((rec["kw"], rec["kh"]))
    assert seen == {(5, 3), (12, 7), (1, 1), (15, 9), (1, 9)}, seen
    # an empty mask leaves the image untouched
    d_im = _dev(im)
    shadow.blur_shadow(d_im, _dev(total), _dev(np.zeros((FH, FW, 3), np.uint8)), .55, ws=ws)
    assert int(info[0]) == 0 and np.array_equal(d_im.cpu().numpy(), im)


@gpu
def test_fuse_reproduces_the_recorded_reference_arithmetic(golden):
    """the recorded blurred array is counts / (kw kh) of the model's closed mask of case 0: the device, given that mask, must land on the
    image the reference's own expression gave"""
    from snerf_amd import shadow
    g = golden
    kw, H, W = _case(g, 0)
    closed = model.interpolate(model.shadow_mask(H=H, W=W, **kw)[0], 20, 3)
    d_im = _dev(g["f_im"])
    shadow.blur_shadow(d_im, _dev(g["f_total"]), _dev(closed), float(g["f_light_scale"]))
    assert np.array_equal(d_im.cpu().numpy(), g["f_fused"])


@pytest.fixture(scope="module")
def frames(golden):
    """per fixture case: an image, a total mask, and the model's answers for cast, cast with check, and a second instance on top"""
    out = []
    for k in range(N_CASES):
        kw, H, W = _case(golden, k)
        rng = np.random.default_rng(40 + k)
        im = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
        total = np.zeros((H, W, 3), np.uint8)
        total[H // 2:H // 2 + H // 4, W // 4:W // 2] = 255
        total[: H // 2, :, 1] = 255
        second = dict(kw, theta=kw["theta"] + 40., bbox_center=np.asarray(kw["bbox_center"]) + np.array([0.8, -0.6, 0.]), ground_height=None)
        _assert_margin(*model.shadow_mask(H=H, W=W, **second)[1])
        one = model.cast(im, total, **kw)
        out.append(dict(kw=kw, H=H, W=W, im=im, total=total, second=second, one=one, two=model.cast(one, total, **second), check=model.cast(im, total, check=True, **kw)))
        assert (one != im).any() and (out[-1]["two"] != one).any() and (out[-1]["check"] != im).any()
    return out


def _cast(caster, im, total, kw, dtype=np.float64, **extra):
    d_im = _dev(im)
    caster.cast(d_im, _dev(total), **dict(kw, vertices=_dev(np.asarray(kw["vertices"]).astype(dtype))), **extra)
    return d_im.cpu().numpy()


@gpu
def test_cast_end_to_end(frames):
    from snerf_amd import shadow
    for f in frames:
        caster = shadow.ShadowCaster(f["H"], f["W"], 600)
        got = _cast(caster, f["im"], f["total"], f["kw"])
        assert np.array_equal(got, f["one"]), int((got != f["one"]).sum())
        assert np.array_equal(_cast(caster, f["im"], f["total"], f["kw"]), got)                      # the same call on a fresh copy: the same bits
        assert np.array_equal(_cast(caster, got, f["total"], f["second"]), f["two"])                   # two instances in sequence
        assert np.array_equal(_cast(caster, f["im"], f["total"], f["kw"], check=True), f["check"])
        v32 = dict(f["kw"], vertices=np.asarray(f["kw"]["vertices"]).astype(np.float32).astype(np.float64))
        _assert_margin(*model.shadow_mask(H=f["H"], W=f["W"], **v32)[1])
        assert np.array_equal(_cast(caster, f["im"], f["total"], f["kw"], dtype=np.float32), model.cast(f["im"], f["total"], **v32))


@gpu
def test_cast_makes_no_host_read_and_no_allocation(frames):
    from snerf_amd import shadow
    f = frames[0]
    caster = shadow.ShadowCaster(f["H"], f["W"], 600)
    d_total, v = _dev(f["total"]), _dev(f["kw"]["vertices"])
    kw = dict(f["kw"], vertices=v)
    ims = [_dev(f["im"]) for _ in range(3)]
    caster.cast(ims[0], d_total, **kw)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode("error")
    try:
        caster.cast(ims[1], d_total, **kw)
        caster.cast(ims[2], d_total, check=True, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    assert np.array_equal(ims[1].cpu().numpy(), f["one"]) and np.array_equal(ims[2].cpu().numpy(), f["check"])
