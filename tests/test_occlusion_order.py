"""The occlusion order of the foreground instances on the device (snerf_amd.foreground: overlap_stats / snerf_fg_overlap, occlusion_order,
composite_frame(order="occlusion")) and the label export (occlusion_level, bbox_result, save_bbox_results), against
tests/overlap_cpu_model.py, the float64 numpy statement of s-nerfpp/stage1_code/utils_render.py:691-808 and :543-640.

The overlap statistics are integers: every comparison is bit-exact.  The order is a chain of decisions z_a < z_b on fp32-traced rays, so
scene S keeps, in the float64 model, every compared pair of z at least 1e-3 apart and every centroid ray at least 1e-3 (barycentric)
from changing sides of any triangle outline; both margins are asserted on the model before anything is compared, so the fp32 tracer
(depth parity 1e-4 relative, tests/test_mesh_trace.py) cannot flip a decision and `before` / `order` must be EQUAL.

Scene S, 48 x 64, fx = fy = 60, cx = 32, cy = 24, camera coordinates +z forward (x right, y down), four meshes that do not touch: a
box around z = 4, a UV sphere (216 faces) around z = 6, and, both turned by -0.6 rad about y so that their left ends are near, a chevron
around z = 8 with a bar one unit in front of it.  The projections of two convex meshes overlap in ONE convex patch, so the chevron is
a 12-face, 8-vertex box whose cross-section is bent into an arrowhead: the bar crosses both of its arms, the two patches are disjoint and
their centroid lies between the arms, where the "camera" ray hits the bar and misses the chevron (last-face fallback).  The bar and the
box / sphere do not overlap: pairs without an edge.  w2c is a small rotation plus a translation, so "reference" casts world-frame rays at
camera-frame meshes: some hit, most fall back to the last face, and the ray of (chevron, bar) misses the bar, whose last face lies
BEHIND the chevron's -- the two ray frames decide that pair differently, so an implementation that casts the wrong frame's ray fails.
Masks: mask_from_mesh of the mesh under diag(1, -1, -1) @ placement (its camera looks down -z)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import overlap_cpu_model as model
from snerf_amd import _lib

gpu = pytest.mark.gpu
built = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libsnerf_hip.so not built (run __graft_entry__.build())")
H, W = 48, 64
K = np.array([[60., 0., 32.], [0., 60., 24.], [0., 0., 1.]])
FLIP = np.diag([1., -1., -1.])
MARGIN = 1e-3


# ---- meshes and scenes ----------------------------------------------------------------------------------------------------------------------
def prism(poly, z0, z1):
    """a closed 12-face mesh from a quadrilateral cross-section (x, y) swept from z0 to z1; the caps are split along the diagonal from
    corner 1 to corner 3 (for the chevron: the one that stays inside) -> (V [8,3], F [12,3]); the last face is a side face"""
    V = np.array([(x, y, z) for z in (z0, z1) for x, y in poly], dtype=np.float64)
    F = [(0, 1, 3), (1, 2, 3), (4, 7, 5), (5, 7, 6)]
    for i in range(4):
        j = (i + 1) % 4
        F += [(i, j, 4 + j), (i, 4 + j, 4 + i)]
    return V, np.array(F, dtype=np.int64)


def box(sx, sy, sz):
    return prism([(-sx / 2, -sy / 2), (-sx / 2, sy / 2), (sx / 2, sy / 2), (sx / 2, -sy / 2)], -sz / 2, sz / 2)


def uv_sphere(stacks=10, slices=12):
    """the unit UV sphere: 2 * slices + 2 * slices * (stacks - 2) faces (216)"""
    V = [(0., 0., 1.)]
    for i in range(1, stacks):
        th = np.pi * i / stacks
        V += [(np.sin(th) * np.cos(2 * np.pi * j / slices), np.sin(th) * np.sin(2 * np.pi * j / slices), np.cos(th)) for j in range(slices)]
    V.append((0., 0., -1.))
    ring = lambda i, j: 1 + (i - 1) * slices + j % slices
    F = [(0, ring(1, j), ring(1, j + 1)) for j in range(slices)]
    for i in range(1, stacks - 1):
        for j in range(slices):
            F += [(ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)), (ring(i, j), ring(i + 1, j + 1), ring(i, j + 1))]
    F += [(len(V) - 1, ring(stacks - 1, j + 1), ring(stacks - 1, j)) for j in range(slices)]
    return np.array(V), np.array(F, dtype=np.int64)


def placement(centre, angle=0., scale=1.):
    """x -> R_y(angle) scale x + centre as a 3 x 4 matrix"""
    c, s = np.cos(angle), np.sin(angle)
    return np.concatenate([np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) * scale, np.asarray(centre, dtype=np.float64)[:, None]], 1)


def cpu_masks(meshes):
    return [model.mask_from_mesh(model.place(V, FLIP @ T), F, H, W, K) for V, F, T in meshes]


def boxes_on_axis(x0=-.3):
    """three axis-aligned unit boxes near the camera axis at z = 4, 6, 8 (index 0 the nearest), shifted so that their masks overlap only
    partly and no centroid ray runs through a cap's diagonal; x0: where box 0 sits"""
    V, F = box(1., 1., 1.)
    return [(V, F, placement((x0, .1, 4.))), (V, F, placement((0., 0., 6.))), (V, F, placement((.3, -.15, 8.)))]


def scene_s():
    """-> (meshes [(V, F, T)] * 4, w2c)"""
    chevron = prism([(-3., -1.5), (0., 1.5), (3., -1.5), (0., 0.)], -.4, .4)
    meshes = [box(1.2, 1.03, .8) + (placement((-.62, .01, 4.), .4),),
              uv_sphere() + (placement((.31, .22, 6.), .7),),
              chevron + (placement((0., 0., 8.), -.6),),
              box(8., .6, .6) + (placement((.05, -1.3, 7.), -.6),)]
    c, s = np.cos(.1), np.sin(.1)
    w2c = np.array([[c, 0, s, 0.], [0, 1, 0, -.4], [-s, 0, c, 0.], [0, 0, 0, 1.]])
    return meshes, w2c


def assert_margins(res):
    assert res["z_gap"] > MARGIN and res["margin"] > MARGIN, (res["z_gap"], res["margin"])


# ---- 1. the model on hand-computed scenes, the host functions, the entry's refusals (no GPU) ---------------------------------------------------
def test_three_boxes_are_ordered_farthest_first():
    meshes = boxes_on_axis()
    res = model.occlusion_order(cpu_masks(meshes), meshes, np.eye(4), K, "camera")
    assert (res["stats"][[0, 0, 1], [1, 2, 2], 0] > 0).all()                     # the masks overlap pairwise
    assert_margins(res)
    assert res["z"] == {(0, 1): (3.5, 5.5), (0, 2): (3.5, 7.5), (1, 2): (5.5, 7.5)}      # the centres of the front caps
    expect = np.zeros((3, 3), dtype=np.int8)
    expect[1, 0] = expect[2, 0] = expect[2, 1] = 1
    assert (res["before"] == expect).all() and res["order"] == [2, 1, 0]


def test_an_instance_without_overlap_gets_no_edge_and_keeps_its_place():
    from snerf_amd import foreground
    meshes = boxes_on_axis(x0=-2.6)                                               # box 0 moved sideways, out of the others' masks
    res = model.occlusion_order(cpu_masks(meshes), meshes, np.eye(4), K, "camera")
    assert res["stats"][0, 1, 0] == 0 and res["stats"][0, 2, 0] == 0 and res["stats"][1, 2, 0] > 0
    expect = np.zeros((3, 3), dtype=np.int8)
    expect[2, 1] = 1
    assert (res["before"] == expect).all()
    assert res["order"] == [0, 2, 1] and foreground.topological_order(res["before"]) == [0, 2, 1]     # the loop emits 0 first: nothing precedes it


def test_no_overlap_at_all_keeps_the_given_order():
    from snerf_amd import foreground
    masks = [np.zeros((H, W, 3), dtype=np.uint8) for _ in range(4)]
    for k, m in enumerate(masks):
        m[5 * k:5 * k + 4, 10 * k:10 * k + 8] = 255
    V, F = box(1., 1., 1.)
    res = model.occlusion_order(masks, [(V, F, None)] * 4, np.eye(4), K, "camera")
    assert not res["before"].any() and res["order"] == [0, 1, 2, 3]
    assert foreground.topological_order(np.zeros((4, 4), dtype=np.int8)) == [0, 1, 2, 3]


def test_a_cycle_raises():
    from snerf_amd import foreground
    cyclic = np.zeros((3, 3), dtype=np.int8)
    cyclic[0, 1] = cyclic[1, 2] = cyclic[2, 0] = 1
    for sort in (model.topological_order, foreground.topological_order):
        with pytest.raises(RuntimeError, match=r"Occlusion judgment fails\.\.\.\."):
            sort(cyclic)
    chain = np.zeros((4, 4), dtype=np.int8)
    chain[3, 1] = chain[1, 0] = chain[2, 0] = 1
    assert foreground.topological_order(chain) == model.topological_order(chain) == [2, 3, 1, 0]


def test_scene_s_keeps_its_margins_in_both_ray_frames():
    """what the GPU comparison rests on, checked on the host masks: the two patches of (chevron, bar), the fallback, the margins"""
    meshes, w2c = scene_s()
    masks = cpu_masks(meshes)
    inter = (masks[2][..., 0] > 0) & (masks[3][..., 0] > 0)
    cols = np.nonzero(inter.any(0))[0]
    assert cols.size and np.diff(cols).max() > 10                                # two patches, a gap between them
    cam = model.occlusion_order(masks, meshes, w2c, K, "camera")
    ref = model.occlusion_order(masks, meshes, w2c, K, "reference")
    assert_margins(cam)
    assert_margins(ref)
    assert sorted(cam["z"]) == [(0, 1), (0, 2), (1, 2), (2, 3)]                  # the bar overlaps neither the box nor the sphere
    assert cam["faces"][2, 3][0] == -1 and cam["faces"][2, 3][1] >= 0            # the centroid ray misses the chevron and hits the bar
    assert all(f >= 0 for pair in ((0, 1), (0, 2), (1, 2)) for f in cam["faces"][pair])
    hits = [f >= 0 for pair in ref["faces"].values() for f in pair]
    assert any(hits) and hits.count(False) >= 3 and ref["faces"][2, 3][1] == -1  # world-frame rays: some hit, the fallback elsewhere
    assert cam["before"][2, 3] == 1 and ref["before"][3, 2] == 1                 # the frames disagree about (chevron, bar)
    assert cam["order"] == [2, 1, 0, 3] and ref["order"] == [3, 2, 1, 0]


def test_occlusion_level_thresholds():
    from snerf_amd.foreground import occlusion_level
    lo, hi = np.nextafter(.01, 0), np.nextafter(.01, 1)
    assert [occlusion_level(v) for v in (0., lo, .01, hi)] == [0, 0, 1, 1]
    assert [occlusion_level(v) for v in (np.nextafter(.5, 0), .5, np.nextafter(.5, 1))] == [1, 2, 2]
    assert [occlusion_level(v) for v in (np.nextafter(.99, 0), .99, np.nextafter(.99, 1), 1.)] == [2, 3, 3, 3]


def test_bbox_result_and_save_bbox_results(tmp_path):
    from snerf_amd import foreground
    w2c = np.array([[0., -1., 0., 1.], [0., 0., -1., 2.], [1., 0., 0., 3.], [0., 0., 0., 1.]])
    car = foreground.bbox_result(w2c, (10., 2., .5), 30., .25, "vehicle", (1.5, 1.8, 4.2))
    assert car["category"] == "Car" and car["occlution"] == 1 and car["confidence"] == 1
    assert (car["height"], car["width"], car["length"]) == (1.5, 1.8, 4.2)
    assert (car["pos_x"], car["pos_y"], car["pos_z"]) == (-1., 1.5, 13.)
    assert all(car[k] == 0. for k in ("alpha", "xmin", "ymin", "xmax", "ymax", "truncated"))
    # M = rot_w2c @ Rz(30 deg) @ rot_axis.T has first row (-sin 30, 0, -cos 30): rot_y = atan2(-cos 30, -sin 30) - pi / 2 = -120 - 90 degrees
    assert abs(car["rot_y"] + 7 * np.pi / 6) < 1e-14
    person = foreground.bbox_result(w2c, (0., 0., 0.), 0., .995, "person", (.5, .6, 1.7))
    assert person["category"] == "Pedestrain" and person["occlution"] == 3
    assert (person["length"], person["width"], person["height"]) == (.5, .6, 1.7)
    bike = foreground.bbox_result(w2c, (0., 0., 0.), 0., 0., "bicycle", (.6, 1.1, 1.8))
    assert bike["category"] == "Bicycle" and (bike["width"], bike["height"], bike["length"]) == (.6, 1.1, 1.8)
    moto = foreground.bbox_result(w2c, (0., 0., 0.), 0., .6, "motorcycle", (.7, 1.2, 2.))
    assert moto["category"] == "Motorcycle" and moto["occlution"] == 2 and (moto["width"], moto["height"], moto["length"]) == (.7, 1.2, 2.)
    thing = foreground.bbox_result(w2c, (0., 0., 0.), 0., 0., "object", (1., 1., 1.))
    assert thing["category"] == "Object" and not {"height", "width", "length"} & set(thing)      # as in the reference
    path = tmp_path / "000000.txt"
    foreground.save_bbox_results(str(path), [car, person])
    assert path.read_bytes() == (b"Car 0.000000 1 0.000000 0.000000 0.000000 0.000000 0.000000 1.500000 1.800000 4.200000 -1.000000 1.500000 13.000000 -3.665191 1.000000\n"
                                 b"Pedestrain 0.000000 3 0.000000 0.000000 0.000000 0.000000 0.000000 1.700000 0.600000 0.500000 1.000000 2.000000 3.000000 -3.141593 1.000000\n")


def test_rot_y_closed_form_matches_scipy():
    Rotation = pytest.importorskip("scipy.spatial.transform").Rotation
    from snerf_amd import foreground
    rng = np.random.default_rng(5)
    rot_axis = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]])
    n = 0
    while n < 12:
        w2c = np.eye(4)
        w2c[:3, :3] = Rotation.from_rotvec(rng.normal(size=3) * 1.5).as_matrix()
        w2c[:3, 3] = rng.normal(size=3)
        theta = rng.uniform(-180., 180.)
        M = w2c[:3, :3] @ Rotation.from_euler("z", theta, degrees=True).as_matrix() @ rot_axis.T
        if abs(M[0, 1]) > .99:                                                  # the gimbal lock of 'yzx'
            continue
        n += 1
        expect = Rotation.from_matrix(M).as_euler("yzx", degrees=False)[0] - np.pi / 2
        assert abs(foreground.rot_y(w2c, theta) - expect) < 1e-12
        assert foreground.bbox_result(w2c, (0., 0., 0.), theta, 0., "vehicle", (1., 1., 1.))["rot_y"] == foreground.rot_y(w2c, theta)


@built
def test_overlap_entry_refuses_bad_arguments_without_a_gpu():
    """argument validation happens before any launch (the pattern of test_abi.py): host addresses that are never looked behind"""
    host = (ctypes.c_char * 64)()
    A = (ctypes.addressof(host) + 15) & ~15
    ptrs = lambda n, hole=None: (ctypes.c_void_p * n)(*[None if k == hole else A for k in range(n)])
    good = dict(masks=ptrs(2), N=2, H=4, W=4, stats=A)
    for change in (dict(N=1), dict(N=33, masks=ptrs(33)), dict(N=0), dict(H=0), dict(H=65536), dict(W=0), dict(W=65536), dict(masks=None),
                   dict(stats=None), dict(masks=ptrs(2, hole=0)), dict(masks=ptrs(2, hole=1)), dict(N=32, masks=ptrs(32, hole=31))):
        a = dict(good, **change)
        with pytest.raises(_lib.SnerfHipError, match="bad argument"):
            _lib.call("snerf_fg_overlap", a["masks"], a["N"], a["H"], a["W"], a["stats"], None)


def test_composite_frame_order_occlusion_needs_every_mesh():
    from snerf_amd import foreground
    frame = (torch.zeros(4, 4, 3, dtype=torch.uint8), torch.zeros(4, 4), torch.zeros(4, 4, dtype=torch.uint8))
    mask = torch.zeros(4, 4, 3, dtype=torch.uint8)
    instances = [dict(image=mask, mask=mask, mesh=(object(), None), intrinsic=K), dict(image=mask, mask=mask, category="person", intrinsic=K)]
    with pytest.raises(ValueError, match=r"instance 1 \(person\) has no mesh"):
        foreground.composite_frame(*frame, instances, order="occlusion", w2c=np.eye(4), intrinsic=K)
    with pytest.raises(ValueError, match="needs w2c"):
        foreground.composite_frame(*frame, instances[:1], order="occlusion", intrinsic=K)
    with pytest.raises(ValueError, match="needs w2c"):
        foreground.composite_frame(*frame, instances[:1], order="occlusion", w2c=np.eye(4))
    with pytest.raises(ValueError, match="order must be"):
        foreground.composite_frame(*frame, instances, order="depth")


# ---- 2. the overlap statistics on the device --------------------------------------------------------------------------------------------------
def _device_stats(masks):
    from snerf_amd import foreground
    dev = [torch.from_numpy(np.ascontiguousarray(m)).cuda() for m in masks]
    first = foreground.overlap_stats(dev)
    second = foreground.overlap_stats(dev)
    assert first.dtype == torch.int64 and tuple(first.shape) == (len(masks), len(masks), 3)
    assert torch.equal(first, second)                                           # a second call: the same bytes
    return first.cpu().numpy()


def _check_stats(masks):
    got, expect = _device_stats(masks), model.overlap_stats(masks)
    lower = np.tril(np.ones(got.shape[:2], dtype=bool))
    assert not got[lower].any()                                                 # a >= b stays zero
    assert (got == expect).all(), np.argwhere(got != expect)[:8]
    return got


def _random_masks(n, h, w, density, seed, planes=False, values=(255,)):
    """planes: one plane three times (the reference's masks); else three independent channels"""
    rng = np.random.default_rng(seed)
    shape = (h, w, 1) if planes else (h, w, 3)
    return [np.broadcast_to(np.where(rng.random(shape) < density, rng.choice(values, size=shape), 0).astype(np.uint8), (h, w, 3)).copy()
            for _ in range(n)]


@gpu
@pytest.mark.parametrize("n", [2, 3, 5])
def test_overlap_stats_small_odd_frame(n):
    _check_stats(_random_masks(n, 37, 53, .4, seed=n, planes=True))
    _check_stats(_random_masks(n, 37, 53, .4, seed=10 + n))                      # channels that differ: triples are counted, not pixels


@gpu
def test_overlap_stats_one_pixel():
    one = np.full((1, 1, 3), 255, dtype=np.uint8)
    assert _check_stats([one, one])[0, 1].tolist() == [3, 0, 0]
    assert not _check_stats([one, np.array([[[0, 7, 0]]], dtype=np.uint8), np.array([[[0, 0, 1]]], dtype=np.uint8)])[1, 2].any()


@gpu
def test_overlap_stats_all_496_pairs():
    got = _check_stats(_random_masks(32, 19, 23, .3, seed=32))
    assert (got[np.triu(np.ones((32, 32), dtype=bool), 1)][:, 0] > 0).all()


@gpu
def test_overlap_stats_values_and_constant_masks():
    masks = _random_masks(3, 37, 53, .5, seed=7, values=(1, 255, 2, 128))        # the test is > 0
    masks += [np.zeros((37, 53, 3), dtype=np.uint8), np.full((37, 53, 3), 255, dtype=np.uint8), np.full((37, 53, 3), 1, dtype=np.uint8)]
    got = _check_stats(masks)
    assert not got[:, 3].any() and not got[3].any()                             # the empty mask overlaps nothing
    assert got[4, 5].tolist() == [3 * 37 * 53, 3 * 53 * 37 * 36 // 2, 3 * 37 * 53 * 52 // 2]


@gpu
def test_overlap_stats_sums_beyond_32_bits():
    h, w = 1024, 2048
    full = np.full((h, w, 3), 255, dtype=np.uint8)
    got = _check_stats([full, full])
    assert got[0, 1].tolist() == [3 * h * w, 3 * w * h * (h - 1) // 2, 3 * h * w * (w - 1) // 2] and got[0, 1, 2] > 2 ** 32


@gpu
def test_overlap_stats_of_unaligned_views():
    """masks that are views at an odd byte offset take the byte-wise loads: the same numbers"""
    from snerf_amd import foreground
    masks = _random_masks(3, 21, 17, .5, seed=3)
    flat = [torch.zeros(21 * 17 * 3 + 16, dtype=torch.uint8, device="cuda") for _ in masks]
    views = []
    for k, (m, f) in enumerate(zip(masks, flat)):
        v = f[2 * k + 1:2 * k + 1 + m.size].view(21, 17, 3)
        v.copy_(torch.from_numpy(m))
        views.append(v)
    assert (foreground.overlap_stats(views).cpu().numpy() == model.overlap_stats(masks)).all()


# ---- 3. occlusion_order and composite_frame(order="occlusion") on scene S ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device_scene():
    """scene S on the device: tracers, placements, the masks mask_from_mesh gives there, and the model's answers ON THOSE MASKS"""
    from snerf_amd import foreground, meshtrace
    meshes, w2c = scene_s()
    tracers = [meshtrace.RayTracer(V.astype(np.float32), F) for V, F, _ in meshes]
    transforms = [T.astype(np.float32) for _, _, T in meshes]
    masks = [foreground.mask_from_mesh(t, (W, H), K, transform=(FLIP @ T).astype(np.float32)) for t, (_, _, T) in zip(tracers, meshes)]
    host_masks = [m.cpu().numpy() for m in masks]
    fp32 = [(V.astype(np.float32), F, T.astype(np.float32)) for V, F, T in meshes]               # what the device holds
    expect = {frame: model.occlusion_order(host_masks, fp32, w2c, K, frame) for frame in ("reference", "camera")}
    return dict(meshes=meshes, w2c=w2c, tracers=tracers, transforms=transforms, masks=masks, expect=expect)


@gpu
@pytest.mark.parametrize("ray_frame", ["reference", "camera"])
def test_occlusion_order_equals_the_model(device_scene, ray_frame):
    from snerf_amd import foreground
    s, expect = device_scene, device_scene["expect"][ray_frame]
    assert_margins(expect)
    assert len(expect["z"]) == 4 and -1 in [f for pair in expect["faces"].values() for f in pair]
    if ray_frame == "camera":
        assert expect["faces"][2, 3][0] == -1 and expect["faces"][2, 3][1] >= 0  # two patches: the ray misses the chevron, hits the bar
    other = device_scene["expect"]["camera" if ray_frame == "reference" else "reference"]
    assert (expect["before"] != other["before"]).any()                          # the wrong frame's ray would not pass
    order, before = foreground.occlusion_order(s["masks"], list(zip(s["tracers"], s["transforms"])), s["w2c"], K, ray_frame=ray_frame)
    assert before.dtype == np.int8 and (before == expect["before"]).all(), (before, expect["before"])   # every pair
    assert order == expect["order"]


@gpu
def test_face_centers_follow_the_callers_numbering(device_scene):
    s = device_scene
    V, F, T = s["meshes"][1]
    ids = torch.tensor([0, 5, 215, -1, 100], device="cuda")
    got = s["tracers"][1].face_centers(ids, s["transforms"][1]).cpu().numpy()
    expect = model.place(V.astype(np.float32), T.astype(np.float32))[F[[0, 5, 215, 215, 100]]].mean(1)
    assert got.dtype == np.float64 and np.abs(got - expect).max() < 1e-12


@gpu
def test_composite_frame_sorts_by_occlusion(device_scene):
    from snerf_amd import foreground
    s = device_scene
    g = torch.Generator().manual_seed(4)
    bg = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).cuda()
    depth = (torch.randint(5 * 256, 9 * 256, (H, W), generator=g).float() / 256).cuda()          # between the instances' depths
    sem = torch.tensor([0, 1, 5, 8, 13], dtype=torch.uint8)[torch.randint(0, 5, (H, W), generator=g)].cuda()
    cats = ["vehicle", "person", "vehicle", "bicycle"]
    inst = [dict(image=torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).cuda(), mask=s["masks"][k], category=cats[k], r=3,
                 mesh=(s["tracers"][k], s["transforms"][k]), intrinsic=K) for k in range(4)]
    # the chevron comes as a mesh to be rendered: it is rendered before the order is taken, and its mask is the tracer's
    from snerf_amd import meshrender
    V, F, T = s["meshes"][2]
    renderer = meshrender.MeshRenderer(V.astype(np.float32), F, vertex_color=np.random.default_rng(2).random((len(V), 3)).astype(np.float32))
    to_renderer = (FLIP @ T).astype(np.float32)                                 # the renderer's camera looks down -z
    assert torch.equal(renderer.render(K[0, 0], K[1, 1], K[0, 2], K[1, 2], H, W, transform=to_renderer)[1], s["masks"][2])
    del inst[2]["image"], inst[2]["mask"]
    inst[2]["render"] = (renderer, to_renderer)
    scramble = [2, 0, 3, 1]                                                     # instances[i] = scene mesh scramble[i]
    given = [inst[k] for k in scramble]
    want = model.occlusion_order([s["masks"][k].cpu().numpy() for k in scramble],
                                 [(s["meshes"][k][0].astype(np.float32), s["meshes"][k][1], s["transforms"][k]) for k in scramble], s["w2c"], K)
    assert_margins(want)
    assert want["order"] != [0, 1, 2, 3]
    got = foreground.composite_frame(bg.clone(), depth.clone(), sem.clone(), given, order="occlusion", w2c=s["w2c"], intrinsic=K)
    ref = foreground.composite_frame(bg.clone(), depth.clone(), sem.clone(), [given[i] for i in want["order"]])
    assert got["order"] == want["order"] and "order" not in ref
    for name in ("fuse", "mask", "bound", "occluded_mask", "depth", "semantic"):
        assert torch.equal(got[name], ref[name]), name
    assert torch.equal(torch.stack(got["occlusion"]), torch.stack(ref["occlusion"]))
    assert float(torch.stack(got["occlusion"]).max()) > .05                      # the background occludes something: the depth test ran
