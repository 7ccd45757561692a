#!/usr/bin/env python3
"""Golden vectors for the projected mesh shadow (snerf_amd.shadow): runs the REFERENCE's own stage-3 helpers
(s-nerfpp/stage3_code/utils.py: process_mesh :339-354, project_to_ground :130-154, project :157-168, points_to_mask :171-192,
check_the_occlusion :214-225) on seeded cases and records the inputs and the output of every one of them as
tests/golden/g18_foreground_shadow.npz -- the stage-3 member of the g18_foreground family of oracle/gen_golden_foreground.py.  For one
blurred array, an image and a total mask it also records check_the_occlusion and the expression of mesh_shadow.py:100-105 evaluated in
numpy.  Build-container only (needs /root/reference).

utils.py imports cv2, imageio and trimesh at module level; the five functions use none of them, so each is replaced by an empty
stand-in.  cv2 being absent, `interpolate` and `cv2.blur` cannot be recorded: the closed mask and the blurred array of the last record
come from tests/shadow_cpu_model.py (OpenCV's definitions).

Every case asserts that no projected coordinate lies within 1e-7 of an integer (and none where the reference's uint16 cast would wrap),
reseeding otherwise: device and numpy float64 differ by ~1e-13 through the order of the products, and this margin is what lets the
splat be compared bit for bit."""
import importlib.util
import os
import sys
import types

sys.dont_write_bytecode = True
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
from oracle import common as _oracle_common  # noqa: E402  (save_golden: writes the fixture, or compares under --check)
import shadow_cpu_model as model  # noqa: E402
OUT = os.path.join(REPO, "tests", "golden")
REF = "/root/reference/s-nerfpp/stage3_code"
N_POINTS = 500
MARGIN = 1e-7
# (H, W, theta, bbox_center, mesh_bias, pitch, yaw, ground_height)
CASES = [(96, 160, 31., (4.0, 2.2, 0.1), (0.1, -0.05, 0.0), 38., 115., None),
         (70, 129, -72.5, (5.5, -1.9, -0.2), (0.0, 0.2, 0.05), 25., -40., 0.0),
         (48, 64, 158., (4.0, 1.0, 0.3), (-0.2, 0.0, 0.1), 52., 200., -0.45)]


def load_utils():
    for name in ("cv2", "imageio", "trimesh"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    spec = importlib.util.spec_from_file_location("stage3_utils", os.path.join(REF, "utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def camera(rng, H, W):
    """c2w of a camera 1.5 m above the origin looking along world +x (z up; camera x right, y down, z forward), turned a little, and P"""
    base = np.array([[0., 0., 1.], [-1., 0., 0.], [0., -1., 0.]])
    ang = rng.uniform(-0.08, 0.08, 3)
    cx, sx, cy, sy, cz, sz = np.cos(ang[0]), np.sin(ang[0]), np.cos(ang[1]), np.sin(ang[1]), np.cos(ang[2]), np.sin(ang[2])
    turn = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    c2w = np.eye(4)
    c2w[:3, :3] = turn @ base
    c2w[:3, 3] = [rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), 1.5 + rng.uniform(-0.1, 0.1)]
    f = 0.75 * W
    P = np.array([[f, 0., W / 2 - 0.37], [0., f * 1.02, H / 2 + 0.21], [0., 0., 1.]])
    return c2w, P


def one_case(utils, k, seed):
    H, W, theta, centre, bias, pitch, yaw, ground = CASES[k]
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(3, N_POINTS))
    d /= np.linalg.norm(d, axis=0, keepdims=True)
    mesh_points = d * np.array([[2.1], [0.9], [0.75]]) + np.array([[0.], [0.], [0.75]])          # a car-sized ellipsoid standing on z = 0
    c2w, P = camera(rng, H, W)
    placed, _ = utils.process_mesh(mesh_points, np.zeros((3, 1)), centre, theta, bias)
    grounded = utils.project_to_ground(placed, pitch, yaw, ground)
    projected = utils.project(grounded, c2w, P)
    with np.errstate(all="ignore"):
        mask = utils.points_to_mask(projected, np.zeros((H, W, 3), np.uint8))
    x, y = model.pixel_coordinates(projected)
    q = np.concatenate([x, y])
    if not np.isfinite(q).all() or np.abs(q).max() >= 6e4 or np.abs(q - np.round(q)).min() <= MARGIN:
        return None
    # the model restates the same expressions: it must give the same bits here, before anything is written
    m_placed = model.process_mesh(mesh_points, centre, theta, bias)
    assert np.array_equal(m_placed, placed), "process_mesh"
    assert np.array_equal(model.project_to_ground(placed, pitch, yaw, ground), grounded), "project_to_ground"
    assert np.array_equal(model.project(grounded, c2w, P), projected), "project"
    assert np.array_equal(model.points_to_mask(projected, H, W), mask), "points_to_mask"
    n_set = int((mask[..., 0] > 0).sum())
    assert 50 < n_set and ((x < 0) | (x >= W) | (y < 0) | (y >= H)).any(), (n_set, "the case should set pixels and clip some points")
    pre = f"c{k}_"
    rec = {pre + "hw": np.array([H, W], np.int64), pre + "mesh_points": mesh_points, pre + "bbox_center": np.array(centre), pre + "theta": np.float64(theta),
           pre + "mesh_bias": np.array(bias), pre + "pitch": np.float64(pitch), pre + "yaw": np.float64(yaw),
           pre + "ground": np.float64(np.nan if ground is None else ground), pre + "ground_none": np.bool_(ground is None), pre + "c2w": c2w, pre + "P": P,
           pre + "placed": placed, pre + "grounded": grounded, pre + "projected": projected, pre + "mask": np.packbits(mask[..., 0] > 0, axis=1),
           pre + "mask_channels_equal": np.bool_((mask[..., 0] == mask[..., 1]).all() and (mask[..., 0] == mask[..., 2]).all() and set(np.unique(mask)) <= {0, 255})}
    print(f"case {k}: seed {seed}, {n_set} pixels set, nearest integer {np.abs(q - np.round(q)).min():.2e}")
    return rec, mask


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference tree not present")
    utils = load_utils()
    arrays, masks = {}, []
    for k in range(len(CASES)):
        seed = 1800 + 10 * k
        while True:
            got = one_case(utils, k, seed)
            if got is not None:
                break
            seed += 1
        arrays.update(got[0])
        masks.append(got[1])
    # occlusion and fuse arithmetic, on the blurred closed mask of case 0
    H, W = CASES[0][:2]
    rng = np.random.default_rng(18)
    closed = model.interpolate(masks[0], 20, 3)
    any_, kw, kh = model.blur_kernel(closed)
    assert any_
    blurred = np.repeat((model.box_counts(closed[..., 0] > 0, kw, kh) * (1.0 / (kw * kh)))[..., None], 3, axis=2)
    im = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    im[:8, :40], im[8:16, :40], im[16:24, :40], im[24:32, :40] = 0, 20, 200, 255
    total = np.zeros((H, W, 3), np.uint8)
    ys, xs = np.nonzero(closed[..., 0])
    total[ys.min():(ys.min() + ys.max()) // 2, xs.min():(xs.min() + xs.max()) // 2, 0] = 255
    total[ys.min():ys.max(), (xs.min() + xs.max()) // 2:, 1] = 255
    total[:, : W // 3, 2] = 7                                            # any value > 0 occludes
    light_scale = .55
    occ = utils.check_the_occlusion(total, blurred)
    # mesh_shadow.py:100-105
    masked_blured_shadow = blurred * occ / 255
    weighted_shadow = light_scale * masked_blured_shadow
    fused = np.uint8(im * (1 - weighted_shadow))
    assert np.array_equal(model.check_the_occlusion(total, blurred), occ) and np.array_equal(model.fuse(im, total, blurred, light_scale), fused)
    assert (fused != im).any() and (occ[..., 0] != occ[..., 1]).any()
    arrays.update(f_blurred=blurred[..., 0], f_kernel=np.array([kw, kh], np.int64), f_im=im, f_total=total, f_light_scale=np.float64(light_scale), f_occ=occ,
                  f_fused=fused)
    path = os.path.join(OUT, "g18_foreground_shadow.npz")
    _oracle_common.save_golden(path, **arrays)
    if "--check" not in sys.argv:
        print(f"wrote g18_foreground_shadow.npz: {os.path.getsize(path)} bytes, kernel {kw} x {kh}")
        assert os.path.getsize(path) <= 256 * 1024


if __name__ == "__main__":
    main()
