"""CPU model of the projected mesh shadow (snerf_amd.shadow, csrc/shadow.hip): plain numpy float64, the whole of
s-nerfpp/stage3_code/mesh_shadow.py:47-111 for one frame and one instance.

Pinned by the reference's own functions (tests/golden/g18_foreground_shadow.npz, tools/gen_golden_shadow.py): process_mesh,
project_to_ground, project, points_to_mask, check_the_occlusion and the fuse expression of mesh_shadow.py:100-105 -- they are restated
here expression by expression, so the fixture compares bit for bit.

PARITY UNPINNED (cv2 is not installed where this was written): `interpolate`'s closing and `cv2.blur` follow OpenCV's published
definitions --
  dilate / erode: dst(x, y) = max / min over 0 <= x', y' < r of src(x + x' - r // 2, y + y' - r // 2), pixels outside the (padded) image
      never win; iterations = n is n successive applications; MORPH_CLOSE = n dilations, then n erosions, same un-reflected window;
  blur: normalised box filter, anchor (kw // 2, kh // 2), BORDER_REFLECT_101; on a 0 / 1 image the window sum is an integer count and
      blurred = count * (1.0 / (kw * kh)).

Documented divergence from points_to_mask: a projected coordinate that is not finite, negative or >= 65536 is dropped (the reference's
float -> uint16 cast wraps those around)."""
from math import cos, pi, sin

import numpy as np


def rot_z(theta):
    """scipy's Rotation.from_euler('z', theta, degrees=True).as_matrix(), operation by operation: the unit quaternion (0, 0, sin(t / 2),
    cos(t / 2)), not re-normalised, then its matrix (20 000 random angles compared bit for bit when the fixture was made)"""
    half = np.deg2rad(theta) / 2
    z, w = np.sin(half), np.cos(half)
    z2, w2, zw = z * z, w * w, z * w
    m = np.zeros((3, 3))
    m[0, 0] = -z2 + w2
    m[1, 0] = 2 * zw
    m[0, 1] = -2 * zw
    m[1, 1] = -z2 + w2
    m[2, 2] = z2 + w2
    return m


def process_mesh(mesh_points, bbox_center, theta, bias, rot=None):
    """utils.py:339-354 (the points only): [3,N] float64 -> [3,N]"""
    rot = rot_z(theta) if rot is None else rot
    mesh_points = rot @ mesh_points + np.array(bbox_center).reshape((3, 1))
    return mesh_points + rot @ np.array(bias).reshape((3, 1))


def light_vector(pitch_angle, yaw_angle):
    pitch_angle, yaw_angle = pitch_angle / 180 * pi, yaw_angle / 180 * pi
    return np.array([sin(pitch_angle) * cos(yaw_angle), sin(pitch_angle) * sin(yaw_angle), cos(pitch_angle)])


def project_to_ground(points_3D, pitch_angle, yaw_angle, ground_height):
    """utils.py:130-154, with its quirk: `not ground_height` is true for None and for 0.0"""
    if points_3D.size == 0:
        return points_3D
    if not ground_height:
        ground_height = np.sort(points_3D[2, ...].copy())[0]          # np.median(z[:1]) of the sorted z: NaN sorts last
    light_vec = light_vector(pitch_angle, yaw_angle)
    coef = (points_3D[2, ...] - ground_height) / light_vec[2]
    return points_3D - light_vec.reshape((3, 1)) * coef


def project(points_3D, c2w, P):
    """utils.py:157-168"""
    world_coords = np.concatenate((points_3D, np.ones((1, points_3D.shape[1]))), axis=0)
    cam_coords = np.linalg.inv(c2w) @ world_coords
    return P @ cam_coords[:3, ...]


def pixel_coordinates(points_2D):
    """the quotients points_to_mask truncates: (x [N], y [N]) float64"""
    with np.errstate(all="ignore"):
        q = points_2D / points_2D[2, :]
    return q[0], q[1]


def points_to_mask(points_2D, H, W):
    """utils.py:171-192 -> [H,W,3] uint8, with the documented drop rule instead of the uint16 wrap-around"""
    x, y = pixel_coordinates(points_2D)
    with np.errstate(all="ignore"):
        ok = (x >= 0) & (x < 65536) & (y >= 0) & (y < 65536)
    xi, yi = x[ok].astype(np.int64), y[ok].astype(np.int64)
    keep = (xi > 0) & (xi < W) & (yi > 0) & (yi < H)
    mask = np.zeros((H, W, 3), dtype=bool)
    mask[yi[keep], xi[keep], ...] = True
    return mask.astype(np.uint8) * 255


def _window(img, r, erode):
    """one dilation (erosion) of a 2-D bool image by the r x r window [-(r // 2), r - 1 - r // 2]; outside never wins"""
    a = r // 2
    for axis in (0, 1):
        n = img.shape[axis]
        acc = np.ones_like(img) if erode else np.zeros_like(img)
        for d in range(max(-a, -n), min(r - a, n + 1)):
            sh = np.ones_like(img) if erode else np.zeros_like(img)        # sh[x] = img[x + d]
            src = [slice(None)] * 2
            dst = [slice(None)] * 2
            src[axis] = slice(max(d, 0), n + min(d, 0))
            dst[axis] = slice(max(-d, 0), n + min(-d, 0))
            sh[tuple(dst)] = img[tuple(src)]
            acc = acc & sh if erode else acc | sh
        img = acc
    return img


def morph_close(img, r, iter):
    """cv2.morphologyEx(img, MORPH_CLOSE, rect (r, r), iterations=iter) on a 2-D bool image"""
    for _ in range(iter):
        img = _window(img, r, False)
    for _ in range(iter):
        img = _window(img, r, True)
    return img


def interpolate(shadow_mask_mat, r=3, iter=3):
    """utils.py:195-211 on an [H,W,3] uint8 mask (channel 0 decides; the reference's masks carry one plane three times)"""
    h, w, _ = shadow_mask_mat.shape
    padded = np.pad(shadow_mask_mat[..., 0] > 0, ((h, h), (w, w)))
    closed = morph_close(padded, r, iter)[h:2 * h, w:2 * w]
    return np.repeat(closed[..., None], 3, axis=2).astype(np.uint8) * 255


def box_counts(mask01, kw, kh):
    """window sums of a 2-D 0 / 1 array: ksize = (kw, kh), anchor (kw // 2, kh // 2), BORDER_REFLECT_101 -> int64 [H,W]"""
    H, W = mask01.shape
    p = np.pad(mask01.astype(np.int64), ((kh // 2, kh - 1 - kh // 2), (kw // 2, kw - 1 - kw // 2)), mode="reflect")
    c = np.concatenate([np.zeros((p.shape[0], 1), np.int64), np.cumsum(p, axis=1)], axis=1)
    rows = c[:, kw:kw + W] - c[:, :W]
    c = np.concatenate([np.zeros((1, W), np.int64), np.cumsum(rows, axis=0)], axis=0)
    return c[kh:kh + H] - c[:H]


def blur_kernel(shadow_mask_mat):
    """mesh_shadow.py:90-97 -> (any, kw, kh)"""
    m = (shadow_mask_mat > 0).max(-1)
    if not m.max():
        return False, 1, 1
    ys, xs = np.nonzero(m)
    w_size, h_size = float(xs.max() - xs.min()), float(ys.max() - ys.min())
    return True, max(1, int(w_size // 5)), max(1, int(h_size // 5))


def check_the_occlusion(mask_mat, shadow_mask_mat):
    """utils.py:214-225"""
    shadow_mask_mat, mask_mat = shadow_mask_mat > 0, mask_mat > 0
    shadow_mask_mat = np.logical_and(shadow_mask_mat, np.logical_not(np.logical_and(shadow_mask_mat, mask_mat)))
    return shadow_mask_mat.astype(np.uint8) * 255


def fuse(im, total_mask_mat, blured_shadow, light_scale=.55):
    """mesh_shadow.py:100-105 on a blurred [H,W,3] float64 array"""
    shadow_mask_mat_ = check_the_occlusion(total_mask_mat, blured_shadow)
    masked_blured_shadow = blured_shadow * shadow_mask_mat_ / 255
    weighted_shadow = light_scale * masked_blured_shadow
    im_fuse = im * (1 - weighted_shadow)
    return np.uint8(im_fuse)


def blur_shadow(im, total_mask_mat, shadow_mask_mat, light_scale=.55):
    """mesh_shadow.py:89-107 -> (image, dict(any, kw, kh, counts))"""
    any_, kw, kh = blur_kernel(shadow_mask_mat)
    if not any_:
        return im.copy(), dict(any=False, kw=kw, kh=kh, counts=None)
    counts = box_counts(shadow_mask_mat[..., 0] > 0, kw, kh)
    blurred = counts * (1.0 / (kw * kh))
    out = fuse(im, total_mask_mat, np.repeat(blurred[..., None], 3, axis=2), light_scale)
    return out, dict(any=True, kw=kw, kh=kh, counts=counts)


def shadow_mask(vertices, bbox_center, theta, mesh_bias, pitch_angle, yaw_angle, c2w, P, H, W, ground_height=None, check=False):
    """steps 1-4 for vertices [N,3] -> ([H,W,3] uint8, (x, y) the quotients)"""
    pts = process_mesh(np.asarray(vertices, dtype=np.float64).T.reshape(3, -1), bbox_center, theta, mesh_bias)
    if not check:
        pts = project_to_ground(pts, pitch_angle, yaw_angle, ground_height)
    p2 = project(pts, np.asarray(c2w, dtype=np.float64), np.asarray(P, dtype=np.float64))
    return points_to_mask(p2, H, W), pixel_coordinates(p2)


def cast(im, total_mask, vertices, bbox_center, theta, mesh_bias, pitch_angle, yaw_angle, c2w, P, ground_height=None, light_scale=.55, check=False,
         interpolate_r=20, interpolate_iter=3):
    """one instance on one frame -> the new image (the input is not modified)"""
    H, W, _ = im.shape
    mask, _ = shadow_mask(vertices, bbox_center, theta, mesh_bias, pitch_angle, yaw_angle, c2w, P, H, W, ground_height, check)
    mask = interpolate(mask, interpolate_r, interpolate_iter)
    if check:
        out = im.copy()
        out[mask > 0] = 0
        return out
    return blur_shadow(im, total_mask, mask, light_scale)[0]
