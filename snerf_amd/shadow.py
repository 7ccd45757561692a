"""Projected mesh shadows of S-NeRF++ stage 3 on the device: the shadow every inserted instance casts on the ground.

Reference counterpart: s-nerfpp/stage3_code/mesh_shadow.py:21-113 generate_one_shadow (one frame, one instance; `align=False`, what its
`__main__` passes at :152-153) with the helpers of stage3_code/utils.py -- :339-354 process_mesh, :130-154 project_to_ground, :157-168
project, :171-192 points_to_mask, :195-211 interpolate, :214-225 check_the_occlusion, :248-269 shadow_fuse (for `check=True`).  There
every instance re-reads and re-writes the frame's PNG and works on PIL images and numpy index lists; here the frame stays in HBM as the
uint8 tensor `foreground.composite_frame` left (stage 2, the diffusion in-painting in between, is an external network: it consumes and
returns the same uint8 frame) and `ShadowCaster.cast` is a fixed sequence of launches: no host read, no allocation after construction.

Pinned against the reference's own functions (tests/golden/g18_foreground_shadow.npz, tools/gen_golden_shadow.py): the geometry (placement,
ground projection with the `if not ground_height` quirk -- None and 0.0 both mean "the smallest z of the placed points" --, camera
projection, the truncating splat with its strict `0 < x < W`, `0 < y < H`), check_the_occlusion and the fuse arithmetic of
mesh_shadow.py:100-105.

PARITY UNPINNED: cv2 is not installed where this was built, so `interpolate`'s closing (cv2.morphologyEx MORPH_CLOSE, rect (r, r),
iterations) and `cv2.blur` follow OpenCV's published definitions -- the window [x - r // 2, x - r // 2 + r) for dilation and erosion
alike (an even r shifts the result), pixels outside the padded image never win; a normalised box filter with anchor (kw // 2, kh // 2)
and BORDER_REFLECT_101.  tests/shadow_cpu_model.py states both in numpy; include/snerf_hip.h has the details.

Divergences: a projected coordinate that is not finite, negative or >= 65536 is dropped (the reference's float -> uint16 cast wraps
those around and can land a stray pixel in the image); `align=True` (`align_mesh`) is not built, the reference's driver never turns it
on.  Masks cross this API as [H,W,3] uint8 0 / 255 like foreground.py's; channel 0 of a shadow mask decides (the reference's carry one
plane three times), the total mask is tested per channel."""
import ctypes
from math import cos, pi, sin

import numpy as np
import torch

from . import ops
from .ops import _dev, _require, _ws


def process_placement(bbox_center, theta, mesh_bias):
    """utils.py:339-354 process_mesh as a host 3 x 4 float64 matrix: x -> Rz(theta degrees) x + bbox_center + Rz mesh_bias"""
    t = float(theta) / 180 * pi
    rot = np.array([[cos(t), -sin(t), 0.], [sin(t), cos(t), 0.], [0., 0., 1.]])
    shift = np.asarray(bbox_center, dtype=np.float64).reshape(3) + rot @ np.asarray(mesh_bias, dtype=np.float64).reshape(3)
    return np.concatenate([rot, shift[:, None]], axis=1)


def light_vector(pitch_angle, yaw_angle):
    """utils.py:149-151: (sin p cos y, sin p sin y, cos p) from degrees, host float64"""
    p, y = float(pitch_angle) / 180 * pi, float(yaw_angle) / 180 * pi
    return np.array([sin(p) * cos(y), sin(p) * sin(y), cos(p)])


def _host(a, what):
    _require(not (torch.is_tensor(a) and a.is_cuda), "%s: host values (a device matrix would cost a sync per call)", what)
    return np.asarray(a, dtype=np.float64)


def world_to_pixel(c2w, P):
    """utils.py:157-168 project as one host 3 x 4 float64 matrix: P (c2w^-1)[:3]"""
    return _host(P, "P")[:3, :3] @ np.linalg.inv(_host(c2w, "c2w"))[:3, :]


def _pack_xf(xf, placement, light, ground_height, w2p, check=False):
    """fill the 28 host doubles of snerf_shadow_project; -> ground_mode: 2 with check (no ground projection), 1 for the reference's `if
    not ground_height` (None and 0.0: the smallest placed z), else 0"""
    use_min = not ground_height
    xf[0:12] = np.asarray(placement, dtype=np.float64).reshape(12).tolist()
    xf[12:15] = np.asarray(light, dtype=np.float64).reshape(3).tolist()
    xf[15] = 0. if use_min else float(ground_height)
    xf[16:28] = np.asarray(w2p, dtype=np.float64).reshape(12).tolist()
    return 2 if check else int(use_min)


def _vertices(v, device=None):
    if not torch.is_tensor(v):
        v = torch.from_numpy(np.ascontiguousarray(np.asarray(v).reshape(-1, 3)))
    if v.dtype not in (torch.float32, torch.float64):
        v = v.double()
    return v.to(device=device if device is not None else torch.device("cuda", torch.cuda.current_device())).reshape(-1, 3).contiguous()


def project_shadow_mask(vertices, bbox_center, theta, mesh_bias, pitch_angle, yaw_angle, c2w, P, H, W, ground_height=None, check=False, ws=None):
    """steps 1-4 of generate_one_shadow -> the [H,W,3] uint8 splat mask of vertices [N,3] (fp32 or fp64).  With check the ground
    projection is skipped (mesh_shadow.py:70-71)."""
    v = _vertices(vertices, None if ws is None else ws.device)
    ws = _ws(ws, lambda: ops.shadow_ws_bytes(H, W, v.shape[0], 1, 0), torch.uint8, v.device, ops._SHADOW_WS)
    xf = (ctypes.c_double * 28)()
    mode = _pack_xf(xf, process_placement(bbox_center, theta, mesh_bias), light_vector(pitch_angle, yaw_angle), ground_height, world_to_pixel(c2w, P), check)
    mask = torch.empty(H, W, 3, dtype=torch.uint8, device=v.device)
    return ops.shadow_project(v, xf, mode, H, W, ws, mask)


def interpolate(mask, r=20, iter=3):
    """utils.py:195-211 -> a new [H,W,3] uint8 mask"""
    H, W, _ = mask.shape
    _dev("mask", mask, dtype=torch.uint8, shape=(H, W, 3))
    ws = torch.empty(ops.shadow_ws_bytes(H, W, 0, r, iter), dtype=torch.uint8, device=mask.device)
    return ops.shadow_close(mask, H, W, r, iter, ws, torch.empty_like(mask))


def blur_shadow(im, total_mask, shadow_mask, light_scale=.55, ws=None):
    """mesh_shadow.py:89-107, in place on im [H,W,3] uint8"""
    H, W, _ = im.shape
    _dev("im total_mask shadow_mask", im, total_mask, shadow_mask, dtype=torch.uint8, shape=(H, W, 3))
    ws = _ws(ws, lambda: ops.shadow_ws_bytes(H, W, 0, 1, 0), torch.uint8, im.device, ops._SHADOW_WS)
    return ops.shadow_fuse(im, total_mask, shadow_mask, H, W, light_scale, False, ws)


class ShadowCaster:
    """`ShadowCaster(H, W, max_vertices)` owns the scratch of the three stages for H x W frames; `cast` darkens a frame in place."""

    def __init__(self, H, W, max_vertices, interpolate_r=20, interpolate_iter=3, device=None):
        self.H, self.W, self.max_vertices, self.r, self.iter = int(H), int(W), int(max_vertices), int(interpolate_r), int(interpolate_iter)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.ws = torch.empty(ops.shadow_ws_bytes(self.H, self.W, self.max_vertices, self.r, self.iter), dtype=torch.uint8, device=self.device)
        self._xf = (ctypes.c_double * 28)()

    def cast(self, im, total_mask, vertices, bbox_center, theta, mesh_bias, pitch_angle, yaw_angle, c2w, P, ground_height=None, light_scale=.55,
             check=False):
        """mesh_shadow.py:47-111 for one frame and one instance, in place on im [H,W,3] uint8: vertices [N,3] fp32 or fp64 ON THE DEVICE
        (N <= max_vertices), total_mask [H,W,3] uint8 (the frame's mask of all instances: it occludes the shadow), the reference's
        keyword names for the rest (host values).  check: the closed projection of the placed mesh blanks the image instead.
        Instances are cast one after the other on the same im, so shadows multiply.  No host read, no allocation."""
        H, W = self.H, self.W
        _dev("im", im, dtype=torch.uint8, shape=(H, W, 3))
        if not check:
            _dev("total_mask", total_mask, dtype=torch.uint8, shape=(H, W, 3))
        _require(torch.is_tensor(vertices) and vertices.is_cuda and vertices.shape[0] <= self.max_vertices,
                 "vertices: a device tensor of at most max_vertices rows")
        mode = _pack_xf(self._xf, process_placement(bbox_center, theta, mesh_bias), light_vector(pitch_angle, yaw_angle), ground_height,
                        world_to_pixel(c2w, P), check)
        ops.shadow_project(vertices, self._xf, mode, H, W, self.ws)
        ops.shadow_close(None, H, W, self.r, self.iter, self.ws)
        return ops.shadow_fuse(im, None if check else total_mask, None, H, W, light_scale, check, self.ws)
