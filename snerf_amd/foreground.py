"""Image-space foreground composite of S-NeRF++ stage 1 on the device.

Reference counterpart: s-nerfpp/stage1_code/generate_images.py:53-200 (the per-frame loop over the instances in occlusion order) with
utils_render.py:826-1005 handle_occlusion_paste, :306-324 get_bound_im, :327-361 fuse_bound_and_im / fuse_bound and
ip_utils.py:10-19 set_diff.  There every step round-trips PIL images and numpy index lists on the host; here the frame (background
rgb, depth, semantic) stays resident in HBM as uint8 / float tensors and every step is one launch.

The mesh depth behind `fg_depth` and the stage-0 instance masks come from `snerf_amd.meshtrace.RayTracer` (`mesh_depth`,
`mask_from_mesh`: snerf_mesh_prepare + snerf_mesh_trace_pinhole, scratch snerf_mesh_ws_bytes; general rays: snerf_mesh_trace), so
`render_image` -> mesh depth -> paste -> boundary algebra -> `FrameWriter` never leaves the device.  The `raytracing` library the
reference calls is not in its tree: see the meshtrace module docstring for what is and is not pinned.

The instance's own `image` and `mask` (api_code/mesh_renderer.py:36-88, nvdiffrast + kaolin in the reference) come from
`snerf_amd.meshrender.MeshRenderer` (snerf_mesh_render_pinhole, scratch snerf_mesh_render_scratch_bytes): an instance of
`composite_frame` may carry `render = (MeshRenderer, transform)` instead of `image` / `mask`, so mesh -> image + mask -> paste needs
no host round trip either.  The placement of :14-34 is `meshrender.center_mesh_bottom`.

The order in which the instances are pasted (utils_render.py:691-808 occlution_order, called from generate_images.py:76-81) is
`occlusion_order`: pairwise overlap statistics of the instance masks in one launch (snerf_fg_overlap), one centroid ray per overlapping
pair traced against both meshes, the reference's topological sort on the host after ONE small read; `composite_frame(order="occlusion")`
runs it between rendering and pasting.  The KITTI-style label row of an instance (utils_render.py:543-640) is `bbox_result` /
`save_bbox_results` (host, from the `occlusion` scalars composite_frame returns; `occlusion_level` is its threshold rule).

The lighting match (utils_render.py:1008-1051 handle_lighting, which fuse() runs on the whole frame after every paste, :300) is
`handle_lighting`: cv2's 8-bit RGB -> HSV, the instance's V shifted by the difference between the mean V of the unmasked pixels in a box
half as large again around the mask and the mean V of the mask, and HSV -> RGB, in one init launch and three kernels without a host read
(snerf_fg_lighting; the conversions alone: `rgb_to_hsv_u8` / `hsv_to_rgb_u8`, snerf_fg_hsv).  `composite_frame(lighting="frame")` runs
it after each paste as the reference does, `lighting="masked"` confines it to the instance's pixels, and the default leaves it out.  The
numpy model the kernels are compared with bit for bit is here too (`handle_lighting_host`, `lighting_stats_host`, `rgb_to_hsv_u8_host`,
`hsv_to_rgb_u8_host`); numpy arrays given to the three public functions go through it, so the reference's own call
`handle_lighting(im_mat, mask_mat)` works without cv2.
PARITY: cv2 is installed neither where this was written nor where it was run, so the two conversions follow OpenCV's published scalar
code (imgproc color_hsv: RGB2HSV_b with H range 180, HSV2RGB_b over HSV2RGB_native) and are UNPINNED against the library -- in particular
whether a SIMD build of HSV2RGB fuses v * (1 - s * h).  Everything after the conversions (box, means, shift, clip, cast) is pinned: it
is the reference's own numpy.  One documented deviation: a mask that fills its whole expanded box leaves no background pixel; the
reference casts the NaN mean of an empty array to uint8 (undefined), here V stays unchanged.

Not here (they stay with the caller): mesh loading (trimesh, kaolin's .obj import) and `trimesh.bounds.oriented_bounds` (the `extents`
of bbox_result: a per-mesh constant) and the kaolin camera algebra of mesh_renderer.py:187-221 (INTEGRATION.md gives the correspondence)."""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from .ops import _dev, _p, _require, _stream

SEMANTIC_ID = {"vehicle": 13, "person": 11, "object": 0, "bicycle": 18, "motorcycle": 17}     # utils_render.py:934-936


def handle_occlusion_paste(bg_im, vehicle_im, mask_im, depth_mat, semantic_mat, fg_depth, category="vehicle"):
    """In place on bg_im [H,W,3] u8, mask_im [H,W,3] u8, depth_mat [H,W] f32, semantic_mat [H,W] u8; `fg_depth` [H,W] f32 = mesh depth
    per pixel (None for category "person").  Returns occlusion_per as a device scalar (no host sync)."""
    H, W = depth_mat.shape
    _dev("bg_im vehicle_im mask_im", bg_im, vehicle_im, mask_im, dtype=torch.uint8, shape=(H, W, 3))
    _dev("semantic_mat", semantic_mat, dtype=torch.uint8, shape=(H, W)); _dev("depth_mat", depth_mat)
    person = category == "person"
    if not person:
        _dev("fg_depth", fg_depth, shape=(H, W))
    cnt = torch.empty(2, dtype=torch.int32, device=bg_im.device)
    _lib.call("snerf_fg_paste", _p(bg_im), _p(vehicle_im), _p(mask_im), _p(depth_mat), _p(semantic_mat), _p(None if person else fg_depth), H * W,
              SEMANTIC_ID[category], int(person), _p(cnt), _stream())
    c = cnt.double()
    return 1 - c[1] / (c[0] + 1)


def _intrinsic(intrinsic):
    """(fx, fy, cx, cy) as python floats from a 3 x 3 (or larger) intrinsic matrix held on the HOST (numpy, nested lists, a CPU tensor)"""
    _require(not (torch.is_tensor(intrinsic) and intrinsic.is_cuda), "intrinsic: host values (a device matrix would cost a sync per call)")
    K = np.asarray(intrinsic, dtype=np.float64)
    return float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])


_FLIP = ((1., 0., 0., 0.), (0., -1., 0., 0.), (0., 0., -1., 0.), (0., 0., 0., 1.))      # utils_render.py:857-862
_FLIP_ON = {}                                                                            # device -> the flip as a [4,4] tensor there (uploaded once)


def mesh_depth(tracer, intrinsic, H, W, mask_im, transform=None):
    """utils_render.py:839-868,887-906: fg_depth [H,W] fp32 for handle_occlusion_paste -- the z-depth of `tracer`'s mesh along the ray
    of every pixel with mask_im[..., 0] > 0, from integer pixel coordinates (get_ray_d_from_xy ignores use_pixel_centers); 0.1 where
    the ray misses or the depth is >= 99 (`depth[depth >= 99.] = .1`), 0 outside the mask.  `transform` (3 x 4 or 4 x 4, host or device)
    is what places the tracer's mesh into `mesh_in_cam_coord`; the reference's diag(1, -1, -1) flip is composed in here.  No host sync."""
    from . import meshtrace
    _dev("mask_im", mask_im, dtype=torch.uint8, shape=(H, W, 3))
    fx, fy, cx, cy = _intrinsic(intrinsic)
    flip = _FLIP_ON.get(tracer.device)
    if flip is None:
        flip = _FLIP_ON[tracer.device] = torch.tensor(_FLIP, dtype=torch.float32, device=tracer.device)
    t = meshtrace._as_transform(transform, tracer.device)
    if t is not None:
        flip = flip[:3, :3] @ t                        # the flip has no translation: [3,3] @ [3,4]
    return tracer.trace_pinhole(fx, fy, cx, cy, H, W, False, mask=mask_im, transform=flip, t_max=99., miss_value=.1)[0]


def mask_from_mesh(tracer, resolution, intrinsic, transform=None):
    """stage0_code/utils_render.py:755-776 get_mask_from_mesh_use_inv: [H,W,3] uint8, 255 where the pixel-centre ray of resolution =
    (W, H) hits the mesh (`depth < 100`).  The mesh is used as given (camera coordinates, no flip), after `transform` if there is one."""
    W, H = resolution
    fx, fy, cx, cy = _intrinsic(intrinsic)
    return tracer.trace_pinhole(fx, fy, cx, cy, int(H), int(W), True, transform=transform, t_max=100., want_hit=True)[1]


def bound_radius(mask_im, category="vehicle"):
    """generate_images.py:127-134 (one small host sync: the band width is a kernel-shape parameter)."""
    if category in ("motorcycle", "bicycle"):
        cols = (mask_im > 0).any(dim=2).any(dim=0)
        return 3 if bool(cols.any()) else 1
    cols = torch.nonzero((mask_im > 0).any(dim=2).any(dim=0))
    if cols.numel() == 0:
        return 1
    return int((float(cols.max() - cols.min()) / 80) ** .82)


def get_bound_im(mask_im, r, return_mask_diff=False):
    """-> bound_im [H,W,3] u8 (and, with return_mask_diff, set_diff(mask_im, bound_im) from the same launch)."""
    H, W, _ = mask_im.shape
    _dev("mask_im", mask_im, dtype=torch.uint8, shape=(H, W, 3))
    bound = torch.empty_like(mask_im)
    diff = torch.empty_like(mask_im) if return_mask_diff else None
    _lib.call("snerf_fg_bound", _p(mask_im), H, W, max(1, int(r)), _p(bound), _p(diff), _stream())
    return (bound, diff) if return_mask_diff else bound


def accumulate(total_mask, total_bound, bound_im, mask_im):
    """In place: total_bound <- fuse_bound(total_mask, total_bound, bound_im, mask_im); total_mask <- mask_im | total_mask.
    Zero-initialised totals reproduce the reference's first-instance special case."""
    _dev("total_mask total_bound bound_im mask_im", total_mask, total_bound, bound_im, mask_im, dtype=torch.uint8, shape=tuple(total_mask.shape))
    _lib.call("snerf_fg_accumulate", _p(total_mask), _p(total_bound), _p(bound_im), _p(mask_im), total_mask.numel(), _stream())


def fuse_bound_and_im(fuse_im, bound_im):
    """In place: fuse_im[bound_im > 0] = 0."""
    _dev("fuse_im bound_im", fuse_im, bound_im, dtype=torch.uint8, shape=tuple(fuse_im.shape))
    _lib.call("snerf_fg_blank", _p(fuse_im), _p(bound_im), fuse_im.numel(), _stream())
    return fuse_im


# ---- the lighting match: utils_render.py:1008-1051 handle_lighting ------------------------------------------------------------------
_HSV_SHIFT = 12
_SDIV = np.concatenate([[0], np.rint((255 << _HSV_SHIFT) / (1.0 * np.arange(1, 256)))]).astype(np.int32)    # color_hsv: sdiv_table, hdiv_table180
_HDIV = np.concatenate([[0], np.rint((180 << _HSV_SHIFT) / (6.0 * np.arange(1, 256)))]).astype(np.int32)
LIGHTING_MAX_PIXELS = 1 << 23      # up to here "all fg V equal" in integers is numpy's `fg_var < 1e-7` for every input (snerf_hip.h)


def _px_host(px):
    px = np.asarray(px)
    _require(px.dtype == np.uint8 and px.ndim >= 1 and px.shape[-1] == 3, "expected a uint8 array [..., 3]")
    return px


def rgb_to_hsv_u8_host(px):
    """numpy model of snerf_fg_hsv(to_rgb=0): OpenCV's 8-bit COLOR_RGB2HSV (H range 180), integers with shift 12 -> new uint8 array"""
    px = _px_host(px).astype(np.int32)
    r, g, b = px[..., 0], px[..., 1], px[..., 2]
    v = np.maximum(np.maximum(r, g), b)
    diff = v - np.minimum(np.minimum(r, g), b)
    s = (diff * _SDIV[v] + (1 << (_HSV_SHIFT - 1))) >> _HSV_SHIFT
    h0 = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h0 * _HDIV[diff] + (1 << (_HSV_SHIFT - 1))) >> _HSV_SHIFT                              # arithmetic shift (int32)
    h = h + np.where(h < 0, 180, 0)
    return np.stack([h, s, v], axis=-1).astype(np.uint8)


def hsv_to_rgb_u8_host(px):
    """numpy model of snerf_fg_hsv(to_rgb=1): OpenCV's 8-bit COLOR_HSV2RGB, fp32 with every operation rounded on its own (numpy keeps
    float32 operands float32) -> new uint8 array.  H = 180 .. 255 follows the same formula."""
    px = _px_host(px)
    f32, one = np.float32, np.float32(1)
    hf = px[..., 0].astype(f32) * (f32(6) / f32(180))
    sf = px[..., 1].astype(f32) * (one / f32(255))
    vf = px[..., 2].astype(f32) * (one / f32(255))
    hf = np.fmod(hf, f32(6))
    sector = np.floor(hf)
    hf = hf - sector
    sector = sector.astype(np.int32)
    bad = (sector < 0) | (sector >= 6)
    sector = np.where(bad, 0, sector)
    hf = np.where(bad, f32(0), hf)
    tab = np.stack([vf, vf * (one - sf), vf * (one - sf * hf), vf * (one - sf * (one - hf))], axis=-1)
    idx = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])[sector]  # [..., (b, g, r)]
    bgr = np.take_along_axis(tab, idx, axis=-1)
    bgr = np.where((sf == 0)[..., None], vf[..., None], bgr)
    if bgr.dtype != np.float32:
        raise RuntimeError("hsv_to_rgb_u8_host: an operation left float32 (the model rounds every operation in fp32)")
    out = np.clip(np.rint(bgr * f32(255)), 0, 255).astype(np.uint8)
    return out[..., ::-1].copy()


def _lighting_stats(v, fg, H, W):
    """v [H,W] uint8 = the V channel, fg [H,W] bool -> the nine python ints of snerf_fg_lighting's stats"""
    ii, jj = np.nonzero(fg)
    if ii.size == 0:
        return [H, -1, W, -1, 0, 0, 0, 0, 0]
    i_min, i_max, j_min, j_max = int(ii.min()), int(ii.max()), int(jj.min()), int(jj.max())
    i_len, j_len = i_max - i_min, j_max - j_min
    i0, i1 = max(0, i_min - i_len // 2 - 1), min(H - 1, i_max + i_len // 2 + 1)
    j0, j1 = max(0, j_min - j_len // 2 - 1), min(W - 1, j_max + j_len // 2 + 1)
    box, bg = v[i0:i1 + 1, j0:j1 + 1].astype(np.int64), ~fg[i0:i1 + 1, j0:j1 + 1]
    vf = v[fg].astype(np.int64)
    return [i_min, i_max, j_min, j_max, int(vf.size), int(vf.sum()), int((vf * vf).sum()), int(bg.sum()), int(box[bg].sum())]


def lighting_stats_host(im, mask):
    """The nine integers snerf_fg_lighting leaves in `stats`: (i_min, i_max, j_min, j_max) of the raw mask (sentinels (H, -1, W, -1) when
    it is empty), n_fg, sum_v_fg, sum_v2_fg, n_bg, sum_v_bg (the last two over the expanded box; 0 for an empty mask) -> int64 [9]"""
    im, mask = _px_host(im), _px_host(mask)
    H, W, _ = im.shape
    return np.array(_lighting_stats(im.max(axis=-1), mask[..., 0] > 0, H, W), dtype=np.int64)


def handle_lighting_host(im, mask, keep_background=False):
    """numpy model of snerf_fg_lighting = utils_render.py:1008-1051 with the conversions above in cv2's place -> new uint8 [H,W,3]"""
    im, mask = _px_host(im), _px_host(mask)
    H, W, _ = im.shape
    _require(mask.shape == im.shape and H * W <= LIGHTING_MAX_PIXELS, "mask and frame [H,W,3], at most 2^23 pixels")
    hsv = rgb_to_hsv_u8_host(im)
    fg = mask[..., 0] > 0
    n_fg, s1, s2, n_bg, s_bg = _lighting_stats(hsv[..., 2], fg, H, W)[4:]
    if n_fg > 0 and n_bg > 0 and n_fg * s2 != s1 * s1:               # `if not fg_var < 1e-7`, in integers; n_bg == 0: the deviation
        fg_mean, bg_mean = np.float64(s1) / np.float64(n_fg), np.float64(s_bg) / np.float64(n_bg)
        v = hsv[..., 2][fg] - fg_mean + bg_mean
        hsv[..., 2][fg] = np.clip(v, 0, 255).astype(np.uint8)
    out = hsv_to_rgb_u8_host(hsv)
    if keep_background:
        out[~fg] = im[~fg]
    return out


def _hsv_u8(px, to_rgb):
    if isinstance(px, np.ndarray):
        return hsv_to_rgb_u8_host(px) if to_rgb else rgb_to_hsv_u8_host(px)
    _dev("px", px, dtype=torch.uint8)
    _require(px.dim() >= 1 and px.shape[-1] == 3 and px.numel() > 0, "expected a non-empty uint8 tensor [..., 3]")
    _lib.call("snerf_fg_hsv", _p(px), px.numel() // 3, int(to_rgb), _stream())
    return px


def rgb_to_hsv_u8(px):
    """cv2.cvtColor(px, cv2.COLOR_RGB2HSV) of 8-bit pixels [..., 3] (H in 0 .. 179).  A device tensor is converted in place (snerf_fg_hsv,
    any byte offset of a contiguous view) and returned; a numpy array goes through the host model and a new array is returned."""
    return _hsv_u8(px, False)


def hsv_to_rgb_u8(px):
    """cv2.cvtColor(px, cv2.COLOR_HSV2RGB) of 8-bit pixels [..., 3]; device tensor in place, numpy array -> new array (see rgb_to_hsv_u8)"""
    return _hsv_u8(px, True)


def handle_lighting(im, mask, keep_background=False, stats=None):
    """utils_render.py:1008-1051 handle_lighting(im_mat, mask_mat).  Device tensors im [H,W,3] u8 and mask [H,W,3] u8 (channel 0 > 0 is
    the instance): in place on im, which is returned; one init launch and three kernels, no host read (snerf_fg_lighting).  `stats`: an
    optional preallocated int64 [9] device tensor (needed under graph capture), left holding (i_min, i_max, j_min, j_max, n_fg, sum_v_fg,
    sum_v2_fg, n_bg, sum_v_bg) as lighting_stats_host gives them.  keep_background=True (an extension) leaves the pixels outside the
    mask untouched; the reference rewrites the whole frame through the lossy 8-bit HSV round trip.  H * W <= 2^23.
    numpy arrays: the reference's own call, through handle_lighting_host -> a new array."""
    if isinstance(im, np.ndarray):
        return handle_lighting_host(im, np.asarray(mask), keep_background)
    H, W, _ = im.shape
    _dev("im mask", im, mask, dtype=torch.uint8, shape=(H, W, 3))
    if stats is None:
        stats = torch.empty(9, dtype=torch.int64, device=im.device)
    _dev("stats", stats, dtype=torch.int64, msg="stats: an int64 [9] device tensor")
    _require(stats.numel() == 9, "stats: an int64 [9] device tensor")
    _lib.call("snerf_fg_lighting", _p(im), _p(mask), H, W, int(bool(keep_background)), _p(stats), _stream())
    return im


def overlap_stats(masks):
    """snerf_fg_overlap: masks = N (2 .. 32) contiguous [H,W,3] uint8 device tensors of one shape -> int64 [N,N,3] on the device; for a < b
    (count, sum of row, sum of col) over np.where((mask_a > 0) & (mask_b > 0)) -- (row, col, channel) triples, not pixels --, zero for
    a >= b.  One launch that reads every mask once; the masks are not stacked or copied.  No host read."""
    masks = list(masks)
    N = len(masks)
    _require(N >= 1, "overlap_stats: at least one mask")
    H, W, _ = masks[0].shape
    _dev("masks", *masks, dtype=torch.uint8, shape=(H, W, 3))
    _require(all(m.device == masks[0].device for m in masks), "overlap_stats: all masks on one device")
    stats = torch.zeros(N, N, 3, dtype=torch.int64, device=masks[0].device)
    ptrs = (ctypes.c_void_p * N)(*[m.data_ptr() for m in masks])
    _lib.call("snerf_fg_overlap", ptrs, N, H, W, _p(stats), _stream())
    return stats


T_MAX_ANY = float(np.finfo(np.float32).max)      # the largest t_max the tracer accepts: trimesh's intersects_first has no range limit


def topological_order(before):
    """utils_render.py:795-806 literally: before [N,N] (host), before[i, j] != 0 = "i is pasted before j".  Repeatedly the smallest index
    not yet emitted whose column is all zero is emitted and its row cleared; RuntimeError on a cycle.  -> list of N indices."""
    A = np.array(before, dtype=np.uint8)
    n = A.shape[0]
    result = []
    while len(result) < n:
        for i in range(n):
            if i not in result and np.sum(A[:, i]) == 0:
                result.append(i)
                A[i, :] = 0
                break
        else:
            raise RuntimeError("Occlusion judgment fails....")
    return result


def occlusion_order(masks, meshes, w2c, P, ray_frame="reference"):
    """utils_render.py:691-808 occlution_order for one frame -> (order: list of N indices, the instances in the order they are to be
    pasted, farthest first; before: host int8 [N,N], before[i, j] = 1 when i must be pasted before j).

    masks: N [H,W,3] uint8 device masks; meshes: N pairs (meshtrace.RayTracer, transform or None), `transform` placing the tracer's mesh
    into camera coordinates as composite_frame's `mesh=` takes it (without the diag(1, -1, -1) flip mesh_depth adds); w2c (4 x 4) and P
    (3 x 3 intrinsic): HOST values.

    Per pair a < b whose masks share a byte (snerf_fg_overlap; :745-751) the pixel (mean col, mean row, 1) of the shared (row, col,
    channel) triples is sent through inv(P) (:753-754); both meshes are traced along that ONE ray (one trace_ids call per mesh, over
    the rays of all its pairs, no range limit) and z = the z of the centre of the first-hit face under `transform` (:732-736)
    decides: z_a < z_b is "a occludes b", b is pasted first; anything else (equal or NaN z included) pastes a first.  Pairs without overlap
    get no edge.  The sort is the reference's loop (topological_order), on the host, after the one host read of this function.

    On a miss trimesh returns -1 and the reference indexes `tri[-1]`: the centre of the LAST face of the mesh as the caller numbered
    it decides.  The same happens here, in both ray frames.

    ray_frame: the reference builds the ray in WORLD coordinates (origin c2w[:3, 3], direction towards c2w (inv(P) pixel, 1), normalised;
    :752-760) and casts it against meshes it has already moved into CAMERA coordinates (:777).  ray_frame="reference" (the default)
    reproduces that as written: unless w2c is near the identity most rays miss and the last-face z decides.  ray_frame="camera" casts
    what was evidently meant, origin 0 and direction inv(P) pixel in the meshes' own frame.

    Parity: trimesh is not part of the reference tree, so how `intersects_first` treats a ray through an edge or a degenerate face is
    not pinned; the semantics are those of meshtrace (watertight, nearest t > 0).  The ray is formed in float64 on the device and
    cast in fp32."""
    _require(ray_frame in ("reference", "camera"), "ray_frame: 'reference' or 'camera'")
    masks, meshes = list(masks), list(meshes)
    N = len(masks)
    _require(len(meshes) == N, "occlusion_order: one (tracer, transform) per mask")
    if N < 2:
        return list(range(N)), np.zeros((N, N), dtype=np.int8)
    dev = masks[0].device
    _require(not any(torch.is_tensor(m) and m.is_cuda for m in (w2c, P)), "w2c, P: host values (a device matrix would cost a sync per call)")
    c2w = np.linalg.inv(np.asarray(w2c, dtype=np.float64)[:4, :4])
    host = np.concatenate([np.linalg.inv(np.asarray(P, dtype=np.float64)[:3, :3]).reshape(-1), c2w[:3].reshape(-1)])
    host = torch.tensor(host, dtype=torch.float64).to(dev)                      # one upload: inv(P) and the top of c2w
    Pinv, c2w_d = host[:9].view(3, 3), host[9:].view(3, 4)
    stats = overlap_stats(masks).double()
    count = stats[..., 0]
    overlap = count > 0                                                        # [N,N], a < b only
    pixel = torch.stack([stats[..., 2] / count, stats[..., 1] / count, torch.ones_like(count)], dim=-1)    # (j.mean(), i.mean(), 1)
    point = pixel @ Pinv.T                                                     # [N,N,3]
    if ray_frame == "reference":
        origin = c2w_d[:, 3].expand(N, N, 3)
        d = (point @ c2w_d[:, :3].T + c2w_d[:, 3]) - origin
        d = d / torch.linalg.norm(d, dim=-1, keepdim=True)
    else:
        origin, d = torch.zeros(N, N, 3, dtype=torch.float64, device=dev), point
    d = torch.where(overlap[..., None], d, torch.zeros_like(d))                # no overlap: a zero direction, which hits nothing
    o32, d32 = origin.float(), d.float()                                       # (one origin for every pair)
    d32 = d32 + d32.transpose(0, 1)                                            # the pair's ray at [a,b] and at [b,a]: the other half is zero
    z = torch.zeros(N, N, dtype=torch.float64, device=dev)                     # z[k, j]: mesh k along the ray of the pair {k, j}
    others = torch.tensor([[j for j in range(N) if j != k] for k in range(N)]).to(dev)                     # [N,N-1], one upload
    for k, (tracer, transform) in enumerate(meshes):
        face = tracer.trace_ids(o32[k, others[k]], d32[k, others[k]], transform, T_MAX_ANY)[3]
        z[k, others[k]] = tracer.face_centers(face, transform)[:, 2]
    a_occludes_b = z < z.transpose(0, 1)                                       # at [a,b], a < b: z_a < z_b
    upper = overlap.triu(1)
    before = ((upper & ~a_occludes_b) | (upper & a_occludes_b).transpose(0, 1)).to(torch.int8).cpu().numpy()     # the one host read
    return topological_order(before), before


def occlusion_level(occlusion_per):
    """utils_render.py:561-568: the KITTI occlusion level 0 / 1 / 2 / 3 of an occluded share, thresholds .01, .5, .99"""
    if occlusion_per < .01:
        return 0
    if occlusion_per < .5:
        return 1
    if occlusion_per < .99:
        return 2
    return 3


CATEGORY_NAME = {"vehicle": "Car", "person": "Pedestrain", "object": "Object", "bicycle": "Bicycle", "motorcycle": "Motorcycle"}   # utils_render.py:579-581 (its spelling)
_EXTENT_FIELDS = {"vehicle": ("height", "width", "length"), "bicycle": ("width", "height", "length"), "person": ("length", "width", "height"),
                  "motorcycle": ("width", "height", "length")}                 # :605-612; "object" gets none


def rot_y(w2c, theta):
    """utils_render.py:590-600,623: Rotation.from_matrix(M).as_euler('yzx')[0] - pi / 2 for M = rot_w2c @ Rz(theta degrees) @ rot_axis.T, in
    closed form: the first angle of scipy's extrinsic 'yzx' is atan2(M[0,2], M[0,0]) (away from the gimbal lock |M[0,1]| = 1)."""
    t = math.radians(float(theta))
    rz = np.array([[math.cos(t), -math.sin(t), 0.], [math.sin(t), math.cos(t), 0.], [0., 0., 1.]])
    rot_axis = np.array([[1., 0., 0.], [0., 0., -1.], [0., 1., 0.]])
    M = np.asarray(w2c, dtype=np.float64)[:3, :3] @ rz @ rot_axis.T
    return math.atan2(M[0, 2], M[0, 0]) - math.pi / 2


def bbox_result(w2c, bbox_center, theta, occlusion_per, category, extents):
    """utils_render.py:583-626 get_bbox_result: the KITTI-style label of one instance in one frame, everything in camera coordinates.
    w2c: 4 x 4 host matrix; bbox_center: the instance's position in the world; theta: its heading in degrees; occlusion_per: a host
    float (composite_frame's `occlusion`); extents: the three `trimesh.bounds.oriented_bounds(mesh)[1]` values, a per-mesh constant the
    caller computes when it loads the mesh, assigned to height / width / length per category as the reference does ("object": none)."""
    w2c = np.asarray(w2c, dtype=np.float64)
    centre = np.concatenate([np.asarray(bbox_center, dtype=np.float64).reshape(3), [1.]])
    pos = (w2c @ centre)[:3]
    res = {"category": CATEGORY_NAME[category], "occlution": occlusion_level(occlusion_per)}
    for field, value in zip(_EXTENT_FIELDS.get(category, ()), extents if extents is not None else ()):
        res[field] = float(value)
    res["pos_x"], res["pos_y"], res["pos_z"] = (float(v) for v in pos)
    for field in ("alpha", "xmin", "ymin", "xmax", "ymax", "truncated"):
        res[field] = .0
    res["rot_y"] = rot_y(w2c, theta)
    res["confidence"] = 1
    return res


def save_bbox_results(path, results):
    """utils_render.py:629-640 save_bbox_result_for_one_frame: one line per label, the reference's format string"""
    with open(path, "w") as f:
        for res in results:
            f.write("%s %f %d %f %f %f %f %f %f %f %f %f %f %f %f %f" %
                    (res["category"], res["truncated"], res["occlution"], res["alpha"], res["xmin"], res["ymin"], res["xmax"], res["ymax"],
                     res["height"], res["width"], res["length"], res["pos_x"], res["pos_y"], res["pos_z"], res["rot_y"], res["confidence"]))
            f.write("\n")


def _image_and_mask(inst, depth_mat):
    """the instance's image and mask: given, or rendered here at the frame's size from render = (MeshRenderer, transform)"""
    if inst.get("render") is None:
        return inst["image"], inst["mask"]
    renderer, transform = inst["render"]
    fx, fy, cx, cy = _intrinsic(inst["intrinsic"])
    return renderer.render(fx, fy, cx, cy, depth_mat.shape[0], depth_mat.shape[1], transform=transform)[:2]


def _ordered_by_occlusion(instances, depth_mat, w2c, intrinsic):
    """composite_frame(order="occlusion"): render what is to be rendered, then -> (the instances in paste order, the order)"""
    instances = [dict(inst) for inst in instances]
    for i, inst in enumerate(instances):
        if inst.get("mesh") is None:
            raise ValueError(f"composite_frame(order='occlusion'): instance {i} ({inst.get('category', 'vehicle')}) has no mesh=(tracer, transform); "
                             "the occlusion order casts a ray against the mesh of every instance, persons included")
    if w2c is None or intrinsic is None:
        raise ValueError("composite_frame(order='occlusion') needs w2c (4 x 4) and intrinsic (3 x 3), the frame's camera")
    for inst in instances:
        if inst.get("intrinsic") is None:
            inst["intrinsic"] = intrinsic
        inst["image"], inst["mask"] = _image_and_mask(inst, depth_mat)
        inst.pop("render", None)                       # rendered: the paste loop takes the image and the mask as given
    order, _ = occlusion_order([inst["mask"] for inst in instances], [inst["mesh"] for inst in instances], w2c, intrinsic)
    return [instances[i] for i in order], order


def composite_frame(bg_im, depth_mat, semantic_mat, instances, order="given", w2c=None, intrinsic=None, lighting=None):
    """The instance loop of generate_images.py:80-166 for one frame.  `instances`: iterable of dict(image [H,W,3] u8, mask [H,W,3] u8,
    fg_depth [H,W] f32 or None, category, r (optional band width)); instead of
    fg_depth an instance may carry mesh = (meshtrace.RayTracer, transform or None) and intrinsic (3 x 3, host): its depth is then
    mesh_depth(tracer, intrinsic, H, W, mask, transform), traced here.  Instead of image and mask an instance may carry render =
    (meshrender.MeshRenderer, transform or None) and intrinsic: both are then rendered here, at the frame's size, with the reference's
    frame-validity rule.
    order="given" (the default): the instances are pasted as they come, already in the reference's occlusion order.  order="occlusion":
    EVERY instance carries mesh = (tracer, transform), persons too (the reference loads a mesh for each), and the frame's `w2c` (4 x 4,
    host) and `intrinsic` (3 x 3, host; also that of an instance without its own) are given; the instances with render = are rendered
    first, all of them, `occlusion_order(masks, meshes, w2c, intrinsic)` sorts them (generate_images.py:76-81) and the loop runs in that
    order.  The result then has `order`, indices into `instances` as given; a missing mesh is a ValueError that names the instance.
    lighting=None (the default): no lighting match.  lighting="frame": `handle_lighting(bg_im, tested)` directly after each paste, for every
    category, with the depth-tested mask, as fuse() does (utils_render.py:300): the whole frame goes through the 8-bit HSV round trip once
    per instance.  lighting="masked": the same with keep_background=True.  Anything else is a ValueError.
    In place on bg_im / depth_mat / semantic_mat; returns dict(fuse, mask, bound, occluded_mask, depth, semantic, occlusion [per
    instance], instance_masks, instance_bounds) = the images the reference saves per frame (:153-154,186-196); the per-instance lists are
    in the order of processing."""
    if order not in ("given", "occlusion"):
        raise ValueError(f"composite_frame: order must be 'given' or 'occlusion', not {order!r}")
    if lighting not in (None, "frame", "masked"):
        raise ValueError(f"composite_frame: lighting must be None, 'frame' or 'masked', not {lighting!r}")
    paste_order = None
    if order == "occlusion":
        instances, paste_order = _ordered_by_occlusion(instances, depth_mat, w2c, intrinsic)
    total_mask, total_bound, total_occluded = torch.zeros_like(bg_im), torch.zeros_like(bg_im), torch.zeros_like(bg_im)
    occ, masks, bounds = [], [], []
    for inst in instances:
        cat = inst.get("category", "vehicle")
        image, mask = _image_and_mask(inst, depth_mat)
        r = inst.get("r")
        if r is None:
            r = bound_radius(mask, cat)
        # the depth test works on a copy of the mask (utils_render.py:280: np.array(mask_im)); the band and the frame's mask come from
        # the instance's full mask, the depth-tested one only feeds the `occluded_mask` image of vehicles (generate_images.py:162-166)
        tested = mask.clone()
        fg_depth = inst.get("fg_depth")
        if fg_depth is None and inst.get("mesh") is not None and cat != "person":
            tracer, transform = inst["mesh"]
            fg_depth = mesh_depth(tracer, inst["intrinsic"], depth_mat.shape[0], depth_mat.shape[1], mask, transform)
        occ.append(handle_occlusion_paste(bg_im, image, tested, depth_mat, semantic_mat, fg_depth, cat))
        if lighting is not None:
            handle_lighting(bg_im, tested, keep_background=lighting == "masked")
        bound, mask_d = get_bound_im(mask, r, return_mask_diff=True)
        accumulate(total_mask, total_bound, bound, mask_d)
        if cat == "vehicle":
            total_occluded = torch.where((tested > 0) | (total_occluded > 0), 255, 0).to(torch.uint8)
        masks.append(mask_d); bounds.append(bound)
    fuse_bound_and_im(bg_im, total_bound)
    out = dict(fuse=bg_im, mask=total_mask, bound=total_bound, occluded_mask=total_occluded, depth=depth_mat, semantic=semantic_mat, occlusion=occ,
               instance_masks=masks, instance_bounds=bounds)
    if paste_order is not None:
        out["order"] = paste_order
    return out
