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

Not here (they stay with the caller): mesh loading (trimesh, kaolin's .obj import), the kaolin camera algebra of
mesh_renderer.py:187-221 (INTEGRATION.md gives the correspondence), the bounding-box export, and `handle_lighting` (cv2's 8-bit HSV
round trip)."""
import numpy as np
import torch

from . import _lib
from .ops import _p, _stream

SEMANTIC_ID = {"vehicle": 13, "person": 11, "object": 0, "bicycle": 18, "motorcycle": 17}     # utils_render.py:934-936


def _u8(t, shape=None):
    assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and (shape is None or tuple(t.shape) == tuple(shape)), \
        "expected a contiguous uint8 CUDA tensor" + ("" if shape is None else f" of shape {tuple(shape)}")
    return t


def handle_occlusion_paste(bg_im, vehicle_im, mask_im, depth_mat, semantic_mat, fg_depth, category="vehicle"):
    """In place on bg_im [H,W,3] u8, mask_im [H,W,3] u8, depth_mat [H,W] f32, semantic_mat [H,W] u8; `fg_depth` [H,W] f32 = mesh depth
    per pixel (None for category "person").  Returns occlusion_per as a device scalar (no host sync)."""
    H, W = depth_mat.shape
    _u8(bg_im, (H, W, 3)); _u8(vehicle_im, (H, W, 3)); _u8(mask_im, (H, W, 3)); _u8(semantic_mat, (H, W))
    assert depth_mat.dtype == torch.float32 and depth_mat.is_contiguous() and depth_mat.is_cuda
    person = category == "person"
    if not person:
        assert fg_depth is not None and fg_depth.dtype == torch.float32 and fg_depth.is_contiguous() and tuple(fg_depth.shape) == (H, W)
    cnt = torch.empty(2, dtype=torch.int32, device=bg_im.device)
    _lib.call("snerf_fg_paste", _p(bg_im), _p(vehicle_im), _p(mask_im), _p(depth_mat), _p(semantic_mat), _p(None if person else fg_depth), H * W,
              SEMANTIC_ID[category], int(person), _p(cnt), _stream())
    c = cnt.double()
    return 1 - c[1] / (c[0] + 1)


def _intrinsic(intrinsic):
    """(fx, fy, cx, cy) as python floats from a 3 x 3 (or larger) intrinsic matrix held on the HOST (numpy, nested lists, a CPU tensor)"""
    assert not (torch.is_tensor(intrinsic) and intrinsic.is_cuda), "intrinsic: host values (a device matrix would cost a sync per call)"
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
    _u8(mask_im, (H, W, 3))
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
    _u8(mask_im, (H, W, 3))
    bound = torch.empty_like(mask_im)
    diff = torch.empty_like(mask_im) if return_mask_diff else None
    _lib.call("snerf_fg_bound", _p(mask_im), H, W, max(1, int(r)), _p(bound), _p(diff), _stream())
    return (bound, diff) if return_mask_diff else bound


def accumulate(total_mask, total_bound, bound_im, mask_im):
    """In place: total_bound <- fuse_bound(total_mask, total_bound, bound_im, mask_im); total_mask <- mask_im | total_mask.
    Zero-initialised totals reproduce the reference's first-instance special case."""
    for t in (total_mask, total_bound, bound_im, mask_im):
        _u8(t, total_mask.shape)
    _lib.call("snerf_fg_accumulate", _p(total_mask), _p(total_bound), _p(bound_im), _p(mask_im), total_mask.numel(), _stream())


def fuse_bound_and_im(fuse_im, bound_im):
    """In place: fuse_im[bound_im > 0] = 0."""
    _u8(fuse_im); _u8(bound_im, fuse_im.shape)
    _lib.call("snerf_fg_blank", _p(fuse_im), _p(bound_im), fuse_im.numel(), _stream())
    return fuse_im


def composite_frame(bg_im, depth_mat, semantic_mat, instances):
    """The instance loop of generate_images.py:80-166 for one frame.  `instances`: iterable (already in the reference's occlusion
    order) of dict(image [H,W,3] u8, mask [H,W,3] u8, fg_depth [H,W] f32 or None, category, r (optional band width)); instead of
    fg_depth an instance may carry mesh = (meshtrace.RayTracer, transform or None) and intrinsic (3 x 3, host): its depth is then
    mesh_depth(tracer, intrinsic, H, W, mask, transform), traced here.  Instead of image and mask an instance may carry render =
    (meshrender.MeshRenderer, transform or None) and intrinsic: both are then rendered here, at the frame's size, with the reference's
    frame-validity rule.
    In place on bg_im / depth_mat / semantic_mat; returns dict(fuse, mask, bound, occluded_mask, depth, semantic, occlusion [per
    instance], instance_masks, instance_bounds) = the images the reference saves per frame (:153-154,186-196)."""
    total_mask, total_bound, total_occluded = torch.zeros_like(bg_im), torch.zeros_like(bg_im), torch.zeros_like(bg_im)
    occ, masks, bounds = [], [], []
    for inst in instances:
        cat = inst.get("category", "vehicle")
        if inst.get("render") is not None:
            renderer, transform = inst["render"]
            fx, fy, cx, cy = _intrinsic(inst["intrinsic"])
            image, mask = renderer.render(fx, fy, cx, cy, depth_mat.shape[0], depth_mat.shape[1], transform=transform)[:2]
        else:
            image, mask = inst["image"], inst["mask"]
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
        bound, mask_d = get_bound_im(mask, r, return_mask_diff=True)
        accumulate(total_mask, total_bound, bound, mask_d)
        if cat == "vehicle":
            total_occluded = torch.where((tested > 0) | (total_occluded > 0), 255, 0).to(torch.uint8)
        masks.append(mask_d); bounds.append(bound)
    fuse_bound_and_im(bg_im, total_bound)
    return dict(fuse=bg_im, mask=total_mask, bound=total_bound, occluded_mask=total_occluded, depth=depth_mat, semantic=semantic_mat, occlusion=occ,
                instance_masks=masks, instance_bounds=bounds)
