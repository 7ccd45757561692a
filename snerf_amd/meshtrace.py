"""First-hit ray tracer for triangle meshes on the device: the `raytracing.RayTracer` of the S-NeRF++ foreground stages.

Reference counterpart: `raytracing.RayTracer(vertices, faces).trace(ray_o, ray_d)` -> `(intersections, face_normals, depth)` as called by
s-nerfpp/stage1_code/utils_render.py:839-868,887-906 (the mesh depth along the masked pixels' rays) and
s-nerfpp/stage0_code/utils_render.py:755-776 (the per-instance hit mask).  **That library is a CUDA-only extension that is not part of the
reference tree, so nothing here could be compared against it**: what it returns for a ray through an edge, how it orients
`face_normals`, what `intersections` holds on a miss and whether it reports hits beyond its max depth of 100 are not pinned.  Defined
here (csrc/meshtrace.hip, include/snerf_hip.h): a hit needs `0 < t < t_max` (t in units of the un-normalised direction), the nearest
hit wins, a miss returns `t_max` as depth and zero `intersections` / `face_normals`; normals are the unit `(b - a) x (c - a)` of the
face, not turned towards the ray.  The triangle test is watertight: a ray through a shared edge or a vertex of a closed surface hits it.
What the callers build on -- depth 100 for no intersection, the z-depth for rays with d_z = -1 -- is reproduced; the tests compare
against an all-pairs float64 Moeller-Trumbore.

The mesh is ordered once, at construction (Morton code of the face centroids, `torch.sort`); every trace call rebuilds the
transformed triangles and the boxes in one small launch pair (F triangles of work), so one RayTracer serves every pose of its mesh."""
import numpy as np
import torch

from . import ops

MAX_DEPTH = 100.         # the library's "no intersection" depth (utils_render.py:867, stage 0 :774)


def _part1by2(x):
    """spread the low 10 bits of x to every third bit"""
    x = x & 0x3ff
    x = (x | (x << 16)) & 0x30000ff
    x = (x | (x << 8)) & 0x300f00f
    x = (x | (x << 4)) & 0x30c30c3
    x = (x | (x << 2)) & 0x9249249
    return x


def morton_order(vertices, faces):
    """-> int64 [F]: the faces sorted by the 30-bit Morton code of their centroids inside the mesh's bounding box (stable; faces with a
    non-finite centroid go first).  vertices [V,3] fp32, faces [F,3] int64 with every index inside [0, V)."""
    F = faces.shape[0]
    if F == 0:
        return torch.zeros(0, dtype=torch.int64, device=faces.device)
    cen = torch.nan_to_num(vertices[faces].mean(dim=1), nan=0., posinf=0., neginf=0.)
    lo, hi = cen.min(dim=0).values, cen.max(dim=0).values
    q = ((cen - lo) / (hi - lo).clamp_min(1e-30) * 1023.).clamp(0., 1023.).long()
    code = _part1by2(q[:, 0]) | (_part1by2(q[:, 1]) << 1) | (_part1by2(q[:, 2]) << 2)
    return torch.sort(code, stable=True).indices


def _as_transform(transform, device):
    """None, or anything array-like of shape [3,4] / [4,4] -> a contiguous fp32 [3,4] tensor on `device` (no host read)"""
    if transform is None:
        return None
    t = transform if torch.is_tensor(transform) else torch.tensor(np.asarray(transform, dtype=np.float32))
    t = t.to(device=device, dtype=torch.float32)
    ops._require(tuple(t.shape) in ((3, 4), (4, 4)), "transform: a 3 x 4 (or 4 x 4 affine) matrix")
    return t[:3].contiguous()


class RayTracer:
    """`RayTracer(vertices, faces)`: vertices [V,3] floats, faces [F,3] integers, numpy arrays or tensors.  Raises ValueError for a face
    index outside [0, V) -- the one host read of this class.  `device`: where the mesh lives (default: the current CUDA device)."""

    def __init__(self, vertices, faces, device=None):
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        v = vertices if torch.is_tensor(vertices) else torch.tensor(np.asarray(vertices, dtype=np.float32))
        f = faces if torch.is_tensor(faces) else torch.tensor(np.asarray(faces).astype(np.int64))
        v = v.to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
        f = f.to(device=dev, dtype=torch.int64).reshape(-1, 3)
        if f.numel() and bool(((f < 0) | (f >= v.shape[0])).any()):
            raise ValueError(f"RayTracer: a face index lies outside [0, {v.shape[0]})")
        order = morton_order(v, f)
        self.device = dev
        self.vertices = v
        self.faces = f[order].to(torch.int32).contiguous()           # in the order the kernel walks them
        self.face_ids = order.to(torch.int32).contiguous()           # ordered position -> the caller's face index
        self.n_faces = int(f.shape[0])
        self.ws = torch.empty(ops.mesh_ws_bytes(self.n_faces), dtype=torch.uint8, device=dev)

    def prepare(self, transform=None):
        """rebuild the workspace for `transform` (3 x 4 or 4 x 4, applied to the vertices as given; None: the mesh as it is)"""
        ops.mesh_prepare(self.vertices, self.faces, self.face_ids, _as_transform(transform, self.device), self.ws)
        return self.ws

    def trace(self, rays_o, rays_d, transform=None, t_max=MAX_DEPTH):
        """-> (intersections [R,3], face_normals [R,3], depth [R]) as fp32 device tensors, the reference's call."""
        return self.trace_ids(rays_o, rays_d, transform, t_max)[:3]

    def trace_ids(self, rays_o, rays_d, transform=None, t_max=MAX_DEPTH, flags=0):
        """-> (intersections, face_normals, depth, face_id [R] int32: the hit face in the constructor's numbering, -1 on a miss)"""
        o = _as_rays(rays_o, self.device)
        d = _as_rays(rays_d, self.device)
        self.prepare(transform)
        depth, face_id, pos, nrm = ops.mesh_trace(self.ws, self.n_faces, o, d, t_max, flags=flags)
        return pos, nrm, depth, face_id

    def trace_pinhole(self, fx, fy, cx, cy, H, W, pixel_center, mask=None, transform=None, t_max=MAX_DEPTH, miss_value=MAX_DEPTH, want_hit=False,
                      flags=0):
        """the camera's own rays (ops.mesh_trace_pinhole) -> (depth [H,W], hit [H,W,3] uint8 or None)"""
        self.prepare(transform)
        return ops.mesh_trace_pinhole(self.ws, self.n_faces, fx, fy, cx, cy, pixel_center, H, W, mask, t_max, miss_value, want_hit, flags,
                                      device=self.device)

    def face_centers(self, face_id, transform=None):
        """-> float64 [..., 3]: trimesh's `triangles_center[face_id]` of the mesh under `transform`, the mean of the three transformed
        vertices, for face ids in the CONSTRUCTOR's numbering (what trace_ids returns).  A negative id counts from the end as a numpy
        index does, so the -1 of a miss names the last face (the reference's `tri[tri_index]` at stage1_code/utils_render.py:733-735).
        No host read; a mesh without faces gives NaN."""
        fid = face_id.to(device=self.device, dtype=torch.int64)
        if self.n_faces == 0:
            return torch.full(tuple(fid.shape) + (3,), float("nan"), dtype=torch.float64, device=self.device)
        if getattr(self, "_position_of", None) is None:          # the caller's face index -> its position in the ordered arrays
            self._position_of = torch.empty(self.n_faces, dtype=torch.int64, device=self.device)
            self._position_of[self.face_ids.long()] = torch.arange(self.n_faces, device=self.device)
        fid = torch.where(fid < 0, fid + self.n_faces, fid)
        tri = self.vertices.double()[self.faces[self._position_of[fid]].long()]             # [..., 3 corners, 3]
        t = _as_transform(transform, self.device)
        if t is not None:
            t = t.double()
            tri = tri @ t[:, :3].T + t[:, 3]
        return tri.mean(dim=-2)


def _as_rays(r, device):
    t = r if torch.is_tensor(r) else torch.tensor(np.asarray(r, dtype=np.float32))
    return t.to(device=device, dtype=torch.float32).reshape(-1, 3).contiguous()
