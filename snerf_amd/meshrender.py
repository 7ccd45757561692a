"""Mesh renderer on the device: the instance image and mask that `foreground.composite_frame` pastes.

Reference counterpart: s-nerfpp/api_code/mesh_renderer.py:36-88 `render(cam)` -- nvdiffrast rasterises the kaolin-transformed vertices,
`interpolate` gives vertex colours (.ply) or uvs (.obj), every material is sampled with `grid_sample`, the frame is rejected by
`valid_mask` (:44-53), and image and mask go through PNG files (`save_image`: floor(255 x + 0.5)) to stage 1.  **nvdiffrast and kaolin
are CUDA-only libraries outside the reference tree, so nothing here could be compared against them**: which triangle owns a pixel centre
on an edge, their near plane and how the kaolin camera of :187-221 maps to (fx, fy, cx, cy, transform) are not pinned (INTEGRATION.md
gives the correspondence as read).  Defined here (csrc/meshtrace.hip, snerf_mesh_render_pinhole): a pixel is covered when its centre's
ray d = (((x + .5) - cx) / fx, -(((y + .5) - cy) / fy), -1) hits the mesh with 0 < t < t_max, by the watertight first-hit walk of
`meshtrace.RayTracer.trace_pinhole` (the same bits); attributes are interpolated with the barycentrics of that hit in 3-D
(perspective-correct); the texture fetch is `grid_sample`'s arithmetic (bilinear, align_corners=False, border padding) and is tested
against `torch.nn.functional.grid_sample`; row 0 is the top row, so the reference's vertical flip has no counterpart; the validity rule
runs on the device, its area test as the integer 2 count > H W instead of the reference's two fp32 divisions."""
import numpy as np
import torch

from . import meshtrace, ops

LENGTH = {"vehicle": 4.5, "person": 1.7, "bicycle": 1.6, "motorcycle": 2.}     # mesh_renderer.py:21-28 (vehicle: the centre of its random draw)


def center_mesh_bottom(vertices, category="vehicle", length=None):
    """mesh_renderer.py:14-34 on whatever device `vertices` [V,3] lives: the bounding box centred, the mesh resting on y = 0, scaled so that
    its longest box side is the category's length (vehicle 4.5, person 1.7, bicycle 1.6, motorcycle 2, anything else: unscaled).
    `length` replaces the reference's `4.5 + (np.random.random() - 0.5) * 0.2` draw for vehicles (and overrides any category).  No host read."""
    v = vertices.to(torch.float32)
    lo, hi = v.min(dim=0, keepdim=True).values, v.max(dim=0, keepdim=True).values
    v = v - (hi + lo) / 2.
    l0 = (hi - lo).max()
    l = length if length is not None else LENGTH.get(category)
    scale = 1. if l is None else l / l0
    v = torch.cat([v[:, :1], v[:, 1:2] - v[:, 1].min(), v[:, 2:]], dim=1)
    return v * scale


def _tensor(a, dtype, device):
    t = a if torch.is_tensor(a) else torch.tensor(np.asarray(a))
    return t.to(device=device, dtype=dtype)


def pack_materials(materials, device):
    """a list of [1,3,h,w] or [3,h,w] float tensors (a `map_Kd / 255.` map or a [1,3,1,1] `Kd` constant, as the reference holds them) ->
    (texels [T,4] fp32 = (r, g, b, 0) of every map back to back, table [M,4] int32 = (texel offset, h, w, 0))"""
    tex, table, off = [], [], 0
    for i, m in enumerate(materials):
        m = _tensor(m, torch.float32, device)
        if m.dim() == 4 and m.shape[0] == 1:
            m = m[0]
        if m.dim() != 3 or m.shape[0] != 3 or m.shape[1] < 1 or m.shape[2] < 1:
            raise ValueError(f"MeshRenderer: material {i} has shape {tuple(m.shape)}, expected [1,3,h,w] or [3,h,w]")
        h, w = int(m.shape[1]), int(m.shape[2])
        tex.append(torch.cat([m.permute(1, 2, 0).reshape(h * w, 3), torch.zeros(h * w, 1, dtype=torch.float32, device=device)], dim=1))
        table.append((off, h, w, 0))
        off += h * w
    if off >= 2 ** 31:
        raise ValueError("MeshRenderer: the materials hold 2^31 texels or more")
    return torch.cat(tex).contiguous(), torch.tensor(table, dtype=torch.int32).to(device)


class MeshRenderer:
    """`MeshRenderer(vertices, faces, vertex_color=...)` for a vertex-colour mesh (.ply: vertex_color [V,3] in 0..1) or
    `MeshRenderer(vertices, faces, uvs=..., face_uvs_idx=..., materials=..., face_material_idx=None)` for a textured one (.obj: uvs [U,2],
    face_uvs_idx [F,3] with -1 = no uv, materials as `pack_materials` takes them, face_material_idx [F], default zeros as
    mesh_renderer.py:159).  `uvs % 1` is applied here, as the reference does at load time.  Raises ValueError for inconsistent shapes or a
    face index outside [0, V) -- the one host read of this class.  Index VALUES of face_uvs_idx and face_material_idx are not read on the host:
    the kernel checks each before use (outside [0, U): uv = (0, 0); outside [0, M): colour 0)."""

    def __init__(self, vertices, faces, vertex_color=None, uvs=None, face_uvs_idx=None, materials=None, face_material_idx=None, device=None):
        textured = uvs is not None or face_uvs_idx is not None or materials is not None or face_material_idx is not None
        if (vertex_color is not None) == textured:
            raise ValueError("MeshRenderer: give either vertex_color or (uvs, face_uvs_idx, materials), not both and not neither")
        if textured and (uvs is None or face_uvs_idx is None or materials is None):
            raise ValueError("MeshRenderer: a textured mesh needs uvs, face_uvs_idx and materials")
        self.tracer = meshtrace.RayTracer(vertices, faces, device=device)
        dev, F, V = self.tracer.device, self.tracer.n_faces, self.tracer.vertices.shape[0]
        self.device = dev
        order = self.tracer.face_ids.long()                                     # ordered position -> the caller's face
        self.vertex_color = self.uvs = self.face_uvs_idx = self.face_material_idx = self.texels = self.materials = None
        if not textured:
            c = _tensor(vertex_color, torch.float32, dev)
            if tuple(c.shape) != (V, 3):
                raise ValueError(f"MeshRenderer: vertex_color has shape {tuple(c.shape)}, expected {(V, 3)}")
            self.vertex_color = c.contiguous()
            return
        uv = _tensor(uvs, torch.float32, dev)
        if uv.dim() != 2 or uv.shape[1] != 2:
            raise ValueError(f"MeshRenderer: uvs has shape {tuple(uv.shape)}, expected [U, 2]")
        fu = _tensor(face_uvs_idx, torch.int64, dev)
        if tuple(fu.shape) != (F, 3):
            raise ValueError(f"MeshRenderer: face_uvs_idx has shape {tuple(fu.shape)}, expected {(F, 3)}")
        fm = torch.zeros(F, dtype=torch.int64, device=dev) if face_material_idx is None else _tensor(face_material_idx, torch.int64, dev)
        if tuple(fm.shape) != (F,):
            raise ValueError(f"MeshRenderer: face_material_idx has shape {tuple(fm.shape)}, expected {(F,)}")
        if len(materials) < 1:
            raise ValueError("MeshRenderer: a textured mesh needs at least one material")
        self.uvs = (uv % 1.).contiguous()                                       # mesh_renderer.py:157
        self.face_uvs_idx = fu[order].to(torch.int32).contiguous()              # in the order the kernel walks the faces
        self.face_material_idx = fm[order].to(torch.int32).contiguous()
        self.texels, self.materials = pack_materials(materials, dev)

    def render(self, fx, fy, cx, cy, H, W, transform=None, t_max=meshtrace.MAX_DEPTH, validate=True, want=(), miss_value=meshtrace.MAX_DEPTH, flags=0):
        """-> (image [H,W,3] uint8, mask [H,W,3] uint8 = 255 / 0, {name: tensor for name in `want`}) with the optional outputs "image_f"
        ([H,W,3] fp32, the clamped colour), "depth" ([H,W] fp32: the z-depth or miss_value) and "face_id" ([H,W] int32 in the constructor's
        numbering, -1 on a miss).  `transform`: the tracer's 3 x 4 / 4 x 4 map from mesh to camera coordinates (-z forward, +y up, host or
        device).  `validate`: an invalid frame (mesh_renderer.py:44-53) comes back empty.  No host sync."""
        unknown = set(want) - {"image_f", "depth", "face_id"}
        ops._require(not unknown, "want: unknown outputs %s", sorted(unknown))
        ws = self.tracer.prepare(transform)
        image, image_f, mask, depth, face_id = ops.mesh_render_pinhole(
            ws, self.tracer.n_faces, fx, fy, cx, cy, H, W, faces=self.tracer.faces if self.vertex_color is not None else None,
            vertex_color=self.vertex_color, uvs=self.uvs, face_uvs_idx=self.face_uvs_idx, face_material_idx=self.face_material_idx,
            texels=self.texels, materials=self.materials, t_max=t_max, miss_value=miss_value, validate=validate, flags=flags,
            want_image_f="image_f" in want, want_mask=True, want_depth="depth" in want, want_face_id="face_id" in want, device=self.device)
        extra = {k: v for k, v in (("image_f", image_f), ("depth", depth), ("face_id", face_id)) if k in want}
        return image, mask, extra
