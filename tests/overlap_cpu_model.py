"""Float64 numpy statement of the reference's occlusion order (s-nerfpp/stage1_code/utils_render.py:691-808 occlution_order) as
snerf_amd.foreground.occlusion_order specifies it: the model the device path is compared with (tests/test_occlusion_order.py).

  overlap_stats       (count, sum row, sum col) of np.where((mask_a > 0) & (mask_b > 0)) per pair a < b        (:745-751)
  centroid_ray        the pair's one ray, ray_frame "reference" (world-frame ray, :752-760) or "camera" (origin 0, inv(P) pixel)
  first_hit           all-pairs Moeller-Trumbore, nearest t > 0 (the reference of tests/test_mesh_trace.py), with the ray's margin
  face_centre_z       z of the centre of a face under the placement; -1 (a miss) is the LAST face, as `tri[-1]` is           (:732-736)
  occlusion_order     the matrix (:781-792) and the literal sort loop (:795-806)

trimesh is not in the reference tree: what `intersects_first` does with a ray through an edge is not pinned, so the scenes of the tests
keep every ray away from every edge (`margin`) and every compared pair of z apart (`z_gap`)."""
import numpy as np


def overlap_stats(masks):
    """masks: N arrays [H,W,3] -> int64 [N,N,3]; (a, b), a < b: (count, sum of i, sum of j) over np.where of the intersection"""
    N = len(masks)
    out = np.zeros((N, N, 3), dtype=np.int64)
    for a in range(N):
        for b in range(a + 1, N):
            inter = np.logical_and(np.asarray(masks[a]) > 0, np.asarray(masks[b]) > 0)
            i_list, j_list, _ = np.where(inter > 0)
            out[a, b] = (i_list.size, i_list.astype(np.int64).sum(), j_list.astype(np.int64).sum())
    return out


def centroid_ray(stat, w2c, P, ray_frame="reference"):
    """stat = (count, sum i, sum j) with count > 0 -> (ray_o [3], ray_d [3]) float64"""
    count, si, sj = (float(v) for v in stat)
    pixel = np.array([sj / count, si / count, 1.]).reshape(3, 1)
    point = np.linalg.inv(np.asarray(P, dtype=np.float64)) @ pixel
    if ray_frame == "camera":
        return np.zeros(3), point[:, 0]
    assert ray_frame == "reference"
    c2w = np.linalg.inv(np.asarray(w2c, dtype=np.float64))
    point = (c2w @ np.concatenate((point, [[1.]]), axis=0))[:3, 0]
    ray_o = c2w[:3, 3]
    return ray_o, (point - ray_o) / np.linalg.norm(point - ray_o)


def first_hit(o, d, V, F):
    """one ray against every triangle in float64 -> (face of the nearest hit with t > 0 or -1, its t or inf, margin).  margin: the least
    |min(u, v, 1 - u - v)| over the triangles in front of the origin (t > 0, non-zero determinant) -- how far, in barycentric
    coordinates, the ray is from changing sides of any triangle's outline; inf when no triangle's plane lies in front."""
    o, d, V = np.asarray(o, np.float64), np.asarray(d, np.float64), np.asarray(V, np.float64)
    F = np.asarray(F)
    a, e1, e2 = V[F[:, 0]], V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]]
    p = np.cross(d[None], e2)
    det = (e1 * p).sum(-1)
    with np.errstate(all="ignore"):
        tv = o[None] - a
        u = (tv * p).sum(-1) / det
        q = np.cross(tv, e1)
        v = (d[None] * q).sum(-1) / det
        t = (e2 * q).sum(-1) / det
        inside = np.minimum(np.minimum(u, v), 1 - u - v)
    front = (det != 0) & (t > 0)
    margin = np.abs(np.where(front, inside, np.inf)).min() if len(F) else np.inf
    tt = np.where(front & (inside >= 0), t, np.inf)
    k = int(tt.argmin()) if len(F) else -1
    if k < 0 or not np.isfinite(tt[k]):
        return -1, np.inf, float(margin)
    return k, float(tt[k]), float(margin)


def place(V, T):
    """vertices [V,3] under the 3 x 4 (or 4 x 4) placement T (None: as they are), float64"""
    V = np.asarray(V, dtype=np.float64)
    if T is None:
        return V
    T = np.asarray(T, dtype=np.float64)[:3]
    return V @ T[:, :3].T + T[:, 3]


def face_centre_z(V, F, T, face):
    """mesh.triangles_center[face, 2] of the placed mesh; face = -1 (a miss) indexes the last face"""
    return float(place(V, T)[np.asarray(F)[face]].mean(axis=0)[2])


def topological_order(before):
    """utils_render.py:795-806, literally"""
    A = np.array(before).astype(np.uint8)
    n = A.shape[0]
    result_list = []
    while len(result_list) < n:
        for i in range(n):
            if i not in result_list and np.sum(A[:, i]) == 0:
                result_list.append(i)
                for j in range(n):
                    if A[i, j] == 1:
                        A[i, j] = 0
                break
        else:
            raise RuntimeError("Occlusion judgment fails....")
    return result_list


def occlusion_order(masks, meshes, w2c, P, ray_frame="reference", sort=True):
    """masks: N arrays [H,W,3]; meshes: N triples (V [V,3], F [F,3], T 3 x 4 placement into camera coordinates or None).
    -> dict(order (None with sort = False), before int8 [N,N], stats, z {(a, b): (z_a, z_b)}, faces {(a, b): (face_a, face_b)},
    z_gap = the least |z_a - z_b| and margin = the least first_hit margin over the overlapping pairs (inf without one))"""
    N = len(masks)
    stats = overlap_stats(masks)
    before = np.zeros((N, N), dtype=np.int8)
    z, faces, z_gap, margin = {}, {}, np.inf, np.inf
    for a in range(N):
        for b in range(a + 1, N):
            if stats[a, b, 0] == 0:
                continue
            ray_o, ray_d = centroid_ray(stats[a, b], w2c, P, ray_frame)
            zs, fs = [], []
            for V, F, T in (meshes[a], meshes[b]):
                face, _, m = first_hit(ray_o, ray_d, place(V, T), F)
                margin = min(margin, m)
                fs.append(face)
                zs.append(face_centre_z(V, F, T, face))
            z[a, b], faces[a, b] = tuple(zs), tuple(fs)
            z_gap = min(z_gap, abs(zs[0] - zs[1]))
            if zs[0] < zs[1]:          # A occludes B: B should appear first
                before[b, a] = 1
            else:
                before[a, b] = 1
    return dict(order=topological_order(before) if sort else None, before=before, stats=stats, z=z, faces=faces, z_gap=z_gap, margin=margin)


def mask_from_mesh(V, F, H, W, K):
    """snerf_amd.foreground.mask_from_mesh on the host: [H,W,3] uint8, 255 where the pixel-centre ray d = ((x + .5 - cx) / fx,
    -(y + .5 - cy) / fy, -1) from the origin hits the mesh (vertices as given: a camera that looks down -z, y up) with 0 < t < 100"""
    V, F = np.asarray(V, np.float64), np.asarray(F)
    fx, fy, cx, cy = K[0][0], K[1][1], K[0][2], K[1][2]
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64), indexing="xy")
    d = np.stack([(x + .5 - cx) / fx, -((y + .5 - cy) / fy), -np.ones_like(x)], -1).reshape(-1, 1, 3)
    a, e1, e2 = V[F[:, 0]][None], (V[F[:, 1]] - V[F[:, 0]])[None], (V[F[:, 2]] - V[F[:, 0]])[None]
    p = np.cross(d, e2)
    det = (e1 * p).sum(-1)
    with np.errstate(all="ignore"):
        u = (-a * p).sum(-1) / det
        q = np.cross(-a, e1)
        v = (d * q).sum(-1) / det
        t = (e2 * q).sum(-1) / det
        hit = ((det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0) & (t < 100.)).any(1).reshape(H, W)
    return np.repeat(np.where(hit, 255, 0).astype(np.uint8)[..., None], 3, axis=2)
