#!/usr/bin/env python3
"""The mesh depth of one foreground instance at the path C frame size on one MI355X: snerf_mesh_prepare + snerf_mesh_trace_pinhole
(foreground.mesh_depth's two calls) for a mesh of about 10^5 triangles against a 1920 x 1280 mask that covers about 10 % of the frame.

    (a) culled         prepare + trace with the chunk and group boxes, every entered chunk staged in LDS (the shipped flavour)
    (b) culled, uniform the same with the chunk's records read through wave-uniform global loads instead (flag MESH_UNIFORM)
    (c) all pairs      the shipped kernel with culling switched off (flag MESH_NO_CULL: every chunk entered)
    (d) all pairs, uniform (c) with MESH_UNIFORM
    (e) torch          an all-pairs Moeller-Trumbore written in torch ops, on --torch-rays of the masked rays against --torch-faces of
                       the faces (what fits memory), scaled to the full problem by the pair count: a reference point, not a competitor
    prepare            the prepare launches alone

Device events around the calls, medians over --rounds rounds after --warmup; the flavours alternate within a round and every timed call
follows an untimed call of the same leg (without it the first leg of a round measured 0.2 ms more than the same flavour elsewhere).  The mesh is an
icosphere subdivided 6 times (81 920 faces) stretched to a car-sized ellipsoid 9 m in front of the camera plus a ground quad split into
18 432 triangles: 100 352 faces.  Prints one JSON line; --out also writes it to a text file."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def icosphere(n):
    t = (1 + 5 ** 0.5) / 2
    v = np.array([(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1),
                  (-t, 0, 1)], dtype=np.float64)
    f = np.array([(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
                  (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)])
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    for _ in range(n):
        e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
        ue, inv = np.unique(e, axis=0, return_inverse=True)
        m = v[ue[:, 0]] + v[ue[:, 1]]
        mid = len(v) + inv.reshape(3, -1)                                        # midpoint vertex of edge j of every face
        v = np.concatenate([v, m / np.linalg.norm(m, axis=1, keepdims=True)])
        a, b, c, ab, bc, ca = f[:, 0], f[:, 1], f[:, 2], mid[0], mid[1], mid[2]
        f = np.concatenate([np.stack(q, 1) for q in ((a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca))])
    return v, f


def ground(nx, nz, y=-1.1):
    x, z = np.meshgrid(np.linspace(-6, 6, nx + 1), np.linspace(-4, -16, nz + 1), indexing="xy")
    v = np.stack([x, np.full_like(x, y), z], -1).reshape(-1, 3)
    i = (np.arange(nz)[:, None] * (nx + 1) + np.arange(nx)[None]).reshape(-1)
    return v, np.concatenate([np.stack([i, i + 1, i + nx + 2], 1), np.stack([i, i + nx + 2, i + nx + 1], 1)])


def torch_all_pairs(o, d, V, F):
    """nearest t > 0 of an all-pairs Moeller-Trumbore in torch ops (fp32): [R] with 100 on a miss"""
    a, e1, e2 = V[F[:, 0]], V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]]
    p = torch.cross(d[:, None], e2[None], dim=-1)
    det = (e1[None] * p).sum(-1)
    tv = o[:, None] - a[None]
    u = (tv * p).sum(-1) / det
    q = torch.cross(tv, e1[None].expand_as(tv), dim=-1)
    v = (d[:, None] * q).sum(-1) / det
    t = (e2[None] * q).sum(-1) / det
    ok = (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0) & (t < 100.)
    return torch.where(ok, t, torch.full_like(t, 100.)).min(dim=1).values


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1280)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--torch-rays", type=int, default=2048)
    ap.add_argument("--torch-faces", type=int, default=8192)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from snerf_amd import meshtrace, ops
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    torch.cuda.set_device(0)
    H, W = args.height, args.width
    sv, sf = icosphere(6)
    gv, gf = ground(96, 96)
    c, s = np.cos(0.6), np.sin(0.6)
    car = sv @ (np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) @ np.diag([2.2, 0.8, 0.9])).T + np.array([0.4, -0.3, -9.])
    V = np.concatenate([car, gv]).astype(np.float32)
    F = np.concatenate([sf, gf + len(car)])
    rt = meshtrace.RayTracer(V, F)
    fx = fy = 0.8 * W
    cx, cy = W / 2 - 0.2, H / 2 + 0.3
    yy, xx = np.mgrid[:H, :W]
    m = ((yy - (cy + 0.3 * fy / 9)) / (0.178 * H)) ** 2 + ((xx - (cx + 0.4 * fx / 9)) / (0.178 * W)) ** 2 <= 1       # an ellipse of ~10 % of the frame around the car
    mask = torch.from_numpy((m[..., None].repeat(3, -1) * 255).astype(np.uint8)).cuda()
    res = {}

    def trace(flags):
        rt.prepare(None)
        res[flags] = ops.mesh_trace_pinhole(rt.ws, rt.n_faces, fx, fy, cx, cy, False, H, W, mask, 99., .1, flags=flags)[0]
    legs = {"a_culled": lambda: trace(0), "b_culled_uniform": lambda: trace(ops.MESH_UNIFORM), "c_all_pairs": lambda: trace(ops.MESH_NO_CULL),
            "d_all_pairs_uniform": lambda: trace(ops.MESH_NO_CULL | ops.MESH_UNIFORM), "prepare": lambda: rt.prepare(None)}
    # the torch expression on a subset that fits memory
    ys, xs = np.nonzero(m)
    pick = np.random.default_rng(0).choice(len(ys), args.torch_rays, replace=False)
    d = np.stack([(xs[pick].astype(np.float32) - np.float32(cx)) / np.float32(fx), -((ys[pick].astype(np.float32) - np.float32(cy)) / np.float32(fy)),
                  -np.ones(len(pick), np.float32)], 1)
    td, to = torch.from_numpy(d).cuda(), torch.zeros(len(pick), 3, device="cuda")
    tV, tF = torch.from_numpy(V).cuda(), torch.from_numpy(F[:args.torch_faces]).cuda()
    legs["e_torch_subset"] = lambda: res.__setitem__("torch", torch_all_pairs(to, td, tV, tF))
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            fn()                                                                # untimed: whatever leg ran before, the timed call finds its own warm state
            t[k].append(event_ms(fn))
    med = {k: statistics.median(v) for k, v in t.items()}
    same = all(torch.equal(res[0], res[f]) for f in (ops.MESH_UNIFORM, ops.MESH_NO_CULL, ops.MESH_NO_CULL | ops.MESH_UNIFORM))
    depth = res[0].cpu().numpy()
    pairs_full, pairs_sub = float(m.sum()) * len(F), float(args.torch_rays) * args.torch_faces
    line = {"shape": [H, W], "faces": int(len(F)), "vertices": int(len(V)), "masked_rays": int(m.sum()), "masked_share": round(float(m.mean()), 4),
            "hit_share_of_masked": round(float(((depth > .1) & m).sum() / m.sum()), 4), "rounds": args.rounds,
            "ms": {k: round(v, 4) for k, v in med.items()}, "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()},
            "culling_beats_all_pairs": bool(med["a_culled"] < med["c_all_pairs"]),
            "all_pairs_over_culled": round(med["c_all_pairs"] / med["a_culled"], 1),
            "uniform_loads_over_lds_culled": round(med["b_culled_uniform"] / med["a_culled"], 3),
            "uniform_loads_over_lds_all_pairs": round(med["d_all_pairs_uniform"] / med["c_all_pairs"], 3),
            "all_pairs_Gpairs_per_s": round(pairs_full / (med["c_all_pairs"] * 1e-3) / 1e9, 1),
            "torch_subset": [args.torch_rays, args.torch_faces], "torch_scaled_to_full_ms": round(med["e_torch_subset"] * pairs_full / pairs_sub, 1),
            "flavours_bit_identical": bool(same)}
    out = json.dumps(line)
    print(out, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/bench_mesh_trace.py: mesh depth of one instance (snerf_mesh_prepare + snerf_mesh_trace_pinhole), one MI355X, device events,\n")
            f.write("# medians in ms.  a = boxes + LDS staging (shipped), b = boxes + wave-uniform loads, c / d = the same kernels with culling off\n")
            f.write("# (every chunk entered), e = an all-pairs torch expression on a subset, scaled by the pair count; prepare = its launches alone.\n")
            f.write(out + "\n")


if __name__ == "__main__":
    main()
