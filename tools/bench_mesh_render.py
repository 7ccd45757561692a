#!/usr/bin/env python3
"""The instance image and mask of one foreground mesh at the path C frame size on one MI355X: snerf_mesh_prepare +
snerf_mesh_render_pinhole (meshrender.MeshRenderer.render's two calls) next to the tracer it is built on, in the same process.

    (a) trace            prepare + snerf_mesh_trace_pinhole, pixel centres, no mask, depth and hit mask: visibility alone (the yardstick)
    (b) vertex colours   prepare + render from vertex colours, image and mask, frame validity on
    (c) texture          prepare + render from one 1024 x 1024 texture, image and mask, frame validity on
    (d) texture, no validity   (c) with validate off: the verdict and the finishing launch left out
    prepare              the prepare launches alone

Device events around the calls, medians over --rounds rounds after --warmup; the legs alternate within a round and every timed call
follows an untimed call of the same leg.  The mesh and the camera are tools/bench_mesh_trace.py's: an icosphere subdivided 6 times
stretched to a car-sized ellipsoid 9 m in front of the camera plus a ground quad split into 18 432 triangles, 100 352 faces; the ground
is narrowed to 0.3 of its width so that the mask does not touch both the left and the right column (the frame is valid, as a frame
the stages keep is; `frame_valid` in the output says so).  Prints one JSON line; --out also writes it to a text file."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from bench_mesh_trace import event_ms, ground, icosphere


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1280)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--texture", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from snerf_amd import meshrender
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    torch.cuda.set_device(0)
    H, W = args.height, args.width
    sv, sf = icosphere(6)
    gv, gf = ground(96, 96)
    gv[:, 0] *= 0.3
    c, s = np.cos(0.6), np.sin(0.6)
    car = sv @ (np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) @ np.diag([2.2, 0.8, 0.9])).T + np.array([0.4, -0.3, -9.])
    V = np.concatenate([car, gv]).astype(np.float32)
    F = np.concatenate([sf, gf + len(car)])
    rng = np.random.default_rng(0)
    colour = meshrender.MeshRenderer(V, F, vertex_color=rng.uniform(0, 1, (len(V), 3)).astype(np.float32))
    # uvs: a smooth chart (the direction from the mesh's centre), so neighbouring pixels fetch neighbouring texels as an unwrapped .obj does
    n = V - V.mean(0)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    uvs = np.stack([np.arctan2(n[:, 0], n[:, 2]) / (2 * np.pi) + 0.5, np.arccos(np.clip(n[:, 1], -1, 1)) / np.pi], 1).astype(np.float32)
    tex = torch.from_numpy(rng.integers(0, 256, (1, 3, args.texture, args.texture)).astype(np.float32) / np.float32(255.))
    textured = meshrender.MeshRenderer(V, F, uvs=uvs, face_uvs_idx=F, materials=[tex])
    fx = fy = 0.8 * W
    cx, cy = W / 2 - 0.2, H / 2 + 0.3
    res = {}
    legs = {"a_trace": lambda: res.__setitem__("a", colour.tracer.trace_pinhole(fx, fy, cx, cy, H, W, True, want_hit=True)),
            "b_vertex_colours": lambda: res.__setitem__("b", colour.render(fx, fy, cx, cy, H, W)),
            "c_texture": lambda: res.__setitem__("c", textured.render(fx, fy, cx, cy, H, W)),
            "d_texture_no_validity": lambda: res.__setitem__("d", textured.render(fx, fy, cx, cy, H, W, validate=False)),
            "prepare": lambda: colour.tracer.prepare(None)}
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
    hit = res["a"][1]
    same = all(torch.equal(res[k][1], hit) for k in "bcd") and torch.equal(res["c"][0], res["d"][0])
    line = {"shape": [H, W], "faces": int(len(F)), "vertices": int(len(V)), "texture": [args.texture, args.texture],
            "hit_share": round(float((hit[..., 0] > 0).float().mean()), 4), "rounds": args.rounds,
            "ms": {k: round(v, 4) for k, v in med.items()}, "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()},
            "vertex_colours_over_trace": round(med["b_vertex_colours"] / med["a_trace"], 3), "texture_over_trace": round(med["c_texture"] / med["a_trace"], 3),
            "frame_valid": bool(res["c"][1].any()), "validity_ms": round(med["c_texture"] - med["d_texture_no_validity"], 4), "masks_equal_the_tracers": bool(same)}
    out = json.dumps(line)
    print(out, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/bench_mesh_render.py: image and mask of one instance (snerf_mesh_prepare + snerf_mesh_render_pinhole), one MI355X, device events,\n")
            f.write("# medians in ms.  a = prepare + snerf_mesh_trace_pinhole with the hit mask (visibility alone), b = render from vertex colours, c = render\n")
            f.write("# from one texture, d = c without the frame-validity launches; prepare = its launches alone.\n")
            f.write(out + "\n")


if __name__ == "__main__":
    main()
