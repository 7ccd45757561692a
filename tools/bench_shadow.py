#!/usr/bin/env python3
"""The projected shadow of one foreground instance at the path C frame size on one MI355X: `shadow.ShadowCaster.cast` (snerf_shadow_project
+ snerf_shadow_close + snerf_shadow_fuse) and its three stages on their own, in the same process.

    cast      the whole call: project and splat, closing (r = 20, 3 iterations), bounding box + box counts + fuse
    project   snerf_shadow_project alone (two-stage minimum of z, splat)
    close     snerf_shadow_close alone, on the splat project left in the scratch
    fuse      snerf_shadow_fuse alone, on the closed mask close left in the scratch

Device events around the calls, medians over --rounds rounds after --warmup; the legs alternate within a round and every timed call
follows an untimed call of the same leg.  The instance is a car-sized ellipsoid of --vertices points 9 m in front of a camera 1.5 m
above the ground.  `cpu_model_s` is tests/shadow_cpu_model.py (numpy float64, one run) on the same inputs: context only, it stands in
for the reference's PIL / numpy / cv2 route, which cannot run here; `equals_model` says whether the frame it gives equals the device's
bit for bit.  Prints one JSON line; --out also writes it to a text file."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from bench_mesh_trace import event_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1280)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--vertices", type=int, default=100000)
    ap.add_argument("--r", type=int, default=20)
    ap.add_argument("--iter", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from snerf_amd import ops, shadow
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    torch.cuda.set_device(0)
    H, W, N = args.height, args.width, args.vertices
    rng = np.random.default_rng(0)
    d = rng.normal(size=(N, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    vertices = d * np.array([2.1, 0.9, 0.75]) + np.array([0., 0., 0.75])
    c2w = np.eye(4)
    c2w[:3, :3] = np.array([[0., 0., 1.], [-1., 0., 0.], [0., -1., 0.]])
    c2w[:3, 3] = [0., 0., 1.5]
    P = np.array([[0.8 * W, 0., W / 2 - 0.2], [0., 0.8 * W, H / 2 + 0.3], [0., 0., 1.]])
    kw = dict(bbox_center=(9., 0.4, 0.), theta=31., mesh_bias=(0.1, 0., 0.), pitch_angle=38., yaw_angle=115., c2w=c2w, P=P, ground_height=None)
    im = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    total = np.zeros((H, W, 3), np.uint8)
    total[H // 3:2 * H // 3, 2 * W // 5:3 * W // 5] = 255
    caster = shadow.ShadowCaster(H, W, N, args.r, args.iter)
    d_v, d_total, d_im = torch.from_numpy(vertices).cuda(), torch.from_numpy(total).cuda(), torch.from_numpy(im).cuda()
    first = d_im.clone()
    caster.cast(first, d_total, d_v, **kw)
    info = ops.shadow_ws_views(caster.ws, H, W)[0].tolist()
    mode = shadow._pack_xf(caster._xf, shadow.process_placement(kw["bbox_center"], kw["theta"], kw["mesh_bias"]),
                           shadow.light_vector(kw["pitch_angle"], kw["yaw_angle"]), None, shadow.world_to_pixel(c2w, P))
    legs = {"cast": lambda: caster.cast(d_im, d_total, d_v, **kw),
            "project": lambda: ops.shadow_project(d_v, caster._xf, mode, H, W, caster.ws),
            "close": lambda: ops.shadow_close(None, H, W, args.r, args.iter, caster.ws),
            "fuse": lambda: ops.shadow_fuse(d_im, d_total, None, H, W, .55, False, caster.ws)}
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
    line = {"shape": [H, W], "vertices": N, "r": args.r, "iter": args.iter, "rounds": args.rounds, "shadow_pixels_share": None, "blur_kernel": info[1:3],
            "bounding_box": info[3:7], "ms": {k: round(v, 4) for k, v in med.items()}, "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()}}
    closed = torch.empty(H, W, 3, dtype=torch.uint8, device="cuda")
    ops.shadow_project(d_v, caster._xf, mode, H, W, caster.ws)
    ops.shadow_close(None, H, W, args.r, args.iter, caster.ws, closed)
    line["shadow_pixels_share"] = round(float((closed[..., 0] > 0).float().mean()), 4)
    if not args.no_model:
        import shadow_cpu_model as model
        t0 = time.perf_counter()
        want = model.cast(im, total, vertices, interpolate_r=args.r, interpolate_iter=args.iter, **kw)
        line["cpu_model_s"] = round(time.perf_counter() - t0, 2)
        line["equals_model"] = bool(np.array_equal(first.cpu().numpy(), want))
    out = json.dumps(line)
    print(out, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/bench_shadow.py: the projected shadow of one instance (snerf_shadow_project + snerf_shadow_close + snerf_shadow_fuse), one MI355X,\n")
            f.write("# device events, medians in ms.  cast = ShadowCaster.cast, the three stages back to back; project / close / fuse = each entry alone on the\n")
            f.write("# scratch the previous one left.  cpu_model_s = tests/shadow_cpu_model.py (numpy float64) on the same inputs, seconds, context only.\n")
            f.write(out + "\n")


if __name__ == "__main__":
    main()
