#!/usr/bin/env python3
"""Training-loop cost of the batch producers, one MI355X: ms per step of whole loops (host work + launches + GPU), wall clock over
--steps steps after --warmup, with a device sync at the end of each timed loop only.
  path A (bench.py's model, bf16, 4096 rays; 6 frames 1600 x 900 fp32 on the host, sparse LiDAR depth, near_far on):
    a_host      the reference-shaped loop: a shuffled image per step, its upload, sample_single_img (numpy pixel draw, near_far
                min / max read back), MipTrainer.step
    a_batcher   sample_utils.ImageRayBatcher.next() (training set resident) + MipTrainer.step
    a_graph     MipTrainer.capture(batcher=...) + replay(): draw and step as one graph launch
  path C (zipnerf.Model fp16, 65 536 rays; 8 frames 1920 x 1280):
    c_host      a numpy _make_ray_batch-shaped batch (np.random.randint draws, float64 pixels_to_rays, gathers from fp32 host images)
                + its upload + ZipTrainer.step
    c_batcher   zipnerf.RayBatcher.next() (uint8 images resident) + ZipTrainer.step
  the batchers alone: next_4096 (ImageRayBatcher), next_65536 (RayBatcher), device events over --draws calls.
Prints one JSON line.  --legs selects legs (comma list)."""
import argparse
import json
import math
import os
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def _wall(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t) * 1e3 / steps, 3)


def _events(fn, n):
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b) * 1e3 / n, 2)


def path_a_scene(N=6, H=900, W=1600, seed=0):
    rng = np.random.default_rng(seed)
    images = rng.random((N, H, W, 3), dtype=np.float32)
    depths = np.zeros((N, H, W), np.float32)
    hit = rng.random((N, H, W)) < 0.05                                     # sparse LiDAR returns
    depths[hit] = rng.uniform(2.0, 80.0, int(hit.sum())).astype(np.float32)
    poses = np.zeros((N, 3, 4), np.float32)
    for i in range(N):
        th = 2 * math.pi * i / N
        poses[i, :, :3] = [[math.cos(th), 0, math.sin(th)], [0, 1, 0], [-math.sin(th), 0, math.cos(th)]]
        poses[i, :, 3] = rng.normal(0, 0.1, 3)
    K = np.tile(np.array([[1266.0, 0, W / 2], [0, 1266.0, H / 2], [0, 0, 1]], np.float32), (N, 1, 1))
    return images, depths, poses, K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--draws", type=int, default=200)
    ap.add_argument("--legs", default="a_host,a_batcher,a_graph,c_host,c_batcher,next")
    args = ap.parse_args()
    legs = set(args.legs.split(","))
    import bench
    from oracle import callers as oc
    from snerf_amd import sample_utils as su, zipnerf
    from snerf_amd.trainer import MipTrainer, ZipTrainer
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    res = {"steps": args.steps, "warmup": args.warmup}

    # ---- path A
    images, depths, poses, K = path_a_scene()
    N = images.shape[0]
    i_train, cam = list(range(N)), np.arange(N, dtype=np.float64)
    sargs = types.SimpleNamespace(no_ndc=True, smooth_loss=False, near_far=True, N_rgb=4096)
    n = 4096
    batcher = su.ImageRayBatcher(sargs, images, depths, poses, K, i_train, 1.8, 110.0, camera_index=cam, batch_n=n, device=dev)
    model = bench.build_model("bf16", dev)
    tr = MipTrainer(model, lr=5e-4)
    if "a_host" in legs:
        order = []

        def host_step():
            if not order:
                order.extend(np.random.permutation(i_train).tolist())         # DataLoader(shuffle=True, batch_size=1)
            i = order.pop()
            rays, trgb, tdep, _, _ = su.sample_single_img(sargs, torch.tensor(images[i]).to(dev), torch.tensor(depths[i]).to(dev), poses[i], K[i],
                                                          1.8, 110.0, near_far=True, batch_n=n, app=cam[i])
            tr.step(rays, trgb, tdep, None)
        res["a_host_ms"] = _wall(host_step, args.steps, args.warmup)
    if "a_batcher" in legs:
        def batcher_step():
            rays, trgb, tdep, _, _, _ = batcher.next()
            tr.step(rays, trgb, tdep, None)
        res["a_batcher_ms"] = _wall(batcher_step, args.steps, args.warmup)
    if "a_graph" in legs:
        tr.capture(None, None, warmup=2, batcher=batcher)
        res["a_graph_ms"] = _wall(tr.replay, args.steps, args.warmup)
    if "next" in legs:
        res["next_4096_us"] = _events(batcher.next, args.draws)
        buf = batcher.buffers()
        res["next_into_4096_us"] = _events(lambda: batcher.next_into(buf), args.draws)
    del batcher, tr, model, images, depths
    torch.cuda.empty_cache()

    # ---- path C
    Nc, Hc, Wc, R = 8, 1280, 1920, 65536
    rng = np.random.default_rng(1)
    imgs_u8 = rng.integers(0, 256, size=(Nc, Hc, Wc, 3), dtype=np.uint8)
    Kc = np.array([[2050.0, 0.0, 960.0], [0.0, 2050.0, 640.0], [0.0, 0.0, 1.0]])
    pixtocams = np.tile(np.linalg.inv(Kc).astype(np.float32), (Nc, 1, 1))
    c2w = np.tile(np.eye(4, dtype=np.float32)[:3], (Nc, 1, 1))
    c2w[:, :, 3] = rng.normal(0, 0.03, (Nc, 3))
    near, far = 0.02, 100.0
    zb = zipnerf.RayBatcher(imgs_u8, pixtocams, c2w, near, far, batch_size=R, device=dev)
    if "next" in legs:
        res["next_65536_us"] = _events(zb.next, args.draws)
        zbuf = zb.buffers()
        res["next_into_65536_us"] = _events(lambda: zb.next_into(zbuf), args.draws)
    if "c_host" in legs or "c_batcher" in legs:
        torch.manual_seed(0)
        m = zipnerf.Model(config=None, raydist_fn='power_transformation', opaque_background=True, compute="fp16", table_dtype="ref",
                          init_std=0.1, device=dev)
        ztr = ZipTrainer(m, lr=1e-2)
        if "c_host" in legs:
            imgs_f32 = (imgs_u8 / 255.).astype(np.float32)                   # the reference's loaders keep float images on the host

            def host_batch():
                x = np.random.randint(0, Wc, R)
                y = np.random.randint(0, Hc, R)
                c = np.random.randint(0, Nc, R)
                b = oc.zip_pixels_to_rays(x, y, c, pixtocams, c2w)
                b.update(lossmult=np.ones((R, 1)), near=np.full((R, 1), near), far=np.full((R, 1), far), cam_idx=c[:, None],
                         rgb=imgs_f32[c, y, x])
                return {k: torch.from_numpy(np.ascontiguousarray(v)).float().to(dev) for k, v in b.items()}

            def c_host_step():
                b = host_batch()
                ztr.step(b, b["rgb"], train_frac=0.5, rand=True)
            res["c_host_ms"] = _wall(c_host_step, max(args.steps // 2, 3), 2)
            del imgs_f32
        if "c_batcher" in legs:
            def c_batcher_step():
                b = zb.next()
                ztr.step(b, b["rgb"], train_frac=0.5, rand=True)
            res["c_batcher_ms"] = _wall(c_batcher_step, max(args.steps // 2, 3), 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
