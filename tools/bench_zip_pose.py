#!/usr/bin/env python3
"""Path C pose refinement inside the fused step (ZipTrainer(pose_net=...).step(pose="train")), one MI355X, 65 536 rays of the waymo.gin
shape (fp16 compute, a RayBatcher batch with depth targets); every figure is a median of --rounds rounds timed with device events around
back-to-back calls after a warm-up:
    kernels  ops.pose_table, ops.pose_rays_apply, ops.pose_rays_grad and ops.sgd_step alone, in microseconds, for tables of 1, 200 and
             1000 cameras with the rays spread evenly over the rows
    steps    ms per step, alternating within a round: `plain` = ZipTrainer.step without pose_net (the launches of the tree before the
             pose kernels existed), `apply` = step(pose="apply"), `train` = step(pose="train") on a table of 1000 cameras, and
             `ray_grads` = the plain step with ray_grads=True: the ray-gradient backward the "train" step needs, without the pose kernels
The reduction's share of the plain step is `grad_share_of_plain_1000` (ops.pose_rays_grad at 1000 cameras over the plain step).
Prints one JSON line; --out also writes it, with the rounds, to a text file."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

ROWS = 65536
CAMS = (1, 200, 1000)


def events(fn, n, warmup):
    """ms per call"""
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from snerf_amd import ops, poses, zipnerf
    from snerf_amd.trainer import ZipTrainer
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    N, H, W = 8, 1280, 1920
    rng = np.random.default_rng(1)
    images = rng.integers(0, 256, size=(N, H, W, 3), dtype=np.uint8)
    K = np.array([[2050.0, 0.0, 960.0], [0.0, 2050.0, 640.0], [0.0, 0.0, 1.0]])
    pixtocams = np.tile(np.linalg.inv(K).astype(np.float32), (N, 1, 1))
    c2w = np.tile(np.eye(4, dtype=np.float32)[:3], (N, 1, 1))
    c2w[:, :, 3] = rng.normal(0, 0.03, (N, 3))
    depths = (rng.random((N, H, W), dtype=np.float32) * 0.8).astype(np.float32)
    bt = zipnerf.RayBatcher(images, pixtocams, c2w, 0.02, 100.0, depths=depths, batch_size=ROWS, device=dev).next()
    tg = dict(depth=bt["depth"], depth_mask=(bt["depth"] > 0.1).float())
    gen = torch.Generator().manual_seed(3)
    rows_of = {c: torch.randint(0, c, (ROWS,), generator=gen).float().to(dev) for c in CAMS}
    res = {"rows": ROWS, "compute": "fp16", "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "reps": args.reps}
    med = lambda v: round(statistics.median(v), 4)
    lines = []

    # ---- the kernels alone
    rays = [bt[k].reshape(-1, 3).float().contiguous() for k in zipnerf.POSE_RAY_KEYS]
    grads = [torch.randn(ROWS, 3, device=dev) * 1e-3 for _ in range(5)]
    for c in CAMS:
        r, t = torch.randn(c, 3, device=dev) * 1e-2, torch.randn(c, 3, device=dev) * 1e-2
        table = ops.pose_table(r, t, 0.25)
        gr, gt = torch.zeros(c, 3, device=dev), torch.zeros(c, 3, device=dev)
        ws = torch.empty(ops.pose_rays_grad_ws(ROWS, c), dtype=torch.float64, device=dev)
        flat, fg = torch.zeros(6 * c, device=dev), torch.zeros(6 * c, device=dev)
        legs = dict(table=lambda: ops.pose_table(r, t, 0.25, out=table), apply=lambda: ops.pose_rays_apply(table, rows_of[c], *rays),
                    grad=lambda: ops.pose_rays_grad(r, 0.25, rows_of[c], *grads, *rays[1:], gr, gt, ws=ws),
                    sgd=lambda: ops.sgd_step(flat, fg, 1e-2, grad_scale=1.0 / 4096))
        for name, fn in legs.items():
            v = [events(fn, args.reps, 10) * 1e3 for _ in range(args.rounds)]
            res[f"{name}_us_{c}"] = med(v)
            lines.append(f"{name:6s} n_cams {c:5d} us per call per round: {' '.join(f'{x:.2f}' for x in v)}")

    # ---- the steps
    def trainer(pose):
        torch.manual_seed(0)
        m = zipnerf.Model(config=None, raydist_fn='power_transformation', opaque_background=True, compute="fp16", table_dtype="ref", init_std=0.1,
                          device=dev)
        return ZipTrainer(m, lr=1e-2, pose_net=poses.LearnPoseV2(CAMS[-1], t_ratio=0.25) if pose else None, pose_lr=1e-4)
    tr_plain, tr_apply, tr_train, tr_rg = trainer(False), trainer(True), trainer(True), trainer(False)
    bp = dict(bt, glo_idx=rows_of[CAMS[-1]][:, None])
    step = lambda tr, **kw: tr.step(bp, bt["rgb"], train_frac=0.5, rand=True, targets=tg, **kw)
    fns = dict(plain=lambda: step(tr_plain), apply=lambda: step(tr_apply, pose="apply"), train=lambda: step(tr_train, pose="train"),
               ray_grads=lambda: step(tr_rg, ray_grads=True))
    rounds = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            rounds[k].append(events(fn, args.steps, args.warmup))
    for k, v in rounds.items():
        res[k + "_ms"] = med(v)
        res[k + "_spread_ms"] = round(max(v) - min(v), 3)
        lines.append(f"{k:9s} ms/step per round: {' '.join(f'{x:.3f}' for x in v)}")
    res["train_minus_plain_ms"] = round(res["train_ms"] - res["plain_ms"], 3)
    res["train_minus_ray_grads_ms"] = round(res["train_ms"] - res["ray_grads_ms"], 3)
    res["grad_share_of_plain_1000"] = round(res["grad_us_1000"] * 1e-3 / res["plain_ms"], 5)
    res["max_abs_r"] = round(float(tr_train.pose.net.r.detach().abs().max()), 8)                  # the "train" leg did move its table
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/bench_zip_pose.py: path C pose refinement in the fused step, one MI355X, waymo.gin model, fp16 compute, 65 536 rays with\n")
            f.write("# depth targets; device events around back-to-back calls.  Kernels alone in us for tables of 1 / 200 / 1000 cameras; steps in ms:\n")
            f.write("# plain = no pose_net, apply / train = step(pose=...) on 1000 cameras, ray_grads = the plain step with ray_grads=True; the legs\n")
            f.write("# alternate within a round.  The summary line holds the medians.\n")
            for s in lines:
                f.write(s + "\n")
            f.write(line + "\n")


if __name__ == "__main__":
    main()
