#!/usr/bin/env python3
"""Pose refinement (configs: pose_refine = True), ms per training step of whole loops on one MI355X at the shipped shape (bench.py's
model: 4096 rays, 64 + 128 samples, hidden 1024, bf16) on an ImageRayBatcher; wall clock over --steps steps after --warmup, one
device sync at the end of each timed loop (tools/bench_train_loop.py's convention):
    glue      the caller-side route: the image index read on the host, poses.LearnPose.forward + sample_utils.apply_pose_transform in
              torch, MipTrainer.step(ray_grads=True), autograd from the three ray gradients into the table, torch.optim.Adam
    fused     MipTrainer(pose_net=...).step(img_i=<device tensor>): snerf_pose_apply, the step, snerf_pose_grad, both fused Adams
    captured  MipTrainer(pose_net=...).capture(batcher=...) + replay(): all of it as one graph launch
`glue` and `fused` are timed alternately --rounds times in the same process (other work shares the host: the spread between rounds is
the noise a difference has to exceed); the reported figure is the median round.  --launches adds the kernel launches per step of the two
eager routes (torch.profiler, a separate untimed pass).  Prints one JSON line; --out also writes it, with the rounds, to a text file."""
import argparse
import json
import os
import statistics
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench_train_loop import _wall, path_a_scene


def launches_per_step(fn, steps=4):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.name and "Memset" not in e.name)
    return round(n / steps, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench
    from snerf_amd import poses, sample_utils as su
    from snerf_amd.trainer import MipTrainer
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    images, depths, cams, K = path_a_scene()
    N, n = images.shape[0], 4096
    sargs = types.SimpleNamespace(no_ndc=True, smooth_loss=False, near_far=True, N_rgb=n)
    mk_batcher = lambda: su.ImageRayBatcher(sargs, images, depths, cams, K, list(range(N)), 1.8, 110.0, camera_index=np.arange(N, dtype=np.float64),
                                            batch_n=n, device=dev)

    # glue: what a caller of MipTrainer.step(ray_grads=True) writes today
    b_glue, tr_glue = mk_batcher(), MipTrainer(bench.build_model("bf16", dev), lr=5e-4)
    net_glue = poses.LearnPose(N, True, False).to(dev)
    opt = torch.optim.Adam([{"params": [p for p in net_glue.parameters() if p.requires_grad], "lr": 1e-4}])

    def glue_step():
        rays, trgb, tdep, _, img, _ = b_glue.next()
        moved = su.apply_pose_transform(rays, net_glue(int(img), transform_only=True))      # (the host read of the image index)
        tr_glue.step(moved, trgb, tdep, None, ray_grads=True)
        opt.zero_grad()
        torch.autograd.backward([moved.directions, moved.viewdirs], list(tr_glue.last_ray_grads[1:]))
        opt.step()

    b_fused = mk_batcher()
    tr_fused = MipTrainer(bench.build_model("bf16", dev), lr=5e-4, pose_net=poses.LearnPose(N, True, False), pose_lr=1e-4)

    def fused_step():
        rays, trgb, tdep, _, img, _ = b_fused.next()
        tr_fused.step(rays, trgb, tdep, None, img_i=img)

    rounds = {"glue": [], "fused": [], "captured": []}
    for _ in range(args.rounds):
        rounds["glue"].append(_wall(glue_step, args.steps, args.warmup))
        rounds["fused"].append(_wall(fused_step, args.steps, args.warmup))
    res = {"steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "rays": n, "compute": "bf16"}
    if args.launches:
        res["glue_launches_per_step"] = launches_per_step(glue_step)
        res["fused_launches_per_step"] = launches_per_step(fused_step)
    b_cap = mk_batcher()
    tr_cap = MipTrainer(bench.build_model("bf16", dev), lr=5e-4, pose_net=poses.LearnPose(N, True, False), pose_lr=1e-4)
    tr_cap.capture(None, None, warmup=2, batcher=b_cap)
    for _ in range(args.rounds):
        rounds["captured"].append(_wall(tr_cap.replay, args.steps, args.warmup))
    for k, v in rounds.items():
        res[k + "_ms"] = statistics.median(v)
    res["fused_over_glue"] = round(res["fused_ms"] / res["glue_ms"], 4)
    moved = {k: float(t.pose.net.r.detach().abs().max()) for k, t in (("fused", tr_fused), ("captured", tr_cap))}
    moved["glue"] = float(net_glue.r.detach().abs().max())
    res["max_abs_r"] = {k: round(v, 6) for k, v in moved.items()}                            # every route did train its table
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/bench_pose_refine.py: ms per training step with pose refinement, one MI355X, 4096 rays, 64 + 128 samples, hidden 1024, bf16\n")
            f.write("# glue = host index read + torch pose transform + step(ray_grads=True) + autograd + torch.optim.Adam; fused = MipTrainer(pose_net=...).step;\n")
            f.write("# captured = the fused step replayed as one graph.  glue / fused alternate within a round; the summary line holds the medians.\n")
            for k, v in rounds.items():
                f.write(f"{k:9s} ms/step per round: {' '.join(f'{x:.3f}' for x in v)}\n")
            f.write(line + "\n")


if __name__ == "__main__":
    main()
