#!/usr/bin/env python3
"""Test-time pose refinement (s-nerf/eval.py:77-114, --test_refine_iter), ms per step of whole loops on one MI355X at the shipped shape
(bench.py's model: 4096 rays, 64 + 128 samples, hidden 1024, bf16) on an ImageRayBatcher; wall clock over --steps steps after --warmup,
one device sync at the end of each timed loop (tools/bench_pose_refine.py's convention):
    full          MipTrainer(pose_net=...).step(rays, target_rgb, target_depth, img_i=img): the fused training step with the learned pose
                  -- every weight gradient, the arena's Adam, the pose table's Adam (tools/bench_pose_refine.py's `fused` leg)
    frozen        the same call on MipTrainer(pose_net=..., freeze_model=True, pose_compose=True): the network held fixed -- the backward's
                  data path alone, snerf_pose_compose_apply / snerf_pose_compose_grad, the pose table's Adam only
    frozen_plain  the frozen trainer on the reference's own loop: RGB loss only (no depth target), so no gradient reaches the proposal level
The legs are timed alternately --rounds times in the same process (other work shares the host: the spread between the rounds of a leg is
the noise a difference has to exceed); the reported figure is the median round.  --legs full times the first leg alone (it uses nothing
this tool's other legs need, so the same file runs on a tree from before they existed: the parent's figure of the unchanged leg).
Prints one JSON line; --out appends it, with the rounds, to a text file under the heading --label."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--legs", default="full,frozen,frozen_plain")
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    legs = args.legs.split(",")
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
    init = torch.eye(4).repeat(N, 1, 1)
    init[:, :3] = torch.from_numpy(cams)
    fns, trainers = {}, {}

    def leg(name, depth, **kw):
        b = mk_batcher()
        tr = trainers[name] = MipTrainer(bench.build_model("bf16", dev), lr=5e-4, pose_net=poses.LearnPose(N, True, False, init), pose_lr=1e-4, **kw)

        def step():
            rays, trgb, tdep, _, img, _ = b.next()
            tr.step(rays, trgb, tdep if depth else None, None, img_i=img)
        fns[name] = step
    if "full" in legs:
        leg("full", True)
    if "frozen" in legs:
        leg("frozen", True, freeze_model=True, pose_compose=True)
    if "frozen_plain" in legs:
        leg("frozen_plain", False, freeze_model=True, pose_compose=True)
    rounds = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            rounds[k].append(_wall(fn, args.steps, args.warmup))
    res = {"label": args.label, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "rays": n, "compute": "bf16"}
    for k, v in rounds.items():
        res[k + "_ms"] = statistics.median(v)
        res[k + "_spread_ms"] = round(max(v) - min(v), 3)
    if "full" in rounds and "frozen" in rounds:
        res["frozen_over_full"] = round(res["frozen_ms"] / res["full_ms"], 4)
        res["full_minus_frozen_ms"] = round(res["full_ms"] - res["frozen_ms"], 3)
        res["largest_spread_ms"] = max(res["full_spread_ms"], res["frozen_spread_ms"])
    res["max_abs_r"] = {k: round(float(t.pose.net.r.detach().abs().max()), 6) for k, t in trainers.items()}      # every leg did train its table
    res["model_steps"] = {k: t.t for k, t in trainers.items()}                                                  # ... and only `full` its network
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(f"# {args.label}: tools/bench_pose_test_refine.py --legs {args.legs}, ms per step, one MI355X, 4096 rays, 64 + 128 samples, hidden 1024, bf16\n")
            for k, v in rounds.items():
                f.write(f"{k:13s} ms/step per round: {' '.join(f'{x:.3f}' for x in v)}\n")
            f.write(line + "\n")


if __name__ == "__main__":
    main()
