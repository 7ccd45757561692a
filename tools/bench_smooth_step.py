#!/usr/bin/env python3
"""The edge-aware smooth loss inside the fused step (configs: smooth_loss = True), ms per training step of whole loops on one MI355X at
the shipped shape (bench.py's model: 64 + 128 samples, hidden 1024, bf16); wall clock over --steps steps after --warmup, one device
sync at the end of each timed loop (tools/bench_train_loop.py's convention):
    plain     ImageRayBatcher of 4096 rays + MipTrainer.step: the step there was before the term
    rays      ImageRayBatcher of 4096 + 8 * 64 = 4608 rays + the same step: what the patch rays cost as rays
    smooth    PatchRayBatcher (4096 pixels + 8 patches of 8 x 8, a sky extra) + MipTrainer(smooth_patch_sz=8).step(n_rgb=, smooth_sky=)
    captured  the smooth step captured with its batcher and replayed as one graph launch
plain / rays / smooth are timed alternately --rounds times in the same process (other work shares the host: the spread between rounds
is the noise a difference has to exceed); the reported figure is the median round.  The launches the term adds are timed on their own
with device events (us, mean of --reps back-to-back calls): the two batcher draws and ops.smooth_loss (its two kernels).  Prints one
JSON line; --out also writes it, with the rounds, to a text file."""
import argparse
import json
import os
import statistics
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench_train_loop import _events, _wall, path_a_scene

N_RGB, N_PATCH, P_SZ = 4096, 8, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench
    from snerf_amd import ops, sample_utils as su
    from snerf_amd.trainer import MipTrainer
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    images, depths, cams, K = path_a_scene()
    N, H, W = images.shape[:3]
    sky = (np.random.default_rng(1).random((N, H, W)) < 0.2).astype(np.float32)
    mk = lambda cls, n, smooth, **kw: cls(types.SimpleNamespace(no_ndc=True, smooth_loss=smooth, near_far=True, N_rgb=n, N_patch=N_PATCH, patch_sz=P_SZ),
                                          images, depths, cams, K, list(range(N)), 1.8, 110.0, camera_index=np.arange(N, dtype=np.float64),
                                          batch_n=n, extras=[sky], device=dev, **kw)
    n_all = N_RGB + N_PATCH * P_SZ * P_SZ

    def plain_route(n):
        b, tr = mk(su.ImageRayBatcher, n, False), MipTrainer(bench.build_model("bf16", dev), lr=5e-4)

        def step():
            rays, trgb, tdep, _, _, _ = b.next()
            tr.step(rays, trgb, tdep)
        return b, tr, step

    b_plain, _, plain_step = plain_route(N_RGB)
    _, _, rays_step = plain_route(n_all)
    b_smooth = mk(su.PatchRayBatcher, N_RGB, True)
    tr_smooth = MipTrainer(bench.build_model("bf16", dev), lr=5e-4, smooth_patch_sz=P_SZ, smooth_lambda=0.1)
    last = {}

    def smooth_step():
        rays, trgb, tdep, _, _, ex = b_smooth.next()
        _, outs = tr_smooth.step(rays, trgb, tdep, n_rgb=b_smooth.n_rgb_rows, smooth_sky=ex[0][b_smooth.n_rgb_rows:])
        last.update(outs=outs, trgb=trgb, sky=ex[0])

    rounds = {"plain": [], "rays": [], "smooth": [], "captured": []}
    for _ in range(args.rounds):
        rounds["plain"].append(_wall(plain_step, args.steps, args.warmup))
        rounds["rays"].append(_wall(rays_step, args.steps, args.warmup))
        rounds["smooth"].append(_wall(smooth_step, args.steps, args.warmup))
    res = {"steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "rays": N_RGB, "patches": N_PATCH, "patch_sz": P_SZ, "compute": "bf16"}

    dist1 = last["outs"][5].reshape(-1)
    g = torch.zeros_like(dist1)
    ws = torch.empty(ops.smooth_loss_ws(N_PATCH), dtype=torch.float64, device=dev)
    out = torch.empty(3, dtype=torch.float32, device=dev)
    buf_p, buf_s = b_plain.buffers(), b_smooth.buffers()
    res["launch_us"] = {
        "image_batch": _events(lambda: b_plain.next_into(buf_p), args.reps),
        "image_patch_batch": _events(lambda: b_smooth.next_into(buf_s), args.reps),
        "smooth_loss": _events(lambda: ops.smooth_loss(last["trgb"][N_RGB:], dist1[N_RGB:], last["sky"][N_RGB:], N_PATCH, P_SZ, 0.1, out=out,
                                                       g_dist=g[N_RGB:], accumulate=True, ws=ws), args.reps),
    }
    res["smooth_loss_value"] = round(float(tr_smooth.last_smooth_loss), 6)

    b_cap = mk(su.PatchRayBatcher, N_RGB, True)
    tr_cap = MipTrainer(bench.build_model("bf16", dev), lr=5e-4, smooth_patch_sz=P_SZ, smooth_lambda=0.1)
    tr_cap.capture(None, None, warmup=2, batcher=b_cap, smooth_sky_extra=0)
    for _ in range(args.rounds):
        rounds["captured"].append(_wall(tr_cap.replay, args.steps, args.warmup))
    for k, v in rounds.items():
        res[k + "_ms"] = statistics.median(v)
    res["smooth_over_plain"] = round(res["smooth_ms"] / res["plain_ms"], 4)
    res["smooth_over_rays"] = round(res["smooth_ms"] / res["rays_ms"], 4)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/bench_smooth_step.py: ms per training step with the edge-aware smooth loss, one MI355X, 64 + 128 samples, hidden 1024, bf16\n")
            f.write("# plain = 4096 rays, no term (the step there was); rays = 4608 rays, no term; smooth = 4096 pixels + 8 patches of 8 x 8 with the term\n")
            f.write("# (PatchRayBatcher, trainer-owned depth targets, snerf_smooth_loss + its finish launch); captured = the smooth step replayed as one graph.\n")
            f.write("# plain / rays / smooth alternate within a round; the summary line holds the medians and the launches' own durations in us\n")
            f.write("# (device events, back-to-back calls).\n")
            for k, v in rounds.items():
                f.write(f"{k:9s} ms/step per round: {' '.join(f'{x:.3f}' for x in v)}\n")
            f.write(line + "\n")


if __name__ == "__main__":
    main()
