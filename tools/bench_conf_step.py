#!/usr/bin/env python3
"""Learned depth confidence (configs: depth_conf = True, precompute_conf = True), ms per training step of whole loops on one MI355X at
the shipped shape (bench.py's model: 4096 rays, 64 + 128 samples, hidden 1024, bf16) on an ImageRayBatcher; wall clock over --steps
steps after --warmup, one device sync at the end of each timed loop (tools/bench_train_loop.py's convention):
    given     MipTrainer.step(conf=<the batcher's gathered confidence map>): a constant per-ray confidence, the route there was before
    table     MipTrainer(conf_net=, conf_maps=).step(img_i=<device tensor>, sel_coords=): snerf_conf_apply, the g_conf loss tail,
              snerf_conf_grad, the model's Adam and the table's
    captured  MipTrainer(conf_net=, conf_maps=).capture(batcher=...) + replay(): all of it as one graph launch
`given` and `table` are timed alternately --rounds times in the same process (other work shares the host: the spread between rounds is
the noise a difference has to exceed); the reported figure is the median round.  The three launches the table adds or changes are
timed on their own with device events (us, mean of --reps back-to-back calls on the last batch): conf_apply, the tail with and
without g_conf, conf_grad (its two kernels) and the table's Adam.  Prints one JSON line; --out also writes it, with the rounds, to a
text file."""
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

MODES = ["rgb", "ssim", "depth"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench
    from snerf_amd import confidence, ops, sample_utils as su
    from snerf_amd.trainer import MipTrainer
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    images, depths, cams, K = path_a_scene()
    N, H, W = images.shape[:3]
    n = 4096
    rng = np.random.default_rng(1)
    all_maps = [{m: torch.from_numpy(rng.random(H * W, dtype=np.float32)) for m in MODES} for _ in range(N)]
    sky = torch.from_numpy(rng.random((N, H, W)) < 0.2)
    fixed = np.stack([np.mean([d[m].numpy() for m in MODES], 0).reshape(H, W) for d in all_maps])      # the table's mix at lambdas = 0
    sargs = types.SimpleNamespace(no_ndc=True, smooth_loss=False, near_far=True, N_rgb=n)
    mk_batcher = lambda extras=None: su.ImageRayBatcher(sargs, images, depths, cams, K, list(range(N)), 1.8, 110.0,
                                                        camera_index=np.arange(N, dtype=np.float64), batch_n=n, extras=extras, device=dev)
    mk_maps = lambda: confidence.ConfidenceMaps(all_maps, list(range(N)), N, H, W, skymask=sky)

    b_given, tr_given = mk_batcher([fixed]), MipTrainer(bench.build_model("bf16", dev), lr=5e-4)

    def given_step():
        rays, trgb, tdep, _, _, ex = b_given.next()
        tr_given.step(rays, trgb, tdep, ex[0])

    b_table = mk_batcher()
    tr_table = MipTrainer(bench.build_model("bf16", dev), lr=5e-4, conf_net=confidence.Confidence(MODES, N), conf_maps=mk_maps())
    last = {}

    def table_step():
        rays, trgb, tdep, sel, img, _ = b_table.next()
        _, outs = tr_table.step(rays, trgb, tdep, img_i=img, sel_coords=sel)
        last.update(outs=outs, trgb=trgb, tdep=tdep, sel=sel, img=img)

    rounds = {"given": [], "table": [], "captured": []}
    for _ in range(args.rounds):
        rounds["given"].append(_wall(given_step, args.steps, args.warmup))
        rounds["table"].append(_wall(table_step, args.steps, args.warmup))
    res = {"steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "rays": n, "compute": "bf16", "modes": len(MODES)}

    # the launches on their own, on the last batch of the table route
    cf, outs = tr_table.conf, last["outs"]
    mp = cf.maps
    dist0, s0, w0, rgb1, dist1, s1, w1 = outs[0], outs[2], outs[3], outs[4], outs[5], outs[7], outs[8]
    conf = cf.apply(last["img"], last["sel"])
    prop = tr_table.proposal_loss
    tail = lambda **kw: (lambda: ops.mip_loss_tail_masked(
        rgb1, last["trgb"], dist1, dist0, last["tdep"], conf, s1 if prop else None, w1 if prop else None, s0 if prop else None,
        w0 if prop else None, tr_table.disparity_depth, tr_table.depth_lambda, tr_table.coarse_depth_mult, tr_table.proposal_lambda, **kw))
    g_conf = tail(want_g_conf=True)()[6]
    scratch = torch.zeros_like(cf.g)
    res["launch_us"] = {
        "conf_apply": _events(lambda: cf.apply(last["img"], last["sel"]), args.reps),
        "tail_plain": _events(lambda: ops.mip_loss_tail(rgb1, last["trgb"], dist1, dist0, last["tdep"], conf, s1 if prop else None,
                                                        w1 if prop else None, s0 if prop else None, w0 if prop else None,
                                                        tr_table.disparity_depth, tr_table.depth_lambda, tr_table.coarse_depth_mult,
                                                        tr_table.proposal_lambda), args.reps),
        "tail_masked": _events(tail(), args.reps),
        "tail_g_conf": _events(tail(want_g_conf=True), args.reps),
        "conf_grad": _events(lambda: ops.conf_grad(mp.maps, mp.slot_of_image, cf.net.lambdas.data, mp.sky, last["img"], last["sel"], g_conf, scratch,
                                                   ws=cf.workspace(n)), args.reps),
    }

    b_cap = mk_batcher()
    tr_cap = MipTrainer(bench.build_model("bf16", dev), lr=5e-4, conf_net=confidence.Confidence(MODES, N), conf_maps=mk_maps())
    tr_cap.capture(None, None, warmup=2, batcher=b_cap)
    for _ in range(args.rounds):
        rounds["captured"].append(_wall(tr_cap.replay, args.steps, args.warmup))
    for k, v in rounds.items():
        res[k + "_ms"] = statistics.median(v)
    res["table_over_given"] = round(res["table_ms"] / res["given_ms"], 4)
    res["max_abs_lambda"] = {k: round(float(t.conf.flat.abs().max()), 6) for k, t in (("table", tr_table), ("captured", tr_cap))}   # both trained
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/bench_conf_step.py: ms per training step with the learned depth confidence, one MI355X, 4096 rays, 64 + 128 samples, hidden 1024, bf16\n")
            f.write("# given = step(conf=<gathered constant map>); table = MipTrainer(conf_net=, conf_maps=).step: conf_apply + g_conf tail + conf_grad + table Adam;\n")
            f.write("# captured = the table step replayed as one graph.  given / table alternate within a round; the summary line holds the medians and the\n")
            f.write("# launches' own durations in us (device events, back-to-back calls).\n")
            for k, v in rounds.items():
                f.write(f"{k:9s} ms/step per round: {' '.join(f'{x:.3f}' for x in v)}\n")
            f.write(line + "\n")


if __name__ == "__main__":
    main()
