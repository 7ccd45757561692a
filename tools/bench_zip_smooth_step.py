#!/usr/bin/env python3
"""The patch terms (d_smo, s_smo) inside the fused path C step: ms per ZipTrainer step on one MI355X at the shipped shape (waymo.gin
model with the semantic head, fp16 compute, 65 536 rows of which the first 256 * 8 * 8 are patches, 19 classes), timed with device events
around --steps back-to-back steps after --warmup:
    off    ZipTrainer.step on the batch with its depth, semantic and mask targets, no patch arguments: every row is a pixel row
    on     the same step with n_patch = 256, patch_size = 8 and the batch's mask on the patch rows
    eager  the two terms written as eager torch ops in fp32, forward and backward, on the same tensors (the step's target colours, NeRF-level
           depth and class probabilities, the mask): what a caller outside the fused step would run per step
    op     ops.zip_smooth_loss alone (its memset, count, main and finish launches), gradients accumulated
off / on alternate --rounds times in the same process (other work shares the host: the spread between rounds is the noise a difference
has to exceed); the reported figures are the median rounds.  Prints one JSON line; --out also writes it, with the rounds, to a text file."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

ROWS_ALL, P_SZ, N_PATCH = 65536, 8, 256


def events_ms(fn, n, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b) / n, 4)


def eager_terms(rgb, depth, sem, mask, P, p, d_mult, s_mult):
    """train.py:283-293 as plain torch ops on [P,p,p,.] views -> d_smo + s_smo"""
    shape = (P, p, p)
    rgb, ok = rgb.reshape(*shape, 3), ~(mask.reshape(shape) > 0)
    ok_x, ok_y = ok[:, :, :-1] & ok[:, :, 1:], ok[:, :-1] & ok[:, 1:]
    w_x, w_y = torch.exp(-(rgb[:, :, :-1] - rgb[:, :, 1:]).abs().mean(-1)), torch.exp(-(rgb[:, :-1] - rgb[:, 1:]).abs().mean(-1))

    def term(z, eps):
        z = z / (z.mean((1, 2), keepdim=True) + eps)
        return ((z[:, :, :-1] - z[:, :, 1:]).abs().sum(-1) * w_x)[ok_x].mean() + ((z[:, :-1] - z[:, 1:]).abs().sum(-1) * w_y)[ok_y].mean()
    return torch.nan_to_num(d_mult * term(1 / (depth.reshape(*shape, 1) + 1e-5), 1e-7)) + torch.nan_to_num(s_mult * term(sem.reshape(*shape, -1), 1e-5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from snerf_amd import ops, zipnerf
    from snerf_amd.trainer import ZipTrainer
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    N, H, W = 8, 1280, 1920
    rng = np.random.default_rng(1)
    images = rng.integers(0, 256, size=(N, H, W, 3), dtype=np.uint8)
    masks = (rng.random((N, H, W), dtype=np.float32) < 0.3).astype(np.float32)
    K = np.array([[2050.0, 0.0, 960.0], [0.0, 2050.0, 640.0], [0.0, 0.0, 1.0]])
    pixtocams = np.tile(np.linalg.inv(K).astype(np.float32), (N, 1, 1))
    c2w = np.tile(np.eye(4, dtype=np.float32)[:3], (N, 1, 1))
    c2w[:, :, 3] = rng.normal(0, 0.03, (N, 3))
    depths = (rng.random((N, H, W), dtype=np.float32) * 0.8).astype(np.float32)
    labels = rng.integers(0, 19, size=(N, H, W)).astype(np.int32)
    batcher = zipnerf.PatchRayBatcher(images, pixtocams, c2w, 0.02, 100.0, P_SZ, depths=depths, semantics=labels, masks=masks, batch_size=ROWS_ALL,
                                      device=dev)
    assert batcher.n_patch == N_PATCH
    bt = batcher.next()
    rows = batcher.n_patch_rows
    # depth and semantic targets in both legs, as a waymo run has them: the gradient paths of the rendered depth and class probabilities exist
    # with and without the patch terms
    valid = (bt["mask"] == 0).float()
    tg = dict(lossmult=valid, depth=bt["depth"], depth_mask=valid * (bt["depth"] > 0.1), complete_mask=1 - valid, semantic=bt["semantic"], semantic_mask=valid)
    torch.manual_seed(0)
    m = zipnerf.Model(config=None, raydist_fn='power_transformation', opaque_background=True, compute="fp16", table_dtype="ref", init_std=0.1,
                      use_semantic=True, device=dev)
    tr = ZipTrainer(m, lr=1e-2)
    last = {}

    def off():
        tr.step(bt, bt["rgb"], train_frac=0.5, rand=True, targets=tg)

    def on():
        _, levels = tr.step(bt, bt["rgb"], train_frac=0.5, rand=True, targets=tg, n_patch=N_PATCH, patch_size=P_SZ, patch_mask=bt["mask"][:rows])
        last["fin"] = levels[2]

    rounds = {"off": [], "on": []}
    for _ in range(args.rounds):
        rounds["off"].append(events_ms(off, args.steps, args.warmup))
        rounds["on"].append(events_ms(on, args.steps, args.warmup))
    fin = last["fin"]
    depth, sem, rgb, mask = fin["depth"][:rows].detach().clone(), fin["semantic"][:rows].detach().clone(), bt["rgb"][:rows], bt["mask"][:rows]
    C = sem.shape[1]

    def eager():
        d, s = depth.requires_grad_(True), sem.requires_grad_(True)
        d.grad = s.grad = None
        eager_terms(rgb, d, s, mask, N_PATCH, P_SZ, tr.d_smo_mult, tr.s_smo_mult).backward()

    g_d, g_s = torch.zeros(rows, device=dev), torch.zeros(rows, C, device=dev)
    out, ws = torch.zeros(4, device=dev), torch.empty(ops.zip_smooth_loss_ws(N_PATCH), dtype=torch.float64, device=dev)
    op = lambda: ops.zip_smooth_loss(rgb, depth.detach(), sem.detach(), mask, N_PATCH, P_SZ, d_mult=tr.d_smo_mult, s_mult=tr.s_smo_mult,
                                     grad_mult=tr.loss_scale, out=out, g_depth=g_d, g_sem=g_s, accumulate=True, ws=ws)
    res = {"steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "rows": ROWS_ALL, "patches": N_PATCH, "patch_size": P_SZ, "classes": C,
           "compute": "fp16", "off_ms": statistics.median(rounds["off"]), "on_ms": statistics.median(rounds["on"]),
           "eager_terms_ms": events_ms(eager, args.reps, 10), "op_ms": events_ms(op, args.reps, 10)}
    with torch.enable_grad():
        want = float(eager_terms(rgb, depth.detach(), sem.detach(), mask, N_PATCH, P_SZ, tr.d_smo_mult, tr.s_smo_mult))
    res.update(added_ms=round(res["on_ms"] - res["off_ms"], 4), on_over_off=round(res["on_ms"] / res["off_ms"], 4),
               valid_edges=[int(out[2]), int(out[3])], terms_op=round(float(out[0]) + float(out[1]), 8), terms_eager=round(want, 8))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/bench_zip_smooth_step.py: ms per ZipTrainer step with the patch terms (d_smo, s_smo), one MI355X, waymo.gin model with the\n")
            f.write("# semantic head, fp16 compute, 65 536 rows with depth, semantic and mask targets; device events around back-to-back steps.\n")
            f.write("# off = no patch arguments; on = the first 256 * 8 * 8 rows as patches (trainer-owned target masks, snerf_zip_smooth_loss behind the\n")
            f.write("# loss tail); off / on alternate within a round.  The summary line holds the medians, the two terms as eager torch ops (forward +\n")
            f.write("# backward, fp32) and the op alone (memset, count, main and finish launches), in ms.\n")
            for k, v in rounds.items():
                f.write(f"{k:4s} ms/step per round: {' '.join(f'{x:.3f}' for x in v)}\n")
            f.write(line + "\n")


if __name__ == "__main__":
    main()
