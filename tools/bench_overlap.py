#!/usr/bin/env python3
"""The pairwise overlap statistics of the instance masks of one frame (`snerf_fg_overlap`, snerf_amd.foreground.overlap_stats) at the path C
frame size on one MI355X, against the torch formulation of the same numbers on the device, in the same process.

    kernel   snerf_fg_overlap alone, adding into one zeroed [N,N,3] int64 table
    call     foreground.overlap_stats: the table's torch.zeros + the launch (what occlusion_order pays)
    torch    per pair a < b: idx = ((m_a > 0) & (m_b > 0)).nonzero(); (len, idx[:, 0].sum(), idx[:, 1].sum()), stacked on the device

The masks: --masks boxes, each 2-10 % of the frame, laid out by a seeded generator so that a few of them overlap (the run prints
how many pairs do).  Device events around --inner back-to-back calls (the kernel is tens of microseconds: one call per event pair would
time the launch), medians over --rounds rounds after --warmup, the legs alternating within a round, every timed batch after an untimed
call of the same leg.  `gbytes_per_s` = one pass over the N masks (N * 3 * H * W bytes, what the kernel must read) over the kernel's
time; the masks of one frame (59 MB at the defaults) fit the 256 MiB Infinity Cache, so repeated calls need not come from HBM.  The
results of the three legs are compared; a difference, or any HIP error, ends the run with a non-zero status.  Run it under `timeout`.
Prints one JSON line; --out also writes it to a text file."""
import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from bench_mesh_trace import event_ms


def box_masks(n, H, W, seed):
    """n [H,W,3] uint8 masks, one filled box each, 2-10 % of the frame, placed in the lower three quarters of the frame so that a few overlap"""
    rng = np.random.default_rng(seed)
    masks = []
    for _ in range(n):
        share = rng.uniform(.02, .10)
        aspect = rng.uniform(1.2, 2.5)
        h = int(round((share * H * W / aspect) ** .5))
        w = int(round(h * aspect))
        y0 = int(rng.integers(H // 4, max(H // 4 + 1, H - h)))
        x0 = int(rng.integers(0, max(1, W - w)))
        m = np.zeros((H, W, 3), dtype=np.uint8)
        m[y0:y0 + h, x0:x0 + w] = 255
        masks.append(m)
    return masks


def torch_stats(masks):
    N = len(masks)
    out = torch.zeros(N, N, 3, dtype=torch.int64, device=masks[0].device)
    for a in range(N):
        for b in range(a + 1, N):
            idx = ((masks[a] > 0) & (masks[b] > 0)).nonzero()
            out[a, b, 0] = idx.shape[0]
            out[a, b, 1:] = idx[:, :2].sum(dim=0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1280)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--masks", type=int, default=8)
    ap.add_argument("--seed", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from snerf_amd import _lib, foreground
    from snerf_amd.ops import _p, _stream
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    torch.cuda.set_device(0)
    H, W, N = args.height, args.width, args.masks
    masks = [torch.from_numpy(m).cuda() for m in box_masks(N, H, W, args.seed)]
    ptrs = (ctypes.c_void_p * N)(*[m.data_ptr() for m in masks])
    table = torch.zeros(N, N, 3, dtype=torch.int64, device="cuda")

    def kernel():
        for _ in range(args.inner):
            _lib.call("snerf_fg_overlap", ptrs, N, H, W, _p(table), _stream())

    def call():
        for _ in range(args.inner):
            foreground.overlap_stats(masks)

    legs = {"kernel": (kernel, args.inner), "call": (call, args.inner), "torch": (lambda: torch_stats(masks), 1)}
    want = torch_stats(masks)
    got = foreground.overlap_stats(masks)
    torch.cuda.synchronize()
    if not torch.equal(got, want):
        raise SystemExit("bench_overlap: snerf_fg_overlap and the torch formulation disagree")
    for _ in range(args.warmup):
        for fn, _ in legs.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, (fn, n) in legs.items():
            fn()                                                                # untimed: the timed batch finds its own warm state
            t[k].append(event_ms(fn) / n)
    launches = (args.warmup + 2 * args.rounds) * args.inner
    if not torch.equal(table, want * launches):                                 # every launch of the kernel leg added the same numbers
        raise SystemExit("bench_overlap: the accumulated table is not launches x the statistics")
    med = {k: statistics.median(v) for k, v in t.items()}
    nbytes = N * 3 * H * W
    line = {"shape": [H, W], "masks": N, "mask_shares": [round(float((m[..., 0] > 0).float().mean()), 4) for m in masks],
            "overlapping_pairs": int((want[..., 0] > 0).sum()), "rounds": args.rounds, "inner": args.inner,
            "ms": {k: round(v, 5) for k, v in med.items()}, "min_max_ms": {k: [round(min(v), 5), round(max(v), 5)] for k, v in t.items()},
            "mask_bytes": nbytes, "kernel_gbytes_per_s": round(nbytes / (med["kernel"] * 1e-3) / 1e9, 1),
            "torch_over_kernel": round(med["torch"] / med["kernel"], 1), "torch_over_call": round(med["torch"] / med["call"], 1)}
    out = json.dumps(line)
    print(out, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/bench_overlap.py: pairwise overlap statistics of the instance masks of one frame (snerf_fg_overlap), one MI355X, device events\n")
            f.write("# around `inner` back-to-back calls, medians in ms per call.  kernel = the entry alone; call = foreground.overlap_stats (torch.zeros + the\n")
            f.write("# launch); torch = per pair ((m_a > 0) & (m_b > 0)).nonzero() sums on the device.  kernel_gbytes_per_s = one pass over the masks / kernel.\n")
            f.write(out + "\n")


if __name__ == "__main__":
    try:
        main()
    except SystemExit:
        raise
    except BaseException as e:                                                  # a HIP error surfaces as an exception of torch or of _lib.call
        print(f"bench_overlap: {type(e).__name__}: {e}", file=sys.stderr, flush=True)
        sys.exit(1)
