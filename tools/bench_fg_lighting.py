#!/usr/bin/env python3
"""The lighting match of one instance on one frame (`snerf_fg_lighting`, snerf_amd.foreground.handle_lighting) at the path C frame size
on one MI355X, next to the least any host route pays on the same machine, in the same process.

    lighting   foreground.handle_lighting(frame, mask, stats=preallocated): the init launch and the three kernels, the whole frame rewritten
    masked     the same with keep_background=True: only the instance's pixels are written
    copies     frame.cpu(), then .cuda() of that host array, with their syncs: the two frame copies any host route (cv2 on the host between
               two pastes) needs per instance.  OpenCV itself is not timed (it is not installed): this is a LOWER bound for that route.

The mask: one ellipse of about --share of the frame.  lighting / masked: device events around --inner back-to-back calls (tens of
microseconds each: one call per event pair would time the launch), per-call medians over --rounds rounds after --warmup, the legs
alternating within a round, every timed batch after an untimed one.  The calls of a batch work on the frame the previous call left
(the conversion is in place); the work per call does not depend on the content.  copies: a host clock around one round trip, ending
in a synchronise.  `lighting_gbytes_per_s` = the bytes the three passes must move (frame + mask read twice, both once more inside the
expanded box, the frame written once) over the call's time; one frame and one mask fit the 256 MiB Infinity Cache, so this is no HBM
rate.  Before timing, one call is compared with the numpy model; a difference, or any HIP error, ends the run with a non-zero status.
Run it under `timeout`.  Prints one JSON line; --out also writes it to a text file."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from bench_mesh_trace import event_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1280)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--share", type=float, default=.08)
    ap.add_argument("--seed", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from snerf_amd import foreground
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    torch.cuda.set_device(0)
    H, W = args.height, args.width
    rng = np.random.default_rng(args.seed)
    frame_h = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    yy, xx = np.mgrid[:H, :W]
    ry = (args.share * H * W / (1.6 * np.pi)) ** .5
    mask_h = ((((yy - .6 * H) / ry) ** 2 + ((xx - .45 * W) / (1.6 * ry)) ** 2 <= 1)[..., None] * np.uint8(255)).repeat(3, -1)
    frame, mask = torch.from_numpy(frame_h).cuda(), torch.from_numpy(mask_h).cuda()
    stats = torch.empty(9, dtype=torch.int64, device="cuda")

    for keep in (False, True):
        got = foreground.handle_lighting(frame.clone(), mask, keep_background=keep, stats=stats).cpu().numpy()
        if not np.array_equal(got, foreground.handle_lighting_host(frame_h, mask_h, keep)) or \
                not np.array_equal(stats.cpu().numpy(), foreground.lighting_stats_host(frame_h, mask_h)):
            raise SystemExit("bench_fg_lighting: snerf_fg_lighting and the numpy model disagree")
    s = foreground.lighting_stats_host(frame_h, mask_h)
    i_len, j_len = int(s[1] - s[0]), int(s[3] - s[2])
    box = (min(H - 1, int(s[1]) + i_len // 2 + 1) - max(0, int(s[0]) - i_len // 2 - 1) + 1) * \
          (min(W - 1, int(s[3]) + j_len // 2 + 1) - max(0, int(s[2]) - j_len // 2 - 1) + 1)

    work = frame.clone()

    def lighting(keep):
        for _ in range(args.inner):
            foreground.handle_lighting(work, mask, keep_background=keep, stats=stats)

    def copies():
        t0 = time.perf_counter()
        host = work.cpu()                                                        # (synchronises)
        back = host.cuda()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, back

    legs = {"lighting": lambda: lighting(False), "masked": lambda: lighting(True)}
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
        copies()
    torch.cuda.synchronize()
    t = {k: [] for k in list(legs) + ["copies"]}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            work.copy_(frame)
            fn()                                                                # untimed: the timed batch finds its own warm state
            t[k].append(event_ms(fn) / args.inner)
        copies()
        t["copies"].append(copies()[0])
    med = {k: statistics.median(v) for k, v in t.items()}
    nbytes = 3 * H * W * (2 + 2 + 1) + 2 * 3 * box                              # passes 1 and 3: frame + mask; pass 3 writes the frame; pass 2: the box rows' share
    line = {"shape": [H, W], "mask_share": round(float(s[4]) / (H * W), 4), "box_share": round(box / (H * W), 4), "rounds": args.rounds,
            "inner": args.inner, "ms": {k: round(v, 5) for k, v in med.items()},
            "min_max_ms": {k: [round(min(v), 5), round(max(v), 5)] for k, v in t.items()}, "lighting_bytes": nbytes,
            "lighting_gbytes_per_s": round(nbytes / (med["lighting"] * 1e-3) / 1e9, 1),
            "copies_over_lighting": round(med["copies"] / med["lighting"], 1)}
    out = json.dumps(line)
    print(out, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/bench_fg_lighting.py: the lighting match of one instance on one frame (snerf_fg_lighting), one MI355X.  lighting / masked = device\n")
            f.write("# events around `inner` back-to-back foreground.handle_lighting calls (keep_background False / True), medians in ms per call; copies =\n")
            f.write("# frame.cpu() + .cuda() with their syncs on a host clock: the two frame copies a host route needs per instance, without its OpenCV\n")
            f.write("# (not installed, not timed): a lower bound.  lighting_gbytes_per_s = the bytes the three passes must move / lighting (cache-resident).\n")
            f.write(out + "\n")


if __name__ == "__main__":
    try:
        main()
    except SystemExit:
        raise
    except BaseException as e:                                                  # a HIP error surfaces as an exception of torch or of _lib.call
        print(f"bench_fg_lighting: {type(e).__name__}: {e}", file=sys.stderr, flush=True)
        sys.exit(1)
