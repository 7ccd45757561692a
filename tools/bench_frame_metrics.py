#!/usr/bin/env python3
"""Frame metrics (PSNR + SSIM of a rendered frame against its ground truth) at the path C frame size, 1920 x 1280, on one MI355X, for an
fp32 and a uint8 ground truth:

    (a) device       metrics.frame_metrics(pred, gt) on the resident tensors (snerf_frame_metrics: a tile launch and a finish launch) plus
                     the read of its five doubles; host clock around the call, which ends in that blocking read.  `a_events` is the same
                     call without the read, between device events.
    (b) host         what a user had to do before: .cpu().numpy() of the rendering and of the ground truth, then the metrics on the host.
                     The host arithmetic here is metrics.frame_metrics_host, OUR float64 numpy model STANDING IN for skimage + cv2 (neither
                     is installed); it is not skimage's timing.
    (c) copies       the two device-to-host copies of (b) alone.

The three alternate within a round; medians over --rounds rounds after --warmup.  GB/s = the bytes (a) must read (the prediction and the
ground truth once) over its time; the share of the 8 TB/s HBM peak is given for the event time.  Prints one JSON line per ground-truth
type; --out also writes the table to a text file."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

HBM_PEAK = 8.0e12


def host_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1280)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from snerf_amd import metrics, ops
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    assert args.rounds >= 1 and args.warmup >= 1
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    H, W = args.height, args.width
    g = torch.Generator(device=dev).manual_seed(0)
    gt8 = torch.randint(0, 256, (H, W, 3), generator=g, device=dev, dtype=torch.uint8)
    gtf = gt8.double().div(255.0).float()
    pred = (gtf + (torch.rand(H, W, 3, generator=g, device=dev) - 0.5) * (40. / 255.)).contiguous()
    out = torch.empty(1, 5, dtype=torch.float64, device=dev)
    ws = torch.empty(ops.frame_metrics_ws(1, H, W), dtype=torch.uint8, device=dev)
    lines = []
    for name, gt in (("fp32", gtf), ("uint8", gt8)):
        res = {}
        a = lambda: res.__setitem__("device", metrics.frame_metrics(pred, gt, out=out, ws=ws).cpu().numpy())
        a_ev = lambda: metrics.frame_metrics(pred, gt, out=out, ws=ws)
        c = lambda: (pred.cpu().numpy(), gt.cpu().numpy())
        b = lambda: res.__setitem__("host", metrics.frame_metrics_host(*c()))
        for _ in range(args.warmup):
            a(); a_ev(); b(); c()
        t = {"a": [], "a_events": [], "b": [], "c": []}
        for _ in range(args.rounds):
            t["a"].append(host_ms(a)); t["a_events"].append(event_ms(a_ev)); t["c"].append(host_ms(c)); t["b"].append(host_ms(b))
        med = {k: statistics.median(v) for k, v in t.items()}
        must_read = H * W * 3 * (4 + (4 if name == "fp32" else 1))
        line = {"shape": [H, W], "gt": name, "rounds": args.rounds,
                "a_device_with_read_ms": round(med["a"], 4), "a_device_events_ms": round(med["a_events"], 4),
                "b_host_route_ms": round(med["b"], 2), "c_two_copies_ms": round(med["c"], 3),
                "a_shorter_than_c": bool(med["a"] < med["c"]), "c_over_a": round(med["c"] / med["a"], 1), "b_over_a": round(med["b"] / med["a"], 1),
                "bytes_a_must_read": must_read, "a_with_read_GBps": round(must_read / (med["a"] * 1e-3) / 1e9, 1),
                "a_events_GBps": round(must_read / (med["a_events"] * 1e-3) / 1e9, 1),
                "a_events_fraction_of_hbm_peak": round(must_read / (med["a_events"] * 1e-3) / HBM_PEAK, 4),
                "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()},
                "device": dict(zip(ops.FRAME_METRIC_NAMES, res["device"][0].tolist())),
                "host_model": dict(zip(ops.FRAME_METRIC_NAMES, res["host"][0].tolist()))}
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/bench_frame_metrics.py: PSNR + SSIM of one 1920 x 1280 frame against its ground truth, one MI355X, medians in ms.\n")
            f.write("# a = metrics.frame_metrics on resident tensors + the read of its five doubles (host clock); a_events = the two launches alone\n")
            f.write("# (device events); b = .cpu().numpy() of both images + metrics.frame_metrics_host, our float64 numpy model standing in for\n")
            f.write("# skimage + cv2 (not installed: not their timing); c = the two device-to-host copies of b alone.  a, a_events, c, b alternate\n")
            f.write("# within a round.  GB/s: the bytes a must read (both images once) over its time.\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
