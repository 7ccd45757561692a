#!/usr/bin/env python3
"""Path B train step, three ways, on one MI355X: the autograd loop (`loop`: exactly bench.py:path_b_leg's train() -- render_rays under
autograd, a dozen torch ops of loss, torch.optim.Adam), trainer.ClassicTrainer.step (`step`) and its captured form (`replay`).
64 coarse + 128 importance samples, two NeRF 8 x 256 networks, bf16; 1024, 4096 and 32 768 rays.

Timing: device events around back-to-back calls after a warm-up of every shape and variant; windows of at least --window seconds
(the call count per window is calibrated per variant and size); --rounds rounds with the variants alternating inside each round;
medians and per-round values.  One JSON line, then the rounds:
    python tools/bench_classic_trainer.py --out profiles/r20_a_classic_trainer.txt [--launches DIR]

Launches per step, as tools/per_step_launches.py counts them (two kernel traces of different step counts, differenced), in runs of
their own -- tracing slows the host, so never together with the timing:
    for v in loop step replay; do for k in 2 8; do
      rocprofv3 --kernel-trace --output-format csv -d DIR/${v}_$k -o b -- python tools/bench_classic_trainer.py --trace $v --rays 1024 --steps $k
    done; done
and `--launches DIR` then adds the counts (and the kernel time per step of those traces) to the JSON line; with `--sizes ""` nothing is
timed and the counts alone are APPENDED to --out as a second JSON line (reads the traces: needs no GPU)."""
import argparse
import glob
import json
import os
import re
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VARIANTS = ("loop", "step", "replay")
N_SAMPLES, N_IMPORTANCE = 64, 128


def make(variant, n_rays, device, compute="bf16"):
    """-> a callable that runs one train step of `variant` on a fixed batch of n_rays (networks, rays and targets as bench.py:path_b_leg)"""
    from snerf_amd import classic
    from snerf_amd.trainer import ClassicTrainer
    torch.manual_seed(0)
    mk = lambda: classic.NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=4, skips=[4], use_viewdirs=True, compute=compute, device=device)
    coarse, fine = mk(), mk()
    g = torch.Generator().manual_seed(1)
    N = n_rays
    d = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)
    o = torch.randn(N, 3, generator=g) * 0.1 + torch.tensor([0.0, 0.0, 4.0])
    rays = torch.cat([o, -d, torch.full((N, 1), 2.0), torch.full((N, 1), 6.0), -d], -1).to(device)
    tgt = torch.rand(N, 3, generator=g).to(device)
    if variant == "loop":
        embed_fn, _ = classic.get_embedder(10, 0)
        embeddirs_fn, _ = classic.get_embedder(4, 0)
        q = classic.make_network_query_fn(embed_fn, embeddirs_fn, netchunk=1 << 30)
        opt = torch.optim.Adam(list(coarse.parameters()) + list(fine.parameters()), lr=5e-4)
        fwd = lambda: classic.render_rays(rays, coarse, q, N_SAMPLES, perturb=1.0, N_importance=N_IMPORTANCE, network_fine=fine, white_bkgd=False,
                                          raw_noise_std=0.0)

        def train():
            opt.zero_grad(set_to_none=False)
            r = fwd()
            loss = ((r["rgb_map"] - tgt) ** 2).mean() + ((r["rgb0"] - tgt) ** 2).mean()
            loss.backward()
            opt.step()
            coarse.arena.bump(); fine.arena.bump()
        return train
    tr = ClassicTrainer(coarse, None, N_SAMPLES, N_IMPORTANCE, fine, lr=5e-4, perturb=1.0, white_bkgd=False, raw_noise_std=0.0)
    if variant == "step":
        return lambda: tr.step(rays, tgt)
    tr.capture(rays, tgt)
    return tr.replay


def timed(fn, n):
    """ms per call of n back-to-back calls between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def launches_from(root):
    """per-step launches and kernel time of every variant from the traces under root/<variant>_<steps>/ (tools/per_step_launches.py)"""
    out = {}
    for v in VARIANTS:
        runs = {}
        for d in glob.glob(os.path.join(root, f"{v}_*")):
            csvs = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
            if csvs:
                runs[int(d.rsplit("_", 1)[1])] = csvs[0]
        if len(runs) < 2:
            continue
        k0, k1 = min(runs), max(runs)
        txt = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "per_step_launches.py"), runs[k0], str(k0), runs[k1], str(k1)],
                             capture_output=True, text=True, check=True).stdout
        m = re.search(r"per step: ([\d.]+) launches, ([\d.]+) ms of kernel time; torch / runtime glue \([^)]*\): ([\d.]+) launches", txt)
        out[v] = {"launches_per_step": float(m.group(1)), "kernel_ms_per_step": float(m.group(2)), "torch_glue_launches_per_step": float(m.group(3)),
                  "trace_steps": [k0, k1], "top": [ln.strip()[:140] for ln in txt.splitlines()[2:8]]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096,32768")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="least seconds per timed window")
    ap.add_argument("--out", default=None)
    ap.add_argument("--launches", default=None, help="directory of the kernel traces (see the module docstring)")
    ap.add_argument("--trace", choices=VARIANTS, default=None, help="trace target: --steps calls of one variant at --rays, nothing timed")
    ap.add_argument("--rays", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=8)
    args = ap.parse_args()
    if args.launches and args.sizes == "":             # the counts alone: reads the traces, needs no GPU
        text = json.dumps({"bench": "classic_trainer_launches", "rays": args.rays, "launches": launches_from(args.launches)}) + "\n"
        print(text, end="")
        if args.out:
            with open(args.out, "a") as f:
                f.write(text)
        return
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured on the host"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.trace:
        fn = make(args.trace, args.rays, dev)
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        return
    assert args.rounds >= 5 and args.window >= 0.5, "at least 5 rounds of at least half a second"
    sizes = [int(s) for s in args.sizes.split(",")]
    res, lines = {}, []
    for n in sizes:
        fns = {v: make(v, n, dev) for v in VARIANTS}
        calls = {}
        for v, fn in fns.items():                       # warm-up of this shape, then the call count that fills the window
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            per = timed(fn, 5)
            calls[v] = max(5, int(args.window * 1.1e3 / per) + 1)
        rounds = {v: [] for v in VARIANTS}
        for r in range(args.rounds):
            order = VARIANTS if r % 2 == 0 else VARIANTS[::-1]
            for v in order:
                rounds[v].append(timed(fns[v], calls[v]))
        med = {v: statistics.median(rounds[v]) for v in VARIANTS}
        spread = max(rounds["loop"]) - min(rounds["loop"])
        res[str(n)] = {"ms_per_step": {v: round(med[v], 4) for v in VARIANTS}, "calls_per_window": calls,
                       "min_window_s": {v: round(min(rounds[v]) * calls[v] / 1e3, 3) for v in VARIANTS},
                       "loop_over_step": round(med["loop"] / med["step"], 3), "loop_over_replay": round(med["loop"] / med["replay"], 3),
                       "loop_round_spread_ms": round(spread, 4), "step_minus_loop_ms": round(med["step"] - med["loop"], 4),
                       "rays_per_s": {v: round(n / med[v] * 1e3, 1) for v in VARIANTS}}
        for v in VARIANTS:
            lines.append(f"rounds {n:6d} rays {v:6s} ms/step: " + " ".join(f"{x:.4f}" for x in rounds[v]) + f"   median {med[v]:.4f}   ({calls[v]} calls per window)")
        del fns
        torch.cuda.empty_cache()
    big = res.get("32768")
    out = {"bench": "classic_trainer", "device": torch.cuda.get_device_name(0), "workload": f"path B train step: {N_SAMPLES} coarse + {N_IMPORTANCE} importance "
           "samples, NeRF 8 x 256 x 2, bf16; loop = bench.py:path_b_leg's train() (autograd + torch.optim.Adam), step = ClassicTrainer.step, replay = its "
           "captured graph", "rounds": args.rounds, "sizes": res}
    if big is not None:
        out["acceptance_32768"] = {"step_minus_loop_ms": big["step_minus_loop_ms"], "loop_round_spread_ms": big["loop_round_spread_ms"],
                                   "ok": big["step_minus_loop_ms"] <= big["loop_round_spread_ms"]}
    if args.launches:
        out["launches"] = launches_from(args.launches)
    text = json.dumps(out) + "\n" + "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
