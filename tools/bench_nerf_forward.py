#!/usr/bin/env python3
"""NeRF 8 x 256 inference on pre-embedded rows (NeRF.forward(x), as batchify(fn, netchunk) calls it) against run_network on the points,
one MI355X, bf16 (or --compute fp16): 65 536 rays x 192 samples.  Three routes, device events, a warm-up:
  run_network   the pts launch (positional encodings computed in the kernel, snerf_fmlp_classic_pts_fwd)
  fused_x       batchify(model, 65536)(x) through snerf_fmlp_classic_x_fwd (x = [Embedder(pts) | Embedder(viewdirs)], fp32)
  per_layer     the same calls with the fused kernel off (fused=False): cast_pad into operand buffers + the per-layer GEMMs
Prints one JSON line (ms per full batch).  --route X: time one route only (rocprofv3 target)."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=65536)
    ap.add_argument("--samples", type=int, default=192)
    ap.add_argument("--netchunk", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--route", default="all", choices=["all", "run_network", "fused_x", "per_layer"])
    ap.add_argument("--compute", default="bf16", choices=["bf16", "fp16"])
    args = ap.parse_args()
    from snerf_amd import classic
    torch.manual_seed(0)
    m = classic.NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=4, skips=[4], use_viewdirs=True, compute=args.compute, device="cuda")
    e, _ = classic.get_embedder(10, 0)
    ev, _ = classic.get_embedder(4, 0)
    N, S = args.rays, args.samples
    pts = torch.rand(N, S, 3, device="cuda") * 4 - 2
    vd = torch.nn.functional.normalize(torch.randn(N, 3, device="cuda"), dim=-1)
    with torch.no_grad():
        x = torch.cat([e(pts.reshape(-1, 3)), ev(vd[:, None].expand(pts.shape).reshape(-1, 3))], -1)

    def batchify(fn, chunk):
        return lambda inputs: torch.cat([fn(inputs[i:i + chunk]) for i in range(0, inputs.shape[0], chunk)], 0)

    def per_layer():
        m.net.fused = False
        try:
            return batchify(m, args.netchunk)(x)
        finally:
            m.net.fused = True
    routes = {"run_network": lambda: classic.run_network(pts, vd, m, e, ev), "fused_x": lambda: batchify(m, args.netchunk)(x),
              "per_layer": per_layer}
    res = {"compute": args.compute, "rays": N, "samples": S, "rows": N * S, "netchunk": args.netchunk, "x_bytes": x.numel() * 4}
    with torch.no_grad():
        for name, fn in routes.items():
            if args.route not in ("all", name):
                continue
            for _ in range(args.warmup):
                fn()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(args.steps):
                fn()
            b.record()
            torch.cuda.synchronize()
            res[name + "_ms"] = round(a.elapsed_time(b) / args.steps, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
