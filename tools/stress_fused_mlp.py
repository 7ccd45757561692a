#!/usr/bin/env python3
"""Race screen for the classic-network paths at a few-tile size (M = 768): the fused kernel (in-kernel embedding), the fused kernel
behind the embedding kernel, and the per-layer GEMM chain must each give bit-identical outputs on repeated evaluation, with vendor
kernels interleaved (different LDS / register garbage).  --compute {bf16,fp16}: the network's compute mode (default bf16)."""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from snerf_amd import classic

import ctypes
_pz = os.path.join(os.path.dirname(os.path.abspath(__file__)), "probes", "liblds_poison.so")
poison = ctypes.CDLL(_pz).lds_poison if os.path.exists(_pz) else None     # optional: NaN-fill every CU's LDS before evaluations
if poison is not None:
    poison.argtypes = [ctypes.c_uint, ctypes.c_void_p]

ap = argparse.ArgumentParser()
ap.add_argument("--compute", default="bf16", choices=["bf16", "fp16"])
args = ap.parse_args()
torch.manual_seed(0)
net = classic.NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=4, skips=[4], use_viewdirs=True, compute=args.compute, device="cuda")
e, ev = classic.get_embedder(10, 0)[0], classic.get_embedder(4, 0)[0]
big = torch.randn(4096, 4096, device="cuda").bfloat16()
bad = 0
for M in (768, 1000, 4096):
    S = 8
    pts = (torch.rand(M // S, S, 3, device="cuda") * 4 - 2)
    vd = torch.nn.functional.normalize(torch.randn(M // S, 3, device="cuda"), dim=-1)
    for mode in ("fused_pts", "fused_embed_kernel", "per_layer"):
        net.net.fused = mode != "per_layer"
        net.net.fused_embed = mode == "fused_pts"
        ref = None
        with torch.no_grad():
            for it in range(300):
                if poison is not None and it % 2 == 1:
                    poison(0x7FC00000 if it % 4 == 1 else 0xFFFFFFFF, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
                out = classic.run_network(pts, vd, net, e, ev).clone()
                if it % 3 == 0:
                    torch.mm(big, big)
                if ref is None:
                    ref = out
                    assert bool(torch.isfinite(ref).all())
                elif not torch.equal(out, ref):
                    bad += 1
                    d = (out - ref).abs()
                    print(f"MISMATCH M={M} {mode} it={it}: {int((d > 0).sum())} elements, max {float(d.max()):.3e}, nonfinite {int((~torch.isfinite(out)).sum())}", flush=True)
                    if bad > 10:
                        sys.exit(1)
net.net.fused = net.net.fused_embed = True
print("stress_fused_mlp:", "OK (all repeats bit-identical)" if bad == 0 else f"{bad} mismatching evaluations")
sys.exit(0 if bad == 0 else 1)
