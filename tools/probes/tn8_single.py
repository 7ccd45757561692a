#!/usr/bin/env python3
"""The 256 x 256 weight-gradient kernel alone (gemm_tn8_kernel, csrc/gemm.hip): a few launches of one wide layer's shape on random operands with
about half zeros -- target for rocprofv3 passes and for timing the two MFMA flavours side by side (SNERF_WGRAD_MFMA=16 | 32 forces one).
    python tools/probes/tn8_single.py [M=524288] [launches=12] [bf16|fp16]
Prints the HIP-event time of every launch after the first two."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from snerf_amd import ops

M = int(sys.argv[1]) if len(sys.argv) > 1 else 524288
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 12
dt = ops.F16 if len(sys.argv) > 3 and sys.argv[3] == "fp16" else ops.BF16
N = K = 1024
g = torch.Generator(device="cuda").manual_seed(3)
def operand(cols):
    x = torch.randn(M, cols, device="cuda", generator=g, dtype=torch.float32)
    x *= torch.rand(M, cols, device="cuda", generator=g) < 0.5
    return x.to(ops.torch_dtype(dt))
dZ, X = operand(N), operand(K)
dW = torch.zeros(N, K, device="cuda")
ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
for e0, e1 in ev:
    e0.record(); ops.linear_wgrad(dZ, X, dW, N, K, dt, variant=3); e1.record()
torch.cuda.synchronize()
us = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev[2:])
print(f"tn8_single M={M} flavour={os.environ.get('SNERF_WGRAD_MFMA', 'default')} dt={dt}: median {us[len(us) // 2]:.1f} us, min {us[0]:.1f}, max {us[-1]:.1f} "
      f"({2.0 * M * N * K / us[len(us) // 2] / 1e6:.1f} TFLOP/s, launch + fold)")
