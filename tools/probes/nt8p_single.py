#!/usr/bin/env python3
"""One launch kind of the persistent NT kernel (gemm_nt8p_kernel), back to back, N = K = 1024, bf16 -- a target for rocprofv3 --pmc passes and for
stand-alone timings of its two MFMA flavours (SNERF_NT_MFMA = 16 | 32 in the environment picks the flavour; unset = the default).

    python tools/probes/nt8p_single.py [M = 524288] [launches = 12] [fwd | dgrad]

fwd = bias + ReLU + bit masks (act 3, the forward launches of the step); dgrad = bit-mask ReLU backward + column sums (act 4, its data gradients,
consuming the masks of one fwd launch).  M = 4194304 makes a dispatch long enough (7-8 ms) for GRBM_GUI_ACTIVE / wall to read as a clock."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from snerf_amd import ops

M = int(sys.argv[1]) if len(sys.argv) > 1 else 524288
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 12
kind = sys.argv[3] if len(sys.argv) > 3 else "fwd"
N = K = 1024
g = torch.Generator(device="cuda").manual_seed(1)
A = (torch.rand(M, K, device="cuda", generator=g) * 2 - 1).bfloat16()
W = ((torch.rand(N, K, device="cuda", generator=g) * 2 - 1) / K ** 0.5).bfloat16()
b = torch.rand(N, device="cuda", generator=g) - 0.5
Y = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
bits = torch.zeros(ops.mask_bits_words(M, N), dtype=torch.int32, device="cuda")
cs = torch.zeros(N, device="cuda")
ops.linear_fwd(A, W, b, Y, K, N, ops.ACT_RELU_BITS, ops.BF16, aux=bits, variant=8)      # (dgrad: the mask words it consumes)


def launch():
    if kind == "fwd":
        ops.linear_fwd(A, W, b, Y, K, N, ops.ACT_RELU_BITS, ops.BF16, aux=bits, variant=8)
    else:
        ops.linear_fwd(A, W, None, Y, K, N, ops.ACT_MASK_BITS, ops.BF16, aux=bits, colsum=cs, variant=8)


for _ in range(2):
    launch()
ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
for e0, e1 in ev:
    e0.record(); launch(); e1.record()
torch.cuda.synchronize()
t = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)
print(f"nt8p_single M={M} {kind} flavour={os.environ.get('SNERF_NT_MFMA', 'default')}: median {t[len(t) // 2]:.1f} us, min {t[0]:.1f}, max {t[-1]:.1f} "
      f"({2.0 * M * N * K / t[len(t) // 2] / 1e6:.1f} TFLOP/s)")
