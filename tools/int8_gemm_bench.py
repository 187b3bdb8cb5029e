#!/usr/bin/env python3
"""ops.int8_gemm against ops.fp8_gemm (row scales on both sides: the same bytes in, the same bytes out) at the four
Llama-3-8B linears with M = 128 and at gate_up with M = 16384.  Device events after warm-up, the two contenders
alternating in blocks of ~0.1 s, >= 0.5 s of timed work per shape and contender, the weights rotating over enough
copies to exceed the 256-MB Infinity Cache.  The spread column is (slowest - fastest block) / mean of one contender
on one shape: what a difference between the two has to exceed.  Not a test.
usage: int8_gemm_bench.py [out.txt]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from iaas_sglang_amd import ops  # noqa: E402

DEV = "cuda"
SHAPES = [("qkv", 128, 6144, 4096), ("o", 128, 4096, 4096), ("gate_up", 128, 28672, 4096), ("down", 128, 4096, 14336),
          ("gate_up prefill", 16384, 28672, 4096)]


def timed(fn, ws, rounds):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(rounds):
        for w in ws:
            fn(w)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def main():
    lines = ["shape (M x N x K)                         int8 us  spread    fp8 us  spread  int8/fp8   int8 TB/s | TOP/s"]
    print(lines[0], flush=True)
    for name, M, N, K in SHAPES:
        ncopy = max(2, -(-600_000_000 // (N * K))) if M <= 256 else 2
        raw = [torch.randint(0, 120, (N, K), dtype=torch.uint8, device=DEV) for _ in range(ncopy)]
        w8 = [(r.view(torch.int8), r.view(ops.FP8_DTYPE)) for r in raw]      # the same bytes, read as either type
        xr = torch.randint(0, 120, (M, K), dtype=torch.uint8, device=DEV)
        sa = torch.rand(M, device=DEV) * 1e-2 + 1e-3
        sb = torch.rand(N, device=DEV) * 1e-3 + 1e-4
        out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
        contenders = {"int8": lambda w: ops.int8_gemm(xr.view(torch.int8), w[0].t(), sa, sb, torch.bfloat16, out=out),
                      "fp8": lambda w: ops.fp8_gemm(xr.view(ops.FP8_DTYPE), w[1].t(), sa, sb, torch.bfloat16, out=out)}
        for fn in contenders.values():
            timed(fn, w8, 2)                                   # warm-up: code objects
        rounds = max(1, int(0.1 / max(timed(contenders["fp8"], w8, 1), 1e-6)))   # ~0.1 s per block
        blocks = {"int8": [], "fp8": []}
        while min(sum(b) for b in blocks.values()) < 0.5:
            for k, fn in contenders.items():                   # alternate
                blocks[k].append(timed(fn, w8, rounds))
        per = rounds * ncopy
        us = {k: sum(b) / (len(b) * per) * 1e6 for k, b in blocks.items()}
        spread = {k: (max(b) - min(b)) / (sum(b) / len(b)) for k, b in blocks.items()}
        rate = (f"{N * K / (us['int8'] * 1e-6) / 1e12:6.2f} TB/s" if M <= 256
                else f"{2 * M * N * K / (us['int8'] * 1e-6) / 1e12:6.0f} TOP/s")
        lines.append(f"{name:16s} {M:5d} x {N:5d} x {K:5d}  {us['int8']:9.1f}  {100 * spread['int8']:5.1f}%  "
                     f"{us['fp8']:8.1f}  {100 * spread['fp8']:5.1f}%  {us['int8'] / us['fp8']:8.2f}   {rate}")
        print(lines[-1], flush=True)
        del raw, w8
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
