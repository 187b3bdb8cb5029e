#!/usr/bin/env python3
"""ops.bf16_gemm_tile against the library GEMM (F.linear, as UnquantizedLinearMethod calls it) at the Llama-3-8B bf16
prefill shapes.  Device events after warm-up, the two contenders alternating, >= 0.5 s of timed work per shape and
contender, the operands rotating over enough copies to exceed the 256-MB Infinity Cache.  Not a test.
usage: bf16_gemm_tile_bench.py [out.txt]"""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from iaas_sglang_amd import ops  # noqa: E402

DEV = "cuda"
PEAK = 2.5e15                          # dense bf16 MFMA peak
LAYERS = [("C2 qkv", 6144, 4096), ("C2 o", 4096, 4096), ("C2 gate_up", 28672, 4096), ("C2 down", 4096, 14336)]
ROWS = [1024, 2048, 8192, 16384]


def timed(fn, pairs, rounds):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(rounds):
        for x, w in pairs:
            fn(x, w)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def main():
    lines = ["shape (M x N x K)                 splits  native us  library us  native TFLOP/s  library TFLOP/s  native of 2.5 PFLOP/s"]
    print(lines[0], flush=True)
    for name, N, K in LAYERS:
        for M in ROWS:
            ncopy = max(2, -(-600_000_000 // (2 * (N + M) * K)))
            pairs = [(torch.randn(M, K, device=DEV).to(torch.bfloat16), torch.randn(N, K, device=DEV).to(torch.bfloat16))
                     for _ in range(ncopy)]
            out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
            assert ops.bf16_gemm_tile_ok(M, N, K, pairs[0][0], pairs[0][1], out)
            splits = ops.lib.mi_bf16_gemm_tile_workspace_bytes(M, N, K) // (4 * M * N) or 1
            contenders = {"native": lambda x, w: ops.bf16_gemm_tile(x, w, out=out), "library": lambda x, w: F.linear(x, w)}
            total, calls = {"native": 0.0, "library": 0.0}, 0
            for fn in contenders.values():
                timed(fn, pairs, 2)                                # warm-up: code objects, library heuristics
            rounds = max(1, int(0.1 / max(timed(contenders["library"], pairs, 1), 1e-6)))   # ~0.1 s per block
            while min(total.values()) < 0.5:
                for k, fn in contenders.items():                   # alternate
                    total[k] += timed(fn, pairs, rounds)
                calls += rounds * ncopy
            us = {k: total[k] / calls * 1e6 for k in total}
            rate = {k: 2.0 * M * N * K / (us[k] * 1e-6) for k in us}
            lines.append(f"{name:10s} {M:5d} x {N:5d} x {K:5d}  {splits:6d}  {us['native']:9.1f}  {us['library']:10.1f}  "
                         f"{rate['native'] / 1e12:14.0f}  {rate['library'] / 1e12:15.0f}  {100 * rate['native'] / PEAK:20.1f}%")
            print(lines[-1], flush=True)
            del pairs, out
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
