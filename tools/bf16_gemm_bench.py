#!/usr/bin/env python3
"""ops.bf16_gemm against the library GEMM (torch.matmul, as the harness calls it) at the lm_head and Llama-3-8B bf16
decode shapes.  Device events after warm-up, the two contenders alternating, >= 0.5 s of timed work per shape and
contender, the weights rotating over enough copies to exceed the 256-MB Infinity Cache.  Not a test.
usage: bf16_gemm_bench.py [out.txt]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from iaas_sglang_amd import ops  # noqa: E402

DEV = "cuda"
PEAK, PLAIN = 8.0e12, 6.0e12          # HBM peak; the plain-load ceiling tools/src/hbm_read.hip measured
SHAPES = [("lm_head", 128, 128256, 4096), ("lm_head TP=8 shard", 256, 16032, 8192), ("C2 qkv", 32, 6144, 4096),
          ("C2 o", 32, 4096, 4096), ("C2 gate_up", 32, 28672, 4096), ("C2 down", 32, 4096, 14336)]


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
    lines = ["shape (M x N x K)                      native us   library us   native TB/s  of 8 TB/s  of 6 TB/s   library TB/s"]
    print(lines[0], flush=True)
    for name, M, N, K in SHAPES:
        wbytes = 2 * N * K
        ncopy = max(2, -(-600_000_000 // wbytes))
        ws = [torch.randn(N, K, device=DEV).to(torch.bfloat16) for _ in range(ncopy)]
        x = torch.randn(M, K, device=DEV).to(torch.bfloat16)
        out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
        contenders = {"native": lambda w: ops.bf16_gemm(x, w, out=out), "library": lambda w: torch.matmul(x, w.t(), out=out)}
        assert ops.bf16_gemm_ok(M, N, K, x, ws[0], out)
        total, calls = {"native": 0.0, "library": 0.0}, 0
        for fn in contenders.values():
            timed(fn, ws, 2)                                   # warm-up: code objects, library heuristics
        rounds = max(1, int(0.1 / max(timed(contenders["library"], ws, 1), 1e-6)))   # ~0.1 s per block
        while min(total.values()) < 0.5:
            for k, fn in contenders.items():                   # alternate
                total[k] += timed(fn, ws, rounds)
            calls += rounds * ncopy
        us = {k: total[k] / calls * 1e6 for k in total}
        rate = {k: wbytes / (us[k] * 1e-6) for k in us}
        lines.append(f"{name:20s} {M:4d} x {N:6d} x {K:5d}  {us['native']:9.1f}  {us['library']:11.1f}  "
                     f"{rate['native'] / 1e12:11.2f}  {100 * rate['native'] / PEAK:8.1f}%  {100 * rate['native'] / PLAIN:8.1f}%  "
                     f"{rate['library'] / 1e12:12.2f}")
        print(lines[-1], flush=True)
        del ws
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
