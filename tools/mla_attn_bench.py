#!/usr/bin/env python3
"""Micro-benchmark of mi_mla_attn, decode shape (env B=128, S=2048, H=16 q heads per rank, SPLITS=1, NPOOL=6 latent pools
cycled so the Infinity Cache cannot help).  Algorithmic bytes = every latent row once (1152 B) + q + o + indices.
Not a test."""
import os
import sys
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from iaas_sglang_amd import ops  # noqa: E402

dev = "cuda"
B, S, H = int(os.environ.get("B", "128")), int(os.environ.get("S", "2048")), int(os.environ.get("H", "16"))
ns, npool, iters = int(os.environ.get("SPLITS", "1")), int(os.environ.get("NPOOL", "6")), int(os.environ.get("ITERS", "30"))
pools = [torch.randn(B * S + 1, 1, 576, device=dev, dtype=torch.float32).to(torch.bfloat16) for _ in range(npool)]
q = torch.randn(B, H, 576, device=dev, dtype=torch.float32).to(torch.bfloat16)
o = torch.empty(B, H, 512, device=dev, dtype=torch.bfloat16)
g = torch.Generator(device=dev).manual_seed(0)
idx = torch.randperm(B * S, device=dev, generator=g).to(torch.int32) + 1
indptr = ops.kv_indptr(torch.full((B,), S, dtype=torch.int64, device=dev))
ws = torch.empty(max(1, ops.decode_workspace_numel(B, H, 512, ns)), dtype=torch.float32, device=dev)
abytes = B * S * 1152 + B * H * (576 + 512) * 2 + 4 * B * S
flops = 2.0 * B * H * S * (576 + 512)


def run(i):
    ops.mla_attention(q, pools[i % npool], o, indptr, idx, 576 ** -0.5, None, ns, ws)


for i in range(2 * npool):
    run(i)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for i in range(iters):
    run(i)
e1.record()
torch.cuda.synchronize()
us = e0.elapsed_time(e1) * 1e3 / iters
print(f"B={B} S={S} H={H} splits={ns}: {us:9.1f} us per call (merge included)  {abytes / us / 1e3:8.1f} GB/s  "
      f"{flops / us / 1e6:7.1f} TFLOP/s")
