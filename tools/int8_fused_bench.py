#!/usr/bin/env python3
"""One W8A8 int8 decoder layer of Llama-3-8B shapes (hidden 4096, qkv 6144, intermediate 14336, KV 2048 per request)
at M = 16, 128, 256: the fused sequence (LlamaStack.forward_decode_fused8) against the unfused sequence of
mi_int8_quant_per_token + mi_int8_gemm + the 16-bit glue kernels (LlamaStack.fuse_decode_layer = False).

A 2-layer stack with a 1024-row lm_head (the same head and tail in both legs) is captured once per leg into a hipGraph,
the replays are checked against the eager logits and against each other (bit-identical), then timed with device events:
the two legs alternate in blocks of ~0.1 s until each has 0.5 s of timed work.  "us/layer" is the step over the 2
layers; the spread is (slowest - fastest block) / mean of one leg, what a difference between the legs has to exceed.
Launches are counted per step from the C-ABI calls (a split-K mi_int8_gemm and every fused int8 form are 2 launches,
split-KV decode attention is counted as its calls).  Not a test.
usage: int8_fused_bench.py [out.txt]"""
import collections
import dataclasses
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from iaas_sglang_amd import harness as H, ops  # noqa: E402
from iaas_sglang_amd._lib import lib  # noqa: E402
from iaas_sglang_amd.attention_backend import MiAttnBackend  # noqa: E402
from iaas_sglang_amd.quantization.w8a8_int8 import W8A8Int8Config, W8A8Int8LinearMethod  # noqa: E402

DEV, DTYPE, LAYERS, KV = "cuda", torch.bfloat16, 2, 2048
TWO_LAUNCH = {"mi_int8_gemm_add_rmsnorm_int8", "mi_int8_gemm_rope_kvwrite", "mi_int8_gemm_silu_mul_int8"}


def count_launches(step):
    """C-ABI calls of one eager step, by name, and the kernel launches they stand for"""
    calls, extra = collections.Counter(), [0]
    check, gemm = ops.check, ops.int8_gemm

    def counting_check(rc, what):
        calls[what] += 1
        return check(rc, what)

    def counting_gemm(a, b_kn, *args, **kw):
        extra[0] += lib.mi_int8_gemm_workspace_bytes(a.shape[0], b_kn.shape[1], a.shape[1]) > 0    # + the slab reduce
        return gemm(a, b_kn, *args, **kw)

    ops.check, ops.int8_gemm = counting_check, counting_gemm
    try:
        step()
    finally:
        ops.check, ops.int8_gemm = check, gemm
    return calls, sum(calls.values()) + extra[0] + sum(calls[n] for n in TWO_LAUNCH)


def timed(graph, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        graph.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def main():
    shape = dataclasses.replace(H.LLAMA3_8B, layers=LAYERS, vocab=1024)
    cfg = W8A8Int8Config.from_config({})
    stack = H.LlamaStack(shape, lambda: W8A8Int8LinearMethod(cfg), DTYPE, DEV, weight_range=0.02)
    lines = ["    M   fused us/layer  spread   unfused us/layer  spread   fused/unfused   launches per step (fused | unfused)"]
    print(lines[0], flush=True)
    for M in (16, 128, 256):
        runner = H.make_runner(shape, max_reqs=M, ctx=KV + 8, pool_tokens=M * KV, dtype=DTYPE, device=DEV, fill_kv=True)
        backend = MiAttnBackend(runner)
        fb = H.make_decode_batch(runner, backend, M, KV, DEV, seed=3)
        h0 = torch.randn(M, shape.hidden, generator=torch.Generator().manual_seed(1)).to(DTYPE).to(DEV)
        hidden = h0.clone()
        backend.init_forward_metadata(fb)
        legs, launches = {}, {}
        for name, fused in (("fused", True), ("unfused", False)):
            def step():
                H.LlamaStack.fuse_decode_layer = fused
                try:
                    hidden.copy_(h0)                         # the residual stream is updated in place
                    return stack.forward(hidden, fb.positions, fb, backend)
                finally:
                    H.LlamaStack.fuse_decode_layer = True
            assert stack._fused_decode8_ok(hidden, fb)
            calls, launches[name] = count_launches(step)
            eager = step().clone()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                step()
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = step()
            for _ in range(3):
                graph.replay()
                torch.cuda.synchronize()
                assert torch.equal(out, eager), f"{name}: graph replay differs from the eager step"
            legs[name] = (graph, out)
            print(f"  [{name} M={M}] C-ABI calls per step: {dict(calls)}", flush=True)
        assert torch.equal(legs["fused"][1], legs["unfused"][1]), "fused and unfused logits differ"
        n = max(1, int(0.1 / max(timed(legs["unfused"][0], 3) / 3, 1e-6)))
        blocks = {"fused": [], "unfused": []}
        while min(sum(b) for b in blocks.values()) < 0.5:
            for name, (graph, _) in legs.items():           # alternate
                blocks[name].append(timed(graph, n))
        us = {k: sum(b) / (len(b) * n * LAYERS) * 1e6 for k, b in blocks.items()}
        spread = {k: (max(b) - min(b)) / (sum(b) / len(b)) for k, b in blocks.items()}
        lines.append(f"{M:5d}   {us['fused']:14.1f}  {100 * spread['fused']:5.1f}%   {us['unfused']:16.1f}  "
                     f"{100 * spread['unfused']:5.1f}%   {us['fused'] / us['unfused']:13.3f}   "
                     f"{launches['fused']} | {launches['unfused']}  ({LAYERS} layers + the first norm; lm_head and input copy not counted)")
        print(lines[-1], flush=True)
        del legs, runner, backend, fb
        torch.cuda.empty_cache()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
