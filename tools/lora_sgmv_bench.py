#!/usr/bin/env python3
"""ops.lora_shrink / ops.lora_expand and the qkv pair (MiLoRABackend.run_qkv_lora) against their algorithmic bytes and
against a torch gather + bmm form of the same arithmetic.  K = 4096, N_out = 6144 (q 4096, k 1024, v 1024), 8 adapters
all of rank r, requests cycling over them.  Device events after warm-up, the contenders alternating, median of 5
blocks per contender; the adapter weights rotate over enough copies to exceed the 256-MB Infinity Cache (every layer of
a model has its own).  Not a test.
usage: lora_sgmv_bench.py [out.txt]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from iaas_sglang_amd import ops  # noqa: E402
from iaas_sglang_amd._compat import LoRABatchInfo  # noqa: E402
from iaas_sglang_amd.lora_backend import MiLoRABackend  # noqa: E402

DEV, DT = "cuda", torch.bfloat16
PLAIN = 6.0e12                        # the plain-load ceiling tools/src/hbm_read.hip measured
K, OFFS, NUM_LORA = 4096, [0, 4096, 5120, 6144], 8
N_OUT = OFFS[-1]
BATCHES = [("decode bs=1", [1]), ("decode bs=64", [1] * 64), ("decode bs=256", [1] * 256), ("extend 8x2048", [2048] * 8)]


def block(fn, sets, rounds):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(rounds):
        for s in sets:
            fn(s)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / (rounds * len(sets))


def measure(contenders, sets):
    """seconds per call of each contender: warm-up, then 5 alternating blocks of ~40 ms, the median block"""
    for fn in contenders.values():
        block(fn, sets, 2)
    rounds = {k: max(1, int(0.04 / max(block(fn, sets, 1) * len(sets), 1e-6))) for k, fn in contenders.items()}
    times = {k: [] for k in contenders}
    for _ in range(5):
        for k, fn in contenders.items():
            times[k].append(block(fn, sets, rounds[k]))
    return {k: statistics.median(v) for k, v in times.items()}


def main():
    head = (f"{'batch':14s} {'r':>3s} {'launch':8s} {'native us':>10s} {'torch us':>9s} {'alg. MB':>8s} {'GB/s':>7s} "
            f"{'of plain 6 TB/s':>15s}")
    lines = ["# bytes: x + the DISTINCT adapters' weights + output (expand: output read and written), each once.",
             "# torch: gather + bmm per slice (decode), one matmul per segment and slice (extend), same roundings.", head]
    print("\n".join(lines), flush=True)
    for name, lens in BATCHES:
        for r in (16, 64):
            bs, S = len(lens), sum(lens)
            widx = [i % NUM_LORA for i in range(bs)]
            used = len(set(widx))
            indptr = torch.zeros(bs + 1, dtype=torch.int32)
            indptr[1:] = torch.cumsum(torch.tensor(lens), 0)
            bi = LoRABatchInfo(bs=bs, seg_lens=torch.tensor(lens, device=DEV), seg_indptr=indptr.to(DEV), max_len=max(lens),
                               weight_indices=torch.tensor(widx, dtype=torch.int32, device=DEV),
                               lora_ranks=torch.full((NUM_LORA,), r, dtype=torch.int64, device=DEV),
                               scalings=torch.full((NUM_LORA,), 0.5, device=DEV))
            be = MiLoRABackend("mi355x", bi)
            set_bytes = NUM_LORA * (3 * r * K + N_OUT * r) * 2
            ncopy = max(2, min(64, -(-600_000_000 // set_bytes))) if S < 4096 else 2
            sets = [((torch.randn(NUM_LORA, 3 * r, K, device=DEV) / 64).to(DT),
                     (torch.randn(NUM_LORA, N_OUT, r, device=DEV) / r ** 0.5).to(DT)) for _ in range(ncopy)]
            x = torch.randn(S, K, device=DEV).to(DT)
            y = torch.randn(S, 3 * r, device=DEV).to(DT)
            out = torch.zeros(S, N_OUT, dtype=DT, device=DEV)
            offs_d = torch.tensor(OFFS, dtype=torch.int32, device=DEV)
            widx_l = bi.weight_indices.long()

            def t_shrink(s, x=x):
                if max(lens) == 1:
                    return torch.bmm(x.unsqueeze(1), s[0][widx_l].transpose(1, 2)).squeeze(1)
                return torch.cat([x[indptr[b]:indptr[b + 1]] @ s[0][widx[b]].T for b in range(bs)])

            def t_expand(s, y=y):
                for j in range(3):
                    yj, cols = y[:, j * r:(j + 1) * r], slice(OFFS[j], OFFS[j + 1])
                    if max(lens) == 1:
                        d = torch.bmm(yj.unsqueeze(1), s[1][widx_l, cols].transpose(1, 2)).squeeze(1)
                        out[:, cols] += d * 0.5
                    else:
                        for b in range(bs):
                            rows = slice(int(indptr[b]), int(indptr[b + 1]))
                            out[rows, cols] += (yj[rows] @ s[1][widx[b], cols].T) * 0.5
                return out

            launches = {
                "shrink": ({"native": lambda s: ops.lora_shrink(x, s[0], bi.seg_indptr, bi.weight_indices, bi.lora_ranks,
                                                                bs, bi.max_len, 3),
                            "torch": t_shrink}, (S * K + used * 3 * r * K + S * 3 * r) * 2),
                "expand": ({"native": lambda s: ops.lora_expand(y, s[1], out, bi.seg_indptr, bi.weight_indices,
                                                                bi.lora_ranks, bi.scalings, bs, bi.max_len, 3, 4096, offs_d),
                            "torch": t_expand}, (S * 3 * r + used * N_OUT * r + 2 * S * N_OUT) * 2),
                "qkv pair": ({"native": lambda s: be.run_qkv_lora(x, s[0], s[1], offs_d, 4096, out),
                              "torch": lambda s: t_expand(s, t_shrink(s))},
                             (S * K + used * (3 * r * K + N_OUT * r) + 2 * S * N_OUT) * 2),
            }
            for launch, (contenders, nbytes) in launches.items():
                t = measure(contenders, sets)
                rate = nbytes / t["native"]
                lines.append(f"{name:14s} {r:3d} {launch:8s} {t['native'] * 1e6:10.1f} {t['torch'] * 1e6:9.1f} "
                             f"{nbytes / 1e6:8.2f} {rate / 1e9:7.0f} {100 * rate / PLAIN:14.1f}%")
                print(lines[-1], flush=True)
            del sets
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
