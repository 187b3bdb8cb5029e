"""Multi-LoRA segmented GEMMs (ops.lora_shrink / ops.lora_expand, MiLoRABackend) against a plain fp64 torch form of
the same arithmetic: exact on integer inputs, close on random ones, following rewritten batch info under graph replay."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
RANKS = [0, 6, 8, 16, 64]                 # adapter a has rank RANKS[a]
SCALINGS = [0.5, 2.0, 0.25, 0.5, 2.0]
R_MAX = 64
# segment lengths and adapters: "extend" crosses the 16- and 64-row blocks and has an empty segment, "decode"
# (max_len <= 16) takes the split-K shrink kernel; every rank occurs on a non-empty segment of both
BATCHES = {"extend": ([1, 15, 16, 17, 0, 33, 70], [3, 1, 4, 2, 4, 0, 4]),
           "decode": ([1, 1, 3, 16, 0, 1, 2], [3, 1, 4, 2, 4, 0, 4])}


def _batch_info(lens, widx, ranks, scalings, rank_dtype=torch.int64, device=DEV):
    from iaas_sglang_amd._compat import LoRABatchInfo
    indptr = torch.zeros(len(lens) + 1, dtype=torch.int32)
    indptr[1:] = torch.cumsum(torch.tensor(lens), 0)
    return LoRABatchInfo(bs=len(lens), seg_lens=torch.tensor(lens, dtype=torch.float32).to(device),
                         seg_indptr=indptr.to(device), max_len=max(lens),
                         weight_indices=torch.tensor(widx, dtype=torch.int32).to(device),
                         lora_ranks=torch.tensor(ranks, dtype=rank_dtype).to(device),
                         scalings=torch.tensor(scalings, dtype=torch.float32).to(device))


def ref_shrink(x, w, lens, widx, ranks, stack_num, out):
    """x [S,K], w [L,N,K] fp64; writes round_T(x . w[a]^T) into the first stack_num * rank columns of `out` (dtype T)."""
    row = 0
    for n_rows, a in zip(lens, widx):
        n_b = min(w.shape[1], stack_num * ranks[a])
        out[row:row + n_rows, :n_b] = (x[row:row + n_rows] @ w[a, :n_b].T).to(out.dtype)
        row += n_rows
    return out


def ref_expand(y, w, lens, widx, ranks, scalings, offs, out):
    """y [S, slices * R], w [L,N_out,R] fp64; out (dtype T) += per slice, with the contract's two roundings."""
    row, R = 0, w.shape[2]
    for n_rows, a in zip(lens, widx):
        rho = min(R, ranks[a])
        rows = slice(row, row + n_rows)
        row += n_rows
        if rho == 0:
            continue
        for j in range(len(offs) - 1):
            acc = y[rows, j * rho:(j + 1) * rho] @ w[a, offs[j]:offs[j + 1], :rho].T
            scaled = (acc * scalings[a]).to(out.dtype)
            out[rows, offs[j]:offs[j + 1]] = (scaled.float() + out[rows, offs[j]:offs[j + 1]].float()).to(out.dtype)
    return out


@functools.lru_cache(maxsize=None)
def _shrink_ints(K, stack_num, S):
    """x, W in {-3..3}: with K <= 4096 every partial sum is an integer below 2^24, so any fp32 order is exact."""
    g = torch.Generator().manual_seed(K * 131 + stack_num)
    x = torch.randint(-3, 4, (S, K), generator=g, dtype=torch.int8)
    w = torch.randint(-3, 4, (len(RANKS), stack_num * R_MAX, K), generator=g, dtype=torch.int8)
    return x, w


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("K,stack_num,wide", [(K, s, False) for K in (64, 200, 4096) for s in (1, 2, 3)] + [(200, 3, True)])
def test_shrink_exact_on_integer_inputs(K, stack_num, wide, batch, dtype):
    from iaas_sglang_amd import ops
    lens, widx = BATCHES[batch]
    S, N = sum(lens), stack_num * R_MAX
    x, w = _shrink_ints(K, stack_num, S)
    bi = _batch_info(lens, widx, RANKS, SCALINGS)
    ref = ref_shrink(x.double(), w.double(), lens, widx, RANKS, stack_num, torch.full((S, N), 0.5, dtype=dtype))
    xd = torch.full((S, K + 64 if wide else K), 5, dtype=dtype, device=DEV)[:, -K:]
    xd.copy_(x.to(dtype))
    out_buf = torch.full((S, N + 8 if wide else N), 0.5, dtype=dtype, device=DEV)     # 0.5: the sentinel, no integer
    out = out_buf[:, :N]
    ops.lora_shrink(xd, w.to(dtype).to(DEV), bi.seg_indptr, bi.weight_indices, bi.lora_ranks, bi.bs, bi.max_len,
                    stack_num, out=out)
    assert torch.equal(out.cpu(), ref)          # columns >= stack_num * rank and rank-0 rows still hold the sentinel
    assert bool((out_buf[:, N:] == 0.5).all())


EXPAND_CASES = {"one": (200, [0, 200], False), "two_equal": (272, [0, 136, 272], False),
                "qkv": (192, [0, 128, 160, 192], True), "qkv_unaligned": (200, [0, 130, 162, 194], True)}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("case", list(EXPAND_CASES))
def test_expand_exact_on_integer_inputs(case, batch, dtype):
    from iaas_sglang_amd import ops
    n_out, offs, on_device = EXPAND_CASES[case]
    lens, widx = BATCHES[batch]
    S, slices = sum(lens), len(offs) - 1
    g = torch.Generator().manual_seed(n_out)
    y = torch.randint(-3, 4, (S, slices * R_MAX), generator=g, dtype=torch.int8)
    w = torch.randint(-3, 4, (len(RANKS), n_out, R_MAX), generator=g, dtype=torch.int8)
    base = torch.randint(-8, 9, (S, n_out), generator=g, dtype=torch.int8).to(dtype)
    bi = _batch_info(lens, widx, RANKS, SCALINGS)
    ref = ref_expand(y.double(), w.double(), lens, widx, RANKS, SCALINGS, offs, base.clone())
    # what lies beyond the adapter's rank must not be read as data: x past slices * rank (a kernel that reads slice j
    # at j * R_MAX lands there) and the weights' k tail hold garbage
    yd, wd, row = y.to(dtype), w.to(dtype), 0
    for n_rows, a in zip(lens, widx):
        yd[row:row + n_rows, slices * min(R_MAX, RANKS[a]):] = 1000.0
        row += n_rows
    for a, rank in enumerate(RANKS):
        wd[a, :, rank:] = float("nan")
    out_buf = torch.full((S, n_out + 8), 0.5, dtype=dtype, device=DEV)
    out = out_buf[:, :n_out]
    out.copy_(base)
    ops.lora_expand(yd.to(DEV), wd.to(DEV), out, bi.seg_indptr, bi.weight_indices, bi.lora_ranks, bi.scalings, bi.bs,
                    bi.max_len, slices, max(b - a for a, b in zip(offs, offs[1:])),
                    torch.tensor(offs, dtype=torch.int32, device=DEV) if on_device else None)
    assert torch.equal(out.cpu(), ref)          # rank-0 rows: the base, bit for bit
    assert bool((out_buf[:, n_out:] == 0.5).all())


def _random_layer(dtype, stack_num, n_out):
    """K = 512, r_max = 16, two adapters of rank 8 and 16; scaled so the shrink output and the result are O(1)."""
    K, r_max = 512, 16
    g = torch.Generator().manual_seed(stack_num)
    a = (torch.randn(2, stack_num * r_max, K, generator=g) / K ** 0.5).to(dtype)
    b = (torch.randn(2, n_out, r_max, generator=g) / r_max ** 0.5).to(dtype)
    return K, a, b, g


def ref_layer(x, a, b, base, lens, widx, ranks, scalings, stack_num, offs):
    """fp64 with the three roundings to T of the two-launch form: shrink output, scaled product, sum."""
    dtype = base.dtype
    y = ref_shrink(x.double(), a.double(), lens, widx, ranks, stack_num,
                   torch.zeros(x.shape[0], a.shape[1], dtype=dtype))
    return ref_expand(y.double(), b.double(), lens, widx, ranks, scalings, offs, base.clone())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lens", [[1] * 8, [5, 40, 19]], ids=["decode", "extend"])
@pytest.mark.parametrize("layer", ["qkv", "gate_up"])
def test_backend_random_mantissas(layer, lens, dtype):
    """rtol 2^-7, atol 2e-3 (tests/test_bf16_gemm_gpu.py, the same accumulate-order difference).  Checked on the CPU
    before the kernels ran: the reference re-summed in fp32 with k visited in a random permutation, rounded at the
    same three points, stays inside this bound against the fp64 reference for both dtypes and all four cases here
    (bf16: identical; fp16: one flipped rounding, 1.95e-3 on a value near 4, 5e-4 above rtol * |ref| of the 2e-3 atol)."""
    from iaas_sglang_amd.lora_backend import MiLoRABackend
    ranks, scalings = [8, 16], [1.0, 0.5]
    widx = [i % 2 for i in range(len(lens))]
    stack_num, offs = (3, [0, 256, 320, 384]) if layer == "qkv" else (2, [0, 192, 384])
    K, a, b, g = _random_layer(dtype, stack_num, offs[-1])
    x = torch.randn(sum(lens), K, generator=g).to(dtype)
    base = torch.randn(sum(lens), offs[-1], generator=g).to(dtype)
    ref = ref_layer(x, a, b, base, lens, widx, ranks, scalings, stack_num, offs)
    be = MiLoRABackend("mi355x")
    be.set_batch_info(_batch_info(lens, widx, ranks, scalings))
    if layer == "qkv":
        out = be.run_qkv_lora(x.to(DEV), a.to(DEV), b.to(DEV), base_output=base.to(DEV),
                              output_offset=torch.tensor(offs, dtype=torch.int32, device=DEV), max_qkv_out_dim=256)
    else:
        out = be.run_gate_up_lora(x.to(DEV), a.to(DEV), b.to(DEV), base_output=base.to(DEV))
    torch.testing.assert_close(out.cpu().double(), ref.double(), rtol=2 ** -7, atol=2e-3)


def test_graph_replay_follows_device_batch_info():
    """The int32 graph-mode tensors of lora_manager.py:77-100, rewritten in place between replays."""
    from iaas_sglang_amd.lora_backend import MiLoRABackend
    dtype, bs, offs = torch.bfloat16, 4, [0, 256, 320, 384]
    K, a, b, g = _random_layer(dtype, 3, offs[-1])
    x = torch.randn(bs, K, generator=g).to(dtype).to(DEV)
    base = torch.randn(bs, offs[-1], generator=g).to(dtype).to(DEV)
    a, b, offs_d = a.to(DEV), b.to(DEV), torch.tensor(offs, dtype=torch.int32, device=DEV)
    bi = _batch_info([1] * bs, [0, 1, 0, 1], [8, 16], [1.0, 0.5], rank_dtype=torch.int32)
    be = MiLoRABackend("mi355x")
    be.set_batch_info(bi)
    out = torch.empty_like(base)

    def run(dst):
        dst.copy_(base)
        return be.run_qkv_lora(x, a, b, base_output=dst, output_offset=offs_d, max_qkv_out_dim=256)

    run(out)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(out)
    for widx, ranks, scalings in [([1, 1, 0, 0], [16, 8], [0.25, 2.0]), ([0, 0, 0, 1], [0, 16], [1.0, 1.5])]:
        bi.weight_indices.copy_(torch.tensor(widx, dtype=torch.int32))
        bi.lora_ranks.copy_(torch.tensor(ranks, dtype=torch.int32))
        bi.scalings.copy_(torch.tensor(scalings))
        eager = run(torch.empty_like(base)).clone()
        for _ in range(3):
            graph.replay()
            assert torch.equal(out, eager)


@pytest.mark.parametrize("case", ["K=100", "r_max=12", "r_max=264", "misaligned x"])
def test_refusals(case):
    from iaas_sglang_amd import ops
    from iaas_sglang_amd._lib import MiHotpathError
    S, K, N = 4, {"K=100": 100}.get(case, 64), {"r_max=12": 12, "r_max=264": 264}.get(case, 16)
    x = torch.ones(S * 128 + 8, dtype=torch.bfloat16, device=DEV)
    x = x[1:1 + S * K].view(S, K) if case == "misaligned x" else x[:S * 128].view(S, 128)[:, :K]
    w = torch.ones(1, N, K, dtype=torch.bfloat16, device=DEV)
    out_buf = torch.full((S, 272), 0.5, dtype=torch.bfloat16, device=DEV)
    bi = _batch_info([1] * S, [0] * S, [8], [1.0])
    with pytest.raises(MiHotpathError, match=r"rc=-2"):
        ops.lora_shrink(x, w, bi.seg_indptr, bi.weight_indices, bi.lora_ranks, bi.bs, bi.max_len, out=out_buf[:, :N])
    assert bool((out_buf == 0.5).all())
