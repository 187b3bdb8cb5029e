"""The native bf16 / fp16 prefill tile GEMM (ops.bf16_gemm_tile): exact on integer inputs, close on random ones, and
reached through MiUnquantizedLinearMethod above 512 rows."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
SPLIT = (520, 256, 64 * 65)     # 3 tiles, 65 k-steps: the plan picks 4 slices of 17, 17, 17 and 14
# one clamped tile and k-step; ragged second m- and n-block; three m-blocks and one k-step more than the 3-stage weight
# ring; 7 k-steps (odd ring wrap); 272 tiles on 256 CUs (a second tile per workgroup); split-K
SHAPES = [(1, 16, 64), (257, 264, 64), (513, 256, 256), (300, 520, 448), (4352, 4096, 64), SPLIT]


@functools.lru_cache(maxsize=None)
def _ints(M, N, K):
    """x, W in {-3..3}, bias in {-8..8} (int8) and the fp64 product.  With K <= 16384 every partial sum is an integer
    below 2^24, so any fp32 summation order is exact."""
    g = torch.Generator().manual_seed(M * 1000003 + N * 1009 + K)
    x = torch.randint(-3, 4, (M, K), generator=g, dtype=torch.int8)
    w = torch.randint(-3, 4, (N, K), generator=g, dtype=torch.int8)
    b = torch.randint(-8, 9, (N,), generator=g, dtype=torch.int8)
    return x, w, b, x.double() @ w.double().T


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_exact_on_integer_inputs(M, N, K, with_bias, dtype):
    from iaas_sglang_amd import ops
    x, w, b, ref = _ints(M, N, K)
    ref = ref + b.double() if with_bias else ref
    xd, wd = x.to(dtype).to(DEV), w.to(dtype).to(DEV)
    bd = b.to(dtype).to(DEV) if with_bias else None
    assert ops.bf16_gemm_tile_ok(M, N, K, xd, wd)
    assert torch.equal(ops.bf16_gemm_tile(xd, wd, bd, out_dtype=torch.float32).cpu().double(), ref)
    assert torch.equal(ops.bf16_gemm_tile(xd, wd, bd).cpu(), ref.to(dtype))          # one RNE rounding
    if (M, N, K) == SPLIT:      # it really split, and without scratch the unsplit walk gives the same exact result
        assert ops.lib.mi_bf16_gemm_tile_workspace_bytes(M, N, K) > 0
        out = torch.empty(M, N, dtype=dtype, device=DEV)
        ops.check(ops.lib.mi_bf16_gemm_tile(xd.data_ptr(), wd.data_ptr(), bd.data_ptr() if with_bias else None,
                                            out.data_ptr(), M, N, K, K, K, N, ops._dt(xd), ops._dt(xd), None, 0,
                                            ops._stream()), "mi_bf16_gemm_tile")
        assert torch.equal(out.cpu(), ref.to(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ldo", [256, 263])      # rows that take vector stores / rows that do not
def test_strided_operands(ldo, dtype):
    from iaas_sglang_amd import ops
    M, N, K = 257, 200, 128
    x, w, b, ref = _ints(M, N, K)
    wide_x = torch.full((M, K + 64), 5, dtype=dtype, device=DEV)
    wide_x[:, 32:32 + K] = x.to(dtype)
    for out_dtype in (dtype, torch.float32):
        wide_out = torch.full((M, ldo), 7, dtype=out_dtype, device=DEV)
        out = wide_out[:, 8:8 + N]
        assert ops.bf16_gemm_tile_ok(M, N, K, wide_x[:, 32:32 + K], w.to(dtype).to(DEV), out)
        ops.bf16_gemm_tile(wide_x[:, 32:32 + K], w.to(dtype).to(DEV), b.to(dtype).to(DEV), out=out)
        assert torch.equal(out.cpu().double(), (ref + b.double()).to(out_dtype).double())
        assert bool((wide_out[:, :8] == 7).all()) and bool((wide_out[:, 8 + N:] == 7).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K", [(520, 1040, 512), (1024, 512, 4096)])
def test_random_mantissas(M, N, K, dtype):
    from iaas_sglang_amd import ops
    g = torch.Generator().manual_seed(N + K)
    x, w = torch.randn(M, K, generator=g).to(dtype), torch.randn(N, K, generator=g).to(dtype)
    ref = x.double() @ w.double().T
    for out_dtype in (dtype, torch.float32):
        out = ops.bf16_gemm_tile(x.to(DEV), w.to(DEV), out_dtype=out_dtype)
        torch.testing.assert_close(out.cpu().double(), ref, rtol=2 ** -7, atol=2e-3)


@pytest.mark.parametrize("M,K,shift", [(16, 48, 0), (16, 64, 1)])   # K % 64, misaligned x
def test_refusals(M, K, shift):
    from iaas_sglang_amd import ops
    x = torch.zeros(M * K + 8, dtype=torch.bfloat16, device=DEV)[shift:shift + M * K].view(M, K)
    w = torch.zeros(32, K, dtype=torch.bfloat16, device=DEV)
    assert not ops.bf16_gemm_tile_ok(M, 32, K, x, w)
    with pytest.raises(ops.MiHotpathError, match=r"rc=-2"):      # MI_ERR_UNSUPPORTED, before any launch
        ops.bf16_gemm_tile(x, w)


@pytest.mark.parametrize("dtype", DTYPES)
def test_linear_method_runs_the_tile_kernel_above_512_rows(dtype):
    from iaas_sglang_amd import ops
    from iaas_sglang_amd.quantization import MiUnquantizedLinearMethod
    N, K = 200, 256
    g = torch.Generator().manual_seed(5)
    method, layer = MiUnquantizedLinearMethod(), torch.nn.Module()
    method.create_weights(layer, K, [N], K, N, dtype)
    layer.to(DEV)
    layer.weight.data.copy_(torch.randn(N, K, generator=g))
    x = torch.randn(2, 260, K, generator=g).to(dtype).to(DEV)
    bias = torch.randn(N, generator=g).to(dtype).to(DEV)
    y = method.apply(layer, x, bias)
    assert y.shape == (2, 260, N) and torch.equal(y.view(520, N), ops.bf16_gemm_tile(x.view(520, K), layer.weight, bias))


@pytest.mark.parametrize("dtype", DTYPES)
def test_split_k_call_is_capturable(dtype):
    from iaas_sglang_amd import ops
    M, N, K = SPLIT
    x, w, b, _ = _ints(M, N, K)
    xd, wd, bd = x.to(dtype).to(DEV), w.to(dtype).to(DEV), b.to(dtype).to(DEV)
    assert ops.lib.mi_bf16_gemm_tile_workspace_bytes(M, N, K) > 0
    eager = ops.bf16_gemm_tile(xd, wd, bd)            # (also sizes the shared workspace before the capture)
    out, graph = torch.empty_like(eager), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        ops.bf16_gemm_tile(xd, wd, bd, out=out)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
