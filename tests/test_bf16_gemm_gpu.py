"""The native bf16 / fp16 decode GEMM (ops.bf16_gemm): exact on integer inputs, close on random ones, and reached
through MiUnquantizedLinearMethod and LlamaStack(native_lm_head=True)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
SHAPES = [(1, 16, 64), (17, 200, 128), (128, 128, 192), (130, 1040, 512), (256, 384, 4096), (257, 136, 256),
          (500, 4096, 2048), (128, 16032, 4096), (32, 4096, 14336)]


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
    assert ops.bf16_gemm_ok(M, N, K, xd, wd)
    assert torch.equal(ops.bf16_gemm(xd, wd, bd, out_dtype=torch.float32).cpu().double(), ref)
    assert torch.equal(ops.bf16_gemm(xd, wd, bd).cpu(), ref.to(dtype))          # one RNE rounding


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ldo", [256, 263])      # rows that take vector stores / rows that do not
def test_strided_operands(ldo, dtype):
    from iaas_sglang_amd import ops
    M, N, K = 17, 200, 128
    x, w, b, ref = _ints(M, N, K)
    wide_x = torch.full((M, K + 64), 5, dtype=dtype, device=DEV)
    wide_x[:, 32:32 + K] = x.to(dtype)
    for out_dtype in (dtype, torch.float32):
        wide_out = torch.full((M, ldo), 7, dtype=out_dtype, device=DEV)
        out = wide_out[:, 8:8 + N]
        assert ops.bf16_gemm_ok(M, N, K, wide_x[:, 32:32 + K], w.to(dtype).to(DEV), out)
        ops.bf16_gemm(wide_x[:, 32:32 + K], w.to(dtype).to(DEV), b.to(dtype).to(DEV), out=out)
        assert torch.equal(out.cpu().double(), (ref + b.double()).to(out_dtype).double())
        assert bool((wide_out[:, :8] == 7).all()) and bool((wide_out[:, 8 + N:] == 7).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K", [(128, 1040, 512), (64, 4096, 4096)])
def test_random_mantissas(M, N, K, dtype):
    from iaas_sglang_amd import ops
    g = torch.Generator().manual_seed(N + K)
    x, w = torch.randn(M, K, generator=g).to(dtype), torch.randn(N, K, generator=g).to(dtype)
    ref = x.double() @ w.double().T
    for out_dtype in (dtype, torch.float32):
        out = ops.bf16_gemm(x.to(DEV), w.to(DEV), out_dtype=out_dtype)
        torch.testing.assert_close(out.cpu().double(), ref, rtol=2 ** -7, atol=2e-3)


@pytest.mark.parametrize("M,K,shift", [(16, 48, 0), (513, 64, 0), (16, 64, 1)])   # K % 64, too many rows, misaligned x
def test_refusals(M, K, shift):
    from iaas_sglang_amd import ops
    x = torch.zeros(M * K + 8, dtype=torch.bfloat16, device=DEV)[shift:shift + M * K].view(M, K)
    w = torch.zeros(32, K, dtype=torch.bfloat16, device=DEV)
    assert not ops.bf16_gemm_ok(M, 32, K, x, w)
    with pytest.raises(ops.MiHotpathError, match=r"rc=-2"):      # MI_ERR_UNSUPPORTED, before any launch
        ops.bf16_gemm(x, w)


@pytest.mark.parametrize("dtype", DTYPES)
def test_linear_method_runs_the_native_kernel(dtype):
    from iaas_sglang_amd import ops
    from iaas_sglang_amd._compat import UnquantizedLinearMethod
    from iaas_sglang_amd.quantization import MiUnquantizedLinearMethod
    N, K = 200, 256
    g = torch.Generator().manual_seed(5)
    method, layer = MiUnquantizedLinearMethod(), torch.nn.Module()
    assert isinstance(method, UnquantizedLinearMethod)
    method.create_weights(layer, K, [N], K, N, dtype)
    layer.to(DEV)
    layer.weight.data.copy_(torch.randn(N, K, generator=g))
    x = torch.randn(2, 8, K, generator=g).to(dtype).to(DEV)
    bias = torch.randn(N, generator=g).to(dtype).to(DEV)
    y = method.apply(layer, x, bias)
    assert y.shape == (2, 8, N) and torch.equal(y.view(16, N), ops.bf16_gemm(x.view(16, K), layer.weight, bias))


def test_native_lm_head_decode_step_eager_and_captured():
    from iaas_sglang_amd import harness as H
    from iaas_sglang_amd.attention_backend import MiAttnBackend
    from iaas_sglang_amd.quantization import Fp8Config
    shape, dtype, B, S = H.TINY, torch.bfloat16, 8, 40
    cfg = Fp8Config(is_checkpoint_fp8_serialized=True, activation_scheme="static")
    runner = H.make_runner(shape, max_reqs=B, ctx=128, pool_tokens=B * S + 8, dtype=dtype, device=DEV, fill_kv=True)
    backend = MiAttnBackend(runner)
    stack = H.LlamaStack(shape, lambda: cfg.get_quant_method(None, ""), dtype, DEV, weight_range=0.05, native_lm_head=True)
    fb = H.make_decode_batch(runner, backend, B, S, DEV, seed=0)
    hidden0 = torch.randn(B, shape.hidden, generator=torch.Generator().manual_seed(3)).to(dtype).to(DEV)
    hidden = hidden0.clone()                 # the step updates its input in place
    backend.init_forward_metadata(fb)
    stack.calibrate_static_input_scales(hidden, fb.positions, fb, backend)
    backend.init_forward_metadata(fb)

    def step():
        hidden.copy_(hidden0)
        return stack.forward_decode_fused(hidden, fb.positions, fb, backend)

    native = step().clone()
    stack.native_lm_head = False
    library = step().clone()
    stack.native_lm_head = True
    torch.testing.assert_close(native.float(), library.float(), rtol=2 ** -7, atol=2e-3)
    assert torch.equal(native.argmax(-1), library.argmax(-1))
    out, graph = torch.empty_like(native), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        out.copy_(stack.forward_decode_fused(hidden, fb.positions, fb, backend))
    for _ in range(3):
        hidden.copy_(hidden0)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, native)
