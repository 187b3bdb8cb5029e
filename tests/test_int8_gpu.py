"""GPU parity of the W8A8 int8 path: per-token quant (bit-exact), mi_int8_gemm against float64, the linear method."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
RTOL = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def ops():
    from iaas_sglang_amd import ops as _ops
    return _ops


def quant_ref(x):
    """per_token_quant_int8 in fp32 on the CPU; the rounding is ties away from zero.  (torch evaluates `127 / absmax`
    as absmax.reciprocal() * 127, and so does the kernel.)"""
    absmax = x.float().abs().amax(dim=1, keepdim=True).clamp_min(1e-10)
    v = x.float() * (127 / absmax)
    return (v.sign() * (v.abs().double() + 0.5).floor()).to(torch.int8), absmax / 127


@functools.lru_cache(maxsize=None)
def gemm_case(M, N, K):
    g = torch.Generator().manual_seed(M * 1000003 + N * 1009 + K)
    a = torch.randint(-128, 128, (M, K), generator=g, dtype=torch.int8)
    b = torch.randint(-128, 128, (N, K), generator=g, dtype=torch.int8)
    sa = torch.empty(M).uniform_(1e-3, 2e-2, generator=g)
    sb = torch.empty(N).uniform_(1e-4, 2e-3, generator=g)
    ref = (a.double() @ b.double().T) * sa.double()[:, None] * sb.double()[None, :]
    return a, b, sa, sb, torch.randn(N, generator=g), ref


def check_gemm(a, b, sa, sb, bias, ref, dtype):
    """three fp32 roundings + the output rounding; atol covers the cancellation against the bias"""
    bias_t = None if bias is None else bias.to(dtype)
    out = ops().int8_gemm(a.to(DEV), b.to(DEV).t(), sa.to(DEV), sb.to(DEV), dtype, None if bias is None else bias_t.to(DEV))
    want = ref if bias is None else ref + bias_t.double()
    err = (out.cpu().double() - want).abs()
    bound = 2.0 ** -20 * ref.abs().max() + RTOL[dtype] * want.abs()
    print(f"max err {err.max():.3e}, worst err/bound {(err / bound).max():.3f}")
    assert out.shape == ref.shape and out.dtype == dtype
    assert bool((err <= bound).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,K", [(1, 64), (3, 14336), (128, 512), (130, 4096)])
def test_quant_bit_exact(dtype, M, K):
    g = torch.Generator().manual_seed(M + K)
    x = (torch.randn(M, K, generator=g) * torch.logspace(-3, 2, M)[:, None]).to(dtype)
    x[-1] = -x[-1].abs()                  # the row's maximum is negative
    if M > 1:
        x[0] = 0                          # absmax clamps to 1e-10, q = 0
    q, s = ops().int8_quant_per_token(x.to(DEV))
    q_ref, s_ref = quant_ref(x)
    assert s.shape == (M, 1) and torch.equal(s.cpu(), s_ref)
    assert torch.equal(q.cpu(), q_ref)


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K", [
    (1, 16, 64),            # a single MFMA depth: only the half phase
    (17, 72, 192),          # ragged M, N no multiple of 16, a whole phase + the half phase
    (128, 128, 1024),
    (128, 4096, 4096),      # split-K engages
    (129, 200, 256),        # the 256-row form of the decode kernel, ragged column block
    (300, 136, 512),        # tile kernel, ragged in both dimensions
    (513, 256, 128),
    (8, 128, 2624),         # split-K whose last slice is the half phase alone
])
def test_gemm_vs_float64(M, N, K, dtype, bias):
    a, b, sa, sb, bv, ref = gemm_case(M, N, K)
    check_gemm(a, b, sa, sb, bv if bias else None, ref, dtype)


@pytest.mark.parametrize("aval", [-128, 127])
def test_gemm_extremes(aval):
    """|acc| = 6.7e7 is far past fp32's exact integers; a saturating or wrongly signed MFMA variant shows here"""
    M, N, K = 16, 16, 4096
    a = torch.full((M, K), aval, dtype=torch.int8)
    b = torch.full((N, K), -128, dtype=torch.int8)
    ref = torch.full((M, N), float(aval) * -128.0 * K, dtype=torch.float64)
    check_gemm(a, b, torch.ones(M), torch.ones(N), None, ref, torch.bfloat16)


@pytest.mark.parametrize("M,N,K", [(128, 4096, 4096), (64, 256, 14336)])
def test_split_k_is_exact(M, N, K):
    from iaas_sglang_amd._lib import MI_BF16, lib
    a, b, sa, sb, _, _ = gemm_case(M, N, K)
    a, b, sa, sb = a.to(DEV), b.to(DEV), sa.to(DEV), sb.to(DEV)
    assert lib.mi_int8_gemm_workspace_bytes(M, N, K) > 0
    split = ops().int8_gemm(a, b.t(), sa, sb, torch.bfloat16)
    plain = torch.empty_like(split)
    rc = lib.mi_int8_gemm(a.data_ptr(), b.data_ptr(), sa.data_ptr(), sb.data_ptr(), None, plain.data_ptr(), M, N, K, K, K,
                          N, MI_BF16, None, 0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and torch.equal(split, plain)


def test_w8a8_int8_linear_method():
    """create_weights -> load (two fused shards) -> process_weights_after_loading -> apply on [2, 5, K]"""
    from iaas_sglang_amd.quantization import W8A8Int8Config
    g = torch.Generator().manual_seed(5)
    K, widths, dtype = 256, [96, 32], torch.bfloat16
    N = sum(widths)

    class FakeLinear(torch.nn.Module):
        output_partition_sizes = widths
    lin = FakeLinear()
    method = W8A8Int8Config.from_config({}).get_quant_method(lin, "model.layers.0.self_attn.qkv_proj")
    method.create_weights(lin, K, widths, K, N, dtype, weight_loader=None)
    lin = lin.to(DEV)
    wq = torch.randint(-127, 128, (N, K), generator=g, dtype=torch.int8)
    ws = torch.empty(N, 1).uniform_(1e-4, 2e-3, generator=g)
    lin.weight.data.copy_(wq)
    lin.weight_scale.data.copy_(ws)
    method.process_weights_after_loading(lin)
    x = torch.randn(2, 5, K, generator=g).to(dtype)
    bias = torch.randn(N, generator=g).to(dtype)
    y = method.apply(lin, x.to(DEV), bias.to(DEV))
    xq, xs = quant_ref(x.reshape(-1, K))
    nobias = (xq.double() @ wq.double().T) * xs.double() * ws.double().T
    ref = (nobias + bias.double()).reshape(2, 5, N)
    assert y.shape == (2, 5, N) and y.dtype == dtype
    err = (y.cpu().double() - ref).abs()
    assert bool((err <= 2.0 ** -20 * nobias.abs().max() + RTOL[dtype] * ref.abs()).all())
