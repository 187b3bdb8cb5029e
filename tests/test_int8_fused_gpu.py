"""GPU parity of the fused W8A8 int8 decoder layer: int8-emitting producers against float64 and against the unfused
chain, the GEMM + consumer forms and the layer stack bit for bit against the unfused chain of the existing ops."""
import functools

import pytest
import torch

from test_int8_gpu import DTYPES, RTOL

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 1e-5


def ops():
    from iaas_sglang_amd import ops as _ops
    return _ops


def rows(M, W, dtype, seed, negative=True):
    """[M, W] of different row magnitudes; row 0 all zeros (M > 1), the last row all negative.  No row is so small
    that fp16's subnormal spacing (2^-25 absolute, outside the relative bound) comes near half an int8 step of it."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, W, generator=g) * torch.logspace(-0.5, 1, M)[:, None]).to(dtype)
    if negative:
        x[-1] = -x[-1].abs()
    if M > 1:
        x[0] = 0
    return x.to(DEV)


def check_quant(q, s, out, y64, dtype):
    """q * scale against float64: half an int8 step + the T roundings; the scale is absmax(out) / 127 exactly"""
    err = (q.double() * s.double() - y64).abs()
    bound = 0.5 * s.double() + 2 * RTOL[dtype] * y64.abs()
    print(f"worst err/bound {(err / bound.clamp_min(1e-300)).max():.3f}")
    assert bool((err <= bound).all())
    assert torch.equal(s.cpu(), out.cpu().float().abs().amax(dim=1, keepdim=True).clamp_min(1e-10) / 127)


@functools.lru_cache(maxsize=None)
def norm_case(M, H, dtype, residual):
    x, w = rows(M, H, dtype, M + H), (1 + 0.1 * torch.rand(H, generator=torch.Generator().manual_seed(H))).to(dtype).to(DEV)
    res = rows(M, H, dtype, M + H + 1) if residual else None
    res_f = res.clone() if residual else None
    return x, w, res, res_f, ops().rmsnorm_int8(x, w, EPS, residual=res_f, want_out=True)


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("H", [128, 4096, 8192])
@pytest.mark.parametrize("M", [1, 17, 130])
@pytest.mark.parametrize("dtype", DTYPES)
def test_rmsnorm_int8_vs_float64(dtype, M, H, residual):
    x, w, res, _, (q, s, out) = norm_case(M, H, dtype, residual)
    v = x.double() + (res.double() if residual else 0)
    y = v * torch.rsqrt((v * v).mean(dim=1, keepdim=True) + EPS) * w.double()
    check_quant(q, s, out, y, dtype)
    assert M == 1 or (not bool(q[0].any()) and bool((q[-1] == -127).any()))     # clamp path; negative maximum


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("H", [128, 4096, 8192])
@pytest.mark.parametrize("M", [1, 17, 130])
@pytest.mark.parametrize("dtype", DTYPES)
def test_rmsnorm_int8_equals_chain(dtype, M, H, residual):
    x, w, res, res_f, (q, s, out) = norm_case(M, H, dtype, residual)
    res_c = res.clone() if residual else None
    out_c = ops().rmsnorm(x, w, EPS, residual=res_c)
    q_c, s_c = ops().int8_quant_per_token(out_c)
    assert torch.equal(q, q_c) and torch.equal(s, s_c) and torch.equal(out, out_c)
    assert not residual or torch.equal(res_f, res_c)


@functools.lru_cache(maxsize=None)
def silu_case(M, I, dtype):
    x = torch.cat([rows(M, I, dtype, M + I, negative=False).abs(), rows(M, I, dtype, M + I + 1)], dim=1)
    return x, ops().silu_and_mul_int8(x, want_out=True)


@pytest.mark.parametrize("I", [64, 14336, 28672])
@pytest.mark.parametrize("M", [1, 17, 130])
@pytest.mark.parametrize("dtype", DTYPES)
def test_silu_and_mul_int8(dtype, M, I):
    x, (q, s, out) = silu_case(M, I, dtype)
    g, u = x[:, :I].double(), x[:, I:].double()
    check_quant(q, s, out, g * torch.sigmoid(g) * u, dtype)
    assert M == 1 or (not bool(q[0].any()) and bool((q[-1] == -127).any()))
    out_c = ops().silu_and_mul(x)
    q_c, s_c = ops().int8_quant_per_token(out_c)
    assert torch.equal(q, q_c) and torch.equal(s, s_c) and torch.equal(out, out_c)


def gemm_case(M, N, K):
    g = torch.Generator(device=DEV).manual_seed(M * 1000003 + N * 1009 + K)
    a = torch.randint(-128, 128, (M, K), generator=g, dtype=torch.int8, device=DEV)
    b = torch.randint(-128, 128, (N, K), generator=g, dtype=torch.int8, device=DEV)
    sa = torch.empty(M, 1, device=DEV).uniform_(1e-3, 2e-2, generator=g)
    sb = torch.empty(N, 1, device=DEV).uniform_(1e-4, 2e-3, generator=g)
    return a, b.t(), sa, sb


@pytest.mark.parametrize("M,N,K", [(1, 128, 64), (17, 4096, 4096), (130, 4096, 14336), (256, 8192, 1024)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_add_rmsnorm_equals_chain(dtype, M, N, K):
    a, b, sa, sb = gemm_case(M, N, K)
    res, w = rows(M, N, dtype, N), (1 + 0.1 * torch.rand(N, device=DEV)).to(dtype)
    res_c = res.clone()
    out_c = ops().rmsnorm(ops().int8_gemm(a, b, sa, sb, dtype), w, EPS, residual=res_c)
    q_c, s_c = ops().int8_quant_per_token(out_c)
    for want_q, want_out in ((True, False), (False, True), (True, True)):
        res_f = res.clone()
        out, q, s = ops().int8_gemm_add_rmsnorm(a, b, sa, sb, res_f, w, EPS, want_q, want_out)
        assert torch.equal(res_f, res_c)
        assert (out is None) == (not want_out) and (not want_out or torch.equal(out, out_c))
        assert (q is None) == (not want_q) and (not want_q or (torch.equal(q, q_c) and torch.equal(s, s_c)))


@pytest.mark.parametrize("Hq,Hkv,D,K", [(4, 1, 128, 192), (32, 8, 128, 4096), (8, 8, 64, 1024)])
@pytest.mark.parametrize("M", [1, 130])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_rope_kvwrite_equals_chain(dtype, M, Hq, Hkv, D, K):
    from iaas_sglang_amd.harness import rope_cache
    a, b, sa, sb = gemm_case(M, (Hq + 2 * Hkv) * D, K)
    g = torch.Generator().manual_seed(M + K)
    cos_sin = rope_cache(D, 512, 10000.0, DEV)
    positions = torch.randint(0, 512, (M,), generator=g).to(DEV)
    loc = (torch.randperm(M + 6, generator=g)[:M] + 1).to(DEV)
    pool0 = torch.randn(2, M + 7, Hkv, D, generator=g).to(dtype).to(DEV)
    qkv = ops().int8_gemm(a, b, sa, sb, dtype)
    q_c, k_c, v_c = qkv[:, :Hq * D], qkv[:, Hq * D:(Hq + Hkv) * D], qkv[:, (Hq + Hkv) * D:]
    ops().rope_neox_(q_c, k_c, positions, cos_sin, D)
    pool_c = pool0.clone()
    ops().kv_write(pool_c[0], pool_c[1], loc, k_c, v_c)
    pool_f = pool0.clone()
    q = ops().int8_gemm_rope_kvwrite(a, b, sa, sb, positions, cos_sin, pool_f[0], pool_f[1], loc, Hq, Hkv, D)
    assert torch.equal(q, q_c) and torch.equal(pool_f, pool_c)
    untouched = torch.ones(M + 7, dtype=torch.bool, device=DEV)
    untouched[loc] = False
    assert torch.equal(pool_f[:, untouched], pool0[:, untouched]) and not torch.equal(pool_f[:, loc], pool0[:, loc])


# (3, 4160, 1024): split-K slabs into the LDS-parked row kernel; the other three: S == 1 (T route) twice, slabs once
@pytest.mark.parametrize("M,I,K", [(1, 64, 64), (17, 1536, 4096), (130, 14336, 4096), (3, 4160, 1024)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_silu_mul_equals_chain(dtype, M, I, K):
    a, b, sa, sb = gemm_case(M, 2 * I, K)
    q_c, s_c = ops().int8_quant_per_token(ops().silu_and_mul(ops().int8_gemm(a, b, sa, sb, dtype)))
    q, s = ops().int8_gemm_silu_mul(a, b, sa, sb, dtype)
    assert torch.equal(q, q_c) and torch.equal(s, s_c) and bool(q.any())


@pytest.mark.parametrize("batch", [3, 130, 260])
def test_int8_layer_stack_fused_equals_unfused(batch):
    """Two layers of W8A8 int8 linears: logits and KV pools of the fused decode step equal the unfused sequence's.
    260 rows are past the fused forms: the general loop with the int8-emitting producers in front of plain GEMMs."""
    from iaas_sglang_amd import harness as H
    from iaas_sglang_amd.attention_backend import MiAttnBackend
    from iaas_sglang_amd.quantization.w8a8_int8 import W8A8Int8Config, W8A8Int8LinearMethod
    shape = H.ModelShape("int8-stack", 512, 2, 4, 1, 128, 1536, 1024, context_len=512)
    dtype, seq = torch.bfloat16, 40
    cfg = W8A8Int8Config.from_config({})
    runner = H.make_runner(shape, max_reqs=batch, ctx=seq + 8, pool_tokens=batch * seq, dtype=dtype, device=DEV, fill_kv=True)
    backend = MiAttnBackend(runner)
    stack = H.LlamaStack(shape, lambda: W8A8Int8LinearMethod(cfg), dtype, DEV, weight_range=0.02)
    fb = H.make_decode_batch(runner, backend, batch, seq, DEV, seed=3)
    hidden = torch.randn(batch, shape.hidden, generator=torch.Generator().manual_seed(1)).to(dtype).to(DEV)
    pool = runner.token_to_kv_pool
    snap = [b.clone() for b in pool.k_buffer + pool.v_buffer]
    logits, kv = [], []
    for fused in (False, True):
        for b, s0 in zip(pool.k_buffer + pool.v_buffer, snap):
            b.copy_(s0)
        H.LlamaStack.fuse_decode_layer = fused
        try:
            backend.init_forward_metadata(fb)
            assert stack._fused_decode8_ok(hidden, fb) == (fused and batch <= 256)
            logits.append(stack.forward(hidden.clone(), fb.positions, fb, backend))
        finally:
            H.LlamaStack.fuse_decode_layer = True
        kv.append([b.clone() for b in pool.k_buffer + pool.v_buffer])
    assert bool(torch.isfinite(logits[1].float()).all()) and bool((logits[1] != logits[1][0, 0]).any())
    assert torch.equal(logits[0], logits[1])
    assert all(torch.equal(x, y) for x, y in zip(*kv))


def test_fused_forms_refuse():
    from iaas_sglang_amd._lib import MI_BF16, MiHotpathError, check, lib
    dtype = torch.bfloat16
    with pytest.raises(MiHotpathError):                       # M = 257: beyond the decode kernel's pass
        ops().int8_gemm_silu_mul(*gemm_case(257, 128, 64), dtype)
    with pytest.raises(MiHotpathError):                       # I = 72 cannot be the next GEMM's K
        ops().int8_gemm_silu_mul(*gemm_case(4, 144, 64), dtype)
    M, N, K = 4, 128, 64
    a, b, sa, sb = gemm_case(M, N, K)
    need = lib.mi_int8_gemm_fused_workspace_bytes(M, N, K)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    q, s = torch.empty(M, N // 2, dtype=torch.int8, device=DEV), torch.empty(M, device=DEV)
    with pytest.raises(MiHotpathError, match="workspace"):
        check(lib.mi_int8_gemm_silu_mul_int8(a.data_ptr(), b.data_ptr(), sa.data_ptr(), sb.data_ptr(), q.data_ptr(),
                                             s.data_ptr(), M, N // 2, K, K, K, MI_BF16, ws.data_ptr(), need - 1,
                                             torch.cuda.current_stream().cuda_stream), "short workspace")
