"""GPU parity at head_dim 256 (Gemma-class heads): the decode and extend kernels through the C ABI
(iaas_sglang_amd.ops -> libmi_hotpath.so) against fp32 math (oracle.attention)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import attention as oa  # noqa: E402  (checker only)

DEV = "cuda"
D = 256
SM = D ** -0.5
BF, HF = torch.bfloat16, torch.float16


def _dtol(dtype):
    return dict(atol=2e-3, rtol=2 ** -7 if dtype == BF else 2 ** -9)


def _xtol(dtype):
    return dict(atol=4e-3, rtol=2 ** -6 if dtype == BF else 2 ** -8)


def _pool(lens, Hkv, dtype, seed, extra=0):
    """Scattered slots for requests of `lens` keys (+ `extra` free slots): k, v pools, req_to_token, generator."""
    g = torch.Generator().manual_seed(seed)
    slots = sum(lens) + extra + 1
    k = torch.randn(slots, Hkv, D, generator=g).to(dtype)
    v = torch.randn(slots, Hkv, D, generator=g).to(dtype)
    perm = torch.randperm(slots - 1, generator=g) + 1
    r2t = torch.zeros(len(lens), max(lens) + 2, dtype=torch.int32)
    off = 0
    for i, L in enumerate(lens):
        r2t[i, :L] = perm[off:off + L].to(torch.int32)
        off += L
    return k, v, r2t, g


def _indices(ops, r2t, lens):
    sl = torch.tensor(lens, dtype=torch.int64, device=DEV)
    indptr = ops.kv_indptr(sl)
    idx = torch.empty(max(1, sum(lens)), dtype=torch.int32, device=DEV)
    ops.kv_indices(r2t.to(DEV), torch.arange(len(lens), device=DEV), sl, indptr, idx)
    return indptr, idx


def _decode(ops, q, k, v, indptr, idx, ns, cap=0.0, **kw):
    B, Hq, _ = q.shape
    ws = torch.empty(max(1, ops.decode_workspace_numel(B, Hq, D, ns)), dtype=torch.float32, device=DEV)
    out = torch.empty_like(q)
    ops.decode_attention(q, k, v, out, indptr, idx, SM, cap, ns, ws, **kw)
    return out


@pytest.mark.parametrize("Hq,Hkv,dtype", [(16, 8, BF), (16, 16, HF), (8, 1, BF), (4, 1, HF)])   # groups 2, 1, 8, 4
def test_decode_ragged_vs_oracle(Hq, Hkv, dtype):
    from iaas_sglang_amd import ops
    lens = [1, 2, 15, 16, 17, 31, 32, 33, 100, 511, 512, 700]
    k, v, r2t, g = _pool(lens, Hkv, dtype, 1)
    q = torch.randn(len(lens), Hq, D, generator=g).to(dtype)
    ref = oa.decode_fp32(q, k, v, r2t, torch.arange(len(lens)), torch.tensor(lens), scaling=SM)
    indptr, idx = _indices(ops, r2t, lens)
    for ns in (1, 4, 16):      # 16: most requests leave empty splits
        out = _decode(ops, q.to(DEV), k.to(DEV), v.to(DEV), indptr, idx, ns)
        torch.testing.assert_close(out.cpu().float(), ref, **_dtol(dtype))


def test_decode_logit_cap_and_spiked_max():
    from iaas_sglang_amd import ops
    lens, Hq, Hkv = [300, 90], 8, 2
    k, v, r2t, g = _pool(lens, Hkv, BF, 4)
    q = torch.randn(2, Hq, D, generator=g).to(BF)
    k[r2t[0, 250].item()] = (q[0, 0] * 3).to(BF)     # a huge logit late in the sequence: the deferred-rescale branch
    indptr, idx = _indices(ops, r2t, lens)
    for cap in (0.0, 30.0):
        ref = oa.decode_fp32(q, k, v, r2t, torch.arange(2), torch.tensor(lens), scaling=SM, logit_cap=cap)
        for ns in (1, 2):
            out = _decode(ops, q.to(DEV), k.to(DEV), v.to(DEV), indptr, idx, ns, cap)
            torch.testing.assert_close(out.cpu().float(), ref, **_dtol(BF))


def test_decode_fixed_chunks_with_work_list():
    from iaas_sglang_amd import ops
    lens, Hq, Hkv, chunk, splits = [1, 700, 130, 17, 64, 65, 300, 511], 16, 8, 64, 8
    k, v, r2t, g = _pool(lens, Hkv, BF, 72)
    q = torch.randn(len(lens), Hq, D, generator=g).to(BF)
    ref = oa.decode_fp32(q, k, v, r2t, torch.arange(len(lens)), torch.tensor(lens), scaling=SM)
    indptr, idx = _indices(ops, r2t, lens)
    work = []
    for b, S in enumerate(lens):     # the kernel's split rule; only the non-empty (request, split) pairs are launched
        per = max((-(-S // splits) + 15) // 16 * 16, chunk)
        work += [(b, s) for s in range(splits) if s * per < S]
    work = torch.tensor(work, dtype=torch.int32, device=DEV)
    out = _decode(ops, q.to(DEV), k.to(DEV), v.to(DEV), indptr, idx, splits, split_chunk=chunk, work=work)
    torch.testing.assert_close(out.cpu().float(), ref, **_dtol(BF))


def test_decode_paged_and_fp8_output_are_bit_identical():
    from iaas_sglang_amd import ops
    P, Hq, Hkv = 16, 16, 8
    lens = [1, P, P + 1, 5 * P - 3, 300, 33]
    g = torch.Generator().manual_seed(16)
    npages = [-(-n // P) for n in lens]
    pages = torch.randperm(sum(npages) + 3, generator=g)[: sum(npages)] + 1
    r2t = torch.zeros(len(lens), max(lens) + 2, dtype=torch.int32)
    off = 0
    for i, n in enumerate(lens):
        sl = (pages[off: off + npages[i]].view(-1, 1) * P + torch.arange(P).view(1, -1)).reshape(-1)
        r2t[i, :n] = sl[:n].to(torch.int32)
        off += npages[i]
    slots = (int(pages.max()) + 1) * P
    k = torch.randn(slots, Hkv, D, generator=g).to(BF).to(DEV)
    v = torch.randn(slots, Hkv, D, generator=g).to(BF).to(DEV)
    q = torch.randn(len(lens), Hq, D, generator=g).to(BF).to(DEV)
    sl = torch.tensor(lens, dtype=torch.int64, device=DEV)
    pi, px = ops.kv_page_tables(r2t.to(DEV), torch.arange(len(lens), device=DEV), sl, P)
    indptr, idx = _indices(ops, r2t, lens)
    qs = torch.tensor([0.05], device=DEV)
    for ns in (1, 4):
        ws = torch.empty(max(1, ops.decode_workspace_numel(len(lens), Hq, D, ns)), dtype=torch.float32, device=DEV)
        o_tok = _decode(ops, q, k, v, indptr, idx, ns)
        o_pg = torch.empty_like(q)
        ops.decode_attention_paged(q, k, v, indptr, pi, px, P, SM, 0.0, ns, ws, o=o_pg)
        assert torch.equal(o_pg, o_tok)
        o8 = torch.empty(len(lens), Hq * D, dtype=torch.float8_e4m3fn, device=DEV)
        ops.decode_attention_fp8out(q, k, v, o8, qs, indptr, idx, SM, 0.0, ns, ws)
        want, _ = ops.fp8_quant_per_tensor(o_tok.view(len(lens), Hq * D), qs)
        assert torch.equal(o8.view(torch.uint8), want.view(torch.uint8))
    ref = oa.decode_fp32(q.cpu(), k.cpu(), v.cpu(), r2t, torch.arange(len(lens)), torch.tensor(lens), scaling=SM)
    torch.testing.assert_close(o_tok.cpu().float(), ref, **_dtol(BF))


def _extend(ops, q, k_new, v_new, kc, vc, r2t, pre, ext, causal=True, cap=0.0, window=-1, splits=1):
    d = lambda t: t.to(DEV)
    kc, vc = d(kc).clone(), d(vc).clone()
    loc = torch.cat([r2t[i, pre[i]:pre[i] + ext[i]] for i in range(len(pre))]).to(torch.int64)
    ops.kv_write(kc, vc, d(loc), d(k_new), d(v_new))
    kvp, idx = _indices(ops, r2t, pre)
    qo = ops.kv_indptr(torch.tensor(ext, dtype=torch.int32, device=DEV))
    out = torch.empty_like(d(q))
    if splits > 1:
        ops.extend_attention_splitkv(d(q), d(k_new), d(v_new), out, kc, vc, qo, kvp, idx, max(ext), SM, splits, None,
                                     cap, causal, window)
    else:
        ops.extend_attention(d(q), d(k_new), d(v_new), out, kc, vc, qo, kvp, idx, max(ext), SM, cap, causal, window)
    torch.cuda.synchronize()
    return out.cpu(), kc.cpu(), vc.cpu()


@pytest.mark.parametrize("Hq,Hkv,dtype", [(16, 8, BF), (4, 4, HF), (8, 1, BF)])
def test_extend_ragged_vs_oracle(Hq, Hkv, dtype):
    from iaas_sglang_amd import ops
    pre, ext = [0, 0, 64, 300, 33, 1, 129, 0], [1, 130, 17, 1, 64, 200, 31, 65]
    lens = [a + b for a, b in zip(pre, ext)]
    kc, vc, r2t, g = _pool(lens, Hkv, dtype, 7)
    r2t[4, :33] = r2t[3, :33]        # shared radix prefix
    E = sum(ext)
    q, k_new, v_new = (torch.randn(E, h, D, generator=g).to(dtype) for h in (Hq, Hkv, Hkv))
    for causal, cap, window in [(True, 0.0, -1), (False, 0.0, -1), (True, 50.0, -1), (True, 0.0, 40)]:
        ref = None
        for splits in (1, 3, 16):    # 16: more splits than key tiles for most blocks
            out, kca, vca = _extend(ops, q, k_new, v_new, kc, vc, r2t, pre, ext, causal, cap, window, splits)
            if ref is None:
                ref = oa.extend_fp32(q, kca, vca, r2t, torch.arange(len(lens)), torch.tensor(lens), torch.tensor(pre),
                                     torch.tensor(ext), scaling=SM, causal=causal, logit_cap=cap, sliding_window=window)
            torch.testing.assert_close(out.float(), ref, **_xtol(dtype))


@pytest.mark.parametrize("skip_prefix", [True, False])
def test_extend_tree_mask_vs_oracle(skip_prefix):
    from iaas_sglang_amd import ops
    B, nd, Hq, Hkv = 3, 4, 16, 8
    seq = [37, 5, 80]
    lens = [s + nd for s in seq]
    kc, vc, r2t, g = _pool(lens, Hkv, BF, 34)
    q, k, v = (torch.randn(B * nd, h, D, generator=g).to(BF) for h in (Hq, Hkv, Hkv))
    new_loc = torch.cat([r2t[i, seq[i]:lens[i]] for i in range(B)]).to(torch.int64)
    kc[new_loc], vc[new_loc] = k, v                    # the oracle reads the new rows back from the pool
    masks, tril, mptr = [], [], [0]
    for i in range(B):
        m = torch.rand(nd, lens[i], generator=g) < 0.6
        m[torch.arange(nd), seq[i] + torch.arange(nd)] = True     # a node always sees itself
        m[:, 0] = True
        t = torch.ones(nd, lens[i], dtype=torch.bool)
        t[:, seq[i]:] = torch.tril(torch.ones(nd, nd, dtype=torch.bool))
        masks.append(m.reshape(-1)); tril.append(t.reshape(-1)); mptr.append(mptr[-1] + nd * lens[i])
    custom_mask, mask_indptr = torch.cat(masks), torch.tensor(mptr, dtype=torch.int64)
    ref = oa.extend_fp32(q, kc, vc, r2t, torch.arange(B), torch.tensor(lens), torch.tensor(seq), torch.full((B,), nd), SM,
                         causal=True, custom_mask=custom_mask, mask_indptr=mask_indptr, skip_prefix_custom_mask=skip_prefix)
    kvp, idx = _indices(ops, r2t, seq)
    qo = torch.arange(0, (B + 1) * nd, nd, dtype=torch.int32, device=DEV)
    args = (q.to(DEV), k.to(DEV), v.to(DEV))
    o, o_c, o_t = (torch.empty_like(args[0]) for _ in range(3))
    ops.extend_attention_masked(*args, o, kc.to(DEV), vc.to(DEV), qo, kvp, idx, custom_mask.to(DEV), mask_indptr.to(DEV), nd,
                                SM, 0.0, skip_prefix)
    torch.testing.assert_close(o.cpu().float(), ref, **_xtol(BF))
    # a lower-triangular mask is the causal rule, bit for bit
    ops.extend_attention(*args, o_c, kc.to(DEV), vc.to(DEV), qo, kvp, idx, nd, SM, 0.0, True, -1)
    ops.extend_attention_masked(*args, o_t, kc.to(DEV), vc.to(DEV), qo, kvp, idx, torch.cat(tril).to(DEV),
                                mask_indptr.to(DEV), nd, SM, 0.0, skip_prefix)
    assert torch.equal(o_c.view(torch.int16), o_t.view(torch.int16))


def test_extend_len1_equals_decode():
    """An extend of one token equals decode on the same pool, within the DECODE tolerance (atol 2e-3, rtol 2^-7).
    With P rounded to bf16 for the P.V MFMA this missed on the request with 2 keys (3 of 20,480 elements, greatest
    absolute difference 2.197e-3 against 2e-3); extends of <= 16 tokens therefore carry P as bf16 hi + lo (PSPLIT)."""
    from iaas_sglang_amd import ops
    pre, Hq, Hkv = [7, 100, 513, 64, 1], 16, 8
    ext = [1] * len(pre)
    lens = [p + 1 for p in pre]
    kc, vc, r2t, g = _pool(lens, Hkv, BF, 3)
    q, k_new, v_new = (torch.randn(len(pre), h, D, generator=g).to(BF) for h in (Hq, Hkv, Hkv))
    out_e, kca, vca = _extend(ops, q, k_new, v_new, kc, vc, r2t, pre, ext)
    indptr, idx = _indices(ops, r2t, lens)
    out_d = _decode(ops, q.to(DEV), kca.to(DEV), vca.to(DEV), indptr, idx, 1)
    torch.testing.assert_close(out_e.float(), out_d.cpu().float(), **_dtol(BF))


def test_refusals_before_any_launch():
    from iaas_sglang_amd import ops
    from iaas_sglang_amd._lib import MiHotpathError
    lens = [40, 3]
    k, v, r2t, g = _pool(lens, 1, BF, 9)
    indptr, idx = _indices(ops, r2t, lens)
    q16 = torch.randn(2, 16, D, generator=g).to(BF).to(DEV)
    with pytest.raises(MiHotpathError, match="rc=-2"):      # group 16: 256 accumulator registers
        ops.decode_attention(q16, k.to(DEV), v.to(DEV), torch.empty_like(q16), indptr, idx, SM)
    k8, v8 = k.to(DEV).to(torch.float8_e4m3fn), v.to(DEV).to(torch.float8_e4m3fn)
    q = q16[:, :4].contiguous()
    with pytest.raises(MiHotpathError, match="rc=-2"):      # fp8 pool: head_dim 128 only
        ops.decode_attention_fp8kv(q, k8, v8, indptr, idx, SM, o=torch.empty_like(q))
    qo = torch.tensor([0, 1, 2], dtype=torch.int32, device=DEV)
    kx = torch.zeros(2, 1, D, dtype=BF, device=DEV)
    with pytest.raises(MiHotpathError, match="rc=-2"):
        ops.extend_attention_fp8kv(q, kx, kx, torch.empty_like(q), k8, v8, 1.0, 1.0, qo, indptr, idx, 1, SM)


def _gemma_backend(pool_tokens):
    """Runner + backend with GEMMA2_9B heads (one layer's pool, random contents), a windowed and a full layer, cap 50."""
    import dataclasses
    from iaas_sglang_amd import harness as H
    from iaas_sglang_amd.attention_backend import MiAttnBackend
    shape = dataclasses.replace(H.GEMMA2_9B, layers=1)
    runner = H.make_runner(shape, max_reqs=8, ctx=2048, pool_tokens=pool_tokens, dtype=BF, device=DEV, fill_kv=True)
    runner.sliding_window_size = 100
    backend = MiAttnBackend(runner)
    layers = [H.AttnLayer(shape.num_heads, D, SM, shape.num_kv_heads, 0, logit_cap=50.0) for _ in range(2)]
    layers[0].sliding_window_size = 100
    return H, shape, runner, backend, layers


@pytest.mark.parametrize("graph", [False, True])
def test_backend_gemma2_layer_pair_decode(graph):
    H, shape, runner, backend, (win_layer, full_layer) = _gemma_backend(2400)
    Hq, W, lens = shape.num_heads, 100, [300, 17, 1500, 64, 101, 102]
    bs = len(lens)
    rpi = torch.zeros(bs, dtype=torch.int64, device=DEV)
    seq_lens = torch.ones(bs, dtype=torch.int64, device=DEV)
    q = torch.zeros(bs, Hq * D, dtype=BF, device=DEV)
    if graph:
        backend.init_cuda_graph_state(bs, bs)
        fbg = H.make_decode_batch(runner, backend, bs, 5, DEV, seed=1)
        fbg.req_pool_indices, fbg.seq_lens = rpi, seq_lens
        backend.init_forward_metadata_capture_cuda_graph(bs, bs, rpi, seq_lens, None, H.ForwardMode.DECODE, None)
        torch.cuda.synchronize()
        cg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(cg):
            o_win_g = backend.forward(q, None, None, win_layer, fbg, save_kv_cache=False)
            o_full_g = backend.forward(q, None, None, full_layer, fbg, save_kv_cache=False)
    fb = H.make_decode_batch(runner, backend, bs, 0, DEV, seed=20, ragged=torch.tensor(lens))
    qc = torch.randn(bs, Hq * D, generator=torch.Generator().manual_seed(8)).to(BF)
    q.copy_(qc)
    if graph:
        rpi.copy_(fb.req_pool_indices); seq_lens.copy_(fb.seq_lens)
        backend.init_forward_metadata_replay_cuda_graph(bs, rpi, seq_lens, sum(lens), None, H.ForwardMode.DECODE, None,
                                                        fb.seq_lens_cpu)
        outs = []
        for _ in range(2):       # two replays: the second must reproduce the first
            cg.replay()
            torch.cuda.synchronize()
            outs.append((o_win_g.clone(), o_full_g.clone()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        o_win, o_full = outs[1]
    else:
        backend.init_forward_metadata(fb)
        o_win = backend.forward(q, None, None, win_layer, fb, save_kv_cache=False)
        o_full = backend.forward(q, None, None, full_layer, fb, save_kv_cache=False)
    pool = runner.token_to_kv_pool
    kc, vc = pool.k_buffer[0].cpu(), pool.v_buffer[0].cpu()
    r2t, sl, rp = runner.req_to_token_pool.req_to_token.cpu(), torch.tensor(lens), fb.req_pool_indices.cpu()
    want_full = oa.decode_fp32(qc.view(bs, Hq, D), kc, vc, r2t, rp, sl, scaling=SM, logit_cap=50.0)
    want_win = oa.extend_fp32(qc.view(bs, Hq, D), kc, vc, r2t, rp, sl, sl - 1, torch.ones(bs, dtype=torch.int64),
                              scaling=SM, causal=True, logit_cap=50.0, sliding_window=W)
    torch.testing.assert_close(o_full.view(bs, Hq, D).cpu().float(), want_full, atol=4e-3, rtol=2 ** -7)
    torch.testing.assert_close(o_win.view(bs, Hq, D).cpu().float(), want_win, atol=4e-3, rtol=2 ** -7)


def test_backend_gemma2_layer_pair_extend():
    H, shape, runner, backend, layers = _gemma_backend(700)
    Hq, Hkv = shape.num_heads, shape.num_kv_heads
    pre, ext = [0, 64, 300, 33], [130, 17, 1, 64]
    fb = H.make_extend_batch(runner, backend, pre, ext, DEV, seed=2)
    g = torch.Generator().manual_seed(11)
    E = sum(ext)
    q, k, v = (torch.randn(E, h, D, generator=g).to(BF) for h in (Hq, Hkv, Hkv))
    backend.init_forward_metadata(fb)
    for layer in layers:
        o = backend.forward(q.view(E, Hq * D).to(DEV), k.to(DEV), v.to(DEV), layer, fb)
        pool = runner.token_to_kv_pool
        ref = oa.extend_fp32(q, pool.k_buffer[0].cpu(), pool.v_buffer[0].cpu(), runner.req_to_token_pool.req_to_token.cpu(),
                             fb.req_pool_indices.cpu(), fb.seq_lens.cpu(), torch.tensor(pre), torch.tensor(ext), scaling=SM,
                             causal=True, logit_cap=50.0, sliding_window=layer.sliding_window_size)
        torch.testing.assert_close(o.view(E, Hq, D).cpu().float(), ref, atol=4e-3, rtol=2 ** -7)
