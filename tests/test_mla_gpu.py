"""GPU parity of MLA attention (mi_mla_attn via ops, MLATokenToKVPool, MiAttnBackend) against float64 math written out here."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
DQ, DV = 576, 512
SM = DQ ** -0.5
BF, HF = torch.bfloat16, torch.float16


def _tol(dtype):
    """fp16: the decode tolerances of test_attention_d256_gpu.py.  bf16: P goes into the P.V MFMA rounded to bf16, up to
    2.4e-3 absolute on near-zero outputs of short rows (measured once): atol 4e-3, under twice that."""
    return dict(atol=4e-3, rtol=2 ** -7) if dtype == BF else dict(atol=2e-3, rtol=2 ** -9)


def _pool(lens, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    slots = sum(lens) + 1
    kv = torch.randn(slots, 1, DQ, generator=g).to(dtype)
    perm = torch.randperm(slots - 1, generator=g) + 1
    r2t = torch.zeros(len(lens), max(lens) + 2, dtype=torch.int32)
    off = 0
    for i, L in enumerate(lens):
        r2t[i, :L] = perm[off:off + L].to(torch.int32)
        off += L
    return kv, r2t, g


def _ref(q, kv, r2t, rows):
    """float64: row t = (request b, n keys) attends kv[req_to_token[b, :n]]; the value is the first 512 dims of the key."""
    out = []
    for t, (b, n) in enumerate(rows):
        k = kv[r2t[b, :n].long(), 0].double()
        out.append(torch.softmax(q[t].double() @ k.T * SM, -1) @ k[:, :DV])
    return torch.stack(out).float()


def _indices(r2t, lens):
    idx = torch.cat([r2t[i, :n] for i, n in enumerate(lens)] + [r2t[0, :1]])
    return torch.tensor([0] + lens).cumsum(0).int().to(DEV), idx.to(DEV)


def _run(q, kv, indptr, idx, ns=1, qo=None, **kw):
    from iaas_sglang_amd import ops
    T, H, _ = q.shape
    ws = torch.empty(max(1, ops.decode_workspace_numel(T, H, DV, ns)), dtype=torch.float32, device=DEV)
    o = torch.empty(T, H, DV, dtype=q.dtype, device=DEV)
    return ops.mla_attention(q.to(DEV), kv.to(DEV), o, indptr, idx, SM, qo, ns, ws, **kw).cpu()


@pytest.mark.parametrize("H,dtype", [(16, BF), (40, HF), (8, BF)])   # one block, three with a partial last, a partial one
def test_decode_vs_float64(H, dtype):
    lens = [1, 2, 15, 16, 17, 63, 64, 65, 127, 129, 700]
    kv, r2t, g = _pool(lens, dtype, 1)
    q = torch.randn(len(lens), H, DQ, generator=g).to(dtype)
    ref, (indptr, idx) = _ref(q, kv, r2t, list(enumerate(lens))), _indices(r2t, lens)
    for ns in (1, 4, 16):      # 16: most rows leave empty splits
        torch.testing.assert_close(_run(q, kv, indptr, idx, ns).float(), ref, **_tol(dtype))


def test_decode_fixed_chunks_work_list_and_plan():
    lens, H, chunk, splits = [1, 700, 130, 17, 64, 65, 300, 0], 16, 64, 16
    kv, r2t, g = _pool(lens, BF, 72)
    q = torch.randn(len(lens), H, DQ, generator=g).to(BF)
    ref, (indptr, idx) = _ref(q, kv, r2t, list(enumerate(lens))), _indices(r2t, lens)
    # the kernel's split rule; only the non-empty (row, split) pairs are launched
    work = [(b, s) for b, S in enumerate(lens) for s in range(splits) if s * max((-(-S // splits) + 15) // 16 * 16, chunk) < S]
    work = torch.tensor(work, dtype=torch.int32, device=DEV)
    out = _run(q, kv, indptr, idx, splits, split_chunk=chunk, work=work)
    torch.testing.assert_close(out.float(), ref, **_tol(BF))
    plan = torch.tensor([work.shape[0], splits, chunk, 0], dtype=torch.int32, device=DEV)
    pad = torch.cat([work, torch.zeros(5, 2, dtype=torch.int32, device=DEV)])     # capacity beyond num_work: those exit
    assert torch.equal(_run(q, kv, indptr, idx, splits, work=(pad, plan)), out)


def test_decode_spiked_max_late_in_the_sequence():
    lens, H = [300, 90], 16
    kv, r2t, g = _pool(lens, BF, 4)
    q = torch.randn(2, H, DQ, generator=g).to(BF)
    kv[r2t[0, 250].item(), 0] = (q[0, 0] * 3).to(BF)     # tile 3, wave 3: every wave rescales by the exchanged maximum
    ref, (indptr, idx) = _ref(q, kv, r2t, list(enumerate(lens))), _indices(r2t, lens)
    for ns in (1, 2):
        torch.testing.assert_close(_run(q, kv, indptr, idx, ns).float(), ref, **_tol(BF))


def test_extend_causal_limit_and_decode_bits():
    H, pre, ext = 16, [0, 5, 64, 130], [1, 17, 64, 3]
    lens = [p + e for p, e in zip(pre, ext)]
    kv, r2t, g = _pool(lens, BF, 9)
    q = torch.randn(sum(ext), H, DQ, generator=g).to(BF)
    rows = [(b, pre[b] + j + 1) for b in range(len(ext)) for j in range(ext[b])]
    ref, (indptr, idx) = _ref(q, kv, r2t, rows), _indices(r2t, lens)
    qo = torch.tensor([0, 1, 18, 82, 85], dtype=torch.int32, device=DEV)
    for ns in (1, 3):
        torch.testing.assert_close(_run(q, kv, indptr, idx, ns, qo).float(), ref, **_tol(BF))
    # one request (60 cached + 6 new keys, n_t crosses the tile edge): row j = a decode call over the first n_t keys
    kv, r2t, g = _pool([66], BF, 10)
    q = torch.randn(6, H, DQ, generator=g).to(BF)
    indptr, idx = _indices(r2t, [66])
    out = _run(q, kv, indptr, idx, 1, torch.tensor([0, 6], dtype=torch.int32, device=DEV))
    for j in range(6):
        cut = torch.tensor([0, 61 + j], dtype=torch.int32, device=DEV)
        assert torch.equal(_run(q[j:j + 1], kv, cut, idx), out[j:j + 1])


def _backend(H_, B, dtype):
    from iaas_sglang_amd import attention_backend as AB, harness as H, mem_cache as MC
    runner = H.make_runner(H.TINY, max_reqs=B, ctx=512, pool_tokens=1024, dtype=dtype, device=DEV)
    runner.model_config.num_attention_heads = H_
    runner.token_to_kv_pool = MC.MLATokenToKVPool(1024, 1, dtype, DV, DQ - DV, 1, DEV)
    runner.req_to_token_pool = MC.ReqToTokenPool(B, 512, DEV)
    layer = H.AttnLayer(H_, DQ, SM, 1, 0)
    layer.v_head_dim = DV
    return H, runner, AB.MiAttnBackend(runner), layer


def test_backend_extend_decode_and_graph_replay():
    Hq, ext, dtype = 16, [100, 64, 5], BF
    (B, E), (H, runner, backend, layer) = (len(ext), sum(ext)), _backend(Hq, len(ext), dtype)
    pool, r2t = runner.token_to_kv_pool, runner.req_to_token_pool.req_to_token
    g = torch.Generator().manual_seed(4)
    slots = (torch.randperm(1000, generator=g) + 1).to(DEV)
    loc, new = slots[:E], slots[E:E + B]
    for i, e in enumerate(ext):      # the extend's slots, then the decode step's
        r2t[i, :e + 1] = torch.cat([loc[sum(ext[:i]): sum(ext[:i + 1])], new[i: i + 1]]).to(torch.int32)
    seq = torch.tensor(ext, dtype=torch.int64, device=DEV)
    fb = SimpleNamespace(forward_mode=H.ForwardMode.EXTEND, batch_size=B, req_pool_indices=torch.arange(B, device=DEV),
                         seq_lens=seq, seq_lens_sum=E, seq_lens_cpu=torch.tensor(ext), extend_prefix_lens_cpu=[0] * B,
                         extend_seq_lens=torch.tensor(ext, dtype=torch.int32, device=DEV), extend_seq_lens_cpu=ext,
                         out_cache_loc=loc, token_to_kv_pool=pool, spec_info=None)
    q, k, kd, qd = (torch.randn(*sh, generator=g).to(dtype) for sh in ((E, Hq * DQ), (E, 1, DQ), (B, 1, DQ), (B, Hq * DQ)))
    backend.init_forward_metadata(fb)
    o = backend.forward(q.to(DEV), k.to(DEV), None, layer, fb)
    kvc = torch.zeros(1025, 1, DQ, dtype=dtype).index_put_((loc.cpu(),), k)
    rows = [(b, j + 1) for b in range(B) for j in range(ext[b])]
    torch.testing.assert_close(o.cpu().view(E, Hq, DV).float(), _ref(q.view(E, Hq, DQ), kvc, r2t.cpu(), rows), **_tol(dtype))
    pool.set_mla_kv_buffer(layer, new, kd[..., :DV].to(DEV), kd[..., DV:].to(DEV))      # the decode step's rows
    kvc[new.cpu()] = kd
    assert torch.equal(pool.get_key_buffer(0).cpu().view(torch.int16), kvc.view(torch.int16))
    fb.forward_mode, fb.out_cache_loc = H.ForwardMode.DECODE, new
    fb.seq_lens, fb.seq_lens_sum, fb.seq_lens_cpu = seq + 1, E + B, torch.tensor(ext) + 1
    backend.init_forward_metadata(fb)
    od = backend.forward(qd.to(DEV), kd.to(DEV), None, layer, fb)
    refs = {d: _ref(qd.view(B, Hq, DQ), kvc, r2t.cpu(), [(b, ext[b] + d) for b in range(B)]) for d in (1, 0)}
    torch.testing.assert_close(od.cpu().view(B, Hq, DV).float(), refs[1], **_tol(dtype))
    # one captured decode step (single stream), replayed with two sets of lengths
    backend.init_cuda_graph_state(B, B)
    rpi, sl, qg = fb.req_pool_indices.clone(), torch.ones(B, dtype=torch.int64, device=DEV), qd.to(DEV)
    backend.init_forward_metadata_capture_cuda_graph(B, B, rpi, sl, None, H.ForwardMode.DECODE, None)
    backend.forward(qg, None, None, layer, fb, save_kv_cache=False)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        og = backend.forward(qg, None, None, layer, fb, save_kv_cache=False)
    for d in (1, 0, 1):
        sl.copy_(seq + d)
        backend.init_forward_metadata_replay_cuda_graph(B, rpi, sl, E + B * d, None, H.ForwardMode.DECODE, None, torch.tensor(ext) + d)
        graph.replay()
        torch.testing.assert_close(og.cpu().view(B, Hq, DV).float(), refs[d], **_tol(dtype))


def test_refusals():
    from iaas_sglang_amd import ops
    from iaas_sglang_amd._lib import MiHotpathError
    kv, r2t, g = _pool([8], BF, 2)
    indptr, idx = _indices(r2t, [8])
    q = torch.randn(1, 16, DQ, generator=g).to(BF).to(DEV)
    with pytest.raises(MiHotpathError, match=r"rc=-2"):      # 576 -> 256
        ops.mla_attention(q, kv.to(DEV), torch.empty(1, 16, 256, dtype=BF, device=DEV), indptr, idx, SM)
    with pytest.raises(MiHotpathError, match=r"rc=-2"):      # fp32
        ops.mla_attention(q.float(), kv.float().to(DEV), torch.empty(1, 16, DV, device=DEV), indptr, idx, SM)
    H, runner, backend, layer = _backend(16, 1, BF)      # both are refused before any metadata is read
    fb = SimpleNamespace(forward_mode=H.ForwardMode.DECODE, token_to_kv_pool=runner.token_to_kv_pool, spec_info=None)
    layer.logit_cap = 30.0
    with pytest.raises(NotImplementedError, match="MLA"):
        backend.forward_decode(q.view(1, -1), kv[:1].to(DEV), None, layer, fb)
    layer.logit_cap = 0.0
    fb.token_to_kv_pool = SimpleNamespace(get_key_buffer=lambda i: torch.zeros(4, 1, DQ, dtype=torch.uint8, device=DEV))
    with pytest.raises(NotImplementedError, match="MLA"):
        backend.forward_decode(q.view(1, -1), kv[:1].to(DEV), None, layer, fb)
