"""Mixture of experts (ops.moe_topk_softmax, ops.moe_fused_experts, MiUnquantizedFusedMoEMethod) against a plain fp64
torch form of the contract in include/mi_hotpath.h, with its four roundings to T and loops over the experts.

Tolerance of the experts tests: the contract evaluated on the CPU with fp64 and with fp32 accumulation (two references,
neither is the code under test) differs by at most 2^-8 = 0.00390625 over the parametrised cases below (reached by the
fp16 routed_scaling case; bf16 cases: 2^-12 at most, fp16 cases without scaling: 2^-9) -- an intermediate rounding that
flipped moves a result by one T-ulp of an O(1) value.  The tests allow twice that, 2^-7, for every case.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
TOL = 2 * 2.0 ** -8
E, K_TOP = 8, 2
COUNTS = [0, 1, 15, 16, 17, 33, 128, 129]   # rows per expert: the 16- and 128-row block edges, an empty expert
T = 170                                     # 339 pairs are odd: slot 340 holds an id outside [0, E) in every case
SHAPES = [(64, 16), (192, 176), (128, 64)]  # (H, I): one k-step; a half k-step in the down GEMM (176 % 32 != 0) and
                                            # ragged 64-column blocks; two column blocks of the tile form's gate_up


def hand_ids(masked):
    """[T, 2] int32 with COUNTS[e] slots of expert e in a fixed random order (some tokens get one expert twice); with
    `masked` the last three tokens hold ids outside [0, E) only."""
    flat = torch.tensor([e for e, n in enumerate(COUNTS) for _ in range(n)] + [E], dtype=torch.int32)
    ids = flat[torch.randperm(flat.numel(), generator=torch.Generator().manual_seed(5))].view(T, K_TOP).clone()
    if masked:
        ids[-3:] = torch.tensor([[-1, E], [1000, -7], [E, E]], dtype=torch.int32)
    return ids


def ref_experts(x, w13, w2, tw, ids, scale, acc=torch.float64):
    """x, w13, w2 of dtype T on the CPU; every product accumulates in `acc`; returns out as dtype T."""
    dt, I = x.dtype, w2.shape[2]
    y = torch.zeros(ids.shape + (x.shape[1],), dtype=torch.float64)
    for e in range(w13.shape[0]):
        t, j = torch.nonzero(ids == e, as_tuple=True)
        gu = (x[t].to(acc) @ w13[e].to(acc).T).to(dt).to(acc)
        act = (torch.nn.functional.silu(gu[:, :I]) * gu[:, I:]).to(dt)
        y[t, j] = ((act.to(acc) @ w2[e].to(acc).T) * tw[t, j][:, None].to(acc)).to(dt).double()
    return (y.to(acc).sum(1) * scale).to(dt)


@functools.lru_cache(maxsize=None)
def case(H, I, dtype, masked=False, scale=1.0):
    g = torch.Generator().manual_seed(H + I)
    x = torch.randn(T, H, generator=g).to(dtype)
    w13 = (torch.randn(E, 2 * I, H, generator=g) / H ** 0.5).to(dtype)
    w2 = (torch.randn(E, H, I, generator=g) / I ** 0.5).to(dtype)
    tw = torch.rand(T, K_TOP, generator=g) * 0.5 + 0.25
    ids = hand_ids(masked)
    return x, w13, w2, tw, ids, ref_experts(x, w13, w2, tw, ids, scale)


def in_sentinel(t):
    """A device copy of `t` as the middle columns of a wider buffer filled with 0.5, and that buffer."""
    buf = torch.full((t.shape[0], t.shape[1] + 64), 0.5, dtype=t.dtype, device=DEV)
    view = buf[:, 32:32 + t.shape[1]]
    view.copy_(t)
    return view, buf


def run_experts(H, I, dtype, form, inplace, masked=False, scale=None):
    from iaas_sglang_amd import ops
    x, w13, w2, tw, ids, ref = case(H, I, dtype, masked, 1.0 if scale is None else scale)
    xd, xbuf = in_sentinel(x)
    od, obuf = in_sentinel(torch.zeros_like(x))
    got = ops.moe_fused_experts(xd, w13.to(DEV), w2.to(DEV), tw.to(DEV), ids.to(DEV), inplace=inplace,
                                routed_scaling_factor=scale, form=form, out=None if inplace else od)
    buf = xbuf if inplace else obuf
    assert got.data_ptr() == (xd if inplace else od).data_ptr()
    assert bool((buf[:, :32] == 0.5).all()) and bool((buf[:, 32 + H:] == 0.5).all())
    if not inplace:
        assert torch.equal(xd.cpu(), x)
    err = (got.cpu().double() - ref.double()).abs().max().item()
    print(f"H {H} I {I} {dtype} {form} max abs err {err:.3g} (allowed {TOL:.3g})")
    assert err <= TOL


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["rows16", "tile"])
@pytest.mark.parametrize("H,I", SHAPES)
def test_experts_hand_built_ids(H, I, form, dtype, inplace):
    run_experts(H, I, dtype, form, inplace)


@pytest.mark.parametrize("form", ["rows16", "tile"])
@pytest.mark.parametrize("masked,scale", [(True, None), (False, 2.5)])
def test_experts_masked_ids_and_routed_scaling(form, masked, scale):
    run_experts(192, 176, torch.float16, form, False, masked, scale)


@pytest.mark.parametrize("gdtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("renormalize", [False, True])
@pytest.mark.parametrize("k", [1, 2, 8])
@pytest.mark.parametrize("n_experts", [8, 64, 256])
def test_router(n_experts, k, renormalize, gdtype):
    """Per row a random permutation of a 0.25-spaced grid (exact in bf16): neighbouring probabilities differ by a
    factor e^0.25, so ids are exact; weights against the fp64 softmax at rtol 2^-16."""
    from iaas_sglang_amd import ops
    g = torch.Generator().manual_seed(n_experts + k)
    grid = (torch.arange(n_experts) - n_experts // 2) * 0.25
    logits = torch.stack([grid[torch.randperm(n_experts, generator=g)] for _ in range(37)]).to(gdtype)
    w, ids = ops.moe_topk_softmax(logits.to(DEV), k, renormalize)
    p = torch.softmax(logits.double(), -1)
    rw, rid = torch.topk(p, k, dim=-1)
    if renormalize:
        rw = rw / rw.sum(-1, keepdim=True)
    assert ids.dtype == torch.int32 and torch.equal(ids.cpu().long(), rid)
    torch.testing.assert_close(w.cpu().double(), rw, rtol=2 ** -16, atol=0)


def test_router_tie_takes_the_lowest_index():
    from iaas_sglang_amd import ops
    w, ids = ops.moe_topk_softmax(torch.full((5, 64), 1.5, device=DEV), 8, True)
    assert torch.equal(ids.cpu(), torch.arange(8, dtype=torch.int32).expand(5, 8))
    assert torch.equal(w.cpu(), torch.full((5, 8), 0.125))


def test_graph_replay_follows_rewritten_ids():
    from iaas_sglang_amd import ops
    x, w13, w2, tw, ids, _ = case(128, 64, torch.bfloat16)
    xd, w13d, w2d, twd, idsd = (t.to(DEV) for t in (x, w13, w2, tw, ids))
    out = torch.empty_like(xd)

    def run(o):
        return ops.moe_fused_experts(xd, w13d, w2d, twd, idsd, form="rows16", out=o)

    run(out)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(out)
    for shift in (3, 6):
        idsd.copy_(((ids + shift) % (E + 1)).to(DEV))      # another distribution, some slots masked (id E)
        twd.copy_(tw.flip(0).to(DEV))
        eager = run(torch.empty_like(xd)).clone()
        for _ in range(3):
            graph.replay()
            assert torch.equal(out, eager)


def test_method_apply_end_to_end():
    from iaas_sglang_amd.quantization.unquantized import MiUnquantizedFusedMoEMethod
    dtype, H, I = torch.bfloat16, 128, 64
    x, w13, w2, _, _, _ = case(H, I, dtype)
    logits = torch.randn(T, E, generator=torch.Generator().manual_seed(9))
    layer, method = torch.nn.Module(), MiUnquantizedFusedMoEMethod()
    method.create_weights(layer, E, H, I, dtype)
    layer.to(DEV)
    layer.w13_weight.data.copy_(w13)
    layer.w2_weight.data.copy_(w2)
    xd = x.to(DEV)
    got = method.apply(layer, xd, logits.to(DEV), top_k=K_TOP, renormalize=True, use_grouped_topk=False)
    assert got.data_ptr() == xd.data_ptr()                  # inplace=True is the reference's default
    tw, ids = torch.topk(torch.softmax(logits.double(), -1), K_TOP, dim=-1)
    ref = ref_experts(x, w13, w2, (tw / tw.sum(-1, keepdim=True)).float(), ids.int(), 1.0)
    assert (got.cpu().double() - ref.double()).abs().max().item() <= TOL
