"""Unquantised (bf16 / fp16) linears on the native 16-bit GEMMs, and unquantised experts on the native MoE kernels."""
from typing import Callable, Optional

import torch

from .. import ops
from .._compat import HAVE_SGLANG, UnquantizedFusedMoEMethod, UnquantizedLinearMethod


class MiUnquantizedLinearMethod(UnquantizedLinearMethod):
    """Drop-in for the reference's UnquantizedLinearMethod (layers/linear.py:152-193): same `create_weights`, same
    [N,K] weight.  `apply` runs decode batches -- whatever `ops.bf16_gemm_ok` accepts: up to 512 rows, K % 64 == 0,
    aligned operands -- through the hand-written decode kernel (`ops.bf16_gemm`), prefill batches of more than 512
    rows that `ops.bf16_gemm_tile_ok` accepts through the hand-written tile kernel (`ops.bf16_gemm_tile`), and every
    other call (K % 64 != 0, unaligned views, other dtypes) through `F.linear` exactly as the parent class does.  That
    last branch is the parent's behaviour for operands the kernels do not cover, not a fallback for a missing kernel."""

    def apply(self, layer, x, bias=None):
        w = layer.weight
        x2 = x.reshape(-1, x.shape[-1])
        M, K = x2.shape
        N = w.shape[0]
        if (x2.is_cuda and x2.dtype == w.dtype and x2.dtype in (torch.bfloat16, torch.float16) and M > 0
                and (bias is None or (bias.dtype == x2.dtype and bias.is_contiguous()))):
            if ops.bf16_gemm_ok(M, N, K, x2, w):
                return ops.bf16_gemm(x2, w, bias).view(*x.shape[:-1], N)
            if M > 512 and ops.bf16_gemm_tile_ok(M, N, K, x2, w):
                return ops.bf16_gemm_tile(x2, w, bias).view(*x.shape[:-1], N)
        return super().apply(layer, x, bias)


class MiUnquantizedFusedMoEMethod(UnquantizedFusedMoEMethod):
    """Drop-in for the reference's UnquantizedFusedMoEMethod (layers/moe/fused_moe_triton/layer.py:96-277): the same
    `create_weights` (w13_weight [E, 2I, H], w2_weight [E, H, I]) and the same `apply` parameter list.  Plain softmax
    routing runs the native router (`ops.moe_topk_softmax`); grouped or biased routing, or a custom routing function,
    goes to the reference's own `select_experts` (its torch code, layers/moe/topk.py:420-510) when SGLang is there.
    The experts always run `ops.moe_fused_experts`; what that call cannot do raises, nothing falls back."""

    def process_weights_after_loading(self, layer: torch.nn.Module) -> None:
        return      # the kernels read the checkpoint layout as it is (no aiter shuffle, layer.py:137-154)

    def apply(self, layer: torch.nn.Module, x: torch.Tensor, router_logits: torch.Tensor, top_k: int,
              renormalize: bool, use_grouped_topk: bool, topk_group: Optional[int] = None,
              num_expert_group: Optional[int] = None, num_fused_shared_experts: int = 0,
              custom_routing_function: Optional[Callable] = None, correction_bias: Optional[torch.Tensor] = None,
              activation: str = "silu", apply_router_weight_on_input: bool = False, inplace: bool = True,
              no_combine: bool = False, routed_scaling_factor: Optional[float] = None) -> torch.Tensor:
        if activation != "silu":
            raise NotImplementedError(f"MiUnquantizedFusedMoEMethod: activation {activation!r} has no kernel (silu only)")
        if apply_router_weight_on_input:
            raise NotImplementedError("MiUnquantizedFusedMoEMethod: apply_router_weight_on_input has no kernel "
                                      "(the router weight meets the down GEMM's accumulator)")
        if no_combine:
            raise NotImplementedError("MiUnquantizedFusedMoEMethod: no_combine has no kernel (the slots are always summed)")
        if getattr(self, "use_triton_kernels", False):
            raise NotImplementedError("MiUnquantizedFusedMoEMethod: the transposed triton_kernels weight layout has no kernel")
        if use_grouped_topk or custom_routing_function is not None or correction_bias is not None:
            if not HAVE_SGLANG:
                raise NotImplementedError("MiUnquantizedFusedMoEMethod: grouped, biased or custom routing runs the "
                                          "reference's select_experts, which needs SGLang; only plain softmax top-k "
                                          "routing is native")
            from sglang.srt.layers.moe.topk import select_experts
            topk_weights, topk_ids = select_experts(
                hidden_states=x, router_logits=router_logits, use_grouped_topk=use_grouped_topk, top_k=top_k,
                renormalize=renormalize, topk_group=topk_group, num_expert_group=num_expert_group,
                num_fused_shared_experts=num_fused_shared_experts, custom_routing_function=custom_routing_function,
                correction_bias=correction_bias, routed_scaling_factor=routed_scaling_factor)
            topk_weights = topk_weights.to(torch.float32).contiguous()
            topk_ids = topk_ids.to(torch.int32).contiguous()
        else:
            topk_weights, topk_ids = ops.moe_topk_softmax(router_logits, top_k, renormalize)
        return ops.moe_fused_experts(x, layer.w13_weight, layer.w2_weight, topk_weights, topk_ids, inplace=inplace,
                                     routed_scaling_factor=routed_scaling_factor)
