"""`--quantization w8a8_int8` checkpoints (SmoothQuant style): int8 weights with one static scale per output
channel, activations quantised to int8 per token at run time.

Mirrors the surface of W8A8Int8Config / W8A8Int8LinearMethod (quantization/w8a8_int8.py:30-75, 78-145).  The
reference's `per_token_quant_int8` + `int8_scaled_mm` (CUDA only, w8a8_int8.py:26-27, 141-145) become
mi_int8_quant_per_token + mi_int8_gemm; there is no other path, any number of rows runs through them.
MoE layers (W8A8Int8MoEMethod) are outside this hot path: get_quant_method answers None for them.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional

import torch
from torch.nn import Parameter

from .. import ops
from .._compat import (ChannelQuantScaleParameter, LinearBase, LinearMethodBase, ModelWeightParameter,
                       QuantizationConfig)


class W8A8Int8Config(QuantizationConfig):
    """Weights static, per channel, symmetric; activations dynamic, per token, symmetric.  The checkpoint's
    quantization dict carries nothing this method needs."""

    def __init__(self) -> None:
        super().__init__()

    def get_name(self) -> str:
        return "w8a8_int8"

    def get_supported_act_dtypes(self) -> List[torch.dtype]:
        return [torch.float16, torch.bfloat16]

    @classmethod
    def get_min_capability(cls) -> int:
        return 75

    @staticmethod
    def get_config_filenames() -> List[str]:
        return []

    def get_scaled_act_names(self) -> List[str]:
        return []

    @classmethod
    def from_config(cls, config: Dict[str, Any]) -> "W8A8Int8Config":
        return cls()

    def get_quant_method(self, layer: torch.nn.Module, prefix: str):
        if isinstance(layer, LinearBase) or hasattr(layer, "output_partition_sizes"):
            return W8A8Int8LinearMethod(self)
        return None   # MoE: not on this path


class W8A8Int8LinearMethod(LinearMethodBase):
    def __init__(self, quantization_config: W8A8Int8Config):
        self.quantization_config = quantization_config

    def create_weights(self, layer: torch.nn.Module, input_size_per_partition: int, output_partition_sizes: List[int],
                       input_size: int, output_size: int, params_dtype: torch.dtype, **extra_weight_attrs):
        weight_loader = extra_weight_attrs.get("weight_loader")
        n = sum(output_partition_sizes)
        layer.logical_widths = output_partition_sizes
        layer.register_parameter("weight", ModelWeightParameter(
            data=torch.empty(n, input_size_per_partition, dtype=torch.int8), input_dim=1, output_dim=0,
            weight_loader=weight_loader))
        layer.register_parameter("weight_scale", ChannelQuantScaleParameter(
            data=torch.empty((n, 1), dtype=torch.float32), output_dim=0, weight_loader=weight_loader))

    def process_weights_after_loading(self, layer: torch.nn.Module) -> None:
        # the [K, N] view of the [N, K] storage: what mi_int8_gemm reads as b_nk
        layer.weight = Parameter(layer.weight.data.t(), requires_grad=False)
        layer.weight_scale = Parameter(layer.weight_scale.data.contiguous(), requires_grad=False)

    def apply(self, layer: torch.nn.Module, x: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
        x2 = x.reshape(-1, x.shape[-1])
        xq, x_scale = ops.int8_quant_per_token(x2)
        out = ops.int8_gemm(xq, layer.weight, x_scale, layer.weight_scale, x.dtype, bias)
        return out.reshape(*x.shape[:-1], out.shape[-1])

    def apply_prequantized(self, layer: torch.nn.Module, xq: torch.Tensor, x_scale: torch.Tensor,
                           out_dtype: torch.dtype, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`apply` minus the activation quantisation: (xq, x_scale) come from a producer that already emitted int8
        (ops.rmsnorm_int8 / silu_and_mul_int8 / a fused consumer)."""
        return ops.int8_gemm(xq, layer.weight, x_scale, layer.weight_scale, out_dtype, bias)

    # ---- decode batches: the linear fused with its consumer (mi_int8_gemm_* forms, M <= 256, no bias)
    def fused_decode8_ok(self, layer: torch.nn.Module, M: int) -> bool:
        K, N = layer.weight.shape
        return getattr(layer, "bias", None) is None and ops.int8_fused_ok(M, N, K)

    def apply_rope_kvwrite8(self, layer, xq, x_scale, positions, cos_sin_cache, k_cache, v_cache, loc, num_q_heads,
                            num_kv_heads, head_dim):
        """q = rope(linear(xq)[:, :q]); k (rope) and v rows go straight into the KV pool at `loc`."""
        return ops.int8_gemm_rope_kvwrite(xq, layer.weight, x_scale, layer.weight_scale, positions, cos_sin_cache, k_cache,
                                          v_cache, loc, num_q_heads, num_kv_heads, head_dim)

    def apply_add_rmsnorm8(self, layer, xq, x_scale, residual, norm_weight, eps, want_q=True, want_out=False):
        """(out | None, q | None, scales | None) of rmsnorm(linear(xq) + residual) * norm_weight; residual updated in place."""
        return ops.int8_gemm_add_rmsnorm(xq, layer.weight, x_scale, layer.weight_scale, residual, norm_weight, eps,
                                         want_q, want_out)

    def apply_silu_mul8(self, layer, xq, x_scale, act_dtype):
        """(q, scales) = per-token int8 of silu(gate) * up, linear(xq) = [gate | up]."""
        return ops.int8_gemm_silu_mul(xq, layer.weight, x_scale, layer.weight_scale, act_dtype)
