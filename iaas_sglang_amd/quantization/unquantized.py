"""Unquantised (bf16 / fp16) linears on the native 16-bit GEMMs."""
import torch

from .. import ops
from .._compat import UnquantizedLinearMethod


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
