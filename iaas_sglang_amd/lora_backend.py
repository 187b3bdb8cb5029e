"""MiLoRABackend: the multi-LoRA segmented GEMMs on the gfx950 kernels of csrc/lora_sgmv.hip.

Drop-in for the reference's TritonLoRABackend (python/sglang/srt/lora/backend/triton_backend.py:13-88): the same four
methods with the same parameter lists, fed by the LoRABatchInfo that LoRAManager sets before each forward
(lora_manager.py:240-296).  Only `bs` and `max_len` of the batch info are read on the host; the tensors go to the
kernels as they are (int64 ranks on the eager path, int32 under graph mode), so a captured call follows them.
"""
from __future__ import annotations

import torch

from . import ops
from ._compat import BaseLoRABackend, LoRABatchInfo


class MiLoRABackend(BaseLoRABackend):

    def __init__(self, name: str, batch_info: LoRABatchInfo = None):
        super().__init__(name, batch_info)
        # the base class looks these up in a table that knows "triton" / "flashinfer" only (base_backend.py:8-21)
        self.fuse_output_add = True
        self.fuse_stacked_lora_b = True

    def _shrink(self, x: torch.Tensor, weights: torch.Tensor, stack_num: int) -> torch.Tensor:
        bi = self.batch_info
        return ops.lora_shrink(x, weights, bi.seg_indptr, bi.weight_indices, bi.lora_ranks, bi.bs, bi.max_len, stack_num)

    def _expand(self, x: torch.Tensor, weights: torch.Tensor, base_output, num_slices: int, slice_width: int,
                n_offs=None) -> torch.Tensor:
        bi = self.batch_info
        if base_output is None:
            base_output = torch.zeros((x.shape[0], weights.shape[-2]), device=x.device, dtype=x.dtype)
        return ops.lora_expand(x, weights, base_output, bi.seg_indptr, bi.weight_indices, bi.lora_ranks, bi.scalings,
                               bi.bs, bi.max_len, num_slices, slice_width, n_offs)

    def run_lora_a_sgemm(self, x: torch.Tensor, weights: torch.Tensor, *args, **kwargs) -> torch.Tensor:
        return self._shrink(x, weights, 1)

    def run_lora_b_sgemm(self, x: torch.Tensor, weights: torch.Tensor, base_output: torch.Tensor = None, *args,
                         **kwargs) -> torch.Tensor:
        return self._expand(x, weights, base_output, 1, weights.shape[-2])

    def run_qkv_lora(self, x: torch.Tensor, qkv_lora_a: torch.Tensor, qkv_lora_b: torch.Tensor,
                     output_offset: torch.Tensor, max_qkv_out_dim: int, base_output: torch.Tensor = None, *args,
                     **kwargs) -> torch.Tensor:
        # x (s, input_dim); qkv_lora_a (num_lora, 3 r, input_dim); qkv_lora_b (num_lora, out_q + 2 out_kv, r)
        assert isinstance(qkv_lora_b, torch.Tensor)
        lora_a_output = self._shrink(x, qkv_lora_a, 3)
        return self._expand(lora_a_output, qkv_lora_b, base_output, 3, max_qkv_out_dim, output_offset)

    def run_gate_up_lora(self, x: torch.Tensor, gate_up_lora_a: torch.Tensor, gate_up_lora_b: torch.Tensor,
                         base_output: torch.Tensor = None, *args, **kwargs) -> torch.Tensor:
        # x (s, input_dim); gate_up_lora_a (num_lora, 2 r, input_dim); gate_up_lora_b (num_lora, 2 output_dim, r)
        assert isinstance(gate_up_lora_b, torch.Tensor)
        lora_a_output = self._shrink(x, gate_up_lora_a, 2)
        return self._expand(lora_a_output, gate_up_lora_b, base_output, 2, gate_up_lora_b.shape[-2] // 2)
