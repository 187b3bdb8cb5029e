"""CPU-only: MiLoRABackend sits behind the reference's LoRA backend interface and register()'s seam selects it."""
import inspect
import types

import pytest
import torch


def test_backend_interface():
    from iaas_sglang_amd._compat import BaseLoRABackend
    from iaas_sglang_amd.lora_backend import MiLoRABackend
    be = MiLoRABackend("mi355x")
    assert isinstance(be, BaseLoRABackend)
    assert be.fuse_output_add is True and be.fuse_stacked_lora_b is True
    x = a = b = base = offs = torch.empty(0)
    # the call forms of the reference's lora/layers.py:83-90 and :298-305, :158-165, :249-256 (with the kwargs of :244-247)
    for method, args, kwargs in [
        (be.run_lora_a_sgemm, (x, a), {}),
        (be.run_lora_b_sgemm, (x, b), {"base_output": base}),
        (be.run_gate_up_lora, (x, a, b), {"base_output": base}),
        (be.run_qkv_lora, (x, a, b), {"base_output": base, "output_offset": offs, "max_qkv_out_dim": 128}),
    ]:
        bound = inspect.signature(method).bind(*args, **kwargs)
        assert "kwargs" not in bound.arguments, f"{method.__name__} swallowed a named argument"


def test_register_seam_selects_the_backend():
    from iaas_sglang_amd import register as R
    from iaas_sglang_amd.lora_backend import MiLoRABackend
    base_backend, lora_manager = types.ModuleType("base_backend"), types.ModuleType("lora_manager")

    def original(name):
        if name != "triton":
            raise ValueError(f"Invalid backend: {name}")
        return "the triton class"

    base_backend.get_backend_from_name = lora_manager.get_backend_from_name = original
    assert R.install_lora_backend(base_backend, lora_manager)
    for module in (base_backend, lora_manager):
        assert module.get_backend_from_name("mi355x") is MiLoRABackend
        assert module.get_backend_from_name("triton") == "the triton class"
        with pytest.raises(ValueError):
            module.get_backend_from_name("nonsense")
