"""CPU-only: the fused-MoE seam of register() and the drop-in surface of MiUnquantizedFusedMoEMethod."""
import inspect
import types

import pytest
import torch

from iaas_sglang_amd.quantization.unquantized import MiUnquantizedFusedMoEMethod
from iaas_sglang_amd.register import install_fused_moe

# UnquantizedFusedMoEMethod.apply of the reference (layers/moe/fused_moe_triton/layer.py:156-174): names and defaults
NO_DEFAULT = inspect.Parameter.empty
REFERENCE_APPLY = [("self", NO_DEFAULT), ("layer", NO_DEFAULT), ("x", NO_DEFAULT), ("router_logits", NO_DEFAULT),
                   ("top_k", NO_DEFAULT), ("renormalize", NO_DEFAULT), ("use_grouped_topk", NO_DEFAULT),
                   ("topk_group", None), ("num_expert_group", None), ("num_fused_shared_experts", 0),
                   ("custom_routing_function", None), ("correction_bias", None), ("activation", "silu"),
                   ("apply_router_weight_on_input", False), ("inplace", True), ("no_combine", False),
                   ("routed_scaling_factor", None)]


def test_install_binds_the_class_on_a_stub_module():
    stub = types.SimpleNamespace(UnquantizedFusedMoEMethod=object)
    assert install_fused_moe(stub) is True
    assert stub.UnquantizedFusedMoEMethod is MiUnquantizedFusedMoEMethod


def test_apply_has_the_reference_parameter_list():
    params = inspect.signature(MiUnquantizedFusedMoEMethod.apply).parameters.values()
    assert [(p.name, p.default) for p in params] == REFERENCE_APPLY


def test_create_weights_registers_the_reference_shapes():
    layer, loader = torch.nn.Module(), object()
    MiUnquantizedFusedMoEMethod().create_weights(layer, 4, 64, 48, torch.bfloat16, weight_loader=loader)
    assert layer.w13_weight.shape == (4, 96, 64) and layer.w2_weight.shape == (4, 64, 48)
    assert layer.w13_weight.dtype == layer.w2_weight.dtype == torch.bfloat16
    assert layer.w13_weight.weight_loader is loader and not layer.w2_weight.requires_grad


@pytest.mark.parametrize("option", [{"activation": "gelu"}, {"apply_router_weight_on_input": True}, {"no_combine": True},
                                    {"use_grouped_topk": True}, {"correction_bias": torch.zeros(4)}])
def test_unsupported_options_raise(option):
    args = dict(layer=None, x=None, router_logits=None, top_k=2, renormalize=True, use_grouped_topk=False)
    with pytest.raises(NotImplementedError):
        MiUnquantizedFusedMoEMethod().apply(**{**args, **option})
