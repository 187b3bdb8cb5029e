"""Host side of the W8A8 int8 linear method: config surface, parameter shapes, registration tables."""
import torch

from iaas_sglang_amd.quantization import (MI_EXTRA_QUANTIZATION_METHODS, MI_QUANTIZATION_METHODS, W8A8Int8Config,
                                          W8A8Int8LinearMethod)


def test_config_surface():
    cfg = W8A8Int8Config.from_config({})
    assert isinstance(cfg, W8A8Int8Config) and cfg.get_name() == "w8a8_int8"
    assert set(cfg.get_supported_act_dtypes()) == {torch.float16, torch.bfloat16}
    assert cfg.get_quant_method(torch.nn.ReLU(), "model.act") is None


def test_linear_method_weights():
    widths, K = [96, 32], 256

    class FakeLinear(torch.nn.Module):
        output_partition_sizes = widths
    lin = FakeLinear()
    method = W8A8Int8Config.from_config({}).get_quant_method(lin, "model.layers.0.mlp.gate_up_proj")
    assert isinstance(method, W8A8Int8LinearMethod)
    method.create_weights(lin, K, widths, K, sum(widths), torch.bfloat16, weight_loader=None)
    assert lin.weight.dtype == torch.int8 and tuple(lin.weight.shape) == (128, K)
    assert lin.weight_scale.dtype == torch.float32 and tuple(lin.weight_scale.shape) == (128, 1)
    method.process_weights_after_loading(lin)
    assert tuple(lin.weight.shape) == (K, 128) and lin.weight.stride(0) == 1      # the [K, N] view of [N, K] storage


def test_registration_tables():
    assert MI_EXTRA_QUANTIZATION_METHODS == {"w8a8_int8": W8A8Int8Config}
    assert set(MI_QUANTIZATION_METHODS) == {"fp8", "awq", "gptq", "compressed-tensors"}
