"""CPU-only: MLATokenToKVPool mirrors the reference's shapes, views and size accounting (memory_pool.py:735-860)."""
import pytest
import torch

from iaas_sglang_amd.mem_cache import MLATokenToKVPool


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_mla_pool_shapes_views_and_size(dtype):
    size, page, R, P, layers = 96, 16, 512, 64, 3
    pool = MLATokenToKVPool(size, page, dtype, R, P, layers, "cpu", start_layer=2)
    assert len(pool.kv_buffer) == layers and pool.token_stride == R + P
    k, v = pool.get_key_buffer(3), pool.get_kv_buffer(3)[1]                     # layer ids count from start_layer
    assert k is pool.kv_buffer[1] and k.shape == (size + page, 1, R + P) and k.dtype == dtype
    assert v.shape == (size + page, 1, R) and v.data_ptr() == k.data_ptr() and v.stride() == k.stride()
    assert pool.get_kv_size_bytes() == layers * (size + page) * (R + P) * 2
    assert pool.mem_usage == pool.get_kv_size_bytes() / (1 << 30)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float8_e4m3fn])
def test_mla_pool_refuses_dtypes_without_a_kernel(dtype):
    with pytest.raises(NotImplementedError, match="MLATokenToKVPool"):
        MLATokenToKVPool(8, 1, dtype, 512, 64, 1, "cpu")
