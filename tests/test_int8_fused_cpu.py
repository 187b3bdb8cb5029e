"""Host side of the fused int8 forms: the workspace query follows the split plan and refuses what the forms refuse."""


def test_fused_workspace_query():
    from iaas_sglang_amd import ops
    from iaas_sglang_amd._lib import lib
    assert lib.mi_int8_gemm_fused_workspace_bytes(16, 4096, 4096) == 8 * 16 * 4096 * 4     # 32 column blocks: 8 slices
    assert lib.mi_int8_gemm_fused_workspace_bytes(16, 28672, 4096) == 16 * 28672 * 4       # fills the chip: one slab
    assert ops.int8_fused_ok(256, 4096, 4096) and not ops.int8_fused_ok(257, 4096, 4096)
    assert not ops.int8_fused_ok(16, 4096, 4000) and not ops.int8_fused_ok(16, 4100, 4096)
