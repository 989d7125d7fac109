"""CPU-side check of the packfile kernels' resources (csrc/pack_kernels.hip), read from the built library's
code-object metadata: the apply kernel keeps everything in registers - no private segment (no spills), no LDS, and the
32 VGPRs DESIGN 4i states, which leave the full 8 wavefronts per SIMD - and none of its siblings uses scratch either."""
from decompress_amd import _lib, build
from tests.test_inf_batch_abi import _all_kernel_metadata

KERNELS = ["headers_kernel", "chain_step_kernel", "chain_finish_kernel", "verdict_kernel", "delta_sizes_kernel", "apply_kernel", "repeats_kernel"]


def test_pack_kernels_resources(tmp_path):
    build.build()
    kernels = _all_kernel_metadata(_lib.SO, tmp_path)
    mine = {k: v for k, v in kernels.items() if "2md2pk" in k}  # namespace md::pk
    for want in KERNELS:
        assert any(want in k for k in mine), (want, sorted(mine))
    assert len(mine) == len(KERNELS), sorted(mine)
    for name, k in mine.items():
        assert k["private_segment_fixed_size"] == 0, (name, k)
    apply = [v for k, v in mine.items() if "apply_kernel" in k][0]
    assert apply["group_segment_fixed_size"] == 0 and apply["vgpr_count"] == 32, apply
