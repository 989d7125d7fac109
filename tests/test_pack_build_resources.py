"""CPU-side check of the index builder's kernels (csrc/pack_build_kernels.hip), read from the built library's
code-object metadata: namespace md::pkb holds exactly its two kernels, and neither uses scratch (no private segment)."""
from decompress_amd import _lib, build
from tests.test_inf_batch_abi import _all_kernel_metadata

KERNELS = ["mark_kernel", "inputs_kernel"]


def test_pack_build_kernels_resources(tmp_path):
    build.build()
    kernels = _all_kernel_metadata(_lib.SO, tmp_path)
    mine = {k: v for k, v in kernels.items() if "2md3pkb" in k}  # namespace md::pkb
    for want in KERNELS:
        assert any(want in k for k in mine), (want, sorted(mine))
    assert len(mine) == len(KERNELS), sorted(mine)
    for name, k in mine.items():
        assert k["private_segment_fixed_size"] == 0, (name, k)
    mark = [v for k, v in mine.items() if "mark_kernel" in k][0]
    assert mark["group_segment_fixed_size"] <= 16 and mark["vgpr_count"] <= 64, mark  # (one word of LDS: the workgroup's count)
