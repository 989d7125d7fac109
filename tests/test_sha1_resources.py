"""CPU-side check of the SHA-1 kernels' resources (csrc/sha1_kernels.hip), read from the built library's
code-object metadata: everything stays in registers - no private segment (no spills, and no array addressed by a variable,
which is what the header's formatter and the schedule's ring could turn into), no LDS - within 128 VGPRs, which leave the
four wavefronts per SIMD that a kernel bound by VALU issue needs; and the hash kernel's exact count, as DESIGN 4j states it."""
from decompress_amd import _lib, build
from tests.test_inf_batch_abi import _all_kernel_metadata

KERNELS = ["sha1_kernel", "names_kernel"]
SHA1_VGPRS = 100


def test_sha1_kernels_resources(tmp_path):
    build.build()
    kernels = _all_kernel_metadata(_lib.SO, tmp_path)
    mine = {k: v for k, v in kernels.items() if "2md3sha" in k}  # namespace md::sha
    for want in KERNELS:
        assert any(want in k for k in mine), (want, sorted(mine))
    assert len(mine) == len(KERNELS), sorted(mine)
    for name, k in mine.items():
        assert k["private_segment_fixed_size"] == 0 and k["group_segment_fixed_size"] == 0, (name, k)
        assert k["vgpr_count"] <= 128, (name, k)
    sha1 = [v for k, v in mine.items() if "sha1_kernel" in k][0]
    assert sha1["vgpr_count"] == SHA1_VGPRS, sha1
