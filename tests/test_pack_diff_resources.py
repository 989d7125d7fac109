"""CPU-side check of the tree-diff kernels' resources (csrc/pack_diff_kernels.hip), read from the built library's
code-object metadata: the md::pkd kernels are there - the table kernel and both forms of the diff kernel -; none has a private
segment (no spills, no array addressed by a variable) or LDS; and their VGPR counts are the ones DESIGN 4o states."""
import os
import re

from decompress_amd import _lib, build
from tests.test_inf_batch_abi import _all_kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the kernel's name in the code object -> its row in DESIGN 4o's table
KERNELS = {"tree_table_kernel": "tree_table_kernel", "tree_diff_kernelILb0E": "tree_diff_kernel<false>", "tree_diff_kernelILb1E": "tree_diff_kernel<true>"}


def test_pack_diff_kernels_resources(tmp_path):
    build.build()
    kernels = _all_kernel_metadata(_lib.SO, tmp_path)
    mine = {k: v for k, v in kernels.items() if "2md3pkd" in k}  # namespace md::pkd
    for want in KERNELS:
        assert any(want in k for k in mine), (want, sorted(mine))
    assert len(mine) == len(KERNELS), sorted(mine)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("## 4o."):]
    for name, k in mine.items():
        assert k["private_segment_fixed_size"] == 0, (name, k)
        assert k["group_segment_fixed_size"] == 0, (name, k)
        assert k["vgpr_count"] <= 64, (name, k)
        row = [v for w, v in KERNELS.items() if w in name][0]
        # the table's row: kernel | VGPRs | LDS bytes | scratch bytes
        assert re.search(r"%s\s*\|\s*%d\s*\|\s*0\s*\|\s*0\s*\|" % (re.escape(row), k["vgpr_count"]), section), (row, k["vgpr_count"])
