"""CPU-side check of the pack writer's kernels' resources (csrc/pack_write_kernels.hip), read from the built
library's code-object metadata: the three md::pkw kernels are there; none has a private segment (no spills, no array
addressed by a variable) or LDS; the delta kernel stays within 128 VGPRs; and the counts are the ones DESIGN 4l states."""
import os
import re

from decompress_amd import _lib, build
from tests.test_inf_batch_abi import _all_kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VGPRS = {"index_kernel": 16, "delta_kernel": 22, "assemble_kernel": 14}


def test_pack_write_kernels_resources(tmp_path):
    build.build()
    kernels = _all_kernel_metadata(_lib.SO, tmp_path)
    mine = {k: v for k, v in kernels.items() if "2md3pkw" in k}  # namespace md::pkw
    for want in VGPRS:
        assert any(want in k for k in mine), (want, sorted(mine))
    assert len(mine) == len(VGPRS), sorted(mine)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for name, k in mine.items():
        assert k["private_segment_fixed_size"] == 0 and k["group_segment_fixed_size"] == 0, (name, k)
        assert k["vgpr_count"] <= 128, (name, k)
        short = [w for w in VGPRS if w in name][0]
        assert k["vgpr_count"] == VGPRS[short], (name, k)
        assert re.search(r"%s\s*\|\s*%d\s*\|" % (short, VGPRS[short]), design), short
