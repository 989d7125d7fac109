"""CPU-side check of the object-graph kernels' resources (csrc/pack_graph_kernels.hip), read from the built
library's code-object metadata: the md::pkg kernels are there; none has a private segment (no spills, no array addressed by
a variable) or LDS; the three that do the work - tree_links_kernel, object_links_kernel, reach_step_kernel - stay within 64
VGPRs, and their counts are the ones DESIGN 4n states."""
import os
import re

from decompress_amd import _lib, build
from tests.test_inf_batch_abi import _all_kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["tree_links_kernel", "object_links_kernel", "gather_kernel", "seed_kernel", "reach_step_kernel", "reach_finish_kernel"]
STATED = ["tree_links_kernel", "object_links_kernel", "reach_step_kernel"]


def test_pack_graph_kernels_resources(tmp_path):
    build.build()
    kernels = _all_kernel_metadata(_lib.SO, tmp_path)
    mine = {k: v for k, v in kernels.items() if "2md3pkg" in k}  # namespace md::pkg
    for want in KERNELS:
        assert any(want in k for k in mine), (want, sorted(mine))
    assert len(mine) == len(KERNELS), sorted(mine)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("## 4n."):]
    for name, k in mine.items():
        assert k["private_segment_fixed_size"] == 0, (name, k)
        assert k["group_segment_fixed_size"] == 0, (name, k)
        short = [w for w in KERNELS if w in name][0]
        if short in STATED:
            assert k["vgpr_count"] <= 64, (name, k)
            # the table's row: kernel | VGPRs | LDS bytes | scratch bytes
            assert re.search(r"%s\s*\|\s*%d\s*\|\s*0\s*\|\s*0\s*\|" % (short, k["vgpr_count"]), section), (short, k["vgpr_count"])
