"""The deflate kernel's tree builder (tree_make_wave, tree_rle_wave, trees_wave in csrc/deflate_kernel.hip) over the
histograms of tests/huffman_tree_cases.py: heap sizes at the kernel's boundaries, ties, codes deeper than 15 and 7 bits,
runs across the run-length pass's 64-position steps.  The block header carries the three trees, so the bytes of
De.Def.encode pin them: they equal the oracle's, and libz's where libz wrote the same block
(tests/test_huffman_trees.py shows on the CPU what that proves).  Needs an MI355X: `pytest -m gpu`."""
import pytest

from tests import deflate_header_model as header_model
from tests import huffman_tree_cases as cases

pytestmark = pytest.mark.gpu

FAMILIES = sorted(cases.FAMILIES)


@pytest.fixture(scope="module")
def eng():
    import decompress_amd
    return decompress_amd.Engine(0)


@pytest.fixture(scope="module")
def encoded(eng):
    """name -> the bytes of De.Def.encode on the GPU, one small launch per case"""
    from decompress_amd import de
    assert de.copy_cmd(32768, 258) == cases.copy_cmd(32768, 258) and de.copy_cmd(1, 3) == cases.copy_cmd(1, 3) and de.EOB == cases.EOB
    return {c.name: de.Def.encode(c.cmds, de.Def.DYNAMIC) for c in cases.all_cases()}


def first_difference(got, want, cap):
    """which tree two blocks differ in first, by their headers"""
    g, w = header_model.inflate(got, cap), header_model.inflate(want, cap)
    if g.info is None or w.info is None:
        return "no dynamic header: %r / %r" % (g.tag, w.tag)
    for key, what in (("lit_lens", "literal/length tree"), ("dist_lens", "distance tree"), ("cl_lens", "code-length tree")):
        if g.info.get(key) != w.info.get(key):
            return "%s: %r, expected %r" % (what, g.info.get(key), w.info.get(key))
    return "the trees' lengths agree: header layout or payload (%r / %r)" % (g.tag, w.tag)


@pytest.mark.parametrize("family", FAMILIES)
def test_encode_equals_oracle_and_libz(encoded, oracle, family):
    for c in cases.FAMILIES[family]():
        got, want = encoded[c.name], oracle.encode_cmds(c.cmds, "dynamic")
        if got != want:
            pytest.fail("%s: %s" % (c.name, first_difference(got, want, len(c.plain))))
        if cases.literal_only(c):
            z = cases.libz_block(c.plain)
            assert z is None or got == z, c.name


def test_gpu_inflates_them_back(eng, encoded):
    every = cases.all_cases()
    res = eng.inflate_many([encoded[c.name] for c in every], [len(c.plain) for c in every])
    for c, (st, used, out, _) in zip(every, res):
        assert (st, used) == (0, len(encoded[c.name])), c.name
        assert out == c.plain, c.name


@pytest.mark.parametrize("level", [1, 6])
@pytest.mark.parametrize("queue", [16, 4096])
def test_literal_only_bytes_through_the_matcher(eng, oracle, level, queue):
    """the same byte strings through the whole kernel: the matcher flattens the deep histograms, the boundary sizes and
    the ties stay, and trees_wave runs in its cost-comparison mode"""
    every = [c for c in cases.all_cases() if cases.literal_only(c)]
    res = eng.deflate_many([c.plain for c in every], level=level, queue=queue)
    for c, (st, out, _) in zip(every, res):
        assert st == 0, c.name
        assert out == oracle.deflate_raw(c.plain, level, queue)[0], c.name
