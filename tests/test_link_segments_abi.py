"""CPU-side checks of the segmented hash-chain pass's plumbing: the kernel is in the library, its test hook
is exported and bound next to the public symbols without being one of them, and the Engine reads it (no GPU needed)."""
import ctypes
import os

from decompress_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_link_segments_hook_exported_and_bound():
    build.build()
    assert "deflate_chunked.hip" in build.SOURCES
    assert hasattr(ctypes.CDLL(_lib.SO), "md_i_link_segments")
    assert "md_i_link_segments" in {name for name, _, _ in _lib.EXTRA}
    assert "md_i_link_segments" not in open(os.path.join(ROOT, "include", "mdeflate.h")).read()
    from decompress_amd import engine
    assert callable(getattr(engine.Engine, "link_segments", None))
    assert callable(getattr(engine.Engine, "deflate_one", None))


def test_link_segments_hook_null_context():
    assert _lib.load().md_i_link_segments(None) == -1
