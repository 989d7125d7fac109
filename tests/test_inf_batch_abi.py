"""CPU-side checks of the many-decoders path (md_inf_batch_*): the twelve functions are declared, exported and
bound, the two test hooks are exported and bound without being public, the hand-out kernel is built and uses no scratch,
and misuse without a context is refused without a device."""
import ctypes
import os
import re
import subprocess

from decompress_amd import _lib, build

LLVM = "/opt/rocm/lib/llvm/bin"

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["md_inf_batch_open", "md_inf_batch_src", "md_inf_batch_decode", "md_inf_batch_pending", "md_inf_batch_out",
         "md_inf_batch_status", "md_inf_batch_error", "md_inf_batch_message", "md_inf_batch_checksum",
         "md_inf_batch_src_rem", "md_inf_batch_reset", "md_inf_batch_close"]
HOOKS = ["md_i_inf_batch_launches", "md_i_inf_batch_attempts"]


def _header():
    return open(os.path.join(ROOT, "include", "mdeflate.h")).read()


def test_inf_batch_declared_exported_bound():
    build.build()
    assert "inflate_batch.hip" in build.SOURCES
    hdr = _header()
    so = ctypes.CDLL(_lib.SO)
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for f in FUNCS:
        assert re.search(r"\b%s\s*\(" % f, hdr), f
        assert hasattr(so, f), f
        assert f in bound, f


def test_inf_batch_hooks_exported_not_public():
    build.build()
    so = ctypes.CDLL(_lib.SO)
    extra = {name for name, _, _ in _lib.EXTRA}
    hdr = _header()
    for h in HOOKS:
        assert hasattr(so, h), h
        assert h in extra, h
        assert h not in hdr, h


def test_inf_batch_null_context_and_batch():
    lib = _lib.load()
    assert not lib.md_inf_batch_open(None, 1, 4)
    assert lib.md_inf_batch_src(None, 0, b"x", 1) < 0
    assert lib.md_inf_batch_src(None, 0, None, 0) < 0
    assert lib.md_inf_batch_decode(None) < 0
    assert lib.md_inf_batch_pending(None, 0) == 0
    assert lib.md_inf_batch_out(None, 0, None, 0) == 0
    assert lib.md_inf_batch_error(None, 0) < 0
    assert lib.md_inf_batch_status(None, 0) == 3  # MD_MALFORMED, as md_def_batch_status
    assert lib.md_inf_batch_checksum(None, 0) == 0
    assert lib.md_inf_batch_src_rem(None, 0) == 0
    assert lib.md_inf_batch_message(None, 0)
    lib.md_inf_batch_reset(None, 0)
    lib.md_inf_batch_close(None)
    assert lib.md_i_inf_batch_launches(None) == -1
    assert lib.md_i_inf_batch_attempts(None, 0) == -1


def _all_kernel_metadata(so, tmp_path):
    """kernel name -> resources, from every source file's offload bundle in the library's .hip_fatbin section (one
    bundle per translation unit, each starting with the bundler's magic)"""
    fat = tmp_path / "fat.bin"
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section=.hip_fatbin=%s" % fat, so, str(tmp_path / "host.o")])
    blob = fat.read_bytes()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    starts = [m.start() for m in re.finditer(re.escape(magic), blob)]
    kernels = {}
    for k, a in enumerate(starts):
        part = tmp_path / ("b%d.bin" % k)
        part.write_bytes(blob[a:starts[k + 1] if k + 1 < len(starts) else len(blob)])
        co = tmp_path / ("b%d.co" % k)
        for t in ("hipv4-amdgcn-amd-amdhsa--gfx950", "hip-amdgcn-amd-amdhsa--gfx950"):
            r = subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=%s" % part,
                                "--targets=%s" % t, "--output=%s" % co], capture_output=True)
            if r.returncode == 0 and co.exists() and co.stat().st_size:
                break
        else:
            continue
        notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", str(co)], text=True)
        for block in re.split(r"\n\s+- \.agpr_count:", notes):
            m = re.search(r"\.name:\s*(\S+)", block)
            if m:
                kernels[m.group(1)] = {key: int(v) for key, v in re.findall(
                    r"\.(group_segment_fixed_size|private_segment_fixed_size|vgpr_count):\s*(\d+)", block)}
    return kernels


def test_inf_handout_kernels_use_no_scratch(tmp_path):
    build.build()
    kernels = _all_kernel_metadata(_lib.SO, tmp_path)
    mine = {k: v for k, v in kernels.items() if "inf_hand_" in k}
    assert len(mine) == 2, sorted(mine)
    for name, k in mine.items():
        assert k["private_segment_fixed_size"] == 0, (name, k)
