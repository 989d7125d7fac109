"""CPU-side check of the sequential deflate kernel's residency: both instantiations of md::defl::deflate_kernel must
leave room for 16 streams per CU - LDS <= 9 448 B (160 KiB / 16 is 10 240; the kernel's 9 448 in whole 512-byte units
fits) and <= 128 VGPRs (4 wavefronts per SIMD) - and spill no more than measured.  Read from the built library's
code-object metadata, so a regression fails here before anyone measures it on a GPU.

Scratch: 28 B (plain) and 76 B (profiled), the values before the kernel was split into phases - all of it the tree
builder's frame and, profiled, some of the profile's words; the plain kernel itself spills nothing."""
import os
import re
import subprocess

from decompress_amd import _lib, build

LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
# (the kernel takes one struct: the prefixes do not depend on what is in it)
PLAIN = "_ZN2md4defl14deflate_kernelILb0EE"
PROFILED = "_ZN2md4defl14deflate_kernelILb1EE"


def _kernel_metadata(so, tmp_path):
    """{kernel name: {field: value}} over every code object of the library (one bundle per .hip file)"""
    fat = tmp_path / "fat.bin"
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section=.hip_fatbin=%s" % fat, so, str(tmp_path / "host.o")])
    blob = fat.read_bytes()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
    kernels = {}
    for k, (a, b) in enumerate(zip(starts, starts[1:] + [len(blob)])):
        one, co = tmp_path / ("bundle%d.bin" % k), tmp_path / ("k%d.co" % k)
        one.write_bytes(blob[a:b])
        for t in ("hipv4-amdgcn-amd-amdhsa--gfx950", "hip-amdgcn-amd-amdhsa--gfx950"):
            r = subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=%s" % one,
                                "--targets=%s" % t, "--output=%s" % co], capture_output=True)
            if r.returncode == 0 and co.exists() and co.stat().st_size:
                break
        else:
            continue
        notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", str(co)], text=True)
        # one YAML mapping per kernel; the fields of interest are scalars inside it
        for block in re.split(r"\n\s+- \.agpr_count:", notes):
            m = re.search(r"\.name:\s*(\S+)", block)
            if m:
                kernels[m.group(1)] = {f: int(v) for f, v in re.findall(
                    r"\.(group_segment_fixed_size|private_segment_fixed_size|vgpr_count|sgpr_count):\s*(\d+)", block)}
    return kernels


def test_deflate_kernel_fits_sixteen_streams_per_cu(tmp_path):
    build.build()
    kernels = _kernel_metadata(_lib.SO, tmp_path)
    for prefix, scratch_cap in ((PLAIN, 28), (PROFILED, 76)):
        found = [k for k in kernels if k.startswith(prefix)]
        assert len(found) == 1, (prefix, sorted(k for k in kernels if "deflate" in k))
        k = kernels[found[0]]
        print(found[0], k)
        assert k["group_segment_fixed_size"] <= 9448, k
        assert k["vgpr_count"] <= 128, k
        assert k["private_segment_fixed_size"] <= scratch_cap, k
