"""CPU-side check of the inflate kernel's residency: the PAIR form of md::wv::inflate_wave_kernel must leave room for
9 streams (18 wavefronts) per CU - LDS <= 17 920 B (160 KiB / 9 in whole 512-byte units), <= 96 VGPRs (5 wavefronts
per SIMD) and no more scratch than before.  Read from the built library's code-object metadata, so a regression
fails here before anyone measures it on a GPU."""
import os
import re
import subprocess

from decompress_amd import _lib, build

LLVM = "/opt/rocm/lib/llvm/bin"
KERNEL = "inflate_wave_kernelILb0ELb1EE"  # <PROF = false, PAIR = true>, whatever its argument list


def _kernel_metadata(so, tmp_path):
    fat = tmp_path / "fat.bin"
    co = tmp_path / "k.co"
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section=.hip_fatbin=%s" % fat, so, str(tmp_path / "host.o")])
    targets = ["hipv4-amdgcn-amd-amdhsa--gfx950", "hip-amdgcn-amd-amdhsa--gfx950"]
    for t in targets:
        r = subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=%s" % fat,
                            "--targets=%s" % t, "--output=%s" % co], capture_output=True)
        if r.returncode == 0 and co.exists() and co.stat().st_size:
            break
    notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", str(co)], text=True)
    # one YAML mapping per kernel; the fields of interest are scalars inside it
    kernels = {}
    for block in re.split(r"\n\s+- \.agpr_count:", notes):
        m = re.search(r"\.name:\s*(\S+)", block)
        if m:
            kernels[m.group(1)] = {k: int(v) for k, v in re.findall(
                r"\.(group_segment_fixed_size|private_segment_fixed_size|vgpr_count):\s*(\d+)", block)}
    return kernels


def test_inflate_pair_kernel_fits_nine_streams_per_cu(tmp_path):
    build.build()
    kernels = _kernel_metadata(_lib.SO, tmp_path)
    names = [name for name in kernels if KERNEL in name]
    assert len(names) == 1, sorted(k for k in kernels if "inflate" in k)
    k = kernels[names[0]]
    assert k["group_segment_fixed_size"] <= 17920, k
    assert k["vgpr_count"] <= 96, k
    assert k["private_segment_fixed_size"] <= 40, k
