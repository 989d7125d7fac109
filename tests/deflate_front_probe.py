"""The deflate front kernels on their own (csrc/deflate_front.hip, deflate_chunked.hip), called as
capi_deflate.cpp's front_workspace / deflate_launch call them, through ctypes on torch buffers: the plan kernel, the
link kernel and the match kernel, and what they leave in the position-indexed workspace.  Needs an MI355X.

TEST INFRASTRUCTURE ONLY."""
import ctypes

import numpy as np


class Front(ctypes.Structure):
    """md::defl::Front, csrc/internal.hpp"""
    _fields_ = [(k, ctypes.c_void_p) for k in ("p_end", "slot", "chunk0", "tail", "flags", "link", "flg", "m", "mq")]


def _lib():
    from decompress_amd import _lib
    lib = _lib.load()
    u32, u64, vp, sz = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_size_t
    fp = ctypes.POINTER(Front)
    lib.md_front_small_bytes.restype, lib.md_front_small_bytes.argtypes = sz, [u32]
    lib.md_front_big_bytes.restype, lib.md_front_big_bytes.argtypes = sz, [u64]
    lib.md_front_carve.restype, lib.md_front_carve.argtypes = None, [vp, vp, u32, u64, fp]
    lib.md_launch_deflate_plan.restype = ctypes.c_int
    lib.md_launch_deflate_plan.argtypes = [u32, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, u64, u32, fp, vp]
    lib.md_deflate_level_params.restype = None
    lib.md_deflate_level_params.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(u32), ctypes.POINTER(u32)]
    lib.md_launch_deflate_front.restype = ctypes.c_int
    lib.md_launch_deflate_front.argtypes = [u32, u32, vp, vp, vp, ctypes.c_int, u32, u32, fp, vp, u32, vp]
    lib.md_launch_link_chunked.restype = ctypes.c_int
    lib.md_launch_link_chunked.argtypes = [vp, vp, vp, u32, u32, u32, fp, vp]
    return lib


class Result:
    """per stream i: p_end[i], tail[i] = (tail0, tail1), and link / flg / m / mq of its positions [0, p_end[i])"""
    def __init__(self, p_end, slot, tail, link, flg, m, mq):
        self.p_end, self.slot, self.tail = p_end, slot, tail
        self._link, self._flg, self._m, self._mq = link, flg, m, mq

    def _cut(self, a, i):
        s = int(self.slot[i])
        return a[s:s + int(self.p_end[i])]

    def link(self, i):
        return self._cut(self._link, i)

    def flg(self, i):
        return self._cut(self._flg, i)

    def m(self, i):
        return self._cut(self._m, i)

    def mq(self, i):
        return self._cut(self._mq, i)


def run(bufs, matcher, level, driver=0, chunked_segment=None, device=0):
    """plan, link and match kernels over the batch `bufs` -> Result.  chunked_segment: ONE stream (De's matcher) whose
    chains md_launch_link_chunked builds in segments of that many positions instead; link and tail only."""
    import torch
    from decompress_amd import workloads
    lib = _lib()
    dev = torch.device("cuda", device)
    n = len(bufs)
    blob, offs, lens = workloads.pack([bytes(b) for b in bufs])
    d_in, d_off, d_len = (torch.from_numpy(a).to(dev) for a in (blob, offs, lens))
    small = torch.zeros(lib.md_front_small_bytes(n), dtype=torch.uint8, device=dev)
    fr = Front()
    lib.md_front_carve(small.data_ptr(), None, n, 0, ctypes.byref(fr))
    torch.cuda.synchronize(dev)
    rc = lib.md_launch_deflate_plan(n, d_len.data_ptr(), driver, matcher, level, 0, 0, ctypes.byref(fr), None)
    assert rc == 0, rc
    torch.cuda.synchronize(dev)
    host = small.cpu().numpy()

    def small_view(ptr, dtype, count):
        o = ptr - small.data_ptr()
        return host[o:o + count * np.dtype(dtype).itemsize].view(dtype).copy()
    slot = small_view(fr.slot, np.uint64, n + 1)
    chunk0 = small_view(fr.chunk0, np.uint32, n + 1)
    assert small_view(fr.flags, np.uint32, 1)[0] == 0, "the plan refused the batch"
    p_end = small_view(fr.p_end, np.uint32, n)
    positions, chunks = int(slot[n]), int(chunk0[n])
    big = torch.zeros(max(256, lib.md_front_big_bytes(positions)), dtype=torch.uint8, device=dev)
    lib.md_front_carve(small.data_ptr(), big.data_ptr(), n, positions, ctypes.byref(fr))
    max_chain, nice = ctypes.c_uint32(), ctypes.c_uint32()
    lib.md_deflate_level_params(driver, matcher, level, ctypes.byref(max_chain), ctypes.byref(nice))
    if chunks:
        if chunked_segment:
            assert n == 1 and matcher == 0
            cus = torch.cuda.get_device_properties(dev).multi_processor_count
            rc = lib.md_launch_link_chunked(d_in.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), int(p_end[0]), chunked_segment,
                                            cus, ctypes.byref(fr), None)
        else:
            rc = lib.md_launch_deflate_front(n, chunks, d_in.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), matcher,
                                             max_chain.value, nice.value, ctypes.byref(fr), None, 0, None)
        assert rc == 0, rc
    torch.cuda.synchronize(dev)
    hb = big.cpu().numpy()

    def big_view(ptr, dtype):
        o = ptr - big.data_ptr()
        return hb[o:o + positions * np.dtype(dtype).itemsize].view(dtype).copy()
    tail = small.cpu().numpy()[fr.tail - small.data_ptr():][:8 * n].view(np.uint32).reshape(n, 2).copy()
    return Result(p_end, slot, tail, big_view(fr.link, np.uint32), big_view(fr.flg, np.uint8), big_view(fr.m, np.uint32),
                  big_view(fr.mq, np.uint32))
