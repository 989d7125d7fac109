"""A serialised inflate index written with struct.pack from the layout in include/mdeflate.h (md_inflate_index_*), for
the tests of md_inflate_index_load / _save: nothing here comes from the code under test."""
import struct

MAGIC = b"MDZINDEX"
HEAD, POINT = 72, 24


def window_len(out):
    return min(32768, out)


def blob(fmt=1, src_len=5000, header_len=2, consumed=4990, size=20000, span=4096, checksum=0x1234abcd,
         points=((16, 0), (9000, 4096), (20001, 12300)), version=1, zero=0, win_lens=None, point_zero=0, windows=None, npoints=None):
    """the index of a stream that does not exist: the fields as given, window k = win_lens[k] (default min(32768, out))
    bytes of a pattern"""
    win_lens = [window_len(o) for _, o in points] if win_lens is None else list(win_lens)
    head = MAGIC + struct.pack("<IIQQQQQQII", version, fmt, src_len, header_len, consumed, size, span,
                               len(points) if npoints is None else npoints, checksum, zero)
    assert len(head) == HEAD
    table = b"".join(struct.pack("<QQII", b, o, w, point_zero) for (b, o), w in zip(points, win_lens))
    if windows is None:
        windows = b"".join(bytes((7 * k + j) & 0xff for j in range(w)) for k, w in enumerate(win_lens))
    return head + table + windows
