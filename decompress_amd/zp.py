"""ZIP archives (.zip .jar .whl .npz .docx ...) through the C ABI's md_zip_* entry points: the directory is read on the
host, every selected entry is decoded (method 8) or copied (method 0) and checked against the directory's CRC-32 in one
batch on the GPU, and the writer compresses all files in one deflate launch."""
import ctypes

from . import engine as _engine
from ._lib import ZipEntry, ZipInfo, ZipResult, ZipSource
from ._lib import load as _load

_INFO_KEYS = ("entries", "total_usize", "dir_off", "dir_size", "prefix", "comment_off", "comment_len", "zip64")
_ENTRY_KEYS = ("header_off", "csize", "usize", "crc32", "external_attr", "method", "flags", "dos_time", "dos_date")


def _raw(src):
    return src if isinstance(src, bytes) else bytes(src)


def _directory(lib, src):
    info = ZipInfo()
    st = lib.md_zip_directory(src, len(src), ctypes.byref(info), None, 0)
    if st != 0:
        raise _engine.Error(lib.md_status_string(st).decode())
    ents = (ZipEntry * max(info.entries, 1))()
    st = lib.md_zip_directory(src, len(src), ctypes.byref(info), ents, info.entries)
    if st != 0:
        raise _engine.Error(lib.md_status_string(st).decode())
    return info, ents


def directory(src):
    """md_zip_directory (host arithmetic, no device needed) -> (entries, info): one dict per entry - name (bytes, the
    directory's copy), header_off, csize, usize, crc32, external_attr, method, flags, dos_time, dos_date - and a dict of
    the archive's: entries, total_usize, dir_off, dir_size, prefix, comment_off, comment_len, zip64.  Raises `Error`
    ("Invalid ZIP directory") for what is no archive."""
    src = _raw(src)
    info, ents = _directory(_load(), src)
    out = []
    for e in ents[:info.entries]:
        d = {k: getattr(e, k) for k in _ENTRY_KEYS}
        d["name"] = src[e.name_off:e.name_off + e.name_len]
        out.append(d)
    return out, {k: getattr(info, k) for k in _INFO_KEYS}


def uncompress(src, select=None, device=0):
    """md_zip_uncompress: every entry (or the directory indices in `select`, in that order, repeats allowed) ->
    [(name, status_name, bytes)].  Entries are independent: a damaged one has a status other than "Ok", and its bytes are
    not to be used; the others are whole.  Raises `Error` for a bad directory or a selection out of range."""
    eng = _engine.default_engine(device)
    src = _raw(src)
    info, ents = _directory(eng.lib, src)
    idx = list(range(info.entries)) if select is None else [int(i) for i in select]
    if any(i < 0 or i >= info.entries for i in idx):
        raise _engine.Error("Invalid argument: selected entry out of range")
    k = len(idx)
    need = sum(ents[i].usize for i in idx)
    sel = (ctypes.c_uint64 * max(k, 1))(*idx)
    dst = ctypes.create_string_buffer(max(need, 1))
    out_off, status, res = (ctypes.c_uint64 * (k + 1))(), (ctypes.c_int32 * max(k, 1))(), ZipResult()
    st = eng.lib.md_zip_uncompress(eng.ctx, src, len(src), sel, k, dst, need, out_off, status, ctypes.byref(res))
    if st != 0:
        eng._check(st)
    raw = dst.raw
    return [(src[ents[i].name_off:ents[i].name_off + ents[i].name_len], _engine.STATUS_NAMES.get(status[j], str(status[j])),
             raw[out_off[j]:out_off[j + 1]]) for j, i in enumerate(idx)]


def _sources(files):
    """[(name, bytes)] (or (name, bytes, external_attr, dos_time, dos_date)) -> (md_zip_source array, the packed bytes)"""
    arr = (ZipSource * max(len(files), 1))()
    blob, at = [], 0
    for s, f in zip(arr, files):
        name, data = f[0], _raw(f[1])
        name = name.encode("utf-8") if isinstance(name, str) else bytes(name)
        s.name, s.name_len, s.off, s.len = name, len(name), at, len(data)
        # (default: a regular file rw-r--r--, 1980-01-01 00:00)
        s.external_attr, s.dos_time, s.dos_date = (f[2], f[3], f[4]) if len(f) == 5 else (0o100644 << 16, 0, 0x21)
        blob.append(data)
        at += len(data)
    return arr, b"".join(blob)


def compress_bound(files):
    """room that always suffices for `compress` of these files (host arithmetic, no device needed); 0: a name is refused"""
    arr, _ = _sources(files)
    return _load().md_zip_compress_bound(len(files), arr)


def compress(files, level=6, dst_len=None, device=0):
    """md_zip_compress: [(name, bytes)] -> the archive's bytes.  All files go through one deflate launch; a file that does
    not get shorter is stored.  The bytes depend on (files, level) alone.  Raises `Error` with the status' name."""
    eng = _engine.default_engine(device)
    arr, blob = _sources(files)
    if dst_len is None:
        dst_len = eng.lib.md_zip_compress_bound(len(files), arr)
    dst = ctypes.create_string_buffer(max(dst_len, 1))
    wrote = ctypes.c_size_t()
    st = eng.lib.md_zip_compress(eng.ctx, level, len(files), arr, blob, len(blob), dst, dst_len, ctypes.byref(wrote))
    if st < 0:
        eng._check(st)
    if st != 0:
        raise _engine.Error(_engine.STATUS_NAMES[st])
    return dst.raw[:wrote.value]
