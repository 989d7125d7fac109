"""Helpers of the many-member GZip tests: files written on the CPU with Python's zlib and struct alone (never by the code
under test) - BGZF as bgzip writes it, RFC 1952 members with FEXTRA / FNAME / FCOMMENT / FHCRC - and libz's reading of a
whole file (zlib with wbits 31, member after member), the yardstick for what md_gz_members_uncompress says."""
import struct
import zlib

EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
BLOCK = 0xff00


def raw_deflate(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def member(data, level=6, extra=None, name=None, comment=None, hcrc=False, flg_or=0, cm=8, body=None, mtime=0, os=255):
    """one RFC 1952 member; extra = the extra field's bytes (None: no FEXTRA)"""
    flg = (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0) | (2 if hcrc else 0) | flg_or
    h = struct.pack("<BBBBIBB", 0x1f, 0x8b, cm, flg, mtime, 0, os)
    if extra is not None:
        h += struct.pack("<H", len(extra)) + extra
    if name is not None:
        h += name + b"\0"
    if comment is not None:
        h += comment + b"\0"
    if hcrc:
        h += struct.pack("<H", zlib.crc32(h) & 0xffff)
    body = raw_deflate(data, level) if body is None else body
    return h + body + struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff)


def bgzf_member(data, level=6, before=b"", after=b"", **kw):
    """a member with the BC size field; before / after: other subfields around it in the extra field"""
    assert len(data) <= 0x10000
    probe = member(data, level, extra=before + b"BC\x02\x00\0\0" + after, **kw)
    return member(data, level, extra=before + b"BC\x02\x00" + struct.pack("<H", len(probe) - 1) + after, **kw)


def subfield(si, payload):
    return si + struct.pack("<H", len(payload)) + payload


def bgzf_file(data, block=BLOCK, level=6, eof=True, **kw):
    """-> (file, [(compressed offset, uncompressed offset)] of its members, the EOF marker included)"""
    out, idx = [], []
    pos = 0
    for u in range(0, len(data), block):
        idx.append((pos, u))
        out.append(bgzf_member(data[u:u + block], level, **kw))
        pos += len(out[-1])
    if eof:
        idx.append((pos, len(data)))
        out.append(EOF_MARKER)
    return b"".join(out), idx


def bgzf_of_members(chunks, level=6, eof=True):
    """members of the given payloads (empty ones allowed) -> (file, index)"""
    out, idx, pos, u = [], [], 0, 0
    for c in chunks:
        idx.append((pos, u))
        out.append(bgzf_member(c, level))
        pos += len(out[-1])
        u += len(c)
    if eof:
        idx.append((pos, u))
        out.append(EOF_MARKER)
    return b"".join(out), idx


def walk_bsize(f):
    """member offsets of a file of BGZF members by their BSIZE fields alone (BC first in the extra field) -> offsets, end"""
    pos, offs = 0, []
    while pos < len(f) and f[pos] != 0:
        assert f[pos:pos + 4] == b"\x1f\x8b\x08\x04" and f[pos + 12:pos + 16] == b"BC\x02\x00", pos
        offs.append(pos)
        pos += struct.unpack_from("<H", f, pos + 16)[0] + 1
    return offs, pos


def libz_members(data):
    """RFC 1952 as libz reads it: every member through zlib (wbits 31), NUL bytes behind a member skipped ->
    ("ok", bytes, members) | ("error", bytes of the members in front of the failing one, members, its offset)"""
    out, pos, members = [], 0, 0
    while True:
        if members:
            while pos < len(data) and data[pos] == 0:
                pos += 1
        if pos == len(data):
            return "ok", b"".join(out), members
        d = zlib.decompressobj(31)
        try:
            piece = d.decompress(data[pos:])
        except zlib.error:
            return "error", b"".join(out), members, pos
        if not d.eof:
            return "error", b"".join(out), members, pos
        out.append(piece)
        pos = len(data) - len(d.unused_data)
        members += 1
