"""A ZIP archive written byte by byte (PKWARE APPNOTE 4.3-4.5), with a switch for every form the reader has to take:
method per entry, data descriptors with and without their signature, extra fields that differ between local header and
directory, the ZIP64 extra field in the directory (fixed fields all-ones, small real values), the ZIP64 end record and
locator, bytes in front of the archive, an archive comment, and a comment that contains an end record's signature.
The witness for all of them is Python's zipfile (test_zip_util.py), not the code under test."""
import struct
import zlib

SIG_LOCAL, SIG_CENTRAL, SIG_END, SIG_END64, SIG_LOC64, SIG_DESC = (b"PK\3\4", b"PK\1\2", b"PK\5\6", b"PK\6\6", b"PK\6\7", b"PK\7\x08")
FAKE_END_COMMENT = SIG_END + b"\0" * 18 + b"yy"  # an "end record" of no entries whose comment would end 2 bytes early


def raw_deflate(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def entry(name, data, method=8, level=6, descriptor=None, local_extra=b"", dir_extra=b"", zip64_dir=False, flags=0, body=None):
    """descriptor: None, "sig" (PK\\7\\8 crc csize usize behind the body) or "nosig" (crc csize usize); with one the local
    header's crc and sizes are zero and flag bit 3 is set.  zip64_dir: the directory's usize, csize and offset are all-ones
    and the ZIP64 extra field 0x0001 carries them.  body: the entry's bytes in the archive, when not those of `data`."""
    name = name.encode("utf-8") if isinstance(name, str) else name
    if any(b >= 0x80 for b in name):
        flags |= 0x0800
    if descriptor:
        flags |= 8
    if body is None:
        body = raw_deflate(data, level) if method == 8 else data
    return dict(name=name, data=data, method=method, descriptor=descriptor, local_extra=local_extra, dir_extra=dir_extra,
                zip64_dir=zip64_dir, flags=flags, body=body, crc=zlib.crc32(data), usize=len(data), csize=len(body))


def extra_field(tag, payload):
    return struct.pack("<HH", tag, len(payload)) + payload


def archive(entries, prefix=b"", comment=b"", zip64_end=False):
    """-> (the archive's bytes, layout): layout[i] = where entry i's local header, body and central header lie (offsets in
    the returned bytes, prefix included)"""
    out = bytearray()
    layout = []
    for e in entries:
        at = len(out)
        d = bool(e["descriptor"])
        out += SIG_LOCAL + struct.pack("<HHHHHIIIHH", 20, e["flags"], e["method"], 0, 0x21, 0 if d else e["crc"], 0 if d else e["csize"],
                                       0 if d else e["usize"], len(e["name"]), len(e["local_extra"]))
        out += e["name"] + e["local_extra"]
        layout.append(dict(local=len(prefix) + at, body=len(prefix) + len(out)))
        out += e["body"]
        if d:
            out += (SIG_DESC if e["descriptor"] == "sig" else b"") + struct.pack("<III", e["crc"], e["csize"], e["usize"])
        e["offset"] = at
    dir_off = len(out)
    for e, where in zip(entries, layout):
        where["central"] = len(prefix) + len(out)
        z = e["zip64_dir"]
        extra = (extra_field(1, struct.pack("<QQQ", e["usize"], e["csize"], e["offset"])) if z else b"") + e["dir_extra"]
        out += SIG_CENTRAL + struct.pack("<HHHHHHIIIHHHHHII", 3 << 8 | 20, 45 if z else 20, e["flags"], e["method"], 0, 0x21, e["crc"],
                                         0xffffffff if z else e["csize"], 0xffffffff if z else e["usize"], len(e["name"]), len(extra), 0, 0, 0,
                                         0o100644 << 16, 0xffffffff if z else e["offset"])
        out += e["name"] + extra
    dir_size, n = len(out) - dir_off, len(entries)
    if zip64_end:
        at = len(out)
        out += SIG_END64 + struct.pack("<QHHIIQQQQ", 44, 45, 45, 0, 0, n, n, dir_size, dir_off)
        out += SIG_LOC64 + struct.pack("<IQI", 0, at, 1)
        out += SIG_END + struct.pack("<HHHHIIH", 0xffff, 0xffff, 0xffff, 0xffff, 0xffffffff, 0xffffffff, len(comment)) + comment
    else:
        out += SIG_END + struct.pack("<HHHHIIH", 0, 0, n, n, dir_size, dir_off, len(comment)) + comment
    return bytes(prefix) + bytes(out), layout


def sample_files(seed=1):
    """a few small files of different kinds: text that compresses, bytes that do not, an empty one, a one-byte one"""
    import random
    rng = random.Random(seed)
    text = bytes(rng.choice(b"abcdefgh \n") for _ in range(30000))
    return [("a/text.txt", text), ("a/noise.bin", rng.randbytes(5000)), ("empty", b""), ("one", b"x"),
            ("dir/", b""), ("naïve.txt", text[:777]), ("zeros", bytes(70000))]


def forms(seed=1):
    """(label, archive, [(name bytes, data)]) for every switch alone, then all of them behind a prefix"""
    files = sample_files(seed)
    plain = lambda **kw: [entry(n, d, method=8 if d else 0, **kw) for n, d in files]
    want = [(n.encode("utf-8"), d) for n, d in files]
    prefix = b"#!/bin/sh\nexec unzip \"$0\"\n" + b"\0" * 37
    cases = [
        ("deflated", dict(entries=plain())),
        ("stored", dict(entries=[entry(n, d, method=0) for n, d in files])),
        ("mixed", dict(entries=[entry(n, d, method=8 if (i & 1 and d) else 0) for i, (n, d) in enumerate(files)])),
        ("descriptor_sig", dict(entries=plain(descriptor="sig"))),
        ("descriptor_nosig", dict(entries=plain(descriptor="nosig"))),
        ("extras_differ", dict(entries=plain(local_extra=extra_field(0x5455, b"\3" + b"\1" * 8) + extra_field(0x7875, b"\1\4" + b"\0" * 8),
                                             dir_extra=extra_field(0x5455, b"\1" + b"\1" * 4)))),
        ("zip64_dir", dict(entries=plain(zip64_dir=True, dir_extra=extra_field(0x5455, b"\1" + b"\2" * 4)))),
        ("zip64_end", dict(entries=plain(), zip64_end=True)),
        ("prefix", dict(entries=plain(), prefix=prefix)),
        ("comment", dict(entries=plain(), comment=b"an archive comment")),
        ("levels", dict(entries=[entry(n, d, method=8, level=1 + i % 9) for i, (n, d) in enumerate(files)])),
        ("everything", dict(entries=[entry(n, d, method=8 if (i & 1 and d) else 0, descriptor=(None, "sig", "nosig")[i % 3], zip64_dir=i % 2 == 0,
                                           local_extra=extra_field(0x7875, b"\1\4" + bytes(8)) if i % 3 == 0 else b"")
                                     for i, (n, d) in enumerate(files)], zip64_end=True, comment=b"c" * 300)),
    ]
    for label, kw in cases:
        yield label, archive(**kw)[0], want
        if "prefix" not in kw:
            yield label + "+prefix", archive(prefix=prefix, **kw)[0], want


def fake_end_archive(seed=1):
    """-> (archive, [(name, data)]): its comment holds PK\\5\\6 + 18 NULs + "yy".  Python 3.10's zipfile takes that for the
    end record and reports an empty archive; the real record is the one whose comment ends with the file."""
    files = sample_files(seed)[:3]
    return archive([entry(n, d) for n, d in files], comment=FAKE_END_COMMENT)[0], [(n.encode("utf-8"), d) for n, d in files]


def zipfile_bytes(files, compression, level=None, comment=b""):
    """the same files written by Python's zipfile"""
    import io
    import zipfile
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", compression, compresslevel=level) as z:
        for n, d in files:
            z.writestr(zipfile.ZipInfo(n if isinstance(n, str) else n.decode("utf-8")), d, compress_type=compression, compresslevel=level)
        z.comment = comment
    return buf.getvalue()
