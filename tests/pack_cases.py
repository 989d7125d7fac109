"""The families of packfile cases the CPU and GPU tests share.  A case is a dict:

  name      unique
  entries   for pack_writer.write_pack, with `kw` (its keyword arguments)
  well      True: a pack git itself accepts and reads as the model does; False: one git index-pack refuses
  idx_only  True: the pack is sound and only the idx (or which idx goes with it) is bent: git index-pack has no word on it
  rc        what md_pack_open returns (default 0)
  expect    {entry: status} of md_pack_read of everything without MD_PACK_VERIFY_CRC; entries not named are Ok
  verify    the same with MD_PACK_VERIFY_CRC, where it differs
  edges     the edges of the issue's list that the case holds
  git_reads False: git index-pack accepts the pack, but git's own readers cannot read it back (one case, the reason beside it)
  claim     a function of the built case -> bool: the edge is really in the bytes (checked by the CPU test)

W is the apply kernel's window: the payload bytes one step looks at."""
import hashlib
import random
import struct

from tests import pack_model as pm
from tests import pack_writer as pw

W = 64


def text(n, seed):
    """n bytes that deflate quickly and well, and differ everywhere"""
    rng = random.Random(seed)
    words = [bytes(rng.randrange(97, 123) for _ in range(rng.randrange(2, 9))) for _ in range(200)]
    out = bytearray()
    while len(out) < n:
        out += rng.choice(words) + b" "
        if rng.random() < 0.05:
            out += b"%d\n" % rng.randrange(1 << 30)
    return bytes(out[:n])


BIG = text(140000, 1)     # its size takes 3 bytes of varint
SMALL = text(100, 2)      # 1 byte
MID = text(3000, 3)


COMMIT = b"tree 4b825dc642cb6eb9a060e54bf8d69288fbee4904\nauthor a <a@b> 0 +0000\ncommitter a <a@b> 0 +0000\n\nm\n"


def blob(data, **kw):
    return dict({"type": 3, "data": data}, **kw)


def delta(base, ins, kind="ofs", **kw):
    return dict({"delta": kind, "base": base, "ins": ins}, **kw)


def _all_copy_opcodes():
    """every opcode 0x80 .. 0xff once: the bytes a mask names are written even where they are 0"""
    ins = []
    for mask in range(128):
        off = (0x21 if mask & 1 else 0) | (0x0300 if mask & 2 else 0) | (0x010000 if mask & 4 else 0)
        size = (5 if mask & 0x10 else 0) | (0x100 if mask & 0x20 else 0)
        ins.append(("copy", off, size or 0x10000, mask))
    return ins


def _mixed(n, seed):
    """n instructions of 2 and 3 bytes, so that the starts fall on every lane"""
    rng = random.Random(seed)
    ins = []
    for k in range(n):
        if rng.random() < 0.5:
            ins.append(("insert", bytes([65 + k % 26])))
        else:
            ins.append(("copy", 1 + rng.randrange(200), 1 + rng.randrange(40), 0x11))
    return ins


def _edit(prev, k):
    """the instructions that turn version k - 1 into version k: a copy, an insert, a copy"""
    at = (37 * k) % (len(prev) - 40) + 1
    return [("copy", 0, at), ("insert", b"<v%d>" % k), ("copy", at + 3, len(prev) - at - 3)]


def _chain(depth, kinds, base=MID):
    entries = [blob(base)]
    cur = base
    for k in range(1, depth + 1):
        ins = _edit(cur, k)
        entries.append(delta(k - 1, ins, kinds[k % len(kinds)]))
        cur = pw._result(cur, ins)
    return entries


def _payload(ins, base_len, result_len):
    return pw.leb128(base_len) + pw.leb128(result_len) + pw.encode_instructions(ins)


def _name(s):
    return hashlib.sha1(s).digest()


def cases():
    out = []

    def add(name, entries, edges, well=True, expect=None, claim=None, **more):
        out.append(dict({"name": name, "entries": entries, "kw": more.pop("kw", {}), "well": well, "idx_only": False, "rc": 0,
                         "expect": expect or {}, "edges": set(edges), "claim": claim, "git_reads": True}, **more))

    D = pm.INVALID_DELTA
    # ---- instructions ----
    add("all 128 copy opcodes", [blob(BIG), delta(0, _all_copy_opcodes())], ["copy opcodes 0x80..0xff"],
        claim=lambda c: [pw.copy_op(*i[1:])[0] for i in c["entries"][1]["ins"]] == list(range(0x80, 0x100)))
    add("copy sizes 0x10000 and 0x10001", [blob(BIG), delta(0, [("copy", 7, 0x10000), ("copy", 3, 0x10001)])], ["size 0 is 0x10000", "size 0x10001"],
        claim=lambda c: pw.copy_op(7, 0x10000) == b"\x81\x07" and pw.copy_op(3, 0x10001) == b"\xd1\x03\x01\x01")
    lens = (1, 15, 16, 17, 63, 64, 65)
    add("copy lengths", [blob(MID), delta(0, [("copy", 3 + 101 * k, n) for k, n in enumerate(lens)])], ["copy lengths 1 15 16 17 63 64 65"])
    add("copy to the base's end", [blob(MID), delta(0, [("copy", len(MID) - 10, 10)])], ["copy ends at the base's end"])
    add("copy one past the base's end", [blob(MID), delta(0, [("copy", len(MID) - 10, 11)], result_size=11)], ["copy one byte past the base"],
        well=False, expect={1: D})
    add("overlapping and repeated sources", [blob(MID), delta(0, [("copy", 0, 100), ("copy", 50, 100), ("copy", 0, 100), ("copy", 0, 100), ("copy", 99, 2)])],
        ["overlapping and repeated source ranges"])
    add("inserts of 1 and 127", [blob(SMALL), delta(0, [("insert", b"x"), ("insert", bytes(range(127))), ("insert", b"y")])], ["inserts of 1 and 127"])
    counts = (W - 1, W, W + 1, 2 * W - 1, 2 * W + 1)
    add("instruction counts around the window", [blob(MID)] + [delta(0, _mixed(n, n)) for n in counts],
        ["instruction counts W-1 W W+1 2W-1 2W+1"], claim=lambda c: [len(e["ins"]) for e in c["entries"][1:]] == list(counts))
    add("five thousand one-byte instructions", [blob(MID), delta(0, [("insert", bytes([k % 251])) if k & 1 else ("copy", k % 2999, 1) for k in range(5000)])],
        ["thousands of one-byte instructions"])
    # (git index-pack accepts it and writes the same idx; git's readers take a delta's result size of 0 for a failure, so
    # cat-file and verify-pack have no word on this one pack: git_reads)
    add("a delta of no instructions", [blob(BIG), delta(0, [])], ["no instructions, result size 0"], git_reads=False)
    add("opcode 0", [blob(MID), delta(0, [("copy", 0, 10), ("raw", b"\0"), ("copy", 0, 10)], result_size=20)], ["opcode 0"], well=False, expect={1: D})
    add("cut inside a copy's operands", [blob(MID), delta(0, [("insert", b"abc"), ("copy", 0x102, 0x203)], cut=2, result_size=3 + 0x203)],
        ["payload cut inside a copy"], well=False, expect={1: D})
    add("cut inside an insert", [blob(MID), delta(0, [("copy", 0, 9), ("insert", b"0123456789")], cut=4, result_size=19)],
        ["payload cut inside an insert"], well=False, expect={1: D})
    add("result size one too small", [blob(MID), delta(0, [("copy", 0, 50), ("insert", b"zz")], result_size=51)], ["result size one too small"],
        well=False, expect={1: D})
    add("result size one too large", [blob(MID), delta(0, [("copy", 0, 50), ("insert", b"zz")], result_size=53)], ["result size one too large"],
        well=False, expect={1: D})
    add("base size mismatch", [blob(MID), delta(0, [("copy", 0, 50)], base_size=len(MID) + 1, result_size=50)], ["base size mismatch"],
        well=False, expect={1: D})
    add("size varints of 1 to 5 bytes", [blob(SMALL)] + [delta(0, [("copy", k, 20 + k)], size_bytes=k) for k in range(1, 6)],
        ["size varints of 1 to 5 bytes"])
    add("a size varint beyond 64 bits", [blob(SMALL), delta(0, [], payload=pw.leb128(100) + b"\xff" * 9 + b"\x7f" + b"\x90\x05")],
        ["size varint overflows 64 bits"], well=False, expect={1: D})
    # ---- chains ----
    add("a chain of 64, OFS and REF mixed", _chain(64, ("ofs", "ref")), ["depth 1", "depth 2", "depth 50", "depth 64", "OFS and REF in one chain"])
    add("a REF base later in the pack", [delta(1, [("copy", 5, 500), ("insert", b"!")], "ref"), blob(MID)], ["REF base later in the pack"],
        claim=lambda c: c["layout"][0]["offset"] < c["layout"][1]["offset"])
    add("a fan of 1000", [blob(MID)] + [delta(0, [("copy", k, 100), ("insert", b"%d" % k)], "ofs" if k & 1 else "ref") for k in range(1000)],
        ["fan of 1000 deltas"])
    add("a REF base that is missing", [blob(MID), delta(None, [("copy", 0, 10)], "ref", base_name=_name(b"nowhere"), base_size=len(MID), result_size=10),
                                       delta(1, [("copy", 0, 5)], "ofs", base_size=10, result_size=5)],
        ["REF base missing"], well=False, expect={1: pm.MISSING_BASE, 2: pm.INVALID_PACK_BASE})
    n0, n1, n2 = _name(b"cycle 0"), _name(b"cycle 1"), _name(b"cycle 2")
    cyc = dict(base_size=10, result_size=10)
    add("a REF cycle of two", [blob(MID), delta(None, [("copy", 0, 10)], "ref", base_name=n1, name=n0, **cyc),
                               delta(None, [("copy", 0, 10)], "ref", base_name=n0, name=n1, **cyc),
                               delta(None, [("copy", 0, 10)], "ref", base_name=n0, **cyc), delta(0, [("copy", 0, 10)])],
        ["REF cycle of two with an innocent delta"], well=False, expect={1: pm.INVALID_PACK, 2: pm.INVALID_PACK, 3: pm.INVALID_PACK})
    add("a REF cycle of three", [delta(None, [("copy", 0, 10)], "ref", base_name=n1, name=n0, **cyc),
                                 delta(None, [("copy", 0, 10)], "ref", base_name=n2, name=n1, **cyc),
                                 delta(None, [("copy", 0, 10)], "ref", base_name=n0, name=n2, **cyc),
                                 delta(None, [("copy", 0, 10)], "ref", base_name=n2, **cyc), blob(SMALL)],
        ["REF cycle of three with an innocent delta"], well=False, expect={k: pm.INVALID_PACK for k in range(4)})
    add("a REF delta of itself", [blob(SMALL), delta(None, [("copy", 0, 10)], "ref", base_name=n0, name=n0, **cyc)], ["REF cycle of one"],
        well=False, expect={1: pm.INVALID_PACK})
    for label, kw in (("0", {"ofs": 0}), ("beyond the object's own offset", {"ofs": 1 << 20}), ("to no object's start", {"ofs_adjust": -1})):
        add("an OFS offset " + label, [blob(MID), delta(0, [("copy", 0, 10)], base_size=len(MID), result_size=10, **kw), blob(SMALL)],
            ["OFS offset " + label], well=False, expect={1: pm.INVALID_PACK})
    add("a root that fails its checksum", [blob(MID, bad_adler=True), delta(0, [("copy", 0, 100)]), delta(1, [("copy", 0, 50)]), blob(SMALL),
                                           delta(3, [("copy", 1, 9)])],
        ["chain whose root fails its zlib checksum"], well=False, expect={0: pm.INVALID_CHECKSUM, 1: pm.INVALID_PACK_BASE, 2: pm.INVALID_PACK_BASE})
    # ---- headers and framing ----
    add("type 0", [blob(SMALL), blob(MID, raw_type=0)], ["type 0"], well=False, expect={1: pm.INVALID_PACK})
    add("type 5", [blob(MID, raw_type=5), blob(SMALL)], ["type 5"], well=False, expect={0: pm.INVALID_PACK})
    add("header size varints of 1 to 10 bytes", [blob(b"tiny %02d" % k, hdr_bytes=k) for k in range(1, 11)], ["header size varints of 1 to 10 bytes"],
        claim=lambda c: [c["layout"][k]["packed_len"] - c["layout"][0]["packed_len"] for k in range(10)] == list(range(10)))
    add("a header size beyond 64 bits", [blob(SMALL), {"type": 3, "data": b"tiny", "hdr_bytes": 11, "hsize": 4 | 1 << 67}], ["header size overflows 64 bits"],
        well=False, expect={1: pm.INVALID_PACK})
    add("header size one too small", [blob(MID, hsize=len(MID) - 1), blob(SMALL)], ["header size below the inflated size"], well=False,
        expect={0: pm.INVALID_SIZE})
    add("header size one too large", [blob(MID, hsize=len(MID) + 1), blob(SMALL)], ["header size above the inflated size"], well=False,
        expect={0: pm.INVALID_SIZE})
    add("a spare byte between two objects", [blob(MID, spare=b"\0"), blob(SMALL)], ["spare byte between two objects"], well=False,
        expect={0: pm.INVALID_SIZE})
    add("a wrong idx CRC", [blob(MID), delta(0, [("copy", 0, 10)]), blob(SMALL)], ["wrong idx CRC seen only with verify"], well=False, idx_only=True,
        kw={"idx_crc": {0: 0x12345678}}, verify={0: pm.INVALID_CHECKSUM, 1: pm.INVALID_PACK_BASE})
    add("pack version 3", [blob(MID), delta(0, [("copy", 0, 10)])], ["pack version 3"], kw={"version": 3})
    add("pack version 4", [blob(MID)], ["pack version 4"], well=False, kw={"version": 4}, rc=pm.UNSUPPORTED)
    add("pack magic", [blob(MID)], ["pack magic"], well=False, kw={"magic": b"PACX"}, rc=pm.INVALID_PACK)
    add("count other than the idx's", [blob(MID), blob(SMALL)], ["count != idx count"], well=False, kw={"count": 3}, rc=pm.INVALID_INDEX)
    add("a trailer that is not the idx's pack checksum", [blob(MID)], ["pack trailer != idx pack checksum"], well=False, idx_only=True,
        kw={"idx_pack_checksum": _name(b"another pack")}, rc=pm.INVALID_INDEX)
    add("an empty pack", [], ["empty pack"])
    add("an empty blob", [blob(b""), blob(SMALL)], ["empty blob"])
    add("every type", [{"type": 1, "data": COMMIT},
                       {"type": 2, "data": b""}, blob(SMALL), {"type": 4, "data": b"object " + b"0" * 40 + b"\ntype blob\ntag t\ntagger a <a@b> 0 +0000\n\nm\n"},
                       delta(0, [("copy", 0, 46), ("insert", b"\nauthor b <b@c> 1 +0000\n"), ("copy", 46, len(COMMIT) - 46)])], ["every type, a delta of a commit"])
    add("an idx with a 64-bit table", [blob(MID), delta(0, [("copy", 0, 10)]), blob(SMALL)], ["idx with a 64-bit table"], well=False, idx_only=True,
        kw={"idx_64bit": True}, claim=lambda c: pm.read_idx(c["idx"])[2]["has64"] == 1)
    return out


REQUIRED_EDGES = {
    "copy opcodes 0x80..0xff", "size 0 is 0x10000", "size 0x10001", "copy lengths 1 15 16 17 63 64 65", "copy ends at the base's end",
    "copy one byte past the base", "overlapping and repeated source ranges", "inserts of 1 and 127", "instruction counts W-1 W W+1 2W-1 2W+1",
    "thousands of one-byte instructions", "no instructions, result size 0", "opcode 0", "payload cut inside a copy", "payload cut inside an insert",
    "result size one too small", "result size one too large", "base size mismatch", "size varints of 1 to 5 bytes", "size varint overflows 64 bits",
    "depth 1", "depth 2", "depth 50", "depth 64", "OFS and REF in one chain", "REF base later in the pack", "fan of 1000 deltas", "REF base missing",
    "REF cycle of two with an innocent delta", "REF cycle of three with an innocent delta", "OFS offset 0", "OFS offset beyond the object's own offset",
    "OFS offset to no object's start", "chain whose root fails its zlib checksum", "type 0", "type 5", "header size varints of 1 to 10 bytes",
    "header size below the inflated size", "header size above the inflated size", "spare byte between two objects",
    "wrong idx CRC seen only with verify", "pack version 3", "pack version 4", "pack magic", "count != idx count", "pack trailer != idx pack checksum",
    "empty pack", "empty blob", "idx with a 64-bit table",
}


def build(case):
    """the case with its bytes: pack, idx, layout, order (entry -> index in the idx)"""
    c = dict(case)
    c["pack"], c["idx"], c["layout"] = pw.write_pack(case["entries"], **case["kw"])
    c["order"] = pw.idx_order(c["layout"])
    return c


def index_cases():
    """(label, idx bytes, md_pack_index's status): one valid idx, with and without a 64-bit table, and every refusal"""
    entries = [blob(text(50 + k, 100 + k)) for k in range(40)]
    pack, good, layout = pw.write_pack(entries)
    _, big, _ = pw.write_pack(entries, idx_64bit=True)
    n = len(entries)
    names_at, off_at = 1032, 1032 + 24 * n

    def poke(b, at, fmt, v):
        b = bytearray(b)
        struct.pack_into(fmt, b, at, v)
        return bytes(b)

    first = good[names_at]  # the least name's first byte: no name lies below it
    assert first < 255 and struct.unpack_from(">I", good, 8 + 4 * first)[0] >= 1
    swapped = bytearray(good)
    swapped[names_at:names_at + 20], swapped[names_at + 20:names_at + 40] = good[names_at + 20:names_at + 40], good[names_at:names_at + 20]
    out = [
        ("good", good, pm.OK), ("good, 64-bit table", big, pm.OK),
        ("a fan-out that decreases", poke(good, 8 + 4 * (first + 1), ">I", 0), pm.INVALID_INDEX),
        ("a name outside its fan-out bucket", poke(good, 8 + 4 * first, ">I", 0), pm.INVALID_INDEX),
        ("names that do not ascend", bytes(swapped), pm.INVALID_INDEX),
        ("equal names", good[:names_at + 20] + good[names_at:names_at + 20] + good[names_at + 40:], pm.INVALID_INDEX),
        ("an escape outside the 64-bit table", poke(big, off_at, ">I", 0x80000000 | n), pm.INVALID_INDEX),
        ("an escape without a table", poke(good, off_at, ">I", 0x80000000), pm.INVALID_INDEX),
        ("too short: the header alone", good[:8], pm.INVALID_INDEX),
        ("too short: four bytes", good[:4], pm.INVALID_INDEX),
        ("too short: one byte missing", good[:-1], pm.INVALID_INDEX),
        ("bytes left over", good + b"\0", pm.INVALID_INDEX),
        ("eight bytes left over", good + bytes(8), pm.INVALID_INDEX),
        ("a count above the file", poke(good, 8 + 4 * 255, ">I", n + 1), pm.INVALID_INDEX),
        ("version 1: no magic", struct.pack(">256I", *[min(k, n) for k in range(256)]) + good[names_at:], pm.UNSUPPORTED),
        ("version 3", poke(good, 4, ">I", 3), pm.UNSUPPORTED),
        ("32-byte names", good[:names_at] + b"".join(good[names_at + 20 * k:names_at + 20 * k + 20] + bytes(12) for k in range(n)) + good[names_at + 20 * n:],
         pm.INVALID_INDEX),
    ]
    return out, pack, layout
