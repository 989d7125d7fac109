"""Packfile cases for MD_PACK_VERIFY_NAME, in the form of tests/pack_cases.py (built with pack_cases.build).  Every pack here
is sound but for the names its idx gives: a read without the flag sees every object as Ok.  A case adds to that form:

  names     {entry: status} of a read of everything with MD_PACK_VERIFY_NAME; entries not named are Ok
  both      the same with MD_PACK_VERIFY_NAME | MD_PACK_VERIFY_CRC, where it differs
  select    entries to read instead of everything (repeats allowed), with `selected`: their statuses in that order

The sizes come from the kernel's paths: header + content = L bytes is hashed in (L + 9 + 63) // 64 blocks, block 0 and the
last one or two are put together byte by byte, and the header's length moves with the size's digits."""
import hashlib

from tests import pack_cases as pc
from tests import pack_model as pm
from tests import pack_writer as pw

TREE = b"100644 a\0" + bytes(range(20)) + b"100644 b\0" + bytes(range(20, 40))
TAG = b"object " + b"0" * 40 + b"\ntype blob\ntag t\ntagger a <a@b> 0 +0000\n\nm\n"
EDGE_REMAINDERS = (0, 1, 55, 56, 57, 63)


def wrong(k):
    return hashlib.sha1(b"a wrong name %d" % k).digest()


def message_length(type_, size):
    """header + content"""
    return len(pw.TYPE_NAMES[type_]) + 1 + len(str(size)) + 1 + size


def edge_sizes():
    """blob sizes whose message length is 64 b + r for b = 0, 1, 2 full blocks and r of EDGE_REMAINDERS (a blob's message
    has 7 bytes at the least: no 0 and no 1)"""
    out = []
    for b in range(3):
        for r in EDGE_REMAINDERS:
            want = 64 * b + r
            out += [s for s in range(want) if message_length(3, s) == want]
    return out


def cases():
    out = []

    def add(name, entries, names=None, **more):
        out.append(dict({"name": name, "entries": entries, "kw": more.pop("kw", {}), "well": False, "idx_only": True, "rc": 0, "expect": {},
                         "names": names or {}, "edges": set(), "claim": None, "git_reads": True}, **more))

    C, B = pm.INVALID_CHECKSUM, pm.INVALID_PACK_BASE
    blob, delta = pc.blob, pc.delta
    add("a wrong name on a lone object", [blob(pc.SMALL, name=wrong(0)), blob(pc.MID)], {0: C})
    add("a wrong name on a base of two", [blob(pc.text(90, 11)), blob(pc.MID, name=wrong(1)), delta(1, [("copy", 0, 100)]), delta(1, [("copy", 7, 300)], "ref"),
                                          blob(pc.text(700, 12)), delta(4, [("copy", 1, 500), ("insert", b"!")])], {1: C, 2: B, 3: B})
    chain = pc._chain(4, ("ofs",))
    chain[2] = dict(chain[2], name=wrong(2))
    add("a wrong name in the middle of a chain", chain, {2: C, 3: B, 4: B}, select=[4], selected=[B])
    add("a wrong name selected twice", [blob(pc.SMALL, name=wrong(3)), blob(pc.MID)], {0: C}, select=[0, 1, 0, 1], selected=[C, 0, C, 0])
    add("a delta and its base both misnamed", [blob(pc.MID, name=wrong(4)), delta(0, [("copy", 0, 64)], name=wrong(5))], {0: C, 1: B})
    add("a tree's bytes stored as a blob", [{"type": 2, "data": TREE, "raw_type": 3}, {"type": 2, "data": TREE + TREE}], {0: C})
    last = bytearray(pw.object_name(3, pc.MID))
    last[19] ^= 1
    add("a name wrong in its last byte", [blob(pc.MID, name=bytes(last)), blob(pc.SMALL)], {0: C})
    add("the empty blob alone", [blob(b"")])
    sizes = edge_sizes()
    base = pc.text(400, 21)
    add("message lengths around the block", [blob(pc.text(s, 300 + k)) for k, s in enumerate(sizes)] + [blob(base)] +
        [delta(len(sizes), [("copy", 1 + k, s)] if s else []) for k, s in enumerate(sizes)], sizes=sizes)
    digits = (9, 10, 99, 100, 999, 1000)
    big = pc.text(1200, 22)
    add("sizes where the header grows", [blob(pc.text(s, 400 + s)) for s in digits] + [blob(big)] + [delta(len(digits), [("copy", 3, s)]) for s in digits],
        sizes=list(digits))
    add("all four types, whole and as deltas", [{"type": 1, "data": pc.COMMIT}, {"type": 2, "data": TREE}, blob(pc.SMALL), {"type": 4, "data": TAG},
                                                delta(0, [("copy", 0, 46), ("insert", b"\nauthor b <b@c> 1 +0000\n"), ("copy", 46, len(pc.COMMIT) - 46)]),
                                                delta(1, [("copy", 0, 29), ("insert", b"100644 c\0" + bytes(20))]), delta(2, [("copy", 10, 80)]),
                                                delta(3, [("copy", 0, len(TAG) - 2), ("insert", b"n\n")], "ref"),
                                                {"type": 4, "data": TAG + b"x", "name": wrong(6)}], {8: C})
    add("a wrong name and a wrong CRC", [blob(pc.MID, name=wrong(7)), delta(0, [("copy", 0, 10)]), blob(pc.SMALL), blob(pc.text(50, 23), name=wrong(8))],
        {0: C, 1: B, 3: C}, kw={"idx_crc": {2: 0x12345678, 3: 0x9abcdef0}}, both={0: C, 1: B, 2: C, 3: C}, verify={2: C, 3: C})
    return out
