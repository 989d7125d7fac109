"""The packs md_pack_index_build is tested with, shared by the CPU and the GPU tests: every case of pack_cases.cases() - the
pack alone, its idx is what the builder has to find - and the builder's own edges.  A built case is a dict:

  name      unique
  pack      the bytes
  flags     of md_pack_index_build (1 = MD_PACK_BUILD_CHECK_TRAILER)
  well      True: git index-pack accepts the pack and writes the idx the model writes
  ours      True: the library accepts what git refuses (one case: a bent trailer that nobody was asked to check)
  idx       pack_writer's idx of the pack, where it wrote one that holds for the pack (None otherwise)
  edges     the edges of the issue's list that the case holds
  claim     a function of the built case -> bool: the edge is really in the bytes (checked by the CPU test)
"""
import functools
import hashlib
import os
import random
import struct
import zlib

from tests import pack_build_model as bm
from tests import pack_cases as pc
from tests import pack_writer as pw

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "git_pack")


def _object_of(c, k):
    return bm.BuildModel(c["pack"], False).objs[k]


def _inner_streams_blob():
    """content of a stored blob: two whole zlib streams, then one whose own Adler-32 is cut off, so that its DEFLATE data ends
    with the content and the four bytes that follow - the blob's own Adler-32 - are what the size query takes for its trailer"""
    a, b, c = zlib.compress(pc.text(700, 11)), zlib.compress(pc.text(900, 12), 9), zlib.compress(pc.text(500, 13))[:-4]
    return b"nested: " + a + b" / " + b + b" / " + c


def _find_tail_candidates():
    """a one-blob pack whose last stream has a passing pair in its last 6 bytes and whose trailer holds another"""
    for k in range(200000):
        pack, idx, layout = pw.write_pack([pc.blob(b"tail %d" % k)])
        end = len(pack) - 20
        near = [z for z in range(end - 5, end) if (pack[z], pack[z + 1]) in bm._PAIRS]
        inside = [z for z in range(end, len(pack) - 1) if (pack[z], pack[z + 1]) in bm._PAIRS]
        if near and inside:
            return k
    raise AssertionError("no such blob")


TAIL_K = 10273  # _find_tail_candidates(), kept: the search takes seconds (the claim checks the bytes)


def _ref_chain(links, behind):
    """a blob and `links` REF_DELTAs, each on the one before; behind: every base lies behind its delta"""
    entries = pc._chain(links, ("ref",), pc.MID)
    if not behind:
        return entries
    n = len(entries)
    out = []
    for k in range(n - 1, -1, -1):
        e = dict(entries[k])
        if "base" in e:
            e["base"] = n - 1 - e["base"]
        out.append(e)
    return out


def _twins(c):
    """every object whose size varint has two or more bytes parses one byte in too, to the same stream"""
    pack, end = c["pack"], len(c["pack"]) - 20
    m = bm.BuildModel(pack, False)
    twins = 0
    for o in m.objs:
        h = bm.parse_header(pack, o["off"] + 1, end)
        twins += h is not None and h[2] == o["z"]
    return m.n == 10 and twins == 9


def _raw_cases():
    out = []

    def add(name, entries, edges, well=True, claim=None, flags=1, ours=False, **kw):
        out.append({"name": name, "entries": entries, "kw": kw, "well": well, "edges": set(edges), "claim": claim, "flags": flags, "ours": ours,
                    "own_idx": True})

    for c in pc.cases():
        # the pack alone: a case whose idx alone is bent is a sound pack here, and the idx knobs are dropped
        kw = {k: v for k, v in c["kw"].items() if not k.startswith("idx_")}
        well = c["well"] or c["idx_only"]
        out.append({"name": c["name"], "entries": c["entries"], "kw": kw, "well": well, "edges": set(), "claim": None, "flags": 1, "ours": False,
                    "own_idx": well})
    rng = random.Random(5)
    noise = bytes(rng.getrandbits(8) for _ in range(256 << 10))
    add("a stored blob that holds zlib streams", [pc.blob(pc.SMALL), pc.blob(_inner_streams_blob(), level=0), pc.blob(pc.MID)],
        ["stored blob with inner zlib streams, one ends on the object's end"],
        claim=lambda c: sum(1 for z, used, _, st in bm.candidate_table(c["pack"])
                            if st == 0 and _object_of(c, 1)["z"] < z and z + used == _object_of(c, 1)["end"]) >= 1
        and sum(1 for z, used, _, st in bm.candidate_table(c["pack"]) if st == 0 and _object_of(c, 1)["z"] < z < _object_of(c, 1)["end"]) >= 3)
    add("a stored blob of 256 KiB of random bytes", [pc.blob(noise, level=0), pc.blob(pc.SMALL)], ["stored random blob, hundreds of false candidates"],
        claim=lambda c: len(bm.candidate_positions(c["pack"])) > 300)
    add("candidates at the pack's tail", [pc.blob(b"tail %d" % TAIL_K)], ["candidate in the last 6 bytes and one inside the trailer"],
        claim=lambda c: any((c["pack"][z], c["pack"][z + 1]) in bm._PAIRS for z in range(len(c["pack"]) - 25, len(c["pack"]) - 20))
        and any((c["pack"][z], c["pack"][z + 1]) in bm._PAIRS for z in range(len(c["pack"]) - 20, len(c["pack"]) - 1))
        and max(bm.candidate_positions(c["pack"])) <= len(c["pack"]) - 26)
    # (sizes of 256 .. 1279: the varint's second byte then holds the type bits 1 .. 4 and is a header's first byte itself)
    add("header twins", [pc.blob(b"one byte")] + [pc.blob(pc.text(250 + 100 * k, 40 + k), hdr_bytes=k) for k in range(2, 11)],
        ["header twins, size varints of 2 to 10 bytes"], claim=_twins)
    for links in (1, 2, 3):
        for behind in (False, True):
            add("%d REF links, bases %s" % (links, "behind" if behind else "in front"), _ref_chain(links, behind),
                ["REF chain of %d, bases %s" % (links, "behind" if behind else "in front")],
                claim=lambda c, links=links: bm.BuildModel(c["pack"]).generations == links + 1)
    add("a thin pack", [pc.blob(pc.MID), pc.delta(None, [("copy", 0, 10)], "ref", base_name=hashlib.sha1(b"elsewhere").digest(),
                                                   base_size=len(pc.MID), result_size=10)], ["thin pack"], well=False)
    n0, n1, n2 = (hashlib.sha1(b"cycle %d" % k).digest() for k in range(3))
    cyc = dict(base_size=10, result_size=10)
    add("a REF cycle of two, built", [pc.blob(pc.MID), pc.delta(None, [("copy", 0, 10)], "ref", base_name=n1, name=n0, **cyc),
                                      pc.delta(None, [("copy", 0, 10)], "ref", base_name=n0, name=n1, **cyc)], ["REF cycle of two"], well=False)
    add("a REF cycle of three, built", [pc.delta(None, [("copy", 0, 10)], "ref", base_name=n1, name=n0, **cyc),
                                        pc.delta(None, [("copy", 0, 10)], "ref", base_name=n2, name=n1, **cyc),
                                        pc.delta(None, [("copy", 0, 10)], "ref", base_name=n0, name=n2, **cyc), pc.blob(pc.SMALL)],
        ["REF cycle of three"], well=False)
    add("the same object twice", [pc.blob(pc.MID), pc.blob(pc.SMALL), pc.blob(pc.MID)], ["same object twice"], well=False)
    add("a count one above", [pc.blob(pc.MID), pc.blob(pc.SMALL)], ["header count one above"], well=False, count=3)
    add("a count one below", [pc.blob(pc.MID), pc.blob(pc.SMALL)], ["header count one below"], well=False, count=1)
    add("garbage in front of the trailer", [pc.blob(pc.MID), pc.blob(pc.SMALL, spare=b"\x78\x9cgarbage")], ["garbage between the last object and the trailer"],
        well=False)
    sound = pw.write_pack([pc.blob(pc.MID), pc.delta(0, [("copy", 0, 10)])])[0]
    bent = sound[-20:-1] + bytes([sound[-1] ^ 1])
    add("a trailer off by one bit, checked", [pc.blob(pc.MID), pc.delta(0, [("copy", 0, 10)])], ["trailer off by one bit, with the flag"], well=False,
        trailer=bent)
    add("a trailer off by one bit, not checked", [pc.blob(pc.MID), pc.delta(0, [("copy", 0, 10)])], ["trailer off by one bit, without the flag"],
        well=False, ours=True, flags=0, trailer=bent)
    add("an empty pack, built", [], ["empty pack"])
    return out


REQUIRED_EDGES = {
    "stored blob with inner zlib streams, one ends on the object's end", "stored random blob, hundreds of false candidates",
    "candidate in the last 6 bytes and one inside the trailer", "header twins, size varints of 2 to 10 bytes",
    "REF chain of 1, bases in front", "REF chain of 1, bases behind", "REF chain of 2, bases in front", "REF chain of 2, bases behind",
    "REF chain of 3, bases in front", "REF chain of 3, bases behind", "thin pack", "REF cycle of two", "REF cycle of three", "same object twice",
    "header count one above", "header count one below", "garbage between the last object and the trailer", "trailer off by one bit, with the flag",
    "trailer off by one bit, without the flag", "empty pack", "golden pack",
}


@functools.lru_cache(maxsize=None)
def cases():
    """every case, built: computed once and shared"""
    out = []
    for c in _raw_cases():
        pack, idx, _ = pw.write_pack(c["entries"], **c["kw"])
        out.append({"name": c["name"], "pack": pack, "flags": c["flags"], "well": c["well"], "ours": c["ours"], "idx": idx if c["own_idx"] and c["well"] else None,
                    "edges": c["edges"], "claim": c["claim"]})
    with open(os.path.join(GOLDEN, "git.pack"), "rb") as f:
        pack = f.read()
    with open(os.path.join(GOLDEN, "git.idx"), "rb") as f:
        idx = f.read()
    out.append({"name": "the golden pack", "pack": pack, "flags": 1, "well": True, "ours": False, "idx": idx, "edges": {"golden pack"}, "claim": None})
    assert len({c["name"] for c in out}) == len(out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def model(name):
    """the model's reading of a case, computed once"""
    c = [c for c in cases() if c["name"] == name][0]
    return bm.BuildModel(c["pack"], bool(c["flags"] & 1))


def accepted(c):
    """the library writes an idx for it"""
    return c["well"] or c["ours"]
