"""A writer of git packfiles (version 2) and their idx (version 2) for the tests: plain Python, no device.  It writes what
it is told, with a knob for every malformed form the cases need; names are SHA-1s from hashlib.  It shares no code with the
reader it is checked against (pack_model.py).

An entry is a dict.  Whole objects:   {"type": 1..4, "data": bytes}
Deltas:                               {"delta": "ofs" | "ref", "base": k (an entry of the list), "ins": [instruction, ..]}
Instructions:  ("copy", offset, size)            the shortest encoding (size 0x10000: no size bytes)
               ("copy", offset, size, mask)      the offset / size bytes named by the 7 bits of mask, the others must be 0
               ("insert", bytes)                 1 .. 127 bytes
               ("raw", bytes)                    these bytes as they are
Knobs of an entry (all optional):
  hsize          the size the header states (default: the length of what is deflated)
  hdr_bytes      the header's size varint padded with empty continuation bytes to this many bytes in all
  raw_type       the type bits of the header (default: the entry's)
  base_size, result_size   the delta's two varints (default: the base's length, the result's length)
  size_bytes     both varints padded to this many bytes
  cut            bytes dropped from the end of the delta's payload
  payload        the delta's whole payload as it is deflated
  ofs            the OFS_DELTA distance as written (default: to the base); ofs_adjust: added to the true distance
  base_name      the REF_DELTA's 20 bytes (default: the base's name)
  bad_adler      the zlib trailer's last byte is inverted
  spare          bytes that follow the object's zlib stream
  name           the object's name in the idx (default: computed; b"?" * 20-like stand-ins for what has no content)
  level          zlib level (default 6)
"""
import hashlib
import struct
import zlib

TYPE_NAMES = {1: b"commit", 2: b"tree", 3: b"blob", 4: b"tag"}
OFS_DELTA, REF_DELTA = 6, 7


def object_name(type_, data):
    return hashlib.sha1(TYPE_NAMES[type_] + b" " + str(len(data)).encode() + b"\0" + data).digest()


def leb128(v, nbytes=None):
    out = bytearray()
    while True:
        b = v & 0x7f
        v >>= 7
        if v or (nbytes is not None and len(out) + 1 < nbytes):
            out.append(b | 0x80)
        else:
            out.append(b)
            break
    return bytes(out)


def object_header(type_, size, nbytes=None):
    out = bytearray()
    b = (type_ & 7) << 4 | (size & 15)
    size >>= 4
    while size or (nbytes is not None and len(out) + 1 < nbytes):
        out.append(b | 0x80)
        b = size & 0x7f
        size >>= 7
    out.append(b)
    return bytes(out)


def ofs_varint(v):
    out = [v & 0x7f]
    v >>= 7
    while v:
        v -= 1
        out.append(0x80 | (v & 0x7f))
        v >>= 7
    return bytes(reversed(out))


def copy_op(offset, size, mask=None):
    """one copy instruction; mask: which of the 4 offset bytes (bits 0-3) and 3 size bytes (bits 4-6) are written"""
    assert 0 <= offset < 1 << 32 and 1 <= size <= 0x10000 + 0xffffff
    enc = 0 if size == 0x10000 else size
    assert enc < 1 << 24
    vals = [(offset >> (8 * k)) & 0xff for k in range(4)] + [(enc >> (8 * k)) & 0xff for k in range(3)]
    if mask is None:
        mask = sum(1 << k for k in range(7) if vals[k])
    assert all(vals[k] == 0 or mask >> k & 1 for k in range(7)), "a byte that is not 0 has to be written"
    return bytes([0x80 | mask]) + bytes(vals[k] for k in range(7) if mask >> k & 1)


def encode_instructions(ins):
    out = bytearray()
    for i in ins:
        if i[0] == "copy":
            out += copy_op(*i[1:])
        elif i[0] == "insert":
            assert 1 <= len(i[1]) <= 127
            out += bytes([len(i[1])]) + i[1]
        else:
            out += i[1]
    return bytes(out)


def _result(base, ins):
    """what the instructions give, or None where they cannot be followed (the writer's own small reading, for the names)"""
    out = bytearray()
    for i in ins:
        if i[0] == "copy":
            if i[1] + i[2] > len(base):
                return None
            out += base[i[1]:i[1] + i[2]]
        elif i[0] == "insert":
            out += i[1]
        else:
            return None
    return bytes(out)


def write_pack(entries, version=2, magic=b"PACK", count=None, trailer=None, idx_crc=None, idx_64bit=False, idx_pack_checksum=None):
    """-> (pack, idx, layout); layout[k]: name, offset, packed_len, type, data of entry k (type / data None where the entry has
    no content to name).  A REF_DELTA's base may lie later in the list.  idx_crc: {k: value} overrides; idx_64bit: every
    offset goes through the 64-bit table."""
    memo = {}

    def content(k):  # (type, data) of entry k, (None, None) where it has none
        if k not in memo:
            e = entries[k]
            memo[k] = (None, None)  # (a cycle ends here)
            if "delta" not in e:
                if e.get("raw_type", e["type"]) in TYPE_NAMES:
                    memo[k] = (e["type"], e["data"])
            elif e.get("base") is not None and not any(x in e for x in ("cut", "base_size", "result_size", "payload", "ofs", "ofs_adjust", "base_name")):
                t, base = content(e["base"])
                data = _result(base, e["ins"]) if base is not None else None
                if data is not None:
                    memo[k] = (t, data)
        return memo[k]

    names = []
    for k, e in enumerate(entries):
        t, data = content(k)
        names.append(e.get("name") or (object_name(t, data) if data is not None else hashlib.sha1(b"no content %d" % k).digest()))
    body = bytearray(magic + struct.pack(">II", version, len(entries) if count is None else count))
    layout = []
    for k, e in enumerate(entries):
        off = len(body)
        t, data = content(k)
        if "delta" in e:
            b = e.get("base")
            base_data = content(b)[1] if b is not None else None
            bs = e.get("base_size", len(base_data) if base_data is not None else 0)
            full = _result(base_data, e["ins"]) if base_data is not None else None
            rs = e.get("result_size", len(full) if full is not None else 0)
            payload = leb128(bs, e.get("size_bytes")) + leb128(rs, e.get("size_bytes")) + encode_instructions(e["ins"])
            if e.get("cut"):
                payload = payload[:-e["cut"]]
            payload = e.get("payload", payload)
            raw_type = OFS_DELTA if e["delta"] == "ofs" else REF_DELTA
            if raw_type == OFS_DELTA:
                link = ofs_varint(e["ofs"] if "ofs" in e else off - layout[b]["offset"] + e.get("ofs_adjust", 0))
            else:
                link = e.get("base_name") or names[b]
        else:
            payload, raw_type, link = e["data"], e["type"], b""
        hdr = object_header(e.get("raw_type", raw_type), e.get("hsize", len(payload)), e.get("hdr_bytes"))
        z = bytearray(zlib.compress(payload, e.get("level", 6)))
        if e.get("bad_adler"):
            z[-1] ^= 0xff
        body += hdr + link + z + e.get("spare", b"")
        layout.append({"name": names[k], "offset": off, "packed_len": len(body) - off, "type": t, "data": data})
    digest = hashlib.sha1(bytes(body)).digest()
    pack = bytes(body) + (digest if trailer is None else trailer)
    return pack, write_idx(pack, layout, idx_crc, idx_64bit, idx_pack_checksum), layout


def write_idx(pack, layout, idx_crc=None, idx_64bit=False, pack_checksum=None):
    order = sorted(range(len(layout)), key=lambda k: layout[k]["name"])
    fan = [0] * 256
    for k in order:
        fan[layout[k]["name"][0]] += 1
    for b in range(1, 256):
        fan[b] += fan[b - 1]
    out = bytearray(b"\xfftOc" + struct.pack(">I", 2) + struct.pack(">256I", *fan))
    for k in order:
        out += layout[k]["name"]
    for k in order:
        o = layout[k]
        crc = zlib.crc32(pack[o["offset"]:o["offset"] + o["packed_len"]])
        out += struct.pack(">I", (idx_crc or {}).get(k, crc))
    big = bytearray()
    for k in order:
        off = layout[k]["offset"]
        if idx_64bit or off >= 1 << 31:
            out += struct.pack(">I", 0x80000000 | len(big) // 8)
            big += struct.pack(">Q", off)
        else:
            out += struct.pack(">I", off)
    out += big + (pack[-20:] if pack_checksum is None else pack_checksum)
    return bytes(out) + hashlib.sha1(bytes(out)).digest()


def idx_order(layout):
    """entry k -> its index in the idx"""
    order = sorted(range(len(layout)), key=lambda k: layout[k]["name"])
    return {k: i for i, k in enumerate(order)}
