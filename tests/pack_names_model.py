"""What md_pack_read / md_pack_verify say with MD_PACK_VERIFY_NAME, stated over the reader of tests/pack_model.py and
hashlib alone.  The rules of include/mdeflate.h, per object and in this order:

  1. a status of its own - from md_pack_open, its zlib stream, its CRC-32 with MD_PACK_VERIFY_CRC, its delta instructions -
     stays what it is without names;
  2. else a failed object anywhere on its chain of bases, failed by name included, is MD_INVALID_PACK_BASE;
  3. else a name other than SHA-1("<type> <size>\\0" + content), the type its root's, is MD_INVALID_CHECKSUM."""
import hashlib

from tests import pack_model as pm

TYPE_NAMES = {1: b"commit", 2: b"tree", 3: b"blob", 4: b"tag"}


def object_name(type_, data):
    return hashlib.sha1(TYPE_NAMES[type_] + b" %d\0" % len(data) + data).digest()


def read(model, select=None, verify_crc=False):
    """-> [(status, bytes)] for the objects `select` (idx order; None: all) of a pm.Model, names verified"""
    plain, named = {}, {}

    def one(i):
        if i not in named:
            o = model.objects[i]
            st, data = (o["status"], b"") if o["status"] != pm.OK else model._decode(i, verify_crc, plain)
            if st == pm.OK and o["link"] and one(o["base"])[0] != pm.OK:
                st = pm.INVALID_PACK_BASE
            if st == pm.OK and object_name(o["type"], data) != o["name"]:
                st = pm.INVALID_CHECKSUM
            named[i] = (st, data if st == pm.OK else b"")
        return named[i]

    return [one(i) for i in (range(len(model.objects)) if select is None else select)]
