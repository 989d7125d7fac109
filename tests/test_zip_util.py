"""The hand-built archives of zip_util.py are good ZIP files by Python's zipfile: they open, every member's CRC holds
(testzip) and the contents are the files that went in.  The one archive zipfile misreads - an end record's signature inside
the comment - is checked against its own construction."""
import io
import zipfile

from tests import zip_util as zu


def _read(blob):
    with zipfile.ZipFile(io.BytesIO(blob)) as z:
        assert z.testzip() is None
        return [(i.filename.encode("utf-8"), z.read(i)) for i in z.infolist()]


def test_every_form_is_a_good_archive():
    labels = []
    for label, blob, want in zu.forms():
        assert _read(blob) == want, label
        labels.append(label)
    assert len(labels) == len(set(labels)) >= 20
    for s in ("descriptor_sig", "descriptor_nosig", "extras_differ", "zip64_dir", "zip64_end", "prefix", "comment", "everything+prefix"):
        assert s in labels


def test_forms_hold_what_they_claim():
    forms = {label: blob for label, blob, _ in zu.forms()}
    assert zu.SIG_DESC in forms["descriptor_sig"] and zu.SIG_DESC not in forms["descriptor_nosig"]
    assert zu.SIG_END64 in forms["zip64_end"] and zu.SIG_LOC64 in forms["zip64_end"] and zu.SIG_END64 not in forms["deflated"]
    assert forms["prefix"].startswith(b"#!/bin/sh") and forms["prefix"].endswith(forms["deflated"])
    with zipfile.ZipFile(io.BytesIO(forms["zip64_dir"])) as z:
        raw = forms["zip64_dir"]
        at = raw.index(zu.SIG_CENTRAL)
        assert raw[at + 20:at + 28] == b"\xff" * 8 and raw[at + 42:at + 46] == b"\xff" * 4  # the fixed fields say nothing
        assert z.infolist()[0].file_size == 30000
    with zipfile.ZipFile(io.BytesIO(forms["comment"])) as z:
        assert z.comment == b"an archive comment"


def test_zipfile_written_helper():
    files = zu.sample_files(3)
    for method, level in ((zipfile.ZIP_STORED, None), (zipfile.ZIP_DEFLATED, 1), (zipfile.ZIP_DEFLATED, 9)):
        assert _read(zu.zipfile_bytes(files, method, level)) == [(n.encode("utf-8"), d) for n, d in files]


def test_fake_end_record_by_construction():
    blob, want = zu.fake_end_archive()
    assert blob.endswith(zu.FAKE_END_COMMENT) and blob.count(zu.SIG_END) == 2
    real = blob.index(zu.SIG_END)
    # the real record: its comment length makes it end with the file; the fake one would end two bytes early
    assert real + 22 + int.from_bytes(blob[real + 20:real + 22], "little") == len(blob)
    fake = blob.rindex(zu.SIG_END)
    assert fake + 22 + int.from_bytes(blob[fake + 20:fake + 22], "little") == len(blob) - 2
    # without the comment it is the same archive, and that one zipfile reads
    plain = blob[:real + 20] + b"\0\0"
    assert _read(plain) == want
    with zipfile.ZipFile(io.BytesIO(blob)) as z:  # (3.10 takes the last signature: an empty archive)
        assert z.namelist() in ([], [n.decode("utf-8") for n, _ in want])
