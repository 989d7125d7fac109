"""`decompress` — the reference's command line tool (bin/decompress.ml:226-344) over the GPU engine.

    python -m decompress_amd.cli [-d] [-f deflate|zlib|gzip|lzo] [-l <level>] [--span <KiB> [--prime]] [<input> [<output>]]

Same flags, defaults and drivers as the reference: inflate unless `-d`; format `deflate` unless `-f`; level 4
unless `-l`; stdin / stdout unless file names are given.  `-d` on raw DEFLATE is the CLI's own driver
(`run_deflate`, bin/decompress.ml:47-75: a Dynamic block per queue flush, then a Fixed last block that holds only
the end-of-block code — MD_DRIVER_CLI), zlib and gzip go through `Zl.Def` / `Gz.Def` (gzip: mtime = now, OS Unix,
bin/decompress.ml:136-155), LZO through `Lzo.compress` / `Lzo.uncompress_with_buffer`.  A malformed input prints
`decompress: <the reference's message>.` and exits with cmdliner's error status (124).

`--span <KiB>` is this tool's own: with `-d` and `-f deflate|zlib|gzip` the stream is written as joined spans of that
many KiB by the whole chip (md_deflate_spans_host; same drivers and header); without `-d`, or with `-f lzo`, it
is an error.  `--prime` goes with `--span` alone: every span's matcher starts from the 32 KiB of text in front of it
(md_set_option "deflate_span_prime"), and the stream is nearly as short as the single one.  Without `--span` the bytes are
the reference's."""
import sys
import time

FORMATS = ("deflate", "zlib", "gzip", "lzo")
CLI_ERROR = 124  # Cmdliner.Cmd.Exit.cli_error: what `Error (false, msg)` becomes (bin/decompress.ml:37, :344)
QUEUE = 4096     # bin/decompress.ml:5


def parse(argv):
    """-> (deflate, format, level, input, output); raises ValueError with the reference's messages"""
    deflate, fmt, level, pos = False, "deflate", 4, []
    i = 0
    while i < len(argv):
        a = argv[i]
        if a == "-d":
            deflate = True
        elif a in ("-f", "--format") or a.startswith("-f") or a.startswith("--format="):
            if a in ("-f", "--format"):
                i += 1
                if i >= len(argv):
                    raise ValueError("option '-f' needs an argument")
                v = argv[i]
            else:
                v = a[len("--format="):] if a.startswith("--format=") else a[2:]
            if v.lower() not in FORMATS:
                raise ValueError('Invalid format: "%s"' % v)  # bin/decompress.ml:276
            fmt = v.lower()
        elif a in ("-l", "--level") or a.startswith("-l") or a.startswith("--level="):
            if a in ("-l", "--level"):
                i += 1
                if i >= len(argv):
                    raise ValueError("option '-l' needs an argument")
                v = argv[i]
            else:
                v = a[len("--level="):] if a.startswith("--level=") else a[2:]
            try:
                level = int(v)
            except ValueError:
                raise ValueError("Invalid level")  # bin/decompress.ml:293
            if level < 0:
                raise ValueError("The compression level must be positive")  # :292
        elif a.startswith("-") and a != "-":
            raise ValueError("unknown option '%s'" % a)
        else:
            pos.append(a)
        i += 1
    if len(pos) > 2:
        raise ValueError("too many arguments")
    return deflate, fmt, level, (pos[0] if pos else None), (pos[1] if len(pos) > 1 else None)


def take_span(argv):
    """`--span <KiB>` / `--span=<KiB>` out of argv -> (the other arguments, span in bytes or None)"""
    rest, span, i = [], None, 0
    while i < len(argv):
        a = argv[i]
        if a == "--span" or a.startswith("--span="):
            if a == "--span":
                i += 1
                if i >= len(argv):
                    raise ValueError("option '--span' needs an argument")
                v = argv[i]
            else:
                v = a[len("--span="):]
            if not v.isdigit() or int(v) < 1:
                raise ValueError("Invalid span")
            span = int(v) << 10
        else:
            rest.append(a)
        i += 1
    return rest, span


def run(deflate, fmt, level, data, now=None, span=None, prime=False):
    """one run of the tool on `data` -> (exit status, output bytes, message for stderr)"""
    import decompress_amd
    from decompress_amd import de, engine, gz, lzo
    eng = engine.default_engine(0)
    if deflate:
        if fmt == "lzo":
            return 0, lzo.compress(data), None
        if span is not None:  # the same drivers and header as below, the stream in joined spans
            f = {"deflate": decompress_amd.FORMAT_DEFLATE, "zlib": decompress_amd.FORMAT_ZLIB, "gzip": decompress_amd.FORMAT_GZIP}[fmt]
            hdr = None
            if fmt == "gzip":
                mtime = int(time.time() if now is None else now) & 0xffffffff
                hdr = dict(mtime=mtime, os=gz.OS["Unix"], hcrc=0, ascii=0, filename=None, comment=None)
            st, out, _ = eng.deflate_spans(data, f, span=span, level=level, queue=QUEUE,
                                           driver=engine.DRIVER_CLI if fmt == "deflate" else engine.DRIVER_ZL, header=hdr,
                                           prime=bool(prime))
            if st != 0:
                return CLI_ERROR, b"", engine.STATUS_NAMES[st]
            return 0, out, None
        if fmt == "deflate":
            st, out, _ = eng.deflate_one(data, decompress_amd.FORMAT_DEFLATE, level=level, queue=QUEUE,
                                         driver=engine.DRIVER_CLI)
        elif fmt == "zlib":
            st, out, _ = eng.deflate_one(data, decompress_amd.FORMAT_ZLIB, level=level, queue=QUEUE,
                                         driver=engine.DRIVER_ZL)
        else:
            mtime = int(time.time() if now is None else now) & 0xffffffff
            hdr = dict(mtime=mtime, os=gz.OS["Unix"], hcrc=0, ascii=0, filename=None, comment=None)
            st, out, _ = eng.deflate_one(data, decompress_amd.FORMAT_GZIP, level=level, queue=QUEUE, header=hdr)
        if st != 0:  # cannot happen with the room deflate_one gives a stream
            return CLI_ERROR, b"", engine.STATUS_NAMES[st]
        return 0, out, None
    if fmt == "lzo":
        cap = max(1 << 16, 8 * len(data))
        while True:  # Lzo.uncompress_with_buffer grows its buffer as it goes; here the capacity is retried
            verdict, out = lzo.uncompress(data, cap)
            if verdict == "Ok":
                return 0, out, None
            if cap >= (1 << 30) or "not large enough" not in eng.lib.md_status_string(engine.STATUS_CODES[out]).decode():
                return CLI_ERROR, b"", eng.lib.md_status_string(engine.STATUS_CODES[out]).decode() + "."
            cap *= 4
    f = {"deflate": decompress_amd.FORMAT_DEFLATE, "zlib": decompress_amd.FORMAT_ZLIB, "gzip": decompress_amd.FORMAT_GZIP}[fmt]
    verdict, out, _ = de.Inf.decode_chunks([data], o_len=1 << 16, fmt=f)  # De.io_buffer_size, the tool's `o`
    if verdict == "Ok":
        return 0, out, None
    msg = eng.lib.md_status_string(engine.STATUS_CODES[verdict]).decode()
    return CLI_ERROR, out, msg + "."  # `Malformed err -> `Error (false, str "%s." err)`; what was flushed stays written


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    try:
        prime = "--prime" in argv
        argv, span = take_span([a for a in argv if a != "--prime"])
        deflate, fmt, level, fin, fout = parse(argv)
        if span is not None and (not deflate or fmt == "lzo"):
            raise ValueError("option '--span' needs '-d' and a format of deflate, zlib or gzip")
        if prime and span is None:
            raise ValueError("option '--prime' needs '--span'")
    except ValueError as e:
        sys.stderr.write("decompress: %s\n" % e)
        return CLI_ERROR
    data = open(fin, "rb").read() if fin else sys.stdin.buffer.read()
    status, out, msg = run(deflate, fmt, level, data, span=span, prime=prime)
    oc = open(fout, "wb") if fout else sys.stdout.buffer
    oc.write(out)
    oc.flush()
    if fout:
        oc.close()
    if msg:
        sys.stderr.write("decompress: %s\n" % msg)
    return status


if __name__ == "__main__":
    sys.exit(main())
