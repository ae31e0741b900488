#!/usr/bin/env python
"""Generates tests/golden/mtext_fixtures.json: what the compiled reference's TeeMultiplexer and PasteMultiplexer
(src/mWigWriter.c:286-327; `mwrite`, `mwrite_bg`, `apply_paste`) print for every case of tests/mtext_model.py's
reference_cases(), in wig, bedGraph and paste mode.

The driver is our own: an array-backed Multiplexer (newCoreMultiplexer with a pop that serves one row of a tile per call) and
functions that run a TeeMultiplexer or a PasteMultiplexer over it into an open_memstream and copy the text out.  It is
compiled together with the reference's sources, unmodified and from where they lie, into a shared object in a temporary
directory.  Nothing compiled is kept.

The generator asserts for EVERY case, none left out, that the reference's text equals the model's byte for byte.  The tiles
themselves are not stored: cases() builds them, and a digest of the input is recorded beside the output.  Cases of up to 200
entries and 4 columns record the whole text; larger ones its SHA-256, its length and the 20 lines on either side of every
block seam.  The paste cases read infiles with a `track` and a `browser` line to skip, \\r\\n endings and a line of more than
4999 bytes (consumed in pieces, one per entry); the infile one line short runs in a forked child: its exit status, its stderr
and what it had written are recorded as data.

Run where the reference's sources are present:  python tests/golden/make_mtext_golden.py <path to the reference>
"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mtext_model as M  # noqa: E402
from make_coverage_golden import REF_SRCS  # noqa: E402

DRIVER = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "wiggletools.h"
#include "wiggleIterator.h"
#include "multiplexer.h"

typedef struct {
    int n_chrom, width, c;
    char **names;
    long long *seg_off, j;
    int *start, *finish;
    double *vals;
} MArr;

static void marr_pop(Multiplexer *m) {
    MArr *a = (MArr *) m->data;
    while (a->c < a->n_chrom && a->j >= a->seg_off[a->c + 1]) a->c++;
    if (a->c >= a->n_chrom) { m->done = true; return; }
    m->chrom = a->names[a->c];
    m->start = a->start[a->j];
    m->finish = a->finish[a->j];
    memcpy(m->values, a->vals + a->j * a->width, sizeof(double) * a->width);
    a->j++;
}

static void marr_seek(Multiplexer *m, const char *chrom, int start, int finish) { }

static Multiplexer *marr_new(int n_chrom, char **names, long long *seg_off, int *start, int *finish, double *vals, int width) {
    MArr *a = (MArr *) calloc(1, sizeof(MArr));
    a->n_chrom = n_chrom; a->names = names; a->seg_off = seg_off; a->start = start; a->finish = finish; a->vals = vals; a->width = width;
    Multiplexer *m = newCoreMultiplexer(a, width, &marr_pop, &marr_seek);
    popMultiplexer(m);
    return m;
}

/* infile NULL: TeeMultiplexer; outpath NULL: into a memory stream.  Returns the text's length (above cap: too small). */
long long golden_mtext(int n_chrom, char **names, long long *seg_off, int *start, int *finish, double *vals, int width, int bedGraph,
                       const char *inpath, const char *outpath, long long cap, char *out) {
    char *buf = NULL;
    size_t len = 0;
    FILE *fp = outpath ? fopen(outpath, "w") : open_memstream(&buf, &len);
    FILE *in = inpath ? fopen(inpath, "r") : NULL;
    Multiplexer *m = marr_new(n_chrom, names, seg_off, start, finish, vals, width);
    runMultiplexer(in ? PasteMultiplexer(m, in, fp, false) : TeeMultiplexer(m, fp, bedGraph, false));
    fclose(fp);
    if (in) fclose(in);
    if (outpath) return 0;
    if ((long long) len <= cap) memcpy(out, buf, len);
    free(buf);
    return (long long) len;
}
'''


def build(ref, tmp):
    drv = os.path.join(tmp, "driver.c")
    open(drv, "w").write(DRIVER)
    so = os.path.join(tmp, "libmtextgold.so")
    subprocess.check_call(["gcc", "-g", "-w", "-O3", "-std=gnu99", "-D_GNU_SOURCE", "-fPIC", "-shared", "-I" + os.path.join(ref, "src")] +
                          [os.path.join(ref, "src", s) for s in REF_SRCS] + [drv, "-o", so, "-lm", "-lpthread"])
    return C.CDLL(so, mode=os.RTLD_LAZY)


def run(lib, T, bedgraph, inpath=None, outpath=None):
    cap = 1 << 25
    out = C.create_string_buffer(cap)
    L = T.L
    names = (C.c_char_p * len(L.names))(*L.names)
    seg = L.seg.astype("int64")
    p = lambda x: C.c_void_p(x.ctypes.data)      # noqa: E731
    lib.golden_mtext.restype = C.c_longlong
    n = lib.golden_mtext(C.c_int(len(L.names)), names, p(seg), p(L.s), p(L.f), p(T.vals), C.c_int(T.width), C.c_int(bedgraph),
                         inpath.encode() if inpath else None, outpath.encode() if outpath else None, C.c_longlong(cap), out)
    assert 0 <= n <= cap, n
    return out.raw[:n]


def infile_of(T, path, short=0):
    """The tile's prefixes as the lines of an infile, with what the reference skips or strips: a browser line, track lines,
    \\r\\n endings.  A prefix of 0 bytes is an empty line: fgets gives "\\n", which is not skipped and strips to nothing."""
    pre = T.prefixes[:len(T.prefixes) - short]
    with open(path, "wb") as fh:
        fh.write(b"browser position chr1:1-1000\ntrack name=golden\n")
        for i, ln in enumerate(pre):
            fh.write(ln + (b"\r\n" if i % 3 == 1 else b"\n"))
            if i == 10:
                fh.write(b"track type=bedGraph\n")


def long_line_case():
    """A line of 12000 bytes, consumed as three prefixes of 4999, 4999 and 2002 bytes; then ordinary lines."""
    T = M.cases()["paste_w3"].part(6, 50)               # (prefixes of up to 40 bytes)
    line = bytes(48 + i % 10 for i in range(12000))
    return M.Tile(T.L, T.vals, [line[:4999], line[4999:9998], line[9998:]] + T.prefixes[3:]), line


def record(name, mode, T, flags, txt):
    c = {"name": "%s/%s" % (name, mode), "case": name, "mode": mode, "flags": flags, "entries": len(T), "width": T.width, "input_sha256": T.digest(),
         "bytes": len(txt), "sha256": hashlib.sha256(txt).hexdigest()}
    if len(T) <= 200 and T.width <= 4 and len(txt) < 20000:
        c["text"] = txt.decode("latin-1")
    else:
        c["seams"] = M.seam_lines(txt, T, flags)
    return c


def main():
    ref = sys.argv[1]
    out = {"generator": "tests/golden/make_mtext_golden.py",
           "source": "compiled reference v1.2.11: TeeMultiplexer / PasteMultiplexer over an array-backed Multiplexer into a memory stream",
           "cases": []}
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(ref, tmp)
        infile = os.path.join(tmp, "in.txt")
        for name, T in M.reference_cases().items():
            assert len(set(T.L.names)) == len(T.L.names), name          # (the reference compares names, the door segments)
            if T.prefixes is not None:
                infile_of(T, infile)
                txt = run(lib, T, 1, infile)
                assert txt == M.text(T, 0)[0], (name, "paste")
                out["cases"].append(record(name, "paste", T, 0, txt))
                continue
            for mode, flags in (("wig", 0), ("bedGraph", M.BEDGRAPH)):
                txt = run(lib, T, flags)
                model = M.text(T, flags)[0]
                assert txt == model, (name, mode, len(txt), len(model)) + M.first_difference(txt, model)
                out["cases"].append(record(name, mode, T, flags, txt))
        # a line of 4999 bytes and more
        T, line = long_line_case()
        with open(infile, "wb") as fh:
            fh.write(line + b"\n" + b"".join(p + b"\n" for p in T.prefixes[3:]))
        txt = run(lib, T, 1, infile)
        assert txt == M.text(T, 0)[0]
        out["cases"].append(record("long_line", "paste", T, 0, txt))
        # an infile one line short: the reference's writer thread calls exit(1); in a forked child, its stderr in a file
        T = M.cases()["paste_w3"].part(6, 50)
        infile_of(T, infile, short=1)
        outpath, errpath = os.path.join(tmp, "short.txt"), os.path.join(tmp, "short.err")
        sys.stdout.flush()
        pid = os.fork()
        if pid == 0:
            os.dup2(os.open(errpath, os.O_WRONLY | os.O_CREAT | os.O_TRUNC), 2)
            run(lib, T, 1, infile, outpath)
            os._exit(0)
        status = os.waitpid(pid, 0)[1]
        written = open(outpath, "rb").read()
        assert os.WIFEXITED(status) and os.WEXITSTATUS(status) == 1
        assert written == M.text(T.part(0, len(T) - 1), 0)[0]
        out["short_infile"] = {"exit_status": os.WEXITSTATUS(status), "stderr": open(errpath).read(), "entries": len(T), "written_entries": len(T) - 1,
                               "written_sha256": hashlib.sha256(written).hexdigest()}
    path = os.path.join(HERE, "mtext_fixtures.json")
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
    size = os.path.getsize(path)
    print("wrote %d texts, every one equal to the model byte for byte, %d bytes" % (len(out["cases"]), size))
    assert size < 250000, size


if __name__ == "__main__":
    main()
