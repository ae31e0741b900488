"""What tests/test_read_dropin_host.py (the emulated drop-in library: the reference-way reader of csrc/wt_read.h) and
tests/test_read_dropin_gpu.py (the product: chunks through wtamd_text_runs_host) share: a ctypes driver of wtamd_WiggleReader and
wtamd_BedReader over temporary files -- pop for pop and through wtamd_iterator_next_block against what the compiled reference's
readers popped (tests/golden/read_fixtures.json: whole files, after seeks, over irregular lines), and in front of MeanReduction
against array readers holding the same runs."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np

import cover_dropin
import read_model as M


class DropIn(cover_dropin.DropIn):
    def __init__(self, path):
        super().__init__(path)
        for name in ("wtamd_WiggleReader", "wtamd_BedReader"):
            getattr(self.L, name).restype = C.c_void_p
            getattr(self.L, name).argtypes = [C.c_char_p]

    def open(self, path, bed):
        return (self.L.wtamd_BedReader if bed else self.L.wtamd_WiggleReader)(str(path).encode())

    def pops(self, wi, limit=None):
        """[(name bytes, start, finish, value bits)] by the reference's protocol; limit: that many pop() calls at the most."""
        w = self.fields(wi)
        out = []
        while w.done == b"\x00" and (limit is None or len(out) < limit):
            out.append((w.chrom, w.start, w.finish, struct.unpack("<Q", struct.pack("<d", w.value))[0]))
            self.L.pop(wi)
        return out

    def blocks(self, wi):
        out = []
        chrom, s, f, v = C.c_char_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        while True:
            n = self.L.wtamd_iterator_next_block(wi, C.byref(chrom), C.byref(s), C.byref(f), C.byref(v))
            assert n >= 0, "wtamd_iterator_next_block refused the iterator"
            if n == 0:
                return out
            sa = np.ctypeslib.as_array(C.cast(s, C.POINTER(C.c_int32)), shape=(n,)).copy()
            fa = np.ctypeslib.as_array(C.cast(f, C.POINTER(C.c_int32)), shape=(n,)).copy()
            va = np.ctypeslib.as_array(C.cast(v, C.POINTER(C.c_uint64)), shape=(n,)).copy()
            out.extend((chrom.value, int(a), int(b), int(x)) for a, b, x in zip(sa, fa, va))


def same_as_fixture(rows, c, what):
    got = M.as_fixture(rows)
    for k in ("n", "sha256", "records", "head", "tail"):
        assert got.get(k) == c.get(k), (what, k, got.get(k) if k != "records" else None)


def check_dropin(D, tmp, setenv, chunks=("", "300", "8")):
    """Every regular case pop for pop and block for block, at the default chunk size and at chunks of a few hundred and of a
    few bytes (cut inside sections and chromosomes); the seeks; the irregular texts the reference reads to their end."""
    fx = M.fixtures()
    cases = M.cases()
    path = os.path.join(str(tmp), "in.txt")
    for chunk in chunks:
        setenv("WTAMD_READ_CHUNK_BYTES", chunk)
        for c in fx["cases"]:
            data, flags = cases[c["name"]]
            if chunk and len(data) > 50000 and chunk != "300":
                continue
            open(path, "wb").write(data)
            bed = bool(flags & M.BED)
            wi = D.open(path, bed)
            w = D.fields(wi)
            assert (w.overlaps, w.default_value) == (b"\x01" if bed else b"\x00", 0.0)
            same_as_fixture(D.pops(wi), c, (c["name"], chunk, "pops"))
            same_as_fixture(D.blocks(D.open(path, bed)), c, (c["name"], chunk, "blocks"))
        for c in fx["seeks"]:
            data, flags = cases[c["case"]]
            open(path, "wb").write(data)
            wi = D.open(path, bool(flags & M.BED))
            D.pops(wi, c["pops"])
            D.seek(wi, c["chrom"], c["start"], c["finish"])
            same_as_fixture(D.pops(wi), c, (c["name"], chunk, "seek"))
        # irregular lines the reference reads on from (it exits on the others: run_exits)
        irr = M.irregular_cases()
        n = 0
        for c in fx["irregular"]:
            if c.get("exit_status") == 0:
                data, flags, _ = irr[c["name"]]
                open(path, "wb").write(data)
                same_as_fixture(D.pops(D.open(path, bool(flags & M.BED))), c, (c["name"], chunk, "irregular"))
                n += 1
        assert n > 30
    setenv("WTAMD_READ_CHUNK_BYTES", "")


def check_mean(D, tmp):
    """MeanReduction over three text files against the same reduction over array readers holding the files' runs."""
    cases = M.cases()
    iters, arrays = [], []
    for k, name in enumerate(("bedgraph_255", "bedgraph_256", "bedgraph_257")):
        data, flags = cases[name]
        path = os.path.join(str(tmp), "mean%d.bg" % k)
        open(path, "wb").write(data)
        iters.append(D.open(path, False))
        rows = M.reference_reading(data, flags)
        names = []
        for r in rows:
            if r[0].decode() not in names:
                names.append(r[0].decode())
        seg = [0] + [sum(1 for r in rows if names.index(r[0].decode()) <= g) for g in range(len(names))]
        vals = [M.bits_to_float(r[3]) for r in rows]
        assert np.array_equal(np.asarray(vals, np.float32).astype(np.float64), np.asarray(vals))
        arrays.append(D.reader(names, seg, [r[1] for r in rows], [r[2] for r in rows], vals, overlapping=False))
    got, want = D.mean_of(iters), D.mean_of(arrays)
    assert len(want) > 300 and got == want


EXITS = r'''
import os, sys
sys.path.insert(0, sys.argv[1])
import read_dropin as R, read_model as M
D = R.DropIn(sys.argv[2])
tmp = sys.argv[3]
path = os.path.join(tmp, "in.txt")
irr, uns = M.irregular_cases(), M.unsorted_cases()
fx = M.fixtures()
todo = [(c, irr[c["name"]][0], irr[c["name"]][1]) for c in fx["irregular"] if c.get("exit_status", 0) != 0] + [(c, uns[c["name"]][0], M.BED) for c in fx["unsorted"]]
for chunk in ("", "8"):
    os.environ["WTAMD_READ_CHUNK_BYTES"] = chunk
    for c, data, flags in todo:
        open(path, "wb").write(data)
        err = os.path.join(tmp, "err.txt")
        sys.stdout.flush()
        pid = os.fork()
        if pid == 0:
            os.dup2(os.open(err, os.O_WRONLY | os.O_CREAT | os.O_TRUNC), 2)
            rows = D.pops(D.open(path, bool(flags & M.BED)))
            os._exit(0)
        status = os.waitpid(pid, 0)[1]
        said = open(err, "rb").read().decode("latin-1").replace(path, "<path>")
        assert os.WIFEXITED(status) and os.WEXITSTATUS(status) == c["exit_status"], (c["name"], chunk, status, said)
        assert said == c["stderr"], (c["name"], chunk, said, c["stderr"])
print("read-exits-ok %d" % len(todo))
'''


def run_exits(lib_path, tmp):
    """The texts the reference gives up on, each in a forked child of a fresh process (which never opens a GPU): the same
    exit status and the same words on stderr."""
    r = subprocess.run([sys.executable, "-c", EXITS, M.HERE, lib_path, str(tmp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "read-exits-ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
