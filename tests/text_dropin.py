"""What tests/test_text_dropin_host.py (the emulated drop-in library: the host sweep) and tests/test_text_dropin_gpu.py (the
product) share: a ctypes driver of wtamd_TeeWiggleIterator and wtamd_toFile over wtamd_ArrayReader /
wtamd_OverlappingArrayReader children (the bulk path, float32 values) and over a popping child (the reference's protocol,
double values) -- the file against the text of tests/text_model.py, which tests/golden/make_text_golden.py holds byte for byte
to the compiled reference's TeeWiggleIterator, and the runs passed on against the compressed list."""
import ctypes as C
import os

import numpy as np

import energy_dropin
import text_model as M


class DropIn(energy_dropin.DropIn):
    def __init__(self, path):
        super().__init__(path)
        L = self.L
        L.wtamd_TeeWiggleIterator.restype = C.c_void_p
        L.wtamd_TeeWiggleIterator.argtypes = [C.c_void_p, C.c_void_p, C.c_char, C.c_char]
        L.wtamd_toFile.restype = None
        L.wtamd_toFile.argtypes = [C.c_void_p, C.c_char_p, C.c_char, C.c_char]
        self.libc = C.CDLL(None)
        self.libc.fopen.restype = C.c_void_p
        self.libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
        self.libc.fclose.argtypes = [C.c_void_p]

    def child(self, L, overlapping=False, popping=None):
        names = [n.decode() for n in L.names]
        if popping is None:
            popping = not f32_exact(L)
        return self.popping_child(names, L, overlapping) if popping else self.bulk_child(names, L, overlapping)

    def tee(self, child, path, bed, hold=False):
        fp = self.libc.fopen(str(path).encode(), b"w")
        assert fp
        return self.L.wtamd_TeeWiggleIterator(child, fp, b"\x01" if bed else b"\x00", b"\x01" if hold else b"\x00"), fp

    def written(self, fp, path):
        self.libc.fclose(fp)
        return open(path, "rb").read()

    def write(self, child, path, bed, how):
        """(the runs passed on, the file): read by pop(), by blocks, or run by wtamd_toFile (which passes nothing on)."""
        if how == "tofile":
            self.L.wtamd_toFile(child, str(path).encode(), b"\x01" if bed else b"\x00", b"\x00")
            return None, open(path, "rb").read()
        wi, fp = self.tee(child, path, bed)
        rows = self.read_pops(wi) if how == "pops" else self.read_blocks(wi)
        return rows, self.written(fp, path)


def f32_exact(L):
    with np.errstate(over="ignore"):
        return np.array_equal(L.v.astype(np.float32).astype(np.float64).view(np.uint64), L.v.view(np.uint64))


def rows_of(L):
    return [(L.names[L.seg_of(i)].decode(), int(L.s[i]), int(L.f[i]), float(L.v[i])) for i in range(len(L))]


def same_rows(a, b):
    return len(a) == len(b) and all(x[:3] == y[:3] and (x[3] == y[3] or (x[3] != x[3] and y[3] != y[3])) for x, y in zip(a, b))


def lists_of(rows, names):
    seg = [0]
    for n in names:
        seg.append(seg[-1] + sum(1 for r in rows if r[0] == n.decode()))
    return M.Lists(names, seg, [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows])


def window_of(D, L):
    """A window inside the second chromosome and what a plain reader serves after a seek to it: (name, lo, hi, Lists)."""
    name = L.names[1].decode()
    lo, hi = int(L.s[L.seg[1] + 3]) + 1, int(L.f[L.seg[1] + 40]) - 1
    plain = D.child(L)
    D.seek(plain, name, lo, hi)
    window = lists_of(D.read_pops(plain), L.names)
    assert 30 < len(window) < 50
    return name, lo, hi, window


def check_dropin(D, tmp, setenv=None):
    """The checks both backends share.  setenv(name, value): given by the product's test, which writes every case with the
    device door and again with WTAMD_NO_DEVICE_TEXT=1."""
    path = os.path.join(str(tmp), "out.txt")
    cases = M.reference_cases()
    lists = [(n, cases[n]) for n in ("chrom_change", "transitions_adjacent", "transitions_gaps", "random_257", "random_10001", "straddle_10000",
                                     "points_across_10000", "names", "values", "values_points", "wide_0", "wide_1")]
    lists.append(("mergeable", M.mergeable_list()))
    seen = {"bulk": 0, "pops": 0, "merged": 0, "wide": 0}
    for no_device in (("0", "1") if setenv else ("0",)):
        if setenv:
            setenv("WTAMD_NO_DEVICE_TEXT", no_device)
        for name, L in lists:
            for bed in (False, True):
                want_l = L if bed else M.compress(L)
                want = M.text(want_l, M.BEDGRAPH if bed else 0)[0]
                for popping in (None, True):
                    for how in ("pops", "blocks", "tofile"):
                        if (popping and how != "pops") or (len(L) > 5000 and how == "pops" and popping is None):
                            continue                                # (pop by pop from Python: the short lists, and the popping child)
                        rows, txt = D.write(D.child(L, popping=popping), path, bed, how)
                        assert txt == want, (name, bed, popping, how, no_device, len(txt), len(want))
                        assert rows is None or same_rows(rows, rows_of(want_l)), (name, bed, how)
                f32 = f32_exact(L)
                seen["bulk" if f32 else "pops"] += 1
                seen["merged"] += int(len(want_l) < len(L))
                seen["wide"] += int(any(M.is_wide(float(x)) for x in L.v))
        # an overlapping child is forced to bedGraph and is not compressed
        L = M.mergeable_list()
        wi, fp = D.tee(D.child(L, overlapping=True), path, False)
        w = D.fields(wi)
        assert w.overlaps == b"\x01"
        rows = D.read_pops(wi)
        assert D.written(fp, path) == M.text(L, M.BEDGRAPH)[0] and same_rows(rows, rows_of(L))
        # holdFire: nothing is written before the first seek; the runs are passed on all the same
        L = cases["random_257"]
        wi, fp = D.tee(D.child(L), path, False, hold=True)
        assert same_rows(D.read_pops(wi), rows_of(L)) and D.written(fp, path) == b""
        name, lo, hi, window = window_of(D, L)
        wi, fp = D.tee(D.child(L), path, False, hold=True)
        D.seek(wi, name, lo, hi)
        rows = D.read_pops(wi)
        assert D.written(fp, path) == M.text(M.compress(window), 0)[0] and same_rows(rows, rows_of(M.compress(window)))
        # SEEK, against the model only: the reference kills its writer thread and loses whatever that thread had not yet printed
        # -- a race with no defined result; the library's rule: the complete blocks of 10000 entries of what
        # was handed on are written, the open block is dropped, the entry count restarts at 0
        L = cases["random_20001"]
        name, lo, hi, window = window_of(D, L)
        for pops, whole in ((5, 0), (9998, 0), (9999, M.BLOCK), (10499, M.BLOCK)):
            for bed in (False, True):
                flags = M.BEDGRAPH if bed else 0
                wi, fp = D.tee(D.child(L), path, bed)
                for _ in range(pops):
                    D.L.pop(wi)                                     # handed on: `pops` runs and the current element
                D.seek(wi, name, lo, hi)
                D.read_pops(wi)
                assert D.written(fp, path) == M.text(L.part(0, whole), flags)[0] + M.text(M.compress(window) if not bed else window, flags)[0], (pops, bed)
    assert min(seen.values()) >= 1, seen
