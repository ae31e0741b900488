"""ctypes driver of the drop-in layer's overlapping-input constructors (wtamd_OverlappingArrayReader, wtamd_CoverageIterator)
for tests/test_cover_model.py (the emulated drop-in library) and tests/test_cover_gpu.py (the product): builds the iterators
over NumPy arrays and reads them the three ways the layer offers -- pop(), wtamd_iterator_next_block, and as children of
newMultiplexer + MeanReduction."""
import ctypes as C

import numpy as np


class WiggleIterator(C.Structure):
    _fields_ = [("chrom", C.c_char_p), ("start", C.c_int), ("finish", C.c_int), ("value", C.c_double), ("valuePtr", C.c_void_p),
                ("done", C.c_char), ("strand", C.c_int), ("data", C.c_void_p), ("pop", C.c_void_p), ("seek", C.c_void_p),
                ("overlaps", C.c_char), ("default_value", C.c_double), ("append", C.c_void_p)]


POP = C.CFUNCTYPE(None, C.c_void_p)
SEEK = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p, C.c_int, C.c_int)


class DropIn:
    def __init__(self, path):
        L = self.L = C.CDLL(path)
        reader = [C.c_int, C.POINTER(C.c_char_p), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double]
        for name in ("wtamd_OverlappingArrayReader", "wtamd_ArrayReader"):
            getattr(L, name).restype = C.c_void_p
            getattr(L, name).argtypes = reader
        L.wtamd_CoverageIterator.restype = C.c_void_p
        L.wtamd_CoverageIterator.argtypes = [C.c_void_p]
        L.pop.restype = None
        L.pop.argtypes = [C.c_void_p]
        L.seek.restype = None
        L.seek.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int]
        L.newMultiplexer.restype = C.c_void_p
        L.newMultiplexer.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_char]
        L.MeanReduction.restype = C.c_void_p
        L.MeanReduction.argtypes = [C.c_void_p]
        L.wtamd_iterator_next_block.restype = C.c_int64
        L.wtamd_iterator_next_block.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                                C.POINTER(C.c_void_p)]
        self.keep = []

    def reader(self, names, seg_off, start, finish, value, overlapping=True):
        arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
        so = np.ascontiguousarray(seg_off, np.int64)
        s, f, v = np.ascontiguousarray(start, np.int32), np.ascontiguousarray(finish, np.int32), np.ascontiguousarray(value, np.float32)
        self.keep.append((arr, so, s, f, v))            # the arrays are borrowed by the reader
        fn = self.L.wtamd_OverlappingArrayReader if overlapping else self.L.wtamd_ArrayReader
        return fn(len(names), arr, so.ctypes.data, s.ctypes.data, f.ctypes.data, v.ctypes.data, 0.0)

    def popping(self, names, seg_off, start, finish, value, overlapping=False, default=0.0):
        """A foreign iterator by the reference's protocol over the chromosomes `names`: a WiggleIterator whose pop is a
        callback, double values, stable chromosome names.  It does not seek."""
        wi = WiggleIterator()
        state = {"j": 0}
        n = len(start)
        chrom = np.repeat(np.arange(len(names)), np.diff(np.asarray(seg_off, np.int64)))
        cnames = [n_.encode() for n_ in names]

        def pop(_):
            j = state["j"]
            if j >= n:
                wi.done = b"\x01"
                return
            wi.chrom = cnames[chrom[j]]
            wi.start, wi.finish, wi.value = int(start[j]), int(finish[j]), float(value[j])
            state["j"] = j + 1

        cb, sk = POP(pop), SEEK(lambda *_: None)
        wi.done = b"\x00"
        wi.overlaps = b"\x01" if overlapping else b"\x00"
        wi.default_value = float(default)
        wi.pop, wi.seek = C.cast(cb, C.c_void_p), C.cast(sk, C.c_void_p)
        pop(None)
        self.keep.append((wi, cb, sk, cnames))
        return C.addressof(wi)

    def coverage(self, child):
        return self.L.wtamd_CoverageIterator(child)

    def fields(self, wi):
        return WiggleIterator.from_address(wi)

    def seek(self, wi, chrom, start, finish):
        self.L.seek(wi, chrom.encode(), int(start), int(finish))

    def read_pops(self, wi):
        """[(chrom, start, finish, value)] by the reference's protocol."""
        w = self.fields(wi)
        out = []
        while w.done == b"\x00":
            out.append((w.chrom.decode(), w.start, w.finish, w.value))
            self.L.pop(wi)
        return out

    def read_blocks(self, wi, pops_between=0):
        """The same through wtamd_iterator_next_block (optionally `pops_between` pop() calls after every block: the two mix)."""
        w = self.fields(wi)
        out = []
        chrom, s, f, v = C.c_char_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        while True:
            n = self.L.wtamd_iterator_next_block(wi, C.byref(chrom), C.byref(s), C.byref(f), C.byref(v))
            assert n >= 0, "wtamd_iterator_next_block refused the iterator"
            if n == 0:
                return out
            i32 = C.POINTER(C.c_int32)
            sa = np.ctypeslib.as_array(C.cast(s, i32), shape=(n,)).copy()
            fa = np.ctypeslib.as_array(C.cast(f, i32), shape=(n,)).copy()
            va = np.ctypeslib.as_array(C.cast(v, C.POINTER(C.c_double)), shape=(n,)).copy()
            out.extend((chrom.value.decode(), int(a), int(b), float(x)) for a, b, x in zip(sa, fa, va))
            for k in range(pops_between):
                self.L.pop(wi)
                if w.done != b"\x00":
                    return out
                if k < pops_between - 1:            # (the last one stays the current element: the next block starts with it)
                    out.append((w.chrom.decode(), w.start, w.finish, w.value))

    def mean_of(self, iters):
        """MeanReduction(newMultiplexer(iters)) drained through the block door."""
        arr = (C.c_void_p * len(iters))(*iters)
        self.keep.append(arr)
        return self.read_blocks(self.L.MeanReduction(self.L.newMultiplexer(arr, len(iters), b"\x00")))


def tracks_case(rng, n_tracks, n_chrom, n_max, span, max_len):
    """n_tracks overlapping tracks over the same chromosomes: [(seg_off, start, finish)] per track."""
    import cover_model as M
    out = []
    for _ in range(n_tracks):
        segs = [M.random_segment(rng, int(rng.integers(0, n_max)), span, max_len) for _ in range(n_chrom)]
        seg_off = np.concatenate([[0], np.cumsum([len(s[0]) for s in segs])]).astype(np.int64)
        out.append((seg_off, np.concatenate([s[0] for s in segs]).astype(np.int32), np.concatenate([s[1] for s in segs]).astype(np.int32)))
    return out


def expected_rows(names, seg_off, start, finish, window=None):
    """The model's depth track of one overlapping track as [(chrom, start, finish, value)]; window = (chrom, lo, hi): the
    model over the intervals of that chromosome that intersect [lo, hi), clipped."""
    import cover_model as M
    rows = []
    for c, name in enumerate(names):
        s, f = start[seg_off[c]:seg_off[c + 1]].astype(np.int64), finish[seg_off[c]:seg_off[c + 1]].astype(np.int64)
        if window is not None:
            if name != window[0]:
                continue
            keep = (f > window[1]) & (s < window[2])
            s, f = np.maximum(s[keep], window[1]), np.minimum(f[keep], window[2])
        cs, cf, cv = M.coverage(s, f)
        rows.extend((name, int(a), int(b), float(x)) for a, b, x in zip(cs, cf, cv))
    return rows


def check_dropin(D, oracle, rng):
    """The checks both backends share: one coverage iterator read by pop(), by blocks and mixed; a seek; several as children
    of a Multiplexer under MeanReduction against the oracle's `mean` over the model's depth tracks (bit-exact: integers)."""
    import cover_model as M
    from wiggletools_amd.runlists import RunLists
    names = ["chr1", "chr2", "chrX"]
    for n_max, span, max_len in ((12, 40, 10), (60, 300, 40), (700, 4000, 60)):
        tracks = tracks_case(rng, 3, len(names), n_max, span, max_len)
        for (seg_off, s, f) in tracks:
            exp = expected_rows(names, seg_off, s, f)
            v = np.ones(len(s), np.float32)
            assert D.read_pops(D.coverage(D.reader(names, seg_off, s, f, v))) == exp
            assert D.read_blocks(D.coverage(D.reader(names, seg_off, s, f, v))) == exp
            assert D.read_blocks(D.coverage(D.reader(names, seg_off, s, f, v)), pops_between=2) == exp
            # seek into a window: the model over the clipped intervals
            wi = D.coverage(D.reader(names, seg_off, s, f, v))
            for (c, lo, hi) in (("chr2", 1 + span // 4, 1 + span // 2), ("chr1", 1, 3), ("chrX", span, span + 50), ("nope", 1, 100)):
                D.seek(wi, c, lo, hi)
                assert D.read_pops(wi) == expected_rows(names, seg_off, s, f, (c, lo, hi)), (c, lo, hi)
        # Multiplexer children
        lists = []
        for (seg_off, s, f) in tracks:
            per_c = []
            for c in range(len(names)):
                cs, cf, cv = M.coverage(s[seg_off[c]:seg_off[c + 1]], f[seg_off[c]:seg_off[c + 1]])
                per_c.append(list(zip(cs.tolist(), cf.tolist(), cv.tolist())))
            lists.append(per_c)
        ec, es, ef, ev = oracle.reduce(RunLists.from_lists(lists).as_dict(), "mean")[:4]
        got = D.mean_of([D.coverage(D.reader(names, seg_off, s, f, np.ones(len(s), np.float32))) for (seg_off, s, f) in tracks])
        assert [g[0] for g in got] == [names[c] for c in ec]
        assert np.array_equal([g[1] for g in got], es) and np.array_equal([g[2] for g in got], ef)
        assert M.same_bits([g[3] for g in got], ev)
    # a child that does not overlap comes back as it is
    seg_off, s, f = np.array([0, 2], np.int64), np.array([1, 5], np.int32), np.array([3, 9], np.int32)
    child = D.reader(["chr1"], seg_off, s, f, np.ones(2, np.float32), overlapping=False)
    assert D.coverage(child) == child
    w = D.fields(D.coverage(D.reader(["chr1"], seg_off, s, f, np.ones(2, np.float32))))
    assert w.overlaps == b"\x00" and w.default_value == 0.0
