"""What tests/test_hist_dropin_host.py (the emulated drop-in library: the host sweep) and tests/test_hist_gpu.py (the product)
share: a ctypes driver of wtamd_histogram, wtamd_normalize_histogram and wtamd_print_histogram over wtamd_ArrayReader children
(the bulk path, float32 values) and over a popping child (cover_dropin.DropIn.popping: the reference's protocol, double
values) -- against the recorded fixtures and the model."""
import ctypes as C

import numpy as np

import cover_dropin
import hist_model as M


class DropIn(cover_dropin.DropIn):
    def __init__(self, path):
        super().__init__(path)
        L = self.L
        L.wtamd_histogram.restype = C.c_void_p
        L.wtamd_histogram.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int]
        L.wtamd_histogram_row.restype = C.POINTER(C.c_double)
        L.wtamd_histogram_row.argtypes = [C.c_void_p, C.c_int]
        for name in ("wtamd_normalize_histogram", "wtamd_destroy_histogram"):
            getattr(L, name).restype = None
            getattr(L, name).argtypes = [C.c_void_p]
        L.wtamd_print_histogram.restype = None
        L.wtamd_print_histogram.argtypes = [C.c_void_p, C.c_void_p]
        L.wtamd_histogram_range.restype = None
        L.wtamd_histogram_range.argtypes = [C.c_void_p, C.c_void_p]
        L.wtamd_histogram_width.argtypes = L.wtamd_histogram_count.argtypes = [C.c_void_p]
        self.libc = C.CDLL(None)
        self.libc.tmpfile.restype = C.c_void_p
        self.libc.fclose.argtypes = self.libc.rewind.argtypes = self.libc.fflush.argtypes = [C.c_void_p]
        self.libc.fread.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
        self.libc.fread.restype = C.c_size_t

    def bulk_child(self, s, f, v):
        """wtamd_ArrayReader over one chromosome: a bulk source, float32 values."""
        names = (C.c_char_p * 1)(b"chr1")
        so = np.array([0, len(s)], np.int64)
        s, f, v = np.ascontiguousarray(s, np.int32), np.ascontiguousarray(f, np.int32), np.ascontiguousarray(v, np.float32)
        self.keep.append((names, so, s, f, v))
        return self.L.wtamd_ArrayReader(1, names, so.ctypes.data, s.ctypes.data, f.ctypes.data, v.ctypes.data, 0.0)

    def popping_child(self, s, f, v):
        """A foreign iterator by the reference's protocol: a WiggleIterator whose pop is a callback, double values."""
        return self.popping(["chr1"], [0, len(s)], s, f, v)

    def printed(self, h):
        fp = self.libc.tmpfile()
        self.L.wtamd_print_histogram(h, fp)
        self.libc.fflush(fp)
        self.libc.rewind(fp)
        buf = C.create_string_buffer(1 << 16)
        n = self.libc.fread(buf, 1, len(buf), fp)
        self.libc.fclose(fp)
        assert n < len(buf)
        return buf.raw[:n].decode()

    def histogram(self, kids, width):
        """(range, matrix, text, normalized text)."""
        arr = (C.c_void_p * len(kids))(*kids)
        h = self.L.wtamd_histogram(arr, len(kids), int(width))
        assert self.L.wtamd_histogram_width(h) == width and self.L.wtamd_histogram_count(h) == len(kids)
        r2 = np.zeros(2)
        self.L.wtamd_histogram_range(h, r2.ctypes.data)
        m = np.array([np.ctypeslib.as_array(self.L.wtamd_histogram_row(h, r), shape=(width,)).copy() for r in range(len(kids))])
        txt = self.printed(h)
        self.L.wtamd_normalize_histogram(h)
        ntxt = self.printed(h)
        self.L.wtamd_destroy_histogram(h)
        return r2, m, txt, ntxt


def check_dropin(D, fixtures, setenv=None):
    """The checks both backends share.  setenv(name, value): given by the product's test, which then reads every case again with
    WTAMD_NO_DEVICE_HIST=1 and expects the device's bits."""
    seen = {"bulk recorded": 0, "bulk rounded": 0}
    for c in fixtures:
        L, w = M.fixture_lists(c)
        rows = L.rows()
        rng, rec = M.fixture_result(c)
        # pop by pop, double values: the recording
        for no_device in (("0", "1") if setenv else ("0",)):
            if setenv:
                setenv("WTAMD_NO_DEVICE_HIST", no_device)
            r2, m, txt, ntxt = D.histogram([D.popping_child(*r) for r in rows], w)
            assert M.same_bits(r2, rng) and M.same_bits(m, rec), (c["name"], "pops", no_device)
            assert txt == c["text"] and ntxt == c["normalized_text"], (c["name"], "pops", no_device)
            # in blocks, float32 values: the recording where the values are exact in float32, else the model over what the reader holds
            L32 = M.Lists(L.seg, L.row, L.n_rows, L.s, L.f, L.v.astype(np.float32).astype(np.float64))
            exact = np.array_equal(L32.v, L.v, equal_nan=True)
            (lo, hi), model = M.histogram(L32, w)
            r2, m, txt, ntxt = D.histogram([D.bulk_child(*r) for r in rows], w)
            assert M.same_bits(r2, [lo, hi]) and M.same_bits(m, model), (c["name"], "blocks", no_device)
            assert txt == M.text((lo, hi), model) and ntxt == M.text((lo, hi), M.normalize(model)), (c["name"], "blocks", no_device)
            if exact:
                assert txt == c["text"] and ntxt == c["normalized_text"], (c["name"], "blocks", no_device)
            seen["bulk recorded" if exact else "bulk rounded"] += 1
        # a bulk child and a popping child side by side
        if len(rows) > 1:
            kids = [D.bulk_child(*rows[0])] + [D.popping_child(r[0], r[1], r[2].astype(np.float32).astype(np.float64)) for r in rows[1:]]
            r2, m, _, _ = D.histogram(kids, w)
            assert M.same_bits(r2, [lo, hi]) and M.same_bits(m, model), (c["name"], "mixed")
    assert min(seen.values()) >= 10, seen
    # the departures' worked example, and width 1 with the second distinct value lower
    r2, m, _, _ = D.histogram([D.popping_child([1, 5, 9, 13, 17], [5, 9, 13, 17, 21], [0, 1, 0.5, 2, 0.25])], 4)
    assert m.tolist() == [[8.0, 4.0, 4.0, 4.0]] and r2.tolist() == [0.0, 2.0]
    r2, m, _, _ = D.histogram([D.bulk_child([1, 5], [5, 9], [1.0, 0.5])], 1)
    assert m.tolist() == [[8.0]]
    # a first row without a value: a NaN range and zeros
    r2, m, _, _ = D.histogram([D.bulk_child([1], [5], [np.nan]), D.bulk_child([], [], [])], 3)
    assert np.isnan(r2).all() and not m.any()
