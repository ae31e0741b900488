"""Python mirror of the DROP-IN layer of the C ABI (include/wiggletools_amd.h): the reference's own
constructors (newMultiplexer, MeanReduction, ..., reference src/wiggletools.h:80-103) plus the
library's bulk doors (wtamd_ArrayReader, wtamd_iterator_next_block, wtamd_drain).  Used by
bench.py's end-to-end leg and by tests; everything here is a thin ctypes call.
"""
import ctypes as C

import numpy as np

from . import _lib

REDUCERS = {"sum": "SumReduction", "product": "ProductReduction", "mult": "ProductReduction", "mean": "MeanReduction",
            "var": "VarianceReduction", "stddev": "StdDevReduction", "entropy": "EntropyReduction", "cv": "CVReduction",
            "CV": "CVReduction", "median": "MedianReduction", "min": "MinReduction", "max": "MaxReduction"}
SET_REDUCERS = {"ttest": "TTestReduction", "wilcoxon": "MWUReduction", "mwu": "MWUReduction"}


def _bind():
    L = _lib.lib()
    if getattr(L, "_wt_dropin_bound", False):
        return L
    L.wtamd_host_alloc.restype = C.c_void_p
    L.wtamd_host_alloc.argtypes = [C.c_size_t]
    L.wtamd_host_free.argtypes = [C.c_void_p]
    L.wtamd_host_free.restype = None
    L.wtamd_ArrayReader.restype = C.c_void_p
    L.wtamd_ArrayReader.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double]
    L.wtamd_BigWiggleReader.restype = C.c_void_p
    L.wtamd_BigWiggleReader.argtypes = [C.c_char_p, C.c_int]
    L.newMultiplexer.restype = C.c_void_p
    L.newMultiplexer.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_char]
    L.newMultiset.restype = C.c_void_p
    L.newMultiset.argtypes = [C.POINTER(C.c_void_p), C.c_int]
    for name in set(REDUCERS.values()) | set(SET_REDUCERS.values()):
        f = getattr(L, name)
        f.restype = C.c_void_p
        f.argtypes = [C.c_void_p]
    L.wtamd_iterator_next_block.restype = C.c_int64
    L.wtamd_iterator_next_block.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                            C.POINTER(C.c_void_p)]
    L.wtamd_drain.restype = C.c_int64
    L.wtamd_drain.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    L.seek.restype = None
    L.seek.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int]
    L._wt_dropin_bound = True
    return L


class PinnedArray:
    """numpy view of page-locked host memory (wtamd_host_alloc)."""

    def __init__(self, n, dtype):
        L = _bind()
        self.n = int(n)
        self.dtype = np.dtype(dtype)
        self.ptr = L.wtamd_host_alloc(max(self.n, 1) * self.dtype.itemsize)
        if not self.ptr:
            raise MemoryError("wtamd_host_alloc(%d bytes)" % (self.n * self.dtype.itemsize))
        ct = np.ctypeslib.as_ctypes_type(self.dtype)
        self.array = np.ctypeslib.as_array(C.cast(self.ptr, C.POINTER(ct)), shape=(max(self.n, 1),))[:self.n]

    def free(self):
        if self.ptr:
            _bind().wtamd_host_free(self.ptr)
            self.ptr = None


def array_reader(chrom_names, seg_off, start_ptr, finish_ptr, value_ptr, default_value=0.0):
    """wtamd_ArrayReader over raw pointers (int addresses); seg_off: n_chrom + 1 offsets."""
    L = _bind()
    names = (C.c_char_p * len(chrom_names))(*[n.encode() for n in chrom_names])
    so = np.ascontiguousarray(seg_off, np.int64)
    return L.wtamd_ArrayReader(len(chrom_names), names, so.ctypes.data, start_ptr, finish_ptr, value_ptr, float(default_value))


def buffered_array_reader(chrom_names, seg_off, start_ptr, finish_ptr, value_ptr, default_value=0.0):
    """wtamd_BufferedArrayReader: the same arrays behind the reference's buffered-reader protocol (a producer thread
    pushing one interval at a time, csrc/wt_bufreader.h)."""
    L = _bind()
    L.wtamd_BufferedArrayReader.restype = C.c_void_p
    L.wtamd_BufferedArrayReader.argtypes = L.wtamd_ArrayReader.argtypes
    names = (C.c_char_p * len(chrom_names))(*[n.encode() for n in chrom_names])
    so = np.ascontiguousarray(seg_off, np.int64)
    return L.wtamd_BufferedArrayReader(len(chrom_names), names, so.ctypes.data, start_ptr, finish_ptr, value_ptr, float(default_value))


def overlapping_array_reader(chrom_names, seg_off, start_ptr, finish_ptr, value_ptr, default_value=0.0):
    """wtamd_OverlappingArrayReader: wtamd_ArrayReader's arguments, intervals sorted by start only, `overlaps` set."""
    L = _bind()
    L.wtamd_OverlappingArrayReader.restype = C.c_void_p
    L.wtamd_OverlappingArrayReader.argtypes = L.wtamd_ArrayReader.argtypes
    names = (C.c_char_p * len(chrom_names))(*[n.encode() for n in chrom_names])
    so = np.ascontiguousarray(seg_off, np.int64)
    return L.wtamd_OverlappingArrayReader(len(chrom_names), names, so.ctypes.data, start_ptr, finish_ptr, value_ptr, float(default_value))


def coverage_iterator(child):
    """wtamd_CoverageIterator: the reference's `coverage` around an overlapping child (the child itself when it does not
    overlap); a bulk source for multiplexer() / reducer(), readable with drain_blocks() and drain_pops()."""
    L = _bind()
    L.wtamd_CoverageIterator.restype = C.c_void_p
    L.wtamd_CoverageIterator.argtypes = [C.c_void_p]
    return L.wtamd_CoverageIterator(child)


def region_iterator(op, source, mask):
    """wtamd_RegionIterator: the reference's `overlaps`, `noverlaps`, `trim` or `nearest` (engine.REGION_OPS) of `source`
    against `mask`; a bulk source for multiplexer() / reducer(), readable with drain_blocks() and drain_pops()."""
    from .engine import REGION_OPS
    L = _bind()
    L.wtamd_RegionIterator.restype = C.c_void_p
    L.wtamd_RegionIterator.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    return L.wtamd_RegionIterator(REGION_OPS[op] if isinstance(op, str) else int(op), source, mask)


def apply_multiplexer(regions, stats, dataset, strict=True):
    """wtamd_ApplyMultiplexer: the reference's `apply` of `dataset` inside every region of `regions`; stats: names of
    engine.APPLY_STATS or raw codes.  A Multiplexer: read it with popMultiplexer or under SelectReduction."""
    from .engine import APPLY_STATS
    L = _bind()
    L.wtamd_ApplyMultiplexer.restype = C.c_void_p
    L.wtamd_ApplyMultiplexer.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_char]
    codes = (C.c_int * len(stats))(*[APPLY_STATS[s] if isinstance(s, str) else int(s) for s in stats])
    return L.wtamd_ApplyMultiplexer(regions, codes, len(stats), dataset, b"\x01" if strict else b"\x00")


def profile_multiplexer(regions, width, dataset):
    """wtamd_ProfileMultiplexer: the reference's `profiles` of `dataset` under every region of `regions` on `width` bins.  A
    Multiplexer: read it with popMultiplexer or under SelectReduction."""
    L = _bind()
    L.wtamd_ProfileMultiplexer.restype = C.c_void_p
    L.wtamd_ProfileMultiplexer.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    return L.wtamd_ProfileMultiplexer(regions, int(width), dataset)


def bin_iterator(child, width):
    """wtamd_BinIterator: the reference's `bin` of `child` over windows of `width` base pairs on the grid from position 1; a bulk
    source for multiplexer() / reducer(), readable with drain_blocks() and drain_pops()."""
    L = _bind()
    L.wtamd_BinIterator.restype = C.c_void_p
    L.wtamd_BinIterator.argtypes = [C.c_void_p, C.c_int]
    return L.wtamd_BinIterator(child, int(width))


def smooth_iterator(child, width):
    """wtamd_SmoothIterator: the reference's `smooth` of `child`, one run per position with the mean of `width` positions around
    it; a bulk source for multiplexer() / reducer(), readable with drain_blocks() and drain_pops()."""
    L = _bind()
    L.wtamd_SmoothIterator.restype = C.c_void_p
    L.wtamd_SmoothIterator.argtypes = [C.c_void_p, C.c_int]
    return L.wtamd_SmoothIterator(child, int(width))


def _read_back(L, write):
    """What write(FILE *) prints, through a temporary file of the C library."""
    libc = C.CDLL(None)
    libc.tmpfile.restype = C.c_void_p
    libc.fclose.argtypes = libc.rewind.argtypes = libc.fflush.argtypes = [C.c_void_p]
    libc.fread.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
    libc.fread.restype = C.c_size_t
    fp = libc.tmpfile()
    if not fp:
        raise OSError("tmpfile()")
    try:
        write(fp)
        libc.fflush(fp)
        libc.rewind(fp)
        out, buf = [], C.create_string_buffer(1 << 16)
        while True:
            n = libc.fread(buf, 1, len(buf), fp)
            if n == 0:
                return b"".join(out).decode()
            out.append(buf.raw[:n])
    finally:
        libc.fclose(fp)


def histogram(iterators, width, normalize=False):
    """wtamd_histogram: the reference's `histogram` of the iterators, one row each, over `width` value bins.  Returns
    ((lo, hi), (rows, width) matrix, the text wtamd_print_histogram writes); normalize=True: after wtamd_normalize_histogram."""
    L = _bind()
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
    arr = (C.c_void_p * len(iterators))(*iterators)
    h = L.wtamd_histogram(arr, len(iterators), int(width))
    try:
        if normalize:
            L.wtamd_normalize_histogram(h)
        r2 = np.zeros(2, np.float64)
        L.wtamd_histogram_range(h, r2.ctypes.data)
        w, n = L.wtamd_histogram_width(h), L.wtamd_histogram_count(h)
        m = np.array([np.ctypeslib.as_array(L.wtamd_histogram_row(h, r), shape=(w,)).copy() for r in range(n)])
        text = _read_back(L, lambda fp: L.wtamd_print_histogram(h, fp))
    finally:
        L.wtamd_destroy_histogram(h)
    return (float(r2[0]), float(r2[1])), m, text


def energy_integrator(child, wavelength):
    """wtamd_EnergyIntegrator: the reference's `energy (wavelength)` of `child`; pop it to the end (drain_pops), then
    energy_result() reads (res, real, im) where the reference keeps them."""
    L = _bind()
    L.wtamd_EnergyIntegrator.restype = C.c_void_p
    L.wtamd_EnergyIntegrator.argtypes = [C.c_void_p, C.c_int]
    return L.wtamd_EnergyIntegrator(child, int(wavelength))


def energy_result(wi):
    """(res, real, im) of an energy integrator: the head of its `data` (res is NaN until it has been popped to the end)."""
    data = C.cast(wi + 40, C.POINTER(C.c_void_p))[0]       # offsetof(struct wiggleIterator_st, data)
    d = np.ctypeslib.as_array(C.cast(data, C.POINTER(C.c_double)), shape=(3,))
    return float(d[0]), float(d[1]), float(d[2])


def energy_spectrum(child, wavelengths):
    """wtamd_EnergySpectrum: every wavelength from one drain of `child`.  Returns (reim (n, 2), energies (n,))."""
    L = _bind()
    L.wtamd_EnergySpectrum.restype = C.c_int
    L.wtamd_EnergySpectrum.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lam = np.ascontiguousarray(wavelengths, np.int32)
    out = np.zeros((len(lam), 2), np.float64)
    _lib.check(L.wtamd_EnergySpectrum(child, len(lam), lam.ctypes.data, out.ctypes.data))
    return out, out[:, 0] * out[:, 0] + out[:, 1] * out[:, 1]


def _c_file(path, mode="w"):
    libc = C.CDLL(None)
    libc.fopen.restype = C.c_void_p
    libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
    libc.fclose.argtypes = [C.c_void_p]
    fp = libc.fopen(str(path).encode(), mode.encode())
    if not fp:
        raise OSError("could not open %s" % path)
    return fp, (lambda: libc.fclose(fp))


def tee_iterator(child, path, bedgraph=False, hold_fire=False):
    """wtamd_TeeWiggleIterator: the reference's `write` / `write_bg` writer of `child` into the file at `path`, passing the
    runs it prints on.  Returns (iterator, close): pop it to the end (drain_pops / drain_blocks), then call close()."""
    L = _bind()
    L.wtamd_TeeWiggleIterator.restype = C.c_void_p
    L.wtamd_TeeWiggleIterator.argtypes = [C.c_void_p, C.c_void_p, C.c_char, C.c_char]
    fp, close = _c_file(path)
    return L.wtamd_TeeWiggleIterator(child, fp, b"\x01" if bedgraph else b"\x00", b"\x01" if hold_fire else b"\x00"), close


def to_file(child, path, bedgraph=False, hold_fire=False):
    """wtamd_toFile: the reference's toFile -- `child` run to its end, the text at `path`."""
    L = _bind()
    L.wtamd_toFile.restype = None
    L.wtamd_toFile.argtypes = [C.c_void_p, C.c_char_p, C.c_char, C.c_char]
    L.wtamd_toFile(child, str(path).encode(), b"\x01" if bedgraph else b"\x00", b"\x01" if hold_fire else b"\x00")


def to_stdout(child, bedgraph=False, hold_fire=False):
    """wtamd_toStdout: the reference's toStdout."""
    L = _bind()
    L.wtamd_toStdout.restype = None
    L.wtamd_toStdout.argtypes = [C.c_void_p, C.c_char, C.c_char]
    L.wtamd_toStdout(child, b"\x01" if bedgraph else b"\x00", b"\x01" if hold_fire else b"\x00")


def _flag(x):
    return b"\x01" if x else b"\x00"


def tee_multiplexer(multi, path, bedgraph=False, hold_fire=False):
    """wtamd_TeeMultiplexer: the reference's `mwrite` / `mwrite_bg` writer of the Multiplexer `multi` into the file at `path`.
    Returns (multiplexer, close): pop it to the end (popMultiplexer / runMultiplexer), then call close()."""
    L = _bind()
    L.wtamd_TeeMultiplexer.restype = C.c_void_p
    L.wtamd_TeeMultiplexer.argtypes = [C.c_void_p, C.c_void_p, C.c_char, C.c_char]
    fp, close = _c_file(path)
    return L.wtamd_TeeMultiplexer(multi, fp, _flag(bedgraph), _flag(hold_fire)), close


def to_stdout_multiplexer(multi, bedgraph=False, hold_fire=False):
    """wtamd_toStdoutMultiplexer: the reference's toStdoutMultiplexer."""
    L = _bind()
    L.wtamd_toStdoutMultiplexer.restype = None
    L.wtamd_toStdoutMultiplexer.argtypes = [C.c_void_p, C.c_char, C.c_char]
    L.wtamd_toStdoutMultiplexer(multi, _flag(bedgraph), _flag(hold_fire))


def paste_multiplexer(multi, in_path, out_path, hold_fire=False):
    """wtamd_PasteMultiplexer: the reference's `apply_paste` writer -- every entry of `multi` behind the next line of the file
    at `in_path`, into the file at `out_path`.  Returns (multiplexer, close)."""
    L = _bind()
    L.wtamd_PasteMultiplexer.restype = C.c_void_p
    L.wtamd_PasteMultiplexer.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char]
    fin, close_in = _c_file(in_path, "r")
    fout, close_out = _c_file(out_path)
    return L.wtamd_PasteMultiplexer(multi, fin, fout, _flag(hold_fire)), (lambda: (close_out(), close_in()))


def wiggle_reader(path):
    """wtamd_WiggleReader: the reference's WiggleReader (wig fixedStep / variableStep and bedGraph text, compressed behind the
    reader), its chunks parsed on the device; bulk-capable."""
    L = _bind()
    L.wtamd_WiggleReader.restype = C.c_void_p
    L.wtamd_WiggleReader.argtypes = [C.c_char_p]
    return L.wtamd_WiggleReader(str(path).encode())


def bed_reader(path):
    """wtamd_BedReader: the reference's BedReader (value 1, overlapping), its chunks parsed on the device; bulk-capable."""
    L = _bind()
    L.wtamd_BedReader.restype = C.c_void_p
    L.wtamd_BedReader.argtypes = [C.c_char_p]
    return L.wtamd_BedReader(str(path).encode())


def bigwig_reader(path, box=True):
    """wtamd_BigWiggleReader: the reference's BigWiggleReader role (bigWiggleReader.c:147-151), bulk-capable."""
    return _bind().wtamd_BigWiggleReader(path.encode(), int(box))


def bigwig_readers(paths, box=True):
    """wtamd_BigWiggleReaders: n files opened side by side."""
    L = _bind()
    L.wtamd_BigWiggleReaders.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_int, C.POINTER(C.c_void_p)]
    arr = (C.c_char_p * len(paths))(*[p.encode() for p in paths])
    out = (C.c_void_p * len(paths))()
    if L.wtamd_BigWiggleReaders(len(paths), arr, int(box), out) != 0:
        raise _lib.WtamdError("wtamd_BigWiggleReaders failed")
    return list(out)


def multiplexer(iters, strict=False):
    L = _bind()
    arr = (C.c_void_p * len(iters))(*iters)
    return L.newMultiplexer(arr, len(iters), b"\x01" if strict else b"\x00")


def reducer(op, iters, n_set0=0, strict=False):
    """The reducer iterator the reference's parser would build for `op` over the child iterators."""
    L = _bind()
    if op in SET_REDUCERS:
        ms = (C.c_void_p * 2)(multiplexer(iters[:n_set0], strict), multiplexer(iters[n_set0:], strict))
        keep = ms                       # newMultiset keeps the caller's array (multiSet.c:118)
        r = getattr(L, SET_REDUCERS[op])(L.newMultiset(ms, 2))
        _KEEP.append(keep)
        return r
    return getattr(L, REDUCERS[op])(multiplexer(iters, strict))


_KEEP = []


def seek(wi, chrom, start, finish):
    """The reference's seek() (wiggleIterator.c:67-70): restricts an iterator to chrom:[start, finish)."""
    _bind().seek(wi, chrom.encode(), int(start), int(finish))


def drain_blocks(wi, on_block=None):
    """Consumes a reducer (or a coverage iterator) through the block door; returns (runs, covered bp)."""
    L = _bind()
    chrom, s, f, v = C.c_char_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    runs = bp = 0
    while True:
        n = L.wtamd_iterator_next_block(wi, C.byref(chrom), C.byref(s), C.byref(f), C.byref(v))
        if n < 0:
            raise _lib.WtamdError("wtamd_iterator_next_block: neither a reducer nor a coverage iterator of this library")
        if n == 0:
            return runs, bp
        runs += n
        if on_block is not None:
            i32 = C.POINTER(C.c_int32)
            sa = np.ctypeslib.as_array(C.cast(s, i32), shape=(n,))
            fa = np.ctypeslib.as_array(C.cast(f, i32), shape=(n,))
            va = np.ctypeslib.as_array(C.cast(v, C.POINTER(C.c_double)), shape=(n,))
            bp += on_block(chrom.value, sa, fa, va)


def pipe_stats(wi):
    from .pipe import PipeStats
    L = _bind()
    st = PipeStats()
    L.wtamd_iterator_pipe_stats.argtypes = [C.c_void_p, C.POINTER(PipeStats)]
    if L.wtamd_iterator_pipe_stats(wi, C.byref(st)) != 0:
        return {}
    return {k: getattr(st, k) for k, _ in PipeStats._fields_}


def drain_pops(wi):
    """Consumes an iterator one pop at a time (in C); returns (runs, covered bp, value sum)."""
    L = _bind()
    bp, acc = C.c_int64(), C.c_double()
    n = L.wtamd_drain(wi, C.byref(bp), C.byref(acc))
    return n, bp.value, acc.value
