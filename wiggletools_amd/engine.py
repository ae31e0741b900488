"""Python mirror of the bulk C ABI (include/wiggletools_amd.h, wtamd_*).

Operator names follow the reference CLI grammar (reference commandParser.c:46-61,
763-826): sum, mult(product), mean, var, stddev, entropy, CV, min, max, median,
ttest, wilcoxon(mwu).  PyTorch is used only to own device memory / streams.
"""
import ctypes as C

import numpy as np

from . import _lib
from .runlists import RunLists

OPS = {"sum": 0, "product": 1, "mult": 1, "mean": 2, "var": 3, "stddev": 4, "entropy": 5, "cv": 6, "CV": 6,
       "min": 7, "max": 8, "median": 9, "ttest": 10, "mwu": 11, "wilcoxon": 11}
STRICT_SET0, STRICT_SET1 = 1, 2
STATS = {"var": 0, "stddev": 1, "cv": 2, "CV": 2, "max": 3, "min": 4, "span": 5}      # WTAMD_STAT_*


def opcode(op):
    if isinstance(op, str):
        if op not in OPS:
            raise ValueError("unknown reducer %r" % op)
        return OPS[op]
    return int(op)


def reducer_default(op, defaults):
    d = np.ascontiguousarray(defaults, np.float64)
    return _lib.lib().wtamd_reducer_default(opcode(op), len(d), d.ctypes.data)


MAP_OPS = {"scale": 0, "offset": 1, "ln": 2, "log": 3, "exp": 4, "expb": 5, "pow": 6, "abs": 7,
           "gt": 8, "gte": 9, "lt": 10, "lte": 11}


def map_default(op, param, default_value):
    return _lib.lib().wtamd_map_default(MAP_OPS[op], float(param), float(default_value))


def map_runlists(rl: RunLists, op, param=0.0):
    """The reference's `map`-able unary operator `op` over every track of `rl`, on device
    (wtamd_runs_map): returns a new RunLists with f64 values and transformed defaults."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    n = int(rl.seg_off[-1])
    n_seg = rl.n_chrom * rl.n_tracks
    seg = np.ascontiguousarray(rl.seg_off, np.int64)
    s = torch.from_numpy(np.ascontiguousarray(rl.start, np.int32)).to(dev)
    f = torch.from_numpy(np.ascontiguousarray(rl.finish, np.int32)).to(dev)
    v = torch.from_numpy(np.ascontiguousarray(rl.value)).to(dev)
    os_ = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    of = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    ov = torch.empty(max(n, 1), dtype=torch.float64, device=dev)
    oseg = np.zeros(n_seg + 1, np.int64)
    _lib.check(_lib.lib().wtamd_runs_map(MAP_OPS[op], float(param), n_seg, seg.ctypes.data, s.data_ptr(), f.data_ptr(),
                                         v.data_ptr(), 1 if rl.value.dtype == np.float64 else 0, os_.data_ptr(),
                                         of.data_ptr(), ov.data_ptr(), oseg.ctypes.data, None))
    m = int(oseg[-1])
    d = np.array([map_default(op, param, x) for x in rl.defaults], np.float64)
    return RunLists(rl.n_chrom, rl.n_tracks, oseg, os_[:m].cpu().numpy(), of[:m].cpu().numpy(), ov[:m].cpu().numpy(), d)


COVER_ANY_ORDER = 1      # WTAMD_COVER_ANY_ORDER


def _overlap_door(rl, union, capacity=None, flags=None):
    """wtamd_runs_coverage / wtamd_runs_union over every segment of `rl`; returns (rc, runs needed, RunLists or None).
    flags (coverage only): not None goes through wtamd_runs_coverage_flags."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    n = int(rl.seg_off[-1])
    n_seg = rl.n_chrom * rl.n_tracks
    cap = (n if union else max(2 * n - 1, 0)) if capacity is None else int(capacity)
    seg = np.ascontiguousarray(rl.seg_off, np.int64)
    s = torch.from_numpy(np.ascontiguousarray(rl.start, np.int32)).to(dev)
    f = torch.from_numpy(np.ascontiguousarray(rl.finish, np.int32)).to(dev)
    os_ = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
    of = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
    ov = torch.empty(max(cap, 1), dtype=torch.float64, device=dev)
    oseg = np.zeros(n_seg + 1, np.int64)
    n_out = C.c_int64()
    L = _lib.lib()
    if union:
        v = torch.from_numpy(np.ascontiguousarray(rl.value)).to(dev)
        rc = L.wtamd_runs_union(n_seg, seg.ctypes.data, s.data_ptr(), f.data_ptr(), v.data_ptr(), 1 if rl.value.dtype == np.float64 else 0,
                                cap, os_.data_ptr(), of.data_ptr(), ov.data_ptr(), oseg.ctypes.data, C.byref(n_out), None)
    elif flags is None:
        rc = L.wtamd_runs_coverage(n_seg, seg.ctypes.data, s.data_ptr(), f.data_ptr(), cap, os_.data_ptr(), of.data_ptr(), ov.data_ptr(),
                                   oseg.ctypes.data, C.byref(n_out), None)
    else:
        rc = L.wtamd_runs_coverage_flags(n_seg, seg.ctypes.data, s.data_ptr(), f.data_ptr(), cap, os_.data_ptr(), of.data_ptr(), ov.data_ptr(),
                                         oseg.ctypes.data, C.byref(n_out), int(flags), None)
    if rc != 0:
        return rc, n_out.value, None
    m = n_out.value
    d = rl.defaults if union else np.zeros(rl.n_tracks, np.float64)
    return 0, m, RunLists(rl.n_chrom, rl.n_tracks, oseg, os_[:m].cpu().numpy(), of[:m].cpu().numpy(), ov[:m].cpu().numpy(), d, rl.chrom_names)


def coverage_runlists(rl: RunLists, any_order=False):
    """The reference's `coverage` (CoverageWiggleIterator, unaryOps.c:303-375) over every track of `rl`, whose intervals may
    overlap (each segment sorted by start), on device (wtamd_runs_coverage): the depth tracks as a new RunLists, f64 values,
    defaults 0.  Without the reference's one run of start == finish per stream (include/wiggletools_amd.h).  any_order: the
    intervals of a segment in any order (wtamd_runs_coverage_flags, WTAMD_COVER_ANY_ORDER)."""
    rc, _, out = _overlap_door(rl, False, flags=COVER_ANY_ORDER if any_order else None)
    _lib.check(rc)
    return out


def union_runlists(rl: RunLists):
    """The reference's UnionWiggleIterator (unaryOps.c:60-92) over every track of `rl` on device (wtamd_runs_union):
    overlapping intervals merged into groups with the first member's start and value (f64) and the largest finish."""
    rc, _, out = _overlap_door(rl, True)
    _lib.check(rc)
    return out


REGION_OPS = {"overlaps": 0, "noverlaps": 1, "trim": 2, "nearest": 3}      # WTAMD_REGION_*


def _region_door(op, source, mask, capacity=None):
    """wtamd_runs_region over every segment pair of `source` and `mask`; op: a name of REGION_OPS or a raw code.  Returns
    (rc, runs needed, RunLists or None)."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    op = REGION_OPS[op] if isinstance(op, str) else int(op)
    n_seg = source.n_chrom * source.n_tracks
    if mask.n_chrom * mask.n_tracks != n_seg:
        raise ValueError("region: source and mask must have the same number of segments")
    n, m = int(source.seg_off[-1]), int(mask.seg_off[-1])
    cap = (n + m if op == REGION_OPS["trim"] else n) if capacity is None else int(capacity)
    seg, mseg = np.ascontiguousarray(source.seg_off, np.int64), np.ascontiguousarray(mask.seg_off, np.int64)
    s = torch.from_numpy(np.ascontiguousarray(source.start, np.int32)).to(dev)
    f = torch.from_numpy(np.ascontiguousarray(source.finish, np.int32)).to(dev)
    v = torch.from_numpy(np.ascontiguousarray(source.value)).to(dev)
    ms = torch.from_numpy(np.ascontiguousarray(mask.start, np.int32)).to(dev)
    mf = torch.from_numpy(np.ascontiguousarray(mask.finish, np.int32)).to(dev)
    os_ = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
    of = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
    ov = torch.empty(max(cap, 1), dtype=torch.float64, device=dev)
    oseg = np.zeros(n_seg + 1, np.int64)
    n_out = C.c_int64()
    rc = _lib.lib().wtamd_runs_region(op, n_seg, seg.ctypes.data, s.data_ptr(), f.data_ptr(), v.data_ptr(),
                                      1 if source.value.dtype == np.float64 else 0, mseg.ctypes.data, ms.data_ptr(), mf.data_ptr(), cap,
                                      os_.data_ptr(), of.data_ptr(), ov.data_ptr(), oseg.ctypes.data, C.byref(n_out), None)
    if rc != 0:
        return rc, n_out.value, None
    k = n_out.value
    return 0, k, RunLists(source.n_chrom, source.n_tracks, oseg, os_[:k].cpu().numpy(), of[:k].cpu().numpy(), ov[:k].cpu().numpy(),
                          source.defaults, source.chrom_names)


def region_runlists(op, source: RunLists, mask: RunLists):
    """The reference's `overlaps`, `noverlaps`, `trim` or `nearest` (unaryOps.c:437-639) of every segment of `source`
    against the segment of `mask` at the same place, on device (wtamd_runs_region): a new RunLists with f64 values and the
    source's defaults.  A trim source must not overlap itself (include/wiggletools_amd.h)."""
    rc, _, out = _region_door(op, source, mask)
    _lib.check(rc)
    return out


APPLY_STATS = {"AUC": 0, "meanI": 1, "varI": 2, "stddevI": 3, "CVI": 4, "maxI": 5, "minI": 6}      # WTAMD_APPLY_*
APPLY_STRICT = 1


def _apply_door(data, regions, default=0.0, strict=True, flags=None):
    """wtamd_runs_apply over every segment pair of `data` and `regions`.  Returns (rc, (n, 6) array); the array starts out
    filled with -1 and a refused call leaves it so."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    n_seg = data.n_chrom * data.n_tracks
    if regions.n_chrom * regions.n_tracks != n_seg:
        raise ValueError("apply: data and regions must have the same number of segments")
    n_r = int(regions.seg_off[-1])
    seg, rseg = np.ascontiguousarray(data.seg_off, np.int64), np.ascontiguousarray(regions.seg_off, np.int64)
    s = torch.from_numpy(np.ascontiguousarray(data.start, np.int32)).to(dev)
    f = torch.from_numpy(np.ascontiguousarray(data.finish, np.int32)).to(dev)
    v = torch.from_numpy(np.ascontiguousarray(data.value)).to(dev)
    rs = torch.from_numpy(np.ascontiguousarray(regions.start, np.int32)).to(dev)
    rf = torch.from_numpy(np.ascontiguousarray(regions.finish, np.int32)).to(dev)
    out = torch.full((max(n_r, 1), 6), -1.0, dtype=torch.float64, device=dev)
    fl = (APPLY_STRICT if strict else 0) if flags is None else int(flags)
    rc = _lib.lib().wtamd_runs_apply(n_seg, seg.ctypes.data, s.data_ptr(), f.data_ptr(), v.data_ptr(),
                                     1 if data.value.dtype == np.float64 else 0, rseg.ctypes.data, rs.data_ptr(), rf.data_ptr(),
                                     float(default), fl, out.data_ptr(), None)
    return rc, out[:n_r].cpu().numpy()


def apply_runlists(data: RunLists, regions: RunLists, default=0.0, strict=True):
    """The reference's `apply` (ApplyMultiplexer, src/apply.c) as six moments per region, on device (wtamd_runs_apply):
    {sum of L v, span, T, min, max, covered} of every segment of `data` inside every region of the segment of `regions` at the
    same place, an (n, 6) array in region order.  strict=False is `fillIn`: uncovered base pairs enter with `default`.  The
    data must not overlap itself (include/wiggletools_amd.h); apply_finish turns a row into a statistic."""
    rc, out = _apply_door(data, regions, default, strict)
    _lib.check(rc)
    return out


def apply_finish(m6, stat):
    """AUC, meanI, varI, stddevI, CVI, maxI or minI (a name of APPLY_STATS or a raw code) from one row of apply_runlists."""
    m = np.ascontiguousarray(m6, np.float64)
    assert m.shape == (6,)
    return _lib.lib().wtamd_apply_finish(m.ctypes.data, APPLY_STATS[stat] if isinstance(stat, str) else int(stat))


PROFILE_SUM = 1


def _profile_door(data, regions, width, default=0.0, sum=False, flags=None):
    """wtamd_runs_profile over every segment pair of `data` and `regions`.  Returns (rc, (n, width) array, or (width,) in sum
    mode); the array starts out filled with -1 and a refused call leaves it so."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    n_seg = data.n_chrom * data.n_tracks
    if regions.n_chrom * regions.n_tracks != n_seg:
        raise ValueError("profile: data and regions must have the same number of segments")
    n_r = int(regions.seg_off[-1])
    seg, rseg = np.ascontiguousarray(data.seg_off, np.int64), np.ascontiguousarray(regions.seg_off, np.int64)
    s = torch.from_numpy(np.ascontiguousarray(data.start, np.int32)).to(dev)
    f = torch.from_numpy(np.ascontiguousarray(data.finish, np.int32)).to(dev)
    v = torch.from_numpy(np.ascontiguousarray(data.value)).to(dev)
    rs = torch.from_numpy(np.ascontiguousarray(regions.start, np.int32)).to(dev)
    rf = torch.from_numpy(np.ascontiguousarray(regions.finish, np.int32)).to(dev)
    fl = (PROFILE_SUM if sum else 0) if flags is None else int(flags)
    rows = 1 if fl & PROFILE_SUM else n_r
    out = torch.full((max(rows, 1), max(int(width), 1)), -1.0, dtype=torch.float64, device=dev)
    rc = _lib.lib().wtamd_runs_profile(n_seg, seg.ctypes.data, s.data_ptr(), f.data_ptr(), v.data_ptr(),
                                       1 if data.value.dtype == np.float64 else 0, rseg.ctypes.data, rs.data_ptr(), rf.data_ptr(),
                                       int(width), float(default), fl, out.data_ptr(), None)
    out = out.cpu().numpy()
    return rc, (out[0] if fl & PROFILE_SUM else out[:n_r])


def profile_runlists(data: RunLists, regions: RunLists, width, default=0.0, sum=False):
    """The reference's `profiles` (ProfileMultiplexer, src/apply.c, over regionProfile, src/plots.c) on device
    (wtamd_runs_profile): every segment of `data` under every region of the segment of `regions` at the same place, squeezed or
    stretched onto `width` bins -- an (n, width) array in region order; sum=True is `profile`: the (width,) column sums.
    Uncovered stretches enter as one sample of `default` each.  The data must not overlap itself (include/wiggletools_amd.h)."""
    rc, out = _profile_door(data, regions, width, default, sum)
    _lib.check(rc)
    return out


def _window_door(rl, width, default=None, clip=(0, 0), capacity=None):
    """wtamd_runs_bin (default given) or wtamd_runs_smooth (default None) over every segment of `rl`.  Returns (rc, runs
    needed, (seg_off, start, finish, value) arrays); the arrays start out filled with -1 and a refused call leaves them so."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    n_seg = rl.n_chrom * rl.n_tracks
    seg = np.ascontiguousarray(rl.seg_off, np.int64)
    w = max(int(width), 1)
    if capacity is None:
        s64, f64 = np.asarray(rl.start, np.int64), np.asarray(rl.finish, np.int64)
        if default is not None:
            capacity = int(((f64 - 2) // w - (s64 - 1) // w + 1).sum()) if len(s64) else 0
        else:
            capacity = sum(int(f64[b - 1]) - max(1, int(s64[a]) - w // 2) + w for a, b in zip(seg[:-1], seg[1:]) if b > a)
            if tuple(clip) != (0, 0):
                capacity = min(capacity, max(int(clip[1]) - int(clip[0]), 0) * n_seg)
    cap = max(int(capacity), 0)
    s = torch.from_numpy(np.ascontiguousarray(rl.start, np.int32)).to(dev)
    f = torch.from_numpy(np.ascontiguousarray(rl.finish, np.int32)).to(dev)
    v = torch.from_numpy(np.ascontiguousarray(rl.value)).to(dev)
    os_ = torch.full((max(cap, 1),), -1, dtype=torch.int32, device=dev)
    of = torch.full((max(cap, 1),), -1, dtype=torch.int32, device=dev)
    ov = torch.full((max(cap, 1),), -1.0, dtype=torch.float64, device=dev)
    oseg = np.zeros(n_seg + 1, np.int64)
    n_out = C.c_int64()
    is64 = 1 if rl.value.dtype == np.float64 else 0
    L = _lib.lib()
    if default is not None:
        rc = L.wtamd_runs_bin(n_seg, seg.ctypes.data, s.data_ptr(), f.data_ptr(), v.data_ptr(), is64, int(width), float(default), cap,
                              os_.data_ptr(), of.data_ptr(), ov.data_ptr(), oseg.ctypes.data, C.byref(n_out), None)
    else:
        rc = L.wtamd_runs_smooth(n_seg, seg.ctypes.data, s.data_ptr(), f.data_ptr(), v.data_ptr(), is64, int(width), int(clip[0]), int(clip[1]), cap,
                                 os_.data_ptr(), of.data_ptr(), ov.data_ptr(), oseg.ctypes.data, C.byref(n_out), None)
    return rc, n_out.value, (oseg, os_.cpu().numpy(), of.cpu().numpy(), ov.cpu().numpy())


def _window_runlists(rl, rc, m, out, defaults):
    _lib.check(rc)
    oseg, os_, of, ov = out
    return RunLists(rl.n_chrom, rl.n_tracks, oseg, os_[:m], of[:m], ov[:m], defaults, rl.chrom_names)


def bin_runlists(rl: RunLists, width):
    """The reference's `bin` (BinningWiggleIterator, unaryOps.c:963-1036) over every track of `rl` on device (wtamd_runs_bin):
    the grid bins [1 + k width, 1 + (k + 1) width) a run intersects, each with the sum of covered x value plus the track's
    default over what is not covered; f64 values, defaults x width.  The runs must not overlap and start at 1 or above
    (include/wiggletools_amd.h)."""
    n_seg = rl.n_chrom * rl.n_tracks
    if len(set(np.asarray(rl.defaults, np.float64).view(np.uint64).tolist())) > 1:
        raise ValueError("bin: the tracks of one call share one default")
    d = float(rl.defaults[0]) if n_seg and len(rl.defaults) else 0.0
    rc, m, out = _window_door(rl, width, d)
    return _window_runlists(rl, rc, m, out, np.asarray(rl.defaults, np.float64) * width)


def smooth_runlists(rl: RunLists, width, clip=(0, 0)):
    """The reference's `smooth` (SmoothWiggleIterator, unaryOps.c:1039-1162) over every track of `rl` on device
    (wtamd_runs_smooth): one run per position with the mean of the window of `width` positions around it, by the reference's
    rules at the ends of a chromosome; clip = (lo, hi) delivers the positions of [lo, hi) only.  The runs must not overlap and
    start at 1 or above (include/wiggletools_amd.h)."""
    rc, m, out = _window_door(rl, width, None, clip)
    return _window_runlists(rl, rc, m, out, rl.defaults)


HIST_RANGE_GIVEN, HIST_ACCUMULATE = 1, 2      # WTAMD_HIST_*


def _hist_door(rl, width, flags=0, range=None, hist=None, seg_row=None, n_rows=None):
    """wtamd_runs_histogram over every segment of `rl`; row of a segment: its track, or seg_row[segment] with n_rows rows.
    Returns (rc, range (2,), matrix (n_rows, width)).  Both outputs start out filled with -1 -- or hold `range` and `hist`, the
    inputs of WTAMD_HIST_RANGE_GIVEN and WTAMD_HIST_ACCUMULATE -- and a refused call leaves them so."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    n_seg = rl.n_chrom * rl.n_tracks
    seg = np.ascontiguousarray(rl.seg_off, np.int64)
    rows = np.ascontiguousarray(np.tile(np.arange(rl.n_tracks), rl.n_chrom) if seg_row is None else seg_row, np.int32)
    assert len(rows) == n_seg
    nr = rl.n_tracks if n_rows is None else int(n_rows)
    s = torch.from_numpy(np.ascontiguousarray(rl.start, np.int32)).to(dev)
    f = torch.from_numpy(np.ascontiguousarray(rl.finish, np.int32)).to(dev)
    v = torch.from_numpy(np.ascontiguousarray(rl.value)).to(dev)
    shape = (max(nr, 1), max(int(width), 1))
    if hist is None:
        out = torch.full(shape, -1.0, dtype=torch.float64, device=dev)
    else:
        out = torch.from_numpy(np.ascontiguousarray(hist, np.float64).reshape(shape)).to(dev)
    r2 = np.full(2, -1.0) if range is None else np.array(range, np.float64)
    rc = _lib.lib().wtamd_runs_histogram(n_seg, seg.ctypes.data, rows.ctypes.data, nr, s.data_ptr(), f.data_ptr(), v.data_ptr(),
                                         1 if rl.value.dtype == np.float64 else 0, int(width), int(flags), r2.ctypes.data, out.data_ptr(), None)
    return rc, r2, out.cpu().numpy()


def histogram_runlists(rl: RunLists, width):
    """The reference's `histogram` (histogram(), src/plots.c:167-194) over `rl` on device (wtamd_runs_histogram), one row per
    track: ((lo, hi), (n_tracks, width) matrix of base pairs per value bin).  Bins are exact over the final range
    (include/wiggletools_amd.h lists where the reference, which re-bins as it streams, differs)."""
    rc, r2, out = _hist_door(rl, width)
    _lib.check(rc)
    return (float(r2[0]), float(r2[1])), out


def _energy_door(rl, wavelengths, seg_base=None):
    """wtamd_runs_energy over every segment of `rl`, in order, as ONE sequence (a track set of one track: its chromosomes).
    Returns (rc, reim (n_wavelengths, 2), end_base).  The outputs start out filled with -1 and a refused call leaves them so."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    n_seg = rl.n_chrom * rl.n_tracks
    seg = np.ascontiguousarray(rl.seg_off, np.int64)
    lam = np.ascontiguousarray(wavelengths, np.int32)
    sb = None if seg_base is None else np.ascontiguousarray(seg_base, np.int64)
    assert sb is None or len(sb) == n_seg
    s = torch.from_numpy(np.ascontiguousarray(rl.start, np.int32)).to(dev)
    f = torch.from_numpy(np.ascontiguousarray(rl.finish, np.int32)).to(dev)
    v = torch.from_numpy(np.ascontiguousarray(rl.value)).to(dev)
    out = np.full((max(len(lam), 1), 2), -1.0)
    end = np.full(1, -1, np.int64)
    rc = _lib.lib().wtamd_runs_energy(n_seg, seg.ctypes.data, None if sb is None else sb.ctypes.data, s.data_ptr(), f.data_ptr(), v.data_ptr(),
                                      1 if rl.value.dtype == np.float64 else 0, len(lam), lam.ctypes.data, out.ctypes.data, end.ctypes.data, None)
    return rc, out, int(end[0])


def energy_runlists(rl: RunLists, wavelengths):
    """The reference's `energy` (EnergyIntegrator, src/statistics.c:345-391) of every track of `rl` on device (wtamd_runs_energy),
    all wavelengths from one read of a track's runs: an (n_tracks, n_wavelengths) array of real^2 + im^2.  A chromosome is shifted
    by the last finishes of the track's chromosomes before it, as the reference's offset rule has it; the runs of a chromosome
    must be sorted and disjoint (include/wiggletools_amd.h lists where the reference, which sums position by position, differs)."""
    out = np.zeros((rl.n_tracks, len(wavelengths)))
    for t in range(rl.n_tracks):
        segs = [(int(rl.seg_off[c * rl.n_tracks + t]), int(rl.seg_off[c * rl.n_tracks + t + 1])) for c in range(rl.n_chrom)]
        idx = np.concatenate([np.arange(a, b) for a, b in segs] + [np.zeros(0, np.int64)]).astype(np.int64)
        one = RunLists(rl.n_chrom, 1, np.concatenate([[0], np.cumsum([b - a for a, b in segs])]), rl.start[idx], rl.finish[idx], rl.value[idx],
                       [rl.defaults[t]])
        rc, reim, _ = _energy_door(one, wavelengths)
        _lib.check(rc)
        out[t] = reim[:, 0] * reim[:, 0] + reim[:, 1] * reim[:, 1]
    return out


TEXT_BEDGRAPH, TEXT_BLOCK = 1, 10000          # WTAMD_TEXT_*
TEXT_CANARY = 0xC7


class TextState(C.Structure):
    """wtamd_text_state: chains the batches of one writer."""
    _fields_ = [(k, C.c_int32) for k in ("in_block", "point_by_point", "last_finish", "continues")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


def _text_door(rl, flags=0, state=None, capacity=None, offset=0, names=None, seg_off=None, n_seg=None):
    """wtamd_runs_text over every segment of `rl` (one track), in order.  Returns (rc, the whole buffer as a uint8 array,
    n_bytes, n_wide, state after as a dict or None).  The text starts at byte `offset` of a device buffer of offset + capacity
    + 64 bytes filled with TEXT_CANARY; capacity None: the size a first call with no room reports.  state: a dict of the
    fields of wtamd_text_state, or None.  names: the segments' names as bytes (default: rl.chrom_names).  seg_off / n_seg: given
    to the door in place of rl's own (the refusals).  n_bytes and n_wide start out as -1."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    assert rl.n_tracks == 1
    names = [n.encode() if isinstance(n, str) else n for n in (rl.chrom_names if names is None else names)]
    arr = (C.c_char_p * max(len(names), 1))(*names)
    seg = np.ascontiguousarray(rl.seg_off if seg_off is None else seg_off, np.int64)
    n_seg = len(names) if n_seg is None else int(n_seg)
    s = torch.from_numpy(np.ascontiguousarray(rl.start, np.int32)).to(dev)
    f = torch.from_numpy(np.ascontiguousarray(rl.finish, np.int32)).to(dev)
    v = torch.from_numpy(np.ascontiguousarray(rl.value)).to(dev)
    is64 = 1 if rl.value.dtype == np.float64 else 0
    fn = _lib.lib().wtamd_runs_text
    nb, nw = C.c_int64(-1), C.c_int64(-1)
    if capacity is None:
        st = TextState(**state) if state is not None else None
        rc = fn(n_seg, seg.ctypes.data, arr, s.data_ptr(), f.data_ptr(), v.data_ptr(), is64, int(flags), C.byref(st) if st is not None else None,
                None, 0, C.byref(nb), C.byref(nw), None)
        capacity = max(int(nb.value), 0)
        nb, nw = C.c_int64(-1), C.c_int64(-1)
    buf = torch.full((offset + capacity + 64,), TEXT_CANARY, dtype=torch.uint8, device=dev)
    st = TextState(**state) if state is not None else None
    rc = fn(n_seg, seg.ctypes.data, arr, s.data_ptr(), f.data_ptr(), v.data_ptr(), is64, int(flags), C.byref(st) if st is not None else None,
            buf.data_ptr() + offset, int(capacity), C.byref(nb), C.byref(nw), None)
    return rc, buf.cpu().numpy(), int(nb.value), int(nw.value), (st.as_dict() if st is not None else None)


def text_runlists(rl: RunLists, bedgraph=False, track=0):
    """The reference's `write` / `write_bg` (printBlock of TeeWiggleIterator, src/wigWriter.c:55-119) of one track of `rl` on
    device (wtamd_runs_text): the bytes of the file.  The list is printed as it is: the compression the reference's wig writer
    puts in front is the caller's (wtamd_runs_compress).  A finite value of 2^64 or more is refused (include/wiggletools_amd.h)."""
    t = int(track)
    segs = [(int(rl.seg_off[c * rl.n_tracks + t]), int(rl.seg_off[c * rl.n_tracks + t + 1])) for c in range(rl.n_chrom)]
    idx = np.concatenate([np.arange(a, b) for a, b in segs] + [np.zeros(0, np.int64)]).astype(np.int64)
    one = RunLists(rl.n_chrom, 1, np.concatenate([[0], np.cumsum([b - a for a, b in segs])]), rl.start[idx], rl.finish[idx], rl.value[idx],
                   [rl.defaults[t]], list(rl.chrom_names))
    rc, buf, nb, _, _ = _text_door(one, TEXT_BEDGRAPH if bedgraph else 0)
    _lib.check(rc)
    return buf[:nb].tobytes()


MTEXT_BEDGRAPH, MTEXT_STRICT, MTEXT_MAX_WIDTH = 1, 2, 65536          # WTAMD_MTEXT_*


def _mtext_door(names, seg_off, start, finish, values, prefixes=None, flags=0, state=None, capacity=None, offset=0, width=None, prefix_mode="both",
                host=False):
    """wtamd_tile_text (host=True: wtamd_tile_text_host) over a tile: names (bytes or str, one per segment), seg_off, start /
    finish (n), values (n x width float64), prefixes (None, or n bytes objects: paste).  Returns what _text_door returns.  width:
    given to the door in place of the tile's own; prefix_mode "prefix" / "off": only that one of prefix / prefix_off is given
    (the refusals)."""
    import torch
    names = [n.encode() if isinstance(n, str) else n for n in names]
    arr = (C.c_char_p * max(len(names), 1))(*names)
    seg = np.ascontiguousarray(seg_off, np.int64)
    s, f = np.ascontiguousarray(start, np.int32), np.ascontiguousarray(finish, np.int32)
    v = np.ascontiguousarray(values, np.float64).reshape(len(s), -1) if len(s) else np.zeros((0, max(int(width or 1), 1)))
    pre = off = None
    if prefixes is not None:
        off = np.zeros(len(s) + 1, np.int64)
        off[1:] = np.cumsum([len(p) for p in prefixes])
        pre = np.frombuffer(b"".join(prefixes) + b"\0", np.uint8).copy()
    w = int(v.shape[1] if width is None else width)
    if host:
        fn, tail = _lib.lib().wtamd_tile_text_host, ()
        ptr = lambda a: a.ctypes.data if a is not None else None       # noqa: E731
        keep = (s, f, v, pre, off)
    else:
        dev = torch.device("cuda", torch.cuda.current_device())
        fn, tail = _lib.lib().wtamd_tile_text, (None,)
        keep = tuple(torch.from_numpy(a).to(dev) if a is not None else None for a in (s, f, v, pre, off))
        ptr = lambda t: t.data_ptr() if t is not None else None        # noqa: E731
    ps, pf, pv, pp, po = (ptr(a) for a in keep)
    if prefix_mode == "prefix":
        po = None
    if prefix_mode == "off":
        pp = None

    def once(text_ptr, cap):
        st = TextState(**state) if state is not None else None
        nb, nw = C.c_int64(-1), C.c_int64(-1)
        rc = fn(len(names), seg.ctypes.data, arr, ps, pf, pv, w, pp, po, int(flags), C.byref(st) if st is not None else None, text_ptr, int(cap),
                C.byref(nb), C.byref(nw), *tail)
        return rc, int(nb.value), int(nw.value), (st.as_dict() if st is not None else None)

    if capacity is None:
        capacity = max(once(None, 0)[1], 0)
    if host:
        buf = np.full(offset + capacity + 64, TEXT_CANARY, np.uint8)
        rc, nb, nw, st = once(buf.ctypes.data + offset, capacity)
        return rc, buf, nb, nw, st
    buf = torch.full((offset + capacity + 64,), TEXT_CANARY, dtype=torch.uint8, device=dev)
    rc, nb, nw, st = once(buf.data_ptr() + offset, capacity)
    return rc, buf.cpu().numpy(), nb, nw, st


def tile_text(names, seg_off, start, finish, values, prefixes=None, bedgraph=False):
    """The reference's `mwrite` / `mwrite_bg` / paste text (printBlock of TeeMultiplexer, src/mWigWriter.c:56-133) of a tile on
    the device (wtamd_tile_text): the bytes of the file.  values: n x width; prefixes: one bytes object per entry (paste)."""
    rc, buf, nb, _, _ = _mtext_door(names, seg_off, start, finish, values, prefixes, MTEXT_BEDGRAPH if bedgraph else 0)
    _lib.check(rc)
    return buf[:nb].tobytes()


READ_BED, READ_EOF = 1, 2          # WTAMD_READ_*
READ_CANARY = 0x5C


class ReadState(C.Structure):
    """wtamd_read_state: chains the chunks of one file; all zero at its start."""
    _fields_ = [("mode", C.c_int32), ("span", C.c_int32), ("step", C.c_int32), ("last_start", C.c_int32), ("next", C.c_int64),
                ("chrom_len", C.c_int32), ("rec_len", C.c_int32), ("chrom", C.c_char * 256), ("rec_name", C.c_char * 256)]

    def as_dict(self):
        return {"mode": int(self.mode), "span": int(self.span), "step": int(self.step), "last_start": int(self.last_start), "next": int(self.next),
                "chrom": self.chrom[:self.chrom_len], "rec_name": self.rec_name[:self.rec_len]}

    @classmethod
    def from_dict(cls, d):
        st = cls()
        if d:
            st.mode, st.span, st.step, st.last_start, st.next = d["mode"], d["span"], d["step"], d["last_start"], d["next"]
            st.chrom_len, st.rec_len = len(d["chrom"]), len(d["rec_name"])
            st.chrom, st.rec_name = d["chrom"], d["rec_name"]
        return st


class ReadCounts(C.Structure):
    """wtamd_read_counts."""
    _fields_ = [(k, C.c_int64) for k in ("n_lines", "n_runs", "n_seg", "n_slow", "n_irregular", "first_irregular", "n_unsorted", "continues")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


def _read_door(data, flags=0, state=None, capacity=None, seg_capacity=None, slow_capacity=None, offset=0):
    """wtamd_text_runs over `data` (bytes), which is copied to byte `offset` of a device allocation.  Returns a dict: rc, counts,
    state (after, as a dict), and the whole of every output array as numpy (start, finish, value as uint64 bits, seg_off,
    seg_name_off, seg_name_len, slow_rec, slow_off), each `capacity` entries (seg_off: seg_capacity + 1) with 8 canary entries of
    READ_CANARY bytes on either side (key + "_lo" / "_hi" hold the guards' bytes).  A capacity None: the count a first call with
    no room reports.  counts start out as -1."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    fn = _lib.lib().wtamd_text_runs
    raw = np.frombuffer(bytes(data), np.uint8)
    text = torch.full((offset + len(raw) + 64,), READ_CANARY, dtype=torch.uint8, device=dev)
    if len(raw):
        text[offset:offset + len(raw)] = torch.from_numpy(raw.copy()).to(dev)
    if capacity is None or seg_capacity is None or slow_capacity is None:
        st, cn = ReadState.from_dict(state), ReadCounts()
        fn(text.data_ptr() + offset, len(raw), int(flags), C.addressof(st), None, None, None, 0, None, None, None, 0, None, None, 0, C.addressof(cn), None)
        capacity = max(int(cn.n_runs), 0) if capacity is None else capacity
        seg_capacity = max(int(cn.n_seg), 0) if seg_capacity is None else seg_capacity
        slow_capacity = max(int(cn.n_slow), 0) if slow_capacity is None else slow_capacity
    G = 8
    sizes = {"start": (capacity, torch.int32), "finish": (capacity, torch.int32), "value": (capacity, torch.int64), "seg_off": (seg_capacity + 1, torch.int64),
             "seg_name_off": (seg_capacity, torch.int64), "seg_name_len": (seg_capacity, torch.int32), "slow_rec": (slow_capacity, torch.int64),
             "slow_off": (slow_capacity, torch.int64)}
    bufs = {k: torch.full(((n + 2 * G) * dt.itemsize,), READ_CANARY, dtype=torch.uint8, device=dev).view(dt) for k, (n, dt) in sizes.items()}
    ptr = lambda k: bufs[k].data_ptr() + G * sizes[k][1].itemsize      # noqa: E731
    st, cn = ReadState.from_dict(state), ReadCounts(*([-1] * 8))
    rc = fn(text.data_ptr() + offset, len(raw), int(flags), C.addressof(st), ptr("start"), ptr("finish"), ptr("value"), int(capacity), ptr("seg_off"),
            ptr("seg_name_off"), ptr("seg_name_len"), int(seg_capacity), ptr("slow_rec"), ptr("slow_off"), int(slow_capacity), C.addressof(cn), None)
    out = {"rc": rc, "counts": cn.as_dict(), "state": st.as_dict()}
    for k, (n, dt) in sizes.items():
        a = bufs[k].cpu().numpy()
        out[k] = a[G:G + n].view(np.uint64) if k == "value" else a[G:G + n]
        out[k + "_lo"], out[k + "_hi"] = a[:G].view(np.uint8), a[G + n:].view(np.uint8)
    out["text_guard"] = text[offset + len(raw):].cpu().numpy()
    return out


def read_text(data: bytes, bed=False) -> RunLists:
    """The reference's WiggleReader (wig fixedStep / variableStep and bedGraph; bed=True: BedReader, value 1) over the bytes of
    a whole file on the device (wtamd_text_runs_host): one track, a chromosome per distinct name in order of first appearance
    (a file that comes back to a chromosome is refused, as a RunLists cannot hold it), f64 values bit for bit strtod's.
    The list is as the lines give it: the reference's reader compresses behind itself (wtamd_runs_compress does that).
    Irregular text (include/wiggletools_amd.h) raises WtamdError."""
    data = bytes(data)
    flags = (READ_BED if bed else 0) | (READ_EOF if data and not data.endswith(b"\n") else 0)
    fn = _lib.lib().wtamd_text_runs_host
    st, cn = ReadState(), ReadCounts()
    n = data.count(b"\n") + 1
    s, f, v = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float64)
    seg, noff, nlen = np.zeros(n + 1, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int32)
    names = C.create_string_buffer(max(len(data), 1) + 257 * 2)
    _lib.check(fn(data, len(data), flags, C.addressof(st), s.ctypes.data, f.ctypes.data, v.ctypes.data, n, seg.ctypes.data, noff.ctypes.data,
                  nlen.ctypes.data, n, C.addressof(names), len(names), C.addressof(cn)))
    m, g = int(cn.n_runs), int(cn.n_seg)
    chrom, p = [], 0
    for k in range(g):
        chrom.append(names.raw[p:p + int(nlen[k])].decode("latin-1"))
        p += int(nlen[k]) + 1
    if len(set(chrom)) != len(chrom):
        raise _lib.WtamdError("read_text: the text comes back to a chromosome it has left")
    return RunLists(g, 1, np.concatenate([seg[:g], [m]]).astype(np.int64), s[:m].copy(), f[:m].copy(), v[:m].copy(), [0.0], chrom)


class TrackSet:
    """N tracks resident in HBM (wtamd_trackset)."""

    def __init__(self, handle, n_chrom, n_tracks, keep=None):
        self._h = handle
        self.n_chrom = n_chrom
        self.n_tracks = n_tracks
        self._keep = keep

    @staticmethod
    def _ranges(ranges, n_chrom):
        """ranges: None or per-chromosome (lo, hi) run-start bounds -> two int32 arrays (or None, None)."""
        if ranges is None:
            return None, None
        assert len(ranges) == n_chrom
        lo = np.ascontiguousarray([r[0] for r in ranges], np.int32)
        hi = np.ascontiguousarray([r[1] for r in ranges], np.int32)
        return lo, hi

    @classmethod
    def from_runlists(cls, rl: RunLists, ranges=None):
        L = _lib.lib()
        value = np.ascontiguousarray(rl.value)
        rlo, rhi = cls._ranges(ranges, rl.n_chrom)
        t = _lib.Tracks(rl.n_chrom, rl.n_tracks, rl.seg_off.ctypes.data, rl.start.ctypes.data,
                        rl.finish.ctypes.data, value.ctypes.data, int(value.dtype == np.float64),
                        rl.defaults.ctypes.data, rlo.ctypes.data if rlo is not None else None,
                        rhi.ctypes.data if rhi is not None else None)
        h = C.c_void_p()
        _lib.check(L.wtamd_trackset_create_host(C.byref(t), C.byref(h)))
        return cls(h, rl.n_chrom, rl.n_tracks)

    @classmethod
    def from_device(cls, n_chrom, n_tracks, seg_off, start, finish, value, defaults, ranges=None):
        """start/finish/value: torch CUDA tensors (int32,int32,float32|float64), kept alive by this object.
        seg_off / defaults: host numpy arrays."""
        import torch
        L = _lib.lib()
        assert start.is_cuda and finish.is_cuda and value.is_cuda
        assert start.dtype == torch.int32 and finish.dtype == torch.int32
        assert value.dtype in (torch.float32, torch.float64)
        seg_off = np.ascontiguousarray(seg_off, np.int64)
        defaults = np.ascontiguousarray(defaults, np.float64)
        rlo, rhi = cls._ranges(ranges, n_chrom)
        t = _lib.Tracks(n_chrom, n_tracks, seg_off.ctypes.data, start.data_ptr(), finish.data_ptr(),
                        value.data_ptr(), int(value.dtype == torch.float64), defaults.ctypes.data,
                        rlo.ctypes.data if rlo is not None else None, rhi.ctypes.data if rhi is not None else None)
        h = C.c_void_p()
        _lib.check(L.wtamd_trackset_create_device(C.byref(t), C.byref(h)))
        return cls(h, n_chrom, n_tracks, keep=(start, finish, value))

    def close(self):
        if self._h is not None:
            _lib.lib().wtamd_trackset_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def max_runs(self):
        return int(_lib.lib().wtamd_trackset_max_runs(self._h))

    def index(self, op="mean", stream=None):
        _lib.check(_lib.lib().wtamd_trackset_index(self._h, opcode(op), stream))

    def stats(self):
        s = _lib.Stats()
        _lib.check(_lib.lib().wtamd_get_stats(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in _lib.Stats._fields_}

    def validate(self):
        """(number of runs violating the input contract, global index of the first or -1)."""
        n, first = C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().wtamd_trackset_validate(self._h, C.byref(n), C.byref(first)))
        return n.value, first.value

    def pearson(self):
        """Pearson correlation of the set's two tracks (reference `pearson a b`), computed on device."""
        out = C.c_double()
        _lib.check(_lib.lib().wtamd_pearson(self._h, C.byref(out)))
        return out.value

    def pearson_moments(self):
        """{n, sum_X, sum_Y, T_XX, T_XY, T_YY} of this track set's part of the genome (6 doubles)."""
        m = np.zeros(6, np.float64)
        _lib.check(_lib.lib().wtamd_pearson_moments(self._h, m.ctypes.data))
        return m

    # ---- host-output convenience (tests, drop-in layer) ----
    def reduce_host(self, op, flags=0, n_set0=0):
        """Returns (chrom, start, finish, value) numpy arrays."""
        cap = max(self.max_runs(), 1)
        s, f, v = np.empty(cap, np.int32), np.empty(cap, np.int32), np.empty(cap, np.float64)
        cro = np.zeros(self.n_chrom + 1, np.int64)
        runs = _lib.Runs(cap, s.ctypes.data, f.ctypes.data, v.ctypes.data, cro.ctypes.data)
        desc = _lib.ReduceDesc(opcode(op), flags, n_set0, 0)
        n = C.c_int64()
        _lib.check(_lib.lib().wtamd_reduce_host(self._h, C.byref(desc), C.byref(runs), C.byref(n)))
        n = n.value
        chrom = np.repeat(np.arange(self.n_chrom, dtype=np.int32), np.diff(cro))
        assert len(chrom) == n
        return chrom, s[:n].copy(), f[:n].copy(), v[:n].copy()

    def multiplex_host(self, flags=0):
        """Returns (chrom, start, finish, values[R,N], inplay[R,N])."""
        cap = max(self.max_runs(), 1)
        N = self.n_tracks
        s, f = np.empty(cap, np.int32), np.empty(cap, np.int32)
        cnt = np.empty(cap, np.float64)      # per-run inplay_count (multiplexer.h:27)
        cro = np.zeros(self.n_chrom + 1, np.int64)
        tile = np.empty((cap, N), np.float64)
        ip = np.empty((cap, N), np.uint8)
        runs = _lib.Runs(cap, s.ctypes.data, f.ctypes.data, cnt.ctypes.data, cro.ctypes.data)
        n = C.c_int64()
        _lib.check(_lib.lib().wtamd_multiplex_host(self._h, flags, C.byref(runs), tile.ctypes.data, ip.ctypes.data,
                                                   C.byref(n)))
        n = n.value
        chrom = np.repeat(np.arange(self.n_chrom, dtype=np.int32), np.diff(cro))
        return chrom, s[:n].copy(), f[:n].copy(), tile[:n].copy(), ip[:n].copy()

    def mtext(self, chrom_names, bedgraph=False, strict=False, state=None):
        """The file `mwrite` / `mwrite_bg` would write for this track set (wtamd_trackset_mtext_host): the tile is materialised
        and printed on the device, only the text comes home.  state: a TextState to chain pieces of a genome, or None."""
        names = [n.encode() if isinstance(n, str) else n for n in chrom_names]
        assert len(names) == self.n_chrom
        arr = (C.c_char_p * max(len(names), 1))(*names)
        flags = (MTEXT_BEDGRAPH if bedgraph else 0) | (MTEXT_STRICT if strict else 0)
        fn = _lib.lib().wtamd_trackset_mtext_host
        nb, nw, nr = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        sp = C.byref(state) if state is not None else None
        rc = fn(self._h, arr, flags, sp, None, 0, C.byref(nb), C.byref(nw), C.byref(nr))
        if rc == 3:                             # WTAMD_ERR_CAPACITY: nb holds the size
            buf = np.empty(nb.value, np.uint8)
            rc = fn(self._h, arr, flags, sp, buf.ctypes.data, len(buf), C.byref(nb), C.byref(nw), C.byref(nr))
            _lib.check(rc)
            return buf[:nb.value].tobytes()
        _lib.check(rc)
        return b""

    # ---- device-resident path (bench, pipelines) ----
    def alloc_runs(self, capacity=None):
        import torch
        cap = max(int(capacity if capacity is not None else self.max_runs()), 1)
        dev = torch.device("cuda", torch.cuda.current_device())
        return DeviceRuns(torch.empty(cap, dtype=torch.int32, device=dev),
                          torch.empty(cap, dtype=torch.int32, device=dev),
                          torch.empty(cap, dtype=torch.float64, device=dev),
                          torch.zeros(self.n_chrom + 1, dtype=torch.int64, device=dev))

    def reduce(self, op, out, flags=0, n_set0=0, stream=None, sync=True):
        """Multiplex+reduce on device into `out` (DeviceRuns). Returns run count when sync."""
        desc = _lib.ReduceDesc(opcode(op), flags, n_set0, 0)
        runs = out.as_struct()
        n = C.c_int64(-1)
        _lib.check(_lib.lib().wtamd_reduce(self._h, C.byref(desc), C.byref(runs),
                                           C.byref(n) if sync else None, stream))
        if sync:
            out.n = n.value
            return n.value
        return None


class DeviceRuns:
    def __init__(self, start, finish, value, chrom_run_off):
        self.start, self.finish, self.value, self.chrom_run_off = start, finish, value, chrom_run_off
        self.n = 0

    def as_struct(self):
        return _lib.Runs(self.start.numel(), self.start.data_ptr(), self.finish.data_ptr(),
                         self.value.data_ptr(), self.chrom_run_off.data_ptr())

    def auc(self, n=None, stream=None):
        r = self.as_struct()
        out = C.c_double()
        _lib.check(_lib.lib().wtamd_runs_auc(C.byref(r), int(self.n if n is None else n), C.byref(out), stream))
        return out.value

    def mean(self, n=None, stream=None):
        """meanI of the run list (reference MeanIntegrator): length-weighted mean of the non-NaN runs."""
        r = self.as_struct()
        out = C.c_double()
        _lib.check(_lib.lib().wtamd_runs_mean(C.byref(r), int(self.n if n is None else n), C.byref(out), stream))
        return out.value

    def moments(self, n=None, stream=None):
        """{sum L v, span, T = sum L (v - mean)^2, min, max, 0} over the non-NaN runs, one pass on the device
        (wtamd_runs_moments): everything varI / stddevI / CVI / maxI / minI need; shards merge theirs in genome order with
        shard.merge_run_moments."""
        r = self.as_struct()
        m = np.zeros(6, np.float64)
        _lib.check(_lib.lib().wtamd_runs_moments(C.byref(r), int(self.n if n is None else n), m.ctypes.data, stream))
        return m

    def _stat(self, kind, n, stream):
        m = self.moments(n, stream)
        return _lib.lib().wtamd_moments_finish(m.ctypes.data, STATS[kind])

    def var(self, n=None, stream=None):
        """varI of the run list (reference VarianceIntegrator): T / (span - 1)."""
        return self._stat("var", n, stream)

    def stddev(self, n=None, stream=None):
        return self._stat("stddev", n, stream)

    def cv(self, n=None, stream=None):
        return self._stat("cv", n, stream)

    def max(self, n=None, stream=None):
        """maxI (reference MaxIntegrator): NaN for a list without a non-NaN run."""
        return self._stat("max", n, stream)

    def min(self, n=None, stream=None):
        return self._stat("min", n, stream)

    def span(self, n=None, stream=None):
        """Base pairs under the non-NaN runs (reference SpanIntegrator)."""
        return self._stat("span", n, stream)

    def compress(self, out=None, n=None, stream=None):
        """Merged run list (reference CompressionWiggleIterator) as a new DeviceRuns."""
        import torch
        n = int(self.n if n is None else n)
        if out is None:
            cap = max(n, 1)
            dev = self.start.device
            out = DeviceRuns(torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev),
                             torch.empty(cap, dtype=torch.float64, device=dev), torch.zeros_like(self.chrom_run_off))
        a, b = self.as_struct(), out.as_struct()
        m = C.c_int64()
        _lib.check(_lib.lib().wtamd_runs_compress(C.byref(a), n, self.chrom_run_off.numel() - 1, C.byref(b), C.byref(m),
                                                  stream))
        out.n = m.value
        return out

    def to_host(self):
        n = self.n
        cro = self.chrom_run_off.cpu().numpy()
        chrom = np.repeat(np.arange(len(cro) - 1, dtype=np.int32), np.diff(cro))
        return chrom, self.start[:n].cpu().numpy(), self.finish[:n].cpu().numpy(), self.value[:n].cpu().numpy()
