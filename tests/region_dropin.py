"""What tests/test_region_model.py (the emulated drop-in library) and tests/test_region_gpu.py (the product) share: the recorded
fixtures as arrays, and a ctypes driver of wtamd_RegionIterator that builds the iterators over NumPy arrays and reads them the
ways the layer offers -- pop(), wtamd_iterator_next_block, after seek(), and as children of newMultiplexer + MeanReduction."""
import ctypes as C
import json
import os

import numpy as np

import cover_dropin
import region_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
_fixtures = None


def load_fixtures():
    global _fixtures
    if _fixtures is None:
        with open(os.path.join(HERE, "golden", "region_fixtures.json")) as fh:
            _fixtures = json.load(fh)["cases"]
    return _fixtures


def _segments(side, n_seg):
    """One segment per chromosome of the case; a chromosome the side does not have is an empty one."""
    seg = np.zeros(n_seg + 1, np.int64)
    for k, c in enumerate(side["chroms"]):
        seg[c + 1] = side["seg_off"][k + 1] - side["seg_off"][k]
    return np.cumsum(seg)


def case_arrays(c):
    """(seg_off, start, finish, value, m_seg_off, m_start, m_finish) of a recorded case."""
    n_seg = len(c["chrom_names"])
    a, m = c["source"], c["mask"]
    return (_segments(a, n_seg), np.array(a["start"], np.int32), np.array(a["finish"], np.int32), np.array(a["value"], np.float64),
            _segments(m, n_seg), np.array(m["start"], np.int32), np.array(m["finish"], np.int32))


def recorded_values(rec):
    return np.array([np.nan if x is None else x for x in rec["value"]], np.float64)


def all_in_one(cases, op):
    """Every case that records `op`, one after the other, as one call."""
    arrs = [case_arrays(c) for c in cases if op in c]
    off = lambda k: np.concatenate([[0], np.cumsum(np.concatenate([np.diff(a[k]) for a in arrs]))]).astype(np.int64)   # noqa: E731
    cat = lambda k: np.concatenate([a[k] for a in arrs])     # noqa: E731
    return off(0), cat(1), cat(2), cat(3), off(4), cat(5), cat(6)


def recorded_rows(c, key):
    rec = c[key]
    v = recorded_values(rec)
    return [(c["chrom_names"][ch], int(a), int(b), float(x)) for ch, a, b, x in zip(rec["chrom"], rec["start"], rec["finish"], v)]


def same_rows(a, b):
    return len(a) == len(b) and [r[:3] for r in a] == [r[:3] for r in b] and M.same_bits([r[3] for r in a], [r[3] for r in b])


class DropIn(cover_dropin.DropIn):
    def __init__(self, path):
        super().__init__(path)
        self.L.wtamd_RegionIterator.restype = C.c_void_p
        self.L.wtamd_RegionIterator.argtypes = [C.c_int, C.c_void_p, C.c_void_p]

    def region(self, op, source, mask):
        return self.L.wtamd_RegionIterator(M.OPS[op], source, mask)

    def side(self, c, which, overlapping):
        """The reader of a recorded case's source or mask: only the chromosomes that side has."""
        d = c[which]
        names = [c["chrom_names"][k] for k in d["chroms"]]
        v = np.array(d["value"], np.float32) if which == "source" else np.ones(len(d["start"]), np.float32)
        return self.reader(names, d["seg_off"], d["start"], d["finish"], v, overlapping=overlapping)

    def case_iter(self, c, op):
        src = self.side(c, "source", c["source"]["overlaps"])
        mask = self.side(c, "mask", True)
        return self.region(op, src, mask)


def expected_rows(op, names, seg, s, f, v, mseg, ms, mf, window=None):
    """The model as [(chrom, start, finish, value)]; window = (chrom, lo, hi): both sides cut down to that chromosome and to
    the intervals that intersect [lo, hi), clipped, as the readers' seek does."""
    rows = []
    for c, name in enumerate(names):
        a, b, ma, mb = int(seg[c]), int(seg[c + 1]), int(mseg[c]), int(mseg[c + 1])
        cs, cf, cv, cms, cmf = s[a:b], f[a:b], v[a:b], ms[ma:mb], mf[ma:mb]
        if window is not None:
            if name != window[0]:
                continue
            keep, mkeep = (cf > window[1]) & (cs < window[2]), (cmf > window[1]) & (cms < window[2])
            cs, cf, cv = np.maximum(cs[keep], window[1]), np.minimum(cf[keep], window[2]), cv[keep]
            cms, cmf = np.maximum(cms[mkeep], window[1]), np.minimum(cmf[mkeep], window[2])
        fn = M.trim_protocol if op == "trim" and M.overlaps_itself([0, len(cs)], cs, cf) else None
        r = fn(cs, cf, cv, cms, cmf) if fn else M.region(op, cs, cf, cv, cms, cmf)
        rows.extend((name, int(x), int(y), float(z)) for x, y, z in zip(*r))
    return rows


def random_case(rng, names, n_max, span, overlapping_source):
    """(seg, s, f, v, mseg, ms, mf): a source (values exact in float32) and an overlapping mask over the same chromosomes."""
    import cover_model as CM
    src = [CM.random_segment(rng, int(rng.integers(0, n_max)), span, max(2, span // 20)) if overlapping_source else
           M.disjoint_segment(rng, int(rng.integers(0, n_max)), span) for _ in names]
    mask = [CM.random_segment(rng, int(rng.integers(0, n_max)), span, max(2, span // 15)) for _ in names]
    seg, s, f = M.flat(src)
    mseg, ms, mf = M.flat(mask)
    return seg, s, f, (rng.integers(-80, 80, len(s)) / 8.0).astype(np.float32), mseg, ms, mf


def check_dropin(D, oracle, fixtures, rng):
    """The checks both backends share."""
    from wiggletools_amd.runlists import RunLists
    ops = sorted(M.OPS, key=M.OPS.get)
    # the recorded cases: pop() against the recording itself, blocks against pop() -- chromosomes missing on either side,
    # and the trim of an overlapping source, which follows the reference's protocol
    n_protocol = 0
    for c in fixtures[::3] + [c for c in fixtures if "trim_overlapping_source" in c][:25]:
        for op in ops:
            key = op if op in c else "trim_overlapping_source"
            n_protocol += key != op
            exp = recorded_rows(c, key)
            assert same_rows(D.read_pops(D.case_iter(c, op)), exp), (c["name"], op)
            assert same_rows(D.read_blocks(D.case_iter(c, op)), exp), (c["name"], op)
    assert n_protocol >= 25
    names = ["chr1", "chr2", "chrX"]
    for n_max, span, overlapping in ((12, 60, False), (80, 600, True), (700, 9000, False)):
        case = random_case(rng, names, n_max, span, overlapping)
        seg, s, f, v, mseg, ms, mf = case

        def make(op):
            return D.region(op, D.reader(names, seg, s, f, v, overlapping=overlapping), D.reader(names, mseg, ms, mf, np.ones(len(ms), np.float32)))
        for op in ops:
            exp = expected_rows(op, names, *case)
            assert same_rows(D.read_pops(make(op)), exp), op
            assert same_rows(D.read_blocks(make(op)), exp), op
            assert same_rows(D.read_blocks(make(op), pops_between=2), exp), op
            wi = make(op)
            for (c, lo, hi) in (("chr2", 1 + span // 4, 1 + span // 2), ("chr1", 1, 3), ("chrX", span // 2, span + 50), ("nope", 1, 100)):
                D.seek(wi, c, lo, hi)
                assert same_rows(D.read_pops(wi), expected_rows(op, names, *case, window=(c, lo, hi))), (op, c, lo, hi)
            w = D.fields(make(op))
            assert w.overlaps == (b"\x01" if overlapping else b"\x00") and w.default_value == 0.0
        if overlapping:
            continue
        # Multiplexer children under MeanReduction against the oracle's `mean` over the model's lists (trim and overlaps of
        # the same source, and noverlaps of another: values k / 8, float32-exact, so the Multiplexer takes
        # the served lists in float32 blocks; tests/compose_dropin.py serves lists that are not)
        other = random_case(rng, names, n_max, span, False)
        kids = [("trim", case), ("overlaps", case), ("noverlaps", other)]
        lists = []
        for op, cs in kids:
            per_c = []
            for k in range(len(names)):
                a, b, ma, mb = int(cs[0][k]), int(cs[0][k + 1]), int(cs[4][k]), int(cs[4][k + 1])
                r = M.region(op, cs[1][a:b], cs[2][a:b], cs[3][a:b], cs[5][ma:mb], cs[6][ma:mb])
                per_c.append(list(zip(r[0].tolist(), r[1].tolist(), r[2].tolist())))
            lists.append(per_c)
        ec, es, ef, ev = oracle.reduce(RunLists.from_lists(lists).as_dict(), "mean")[:4]
        got = D.mean_of([D.region(op, D.reader(names, cs[0], cs[1], cs[2], cs[3], overlapping=False),
                                  D.reader(names, cs[4], cs[5], cs[6], np.ones(len(cs[5]), np.float32))) for op, cs in kids])
        assert [g[0] for g in got] == [names[c] for c in ec]
        assert np.array_equal([g[1] for g in got], es) and np.array_equal([g[2] for g in got], ef)
        assert M.same_bits([g[3] for g in got], ev)
