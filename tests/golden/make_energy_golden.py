#!/usr/bin/env python
"""Generates tests/golden/energy_fixtures.json: small run lists, the VERBATIM real, im and res of the compiled reference's
EnergyIntegrator (src/statistics.c:345-391; `energy`) over them, and the exact value of the closed form (energy_model.exact:
mpmath at 60 digits, rounded once) -- and tests/golden/energy_seams.json, the exact values of energy_model.seam_cases().

The driver is our own: the array-backed child iterator of make_apply_golden.py and a function that builds the integrator, pops
it to its end (in some cases seeking in the middle) and copies the three doubles out through a view of the reference's
EnergyData.  It is compiled together with the reference's sources, unmodified and from where they lie, into a shared object in a
temporary directory.  Nothing compiled is kept.

Cases: 1-3 chromosomes, in some cases one of them empty; at most 40 runs; values alternately multiples of 1/8 and full-mantissa
doubles; one case with a NaN; an overlapping child in one case of three (the reference's union runs); a seek in the middle in
another third; run lengths that are multiples of the wavelengths, and of 1.  Wavelengths 1, 2, 3, 7, 10, 147, 200, 1000 and
300007, larger than every position.  For every recorded value, none left out, the generator asserts
    |reference - exact| <= 2^-53 S (16 P / lam + B + 8)
with P the largest |position| (offset included), B the base pairs and S = sum |v| L (ISSUE / DESIGN.md: the reference's argument
-2 p PI / lam carries about 2.5 roundings of 2^-53 2 pi P / lam, its running sums B additions).

Run where the reference's sources are present:  python tests/golden/make_energy_golden.py <path to the reference>
"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import energy_model as M  # noqa: E402
import make_apply_golden as AG  # noqa: E402
from make_coverage_golden import REF_SRCS  # noqa: E402

WAVELENGTHS = [1, 2, 3, 7, 10, 147, 200, 1000, 300007]
NAMES = ["chr1", "chr2", "chr3"]

DRIVER = AG.DRIVER + r'''
/* what statistics.c keeps behind the integrator's data */
typedef struct { double res; double real; double im; int wavelength; int chrom_offset; WiggleIterator *source; } EnergyView;

/* pre >= 0: pop `pre` times, seek, then pop to the end; pre < 0: pop to the end.  out: real, im, res, res before the end. */
void golden_energy(int n_chrom, char **names, long long *seg_off, int *start, int *finish, double *value, int overlaps, int wavelength,
                   int pre, const char *chrom, int a, int b, double *out) {
    WiggleIterator *child = arr_new(n_chrom, names, seg_off, start, finish, value, 0);
    child->overlaps = overlaps;
    WiggleIterator *wi = EnergyIntegrator(child, wavelength);
    out[3] = *(double *) wi->data;
    if (pre >= 0) {
        for (int i = 0; i < pre; i++) pop(wi);
        seek(wi, chrom, a, b);
    }
    while (!wi->done) pop(wi);
    EnergyView *e = (EnergyView *) wi->data;
    out[0] = e->real; out[1] = e->im; out[2] = e->res;
}
'''


def build(ref, tmp):
    drv = os.path.join(tmp, "driver.c")
    open(drv, "w").write(DRIVER)
    so = os.path.join(tmp, "libenergygold.so")
    subprocess.check_call(["gcc", "-g", "-w", "-O3", "-std=gnu99", "-D_GNU_SOURCE", "-fPIC", "-shared", "-I" + os.path.join(ref, "src")] +
                          [os.path.join(ref, "src", s) for s in REF_SRCS] + [drv, "-o", so, "-lm", "-lpthread"])
    return C.CDLL(so, mode=os.RTLD_LAZY)


def run(L, names, lists, overlaps, lam, seek):
    p = lambda x: C.c_void_p(x.ctypes.data)      # noqa: E731
    arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
    out = np.zeros(4)
    L.golden_energy.restype = None
    pre, chrom, a, b = (seek["pre"], seek["chrom"].encode(), seek["start"], seek["finish"]) if seek else (-1, b"", 0, 0)
    L.golden_energy(C.c_int(len(names)), arr, p(lists.seg), p(lists.s), p(lists.f), p(lists.v), C.c_int(int(overlaps)), C.c_int(lam),
                    C.c_int(pre), C.c_char_p(chrom), C.c_int(a), C.c_int(b), p(out))
    return out


def make_case(rng, k):
    n_chrom = 1 + k % 3
    overlaps = k % 3 == 2
    eighths = k % 2 == 0
    lengths = np.array([1, 1, 2, 3, 7, 10, 14, 20, 147, 200, 294, 33, 61])
    segs, left = [], 40
    for c in range(n_chrom):
        n = int(rng.integers(2, max(3, left // (n_chrom - c)) + 1))
        left -= n
        ln = lengths[rng.integers(0, len(lengths), n)]
        if overlaps:                                        # sorted by start only
            s = np.sort(rng.integers(1, 20000, n))
            s[1::3] = s[0::3][:len(s[1::3])] + 1            # (some pairs do overlap)
            s = np.sort(s)
        else:
            s = 1 + np.cumsum(rng.integers(0, 900, n) + np.concatenate([[0], ln[:-1]]))
        v = rng.integers(-80, 81, n) / 8.0 if eighths else rng.uniform(-10, 10, n)
        segs.append([s.astype(np.int32), (s + ln).astype(np.int32), v])
    if n_chrom > 1 and k % 4 == 1:                          # an empty chromosome, in the middle where there is one
        segs[1 if n_chrom == 3 else 0] = [np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0)]
    if k == 6:
        segs[-1][2][1] = np.nan
    seek = None
    full = [c for c in range(n_chrom) if len(segs[c][0])]
    if k % 3 == 1 and len(full) >= 2 and len(segs[full[0]][0]) >= 3:
        c = full[-1]
        n = len(segs[c][0])
        i = int(rng.integers(0, n))
        j = int(rng.integers(i, n))
        # (the pops before the seek end with the first chromosome: the drop-in, which serves a chromosome per pop, can do the same)
        seek = {"pre": len(segs[full[0]][0]) - 1, "chrom": NAMES[c], "start": int(segs[c][0][i]), "finish": int(segs[c][1][j])}
    return segs, overlaps, seek


def main():
    ref = sys.argv[1]
    rng = np.random.default_rng(20261203)
    out = {"generator": "tests/golden/make_energy_golden.py",
           "source": "compiled reference v1.2.11: EnergyIntegrator over an array-backed child, real / im / res through a view of EnergyData; "
                     "exact: the closed form by mpmath at 60 digits",
           "cases": []}
    seen = {"overlaps": 0, "seek": 0, "nan": 0, "empty_chrom": 0, "three": 0, "zero": 0}
    worst = 0.0
    with tempfile.TemporaryDirectory() as tmp:
        L = build(ref, tmp)
        for k in range(30):
            segs, overlaps, seek = make_case(rng, k)
            names = NAMES[:len(segs)]
            child = M.Lists.from_segments(segs)
            case = {"name": "case%03d" % k, "overlaps": bool(overlaps), "wavelengths": WAVELENGTHS, "seek": seek,
                    "chroms": [{"name": n, "start": r[0].tolist(), "finish": r[1].tolist(), "value": [M._hex(x) for x in r[2].tolist()]}
                               for n, r in zip(names, segs)]}
            lists = M.fixture_lists(case)
            assert len(lists.s) <= 40
            star = M.exact(lists, WAVELENGTHS)
            base, _ = M.bases(lists)
            P = max([abs(base[g] + int(x)) for g in range(lists.n_seg) for x in list(lists.s[lists.seg[g]:lists.seg[g + 1]]) + list(lists.f[lists.seg[g]:lists.seg[g + 1]])] + [0])
            B = int((lists.f.astype(np.int64) - lists.s).sum())
            assert P <= 2 ** 17 and B <= 2 * 10 ** 4, (k, P, B)
            S = M.weight(lists)
            recorded = []
            for w, lam in enumerate(WAVELENGTHS):
                got = run(L, names, child, overlaps, lam, seek)
                assert got[3] != got[3], "res is NaN before the end"
                if np.isnan(star[w]).any():
                    assert np.isnan(got[:3]).all(), (k, lam, got)
                else:
                    bound = 2.0 ** -53 * S * (16.0 * P / lam + B + 8)
                    err = np.abs(got[:2] - star[w]).max()
                    assert err <= bound, (k, lam, got, star[w], err, bound)
                    worst = max(worst, err / bound)
                    assert got[2] == got[0] * got[0] + got[1] * got[1]
                    seen["zero"] += int((star[w] == 0).any())
                recorded.append([M._hex(x) for x in got[:3]])
            case["reference"] = recorded
            case["exact"] = [[M._hex(x) for x in row] for row in star]
            case["S"] = S.hex()
            out["cases"].append(case)
            seen["overlaps"] += int(overlaps)
            seen["seek"] += int(seek is not None)
            seen["nan"] += int(np.isnan(child.v).any())
            seen["empty_chrom"] += int(any(len(r[0]) == 0 for r in segs))
            seen["three"] += int(len(segs) == 3)
    assert min(seen.values()) >= 1, seen
    path = os.path.join(HERE, "energy_fixtures.json")
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
    print("wrote %d cases, every reference value inside its bound (worst %.3f of it), %r, %d bytes" % (len(out["cases"]), worst, seen, os.path.getsize(path)))
    assert os.path.getsize(path) < 400000
    seams = {"generator": "tests/golden/make_energy_golden.py", "source": "energy_model.exact over energy_model.seam_cases()", "cases": {}}
    for name, (lists, lam, sb) in sorted(M.seam_cases().items()):
        star = M.exact(lists, lam, sb)
        S = M.weight(lists)
        seams["cases"][name] = {"n": len(lists.s), "S": None if S != S or S == float("inf") else S.hex(), "exact": [[M._hex(x) for x in row] for row in star],
                                "end_base": M.bases(lists, sb)[1]}
        print(name, len(lists.s), len(lam), flush=True)
    path = os.path.join(HERE, "energy_seams.json")
    with open(path, "w") as fh:
        json.dump(seams, fh, separators=(",", ":"))
    print("wrote %d seam cases, %d bytes" % (len(seams["cases"]), os.path.getsize(path)))


if __name__ == "__main__":
    main()
