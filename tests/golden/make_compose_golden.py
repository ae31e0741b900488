#!/usr/bin/env python
"""Generates tests/golden/compose_fixtures.json: the VERBATIM output of the compiled reference's operator iterators STACKED --
SmoothWiggleIterator under BinningWiggleIterator and the other way round, either under OverlapWiggleIterator,
NoverlapWiggleIterator and TrimWiggleIterator, NearestWiggleIterator with distances beyond 2^24, ScaleWiggleIterator, and
SumReduction / MeanReduction of such stacks -- pop by pop: the pin that the reference hands doubles down a stack.

The driver is our own: the array-backed child iterator of make_apply_golden.py and an evaluator of the postfix programs of
tests/compose_dropin.py (STACKS) that builds the reference's iterators and pops the top one to its end.  It is compiled
together with the reference's sources, unmodified and from where they lie, into a shared object in a temporary directory.
Nothing compiled is kept.

The lists (compose_dropin.golden_lists): 1 and 3 chromosomes of at most 120 positions, the last of three shorter than the
window widths; values k / 8 with 2^23 <= k < 2^24, so that the smoothed values are dyadic rationals of more than 24 bits -- exact in
binary, whatever the order of the reference's additions, and not in float32.  The generator asserts that the composed Python
models (compose_dropin.model_stack: window_model, region_model and the oracle's reducers) reproduce every recorded value bit
for bit, and that more than half of the recorded values are not float32-exact.

Run where the reference's sources are present:  python tests/golden/make_compose_golden.py <path to the reference>
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
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import compose_dropin as X  # noqa: E402
import make_apply_golden as AG  # noqa: E402
from make_coverage_golden import REF_SRCS  # noqa: E402

OPCODES = {"src": 0, "mask": 1, "smooth": 2, "bin": 3, "scale": 4, "overlaps": 5, "noverlaps": 6, "trim": 7, "nearest": 8, "sum": 9, "mean": 10}

DRIVER = AG.DRIVER + r'''
/* lists 0 .. n_lists - 1: tracks and masks alike, every one over all the chromosomes; the program: op, iarg, darg per step */
long long golden_compose(int n_chrom, char **names, long long **seg_off, int **start, int **finish, double **value,
                         int n_steps, int *op, int *iarg, double *darg, long long cap, int *o_chrom, int *o_start, int *o_finish, double *o_value) {
    WiggleIterator *st[16];
    int top = 0;
    for (int k = 0; k < n_steps; k++) {
        int a = iarg[k];
        switch (op[k]) {
        case 0: case 1:
            st[top++] = arr_new(n_chrom, names, seg_off[a], start[a], finish[a], value[a], 0);
            st[top - 1]->overlaps = op[k] == 1;        /* a mask is a BED reader: it may overlap itself */
            break;
        case 2: st[top - 1] = SmoothWiggleIterator(st[top - 1], a); break;
        case 3: st[top - 1] = BinningWiggleIterator(st[top - 1], a); break;
        case 4: st[top - 1] = ScaleWiggleIterator(st[top - 1], darg[k]); break;
        case 5: top--; st[top - 1] = OverlapWiggleIterator(st[top - 1], st[top]); break;
        case 6: top--; st[top - 1] = NoverlapWiggleIterator(st[top - 1], st[top]); break;
        case 7: top--; st[top - 1] = TrimWiggleIterator(st[top - 1], st[top]); break;
        case 8: top--; st[top - 1] = NearestWiggleIterator(st[top - 1], st[top]); break;
        default: {
            WiggleIterator **kids = (WiggleIterator **) calloc(a, sizeof(WiggleIterator *));
            for (int q = 0; q < a; q++) kids[q] = st[top - a + q];
            top -= a;
            Multiplexer *m = newMultiplexer(kids, a, false);
            st[top++] = op[k] == 9 ? SumReduction(m) : MeanReduction(m);
        }
        }
    }
    WiggleIterator *wi = st[0];
    long long n = 0;
    while (!wi->done) {
        if (n < cap) {
            int c = 0;
            while (c < n_chrom && strcmp(names[c], wi->chrom)) c++;
            o_chrom[n] = c; o_start[n] = wi->start; o_finish[n] = wi->finish; o_value[n] = wi->value;
        }
        n++;
        pop(wi);
    }
    return n;
}
'''


def build(ref, tmp):
    drv = os.path.join(tmp, "driver.c")
    open(drv, "w").write(DRIVER)
    so = os.path.join(tmp, "libcomposegold.so")
    subprocess.check_call(["gcc", "-g", "-w", "-O3", "-std=gnu99", "-fPIC", "-shared", "-I" + os.path.join(ref, "src")] +
                          [os.path.join(ref, "src", s) for s in REF_SRCS] + [drv, "-o", so, "-lm", "-lpthread"])
    return C.CDLL(so, mode=os.RTLD_LAZY)


def run(L, names, tracks, masks, prog):
    """The program over the lists (a mask's number follows the tracks'): [(chromosome, start, finish, value)]."""
    lists = [X._flat(t) for t in tracks] + [X._flat([(s, f, np.ones(len(s))) for s, f in m]) for m in masks]
    keep = [[np.ascontiguousarray(a, dt) for a, dt in zip(x, (np.int64, np.int32, np.int32, np.float64))] for x in lists]
    ptrs = [(C.c_void_p * len(keep))(*[k[q].ctypes.data for k in keep]) for q in range(4)]
    arr = (C.c_char_p * len(names))(*[x.encode() for x in names])
    ops = np.array([OPCODES[o] for o, _ in prog], np.int32)
    ia = np.array([(a + len(tracks) if o == "mask" else 0 if o == "scale" else a) for o, a in prog], np.int32)
    da = np.array([a if o == "scale" else 0.0 for o, a in prog], np.float64)
    cap = 1 << 16
    oc, os_, of, ov = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.float64)
    p = lambda x: C.c_void_p(x.ctypes.data)      # noqa: E731
    L.golden_compose.restype = C.c_longlong
    n = L.golden_compose(C.c_int(len(names)), arr, ptrs[0], ptrs[1], ptrs[2], ptrs[3], C.c_int(len(prog)), p(ops), p(ia), p(da),
                         C.c_longlong(cap), p(oc), p(os_), p(of), p(ov))
    assert 0 < n <= cap, (n, cap)
    return [(int(c), int(a), int(b), float(x)) for c, a, b, x in zip(oc[:n], os_[:n], of[:n], ov[:n])]


def main():
    ref = sys.argv[1]
    from oracle import oracle
    oracle.build()
    out = {"generator": "tests/golden/make_compose_golden.py",
           "source": "compiled reference v1.2.11: its operator iterators and reducers stacked over array-backed children, every pop",
           "cases": []}
    n_rows = n_inexact = 0
    with tempfile.TemporaryDirectory() as tmp:
        L = build(ref, tmp)
        for length, n_chrom in ((120, 1), (90, 3)):
            names, tracks, masks = X.golden_lists(length, n_chrom)
            rec = {"name": "len%d_chroms%d" % (length, n_chrom), "chrom_names": names,
                   "tracks": [[[s.tolist(), f.tolist(), v.tolist()] for s, f, v in t] for t in tracks],
                   "masks": [[[s.tolist(), f.tolist()] for s, f in m] for m in masks], "stacks": {}}
            for name, prog in X.STACKS.items():
                rows = run(L, names, tracks, masks, prog)
                assert all(np.isfinite(r[3]) for r in rows), name
                model = X.model_stack(prog, names, tracks, masks, oracle)
                assert X.bits([(names[r[0]],) + r[1:] for r in rows]) == X.bits(model), (rec["name"], name)
                v = np.array([r[3] for r in rows])
                n_rows += len(v)
                n_inexact += int((v.astype(np.float32).astype(np.float64) != v).sum())
                rec["stacks"][name] = {"program": prog, "rows": [list(r) for r in rows]}
            back = X.fixture_lists(json.loads(json.dumps(rec)))
            assert all(np.array_equal(a, b) for t, u in zip(back[1], tracks) for x, y in zip(t, u) for a, b in zip(x, y))
            out["cases"].append(rec)
    assert 2 * n_inexact >= n_rows, (n_inexact, n_rows)
    path = os.path.join(HERE, "compose_fixtures.json")
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
    size = os.path.getsize(path)
    print("wrote %d cases, %d recorded values all equal to the composed models bit for bit, %d of them not float32-exact, %d bytes" %
          (len(out["cases"]), n_rows, n_inexact, size))
    assert size < 200000, size


if __name__ == "__main__":
    main()
