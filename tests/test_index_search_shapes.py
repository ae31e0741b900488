"""The searched window index (csrc/wt_isearch.h, wt_index_coarse_kernel / wt_index_search_kernel) at the shapes where its
strips, its 16-track groups and its interpolation can go wrong.  WTAMD_INDEX_CHECK=1 builds the index by the scan over every
finish[] as well and fails the reduction if one entry differs; the reduced runs are compared with the oracle.  The switch is
read once per process: one child runs all the cases."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, "tests")
from helpers import assert_runs_equal
from oracle import oracle as O
from wiggletools_amd import engine as E
from wiggletools_amd.runlists import RunLists, synth

O.build()
KINDS = ["uniform", "empty", "single", "clustered", "last_window", "on_boundaries"]


def window_bp(op, n):
    ts = E.TrackSet.from_runlists(synth(n, [3000], mean_run=16, seed=1))
    ts.reduce_host(op)
    w = ts.stats()["window_bp"]
    ts.close()
    return w


def track(kind, L, W, rng):
    """Runs (start, finish) of one track on a chromosome whose data spans [1, 1 + L): the window grid starts at 1."""
    if kind == "empty" or L <= 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    if kind == "uniform":
        ends = np.cumsum(rng.geometric(1 / 16.0, L // 8 + 16))
        ends = ends[ends < L]
        ends = np.concatenate([ends, [L]])
        return np.concatenate([[0], ends[:-1]]) + 1, ends + 1
    if kind == "single":
        return np.array([1]), np.array([1 + L])
    if kind == "clustered":         # 99 % of the runs in the first 1 % of the coordinates, then one far run
        k = max(L // 100, 2)
        s = np.arange(0, k - 1, 1)
        return np.concatenate([s, [L - 5]]) + 1, np.concatenate([s + 1, [L]]) + 1
    nw = (L + W - 1) // W
    if kind == "last_window":
        a = (nw - 1) * W + 2
        s = np.arange(a, L - 1, 3)
        return s + 1, s + 3
    if kind == "on_boundaries":     # every finish (and every start but the first) is a window boundary 1 + m W
        b = np.arange(1, nw) * W
        b = b[b < L]
        ends = np.concatenate([b, [L]])
        return np.concatenate([[0], ends[:-1]]) + 1, ends + 1
    raise ValueError(kind)


def case(kinds, lens, W, seed):
    rng = np.random.default_rng(seed)
    seg, S, F = [0], [], []
    for L in lens:
        for k in kinds:
            s, f = track(k, L, W, rng)
            S.append(s); F.append(f); seg.append(seg[-1] + len(s))
    s = np.concatenate(S).astype(np.int32); f = np.concatenate(F).astype(np.int32)
    v = (rng.integers(1, 800, len(s)) / 8.0).astype(np.float32)
    return RunLists(len(lens), len(kinds), seg, s, f, v)


n_cases = 0
for op in ("mean", "product"):
    for n in (1, 17, 33):
        W = window_bp(op, n)
        # rows = windows + 1 per chromosome: 70 rows (two strips of 64, the second partial); 100, an empty chromosome, 30
        # (a strip straddles a chromosome edge)
        shapes = {"one": [69 * W - 3], "three": [99 * W - 5, 0, 29 * W - 1]}
        for name, lens in shapes.items():
            sets = [[k] for k in KINDS] if n == 1 else [[KINDS[i % len(KINDS)] for i in range(n)]]
            for kinds in sets:
                rl = case(kinds, lens, W, 100 * n + len(lens))
                ts = E.TrackSet.from_runlists(rl)
                got = ts.reduce_host(op)
                st = ts.stats()
                ts.close()
                what = "%s, %d tracks (%s), %s" % (op, n, kinds[0] if n == 1 else "all kinds", name)
                assert st["window_bp"] == W, (what, st)
                assert st["kernel"] == (1 if op == "mean" else 0), (what, st)
                if n > 1 or kinds[0] in ("uniform", "single", "on_boundaries"):
                    assert st["n_windows"] == (69 if name == "one" else 99 + 1 + 29), (what, st)
                assert_runs_equal(got, O.reduce(rl.as_dict(), op), 0.0, what)       # (both reducers are bit-exact against the oracle)
                n_cases += 1
print("index-shapes-ok %d" % n_cases)
'''


def test_gpu_index_search_shapes():
    """70 rows on one chromosome; 100 + an empty chromosome + 30 rows; 1, 17 and 33 tracks; uniform, empty, single-run,
    clustered, last-window-only and on-boundary tracks; `mean` on the difference-array width (WTAMD_DELTA_MIN_TRACKS=1) and
    `product` on the general width -- searched index == scanned index (WTAMD_INDEX_CHECK=1), runs == oracle."""
    env = dict(os.environ, WTAMD_INDEX_CHECK="1", WTAMD_DELTA_MIN_TRACKS="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "index-shapes-ok 32" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
