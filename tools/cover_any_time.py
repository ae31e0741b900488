"""Times wtamd_runs_coverage_flags with WTAMD_COVER_ANY_ORDER (csrc/wt_cover.hip) on the GPU next to wtamd_runs_coverage over
the same intervals sorted by start: the any-order path runs the same passes and sorts nothing, so it should cost what the
sorted one costs, give or take the spread.

Input (one segment): the covering components of 10^7 synthetic 100-bp reads over 2.5 * 10^8 bp, in file order -- reads sorted
by position, components in CIGAR order; 1 % of the reads are spliced (50M <gap>N 50M, gap 100 .. 10 000: two components, the
second far to the right of the reads that follow), 5 % carry a deletion (40M 3D 60M: three touching components).
  file_order   flag set, the list as a SAM file gives it
  shuffled     flag set, the same intervals in random order (no locality left for the bitmap and delta atomics)
  sorted_any   flag set, the list sorted by start
  sorted       flags 0 (wtamd_runs_coverage), the list sorted by start
Every variant is timed with events around the whole call (its device allocations, its passes and the copies of its counters
included), the variants ALTERNATING inside each of --reps rounds after one warm-up round; minimum, median and maximum are
recorded.  The four results are compared on the device: equal, byte for byte.

  python tools/cover_any_time.py [--out profiles/cover_any_order.json] [--reps 5] [--reads 10000000]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ANY_ORDER = 1


def make_reads(rng, n, span):
    """(start, finish) of every covering component, in file order."""
    pos = np.sort(rng.integers(1, span, n)).astype(np.int64)
    kind = rng.random(n)
    spliced, deletion = kind < 0.01, (kind >= 0.01) & (kind < 0.06)
    gap = rng.integers(100, 10001, n)
    count = np.where(spliced, 2, np.where(deletion, 3, 1))
    off = np.concatenate([[0], np.cumsum(count)])
    s, f = np.zeros(off[-1], np.int64), np.zeros(off[-1], np.int64)
    first = off[:-1]
    plain = ~spliced & ~deletion
    s[first[plain]], f[first[plain]] = pos[plain], pos[plain] + 100
    k, p = first[spliced], pos[spliced]
    s[k], f[k] = p, p + 50
    s[k + 1], f[k + 1] = p + 50 + gap[spliced], p + 100 + gap[spliced]
    k, p = first[deletion], pos[deletion]
    s[k], f[k] = p, p + 40
    s[k + 1], f[k + 1] = p + 40, p + 43
    s[k + 2], f[k + 2] = p + 43, p + 103
    return s.astype(np.int32), f.astype(np.int32), int(spliced.sum()), int(deletion.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cover_any_order.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--span", type=int, default=250_000_000)
    a = ap.parse_args()
    import torch
    from wiggletools_amd import _lib
    assert torch.cuda.is_available(), "tools/cover_any_time.py measures on the GPU"
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(2027)
    s, f, n_spliced, n_del = make_reads(rng, a.reads, a.span)
    n = len(s)
    o = np.argsort(s, kind="stable")
    sh = rng.permutation(n)
    breaks = int(np.count_nonzero(np.diff(s.astype(np.int64)) < 0))
    assert breaks > 0
    inputs = {"file_order": (s, f, ANY_ORDER), "shuffled": (s[sh], f[sh], ANY_ORDER), "sorted_any": (s[o], f[o], ANY_ORDER),
              "sorted": (s[o], f[o], None)}
    cap = 2 * n - 1
    seg = np.array([0, n], np.int64)
    state = {}
    for name, (vs, vf, flags) in inputs.items():
        state[name] = dict(s=torch.from_numpy(np.ascontiguousarray(vs)).to(dev), f=torch.from_numpy(np.ascontiguousarray(vf)).to(dev), flags=flags,
                           os=torch.empty(cap, dtype=torch.int32, device=dev), of=torch.empty(cap, dtype=torch.int32, device=dev),
                           ov=torch.empty(cap, dtype=torch.float64, device=dev), ms=[], n_out=0)

    def call(st):
        oseg, n_out = np.zeros(2, np.int64), C.c_int64()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if st["flags"] is None:
            rc = L.wtamd_runs_coverage(1, seg.ctypes.data, st["s"].data_ptr(), st["f"].data_ptr(), cap, st["os"].data_ptr(), st["of"].data_ptr(),
                                       st["ov"].data_ptr(), oseg.ctypes.data, C.byref(n_out), None)
        else:
            rc = L.wtamd_runs_coverage_flags(1, seg.ctypes.data, st["s"].data_ptr(), st["f"].data_ptr(), cap, st["os"].data_ptr(), st["of"].data_ptr(),
                                             st["ov"].data_ptr(), oseg.ctypes.data, C.byref(n_out), st["flags"], None)
        e1.record()
        e1.synchronize()
        _lib.check(rc)
        st["n_out"] = n_out.value
        return e0.elapsed_time(e1)

    for k in range(a.reps + 1):
        for name in inputs:
            ms = call(state[name])
            if k:
                state[name]["ms"].append(ms)
    ref = state["sorted"]
    m = ref["n_out"]
    rec = {"tool": "tools/cover_any_time.py", "reads": a.reads, "spliced_reads": n_spliced, "reads_with_a_deletion": n_del, "intervals": n,
           "span_bp": a.span, "order_breaks_in_file_order": breaks, "runs": m,
           "timing": "events around the whole call, allocations included; variants alternate inside each of %d rounds after one warm-up round" % a.reps}
    for name, st in state.items():
        same = st["n_out"] == m and all(bool(torch.equal(st[k][:m], ref[k][:m])) for k in ("os", "of", "ov"))
        assert same, name
        ms = sorted(st["ms"])
        rec[name] = {"ms": st["ms"], "min_ms": ms[0], "median_ms": ms[len(ms) // 2], "max_ms": ms[-1], "intervals_per_s": n / (ms[0] * 1e-3),
                     "equal_to_sorted": same}
    spread = rec["sorted"]["max_ms"] - rec["sorted"]["min_ms"]
    rec["spread_of_sorted_ms"] = spread
    for name in ("file_order", "shuffled", "sorted_any"):
        rec[name]["median_over_sorted_median"] = rec[name]["median_ms"] / rec["sorted"]["median_ms"]
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
