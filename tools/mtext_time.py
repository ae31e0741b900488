"""Times the tile-text door (csrc/wt_mtext.hip: wtamd_tile_text, wtamd_trackset_mtext) on the GPU.

Shapes, all resident in HBM, one segment: width 1 x 6 * 10^7 entries in bedGraph mode (the list of tools/text_time.py, so that
wtamd_runs_text over the same list, timed in the same run, is the yardstick); width 2 x 3 * 10^7; width 100 x 6 * 10^5 in
bedGraph mode and in wig mode with 40 % of the entries 1 to 3 bp long; and wtamd_trackset_mtext over 100 resident synthetic
tracks of one chromosome (600000 bp; the tile materialised and printed on the device).  Every call is timed with events around the whole
call (its pool allocations, its four passes, the copies of its tables and scalars included), --reps times after one warm-up:
minimum, median and (max - min) / min are kept.  A call with no room (capacity 0) stops after the scan and is timed the same
way: the emit pass by difference.  The text of a prefix of whole blocks is compared byte for byte with tests/mtext_model.py.

With --reference <the reference's sources> the compiled reference's TeeMultiplexer is timed INSTEAD, on this host's CPU,
through the array-backed Multiplexer of tests/golden/make_mtext_golden.py into /dev/null, over a PREFIX of --ref-entries
entries of each tile shape: the ratios to the device are ratios of RATES, EXTRAPOLATED from that prefix and labelled so.  It
needs no GPU and adds its figures to the file the device run wrote.

  python tools/mtext_time.py [--out profiles/mtext.json] [--reps 5] [--scale 1.0] [--reference PATH] [--ref-entries N]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from region_time import make_source, timed  # noqa: E402
from text_time import make_short  # noqa: E402

DEVNULL_DRIVER = r'''
long long time_mtext(int n_chrom, char **names, long long *seg_off, int *start, int *finish, double *vals, int width, int bedGraph) {
    FILE *fp = fopen("/dev/null", "w");
    Multiplexer *m = TeeMultiplexer(marr_new(n_chrom, names, seg_off, start, finish, vals, width), fp, bedGraph, false);
    long long n = 0;
    while (!m->done) { n++; popMultiplexer(m); }
    fclose(fp);
    return n;
}
'''


def tile_shapes(a):
    """{name: (start, finish, values[n, width], bedGraph)}"""
    rng = np.random.default_rng(2026)
    n1, n2, n100 = int(60_000_000 * a.scale), int(30_000_000 * a.scale), int(600_000 * a.scale)
    s, f, v = make_source(rng, n1)
    ws, wf, _ = make_short(rng, n100)
    cells = lambda n, w: (rng.integers(0, 4000, (n, w)) / 16.0)       # noqa: E731
    return {"w1_bedgraph": (s, f, v.astype(np.float64).reshape(-1, 1), True), "w2_bedgraph": (s[:n2], f[:n2], cells(n2, 2), True),
            "w100_bedgraph": (s[:n100], f[:n100], cells(n100, 100), True), "w100_wig_short_runs": (ws, wf, cells(n100, 100), False)}


def reference(a, shapes):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_mtext_golden as G
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        drv = os.path.join(tmp, "driver.c")
        open(drv, "w").write(G.DRIVER + DEVNULL_DRIVER)
        so = os.path.join(tmp, "libmtexttime.so")
        subprocess.check_call(["gcc", "-g", "-w", "-O3", "-std=gnu99", "-D_GNU_SOURCE", "-fPIC", "-shared", "-I" + os.path.join(a.reference, "src")] +
                              [os.path.join(a.reference, "src", x) for x in G.REF_SRCS] + [drv, "-o", so, "-lm", "-lpthread"])
        L = C.CDLL(so, mode=os.RTLD_LAZY)
        L.time_mtext.restype = C.c_longlong
        for name, (s, f, v, bed) in shapes.items():
            k = min(max(a.ref_entries // v.shape[1], 10000), len(s))
            names = (C.c_char_p * 1)(b"chr1")
            seg = np.array([0, k], np.int64)
            s, f, v = np.ascontiguousarray(s[:k]), np.ascontiguousarray(f[:k]), np.ascontiguousarray(v[:k])
            p = lambda x: C.c_void_p(x.ctypes.data)      # noqa: E731
            t0 = time.perf_counter()
            n = L.time_mtext(1, names, p(seg), p(s), p(f), p(v), int(v.shape[1]), int(bed))
            dt = time.perf_counter() - t0
            out[name] = {"entries": k, "entries_passed_on": int(n), "seconds": dt, "entries_per_s": k / dt, "values_per_s": k * v.shape[1] / dt}
            print(json.dumps({"reference": {name: out[name]}}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mtext.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="scales every shape's entry count (a quick look)")
    ap.add_argument("--check-entries", type=int, default=20_000)
    ap.add_argument("--reference", default=None)
    ap.add_argument("--ref-entries", type=int, default=3_000_000, help="cells of the prefix the reference prints per shape")
    a = ap.parse_args()
    shapes = tile_shapes(a)
    if a.reference:
        rec = json.load(open(a.out)) if os.path.exists(a.out) else {"tool": "tools/mtext_time.py"}
        ref = reference(a, shapes)
        rec["reference_1_thread"] = {"what": "the compiled reference's TeeMultiplexer (its writer thread printing) over an array-backed Multiplexer into /dev/null, "
                                             "popped to the end; on the CPU of the host that ran --reference (not the GPU host); EXTRAPOLATED: a PREFIX of about "
                                             "%d cells per shape, the device_over_reference figures are ratios of RATES, not of like-for-like times" % a.ref_entries,
                                     "shapes": ref}
        for name, d in ref.items():
            if name in rec.get("shapes", {}):
                rec["shapes"][name]["device_over_reference_entries_per_s"] = rec["shapes"][name]["entries_per_s"] / d["entries_per_s"]
        json.dump(rec, open(a.out, "w"), indent=1)
        return
    import torch
    import mtext_model as M
    from wiggletools_amd import _lib, engine, synthgen
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    rec = {"tool": "tools/mtext_time.py", "device": torch.cuda.get_device_name(0), "reps": a.reps, "scale": a.scale,
           "timing": "events around the call, pool allocations included; --reps after one warm-up per shape: ms lists every repeat, best_ms the minimum, "
                     "spread = (max - min) / min; measure_and_scan: the same call with capacity 0, which stops after the scan (cells, mode, scan); "
                     "emit_by_difference: the difference of the two minima",
           "GB_per_s": "(8 B per entry + 8 B per cell + the bytes written) / time",
           "not_measured": "no kernel trace (the passes' own durations are known only through the call with no room); the D2H copy of the text; no alternative "
                           "kernel shape (cells per workgroup, items per lane, one alignment per copy of a point-by-point row) was timed",
           "shapes": {}}
    names = (C.c_char_p * 1)(b"chr1")
    nb, nw = C.c_int64(), C.c_int64()
    for name, (hs, hf, hv, bed) in shapes.items():
        n, w = hv.shape
        seg = np.array([0, n], np.int64)
        ds, df, dv = torch.from_numpy(np.ascontiguousarray(hs)).to(dev), torch.from_numpy(np.ascontiguousarray(hf)).to(dev), torch.from_numpy(hv).to(dev)
        flags = 1 if bed else 0

        def call(text, cap, want):
            rc = L.wtamd_tile_text(1, seg.ctypes.data, names, ds.data_ptr(), df.data_ptr(), dv.data_ptr(), w, None, None, flags, None, text, cap, C.byref(nb),
                                   C.byref(nw), None)
            assert rc == want, (rc, L.wtamd_last_error())

        t_ms = timed(a.reps, lambda: call(None, 0, 3))
        size = int(nb.value)
        text = torch.empty(size, dtype=torch.uint8, device=dev)
        t = timed(a.reps, lambda: call(text.data_ptr(), size, 0))
        best = min(t) * 1e-3
        d = {"mode": "bedGraph" if bed else "wig", "entries": n, "width": w, "bytes": size, "bytes_per_entry": size / n, "ms": t, "best_ms": min(t),
             "median_ms": float(np.median(t)), "spread": (max(t) - min(t)) / min(t), "entries_per_s": n / best, "values_per_s": n * w / best,
             "GB_per_s": (8.0 * n + 8.0 * n * w + size) / best / 1e9, "measure_and_scan": {"ms": t_ms, "best_ms": min(t_ms)},
             "emit_by_difference_ms": min(t) - min(t_ms)}
        k = min(a.check_entries // M.BLOCK * M.BLOCK, n)
        if k:
            expect = M.text(M.Tile(M.Lists(["chr1"], [0, k], hs[:k], hf[:k], np.zeros(k)), hv[:k]), flags)[0]
            d["prefix_checked_entries"] = k
            d["prefix_equal_to_model_byte_for_byte"] = bool(text[:len(expect)].cpu().numpy().tobytes() == expect)
        if name == "w1_bedgraph":                   # the single-column door over the same list, f64 values as here
            def one(tp, cap, want):
                rc = L.wtamd_runs_text(1, seg.ctypes.data, names, ds.data_ptr(), df.data_ptr(), dv.data_ptr(), 1, flags, None, tp, cap, C.byref(nb), C.byref(nw), None)
                assert rc == want, (rc, L.wtamd_last_error())
            t1 = timed(a.reps, lambda: one(text.data_ptr(), size, 0))
            d["runs_text_same_list"] = {"ms": t1, "best_ms": min(t1), "bytes": int(nb.value)}
            d["time_over_runs_text"] = min(t) / min(t1)
        rec["shapes"][name] = d
        print(json.dumps({name: d}), flush=True)
        del text, ds, df, dv
    # 100 resident tracks of one chromosome: multiplexed and printed on the device
    clen = int(600_000 * a.scale)
    tseg, tstart, tfinish, tvalue = synthgen.device_tracks(7, [clen], 100)
    ts = engine.TrackSet.from_device(1, 100, tseg, tstart, tfinish, tvalue, np.zeros(100))
    nr = C.c_int64()
    cn = (C.c_char_p * 1)(b"chr1")

    def tcall(text, cap, want):
        rc = L.wtamd_trackset_mtext(ts._h, cn, 1, None, text, cap, C.byref(nb), C.byref(nw), C.byref(nr), None)
        assert rc == want, (rc, L.wtamd_last_error())

    t_ms = timed(a.reps, lambda: tcall(None, 0, 3))
    size = int(nb.value)
    text = torch.empty(size, dtype=torch.uint8, device=dev)
    t = timed(a.reps, lambda: tcall(text.data_ptr(), size, 0))
    n = int(nr.value)
    rec["shapes"]["trackset_100_tracks_bedgraph"] = {"chromosome_bp": clen, "entries": n, "width": 100, "bytes": size, "ms": t, "best_ms": min(t),
                                                     "spread": (max(t) - min(t)) / min(t), "entries_per_s": n / (min(t) * 1e-3),
                                                     "multiplex_measure_and_scan": {"ms": t_ms, "best_ms": min(t_ms)},
                                                     "emit_by_difference_ms": min(t) - min(t_ms)}
    print(json.dumps({"trackset": rec["shapes"]["trackset_100_tracks_bedgraph"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
