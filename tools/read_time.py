"""Times the read door (csrc/wt_read.hip: wtamd_text_runs) on the GPU.

The two lists of tools/text_time.py -- 6 * 10^7 runs each, one in bedGraph mode, one in wig mode with a realistic share of short
runs -- are printed in HBM by wtamd_runs_text and parsed by wtamd_text_runs where they lie.  Reported per shape: the bytes read,
the records, segments and slow values found, bytes per second and records per second, and the ratio to wtamd_runs_text over
the same list in the same run.  Every call is timed with events around the whole call (its pool allocations, its six passes,
the copies of its states and scalars included), --reps times after one warm-up per shape: minimum, median and (max - min) / min
are kept.  A call with no room (capacities 0) runs the lines, scan, count and scan2 passes only and is timed the same way: the
write and state passes by difference.  A prefix of --check-runs runs is compared with tests/read_model.py record for record.

With --reference <the reference's sources> the compiled reference's WiggleReader is timed INSTEAD, on this host's CPU, one
thread, over the text of a PREFIX of --ref-runs runs (printed by tests/text_model.py, whose text the device's is held to),
popped to the end: the ratios to the device are ratios of RATES, EXTRAPOLATED from that prefix and labelled so.  It needs no
GPU and adds its figures to the file the device run wrote.

  python tools/read_time.py [--out profiles/read.json] [--reps 5] [--runs 60000000] [--reference PATH] [--ref-runs N]
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

COUNT_DRIVER = r'''
long long time_read(char *path) {
    WiggleIterator *wi = WiggleReader(path);
    long long n = 0;
    while (!wi->done) { n++; pop(wi); }
    return n;
}
'''


def reference(a, shapes):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_read_golden as G
    import text_model as T
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        drv = os.path.join(tmp, "driver.c")
        open(drv, "w").write(G.DRIVER + COUNT_DRIVER)
        so = os.path.join(tmp, "libreadtime.so")
        subprocess.check_call(["gcc", "-g", "-w", "-O3", "-std=gnu99", "-D_GNU_SOURCE", "-fPIC", "-shared", "-I" + os.path.join(a.reference, "src")] +
                              [os.path.join(a.reference, "src", x) for x in G.REF_SRCS] + [drv, "-o", so, "-lm", "-lpthread"])
        L = C.CDLL(so, mode=os.RTLD_LAZY)
        L.time_read.restype = C.c_longlong
        for name, (s, f, v, bed) in shapes.items():
            k = min(a.ref_runs, len(s))
            txt = T.text(T.Lists(["chr1"], [0, k], s[:k], f[:k], v[:k].astype(np.float64)), 1 if bed else 0)[0]
            path = os.path.join(tmp, name + ".txt")
            open(path, "wb").write(txt)
            t0 = time.perf_counter()
            n = L.time_read(path.encode())
            dt = time.perf_counter() - t0
            out[name] = {"runs_printed": k, "bytes": len(txt), "lines": txt.count(b"\n"), "runs_popped_behind_its_compression": int(n), "seconds": dt,
                         "bytes_per_s": len(txt) / dt}
            print(json.dumps({"reference": {name: out[name]}}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "read.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=60_000_000)
    ap.add_argument("--check-runs", type=int, default=100_000)
    ap.add_argument("--reference", default=None)
    ap.add_argument("--ref-runs", type=int, default=200_000)
    a = ap.parse_args()
    rng = np.random.default_rng(2026)
    s, f, v = make_source(rng, a.runs)
    ws, wf, wv = make_short(rng, a.runs)
    n = len(s)
    shapes = {"bedgraph": (s, f, v, True), "wig_short_runs": (ws, wf, wv, False)}
    if a.reference:
        rec = json.load(open(a.out)) if os.path.exists(a.out) else {"tool": "tools/read_time.py"}
        ref = reference(a, shapes)
        rec["reference_1_thread"] = {"what": "the compiled reference's WiggleReader (fgets, countWords, sscanf; its compression rule behind it) over a file "
                                             "in the page cache, popped to the end; on the CPU of the host that ran --reference (not the GPU host); "
                                             "EXTRAPOLATED: the text of a PREFIX of %d runs, the device_over_reference figures are ratios of RATES, not of "
                                             "like-for-like times" % a.ref_runs, "shapes": ref}
        for name, d in ref.items():
            if name in rec.get("shapes", {}):
                rec["shapes"][name]["device_over_reference_bytes_per_s"] = rec["shapes"][name]["bytes_per_s"] / d["bytes_per_s"]
        json.dump(rec, open(a.out, "w"), indent=1)
        return
    import torch
    import read_model as M
    import text_model as T
    from wiggletools_amd import _lib, engine
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    rec = {"tool": "tools/read_time.py", "device": torch.cuda.get_device_name(0), "dataset_runs": n, "reps": a.reps,
           "timing": "events around the call, pool allocations included; --reps after one warm-up per shape: ms lists every repeat, best_ms the minimum, "
                     "spread = (max - min) / min; counting: the same call with capacities 0, which stops after scan2; write_by_difference: the difference of "
                     "the two minima; runs_text: wtamd_runs_text printing the same text in the same run",
           "not_measured": "the kernels' own durations (no kernel trace was taken), the _host door, text with many chromosomes", "shapes": {}}
    names = (C.c_char_p * 1)(b"chr1")
    seg = np.array([0, n], np.int64)
    for name, (hs, hf, hv, bed) in shapes.items():
        ds, df, dv = torch.from_numpy(hs).to(dev), torch.from_numpy(hf).to(dev), torch.from_numpy(hv).to(dev)
        flags = 1 if bed else 0
        nb, nw = C.c_int64(), C.c_int64()

        def write(text, cap, want):
            rc = L.wtamd_runs_text(1, seg.ctypes.data, names, ds.data_ptr(), df.data_ptr(), dv.data_ptr(), 0, flags, None, text, cap, C.byref(nb), C.byref(nw), None)
            assert rc == want, (rc, L.wtamd_last_error())

        write(None, 0, 3)
        size = int(nb.value)
        text = torch.empty(size + 16, dtype=torch.uint8, device=dev)
        tw = timed(a.reps, lambda: write(text.data_ptr(), size, 0))
        del ds, df, dv
        cn = engine.ReadCounts()

        def read(ptrs, caps, want):
            st = engine.ReadState()
            rc = L.wtamd_text_runs(text.data_ptr(), size, 0, C.addressof(st), ptrs[0], ptrs[1], ptrs[2], caps[0], ptrs[3], ptrs[4], ptrs[5], caps[1], ptrs[6],
                                   ptrs[7], caps[2], C.addressof(cn), None)
            assert rc == want, (rc, L.wtamd_last_error())

        t_count = timed(a.reps, lambda: read([None] * 8, (0, 0, 0), 3))
        m, g, k = int(cn.n_runs), int(cn.n_seg), int(cn.n_slow)
        os_, of = torch.empty(m, dtype=torch.int32, device=dev), torch.empty(m, dtype=torch.int32, device=dev)
        ov = torch.empty(m, dtype=torch.float64, device=dev)
        sg, so = torch.empty(g + 1, dtype=torch.int64, device=dev), torch.empty(g, dtype=torch.int64, device=dev)
        sl = torch.empty(g, dtype=torch.int32, device=dev)
        wr, wo = torch.empty(max(k, 1), dtype=torch.int64, device=dev), torch.empty(max(k, 1), dtype=torch.int64, device=dev)
        ptrs = [x.data_ptr() for x in (os_, of, ov, sg, so, sl, wr, wo)]
        t = timed(a.reps, lambda: read(ptrs, (m, g, k), 0))
        best = min(t) * 1e-3
        d = {"mode": "bedGraph" if bed else "wig", "bytes": size, "lines": int(cn.n_lines), "records": m, "segments": g, "slow_values": k,
             "share_of_slow_values": k / max(m, 1), "ms": t, "best_ms": min(t), "median_ms": float(np.median(t)), "spread": (max(t) - min(t)) / min(t),
             "bytes_per_s": size / best, "records_per_s": m / best, "runs_printed_per_s": n / best,
             "counting": {"ms": t_count, "best_ms": min(t_count)}, "write_by_difference_ms": min(t) - min(t_count),
             "runs_text": {"ms": tw, "best_ms": min(tw)}, "time_over_runs_text": min(t) / min(tw)}
        # a prefix against the model, record for record (a prefix of whole blocks of the writer is a text of its own)
        kk = min(a.check_runs // T.BLOCK * T.BLOCK, n)
        if kk:
            want = M.read(T.text(T.Lists(["chr1"], [0, kk], hs[:kk], hf[:kk], hv[:kk].astype(np.float64)), flags)[0], 0)
            r = len(want.recs)
            got = list(zip(os_[:r].cpu().tolist(), of[:r].cpu().tolist(), ov[:r].view(torch.int64).cpu().numpy().view(np.uint64).tolist()))
            d["prefix_checked_records"] = r
            d["prefix_equal_to_model_record_for_record"] = bool(got == [(x[1], x[2], x[3]) for x in want.recs])
        rec["shapes"][name] = d
        print(json.dumps({name: d}), flush=True)
        del text, os_, of, ov, sg, so, sl, wr, wo
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
