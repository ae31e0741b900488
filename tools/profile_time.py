"""Times the profile door (csrc/wt_profile.hip, wtamd_runs_profile) on the GPU and wtamd_runs_apply (fill-in) over the same
regions in the same process: apply does strictly less work per region -- one search and six doubles instead of a search per
bin and `width` doubles --, so the ratio to it, next to the bytes the profile has to write, is the figure to watch.

Input (one segment): the dataset tools/region_time.py builds -- 6 * 10^7 runs that do not overlap, f32 values, resident in HBM --
against 10^6 regions of 10 runs on 100 and on 1000 bins (the latter stretches: c > 1), 10^4 regions of 5 000 runs on 1000 bins
and 1 region over everything on 1000 bins, each per region (`profiles`) and summed (`profile`).  Every call is timed with events
around the whole call (its pool allocations, its passes and the copies of its counters included), --reps times after one
warm-up; the minimum counts.  GB/s = (12 bytes per run under a region + 8 bytes per bin written) / time.

With --reference <the reference's sources> the compiled reference's ProfileMultiplexer is timed INSTEAD, on this host's CPU, on
one thread, through the driver of tests/golden/make_profile_golden.py (array children): over the same dataset and the first
--ref-regions regions of each shape, as regions per second.  It needs no GPU and adds its figures to the file the device run
wrote.

  python tools/profile_time.py [--out profiles/profile.json] [--reps 3] [--runs 60000000] [--reference PATH]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from apply_time import make_regions  # noqa: E402
from region_time import make_source, timed  # noqa: E402

SHAPES = (("1e6_regions_of_10_runs_on_100_bins", 1_000_000, 10, 100), ("1e6_regions_of_10_runs_on_1000_bins", 1_000_000, 10, 1000),
          ("1e4_regions_of_5000_runs_on_1000_bins", 10_000, 5_000, 1000), ("1_region_over_everything_on_1000_bins", 1, 0, 1000))


def reference(a, s, f, v, shapes):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import make_profile_golden as G
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        L = G.build(a.reference, tmp)
        for name, rs, rf, runs, W in shapes:
            if not runs:
                out[name] = {"skipped": "a region of 10^6 bp and more takes the reference's unbuffered path (apply.c:197), which the profile door does not model"}
                continue
            k = min(len(rs), a.ref_regions if runs == 10 else max(a.ref_regions // 100, 1))
            data = (["chr1"], [(s, f)], v.astype(np.float64))
            t0 = time.perf_counter()
            rec = G.run(L, ["chr1"], data, (["chr1"], [(rs[:k], rf[:k])]), 0.0, W)
            dt = time.perf_counter() - t0
            out[name] = {"regions": k, "seconds": dt, "regions_per_s": k / dt, "base_pairs_per_s": float((rf[:k].astype(np.int64) - rs[:k]).sum()) / dt,
                         "first_row_first_bins": rec["rows"][0][:4]}
            print(json.dumps({"reference": {name: out[name]}}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "profile.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--runs", type=int, default=60_000_000)
    ap.add_argument("--reference", default=None)
    ap.add_argument("--ref-regions", type=int, default=2_000)
    a = ap.parse_args()
    rng = np.random.default_rng(2026)
    s, f, v = make_source(rng, a.runs)
    n = len(s)
    shapes, made = [], {}
    for name, count, runs, W in SHAPES:
        if (count, runs) not in made:
            made[(count, runs)] = make_regions(rng, s, f, count, runs)
        shapes.append((name,) + made[(count, runs)] + (runs, W))
    if a.reference:
        rec = json.load(open(a.out)) if os.path.exists(a.out) else {"tool": "tools/profile_time.py"}
        rec["reference_1_thread"] = {"what": "the compiled reference's ProfileMultiplexer, array children; on the CPU of the host that ran --reference (not the "
                                             "GPU host); a prefix of the regions of each shape: device_over_reference_regions_per_s is a ratio of rates "
                                             "EXTRAPOLATED from that prefix, not of like-for-like times",
                                     "shapes": reference(a, s, f, v, shapes)}
        for name, d in rec["reference_1_thread"]["shapes"].items():
            if name in rec and "per_region" in rec[name] and "regions_per_s" in d:
                rec[name]["device_over_reference_regions_per_s"] = rec[name]["per_region"]["regions_per_s"] / d["regions_per_s"]
        json.dump(rec, open(a.out, "w"), indent=1)
        return
    import torch
    from wiggletools_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    ds, df, dv = torch.from_numpy(s).to(dev), torch.from_numpy(f).to(dev), torch.from_numpy(v).to(dev)
    seg = np.array([0, n], np.int64)
    rec = {"tool": "tools/profile_time.py", "device": torch.cuda.get_device_name(0), "dataset_runs": n, "span_bp": int(f[-1]), "value": "f32",
           "timing": "events around the call, pool allocations included; minimum of --reps after one warm-up",
           "GB_per_s": "(12 B per run under a region + 8 B per bin written) / time", "default": 0.0}
    for name, rs, rf, per, W in shapes:
        drs, drf = torch.from_numpy(rs).to(dev), torch.from_numpy(rf).to(dev)
        rseg = np.array([0, len(rs)], np.int64)
        under = len(rs) * per if per else n
        r = {"regions": len(rs), "runs_under_regions": under, "width": W, "mean_region_bp": float((rf.astype(np.int64) - rs).mean())}
        m6 = torch.empty((len(rs), 6), dtype=torch.float64, device=dev)
        t = timed(a.reps, lambda: _lib.check(L.wtamd_runs_apply(1, seg.ctypes.data, ds.data_ptr(), df.data_ptr(), dv.data_ptr(), 0, rseg.ctypes.data,
                                                                drs.data_ptr(), drf.data_ptr(), 0.0, 0, m6.data_ptr(), None)))
        r["apply_fillin"] = {"ms": t, "best_ms": min(t)}
        del m6
        for mode, flags, n_out in (("per_region", 0, len(rs) * W), ("sum", 1, W)):
            out = torch.empty(n_out, dtype=torch.float64, device=dev)
            t = timed(a.reps, lambda: _lib.check(L.wtamd_runs_profile(1, seg.ctypes.data, ds.data_ptr(), df.data_ptr(), dv.data_ptr(), 0, rseg.ctypes.data,
                                                                      drs.data_ptr(), drf.data_ptr(), W, 0.0, flags, out.data_ptr(), None)))
            best = min(t) * 1e-3
            r[mode] = {"ms": t, "best_ms": min(t), "regions_per_s": len(rs) / best, "bytes_written": 8 * len(rs) * W,
                       "GB_per_s": (12.0 * under + 8.0 * len(rs) * W) / best / 1e9, "time_over_apply": min(t) / r["apply_fillin"]["best_ms"],
                       "first_bins": out[:4].cpu().tolist()}
            if flags == 0:
                total = out.view(len(rs), W).sum(0)
            else:       # the tree's sum against a plain column sum of the rows: to rounding
                assert torch.allclose(out, total, rtol=1e-9, atol=1e-6), (out[:4], total[:4])
            del out
        rec[name] = r
        print(json.dumps({name: r}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
