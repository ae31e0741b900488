"""Times the energy door (csrc/wt_energy.hip: wtamd_runs_energy) on the GPU.

The dataset tools/region_time.py builds -- 6 * 10^7 sorted disjoint runs, f32 values, resident in HBM, one segment -- at 1, 16
and 256 wavelengths, the wavelengths around 10 (`helix`), around 147-200 (`nucleosome`) and around 10^6 (`long`).  Reported per
shape: time; runs * wavelengths per second; nanoseconds per (run, wavelength); GB/s counting the 12 bytes per run of ONE read;
the time as a multiple of wtamd_runs_moments over the same list in the same process (f64 values: 16 bytes per run streamed
once, nothing computed).  Every call is timed with events around the whole call (its pool allocations, its three passes and its
copies included), --reps times after one warm-up per shape: minimum, median and (max - min) / min are kept.  Every
one-wavelength shape is checked against the same door over the list cut in two: the halves' sums must agree with the single
call to the door's bound, and the second half's end_base must be the single call's (--no-check skips that).

With --reference <the reference's sources> the compiled reference's EnergyIntegrator is timed INSTEAD, on this host's CPU, on
one thread, through the driver of tests/golden/make_energy_golden.py (an array child), over a PREFIX of --ref-runs runs (one
pass serves one wavelength): the ratios to the device are then ratios of RATES, EXTRAPOLATED from that prefix and labelled so.
It needs no GPU and adds its figures to the file the device run wrote.

Where the time goes: csrc/build.py's build_source_variant("wt_energy.hip", "noprobe1", ["-DWEN_PROBE=1"]) builds a library whose
main pass reduces the phases but calls no trigonometric function, -DWEN_PROBE=2 one that calls them without reducing a phase
(both give wrong sums).  WTAMD_LIB=<that library> python tools/energy_time.py --no-check --kinds nucleosome --counts 256 --out
<another file> times it.

  python tools/energy_time.py [--out profiles/energy.json] [--reps 5] [--runs 60000000] [--reference PATH] [--ref-runs N]
"""
import argparse
import json
import os
import sys
import tempfile
import time
import ctypes as C

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from region_time import make_source, timed  # noqa: E402

COUNTS = (1, 16, 256)
CENTRES = {"helix": 10, "nucleosome": 147, "long": 1000000}


def wavelengths(kind, k):
    """k wavelengths from the centre upwards (helix: 10, 11, ...; nucleosome: 147 .. 200 and on; long: 10^6 in steps of 997)."""
    c = CENTRES[kind]
    return np.array([c + j * (997 if kind == "long" else 1) for j in range(k)], np.int32)


def reference(a, s, f, v):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import energy_model as M
    import make_energy_golden as G
    k = min(a.ref_runs, len(s))
    lists = M.Lists([0, k], s[:k], f[:k], v[:k].astype(np.float64))
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        L = G.build(a.reference, tmp)
        for kind in CENTRES:
            lam = int(wavelengths(kind, 1)[0])
            t0 = time.perf_counter()
            got = G.run(L, ["chr1"], lists, False, lam, None)
            dt = time.perf_counter() - t0
            out[kind] = {"runs": k, "wavelength": lam, "seconds": dt, "run_wavelengths_per_s": k / dt, "real_im": got[:2].tolist()}
            print(json.dumps({"reference": {kind: out[kind]}}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "energy.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=60_000_000)
    ap.add_argument("--reference", default=None)
    ap.add_argument("--ref-runs", type=int, default=2_000_000)
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--counts", default=",".join(str(k) for k in COUNTS))
    ap.add_argument("--kinds", default=",".join(CENTRES))
    a = ap.parse_args()
    counts, kinds = [int(x) for x in a.counts.split(",")], a.kinds.split(",")
    import energy_model as M
    rng = np.random.default_rng(2026)
    s, f, v = make_source(rng, a.runs)
    n = len(s)
    if a.reference:
        rec = json.load(open(a.out)) if os.path.exists(a.out) else {"tool": "tools/energy_time.py"}
        shapes = reference(a, s, f, v)
        rec["reference_1_thread"] = {"what": "the compiled reference's EnergyIntegrator over an array child, one wavelength per pass; on the CPU of the host "
                                             "that ran --reference (not the GPU host), one thread; a PREFIX of %d runs: the device_over_reference figures "
                                             "are ratios of RATES EXTRAPOLATED from that prefix, not of like-for-like times" % min(a.ref_runs, n),
                                     "shapes": shapes}
        for name, d in rec.get("shapes", {}).items():
            r = shapes.get(d["wavelengths"])
            if r:
                d["device_over_reference_run_wavelengths_per_s_EXTRAPOLATED"] = d["run_wavelengths_per_s"] / r["run_wavelengths_per_s"]
        json.dump(rec, open(a.out, "w"), indent=1)
        return
    import torch
    from wiggletools_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    ds, df, dv = torch.from_numpy(s).to(dev), torch.from_numpy(f).to(dev), torch.from_numpy(v).to(dev)
    rec = {"tool": "tools/energy_time.py", "device": torch.cuda.get_device_name(0), "dataset_runs": n, "value": "f32", "reps": a.reps,
           "timing": "events around the call, pool allocations included; --reps after one warm-up per shape: ms lists every repeat, best_ms the minimum, "
                     "spread = (max - min) / min",
           "GB_per_s": "12 B per run / time (one read of the list)", "shapes": {}}
    dv64 = dv.double()
    runs = _lib.Runs(n, ds.data_ptr(), df.data_ptr(), dv64.data_ptr(), None)
    m6 = np.zeros(6)
    t = timed(a.reps, lambda: _lib.check(L.wtamd_runs_moments(C.byref(runs), n, m6.ctypes.data, None)))
    mom = {"ms": t, "best_ms": min(t), "median_ms": float(np.median(t)), "spread": (max(t) - min(t)) / min(t), "GB_per_s": 16.0 * n / (min(t) * 1e-3) / 1e9}
    rec["runs_moments_f64"] = mom
    print(json.dumps({"runs_moments_f64": mom}), flush=True)
    del dv64
    seg = np.array([0, n], np.int64)
    S = float(np.abs(v.astype(np.float64)) @ (f.astype(np.int64) - s).astype(np.float64))
    for kind in kinds:
        for k in counts:
            lam = wavelengths(kind, k)
            out, end = np.zeros((k, 2)), np.zeros(1, np.int64)
            t = timed(a.reps, lambda: _lib.check(L.wtamd_runs_energy(1, seg.ctypes.data, None, ds.data_ptr(), df.data_ptr(), dv.data_ptr(), 0, k,
                                                                     lam.ctypes.data, out.ctypes.data, end.ctypes.data, None)))
            best = min(t) * 1e-3
            name = "%s_k%d" % (kind, k)
            d = {"wavelengths": kind, "n_wavelengths": k, "first_wavelength": int(lam[0]), "ms": t, "best_ms": min(t), "median_ms": float(np.median(t)),
                 "spread": (max(t) - min(t)) / min(t), "run_wavelengths_per_s": n * k / best, "ns_per_run_wavelength": best * 1e9 / (n * k),
                 "GB_per_s": 12.0 * n / best / 1e9, "time_over_runs_moments": min(t) / mom["best_ms"], "real_im_first": out[0].tolist()}
            if not a.no_check and k == 1:
                half = n // 2 + 7
                acc, e = np.zeros(2), np.zeros(1, np.int64)
                for a0, b0 in ((0, half), (half, n)):
                    part = np.zeros((1, 2))
                    sg, sb = np.array([0, b0 - a0], np.int64), np.zeros(1, np.int64)
                    _lib.check(L.wtamd_runs_energy(1, sg.ctypes.data, sb.ctypes.data, ds[a0:b0].data_ptr(), df[a0:b0].data_ptr(), dv[a0:b0].data_ptr(), 0, 1,
                                                   lam.ctypes.data, part.ctypes.data, e.ctypes.data, None))
                    acc += part[0]
                d["split_agrees_within_bound"] = bool((np.abs(acc - out[0]) <= 2 * M.door_bound(n, S)).all() and int(e[0]) == int(end[0]))
                d["split_difference_over_bound"] = float(np.abs(acc - out[0]).max() / M.door_bound(n, S))
            rec["shapes"][name] = d
            print(json.dumps({name: d}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
