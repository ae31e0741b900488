"""The phase reduction of csrc/wt_energy.h (wen_bm, wen_phase, wen_mod: a modulus by a host-made double reciprocal with one
correction) against integer arithmetic, over the whole range the door admits -- in the style of tests/test_div_by_count.py.
m = (2 (base + start) + L - 1) mod 2 lam and q = L mod 2 lam are compared in C with 128-bit integers (tests/energy_emu.cpp), for
every lam in [1, 4096] plus 2^16 +- 1, 2^30 +- 1 and 2^31 - 1: numerators 0, +-1, k 2 lam - 1, k 2 lam, k 2 lam + 1 for the extreme k the
door admits (|base| <= 2^62 - 2^31, coordinates any int32 with start < finish), and 10^5 seeded random ones per wavelength."""
import ctypes as C

import numpy as np

import energy_model as M

LAMS = list(range(1, 4097)) + [2 ** 16 - 1, 2 ** 16 + 1, 2 ** 30 - 1, 2 ** 30 + 1, 2 ** 31 - 1]
MAX_BASE = 2 ** 62 - 2 ** 31
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def _edge_runs(lam):
    """(base, start, finish) whose numerator 2 (base + start) + L - 1 is 0, +-1 and k 2 lam - 1, k 2 lam, k 2 lam + 1 at the extreme k
    of either sign, and the extremes of every argument."""
    d = 2 * lam
    out = []
    for target in [0, 1, -1] + [k * d + e for k in (MAX_BASE // lam - 2, -(MAX_BASE // lam) + 2, (2 ** 32) // d, -((2 ** 32) // d)) for e in (-1, 0, 1)]:
        # numerator = 2 a + L - 1: L = 1 gives the even targets (a = target / 2), L = 2 the odd ones (a = (target - 1) / 2)
        ln = 1 if target % 2 == 0 else 2
        a = (target - ln + 1) // 2
        s = max(I32_MIN, min(I32_MAX - ln, a))
        base = a - s
        if abs(base) <= MAX_BASE:
            out.append((base, s, s + ln))
    for base in (MAX_BASE, -MAX_BASE, 0):
        out += [(base, I32_MIN, I32_MAX), (base, I32_MIN, I32_MIN + 1), (base, I32_MAX - 1, I32_MAX), (base, -1, 0), (base, 0, 1)]
    return out


def test_phase_reduction_is_exact_over_the_admitted_range():
    lib = M.emu_lib()
    lib.energy_mod_check.restype = C.c_int64
    lib.energy_mod_check.argtypes = [C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    rng = np.random.default_rng(20261204)
    n = 100000
    base = rng.integers(-MAX_BASE, MAX_BASE + 1, n)
    base[: n // 4] = rng.integers(-2 ** 33, 2 ** 33, n // 4)
    s = rng.integers(I32_MIN, I32_MAX, n).astype(np.int32)
    ln = np.where(rng.random(n) < 0.5, rng.integers(1, 5000, n), rng.integers(1, 2 ** 32, n))
    f = np.minimum(s.astype(np.int64) + ln, I32_MAX).astype(np.int32)
    assert (f > s).all()
    for lam in LAMS:
        e = _edge_runs(lam)
        eb, es, ef = (np.array([r[k] for r in e], t) for k, t in ((0, np.int64), (1, np.int32), (2, np.int32)))
        assert lib.energy_mod_check(lam, len(e), eb.ctypes.data, es.ctypes.data, ef.ctypes.data) == 0, lam
        assert lib.energy_mod_check(lam, n, base.ctypes.data, s.ctypes.data, f.ctypes.data) == 0, lam


def test_the_edges_are_what_python_integers_give():
    """The C comparison's own yardstick, for a few wavelengths, against Python's integers through the emulated door's phase: a run
    of length 1 at position p contributes cos / sin of -2 pi p / lam, which for p a multiple of lam is exactly (1, -0 or 0)."""
    for lam in (2, 7, 4096, 2 ** 31 - 1):
        for k in (MAX_BASE // lam - 2, -(MAX_BASE // lam) + 2):
            p = k * lam
            L = M.Lists([0, 1], [0], [1], [1.0])
            rc, out, _ = M.emu_door(L, [lam], [p])
            assert rc == 0 and abs(out[0, 0] - 1.0) <= M.door_bound(1, 1.0) and out[0, 1] == 0.0, (lam, k, out)


def test_the_raw_modulus_below_2_35():
    lib = M.emu_lib()
    lib.energy_rawmod_check.restype = C.c_int64
    lib.energy_rawmod_check.argtypes = [C.c_int32, C.c_int64, C.c_void_p]
    rng = np.random.default_rng(20261205)
    for lam in LAMS[::64] + LAMS[-5:]:
        d = 2 * lam
        top = (2 ** 35 - 1) // d
        x = np.concatenate([[0, 1, 2 ** 35 - 1], [k * d + e for k in (1, top // 2, top) for e in (-1, 0, 1) if 0 <= k * d + e < 2 ** 35],
                            rng.integers(0, 2 ** 35, 20000)]).astype(np.uint64)
        assert lib.energy_rawmod_check(lam, len(x), x.ctypes.data) == 0, lam
