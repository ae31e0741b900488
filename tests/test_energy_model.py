"""The exact model of tests/energy_model.py against every value recorded from the compiled reference's EnergyIntegrator
(tests/golden/energy_fixtures.json): real and im within the reference's own error bound 2^-53 S (16 P / lam + B + 8), res its
real^2 + im^2, NaN where a value is NaN.  The recorded exact values are read back; with mpmath present they are recomputed and
must be the recorded bits."""
import numpy as np
import pytest

import energy_model as M


def _extent(lists):
    base, _ = M.bases(lists)
    P = max([abs(base[g] + int(x)) for g in range(lists.n_seg) for x in list(lists.s[lists.seg[g]:lists.seg[g + 1]]) + list(lists.f[lists.seg[g]:lists.seg[g + 1]])] + [0])
    return P, int((lists.f.astype(np.int64) - lists.s).sum())


def test_the_recorded_reference_lies_within_its_bound_of_the_exact_value():
    seen = {"overlaps": 0, "seek": 0, "nan": 0, "empty": 0, "zero": 0}
    for c in M.fixtures():
        lists = M.fixture_lists(c)
        assert len(lists.s) <= 40
        P, B = _extent(lists)
        assert P <= 2 ** 17 and B <= 2 * 10 ** 4
        S = M.weight(lists)
        assert S == M._num(c["S"]) or S != S
        star, ref = M.fixture_exact(c), M.fixture_reference(c)
        for k, lam in enumerate(M.fixture_wavelengths(c)):
            if np.isnan(star[k]).any():
                assert np.isnan(ref[k]).all(), (c["name"], lam)
                continue
            bound = 2.0 ** -53 * S * (16.0 * P / lam + B + 8)
            assert (np.abs(ref[k, :2] - star[k]) <= bound).all(), (c["name"], lam, ref[k], star[k], bound)
            assert ref[k, 2] == ref[k, 0] * ref[k, 0] + ref[k, 1] * ref[k, 1]
            if lam >= 2:
                assert bound < 1e-10 * S
            seen["zero"] += int((star[k] == 0).any())
        seen["overlaps"] += int(c["overlaps"])
        seen["seek"] += int(c["seek"] is not None)
        seen["nan"] += int(np.isnan(star).any())
        seen["empty"] += int(any(len(r["start"]) == 0 for r in c["chroms"]))
    assert min(seen.values()) >= 1, seen


def test_the_offset_rule_and_the_union_of_the_model():
    L = M.Lists.from_segments([([1, 5], [3, 9], [1.0, 2.0]), ([], [], []), ([2], [4], [1.0])])
    assert M.bases(L) == ([0, 9, 9], 13)
    assert M.bases(L, [5, 0, 100]) == ([5, 0, 100], 104)
    U = M.union(M.Lists.from_segments([([1, 2, 10, 10], [5, 3, 12, 15], [1.0, 2.0, 3.0, 4.0])]))
    assert (U.s.tolist(), U.f.tolist(), U.v.tolist()) == ([1, 10], [5, 15], [1.0, 3.0])


def test_the_recorded_exact_values_are_what_mpmath_gives():
    pytest.importorskip("mpmath")
    for c in M.fixtures()[::3]:
        assert M.same_bits(M.exact(M.fixture_lists(c), M.fixture_wavelengths(c)), M.fixture_exact(c)), c["name"]
    seams, rec = M.seam_cases(), M.seam_values()
    assert sorted(seams) == sorted(rec)
    for name in ("runs_1", "runs_5", "far", "far_base", "wavelengths_9", "nan_first"):
        lists, lam, sb = seams[name]
        assert M.same_bits(M.exact(lists, lam, sb), np.array([[M._num(a), M._num(b)] for a, b in rec[name]["exact"]]).reshape(-1, 2)), name
        assert rec[name]["n"] == len(lists.s) and rec[name]["end_base"] == M.bases(lists, sb)[1]
