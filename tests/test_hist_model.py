"""The NumPy model of the histogram rule (tests/hist_model.py) pinned to every case recorded from the compiled reference
(tests/golden/hist_fixtures.json): the matrix and the range bit for bit, both printed texts byte for byte.  No case is left out;
every case meets the condition under which the reference's streaming histogram and the two-pass rule are the same thing."""
import numpy as np

import hist_model as M


def test_the_model_gives_every_recorded_matrix_range_and_text():
    cases = M.fixtures()
    assert len(cases) >= 60
    for c in cases:
        L, w = M.fixture_lists(c)
        assert M.reference_equal(L, w), c["name"]
        rng, rec = M.fixture_result(c)
        (lo, hi), model = M.histogram(L, w)
        assert M.same_bits(model, rec) and M.same_bits([lo, hi], rng), c["name"]
        assert M.text((lo, hi), model) == c["text"], c["name"]
        assert M.text((lo, hi), M.normalize(model)) == c["normalized_text"], c["name"]


def test_the_fixtures_hold_what_the_issue_lists():
    cases = M.fixtures()
    assert sorted({c["width"] for c in cases}) == list(M.WIDTHS)
    assert {len(c["rows"]) for c in cases} == {1, 2, 3}
    assert all(len(r["start"]) <= 41 for c in cases for r in c["rows"])
    firsts = [[x for x in c["rows"][0]["value"] if x is not None][:2] for c in cases]
    assert any(a < b for a, b in firsts) and any(a > b for a, b in firsts)
    assert all(a <= b for (a, b), c in zip(firsts, cases) if c["width"] == 1)
    assert any(c["rows"][0]["value"][0] is None for c in cases)                                         # a NaN run leads row 0
    assert any(max(max(row) for row in c["hist"]) > 2 ** 32 for c in cases)
    assert any(c["range"][0] == c["range"][1] for c in cases)
    assert any(len(r["start"]) == 0 for c in cases for r in c["rows"])
    assert any(len(r["value"]) and all(x is None for x in r["value"]) for c in cases for r in c["rows"])
    assert any("nan" in c["normalized_text"] for c in cases)


def test_the_worked_example_of_the_departures():
    """Lengths 4, values 0, 1, 0.5, 2, 0.25, width 4: the value 2 leaves the range of the first two, the reference re-bins by
    interpolation and reports 8 8 0 4; the exact histogram is 8 4 4 4."""
    L = M.Lists.from_rows([([1, 5, 9, 13, 17], [5, 9, 13, 17, 21], [0, 1, 0.5, 2, 0.25])])
    assert not M.reference_equal(L, 4)
    rng, m = M.histogram(L, 4)
    assert rng == (0.0, 2.0) and m.tolist() == [[8.0, 4.0, 4.0, 4.0]]
    # width 1 with the second distinct value lower: the reference zeroes the only column; the rule gives the total span
    L = M.Lists.from_rows([([1, 5], [5, 9], [1.0, 0.5])])
    assert not M.reference_equal(L, 1) and M.reference_equal(L, 2)
    assert M.histogram(L, 1)[1].tolist() == [[8.0]]


def test_range_given_and_accumulate_compose():
    L, w = M.seam_cases()["chromosome_major"]
    rng, m = M.histogram(L, w)
    a, b = L.part(0, 100), L.part(100, len(L.s))
    _, ma = M.histogram(a, w, given=rng)
    _, mb = M.histogram(b, w, given=rng, base=ma)
    assert M.same_bits(mb, m)


def test_a_zero_extreme_is_plus_zero_and_an_empty_input_has_no_range():
    L, w = M.seam_cases()["minus_zero"]
    (lo, hi), m = M.histogram(L, w)
    assert M.same_bits([lo, hi], [0.0, 0.0]) and m[0, 1:].sum() == 0
    L, w = M.seam_cases()["no_value"]
    (lo, hi), m = M.histogram(L, w)
    assert np.isnan(lo) and np.isnan(hi) and not m.any()
