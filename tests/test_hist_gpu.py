"""Value histograms on the device (csrc/wt_hist.hip: wtamd_runs_histogram) against the NumPy model of tests/hist_model.py, which
tests/test_hist_model.py pins to every matrix, range and text recorded from the compiled reference: bit for bit, with f32 and
f64 input of the same values giving the same bits.  The seam sizes come from the header's constants (hist_model.constants)."""
import numpy as np
import pytest

import hist_model as M

pytestmark = pytest.mark.gpu

SEAMS = M.seam_cases()
ERR_ARG = 1


def _door(L, w, flags=0, given=None, base=None, dtype=np.float64):
    from wiggletools_amd import engine
    from wiggletools_amd.runlists import RunLists
    rl = RunLists(len(L.row), 1, L.seg, L.s, L.f, L.v.astype(dtype), [0.0])
    return engine._hist_door(rl, w, flags, given, base, seg_row=L.row, n_rows=L.n_rows)


def test_fixtures_case_by_case():
    for c in M.fixtures():
        L, w = M.fixture_lists(c)
        rng, model = M.check_case(_door, L, w, c["name"], dtypes=(np.float64,))
        assert M.same_bits(model, M.fixture_result(c)[1]) and M.same_bits(rng, M.fixture_result(c)[0])
        # the same values rounded to float32: as f32 and as f64 input
        L32 = M.Lists(L.seg, L.row, L.n_rows, L.s, L.f, L.v.astype(np.float32).astype(np.float64))
        M.check_case(_door, L32, w, (c["name"], "f32"))


def test_all_fixtures_in_one_call_with_seg_row_mapping():
    L, rows = M.all_fixtures_as_one()
    for w in (10, M.constants()["LDS_WIDTH"] + 1):
        M.check_case(_door, L, w, w, dtypes=(np.float64,))


@pytest.mark.parametrize("name", sorted(SEAMS))
def test_seams(name):
    """Rows of a share - 1, a share, + 1 and 3 shares + 1 with row boundaries inside a share, an empty row, an all-NaN row;
    segments of a row apart and together; widths 1, 2, LDS_WIDTH and LDS_WIDTH + 1 with one column, two alternating columns, 64
    distinct columns in a wave and a column past 2^32; values on exact bin edges; v == hi; lo == hi; -0.0; no value at all."""
    L, w = SEAMS[name]
    M.check_case(_door, L, w, name)


def test_histogram_runlists_has_one_row_per_track():
    from wiggletools_amd import engine
    from wiggletools_amd.runlists import RunLists
    L, w = SEAMS["chromosome_major"]
    rl = RunLists(3, 3, L.seg, L.s, L.f, L.v.astype(np.float32), [0.0] * 3)
    rng, m = engine.histogram_runlists(rl, w)
    (lo, hi), model = M.histogram(L, w)
    assert M.same_bits(rng, [lo, hi]) and M.same_bits(m, model)


def test_a_split_list_composes_to_the_bits_of_the_single_call():
    S = M.constants()["SHARE"]
    L, w = SEAMS["rows"]
    M.check_split(_door, L, w, [S - 3, S + 1, 4 * S + 70], "rows")
    L, w = SEAMS["wave_of_columns_w%d" % (M.constants()["LDS_WIDTH"] + 1)]
    M.check_split(_door, L, w, [1, 2, S], "global regime")


def test_refusals_return_err_arg_and_write_nothing():
    """Every refusal is decided by the argument checks or by the validation pass, before anything is written."""
    M.check_refusals(_door, ERR_ARG)
    from wiggletools_amd import _lib
    assert b"wtamd_runs_histogram" in _lib.lib().wtamd_last_error()


def test_the_host_entry_gives_the_same_bits():
    import ctypes as C
    from wiggletools_amd import _lib
    for name in ("rows", "track_major", "past_2_32_w2"):
        L, w = SEAMS[name]
        (lo, hi), model = M.histogram(L, w)
        r2, out = np.full(2, -1.0), np.full((L.n_rows, w), -1.0)
        rc = _lib.lib().wtamd_runs_histogram_host(len(L.row), L.seg.ctypes.data, L.row.ctypes.data, L.n_rows, L.s.ctypes.data, L.f.ctypes.data,
                                                  L.v.ctypes.data, w, 0, r2.ctypes.data, out.ctypes.data)
        assert rc == 0 and M.same_bits(r2, [lo, hi]) and M.same_bits(out, model), name
        rc = _lib.lib().wtamd_runs_histogram_host(len(L.row), L.seg.ctypes.data, L.row.ctypes.data, L.n_rows, L.s.ctypes.data, L.f.ctypes.data,
                                                  L.v.ctypes.data, w, M.RANGE_GIVEN | M.ACCUMULATE, r2.ctypes.data, out.ctypes.data)
        assert rc == 0 and M.same_bits(out, 2 * model), name


def test_dropin():
    """wtamd_histogram, wtamd_normalize_histogram and wtamd_print_histogram of the product over bulk and popping children, and
    again with WTAMD_NO_DEVICE_HIST=1: the recorded texts byte for byte."""
    import os
    import hist_dropin
    from wiggletools_amd import _lib

    def setenv(k, v):
        os.environ[k] = v

    hist_dropin.check_dropin(hist_dropin.DropIn(_lib.LIB_PATH), M.fixtures(), setenv)
    os.environ.pop("WTAMD_NO_DEVICE_HIST", None)


def test_python_dropin_histogram():
    from wiggletools_amd import dropin
    c = [c for c in M.fixtures() if len(c["rows"]) == 2 and c["width"] == 10 and all(len(r["start"]) for r in c["rows"])][0]
    L, w = M.fixture_lists(c)
    L = M.Lists(L.seg, L.row, L.n_rows, L.s, L.f, L.v.astype(np.float32).astype(np.float64))
    keep, kids = [], []
    for s, f, v in L.rows():
        s, f, v = np.ascontiguousarray(s), np.ascontiguousarray(f), np.ascontiguousarray(v, np.float32)
        keep.append((s, f, v))
        kids.append(dropin.array_reader(["chr1"], [0, len(s)], s.ctypes.data, f.ctypes.data, v.ctypes.data))
    rng, m, txt = dropin.histogram(kids, w)
    (lo, hi), model = M.histogram(L, w)
    assert M.same_bits(rng, [lo, hi]) and M.same_bits(m, model) and txt == M.text((lo, hi), model)
