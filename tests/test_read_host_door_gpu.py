"""wtamd_text_runs_host (csrc/wt_read.hip) called directly: chunks chained through the state (a segment whose name comes from
the state that came in), the names copied out or not asked for, a name buffer one byte short, and more slow values than the
door's first slow list holds (the retry with the count needed): records, names and values, the slow ones by strtod, equal to
the model's."""
import ctypes as C

import numpy as np
import pytest

import read_model as M

pytestmark = pytest.mark.gpu


def _host(data, flags, state, names=True, name_cap=None, cap=None):
    from wiggletools_amd import _lib, engine
    n = (data.count(b"\n") + 1) if cap is None else cap
    s, f, v = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float64)
    seg, noff, nlen = np.zeros(n + 1, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int32)
    size = (len(data) + n + 600) if name_cap is None else name_cap
    buf = C.create_string_buffer(max(size, 1))
    st, cn = engine.ReadState.from_dict(state), engine.ReadCounts()
    rc = _lib.lib().wtamd_text_runs_host(data, len(data), flags, C.addressof(st), s.ctypes.data, f.ctypes.data, v.ctypes.data, n, seg.ctypes.data,
                                         noff.ctypes.data, nlen.ctypes.data, n, C.addressof(buf) if names else None, size if names else 0, C.addressof(cn))
    m, g = int(cn.n_runs), int(cn.n_seg)
    got_names, p = [], 0
    for k in range(g if names and rc == 0 else 0):
        got_names.append(buf.raw[p:p + int(nlen[k])])
        p += int(nlen[k]) + 1
    recs = [(int(s[i]), int(f[i]), int(v[i:i + 1].view(np.uint64)[0])) for i in range(m)] if rc == 0 else []
    return rc, recs, [int(x) for x in seg[:g]], got_names, st.as_dict(), cn.as_dict()


def _want(data, flags, state):
    m = M.read(data, flags, state)
    st0 = state or M.fresh_state()
    names = [st0["chrom"] if off == M.STATE_NAME else data[off:off + ln] for _, off, ln in m.segs]
    return m, [(r[1], r[2], r[3]) for r in M.patched(data, m)], [x[0] for x in m.segs], names


def test_chunks_chain_and_names_come_from_the_state():
    for name in ("section_three_tiles", "same_chrom_headers", "values", "mixed_257"):
        data, flags = M.cases()[name]
        st = None
        for a, b in zip([0] + M.cut_points(data), M.cut_points(data) + [len(data)]):
            piece = data[a:b]
            m, recs, segs, names = _want(piece, flags, st)
            rc, got, gsegs, gnames, st2, cn = _host(piece, flags, st)
            assert rc == 0 and got == recs and gsegs == segs and gnames == names and st2 == m.state and cn == m.counts, (name, a, b)
            rc, got, gsegs, _, st3, _ = _host(piece, flags, st, names=False)
            assert rc == 0 and got == recs and st3 == m.state, (name, a, b, "no names")
            st = st2
    assert any(off == M.STATE_NAME for _, off, _ in M.read(b"1\n2\n", 0, {"mode": 1, "span": 1, "step": 1, "last_start": 0, "next": 5, "chrom": b"chrS", "rec_name": b""}).segs)
    rc, got, _, gnames, _, _ = _host(b"1\n2\n", 0, {"mode": 1, "span": 1, "step": 1, "last_start": 0, "next": 5, "chrom": b"chrS", "rec_name": b""})
    assert rc == 0 and gnames == [b"chrS"] and [r[:2] for r in got] == [(5, 6), (6, 7)]


def test_a_name_buffer_one_byte_short_and_a_run_array_one_short():
    data, flags = M.cases()["chrom_changes"]
    m, recs, segs, names = _want(data, flags, None)
    need = sum(len(n) + 1 for n in names)
    st0 = M.fresh_state()
    rc, _, _, _, st, _ = _host(data, flags, None, name_cap=need - 1)
    assert rc == M.ERR_CAPACITY and st == st0
    rc, got, _, gnames, _, _ = _host(data, flags, None, name_cap=need)
    assert rc == 0 and got == recs and gnames == names
    rc, _, _, _, st, cn = _host(data, flags, None, cap=len(recs) - 1)
    assert rc == M.ERR_CAPACITY and st == st0 and cn == m.counts


def test_more_slow_values_than_the_first_slow_list_holds():
    toks = [b"0.%017d" % (10 ** 16 + 7 * i + 1) for i in range(1500)] + [b"1.5"]
    data = b"fixedStep chrom=chr1 start=1 step=1\n" + b"\n".join(toks) + b"\n"
    m, recs, _, _ = _want(data, 0, None)
    assert m.counts["n_slow"] > 1024              # (the door's first slow list holds 1024; numerals that end in 0 are exact)
    rc, got, _, _, _, cn = _host(data, 0, None)
    assert rc == 0 and cn == m.counts and got == recs
