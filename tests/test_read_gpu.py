"""Wig, bedGraph and BED text into run lists on the device (csrc/wt_read.hip: wtamd_text_runs) against the Python model of
tests/read_model.py, which tests/golden/make_read_golden.py holds record for record to what the compiled reference's WiggleReader
and BedReader popped, and against the recorded readings themselves (tests/golden/read_fixtures.json).  No tolerance exists here:
records, segments, slow list, counts, state and every value bit are equal."""
import numpy as np
import pytest

import read_model as M

pytestmark = pytest.mark.gpu

CASES = M.cases()


@pytest.fixture(scope="module", autouse=True)
def _pools_as_a_fresh_process_has_them():
    """The staging buffers of these tests rest in the library's process-wide pools afterwards; tests that count the pools'
    misses (tests/test_trackset_pool.py) expect to meet nothing larger than their own buffers there."""
    yield
    from wiggletools_amd import _lib
    _lib.lib().wtamd_pool_trim()


def _door(data, flags=0, state=None, capacity=None, seg_capacity=None, slow_capacity=None, offset=0):
    from wiggletools_amd import engine
    return engine._read_door(data, flags, state, capacity, seg_capacity, slow_capacity, offset)


@pytest.fixture(scope="module")
def device_readings():
    """Every regular case through the door, once: {name: the door's output} (checked against the model on the way)."""
    out = {}
    for name, (data, flags) in CASES.items():
        out[name] = _door(data, flags)
        M.check_reading(out[name], data, flags, None, name)
    return out


def _records(out, data, patched=True):
    """[(name, start, finish, bits)] of a door's output over a whole file, the slow values through float()."""
    n, g = out["counts"]["n_runs"], out["counts"]["n_seg"]
    bits = [int(x) for x in out["value"][:n]]
    if patched:
        for r, off in zip(out["slow_rec"][:out["counts"]["n_slow"]], out["slow_off"][:out["counts"]["n_slow"]]):
            end = data.index(b"\n", int(off)) if b"\n" in data[int(off):] else len(data)
            bits[int(r)] = M.float_to_bits(float(data[int(off):end].decode()))
    recs = []
    for k in range(g):
        off, ln = int(out["seg_name_off"][k]), int(out["seg_name_len"][k])
        for i in range(int(out["seg_off"][k]), int(out["seg_off"][k + 1])):
            recs.append((data[off:off + ln], int(out["start"][i]), int(out["finish"][i]), bits[i]))
    return recs


def test_fixtures_record_for_record(device_readings):
    """What the reference popped: the device's records, slow values patched, behind the compression rule for a wig reader."""
    fx = M.fixtures()["cases"]
    assert sorted(c["name"] for c in fx) == sorted(device_readings)
    for c in fx:
        data, flags = CASES[c["name"]]
        recs = _records(device_readings[c["name"]], data)
        got = M.as_fixture(recs if flags & M.BED else M.compress(recs))
        for k in ("n", "sha256", "records", "head", "tail"):
            assert got.get(k) == c.get(k), (c["name"], k)


def test_quotients_and_products_are_the_host_s_bits():
    """f64 W * 10^E and W / 10^-E on the device against float() over the number cases and a 10^5-numeral sample of the fuzz
    generator: one text, a fixedStep line a numeral."""
    toks = [t for t in M.NUMBERS + M.fuzz_numerals(100000) if M.number(t) is not None]
    data = b"fixedStep chrom=chr1 start=1 step=1\n" + b"\n".join(toks) + b"\n"
    out = _door(data, 0)
    assert out["rc"] == M.OK and out["counts"]["n_runs"] == len(toks)
    want = [M.number(t) for t in toks]
    got = out["value"][:len(toks)].tolist()
    bad = [(toks[i], "%016x" % got[i], "%016x" % want[i][0]) for i in range(len(toks)) if got[i] != want[i][0]]
    assert not bad, bad[:5]
    assert out["slow_rec"][:out["counts"]["n_slow"]].tolist() == [i for i, w in enumerate(want) if w[1]]
    exact = sum(1 for w in want if not w[1])
    assert exact > 10000 and len(want) - exact > 10000


def test_the_same_bytes_on_a_second_call(device_readings):
    for name in ("mixed_20001", "values", "bed_257"):
        data, flags = CASES[name]
        again = _door(data, flags)
        for k in list(M.KEYS) + ["counts", "state"]:
            a, b = again[k], device_readings[name][k]
            assert (a == b) if isinstance(a, dict) else np.array_equal(a, b), (name, k)


def test_text_at_every_alignment():
    for name in ("mixed_257", "line_straddles"):
        data, flags = CASES[name]
        for off in range(16):
            M.check_reading(_door(data, flags, offset=off), data, flags, None, (name, off))


def test_one_entry_short_is_refused_with_the_counts_needed():
    M.check_capacities(_door, *CASES["values"], "values")


def test_refusals_write_nothing_and_leave_the_state():
    M.check_refusals(_door)


def test_an_empty_call_leaves_the_state_alone():
    M.check_empty(_door)


@pytest.mark.parametrize("name", ["mixed_257", "section_three_tiles", "same_chrom_headers", "bedgraph_after_fixed", "chrom_changes", "short_lines",
                                  "header_ends_tile", "values", "bed_257", "no_final_newline_fixed"])
def test_cut_texts_chain_through_the_state(name):
    """Cut after a header, inside a fixedStep section, between chromosomes and at tile edges: equal to the whole."""
    M.check_chained(_door, *CASES[name], name)


def test_round_trip_through_the_writer():
    """compress(parse(wtamd_runs_text(L))) == compress(L) for the value-exact lists of text_model.cases() (multiples of 1/16),
    in both modes; for the others parse equals the model's reading of the same bytes."""
    import text_model as T
    from wiggletools_amd import engine
    from wiggletools_amd.runlists import RunLists
    for name, L in T.cases().items():
        if len(L) > 300 and name != "random_10001":
            continue
        exact = bool(np.all(np.isfinite(L.v)) and np.all(L.v * 16 == np.round(L.v * 16)) and np.all(np.abs(L.v) < 2.0 ** 30))
        rl = RunLists(len(L.names), 1, L.seg, L.s, L.f, L.v, [0.0], [n.decode("latin-1") for n in L.names])
        for flags in (0, T.BEDGRAPH):
            rc, buf, nb, _, _ = engine._text_door(rl, flags)
            assert rc == 0
            data = buf[:nb].tobytes()
            out = _door(data, 0)
            M.check_reading(out, data, 0, None, (name, flags))
            if exact:
                got = M.compress(_records(out, data))
                C = T.compress(L)
                want = [(C.names[C.seg_of(i)], int(C.s[i]), int(C.f[i]), M.float_to_bits(float(C.v[i]))) for i in range(len(C))]
                assert got == want, (name, flags)


def test_read_text_returns_the_run_lists():
    from wiggletools_amd import engine
    data, _ = CASES["bedgraph_257"]
    rl = engine.read_text(data)
    m = M.read(data, 0)
    assert rl.n_tracks == 1 and list(rl.chrom_names) == [m.recs[s[0]][0].decode() for s in m.segs]
    assert rl.start.tolist() == [r[1] for r in m.recs] and rl.finish.tolist() == [r[2] for r in m.recs]
    assert rl.value.view(np.uint64).tolist() == [r[3] for r in M.patched(data, m)]
    data, flags = CASES["values"]
    rl = engine.read_text(data)
    m = M.read(data, flags)
    assert rl.value.view(np.uint64).tolist() == [r[3] for r in M.patched(data, m)]      # (the slow values by strtod)
    bed = engine.read_text(CASES["bed_eof"][0], bed=True)
    assert bed.start.tolist() == [2, 2] and bed.value.tolist() == [1.0, 1.0]
    with pytest.raises(Exception):
        engine.read_text(b"chr1\t1\t2\t3\n\nchr1\t2\t3\t4\n")
