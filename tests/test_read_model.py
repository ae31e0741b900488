"""The Python model of the reader's rule (tests/read_model.py) against what the compiled reference's WiggleReader and BedReader
popped (tests/golden/read_fixtures.json, written by tests/golden/make_read_golden.py, which asserts the same for every case):
record for record, value bits included."""
import hashlib

import read_model as M

CASES = M.cases()


def test_every_case_is_recorded_and_is_the_reference_s_reading():
    fx = M.fixtures()["cases"]
    assert sorted(c["name"] for c in fx) == sorted(CASES)
    for c in fx:
        data, flags = CASES[c["name"]]
        assert (c["flags"], c["bytes"], c["input_sha256"]) == (flags, len(data), hashlib.sha256(data).hexdigest()), (c["name"], "the case is not the one recorded")
        got = M.as_fixture(M.reference_reading(data, flags))
        for k in ("n", "sha256", "records", "head", "tail"):
            assert got.get(k) == c.get(k), (c["name"], k)


def test_the_shapes_the_passes_can_go_wrong_at():
    assert len(M.fixtures()["cases"]) == len(CASES)
    for n in (1, 255, 256, 257, 20001):
        assert CASES["mixed_%d" % n][0].count(b"\n") == n
    assert CASES["newline_last_byte"][0][M.TILE - 1:M.TILE] == b"\n" and CASES["newline_first_byte"][0][M.TILE:M.TILE + 1] == b"\n"
    assert CASES["header_ends_tile"][0][:M.TILE].endswith(b"span=5\n")
    assert len(CASES["section_three_tiles"][0]) > 2 * M.TILE and len(CASES["many_tiles"][0]) > 256 * M.TILE
    assert max(len(ln) for ln in CASES["long_comment"][0].split(b"\n")) == M.LINE_MAX - 1 == max(len(ln) for ln in CASES["long_number"][0].split(b"\n"))
    m = M.read(*CASES["values"])
    slow = {CASES["values"][0][off:CASES["values"][0].index(b"\n", off)] for _, off in m.slow}
    assert {b"9007199254740993", b"1e23", b"1e-23", b"12345678901234567890", b"4.9e-324", b"1e400"} <= slow
    assert not slow & {b"9007199254740992", b"1e22", b"1e-22", b"-0.000000", b"nan", b"-inf", b"1.500000", b"123e20"}


def test_every_irregular_class_is_one_line_first_and_last():
    cases = M.irregular_cases()
    assert sorted(c["name"] for c in M.fixtures()["irregular"]) == sorted(cases)
    assert len(cases) >= 2 * len(M.irregular_lines())
    for name, (data, flags, where) in cases.items():
        m = M.read(data, flags)
        assert m.rc == M.ERR_ARG and m.counts["n_irregular"] == 1 and m.counts["first_irregular"] == where, (name, m.counts)


def test_unsorted_bed_ends_the_reference_with_its_message():
    fx = {c["name"]: c for c in M.fixtures()["unsorted"]}
    for name, (data, n) in M.unsorted_cases().items():
        assert fx[name]["exit_status"] == 1 and "is not sorted" in fx[name]["stderr"] and fx[name]["input_sha256"] == hashlib.sha256(data).hexdigest()
        assert M.read(data, M.BED).counts["n_unsorted"] == n


def test_the_state_chains_the_model():
    for name in ("mixed_257", "same_chrom_headers", "values", "bed_257"):
        data, flags = CASES[name]
        M.check_chained(lambda d, f, state=None: _as_door(M.read(d, f, state)), data, flags, name)


def _as_door(m):
    import numpy as np
    n, g, k = m.counts["n_runs"], m.counts["n_seg"], m.counts["n_slow"]
    out = {"rc": m.rc, "counts": m.counts, "state": m.state, "start": np.array([r[1] for r in m.recs], np.int32), "finish": np.array([r[2] for r in m.recs], np.int32),
           "value": np.array([r[3] for r in m.recs], np.uint64), "seg_off": np.array([s[0] for s in m.segs] + ([n] if n else []), np.int64),
           "seg_name_off": np.array([s[1] for s in m.segs], np.int64), "seg_name_len": np.array([s[2] for s in m.segs], np.int32),
           "slow_rec": np.array([s[0] for s in m.slow], np.int64), "slow_off": np.array([s[1] for s in m.slow], np.int64),
           "text_guard": np.full(1, M.CANARY, np.uint8)}
    for key in M.KEYS:
        out[key + "_lo"] = out[key + "_hi"] = np.full(1, M.CANARY, np.uint8)
    return out
