"""The Python model of the Multiplexer writer (tests/mtext_model.py) against what the compiled reference printed
(tests/golden/mtext_fixtures.json, recorded by tests/golden/make_mtext_golden.py, which asserts equality for every case) and,
where the compiled reference is present, against its `mwrite` / `mwrite_bg` of fuzzed track sets (oracle.mwrite): strict and
not, non-zero defaults, both modes."""
import hashlib

import numpy as np
import pytest

import mtext_model as M
from helpers import random_case


def test_the_model_against_the_recorded_reference_texts():
    fx = M.fixtures()
    every = M.reference_cases()
    seen = set()
    for c in fx["cases"]:
        if c["case"] not in every:
            continue                                            # (the long line: below)
        T = every[c["case"]]
        txt = M.text(T, c["flags"])[0]
        assert c["input_sha256"] == T.digest(), (c["name"], "the case is not the one recorded")
        assert (len(T), T.width) == (c["entries"], c["width"])
        assert len(txt) == c["bytes"] and hashlib.sha256(txt).hexdigest() == c["sha256"], c["name"]
        if "text" in c:
            assert txt == c["text"].encode("latin-1"), c["name"]
        else:
            assert M.seam_lines(txt, T, c["flags"]) == c["seams"], c["name"]
        seen.add((c["case"], c["flags"]))
    assert seen == {(k, fl) for k, T in every.items() for fl in M.flags_of(T)}      # every case in every mode it has
    assert sum(1 for c in fx["cases"] if "text" in c) >= 10 and sum(1 for c in fx["cases"] if c.get("seams")) >= 8


def test_the_recorded_paste_corners():
    fx = M.fixtures()
    c = next(c for c in fx["cases"] if c["case"] == "long_line")
    T = M.cases()["paste_w3"].part(6, 50)
    line = bytes(48 + i % 10 for i in range(12000))                # one line of the infile, consumed by three entries
    T = M.Tile(T.L, T.vals, [line[:4999], line[4999:9998], line[9998:]] + T.prefixes[3:])
    txt = M.text(T, 0)[0]
    assert c["input_sha256"] == T.digest() and (len(txt), hashlib.sha256(txt).hexdigest()) == (c["bytes"], c["sha256"])
    s = fx["short_infile"]
    assert s["exit_status"] == 1 and s["stderr"] == "Could not paste data to file lines, inconsistent number of lines.\n"
    T = M.cases()["paste_w3"].part(6, 50)
    assert (s["entries"], s["written_entries"]) == (len(T), len(T) - 1)
    assert hashlib.sha256(M.text(T.part(0, len(T) - 1), 0)[0]).hexdigest() == s["written_sha256"]


def test_width_one_bedgraph_is_the_single_column_writers_line():
    import text_model as tm
    L = tm.cases()["random_257"]
    assert M.text(M.Tile(L, L.v.reshape(-1, 1)), M.BEDGRAPH)[0] == tm.text(L, tm.BEDGRAPH)[0]


@pytest.mark.parametrize("seed", range(3))
def test_the_model_against_the_reference_mwrite(oracle, tmp_path, seed):
    if not oracle.have_ref():
        pytest.skip("compiled reference not available")
    R = oracle.ref_harness()
    t = random_case(9800 + seed, n_tracks=4, max_len=3000)
    d = t.as_dict()
    for strict in (0, 1):
        chrom, s, f, tile, _ = oracle.multiplex(d, strict)
        if len(s) == 0:
            continue
        seg = np.concatenate([[0], np.cumsum(np.bincount(chrom, minlength=t.n_chrom))])
        T = M.Tile(M.Lists(list(t.chrom_names), seg, s, f, np.zeros(len(s))), tile)
        for bg in (False, True):
            ref = R.mwrite(d, tmp_path / "b.txt", bedgraph=bg, flags=strict).encode("latin-1")
            mine = M.text(T, M.BEDGRAPH if bg else 0)[0]
            assert mine == ref, (strict, bg) + M.first_difference(mine, ref)
