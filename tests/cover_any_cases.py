"""Cases and helpers of the any-order coverage tests (tests/test_cover_any_order_emu.py on the CPU, test_cover_any_order_gpu.py
on the device): segments whose intervals are NOT sorted by start, for wtamd_runs_coverage_flags with WTAMD_COVER_ANY_ORDER.

What such a call must give is fixed without looking at the code under test: the coverage rule (tests/cover_model.py, pinned to
the compiled reference by tests/test_cover_model.py) is a function of the SET of a segment's intervals, so the expected result
is the model over the same intervals sorted by start -- and the door without the flag over that sorted list gives it too."""
import ctypes as C
import os

import numpy as np

import cover_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
ANY_ORDER = 1               # WTAMD_COVER_ANY_ORDER
EMPTY = (np.zeros(0, np.int32), np.zeros(0, np.int32))


def _i32(s, f):
    return np.asarray(s, np.int32), np.asarray(f, np.int32)


def _shuffled(rng, seg):
    o = rng.permutation(len(seg[0]))
    return seg[0][o], seg[1][o]


def spliced_reads(rng, n_reads, span, read_len=50):
    """The covering components of reads sorted by position, in file order: one read in eight is spliced (two components a long
    gap apart), so a later read's start follows an interval that starts far to its right."""
    pos = np.sort(rng.integers(1, span, n_reads))
    s, f = [], []
    for k, p in enumerate(pos):
        s.append(p); f.append(p + read_len)
        if k % 8 == 3:
            gap = int(rng.integers(100, 3000))
            s.append(p + read_len + gap); f.append(p + 2 * read_len + gap)
    return _i32(s, f)


def cases():
    """name -> list of segments (start, finish), intervals in the order the door is to take them."""
    rng = np.random.default_rng(21)
    out = {}
    # the smallest start is not the first interval: the last one, one in the middle, and the first finish is not the largest
    out["min_last"] = [_i32([40, 30, 20, 10], [45, 100, 25, 12])]
    out["min_middle"] = [_i32([500, 7, 300, 7, 301], [501, 9, 400, 300, 302])]
    out["issue_trap"] = [_i32([100, 1150, 120], [150, 1200, 170])]                  # 50M1000N50M at 100, then a read at 120
    out["two"] = [_i32([9, 3], [12, 9])]                                            # touching, backwards
    out["reversed"] = [tuple(x[::-1].copy() for x in M.random_segment(rng, 700, 30000, 90))]
    # one break of the order exactly across the seam of the 256-interval blocks of the pre-pass (255 | 256), and at 511 | 512
    s, f = M.random_segment(rng, 600, 9000, 40)
    for k in (255, 511):
        s[[k, k + 1]] = s[[k + 1, k]]; f[[k, k + 1]] = f[[k + 1, k]]
        if s[k] <= s[k + 1]:                                                         # (equal starts: force a real break)
            s[k] = s[k + 1] + 5; f[k] = s[k] + 3
    assert s[255] > s[256] and s[511] > s[512]
    out["break_at_block_seam"] = [(s, f)]
    # the smallest start of a segment sits in its SECOND block, the largest finish in its first
    s, f = M.random_segment(rng, 520, 5000, 30)
    s, f = s + 1000, f + 1000
    s[300], f[300] = 3, 5
    f[2] = 9000
    out["min_in_second_block"] = [(s, f)]
    # segment boundaries inside a block (250 | 10 | 300: block 0 holds two boundaries, block 1 one), every segment shuffled,
    # and the last interval of a segment above / the first of the next below: breaks on both sides of a boundary
    segs = [_shuffled(rng, M.random_segment(rng, n, 4000, 60)) for n in (250, 10, 300)]
    out["breaks_across_segment_boundaries"] = [segs[0], EMPTY, segs[1], segs[2], EMPTY]
    # a boundary exactly at the block seam (256 | 256), shuffled
    out["boundary_at_block_seam"] = [_shuffled(rng, M.random_segment(rng, 256, 3000, 50)) for _ in range(2)]
    out["segments50"] = [_shuffled(rng, M.random_segment(rng, int(rng.integers(0, 30)), 2000, 50)) if k % 7 else EMPTY for k in range(50)]
    out["spliced"] = [spliced_reads(rng, 900, 60000), EMPTY, spliced_reads(rng, 300, 20000)]
    out["shuffled_many"] = [_shuffled(rng, M.random_segment(rng, 5000, 400000, 150))]
    out["identical"] = [(np.full(700, 17, np.int32), np.full(700, 4000, np.int32))]
    # an interval over everything LAST, behind the short ones it covers (a carry into every piece when cut at positions)
    sh = rng.permutation(np.arange(2, 200000, 97))
    out["long_one_last"] = [_i32(np.concatenate([sh, [1]]), np.concatenate([sh + rng.integers(1, 90, len(sh)), [200100]]))]
    return out


def sorted_by_start(segs):
    out = []
    for s, f in segs:
        o = np.argsort(s, kind="stable")
        out.append((s[o], f[o]))
    return out


def is_unsorted(segs):
    return any(len(s) > 1 and bool(np.any(np.diff(s.astype(np.int64)) < 0)) for s, _ in segs)


def expected(segs):
    """(o_seg_off, start, finish, value) of the model over every segment sorted by start."""
    seg, s, f = M.flat(sorted_by_start(segs))
    return M.segmented(M.coverage, seg, s, f)


def pieces_case():
    """One 1.3e7-bp segment in any order between small ones, for a scratch budget of 1 MiB (5.6 Mbp a pass) on the device: three
    pieces, an interval across both cuts that comes last, spliced reads whose second component lies in a later piece than
    the read that follows them, a stretch of depth 0 across a cut."""
    rng = np.random.default_rng(22)
    a = spliced_reads(rng, 3000, 5400000)
    b = spliced_reads(rng, 3000, 5000000)
    b = (b[0] + 5700000, b[1] + 5700000)                 # (5.40 .. 5.70 Mbp: empty but for the long interval and the hops)
    hop_s = rng.integers(1000, 5000000, 200)             # components 6 Mbp to the right of the read they belong to
    s = np.concatenate([a[0], hop_s, b[0], hop_s + 6000000, [12990000, 2000]])
    f = np.concatenate([a[1], hop_s + 40, b[1], hop_s + 6000040, [13000000, 12000000]])
    big = _i32(s, f)
    small = [_shuffled(rng, M.random_segment(rng, 300, 2000000, 200)) for _ in range(4)]
    return small[:2] + [EMPTY, big, EMPTY] + small[2:]


def sam_fixtures():
    """tests/golden/sam_cover_fixtures.json: per case the covering components of a SAM text's reads in file order (one segment
    per stretch of one name) and what the compiled reference's SamReader popped over that text, as
    (name, segs, (o_seg_off, start, finish, value))."""
    import json
    with open(os.path.join(HERE, "golden", "sam_cover_fixtures.json")) as fh:
        cases = json.load(fh)["cases"]
    out = []
    for c in cases:
        off, s, f = c["seg_off"], np.array(c["start"], np.int32), np.array(c["finish"], np.int32)
        segs = [(s[off[g]:off[g + 1]], f[off[g]:off[g + 1]]) for g in range(len(off) - 1)]
        p = c["pops"]
        # the reference pops name stretch after name stretch: the offset of a stretch is where its name begins
        bounds = [0] + [k for k in range(1, len(p["chrom"])) if p["chrom"][k] != p["chrom"][k - 1]] + [len(p["chrom"])]
        assert [p["chrom"][k] for k in bounds[:-1]] == c["seg_name"] and c["unsorted_segments"] >= 1
        out.append((c["name"], segs, (np.array(bounds, np.int64), np.array(p["start"], np.int32), np.array(p["finish"], np.int32),
                                      np.array(p["value"], np.float64))))
    return out


# ---- the door with its flags on the CPU (tests/cover_any_emu.cpp) ----
_LIB = []


def emu_lib():
    if not _LIB:
        from emu import build
        so = build.build_lib(os.path.join(HERE, "emu", "libwt_cover_any_emu.so"), [os.path.join(HERE, "cover_any_emu.cpp")], libs=["-lm"])
        _LIB.append(C.CDLL(so))
    return _LIB[0]


def emu_coverage(seg_off, start, finish, flags, order=0, seed=0, capacity=None, budget=256 << 20):
    """Returns (rc, n_out, o_seg_off, start, finish, value, launches)."""
    L = emu_lib()
    seg_off = np.ascontiguousarray(seg_off, np.int64)
    start, finish = np.ascontiguousarray(start, np.int32), np.ascontiguousarray(finish, np.int32)
    cap = max(2 * len(start), 1) if capacity is None else capacity
    os_, of, ov = (np.zeros(max(cap, 1), dt) for dt in (np.int32, np.int32, np.float64))
    oseg = np.zeros(len(seg_off), np.int64)
    n_out, launches = C.c_int64(), C.c_int64()
    rc = L.cover_any_emu_coverage(C.c_int(order), C.c_uint64(seed), C.c_int64(len(seg_off) - 1), C.c_void_p(seg_off.ctypes.data),
                                  C.c_void_p(start.ctypes.data), C.c_void_p(finish.ctypes.data), C.c_int64(cap), C.c_void_p(os_.ctypes.data),
                                  C.c_void_p(of.ctypes.data), C.c_void_p(ov.ctypes.data), C.c_void_p(oseg.ctypes.data), C.byref(n_out),
                                  C.c_int64(budget), C.c_uint32(flags), C.byref(launches))
    m = min(n_out.value, cap)
    return rc, n_out.value, oseg, os_[:m], of[:m], ov[:m], launches.value
