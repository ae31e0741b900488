"""The reader's rule in plain Python (wtamd_text_runs, include/wiggletools_amd.h; the reference's WiggleReader, src/wigReader.c,
and BedReader, src/bedReader.c): line classes by regular expressions, the header state one line after the other, float() as a
correctly rounded strtod, the slow set from Python integers.  Also the cases every test of the read unit shares (cases(),
irregular_cases()), the fixtures recorded from the compiled reference (tests/golden/read_fixtures.json, written by
tests/golden/make_read_golden.py), and the ctypes side of tests/read_emu.cpp."""
import ctypes as C
import hashlib
import json
import os
import re
import struct

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "wiggletools_amd", "csrc")
HEADER = os.path.join(CSRC, "wt_read.h")
TILE = 4096
LINE_MAX = 4999
BED, EOF = 1, 2
M_BEDGRAPH, M_FIXED, M_VARIABLE = 0, 1, 2
OK, ERR_ARG, ERR_CAPACITY = 0, 1, 3
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
NAN_BITS = 0x7ff8000000000000
STATE_NAME = -1

INT = rb"-?(?:0|[1-9][0-9]*)"
NUM = rb"-?(?:(?:[0-9]+(?:\.[0-9]+)?|\.[0-9]+)(?:[eE][+-]?[0-9]{1,3})?|nan|inf)"
NAME = rb"[\x21-\xff]{1,255}"
RE_INT, RE_NUM, RE_NAME = (re.compile(b"(?:" + x + b")\\Z", re.S) for x in (INT, NUM, NAME))
RE_DEC = re.compile(rb"(-?)([0-9]*)(?:\.([0-9]*))?(?:[eE]([+-]?[0-9]+))?\Z")
RE_BED = re.compile(b"(" + NAME + b")[ \t]+(-?[0-9]*)[ \t]+(-?[0-9]*)(.*)\\Z", re.S)


def float_to_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def bits_to_float(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def number(tok):
    """(bits, slow) of a `number`, None if it is none.  float() is a correctly rounded strtod; the slow set is decided on
    Python integers: W above 2^53 or |E| above 22 (W != 0)."""
    if not RE_NUM.match(tok):
        return None
    neg = tok.startswith(b"-")
    body = tok[1:] if neg else tok
    if body == b"nan":
        return NAN_BITS | (neg << 63), False
    if body == b"inf":
        return 0x7ff0000000000000 | (neg << 63), False
    _, ip, fp, ex = RE_DEC.match(tok).groups()
    fp = (fp or b"").rstrip(b"0")
    digits = (ip + fp).lstrip(b"0")
    E = int(ex or b"0") - len(fp)
    if not digits:
        return neg << 63, False
    if len(digits) > 17 or int(digits) > 2 ** 53 or abs(E) > 22:
        return NAN_BITS, True
    return float_to_bits(float(tok.decode())), False


def integer(tok):
    if not RE_INT.match(tok) or len(tok) > 11:
        return None
    v = int(tok)
    return v if I32_MIN <= v <= I32_MAX else None


def fresh_state():
    return {"mode": 0, "span": 0, "step": 0, "last_start": 0, "next": 0, "chrom": b"", "rec_name": b""}


def header(line, fixed, newline=True):
    """{chrom, chrom_off (in the line), start, step, span} of a header line, None if it is irregular.  A chrom value that ends
    the line keeps the line's newline, as the reference's strtok leaves it (wigReader.c:43-62)."""
    p = 9 if fixed else 12
    seen = {}
    while p < len(line):
        if line[p:p + 1] not in (b" ", b"\t"):
            return None
        p += 1
        m = re.compile(rb"[^ \t]*").match(line, p)
        tok = m.group(0)
        if b"=" not in tok:
            return None
        key, val = tok.split(b"=", 1)
        allowed = (b"chrom", b"start", b"step", b"span") if fixed else (b"chrom", b"span")
        if key not in allowed or key in seen:
            return None
        if key == b"chrom":
            if not RE_NAME.match(val) or b"=" in val:
                return None
            if m.end() == len(line) and newline:
                val += b"\n"
                if len(val) > 255:
                    return None
            seen[key] = (val, p + 6)
        else:
            v = integer(val)
            if v is None or (key != b"start" and v < 1):
                return None
            seen[key] = v
        p = m.end()
    need = (b"chrom", b"start", b"step") if fixed else (b"chrom",)
    if any(k not in seen for k in need):
        return None
    return {"chrom": seen[b"chrom"][0], "chrom_off": seen[b"chrom"][1], "start": seen.get(b"start", 0), "step": seen.get(b"step", 0),
            "span": seen.get(b"span", 1)}


class Reading:
    """What the door returns for a text: rc, counts, and on success recs [(name, start, finish, value bits)], segs [(first
    record, name offset, name length)], slow [(record, offset)], state after."""


def read(data, flags=0, state=None):
    data = bytes(data)
    st0 = dict(state) if state else fresh_state()
    r = Reading()
    r.counts = {"n_lines": 0, "n_runs": 0, "n_seg": 0, "n_slow": 0, "n_irregular": 0, "first_irregular": -1, "n_unsorted": 0, "continues": 0}
    r.recs, r.segs, r.slow, r.state = [], [], [], st0
    r.rc = OK
    if flags & ~(BED | EOF):
        r.rc, r.counts = ERR_ARG, None
        return r
    if not data:
        return r
    if not data.endswith(b"\n") and not flags & EOF:
        r.rc, r.counts = ERR_ARG, None
        return r
    st = dict(st0)
    chrom_off = STATE_NAME
    bed = bool(flags & BED)
    off = 0
    lines = data.split(b"\n")
    if data.endswith(b"\n"):
        lines.pop()
    cn = r.counts
    for line in lines:
        s = off
        off += len(line) + 1
        cn["n_lines"] += 1
        rec = None                              # (name, name_off, start, finish, bits, slow, num_off)
        bad = False
        if len(line) == 0 or len(line) >= LINE_MAX:
            bad = True
        elif line[:1] == b"#":
            continue
        elif bed:
            m = RE_BED.match(line) if b"\r" not in line else None
            a, b = (integer(m.group(2)), integer(m.group(3))) if m else (None, None)
            if a is None or b is None or a >= I32_MAX or b >= I32_MAX or (b == 0 and m.group(4)[:1] in (b"x", b"X")):
                bad = True
            else:
                rec = (m.group(1), s, a + 1, b + 1, 0x3ff0000000000000, False, s)
        elif line.startswith(b"track"):
            continue
        elif line.startswith(b"variableStep") or line.startswith(b"fixedStep"):
            fixed = line.startswith(b"fixedStep")
            h = header(line, fixed, s + len(line) < len(data))
            if h is None:
                bad = True
            else:
                st.update(mode=M_FIXED if fixed else M_VARIABLE, span=h["span"], step=h["step"], next=h["start"] if fixed else 0, chrom=h["chrom"])
                chrom_off = s + h["chrom_off"]
                continue
        else:
            f = re.split(b"[ \t]", line)
            num = number(f[-1]) if b"\r" not in line else None
            num_off = s + len(line) - len(f[-1])
            if num is None or len(f) not in (1, 2, 4):
                bad = True
            elif len(f) == 4:
                a, b = integer(f[1]), integer(f[2])
                if not RE_NAME.match(f[0]) or a is None or b is None or a >= I32_MAX or b >= I32_MAX:
                    bad = True
                else:
                    rec = (f[0], s, a + 1, b + 1, num[0], num[1], num_off)
            elif len(f) == 2:
                a = integer(f[0])
                if a is None or st["mode"] != M_VARIABLE or a + st["span"] > I32_MAX:
                    bad = True
                else:
                    rec = (st["chrom"], chrom_off, a, a + st["span"], num[0], num[1], num_off)
            else:
                a = st["next"]
                if st["mode"] != M_FIXED or a > I32_MAX or a + st["span"] > I32_MAX or a < I32_MIN:
                    bad = True
                else:
                    rec = (st["chrom"], chrom_off, a, a + st["span"], num[0], num[1], num_off)
                    st["next"] += st["step"]
        if bad:
            if cn["n_irregular"] == 0:
                cn["first_irregular"] = s
            cn["n_irregular"] += 1
            continue
        name, name_off, a, b, bits, slow, num_off = rec
        if not bed and name_off == s:           # a bedGraph line (its own name) sets the mode
            st.update(mode=M_BEDGRAPH, span=0, step=0, next=0, chrom=b"")
            chrom_off = STATE_NAME
        have = bool(r.recs) or bool(st["rec_name"])
        if not r.recs:
            cn["continues"] = int(have and name == st["rec_name"])
        if not r.recs or name != st["rec_name"]:
            r.segs.append((len(r.recs), name_off, len(name)))
        if bed and have and (name < st["rec_name"] or (name == st["rec_name"] and a < st["last_start"])):
            cn["n_unsorted"] += 1
        if slow:
            r.slow.append((len(r.recs), num_off))
        r.recs.append((name, a, b, bits))
        st["rec_name"], st["last_start"] = name, a
    cn["n_runs"], cn["n_seg"], cn["n_slow"] = len(r.recs), len(r.segs), len(r.slow)
    if cn["n_irregular"] or cn["n_unsorted"]:
        r.rc = ERR_ARG
        r.recs, r.segs, r.slow = [], [], []
        return r
    r.state = st
    return r


def patched(data, r):
    """The records with the slow values through float(), as the caller patches them: [(name, start, finish, bits)]."""
    out = list(r.recs)
    for k, off in r.slow:
        end = data.index(b"\n", off) if b"\n" in data[off:] else len(data)
        n, a, b, _ = out[k]
        out[k] = (n, a, b, float_to_bits(float(data[off:end].decode())))
    return out


def compress(recs):
    """The reference's CompressionWiggleIterator (unaryOps.c:235-253) behind its reader: adjacent records of one name merge
    while start == the group's finish and (both NaN or |value - the value of the group's first| < 1e-6)."""
    out = []
    for n, a, b, bits in recs:
        x = bits_to_float(bits)
        if out and out[-1][0] == n and a == out[-1][2]:
            y = bits_to_float(out[-1][3])
            if (x != x and y != y) or abs(x - y) < 1e-6:
                out[-1] = (out[-1][0], out[-1][1], b, out[-1][3])
                continue
        out.append((n, a, b, bits))
    return out


# ---- the cases ----
def _pad_to(txt, target):
    """txt and a comment line that ends (its newline) at byte target - 1: the next line starts at `target`."""
    need = target - len(txt)
    assert need >= 2, (len(txt), target)
    return txt + b"#" + b"p" * (need - 2) + b"\n"


def _vals(n, k=0):
    return [((i * 37 + k) % 101) / 8.0 - 3.0 + (i % 2) * 0.0625 for i in range(n)]


def _bedgraph(n, seed, names=(b"chr1", b"chr2", b"chrX")):
    rng = np.random.default_rng(seed)
    cuts = sorted(rng.choice(np.arange(1, max(n, 2)), min(len(names) - 1, max(n - 1, 0)), replace=False).tolist()) if n > 1 else []
    out, p, g = [], 0, 0
    vals = _vals(n, seed)
    for i in range(n):
        if g < len(cuts) and i == cuts[g]:
            g, p = g + 1, 0
        p += int(rng.integers(0, 4))
        ln = int(rng.integers(1, 9))
        sep = b"\t" if i % 5 else b" "
        out.append(names[g] + sep + b"%d" % p + b"\t" + b"%d" % (p + ln) + sep + (b"%f" % vals[i] if i % 3 else repr(vals[i]).encode()) + b"\n")
        p += ln
    return b"".join(out)


def _mixed(n, seed):
    """n lines of every class: sections of fixedStep, variableStep and bedGraph with comments and track lines inside."""
    rng = np.random.default_rng(seed)
    out, vals, i = [], _vals(n, seed), 0
    names = [b"chr1", b"chr1", b"chr2", b"c", b"chr10"]
    k = 0
    while len(out) < n:
        kind = k % 3
        name = names[k % len(names)]
        m = int(rng.integers(1, 700 if n > 1000 else 40))
        k += 1
        if kind == 0:
            span = int(rng.integers(1, 4))
            out.append(b"fixedStep chrom=" + name + b" start=%d step=%d" % (int(rng.integers(1, 1000)), int(rng.integers(1, 5))) +
                       (b" span=%d" % span if span > 1 else b"") + b"\n")
        elif kind == 1:
            out.append(b"variableStep chrom=" + name + (b"\tspan=3" if k % 2 else b"") + b"\n")
        p = 1
        for j in range(m):
            if len(out) >= n:
                break
            v = b"%f" % vals[i % len(vals)] if j % 4 else repr(vals[i % len(vals)]).encode()
            i += 1
            if j % 50 == 17:
                out.append(b"# a comment inside\n" if j % 100 == 17 else b"track type=wiggle_0 name=x\n")
                continue
            if kind == 0:
                out.append(v + b"\n")
            elif kind == 1:
                p += int(rng.integers(3, 9))
                out.append(b"%d" % p + (b" " if j % 3 else b"\t") + v + b"\n")
            else:
                p += int(rng.integers(0, 5))
                out.append(name + b"\t%d\t%d\t" % (p, p + 2) + v + b"\n")
                p += 2
    return b"".join(out[:n])


NUMBERS = [b"9007199254740992", b"9007199254740993", b"-9007199254740992", b"9007199254740992e22", b"9007199254740991e-22", b"1e22", b"1e-22", b"1e23",
           b"1e-23", b"123e20", b"123e-25", b"1234567890123456789", b"12345678901234567890", b"0.1234567890123456789", b"1.500000", b"100.000",
           b"0.000001", b"-0.000000", b"0.000000", b"nan", b"-nan", b"inf", b"-inf", b"4.9e-324", b"1e-310", b"1e400", b"-1e999", b"2.5E+3", b".5",
           b"-.25e-2", b"0e999", b"00012.5000", b"1e022", b"0.1", b"0.3", b"1234.5678e-10", b"3.141592653589793", b"2.2250738585072014e-308",
           b"1.7976931348623157e308", b"0.000000000000000000000001", b"10000000000000000000000", b"1e0", b"7", b"-7.125", b"123456.789000",
           b"0.30000000000000004", b"9007199254740993e-5", b"8.5e-22", b"4503599627370497.5", b"5e-1", b"0.5e1", b"000.000e-000"]


def cases():
    """{name: (text, flags)}: regular texts, the smallest shapes at which each pass can go wrong."""
    out = {}
    for n in (1, 255, 256, 257):
        out["bedgraph_%d" % n] = (_bedgraph(n, 100 + n), 0)
        out["mixed_%d" % n] = (_mixed(n, 200 + n), 0)
    out["mixed_20001"] = (_mixed(20001, 7), 0)
    # more than 256 lines in a tile (several rounds), a header in the middle of a round and as a round's last line
    short = b"fixedStep chrom=chr1 start=1 step=1\n" + b"".join(b"%d\n" % (i % 10) for i in range(254)) + b"fixedStep chrom=chr2 start=5 step=2 span=2\n"
    short += b"".join(b"%d\n" % (i % 7) for i in range(3000)) + b"variableStep chrom=chr2\n" + b"".join(b"%d %d\n" % (10 + 2 * i, i % 9) for i in range(600))
    out["short_lines"] = (short, 0)
    # a line across a tile boundary: its newline the last byte of a tile, and the first byte of the next; a header that is the
    # last line of a tile; a section over three tiles with comments and track lines inside
    bg = b"chr1\t10\t20\t1.5\n"
    t = _pad_to(b"", TILE - len(bg)) + bg + bg
    assert t[TILE - 1:TILE] == b"\n"
    out["newline_last_byte"] = (t, 0)
    t = _pad_to(b"", TILE - len(bg) + 1) + bg + b"chr1\t20\t30\t2.5\n"
    assert t[TILE:TILE + 1] == b"\n"
    out["newline_first_byte"] = (t, 0)
    t = _pad_to(bg, TILE - 7) + b"chr2\t100\t200\t-3.25\n" + bg.replace(b"chr1", b"chr2").replace(b"10\t20", b"300\t400")
    out["line_straddles"] = (t, 0)
    hdr = b"fixedStep chrom=chr7 start=100 step=10 span=5\n"
    t = _pad_to(b"chr1\t1\t2\t3\n", TILE - len(hdr)) + hdr + b"1.25\n2.5\n"
    assert t[TILE - 1:TILE] == b"\n"
    out["header_ends_tile"] = (t, 0)
    t = _pad_to(b"", TILE - 20) + hdr + b"1.25\n2.5\n"
    out["header_straddles"] = (t, 0)
    sec = [hdr]
    for i in range(1100):
        sec.append(b"%f\n" % (i / 8.0))
        if i % 97 == 5:
            sec.append(b"# not a data line\n")
        if i % 211 == 7:
            sec.append(b"track name=inside\n")
    t = b"".join(sec)
    assert len(t) > 2 * TILE + 100
    out["section_three_tiles"] = (t + b"variableStep chrom=chr7 span=2\n5 1\n9 2\n", 0)
    out["span_defaults"] = (b"variableStep chrom=chr1 span=5\n10 1\n20 2\nvariableStep chrom=chr1\n30 3\nfixedStep chrom=chr1 start=50 step=2 span=2\n1\n2\n"
                            b"fixedStep chrom=chr1 start=60 step=3\n4\n5\n", 0)
    out["two_headers"] = (b"fixedStep chrom=chr1 start=1 step=1\nvariableStep chrom=chr2\n5 1\nvariableStep chrom=chr3\nfixedStep chrom=chr4 start=9 step=9\n7\n8\n", 0)
    out["same_chrom_headers"] = (b"fixedStep chrom=chr1 start=1 step=1\n1\n2\nfixedStep chrom=chr1 start=10 step=1\n3\nvariableStep chrom=chr1\n20 4\n"
                                 b"chr1\t30\t40\t5\nchr1\t40\t50\t6\nfixedStep chrom=chr1 start=100 step=1\n7\n", 0)
    out["bedgraph_after_fixed"] = (b"fixedStep chrom=chr1 start=1 step=1\n1\n2\nchr1\t5\t6\t3\nchr2\t5\t6\t4\nvariableStep chrom=chr2\n9 5\nchr3\t1\t2\t6\n", 0)
    out["chrom_changes"] = (b"".join(b"chr%d\t%d\t%d\t%d.5\n" % (c, p, p + 3, c + p) for c in (1, 2, 10, 3) for p in (0, 3, 10)) +
                            b"chr1\t0\t5\t1\n", 0)
    long_name = b"N" * 255
    out["names"] = (b"c\t1\t2\t1\nc\t2\t3\t2\n" + long_name + b"\t1\t2\t3\nfixedStep chrom=" + long_name + b" start=1 step=1\n4\nfixedStep chrom=d start=1 step=1\n5\n"
                    b"a=b\t1\t2\t6\n\xe9\xff\t1\t2\t7\n", 0)
    out["coordinates"] = (b"chr1\t-2147483648\t-2147483647\t1\nchr1\t-1\t0\t2\nchr1\t0\t2147483646\t3\nchr1\t2147483646\t2147483646\t4\n"
                          b"variableStep chrom=chr2 span=1\n-2147483648 5\n2147483646 6\nfixedStep chrom=chr3 start=2147483645 step=1\n7\n8\n"
                          b"fixedStep chrom=chr3 start=-2147483648 step=2147483647 span=1\n9\n10\n11\n-0 12\n", 0)
    out["coordinates"] = (out["coordinates"][0].replace(b"-0 12\n", b"variableStep chrom=chr4\n-0 12\n"), 0)
    out["long_comment"] = (b"chr1\t1\t2\t3\n#" + b"c" * 4997 + b"\nchr1\t2\t3\t4\ntrack" + b"t" * 4993 + b"\nchr1\t3\t4\t5\n", 0)
    digits = b"".join(b"%d" % ((i * 7) % 10) for i in range(4980))
    out["long_number"] = (b"fixedStep chrom=chr1 start=1 step=1\n0." + b"0" * 4990 + b"1e999\n" + b"1" + b"0" * 4997 + b"\n" + b"0" * 4997 + b"7\n"
                          b"chr1\t5\t6\t1." + digits + b"\n", 0)
    out["values"] = (b"fixedStep chrom=chr1 start=1 step=1\n" + b"".join(v + b"\n" for v in NUMBERS) + b"variableStep chrom=chr1\n" +
                     b"".join(b"%d\t" % (1000 + 2 * i) + v + b"\n" for i, v in enumerate(NUMBERS)) +
                     b"".join(b"chrV\t%d\t%d " % (3 * i, 3 * i + 1) + v + b"\n" for i, v in enumerate(NUMBERS)), 0)
    out["no_final_newline"] = (b"chr1\t1\t2\t3\nchr1\t2\t3\t4.5", EOF)
    out["no_final_newline_fixed"] = (_pad_to(b"fixedStep chrom=chr1 start=1 step=1\n", TILE - 2) + b"1\n2\n33", EOF)
    out["eof_flag_with_newline"] = (b"chr1\t1\t2\t3\n", EOF)
    out["only_comments"] = (b"# nothing\ntrack x\n#\n", 0)
    out["header_only"] = (b"# nothing\nfixedStep chrom=chr9 start=7 step=3 span=2\n", 0)
    out["many_tiles"] = (b"".join(b"#" + b"z" * 3990 + b"\n" + b"chr%d\t%d\t%d\t%d\n" % (i // 100, i, i + 1, i) for i in range(300)), 0)
    # BED
    out["bed_basic"] = (b"# a bed file\nchr1\t1\t10\nchr1 1 5 name 0 +\nchr1\t \t3\t4\tx\nchr1\t3\t3\nchr1\t7\t20abc\nchr2\t0\t1\ttrack\nchr2\t0\t100\n"
                        b"track\t5\t6\n", BED)
    out["bed_257"] = (b"".join(b"chr%d\t%d\t%d\tn%d\t0\t-\n" % (1 + i // 100, (i % 100) * 5, (i % 100) * 5 + 30 - (i % 7), i) for i in range(257)), BED)
    out["bed_straddle"] = (_pad_to(b"chr1\t1\t2\n", TILE - 4) + b"chr1\t5\t9\nchr1\t5\t6\nchr1\t6\t6\n", BED)
    out["bed_eof"] = (b"chr1\t1\t2\nchr1\t1\t2", BED | EOF)
    return out


def irregular_lines():
    """[(what, line, flags, context)]: one irregular line of every class; context: the regular lines in front of it."""
    var, fix = b"variableStep chrom=chr1\n5 1\n", b"fixedStep chrom=chr1 start=1 step=1\n1\n"
    bg = b"chr1\t1\t2\t3\n"
    L = [("a carriage return", b"chr1\t5\t6\t1\r", 0, bg), ("an empty line", b"", 0, bg), ("4999 bytes", b"#" + b"x" * 4998, 0, bg),
         ("a double separator", b"chr1\t5\t\t6\t1", 0, bg), ("a leading blank", b" 7", 0, fix), ("a trailing tab", b"7\t", 0, fix),
         ("three fields", b"chr1 5 6", 0, bg), ("five fields", b"chr1 5 6 7 8", 0, bg), ("an unknown key", b"fixedStep chrom=c start=1 step=1 stop=2", 0, bg),
         ("step 0", b"fixedStep chrom=c start=1 step=0", 0, bg), ("span 0", b"variableStep chrom=c span=0", 0, bg),
         ("a keyword that goes on", b"fixedStepX chrom=c start=1 step=1", 0, bg), ("a keyword alone", b"variableStep", 0, bg),
         ("a missing step", b"fixedStep chrom=c start=1", 0, bg), ("a key twice", b"variableStep chrom=c chrom=d", 0, bg),
         ("step on variableStep", b"variableStep chrom=c step=2", 0, bg), ("two blanks in a header", b"fixedStep  chrom=c start=1 step=1", 0, bg),
         ("chrom with '='", b"variableStep chrom=a=b", 0, bg), ("an octal int", b"chr1\t010\t20\t1", 0, bg), ("a hex int", b"chr1\t0x10\t20\t1", 0, bg),
         ("a plus sign", b"chr1\t+5\t20\t1", 0, bg), ("an int above int32", b"chr1\t5\t2147483647\t1", 0, bg), ("eleven digits", b"chr1\t5\t12345678901\t1", 0, bg),
         ("four exponent digits", b"1e5555", 0, fix), ("a dot without digits", b"1.", 0, fix), ("NaN in capitals", b"NaN", 0, fix), ("a comma", b"1,5", 0, fix),
         ("two fields under fixedStep", b"7 1", 0, fix), ("one field under variableStep", b"7", 0, var), ("one field at the start", b"7", 0, b""),
         ("one field after bedGraph", b"7", 0, fix + bg), ("a name of 256 bytes", b"N" * 256 + b"\t1\t2\t3", 0, bg),
         ("fixedStep beyond int32", b"1", 0, b"fixedStep chrom=c start=2147483646 step=1\n1\n"), ("variableStep span beyond int32", b"2147483647 1", 0, var),
         ("a bed line without ints", b"chr1\tx\t5", BED, b"chr1\t1\t2\n"), ("a bed line with one int", b"chr1\t7", BED, b"chr1\t1\t2\n"),
         ("a bed hex", b"chr1\t7\t0x10", BED, b"chr1\t1\t2\n"), ("a bed leading blank", b" chr1\t7\t8", BED, b"chr1\t1\t2\n"),
         ("a bed carriage return", b"chr1\t7\t8\r", BED, b"chr1\t1\t2\n"), ("an empty bed line", b"", BED, b"chr1\t1\t2\n")]
    return L


def irregular_cases():
    """{name: (text, flags, byte offset of the irregular line)}: every irregular line as the first and as the last line."""
    out = {}
    for what, line, flags, ctx in irregular_lines():
        tail = b"chr1\t100\t200\t1\n" if not flags else b"chr1\t100\t200\n"
        out[what + " / last"] = (ctx + line + b"\n", flags, len(ctx))
        if not ctx.startswith((b"fixedStep", b"variableStep")) and what != "one field at the start":
            out[what + " / first"] = (line + b"\n" + tail, flags, 0)
        else:
            out[what + " / before a tail"] = (ctx + line + b"\n" + tail, flags, len(ctx))
    out["one field at the start / first"] = (b"7\nchr1\t1\t2\t3\n", 0, 0)
    return out


# BED lines on which the reference's sscanf converts fewer than three fields: it goes on with uninitialised locals, so what it
# pops is whatever its stack held -- recorded as undefined, compared nowhere
UNDEFINED_IN_REFERENCE = ("a bed line without ints", "a bed line with one int", "an empty bed line")


def unsorted_cases():
    """{name: (text, number of records before their predecessor)}"""
    return {"a lower start": (b"chr1\t5\t6\nchr1\t4\t9\nchr1\t4\t5\n", 1), "a lower name": (b"chr2\t5\t6\nchr10\t7\t9\nchr10\t1\t2\nchr3\t0\t1\n", 2),
            "across a tile": (_pad_to(b"chr1\t50\t60\n", TILE) + b"chr1\t49\t70\n", 1)}


def seek_cases():
    """{case/what: (pops before, chrom, start, finish)}: seeks forwards, backwards, into and across chromosomes, past the end."""
    return {"chrom_changes/fresh": (0, b"chr2", 2, 9), "chrom_changes/backwards": (7, b"chr1", 1, 100), "chrom_changes/forwards": (1, b"chr10", 5, 12),
            "chrom_changes/after the end": (40, b"chr2", 1, 5), "mixed_257/inside": (3, b"chr1", 30, 60), "mixed_257/a later chromosome": (0, b"chr2", 1, 100000),
            "same_chrom_headers/clip": (0, b"chr1", 11, 45), "bedgraph_257/forwards": (20, b"chr2", 10, 400), "bedgraph_257/backwards": (200, b"chr1", 50, 300),
            "bed_257/a later chromosome": (0, b"chr2", 1, 140), "bed_257/backwards": (150, b"chr1", 1, 60), "bed_basic/fresh": (0, b"chr1", 1, 8),
            "section_three_tiles/inside": (0, b"chr7", 5000, 9000), "short_lines/forwards": (2, b"chr2", 601, 900)}


# ---- fixtures ----
def fixtures():
    return json.load(open(os.path.join(HERE, "golden", "read_fixtures.json")))


def records_digest(recs):
    h = hashlib.sha256()
    for n, a, b, bits in recs:
        h.update(n + b"\0" + struct.pack("<iiQ", a, b, bits))
    return h.hexdigest()


def as_fixture(recs):
    """The form a record list takes in the fixtures: whole up to 300 records, else a digest and the ends."""
    rows = [[n.decode("latin-1"), a, b, "%016x" % bits] for n, a, b, bits in recs]
    out = {"n": len(rows), "sha256": records_digest(recs)}
    if len(rows) <= 300:
        out["records"] = rows
    else:
        out["head"], out["tail"] = rows[:8], rows[-8:]
    return out


def reference_reading(data, flags):
    """What the reference's reader pops for a regular text, by the model: compressed for a wig reader, as it is for BED."""
    r = read(data, flags)
    assert r.rc == OK
    recs = patched(data, r)
    return recs if flags & BED else compress(recs)


# ---- the emulated passes and the host sweep ----
_LIB = None


def emu_lib():
    """tests/emu/libwt_read_emu.so (tests/read_emu.cpp), built by tests/emu/build.py's build_lib and loaded once."""
    global _LIB
    if _LIB is None:
        from emu import build
        _LIB = C.CDLL(build.build_lib(os.path.join(build.HERE, "libwt_read_emu.so"), [os.path.join(HERE, "read_emu.cpp")], libs=["-lm"]))
    return _LIB


class State(C.Structure):
    _fields_ = [("mode", C.c_int32), ("span", C.c_int32), ("step", C.c_int32), ("last_start", C.c_int32), ("next", C.c_int64),
                ("chrom_len", C.c_int32), ("rec_len", C.c_int32), ("chrom", C.c_char * 256), ("rec_name", C.c_char * 256)]

    def as_dict(self):
        return {"mode": int(self.mode), "span": int(self.span), "step": int(self.step), "last_start": int(self.last_start), "next": int(self.next),
                "chrom": self.chrom[:self.chrom_len], "rec_name": self.rec_name[:self.rec_len]}

    @classmethod
    def from_dict(cls, d):
        st = cls()
        if d:
            st.mode, st.span, st.step, st.last_start, st.next = d["mode"], d["span"], d["step"], d["last_start"], d["next"]
            st.chrom_len, st.rec_len = len(d["chrom"]), len(d["rec_name"])
            st.chrom, st.rec_name = d["chrom"], d["rec_name"]
        return st


class Counts(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("n_lines", "n_runs", "n_seg", "n_slow", "n_irregular", "first_irregular", "n_unsorted", "continues")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


CANARY = 0x5C
GUARD = 8
KEYS = {"start": np.int32, "finish": np.int32, "value": np.uint64, "seg_off": np.int64, "seg_name_off": np.int64, "seg_name_len": np.int32,
        "slow_rec": np.int64, "slow_off": np.int64}


def host_door(which, order=0, seed=7):
    """door(data, flags, state, capacity, seg_capacity, slow_capacity, offset) -> the dict of engine._read_door, over HOST arrays:
    which "emu" (the passes through the CPU launcher) or "host" (the host sweep)."""
    def door(data, flags=0, state=None, capacity=None, seg_capacity=None, slow_capacity=None, offset=0):
        lib = emu_lib()
        raw = np.full(offset + len(data) + 64, CANARY, np.uint8)
        raw[offset:offset + len(data)] = np.frombuffer(bytes(data), np.uint8)
        model = read(data, flags, state)
        cn0 = model.counts or {"n_runs": 0, "n_seg": 0, "n_slow": 0}
        capacity = cn0["n_runs"] if capacity is None else capacity
        seg_capacity = cn0["n_seg"] if seg_capacity is None else seg_capacity
        slow_capacity = cn0["n_slow"] if slow_capacity is None else slow_capacity
        sizes = {"start": capacity, "finish": capacity, "value": capacity, "seg_off": seg_capacity + 1, "seg_name_off": seg_capacity,
                 "seg_name_len": seg_capacity, "slow_rec": slow_capacity, "slow_off": slow_capacity}
        bufs = {k: np.frombuffer(bytes([CANARY]) * ((n + 2 * GUARD) * np.dtype(KEYS[k]).itemsize), KEYS[k]).copy() for k, n in sizes.items()}
        p = lambda k: C.c_void_p(bufs[k].ctypes.data + GUARD * bufs[k].itemsize)      # noqa: E731
        st, cn = State.from_dict(state), Counts(*([-1] * 8))
        head = (C.c_int(order), C.c_uint64(seed)) if which == "emu" else ()
        tail = (None,) if which == "emu" else ()
        fn = lib.read_emu_door if which == "emu" else lib.read_host
        rc = fn(*head, C.c_void_p(raw.ctypes.data + offset), C.c_int64(len(data)), C.c_uint32(flags), C.byref(st), p("start"), p("finish"), p("value"),
                C.c_int64(capacity), p("seg_off"), p("seg_name_off"), p("seg_name_len"), C.c_int64(seg_capacity), p("slow_rec"), p("slow_off"),
                C.c_int64(slow_capacity), C.byref(cn), *tail)
        out = {"rc": rc, "counts": cn.as_dict(), "state": st.as_dict()}
        for k, n in sizes.items():
            out[k] = bufs[k][GUARD:GUARD + n]
            out[k + "_lo"], out[k + "_hi"] = bufs[k][:GUARD].view(np.uint8), bufs[k][GUARD + n:].view(np.uint8)
        out["text_guard"] = raw[offset + len(data):]
        return out
    return door


def number_c(tok):
    """The header's number parser on one numeral: None, or (bits, slow)."""
    bits = C.c_uint64(0)
    k = emu_lib().read_number(C.c_char_p(bytes(tok)), C.c_int64(len(tok)), C.byref(bits))
    return None if k == 0 else (int(bits.value) if k == 1 else NAN_BITS, k == 2)


# ---- checks every door's tests share ----
def guards_intact(out):
    return all((out[k + "_lo"] == CANARY).all() and (out[k + "_hi"] == CANARY).all() for k in KEYS) and bool((out["text_guard"] == CANARY).all())


def nothing_written(out):
    return guards_intact(out) and all((out[k].view(np.uint8) == CANARY).all() for k in KEYS)


def state_of(d):
    return dict(d or fresh_state())


def check_reading(out, data, flags, state, what, host_values=False):
    """`out` (a door's) is the model's reading of the text, exactly.  host_values: the door has patched the slow values itself
    (the host sweep)."""
    m = read(data, flags, state)
    assert m.rc == OK, what
    assert out["rc"] == OK, (what, out["rc"], out["counts"])
    assert out["counts"] == m.counts, (what, out["counts"], m.counts)
    n, g, k = m.counts["n_runs"], m.counts["n_seg"], m.counts["n_slow"]
    recs = patched(data, m) if host_values else m.recs
    assert out["start"][:n].tolist() == [r[1] for r in recs], what
    assert out["finish"][:n].tolist() == [r[2] for r in recs], what
    got = out["value"][:n].view(np.uint64).tolist()
    want = [r[3] for r in recs]
    if got != want:
        i = next(i for i in range(n) if got[i] != want[i])
        raise AssertionError((what, "value of record", i, "%016x" % got[i], "%016x" % want[i]))
    assert out["seg_off"][:g + (1 if n else 0)].tolist() == [s[0] for s in m.segs] + ([n] if n else []), what
    assert out["seg_name_off"][:g].tolist() == [s[1] for s in m.segs], (what, out["seg_name_off"][:g].tolist(), [s[1] for s in m.segs])
    assert out["seg_name_len"][:g].tolist() == [s[2] for s in m.segs], what
    assert out["slow_rec"][:k].tolist() == [s[0] for s in m.slow] and out["slow_off"][:k].tolist() == [s[1] for s in m.slow], what
    assert out["state"] == m.state, (what, out["state"], m.state)
    assert guards_intact(out), what
    # whatever lies beyond the counts is untouched
    for key, used in (("start", n), ("finish", n), ("value", n), ("seg_off", g + (1 if n else 0)), ("seg_name_off", g), ("seg_name_len", g), ("slow_rec", k),
                      ("slow_off", k)):
        assert (out[key][used:].view(np.uint8) == CANARY).all(), (what, key)
    return m


def cut_points(data):
    """Offsets of line starts to cut a text at: after a header, inside a fixedStep section, between chromosomes, at tile edges,
    and one cut twice (an empty chunk)."""
    starts = [0] + [i + 1 for i, ch in enumerate(data[:-1]) if ch == 10]
    cuts = set()
    for i, s in enumerate(starts[1:], 1):
        prev = data[starts[i - 1]:s]
        if prev.startswith((b"fixedStep", b"variableStep")):
            cuts.add(s)
    picks = sorted(cuts)[:3]
    picks += [starts[len(starts) // 3], starts[2 * len(starts) // 3]]
    for edge in range(TILE, len(data), TILE):
        picks.append(min(starts, key=lambda s: abs(s - edge)))
        if len(picks) > 9:
            break
    picks = sorted(set(p for p in picks if 0 < p < len(data)))
    return sorted(picks + picks[:1])


def check_chained(door, data, flags, what):
    """The text cut at line starts and chained through the state is the whole: records, segments (a chunk's first segment
    joined to the one before where `continues` says so), slow list and state."""
    whole = read(data, flags)
    assert whole.rc == OK
    cuts = cut_points(data)
    edges = [0] + cuts + [len(data)]
    st = fresh_state()
    recs, seg_names, slow = [], [], []
    for a, b in zip(edges[:-1], edges[1:]):
        piece = data[a:b]
        fl = flags if b == len(data) else flags & ~EOF
        out = door(piece, fl, state=st)
        check_reading(out, piece, fl, st, (what, a, b))
        n, g, k = (out["counts"][x] for x in ("n_runs", "n_seg", "n_slow"))
        segs = [(int(out["seg_off"][i]), int(out["seg_name_off"][i]), int(out["seg_name_len"][i])) for i in range(g)]
        for i, (first, off, ln) in enumerate(segs):
            name = st["chrom"] if off == STATE_NAME else piece[off:off + ln]
            if not (i == 0 and out["counts"]["continues"]):
                seg_names.append((len(recs) + first, name))
        end = [s[0] for s in segs[1:]] + [n]
        for (first, off, ln), e in zip(segs, end):
            name = st["chrom"] if off == STATE_NAME else piece[off:off + ln]
            for i in range(first, e):
                recs.append((name, int(out["start"][i]), int(out["finish"][i]), int(out["value"][i])))
        slow += [(len(recs) - n + int(r), a + int(o)) for r, o in zip(out["slow_rec"][:k], out["slow_off"][:k])]
        st = out["state"]
    assert recs == whole.recs, what
    assert seg_names == [(s[0], whole.recs[s[0]][0]) for s in whole.segs], what
    assert slow == whole.slow, what
    assert st == whole.state, (what, st, whole.state)


def check_refusals(door):
    """Every refusal writes nothing and leaves the state untouched; irregular and unsorted texts report their counts."""
    st0 = {"mode": M_FIXED, "span": 2, "step": 3, "last_start": 40, "next": 77, "chrom": b"chr1", "rec_name": b"chr1"}
    for name, (data, flags, where) in irregular_cases().items():
        for st in (None, st0):
            if st is not None and name.startswith("one field"):
                continue
            out = door(data, flags, state=st, capacity=64, seg_capacity=64, slow_capacity=64, offset=3)
            m = read(data, flags, st)
            assert m.rc == ERR_ARG and m.counts["n_irregular"] == 1 and m.counts["first_irregular"] == where, (name, m.counts)
            assert out["rc"] == ERR_ARG, (name, out["rc"], out["counts"])
            assert (out["counts"]["n_lines"], out["counts"]["n_irregular"], out["counts"]["first_irregular"]) == (m.counts["n_lines"], 1, where), (name, out["counts"])
            assert nothing_written(out) and out["state"] == state_of(st), name
    for name, (data, n_unsorted) in unsorted_cases().items():
        out = door(data, BED, state=None, capacity=64, seg_capacity=64, slow_capacity=64)
        m = read(data, BED)
        assert m.counts["n_unsorted"] == n_unsorted, (name, m.counts)
        assert out["rc"] == ERR_ARG and out["counts"] == m.counts, (name, out["counts"], m.counts)
        assert nothing_written(out) and out["state"] == fresh_state(), name
    # a BED record before the state's last record
    st = dict(fresh_state(), rec_name=b"chr2", last_start=50)
    for data, bad in ((b"chr2\t48\t60\n", 1), (b"chr10\t90\t95\n", 1), (b"chr2\t49\t60\n", 0), (b"chr3\t0\t1\n", 0)):
        out = door(data, BED, state=st, capacity=4, seg_capacity=4, slow_capacity=4)
        assert out["counts"]["n_unsorted"] == bad and out["rc"] == (ERR_ARG if bad else OK), (data, out["counts"])
    bg = b"chr1\t1\t2\t3\nchr1\t2\t3\t4\n"
    for what, data, flags in (("an unknown flag", bg, 4), ("an unknown flag beside the known", bg, 8 | BED), ("no final newline", bg[:-1], 0),
                              ("no final newline, BED", b"chr1\t1\t2", BED)):
        out = door(data, flags, state=st0, capacity=64, seg_capacity=64, slow_capacity=64)
        assert out["rc"] == ERR_ARG and nothing_written(out) and out["state"] == st0, what
        assert out["counts"] == {k: -1 for k in out["counts"]}, what


def check_capacities(door, data, flags, what):
    m = read(data, flags)
    n, g, k = m.counts["n_runs"], m.counts["n_seg"], m.counts["n_slow"]
    assert n > 1 and g > 1 and k > 1, what
    for caps in ((n - 1, g, k), (n, g - 1, k), (n, g, k - 1), (0, 0, 0)):
        out = door(data, flags, state=None, capacity=caps[0], seg_capacity=caps[1], slow_capacity=caps[2], offset=1)
        assert out["rc"] == ERR_CAPACITY, (what, caps, out["rc"])
        assert out["counts"] == m.counts, (what, caps)
        assert nothing_written(out) and out["state"] == fresh_state(), (what, caps)
    out = door(data, flags, state=None, capacity=n + 5, seg_capacity=g + 5, slow_capacity=k + 5)
    check_reading(out, data, flags, None, what)


def check_empty(door):
    st0 = {"mode": M_VARIABLE, "span": 2, "step": 0, "last_start": 40, "next": 0, "chrom": b"chr1", "rec_name": b"chrZ"}
    out = door(b"", 0, state=st0, capacity=4, seg_capacity=4, slow_capacity=4)
    assert out["rc"] == OK and nothing_written(out) and out["state"] == st0
    assert out["counts"] == {"n_lines": 0, "n_runs": 0, "n_seg": 0, "n_slow": 0, "n_irregular": 0, "first_irregular": -1, "n_unsorted": 0, "continues": 0}


def fuzz_numerals(n, seed=11):
    """n numerals: every digit count 1 .. 20, exponents -30 .. 30, W at the boundary, fractions with trailing zeros."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        nd = 1 + i % 20
        digits = "".join(str(int(d)) for d in rng.integers(0, 10, nd))
        if i % 7 == 0:
            digits = str(2 ** 53 + int(rng.integers(-2, 3)))
        cut = int(rng.integers(0, len(digits) + 1))
        s = digits[:cut] + ("." + digits[cut:] if cut < len(digits) else "")
        if s.startswith("."):
            s = ("0" if i % 2 else "") + s
        if i % 3:
            s += ("e" if i % 2 else "E") + ("%+d" if i % 5 else "%d") % int(rng.integers(-30, 31))
        out.append((("-" if i % 4 == 0 else "") + s).encode())
    return out
