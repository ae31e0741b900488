"""What tests/test_mtext_dropin_host.py (the emulated drop-in library: the host sweep) and tests/test_mtext_dropin_gpu.py (the
product) share: a ctypes driver of wtamd_TeeMultiplexer, wtamd_toStdoutMultiplexer and wtamd_PasteMultiplexer over this
library's Multiplexer and over wtamd_ApplyMultiplexer -- the file against the text of tests/mtext_model.py of the rows the same
Multiplexer serves without a writer.  Run as a program (python mtext_dropin.py stdout|short LIBRARY [DIR]) it is the child
process of the two checks that need one: the text on stdout, and the infile one line short, which ends in exit(1)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [HERE, os.path.dirname(HERE)]

import apply_dropin  # noqa: E402
import mtext_model as M  # noqa: E402

SHORT_MESSAGE = "Could not paste data to file lines, inconsistent number of lines.\n"


class DropIn(apply_dropin.DropIn):
    def __init__(self, path):
        super().__init__(path)
        L = self.L
        L.wtamd_TeeMultiplexer.restype = C.c_void_p
        L.wtamd_TeeMultiplexer.argtypes = [C.c_void_p, C.c_void_p, C.c_char, C.c_char]
        L.wtamd_PasteMultiplexer.restype = C.c_void_p
        L.wtamd_PasteMultiplexer.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char]
        L.wtamd_toStdoutMultiplexer.restype = None
        L.wtamd_toStdoutMultiplexer.argtypes = [C.c_void_p, C.c_char, C.c_char]
        self.libc = C.CDLL(None)
        self.libc.fopen.restype = C.c_void_p
        self.libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
        self.libc.fclose.argtypes = [C.c_void_p]

    def fopen(self, path, mode=b"w"):
        fp = self.libc.fopen(str(path).encode(), mode)
        assert fp
        return fp

    def tracks(self, rl):
        """This library's Multiplexer over the tracks of a RunLists (wtamd_ArrayReader children, float32 values)."""
        kids = []
        for i in range(rl.n_tracks):
            seg, idx = [0], []
            for c in range(rl.n_chrom):
                a, b = int(rl.seg_off[c * rl.n_tracks + i]), int(rl.seg_off[c * rl.n_tracks + i + 1])
                idx += range(a, b)
                seg.append(seg[-1] + b - a)
            arr = (C.c_char_p * rl.n_chrom)(*[n.encode() for n in rl.chrom_names])
            so = np.ascontiguousarray(seg, np.int64)
            s, f, v = (np.ascontiguousarray(x[idx], dt) for x, dt in ((rl.start, np.int32), (rl.finish, np.int32), (rl.value, np.float32)))
            self.keep.append((arr, so, s, f, v))
            kids.append(self.L.wtamd_ArrayReader(rl.n_chrom, arr, so.ctypes.data, s.ctypes.data, f.ctypes.data, v.ctypes.data, float(rl.defaults[i])))
        arr = (C.c_void_p * len(kids))(*kids)
        self.keep.append(arr)
        return self.L.newMultiplexer(arr, len(kids), b"\x00")

    def tee(self, m, path, bed, hold=False):
        fp = self.fopen(path)
        return self.L.wtamd_TeeMultiplexer(m, fp, b"\x01" if bed else b"\x00", b"\x01" if hold else b"\x00"), fp

    def paste(self, m, infile, path, hold=False):
        fin, fp = self.fopen(infile, b"r"), self.fopen(path)
        return self.L.wtamd_PasteMultiplexer(m, fin, fp, b"\x01" if hold else b"\x00"), fp

    def written(self, fp, path):
        self.libc.fclose(fp)
        return open(path, "rb").read()


def tile_of(rows, prefixes=None):
    """The rows a Multiplexer served ([(chrom, start, finish, [values])]) as the model's Tile: a segment per stretch of one name."""
    names, seg = [], [0]
    for i, r in enumerate(rows):
        if i == 0 or r[0] != rows[i - 1][0]:
            if i:
                seg.append(i)
            names.append(r[0])
    seg.append(len(rows))
    if not rows:
        return M.Tile(M.Lists(["none"], [0, 0], [], [], []), np.zeros((0, 1)))
    L =M.Lists(names, seg, [r[1] for r in rows], [r[2] for r in rows], np.zeros(len(rows)))
    return M.Tile(L, np.array([r[3] for r in rows], np.float64).reshape(len(rows), -1), prefixes)


def same_rows(a, b):
    return len(a) == len(b) and all(x[:3] == y[:3] and np.array_equal(np.array(x[3]).view(np.uint64), np.array(y[3]).view(np.uint64)) for x, y in zip(a, b))


def big_tracks():
    """Three tracks, two chromosomes, more than 25000 aligned runs, runs of 1 bp and more: both modes occur."""
    from wiggletools_amd import runlists
    rl = runlists.synth(3, [32000, 21000], mean_run=4, gap_prob=0.1, seed=4711, dtype=np.float32, defaults=[0.0, 2.5, -1.0])
    rl.chrom_names = ["chr1", "chr2"]
    return rl


def small_tracks():
    from wiggletools_amd import runlists
    rl = runlists.synth(4, [900, 700, 400], mean_run=3, gap_prob=0.2, seed=12, dtype=np.float32, defaults=[0.0, 0.5, 0.0, 3.0])
    rl.chrom_names = ["chrA", "chrB", "chrC"]
    return rl


def apply_parts(D, strict=False):
    """wtamd_ApplyMultiplexer of three statistics over 700 regions of two chromosomes, and the regions as the lines of a BED
    file: `apply_paste`'s shape."""
    from wiggletools_amd import runlists
    rl = runlists.synth(1, [30000, 20000], mean_run=5, gap_prob=0.2, seed=99, dtype=np.float32)
    names = ["chr1", "chr2"]
    seg = [0, int(rl.seg_off[1]), int(rl.seg_off[2])]
    data = D.reader(names, seg, rl.start, rl.finish, rl.value, overlapping=False)
    rs = np.concatenate([np.arange(400) * 70 + 5, np.arange(300) * 60 + 11]).astype(np.int32)
    rf = rs + 50
    regions = D.reader(names, [0, 400, 700], rs, rf, np.ones(700, np.float32), overlapping=True)
    lines = ["%s\t%d\t%d\tregion%d" % (names[0] if i < 400 else names[1], rs[i] - 1, rf[i] - 1, i) for i in range(700)]
    return D.apply(regions, ["AUC", "meanI", "maxI"], data, strict), lines


def paste_file(lines, path, short=0):
    """The lines as an infile with what the reference skips or strips: a browser line and two track lines, \\r\\n endings;
    `short`: that many lines are missing at the end.  Returns the prefixes the writer is to print."""
    lines = lines[:len(lines) - short]
    with open(path, "wb") as fh:
        fh.write(b"browser position chr1:1-1000\ntrack name=regions\n")
        for i, ln in enumerate(lines):
            fh.write(ln.encode() + (b"\r\n" if i % 3 == 1 else b"\n"))
            if i == 10:
                fh.write(b"track type=bed\n")
    return [ln.encode() for ln in lines]


def check_dropin(D, tmp, setenv=None):
    """The checks both backends share.  setenv(name, value): given by the product's test, which writes every case with the
    device door and again with WTAMD_NO_DEVICE_MTEXT=1."""
    path, infile = os.path.join(str(tmp), "out.txt"), os.path.join(str(tmp), "in.bed")
    big, small = big_tracks(), small_tracks()
    plain = {"big": D.read_mux(D.tracks(big)), "small": D.read_mux(D.tracks(small))}
    assert len(plain["big"]) > 25000                            # two block boundaries inside
    for no_device in (("0", "1") if setenv else ("0",)):
        if setenv:
            setenv("WTAMD_NO_DEVICE_MTEXT", no_device)
        # over this library's Multiplexer: the rows seen are those seen without the writer, the file is the model's text of them
        for name, rl in (("big", big), ("small", small)):
            T = tile_of(plain[name])
            for bed in (False, True):
                m, fp = D.tee(D.tracks(rl), path, bed)
                rows = D.read_mux(m)
                txt = D.written(fp, path)
                expect = M.text(T, M.BEDGRAPH if bed else 0)[0]
                assert same_rows(rows, plain[name]), (name, bed)
                assert txt == expect, (name, bed, no_device) + M.first_difference(txt, expect)
        assert b"fixedStep" in M.text(tile_of(plain["big"]), 0)[0]
        # over wtamd_ApplyMultiplexer: tee, and paste behind the regions' own lines
        m0, lines = apply_parts(D)
        rows0 = D.read_mux(m0)
        assert len(rows0) == 700
        for bed in (False, True):
            m, fp = D.tee(apply_parts(D)[0], path, bed)
            rows = D.read_mux(m)
            assert same_rows(rows, rows0) and D.written(fp, path) == M.text(tile_of(rows0), M.BEDGRAPH if bed else 0)[0], bed
        pre = paste_file(lines, infile)
        m, fp = D.paste(apply_parts(D)[0], infile, path)
        rows = D.read_mux(m)
        expect = M.text(tile_of(rows0, pre), 0)[0]
        txt = D.written(fp, path)
        assert same_rows(rows, rows0) and txt == expect, M.first_difference(txt, expect)
        assert expect.startswith(b"chr1\t4\t54\tregion0\t")
        if no_device == "1":
            continue                                            # (the corners below reach the formatter through the same call)
        # a line of 4999 bytes and more is consumed in pieces, one per entry, as the reference's fgets(buffer, 5000) does
        long_line = "x" * 12000
        with open(infile, "wb") as fh:
            fh.write((long_line + "\n" + "\n".join(lines[:697]) + "\n").encode())
        m, fp = D.paste(apply_parts(D)[0], infile, path)
        D.read_mux(m)
        pre = [long_line[:4999].encode(), long_line[4999:9998].encode(), long_line[9998:].encode()] + [ln.encode() for ln in lines[:697]]
        assert D.written(fp, path) == M.text(tile_of(rows0, pre), 0)[0]
        # holdFire: nothing is written before the first seek; the rows are passed on all the same
        m, fp = D.tee(D.tracks(small), path, False, hold=True)
        assert same_rows(D.read_mux(m), plain["small"]) and D.written(fp, path) == b""
        # SEEK, by the library's rule: the complete blocks of what was handed on are written, the open block is
        # dropped, the entry count restarts at 0; holdFire: the first seek opens fire
        lo, hi = 2000, 9000
        p = D.tracks(big)
        D.L.seekMultiplexer(p, b"chr2", lo, hi)
        window = D.read_mux(p)
        assert 1000 < len(window) < 9000
        for pops, whole, hold in ((5, 0, False), (9998, 0, False), (9999, M.BLOCK, False), (20499, 2 * M.BLOCK, False), (300, 0, True)):
            for bed in (False, True):
                flags = M.BEDGRAPH if bed else 0
                m, fp = D.tee(D.tracks(big), path, bed, hold)
                for _ in range(pops):
                    D.L.popMultiplexer(m)                        # handed on: `pops` rows and the current one
                D.L.seekMultiplexer(m, b"chr2", lo, hi)
                rows = D.read_mux(m)
                txt = D.written(fp, path)
                expect = M.text(tile_of(plain["big"][:whole]), flags)[0] + M.text(tile_of(window), flags)[0]
                assert same_rows(rows, window) and txt == expect, (pops, bed, hold) + M.first_difference(txt, expect)


def check_children(lib_path, tmp, amd=False):
    """The two checks that need a process of their own."""
    env = dict(os.environ)
    me = os.path.abspath(__file__)
    for bed in ("0",):                          # (wig mode: headers, rows in copies and bedGraph lines; the mode is not stdout's matter)
        r = subprocess.run([sys.executable, me, "stdout", lib_path, bed, "amd" if amd else "emu"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        D = DropIn(lib_path)
        expect = M.text(tile_of(D.read_mux(D.tracks(small_tracks()))), M.BEDGRAPH if bed == "1" else 0)[0]
        assert r.stdout == expect, M.first_difference(r.stdout, expect)
    out = os.path.join(str(tmp), "short.txt")
    r = subprocess.run([sys.executable, me, "short", lib_path, str(tmp), "amd" if amd else "emu"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert r.returncode == 1 and r.stderr.decode().endswith(SHORT_MESSAGE), (r.returncode, r.stderr.decode()[-2000:])
    D = DropIn(lib_path)
    m0, lines = apply_parts(D)
    rows0 = D.read_mux(m0)
    assert open(out, "rb").read() == M.text(tile_of(rows0[:699], [ln.encode() for ln in lines[:699]]), 0)[0]


def _main(argv):
    what, lib_path = argv[1], argv[2]
    if argv[-1] == "amd":
        from wiggletools_amd import _lib
        _lib.lib()                              # (PyTorch's HIP runtime goes first)
    D = DropIn(lib_path)
    if what == "stdout":
        D.L.wtamd_toStdoutMultiplexer(D.tracks(small_tracks()), b"\x01" if argv[3] == "1" else b"\x00", b"\x00")
        return 0
    tmp = argv[3]
    m0, lines = apply_parts(D)
    infile = os.path.join(tmp, "short.bed")
    paste_file(lines, infile, short=1)
    m, fp = D.paste(m0, infile, os.path.join(tmp, "short.txt"))
    D.read_mux(m)                               # ends in the library's exit(1)
    return 0


if __name__ == "__main__":
    sys.exit(_main(sys.argv))
