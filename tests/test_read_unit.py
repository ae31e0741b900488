"""The C ABI of the read unit (csrc/wt_read.hip): its doors are exported by the library and declared by
include/wiggletools_amd.h, its constants are defined, the state's size is the one a C compiler gives the declared struct, the
Python mirror has its names; and its kernels as the cross-compiled gfx950 code object holds them."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wtamd_text_runs", "wtamd_text_runs_host")


@pytest.fixture(scope="module")
def library():
    import __graft_entry__ as g
    g.build()
    from wiggletools_amd import _lib
    return _lib.LIB_PATH


def test_the_library_exports_the_doors(library):
    lib = ctypes.CDLL(library)
    assert not [n for n in NAMES if not hasattr(lib, n)]
    out = subprocess.check_output(["nm", "-D", "--defined-only", library]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [n for n in ("WiggleReader", "BedReader") if n in exported]


def test_the_header_declares_them_and_python_mirrors_them(library):
    txt = open(os.path.join(ROOT, "include", "wiggletools_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, txt), n
    for rx in (r"#define WTAMD_READ_BED\s+1u", r"#define WTAMD_READ_EOF\s+2u", r"#define WTAMD_READ_BEDGRAPH_MODE\s+0\b", r"#define WTAMD_READ_FIXED_MODE\s+1\b",
               r"#define WTAMD_READ_VARIABLE_MODE\s+2\b", r"\}\s*wtamd_read_state;", r"\}\s*wtamd_read_counts;"):
        assert re.search(rx, txt), rx
    from wiggletools_amd import engine
    assert all(hasattr(engine, f) for f in ("read_text", "_read_door", "ReadState", "ReadCounts", "READ_BED", "READ_EOF"))
    import read_model as M
    assert (engine.READ_BED, engine.READ_EOF, engine.READ_CANARY) == (M.BED, M.EOF, M.CANARY)
    assert ctypes.sizeof(engine.ReadState) == ctypes.sizeof(M.State) == 544 and ctypes.sizeof(engine.ReadCounts) == 64
    hdr = open(M.HEADER).read()
    assert int(re.search(r"#define WTR_TILE (\d+)\b", hdr).group(1)) == M.TILE
    assert int(re.search(r"#define WTR_LINE_MAX (\d+)\b", hdr).group(1)) == M.LINE_MAX


def test_the_state_s_size_to_a_c_compiler(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no host C compiler")
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include "wiggletools_amd.h"\n'
                   '_Static_assert(sizeof(wtamd_read_state) == 544, "wtamd_read_state");\n'
                   '_Static_assert(offsetof(wtamd_read_state, next) == 16 && offsetof(wtamd_read_state, chrom) == 32, "wtamd_read_state");\n'
                   '_Static_assert(offsetof(wtamd_read_state, rec_name) == 288, "wtamd_read_state");\n'
                   '_Static_assert(sizeof(wtamd_read_counts) == 64, "wtamd_read_counts");\nint main(void) { return 0; }\n')
    subprocess.check_call([cc, "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "size.o")])


def test_the_six_passes_keep_everything_in_registers():
    """The project's standing condition for side units: lines, scan, count, scan2, write and state are there, at 256 lanes, with
    no spilled vector register and no scratch memory."""
    from test_kernel_resources import _kernels
    mine = {name: k for name, k in _kernels().items() if "wt_read_kernel" in name}
    assert len(mine) == 6, sorted(mine)
    for name, k in mine.items():
        assert k["spill"] == 0 and k["scratch"] == 0 and k["max_wg"] == 256, (name, k)
