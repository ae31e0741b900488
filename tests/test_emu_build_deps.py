"""tests/emu/build.py decides from the compiler's own dependency records (-MMD, one per object) and the recorded command lines
whether a test library is still good: first on a throw-away tree (nothing in the checkout is touched), then the records of
the real libraries, which must name the headers their sources reach only through other headers."""
import os
import subprocess

import pytest

from emu import build as B

CSRC = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "wiggletools_amd", "csrc"))
INCLUDE = os.path.normpath(os.path.join(CSRC, "..", "..", "include"))


def _age(tree, seconds=10):
    """Every file under `tree` becomes `seconds` older, so that a file touched afterwards is newer without lying in the future."""
    for d, _, files in os.walk(tree):
        for f in files:
            st = os.stat(os.path.join(d, f))
            os.utime(os.path.join(d, f), ns=(st.st_atime_ns, st.st_mtime_ns - seconds * 10 ** 9))


def test_the_builder_on_a_throw_away_tree(tmp_path):
    (tmp_path / "inc").mkdir()
    (tmp_path / "inc" / "inner.h").write_text("#define INNER 3\n")
    (tmp_path / "outer.h").write_text('#include "inc/inner.h"\n#define OUTER (INNER + 1)\n')
    (tmp_path / "first.h").write_text("#define FIRST 5\n")
    (tmp_path / "a.cpp").write_text('#include "first.h"\nextern "C" int a(void) { return FIRST; }\n')
    (tmp_path / "b.cpp").write_text('#include "outer.h"\nextern "C" int b(void) { return OUTER; }\n')
    so, srcs = str(tmp_path / "libt.so"), [str(tmp_path / "a.cpp"), str(tmp_path / "b.cpp")]
    stamp = lambda: os.stat(so).st_mtime_ns      # noqa: E731

    def rebuilt_after(change):
        """change() makes the library stale: the next call gives a library newer than everything recorded, the one after reuses it."""
        _age(str(tmp_path))
        before = stamp()
        change()
        assert B.build_lib(so, srcs) == so
        after = stamp()
        assert after > before
        assert B.newer_than(so, B.recorded_deps(so, srcs))
        assert B.build_lib(so, srcs) == so and stamp() == after
        return after

    assert B.build_lib(so, srcs) == so
    deps = B.recorded_deps(so, srcs)
    assert sorted(os.path.relpath(d, str(tmp_path)) for d in deps) == ["a.cpp", "b.cpp", "first.h", "inc/inner.h", "outer.h"]
    first = stamp()
    assert B.build_lib(so, srcs) == so and stamp() == first                 # a second call reuses the library
    rebuilt_after(lambda: os.utime(str(tmp_path / "inc" / "inner.h")))    # a newer nested header
    rebuilt_after(lambda: os.utime(str(tmp_path / "first.h")))            # a newer header of the first source alone
    rebuilt_after(lambda: os.remove(str(tmp_path / ".obj" / "libt.so" / "b.cpp.o.d")))      # a record is gone
    # other flags under the same name: rebuilt, and rebuilt again when the first flags come back
    before = stamp()
    assert B.build_lib(so, srcs, flags=["-DOTHER=1"]) == so and stamp() != before
    flagged = stamp()
    assert B.build_lib(so, srcs, flags=["-DOTHER=1"]) == so and stamp() == flagged
    assert B.build_lib(so, srcs) == so and stamp() != flagged
    # a header that is gone counts as stale (here: the build fails, it does not hand out the old library)
    os.remove(str(tmp_path / "first.h"))
    with pytest.raises(subprocess.CalledProcessError):
        B.build_lib(so, srcs)


def _names(so, sources):
    deps = B.recorded_deps(so, sources)
    assert deps is not None, so
    return set(deps)


def test_the_dropin_library_records_the_units_headers():
    deps = _names(B.build_dropin(), B.DROPIN_SOURCES)
    for h in ("wt_window.h", "wt_apply.h", "wt_profile.h", "wt_region.h", "wt_cover.h", "wt_moments_merge.h", "wt_hist.h", "wt_energy.h", "wt_text.h"):
        assert os.path.join(CSRC, h) in deps, h
    assert os.path.join(INCLUDE, "wiggletools_amd.h") in deps


def test_the_emulator_records_the_index_search():
    assert os.path.join(CSRC, "wt_isearch.h") in _names(B.build(), [os.path.join(B.HERE, "wt_emu.cpp")])


def test_the_profile_unit_records_the_units_below_it():
    deps = _names(B.unit_lib("profile"), B.unit_sources("profile"))
    for h in ("wt_profile.h", "wt_apply.h", "wt_region.h", "wt_cover.h", "wt_moments_merge.h"):
        assert os.path.join(CSRC, h) in deps, h
