"""Builds the CPU-side test libraries under tests/emu/ (the emulator of the HIP kernels, the emulated drop-in layer, the units'
plain-C++ passes): every source to its own object with the compiler's dependency record (-MMD), one link.  A library is reused
only while it is newer than every file those records name and was built by the command line in use now; no header is listed
by hand."""
import ctypes
import fcntl
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "..", "wiggletools_amd", "csrc")
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas"]
UNITS = ("cover", "region", "apply", "profile", "window", "hist", "energy", "text")


def _objdir(so, objdir=None):
    return objdir or os.path.join(os.path.dirname(so), ".obj", os.path.basename(so))


def _objects(so, sources, objdir=None):
    return [os.path.join(_objdir(so, objdir), os.path.basename(s) + ".o") for s in sources]


def recorded_deps(so, sources, objdir=None):
    """Every file the compiler read when it made the objects of `so` (their -MMD records, written relative to the library's
    directory: they hold wherever the tree lies), as normalised absolute paths; None when a record is missing or unreadable."""
    base, files = os.path.dirname(so), []
    for obj in _objects(so, sources, objdir):
        try:
            words = open(obj + ".d").read().replace("\\\n", " ").split()
        except OSError:
            return None
        mine = [os.path.normpath(os.path.join(base, w)) for w in words if not w.endswith(":")]
        if not mine:
            return None
        files += mine
    return files


def newer_than(target, files):
    """`target` exists and no file of `files` (None: unknown) is missing or newer than it."""
    try:
        t = os.path.getmtime(target)
        return files is not None and all(os.path.getmtime(f) <= t for f in files)
    except OSError:
        return False


def build_lib(so, sources, flags=(), libs=(), objdir=None, force=False):
    """`so` from `sources` with FLAGS + flags, linked with libs; returns so.  Objects, their dependency records and the record of
    the command lines go to objdir (default: .obj/<library's name>/ beside the library).  One build at a time (pytest-xdist
    workers share the checkout): g++ to temporary names, os.replace() into place."""
    so, base = os.path.abspath(so), os.path.dirname(os.path.abspath(so))
    objdir = _objdir(so, objdir)
    rel = lambda p: os.path.relpath(p, base)      # noqa: E731
    objs = _objects(so, sources, objdir)
    compiles = [["g++"] + FLAGS + list(flags) + ["-MMD", "-MF", rel(o) + ".d", "-c", rel(s), "-o", rel(o) + ".tmp"] for s, o in zip(sources, objs)]
    link = ["g++", "-shared", "-fPIC", "-o", rel(so) + ".tmp"] + [rel(o) for o in objs] + list(libs)
    commands = "".join(" ".join(c) + "\n" for c in compiles + [link])
    record = os.path.join(objdir, "commands")

    def same_commands():
        try:
            return open(record).read() == commands
        except OSError:
            return False

    def fresh():
        return same_commands() and newer_than(so, recorded_deps(so, sources, objdir))

    if not force and fresh():
        return so
    with open(os.path.join(HERE, ".build.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        if not force and fresh():
            return so                                   # another worker built it while this one waited
        os.makedirs(objdir, exist_ok=True)
        keep = not force and same_commands()            # objects of these very commands may be reused one by one
        if os.path.exists(record):
            os.remove(record)                           # (until the link is done, nothing here counts as built)

        def compile_one(k):
            if not (keep and newer_than(objs[k], recorded_deps(so, sources[k:k + 1], objdir))):
                subprocess.check_call(compiles[k], cwd=base)
                os.replace(objs[k] + ".tmp", objs[k])

        with ThreadPoolExecutor(min(16, len(sources))) as ex:
            list(ex.map(compile_one, range(len(sources))))
        subprocess.check_call(link, cwd=base)
        os.replace(so + ".tmp", so)
        with open(record, "w") as f:
            f.write(commands)
    return so


def _emu(name):
    return os.path.join(HERE, name)


def build(force=False):
    """tests/emu/libwt_emu.so: the CPU emulator of the HIP kernels (wt_emu.cpp executes the kernels' own bodies, csrc/wt_exec.h)."""
    return build_lib(_emu("libwt_emu.so"), [_emu("wt_emu.cpp")], libs=["-lm"], force=force)


def build_variant(name, flags):
    """tests/emu/libwt_emu_<name>.so: the emulator compiled with extra flags (compile-time switches of the kernels' logic that are
    not the default, e.g. -DWT_DELTA_PARK=2)."""
    return build_lib(_emu("libwt_emu_%s.so" % name), [_emu("wt_emu.cpp")], flags=flags, libs=["-lm"])


def build_inflate_variant(name, flags):
    """tests/emu/libwt_inflate_<name>.so: the lane state machine of csrc/wt_inflate.h alone (wt_inflate_variant.cpp), compiled
    with extra flags (e.g. -DWT_INF_ROUND=3).  Exports wtemu_inflate and wtemu_inflate_ring like the emulated pipeline."""
    return build_lib(_emu("libwt_inflate_%s.so" % name), [_emu("wt_inflate_variant.cpp")], flags=flags)


DROPIN_SOURCES = [_emu("wt_emu.cpp"), _emu("wt_pipe_emu.cpp")] + [os.path.join(CSRC, s) for s in ("wt_iter_abi.cpp", "wt_defaults.cpp", "wt_bigwig.cpp")]


def build_dropin(force=False):
    """tests/emu/libwt_dropin_emu.so: the product's drop-in layer (csrc/wt_iter_abi.cpp, csrc/wt_defaults.cpp) linked against the
    emulated pipeline (wt_pipe_emu.cpp + wt_emu.cpp)."""
    return build_lib(_emu("libwt_dropin_emu.so"), DROPIN_SOURCES, libs=["-lm", "-lz", "-lpthread"], force=force)


def unit_sources(unit):
    return [os.path.join(HERE, "..", "%s_emu.cpp" % unit)]


def unit_lib(unit, force=False):
    """tests/emu/libwt_<unit>_emu.so: the plain-C++ passes and host sweep of one run-list unit (tests/<unit>_emu.cpp)."""
    assert unit in UNITS, unit
    return build_lib(_emu("libwt_%s_emu.so" % unit), unit_sources(unit), libs=["-lm"], force=force)


_LOADED = {}


def load_unit(unit):
    """unit_lib(unit) as a ctypes library, built and loaded once per process (the models' emu_lib())."""
    if unit not in _LOADED:
        _LOADED[unit] = ctypes.CDLL(unit_lib(unit))
    return _LOADED[unit]


if __name__ == "__main__":
    print(build(force=True))
    print(build_dropin(force=True))
