"""Builds wiggletools_amd/csrc/libwiggletools_amd.so for gfx950 (hipcc cross-compiles without a GPU)."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libwiggletools_amd.so")
# the kernel units (wt_kernels.h): the heavy compiles, one thread each
KERNEL_SRCS = ["wt_reduce_stream.hip", "wt_reduce_moments.hip", "wt_reduce_order.hip", "wt_patch_kernels.hip", "wt_delta_kernels.hip", "wt_walk.hip"]
SRCS = KERNEL_SRCS + ["wt_engine.hip", "wt_pool.hip", "wt_pipe.hip", "wt_compress.hip", "wt_moments.hip", "wt_map.hip", "wt_cover.hip", "wt_region.hip", "wt_apply.hip", "wt_profile.hip", "wt_window.hip", "wt_hist.hip", "wt_energy.hip", "wt_text.hip", "wt_mtext.hip", "wt_read.hip", "wt_synth.hip", "wt_bwdev.hip", "wt_defaults.cpp", "wt_iter_abi.cpp", "wt_bigwig.cpp", "wt_bwwrite.cpp"]
LIBS = ["-lz"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
         "-Wall", "-Wno-unused-function", "-Wno-pass-failed"]


def build_source_variant(srcs, name, extra_flags):
    """Experiment helper: recompiles the given sources (one name or a list; SRCS: all) with extra flags, in parallel, and links
    them with the objects of the last build() (run build() first) into libwiggletools_amd_<name>.so (select it at run time with
    WTAMD_LIB=<path>), e.g. build_source_variant("wt_bwdev.hip", "round8", ["-DWT_INF_ROUND=8"]) or, for a switch of the reducing
    kernels, build_source_variant(KERNEL_SRCS + ["wt_engine.hip"], "prof", ["-DWT_PROFILE"]): the six kernel units and the engine,
    which prints their counters, are the units a -DWT_PROFILE variant needs; wt_pipe.hip and the side units do not read the switch."""
    from concurrent.futures import ThreadPoolExecutor
    srcs = [srcs] if isinstance(srcs, str) else list(srcs)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdir = os.path.join(HERE, ".obj")
    cflags = [f for f in FLAGS if f != "-shared"]

    def compile_one(src):
        obj = os.path.join(objdir, "%s_%s.o" % (src, name))
        subprocess.check_call([hipcc] + cflags + list(extra_flags) + ["-c", os.path.join(HERE, src), "-o", obj])
        return obj

    with ThreadPoolExecutor(len(srcs)) as ex:
        objs = list(ex.map(compile_one, srcs))
    others = [os.path.join(objdir, s + ".o") for s in SRCS if s not in srcs]
    out = os.path.join(HERE, "libwiggletools_amd_%s.so" % name)
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + others + LIBS + ["-o", out])
    return out


def build(force=False, verbose=False):
    """Every source to its own object (in parallel: the kernel units take up to three minutes each), then one link."""
    import time
    from concurrent.futures import ThreadPoolExecutor
    srcs = [os.path.join(HERE, s) for s in SRCS]
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdir = os.path.join(HERE, ".obj")
    os.makedirs(objdir, exist_ok=True)
    cflags = [f for f in FLAGS if f != "-shared"]

    def newer_than_deps(target, obj):
        """`target` is newer than obj's source and every header the compiler saw when it made obj (-MMD dependency file)."""
        try:
            words = open(obj + ".d").read().replace("\\\n", " ").split()
            t = os.path.getmtime(target)
        except OSError:
            return False
        files = [os.path.join(HERE, w) for w in words[1:] if not w.endswith(":")]      # (written relative to HERE: they hold wherever the tree lies)
        return bool(files) and all(os.path.exists(f) and os.path.getmtime(f) <= t for f in files)

    # the library against the union of the dependency files: every header any source includes counts, none is listed by hand
    objs = [os.path.join(objdir, os.path.basename(s) + ".o") for s in srcs]
    if not force and all(newer_than_deps(SO, o) for o in objs):
        if verbose:
            print("wiggletools_amd: libwiggletools_amd.so is newer than the sources / headers of its %d objects: REUSED (force=True recompiles)" % len(objs))
        return SO
    if verbose:
        print("wiggletools_amd: COMPILING %d sources for gfx950 with hipcc" % len(srcs))

    def compile_one(src):
        obj = os.path.join(objdir, os.path.basename(src) + ".o")
        if not force and newer_than_deps(obj, obj):
            if verbose:
                print("wiggletools_amd: %s unchanged: object REUSED" % os.path.basename(src))
            return obj
        cmd = [hipcc] + cflags + ["-MMD", "-MF", os.path.relpath(obj, HERE) + ".d", "-c", os.path.basename(src), "-o", os.path.relpath(obj, HERE)]
        if verbose:
            print(" ".join(cmd))
        t0 = time.time()
        subprocess.check_call(cmd, cwd=HERE)
        if verbose:
            print("wiggletools_amd: %s compiled in %.0f s" % (os.path.basename(src), time.time() - t0))
        return obj

    with ThreadPoolExecutor(len(srcs)) as ex:
        objs = list(ex.map(compile_one, srcs))
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + LIBS + ["-o", SO]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return SO


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
