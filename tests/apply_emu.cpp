// apply_emu.cpp -- the apply passes of csrc/wt_apply.h on the CPU (test infrastructure of tests/test_apply_model.py).
// The header is compiled with -DWT_EMU: a pass is a function of (arguments, workgroup index), and the launcher of
// tests/emu/runs_launcher.h runs the workgroups of every pass one after the other, forwards, backwards or shuffled.  The
// door (validation, bounds, scan, chunk, final) is the product's own template over this launcher; apply_host is the
// product's host sweep.
#define WT_EMU 1
#include "emu/runs_launcher.h"
#include "../wiggletools_amd/csrc/wt_apply.h"

namespace {

struct ApplyLauncher : CpuLauncher {
    using CpuLauncher::CpuLauncher;
    bool run_apply(int kernel, long long blocks, const WapArgs &a) { return run_blocks<WapLds>(wap_run_block, kernel, blocks, a); }
};

}  // namespace

extern "C" {

int apply_emu(int order, uint64_t seed, int64_t n_seg, const int64_t *seg_off, const int32_t *start, const int32_t *finish, const void *value,
              int value_is_f64, const int64_t *r_seg_off, const int32_t *r_start, const int32_t *r_finish, double default_value, uint32_t flags,
              double *moments6) {
    ApplyLauncher l(order, seed);
    const char *why = "";
    return wap_apply(l, (long long) n_seg, seg_off, start, finish, value, value_is_f64, r_seg_off, r_start, r_finish, default_value,
                     (unsigned int) flags, moments6, &why);
}

int apply_host(int64_t n, const int32_t *start, const int32_t *finish, const double *value, int64_t n_r, const int32_t *r_start,
               const int32_t *r_finish, double default_value, uint32_t flags, double *moments6) {
    return wap_apply_host((long long) n, start, finish, value, (long long) n_r, r_start, r_finish, default_value, (unsigned int) flags, moments6);
}

}  // extern "C"
