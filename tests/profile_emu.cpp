// profile_emu.cpp -- the profile passes of csrc/wt_profile.h on the CPU (test infrastructure of tests/test_profile_model.py).
// The header is compiled with -DWT_EMU: a pass is a function of (arguments, workgroup index), and the launcher of
// tests/emu/runs_launcher.h runs the workgroups of every pass one after the other, forwards, backwards or shuffled.  The
// door (validation, bounds, bins, scan, heavy, fold, add) is the product's own template over this launcher; profile_host is
// the product's host sweep.
#define WT_EMU 1
#include "emu/runs_launcher.h"
#include "../wiggletools_amd/csrc/wt_profile.h"

namespace {

struct ProfileLauncher : CpuLauncher {
    using CpuLauncher::CpuLauncher;
    bool run_profile(int kernel, long long blocks, const WprArgs &a) { return run_blocks<WprLds>(wpr_run_block, kernel, blocks, a); }
};

}  // namespace

extern "C" {

int profile_emu(int order, uint64_t seed, int64_t n_seg, const int64_t *seg_off, const int32_t *start, const int32_t *finish, const void *value,
                int value_is_f64, const int64_t *r_seg_off, const int32_t *r_start, const int32_t *r_finish, int32_t width, double default_value,
                uint32_t flags, int64_t batch, double *profile) {
    ProfileLauncher l(order, seed);
    const char *why = "";
    return wpr_profile(l, (long long) n_seg, seg_off, start, finish, value, value_is_f64, r_seg_off, r_start, r_finish, (long long) width,
                       default_value, (unsigned int) flags, (long long) batch, profile, &why);
}

int profile_host(int64_t n, const int32_t *start, const int32_t *finish, const double *value, int64_t n_r, const int32_t *r_start,
                 const int32_t *r_finish, int32_t width, double default_value, uint32_t flags, double *profile) {
    return wpr_profile_host((long long) n, start, finish, value, (long long) n_r, r_start, r_finish, (long long) width, default_value,
                            (unsigned int) flags, profile);
}

}  // extern "C"
