// window_emu.cpp -- the bin / smooth passes of csrc/wt_window.h on the CPU (test infrastructure of tests/test_window_model.py).
// The header is compiled with -DWT_EMU: a pass is a function of (arguments, workgroup index), and the launcher of
// tests/emu/runs_launcher.h runs the workgroups of every pass one after the other, forwards, backwards or shuffled.  The two
// doors are the product's own templates over this launcher; window_host_* are the product's host sweeps.
#define WT_EMU 1
#include "emu/runs_launcher.h"
#include "../wiggletools_amd/csrc/wt_window.h"

namespace {

struct WindowLauncher : CpuLauncher {
    using CpuLauncher::CpuLauncher;
    bool run_window(int kernel, long long blocks, const WwnArgs &a) { return run_blocks<WwnLds>(wwn_run_block, kernel, blocks, a); }
};

}  // namespace

extern "C" {

int window_emu_bin(int order, uint64_t seed, int64_t n_seg, const int64_t *seg_off, const int32_t *start, const int32_t *finish, const void *value,
                   int value_is_f64, int32_t width, double default_value, int64_t capacity, int32_t *o_start, int32_t *o_finish, double *o_value,
                   int64_t *o_seg_off, int64_t *n_out) {
    WindowLauncher l(order, seed);
    const char *why = "";
    return wwn_bin_door(l, (long long) n_seg, seg_off, start, finish, value, value_is_f64, (long long) width, default_value, (long long) capacity, o_start,
                        o_finish, o_value, o_seg_off, n_out, &why);
}

int window_emu_smooth(int order, uint64_t seed, int64_t n_seg, const int64_t *seg_off, const int32_t *start, const int32_t *finish, const void *value,
                      int value_is_f64, int32_t width, int32_t clip_lo, int32_t clip_hi, int64_t capacity, int32_t *o_start, int32_t *o_finish,
                      double *o_value, int64_t *o_seg_off, int64_t *n_out) {
    WindowLauncher l(order, seed);
    const char *why = "";
    return wwn_smooth_door(l, (long long) n_seg, seg_off, start, finish, value, value_is_f64, (long long) width, (long long) clip_lo, (long long) clip_hi,
                           (long long) capacity, o_start, o_finish, o_value, o_seg_off, n_out, &why);
}

int window_host_bin(int64_t n, const int32_t *start, const int32_t *finish, const double *value, int32_t width, double default_value, int64_t capacity,
                    int32_t *o_start, int32_t *o_finish, double *o_value, int64_t *n_out) {
    long long k = 0;
    const int rc = wwn_bin_host((long long) n, start, finish, value, (long long) width, default_value, (long long) capacity, o_start, o_finish, o_value, &k);
    *n_out = k;
    return rc;
}

int window_host_smooth(int64_t n, const int32_t *start, const int32_t *finish, const double *value, int32_t width, int32_t clip_lo, int32_t clip_hi,
                       int64_t capacity, int32_t *o_start, int32_t *o_finish, double *o_value, int64_t *n_out) {
    long long k = 0;
    const int rc = wwn_smooth_host((long long) n, start, finish, value, (long long) width, (long long) clip_lo, (long long) clip_hi, (long long) capacity,
                                   o_start, o_finish, o_value, &k);
    *n_out = k;
    return rc;
}

}  // extern "C"
