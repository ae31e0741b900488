// cover_emu.cpp -- the coverage / union passes of csrc/wt_cover.h on the CPU (test infrastructure of tests/test_cover_model.py).
// The header is compiled with -DWT_EMU: a pass is a function of (arguments, workgroup index), and the launcher of
// tests/emu/runs_launcher.h runs the workgroups of every pass one after the other, forwards, backwards or shuffled.  The
// doors (grouping under the scratch budget, cuts at positions, capacity) are the product's own templates over this
// launcher.
#define WT_EMU 1
#include "emu/runs_launcher.h"

extern "C" {

int cover_emu_coverage(int order, uint64_t seed, int64_t n_seg, const int64_t *seg_off, const int32_t *start, const int32_t *finish,
                       int64_t capacity, int32_t *o_start, int32_t *o_finish, double *o_value, int64_t *o_seg_off, int64_t *n_out,
                       int64_t budget_bytes, int64_t *launches) {
    CpuLauncher l(order, seed);
    const char *why = "";
    const int rc = wcv_coverage(l, (long long) n_seg, seg_off, start, finish, (long long) capacity, o_start, o_finish, o_value, o_seg_off,
                                n_out, (long long) budget_bytes, &why);
    if (launches) *launches = l.launches;
    return rc;
}

int cover_emu_union(int order, uint64_t seed, int64_t n_seg, const int64_t *seg_off, const int32_t *start, const int32_t *finish,
                    const void *value, int value_is_f64, int64_t capacity, int32_t *o_start, int32_t *o_finish, double *o_value,
                    int64_t *o_seg_off, int64_t *n_out) {
    CpuLauncher l(order, seed);
    const char *why = "";
    return wcv_union(l, (long long) n_seg, seg_off, start, finish, value, value_is_f64, (long long) capacity, o_start, o_finish, o_value,
                     o_seg_off, n_out, &why);
}

}  // extern "C"
