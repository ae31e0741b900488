// cover_any_emu.cpp -- the coverage door of csrc/wt_cover.h with its flags on the CPU (test infrastructure of
// tests/test_cover_any_order_emu.py): wcv_coverage_flags over the launcher of tests/emu/runs_launcher.h, which runs the
// workgroups of every pass one after the other, forwards, backwards or shuffled.  tests/cover_emu.cpp keeps the door without
// flags.
#define WT_EMU 1
#include "emu/runs_launcher.h"

extern "C" {

int cover_any_emu_coverage(int order, uint64_t seed, int64_t n_seg, const int64_t *seg_off, const int32_t *start, const int32_t *finish,
                           int64_t capacity, int32_t *o_start, int32_t *o_finish, double *o_value, int64_t *o_seg_off, int64_t *n_out,
                           int64_t budget_bytes, uint32_t flags, int64_t *launches) {
    CpuLauncher l(order, seed);
    const char *why = "";
    const int rc = wcv_coverage_flags(l, (long long) n_seg, seg_off, start, finish, (long long) capacity, o_start, o_finish, o_value,
                                      o_seg_off, n_out, (long long) budget_bytes, flags, &why);
    if (launches) *launches = l.launches;
    return rc;
}

}  // extern "C"
