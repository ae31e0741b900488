// text_emu.cpp -- the text passes of csrc/wt_text.h on the CPU (test infrastructure of tests/test_text_emu.py).  The header is
// compiled with -DWT_EMU: a pass is a function of (arguments, workgroup index), and the launcher of tests/emu/runs_launcher.h
// runs the workgroups of every pass one after the other, forwards, backwards or shuffled.  The door is the product's own
// template over this launcher; text_host is the product's host sweep; text_fmt is the product's integer "%lf".
#define WT_EMU 1
#include "emu/runs_launcher.h"
#include "../wiggletools_amd/csrc/wt_text.h"

namespace {

struct TextLauncher : CpuLauncher {
    using CpuLauncher::CpuLauncher;
    bool run_text(int kernel, long long blocks, const WtxArgs &a) { return run_blocks<WtxLds>(wtx_run_block, kernel, blocks, a); }
};

}  // namespace

extern "C" {

int text_emu_door(int order, uint64_t seed, int64_t n_seg, const int64_t *seg_off, const char *const *seg_name, const int32_t *start,
                  const int32_t *finish, const void *value, int value_is_f64, uint32_t flags, WtxState *state, char *text, int64_t capacity,
                  int64_t *n_bytes, int64_t *n_wide, int64_t *launches) {
    TextLauncher l(order, seed);
    const char *why = "";
    const int rc = wtx_door(l, (long long) n_seg, seg_off, seg_name, start, finish, value, value_is_f64, (unsigned int) flags, state, text,
                            (long long) capacity, n_bytes, n_wide, &why);
    if (launches) *launches = l.launches;
    return rc;
}

int text_host(int64_t n_seg, const int64_t *seg_off, const char *const *seg_name, const int32_t *start, const int32_t *finish, const double *value,
              uint32_t flags, WtxState *state, char *text, int64_t capacity, int64_t *n_bytes, int64_t *n_wide) {
    return wtx_host((long long) n_seg, seg_off, seg_name, start, finish, value, (unsigned int) flags, state, text, (long long) capacity, n_bytes, n_wide);
}

// the integer "%lf" of one value into buf (at least 32 bytes): its length, or -1 for a wide value
int text_fmt(double v, char *buf) {
    const WtxNum n = wtx_num(v);
    if (n.kind == WTX_WIDE) return -1;
    const WtxOut o = {(unsigned char *) buf, 0, 32, 0};
    return (int) wtx_put_num(o, 0, n);
}

}  // extern "C"
