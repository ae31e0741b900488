// read_emu.cpp -- the reading passes of csrc/wt_read.h on the CPU (test infrastructure of tests/test_read_emu.py).  The header is
// compiled with -DWT_EMU: a pass is a function of (arguments, workgroup index), and the launcher of tests/emu/runs_launcher.h
// runs the workgroups of every pass one after the other, forwards, backwards or shuffled.  The door is the product's own
// template over this launcher; read_host is the product's host sweep; read_number is the product's number parser.
#define WT_EMU 1
#include "emu/runs_launcher.h"
#include "../wiggletools_amd/csrc/wt_read.h"

namespace {

struct ReadLauncher : CpuLauncher {
    using CpuLauncher::CpuLauncher;
    bool run_read(int kernel, long long blocks, const WtrArgs &a) { return run_blocks<WtrLds>(wtr_run_block, kernel, blocks, a); }
};

}  // namespace

extern "C" {

int read_emu_door(int order, uint64_t seed, const char *text, int64_t n_bytes, uint32_t flags, WtrState *state, int32_t *start, int32_t *finish,
                  double *value, int64_t capacity, int64_t *seg_off, int64_t *seg_name_off, int32_t *seg_name_len, int64_t seg_capacity,
                  int64_t *slow_rec, int64_t *slow_off, int64_t slow_capacity, WtrCounts *counts, int64_t *launches) {
    ReadLauncher l(order, seed);
    const char *why = "";
    const int rc = wtr_door(l, text, (long long) n_bytes, (unsigned int) flags, state, start, finish, value, (long long) capacity, seg_off, seg_name_off,
                            seg_name_len, (long long) seg_capacity, slow_rec, slow_off, (long long) slow_capacity, counts, &why);
    if (launches) *launches = l.launches;
    return rc;
}

int read_host(const char *text, int64_t n_bytes, uint32_t flags, WtrState *state, int32_t *start, int32_t *finish, double *value, int64_t capacity,
              int64_t *seg_off, int64_t *seg_name_off, int32_t *seg_name_len, int64_t seg_capacity, int64_t *slow_rec, int64_t *slow_off,
              int64_t slow_capacity, WtrCounts *counts) {
    return wtr_host(text, (long long) n_bytes, (unsigned int) flags, state, start, finish, value, (long long) capacity, seg_off, seg_name_off,
                    seg_name_len, (long long) seg_capacity, slow_rec, slow_off, (long long) slow_capacity, counts);
}

// the header's parser on one numeral: 0 not a number, 1 exact (*bits), 2 slow
int read_number(const char *s, int64_t n, uint64_t *bits) {
    WtrCtx c;
    c.text = (const unsigned char *) s; c.n = n; c.lo = 0; c.hi = 0; c.win = c.text; c.shift = 0;
    wtr_u64 b = 0;
    int slow = 0;
    if (!wtr_number(c, 0, n, &b, &slow)) return 0;
    *bits = b;
    return slow ? 2 : 1;
}

int read_sizes(int which) { return which == 0 ? (int) sizeof(WtrState) : which == 1 ? (int) sizeof(WtrCounts) : which == 2 ? (int) sizeof(WtrTile) : WTR_TILE; }

}  // extern "C"
