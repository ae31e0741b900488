// wt_emu.cpp -- TEST INFRASTRUCTURE ONLY (never linked into the product).
//
// CPU emulation of the HIP kernels in wiggletools_amd/csrc: one emulated workgroup, windows in ticket order.  It exists so that
// the alignment / reducer / look-back logic can be checked against the oracle in the build container, which has no GPU.  Built
// by tests/emu/build.py into tests/emu/libwt_emu.so.
//
// THE EMULATOR EXECUTES THE KERNELS' OWN BODIES.  wt_reduce_kernel.h, wt_patch_kernel.h, wt_delta_kernel.h and wt_walk_kernel.h
// are each one text (wt_exec.h documents the vocabulary, both expansions side by side): under WT_EMU a kernel is a function
// template over EmuRun below, a fragment (WT_DO) is queued with ph(), WT_SYNC is barrier().  What lies between two barriers --
// one __syncthreads() interval of the kernel, no more and no fewer -- runs at the barrier; inside it the wavefronts run in the
// order WTEMU_WAVE_ORDER asks for (forward | reverse | rotate:<k> | shuffle:<seed>, WaveSched below);
// tests/test_emu_wave_order.py holds every order to the same bits.  An interval in which shared device code lets two wavefronts
// touch one LDS word, one of them writing, shows there.  The intervals of a kernel are read in its header, not here.
//
// SUBSTITUTED (device-only wave code, `#ifndef WT_EMU`; what stands in its place is NOT vouched for by the wave-order tests -- only
// the -m gpu parity tests cover the device flavour; each substitute is defined beside the device function, `a | b`: two fragments
// with a loop boundary, sub_barrier(), between them): wt_delta_ranges_w1 (-> wt_delta_ranges1), wt_delta_ranges_w2 (->
// wt_delta_ranges2 | wt_delta_ranges3), wt_walk_ranges_w2 (-> wt_walk_ranges3), wt_delta_scan_w1 / _tt / _mm (-> wt_delta_scan1* |
// wt_delta_scan2*), wt_delta_escan_wave (-> wt_phase_escan over wave 0's lanes), wt_waves_before32 / 64 inside scan3*, the
// ballots of wt_delta_combine_tt, the wave reductions of wt_delta_copy_out and its WT_DELTA_COPY2 form, wt_lookback_publish /
// _complete (wt_exec.h: one-lane flavours), and the whole early-publish route of Sum / Mean (EP: wt_delta_scan3_cov / _val,
// wt_delta_stage_ep, wt_delta_note_offset_ep -- the emulator is built with WT_DELTA_EARLY_PUBLISH 0 and follows the kernel's
// other branch).
// NOT PERMUTED: the stretch-walking rounds (WT_WALK_ROUND / WT_MWALK_ROUND -> emu_walk_lanes / emu_mwalk_lanes below:
// wt_walk_lane / wt_mwalk_lane, the two lanes of a pair as two real threads); they run after the other fragments of their
// interval, pairs ascending.  No interval is pinned to `forward`.
#define WT_EMU 1
#define WT_DELTA_EARLY_PUBLISH 0
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>
#include <thread>
#include <type_traits>

#include "../../wiggletools_amd/csrc/wt_core.h"
#include "../../wiggletools_amd/csrc/wt_plan.h"

namespace {

// ---------------------------------------------------------------------------
// The workgroup scheduler.  ph(...) hands over what every lane does next (a "fragment", WT_DO: one phase call, with the
// kernel's own `if (tid ...)` around it), barrier() stands where the kernel has __syncthreads().  Nothing runs until the barrier: then the interval's fragments are run wave by wave in the order the run
// asked for (WTEMU_WAVE_ORDER), inside a wave fragment by fragment with the lanes ascending -- a wavefront executes in
// lockstep, and the WT_EMU stubs of the ballots rely on "lane 0 of a word first" (wt_delta_combine_tt).
// ---------------------------------------------------------------------------
struct WaveSched {
    enum { FORWARD, REVERSE, ROTATE, SHUFFLE };
    int mode = FORWARD;
    unsigned long long arg = 0;         // rotate: the first wave; shuffle: the seed
    unsigned long long n_interval = 0;  // counter of the counter-based generator: the permutation of interval i depends on (seed, i) alone
    struct Frag { int n; std::function<void(int)> f; };
    std::vector<Frag> pend;
    std::vector<int> order;

    // "forward" | "reverse" | "rotate:<k>" | "shuffle:<seed>"; false: not understood
    bool parse(const char *s) {
        mode = FORWARD; arg = 0;
        if (!s || !*s || !strcmp(s, "forward")) return true;
        if (!strcmp(s, "reverse")) { mode = REVERSE; return true; }
        if (!strncmp(s, "rotate:", 7)) { mode = ROTATE; arg = strtoull(s + 7, nullptr, 10); return true; }
        if (!strncmp(s, "shuffle:", 8)) { mode = SHUFFLE; arg = strtoull(s + 8, nullptr, 10); return true; }
        return false;
    }
    static unsigned long long mix(unsigned long long x) {       // splitmix64's finaliser
        x += 0x9E3779B97F4A7C15ull;
        x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
        x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
        return x ^ (x >> 31);
    }
    void make_order(int nw) {
        order.resize(nw);
        for (int i = 0; i < nw; i++) order[i] = i;
        if (nw < 2) return;
        if (mode == REVERSE) std::reverse(order.begin(), order.end());
        else if (mode == ROTATE) std::rotate(order.begin(), order.begin() + (int) (arg % (unsigned long long) nw), order.end());
        else if (mode == SHUFFLE) {
            const unsigned long long key = mix(arg ^ mix(n_interval));
            for (int i = nw - 1; i > 0; i--) std::swap(order[i], order[(int) (mix(key + (unsigned long long) i) % (unsigned long long) (i + 1))]);
        }
    }
    // one interval: every pending fragment over its lanes
    void run() {
        int nmax = 0;
        for (const Frag &g : pend) nmax = std::max(nmax, g.n);
        make_order((nmax + 63) / 64);
        for (int w : order)
            for (const Frag &g : pend)
                for (int t = w * 64; t < std::min(g.n, w * 64 + 64); t++) g.f(t);
        pend.clear();
        n_interval++;
    }
};

// One emulated workgroup: what a kernel's body (wt_exec.h, under WT_EMU) runs on
struct EmuRun {
    WtParams P;
    WtPlan plan;
    std::vector<char> lds, slab;        // slab: the workgroup's global scratch (P.g_scratch points at it)
    long long n_redo = 0, n_rounds = 0, n_fallback = 0;     // counted by the kernels' text (WT_EMU_ONLY, WT_WALK_ROUND)
    WaveSched S;

    template <class F> void ph(int n, F f) { S.pend.push_back(WaveSched::Frag{n, std::function<void(int)>(f)}); }
    void barrier() { S.run(); }             // where the kernel has __syncthreads()
    void sub_barrier() { S.run(); }         // a loop boundary inside the substitute of ONE device call (see above)
    void flush() { S.run(); }               // before a piece that the scheduler does not run (the stretch-walking rounds), and when a kernel ends
};

// the stretch-walking rounds: the two lanes of a stretch run side by side as two real threads (they exchange values:
// wt_pair_xchg), one pair at a time, lanes ascending -- not the scheduler's
template <bool FIXED, bool PAIR>
void emu_walk_lanes(EmuRun &R, WtCtx &c, WtWalkCtx &w, std::vector<WtWalkLane> &L, int l0, int l1, uint32_t ev0) {
    const WtParams &P = R.P;
    const int T = R.plan.T;
    if (!PAIR) {
        for (int t = l0; t < l1; t++) wt_walk_lane<FIXED, false>(P, c, w, L[t], ev0, t, T);
        return;
    }
    for (int q = l0; q < l1; q++) {
        std::thread odd([&, q] { wt_walk_lane<FIXED, true>(P, c, w, L[2 * q + 1], ev0, 2 * q + 1, T); });
        wt_walk_lane<FIXED, true>(P, c, w, L[2 * q], ev0, 2 * q, T);
        odd.join();
    }
}
template <bool FIXED>
void emu_mwalk_lanes(EmuRun &R, WtCtx &c, WtWalkCtx &w, std::vector<WtWalkLane> &L, int l0, int l1, uint32_t ev0) {
    const WtParams &P = R.P;
    const int T = R.plan.T;
    for (int q = l0; q < l1; q++) {
        std::thread odd([&, q] { wt_mwalk_lane<FIXED>(P, c, w, L[2 * q + 1], ev0, 2 * q + 1, T); });
        wt_mwalk_lane<FIXED>(P, c, w, L[2 * q], ev0, 2 * q, T);
        odd.join();
    }
}

}  // namespace

// the kernels' bodies
#include "../../wiggletools_amd/csrc/wt_reduce_kernel.h"
#include "../../wiggletools_amd/csrc/wt_patch_kernel.h"
#include "../../wiggletools_amd/csrc/wt_delta_kernel.h"
#include "../../wiggletools_amd/csrc/wt_walk_kernel.h"

namespace {

// Functor of wt_dispatch (wt_plan.h): the general kernel of (op, value type, ...), or -- Q set -- the patch kernel over Q's
// windows (float values and scratch, no register columns: wt_patch_compatible)
struct EmuReduce {
    EmuRun &R;
    const WtPatchArgs *Q;
    template <int OP, class ValT, class ScrT, int K, bool MULTI, int NR = 0>
    void run() {
        if (!Q) wt_reduce_kernel<OP, ValT, ScrT, K, MULTI, NR>(R, R.P);
        else if constexpr (NR == 0 && std::is_same<ValT, float>::value && std::is_same<ScrT, float>::value) wt_patch_kernel<OP, K, MULTI>(R, R.P, *Q);
        else { fprintf(stderr, "wtemu: no patch kernel for this plan\n"); abort(); }
    }
};
template <int OP> void emu_delta(EmuRun &R) { if (R.P.delta_df) wt_delta_kernel<OP, true>(R, R.P); else wt_delta_kernel<OP, false>(R, R.P); }

}  // namespace

extern "C" {

// Returns number of runs (>= 0) or a negative error.  All pointers are host.
// info[0..3] receive W, T, lds_bytes, n_windows.
long long wtemu_reduce(int n_chrom, int n_tracks, const int64_t *seg_off, const int32_t *start,
                       const int32_t *finish, const void *value, int value_is_f64, const double *defaults,
                       int op, unsigned flags, int n_set0, long long capacity,
                       int32_t *o_start, int32_t *o_finish, double *o_value, int64_t *chrom_run_off,
                       double *o_tile, uint8_t *o_inplay, long long *info,
                       const int32_t *range_lo, const int32_t *range_hi) {
    const bool s32 = !value_is_f64 && wt_defaults_fit_f32(defaults, n_tracks);
    const int64_t n_seg = (int64_t) n_chrom * n_tracks;
    std::vector<int32_t> fs(n_seg, 0), lf(n_seg, 0);
    for (int64_t s = 0; s < n_seg; s++)
        if (seg_off[s + 1] > seg_off[s]) { fs[s] = start[seg_off[s]]; lf[s] = finish[seg_off[s + 1] - 1]; }
    const int64_t total = seg_off[n_seg];
    std::vector<unsigned long long> counters(WT_CTR_N, 0);
    long long used_delta = 0, delta_bad = 0, n_redo_total = 0, patched = 0, walk_used = 0, walk_rounds = 0, walk_fallback = 0;
    std::vector<int32_t> bad_list;
    std::vector<long long> bad_goff;
    const char *wave_order = getenv("WTEMU_WAVE_ORDER");        // the order of the wavefronts inside every barrier interval (WaveSched)
    WtWindowTables delta_tab;
    int delta_W = 0;
    std::vector<unsigned long long> delta_counters;
    // the engine's policy: exact difference-array path first when eligible, the general kernel
    // if any window had to give up
    for (int attempt = 0; attempt < 2; attempt++) {
        const bool delta = attempt == 0 && o_tile == nullptr && wt_delta_eligible(op, value_is_f64 != 0, n_tracks, defaults);
        if (attempt == 0 && !delta) continue;
        EmuRun R;
        if (!R.S.parse(wave_order)) { fprintf(stderr, "wtemu: WTEMU_WAVE_ORDER=%s not understood\n", wave_order); return -12; }
        std::string err;
        if (delta) wt_make_delta_plan_for(R.plan, n_tracks, op);
        else {
            // the engine's general plan (wt_plan.h), with the emulator's own switches: the median walks unless WTAMD_NO_WALK, MWU
            // (wt_mwalk.h) when WTAMD_MWALK=1 asks for it -- the engine's sample of the values is not taken here
            const bool walk = !o_tile && !getenv("WTAMD_NO_WALK");
            const bool mwu_walk = walk && getenv("WTAMD_MWALK") && atoi(getenv("WTAMD_MWALK")) != 0;
            if (!wt_pick_general_plan(n_tracks, op, value_is_f64 != 0, s32, n_set0, walk, mwu_walk, 0.0, R.plan, err)) { fprintf(stderr, "wtemu: %s\n", err.c_str()); return -10; }
        }
        WtWindowTables tab;
        wt_make_windows(n_chrom, n_tracks, seg_off, fs.data(), lf.data(), R.plan.W, tab, range_lo, range_hi);
        std::vector<uint32_t> widx((size_t) tab.n_rows * n_tracks, 0);
        std::vector<unsigned long long> status(tab.n_windows, 0);
        counters.assign(WT_CTR_N, 0);
        if (delta) { bad_list.assign(tab.n_windows + 1, 0); bad_goff.assign((tab.n_windows + 1) * WT_BAD_SUB, 0); }

        WtParams &P = R.P;
        memset(&P, 0, sizeof(P));
        P.start = start; P.finish = finish; P.value = value; P.seg_off = seg_off; P.defaults = defaults;
        P.n_chrom = n_chrom; P.n_tracks = n_tracks;
        P.cbase = tab.cbase.data(); P.c_nwin = tab.c_nwin.data(); P.c_hi = tab.c_hi.data(); P.c_first_win = tab.c_first_win.data();
        P.n_windows = tab.n_windows; P.win_chrom = tab.win_chrom.data(); P.widx = widx.data();
        P.op = op; P.flags = flags; P.n_set0 = n_set0;
        P.status = status.data(); P.counters = counters.data();
        P.capacity = capacity; P.o_start = o_start; P.o_finish = o_finish; P.o_value = o_value;
        P.chrom_run_off = chrom_run_off; P.o_tile = o_tile; P.o_inplay = o_inplay;
        wt_plan_to_params(R.plan, P);
        std::vector<double> mwu_table;
        if (op == WT_OP_MWU && !getenv("WTAMD_MWU_DEVICE_ERF")) {
            if (wt_mwu_make_table(n_set0, n_tracks - n_set0, mwu_table)) { P.mwu_table = mwu_table.data(); P.mwu_kmax = (int) mwu_table.size() - 1; }
        }
        if (delta) { P.bad_list = bad_list.data(); P.bad_goff = bad_goff.data(); wt_delta_defaults_params(defaults, n_tracks, P); }
        // few inexact windows: the general kernel rewrites the values of just those (the engine's
        // wt_patch_kernel); many: it redoes everything
        WtPatchArgs Q;
        unsigned long long n_bad = 0;
        const bool patching = !delta && attempt == 1 && delta_bad > 0 && wt_few_enough_to_patch(delta_bad, delta_tab.n_windows) &&
                              wt_patch_compatible(R.plan, delta_W, s32, value_is_f64 != 0);
        if (patching) {
            const int ratio = delta_W / R.plan.W;
            // (the patch kernel's own arguments: it takes every narrower window as an item of its own, at the offset the
            //  difference-array kernel recorded for its sub-range; the one emulated workgroup takes the items in turn)
            n_bad = (unsigned long long) delta_bad;
            Q.bad_list = bad_list.data(); Q.bad_goff = bad_goff.data(); Q.n_bad = &n_bad;
            Q.d_win_chrom = delta_tab.win_chrom.data(); Q.d_c_first_win = delta_tab.c_first_win.data(); Q.ratio = ratio;
            patched = delta_bad;
        }

        // window index "kernel"
        P.n_total = total;
        if (total > 0) {
            WtIndexCursor cur;
            wt_index_cursor_set(P, cur, wt_index_find_segment(P, 0));
            for (int64_t g = 0; g < total; g++) wt_index_apply(P, cur, g, finish[g], g > 0 ? finish[g - 1] : 0);
        }

        R.lds.assign((size_t) R.plan.lds_bytes + 64, 0);
        R.slab.assign((size_t) P.g_scratch_slab + (size_t) P.g_attr_slab + 64, 0);       // one emulated workgroup: one slab
        P.g_scratch = R.slab.data();
        if (total > 0) {
            if (delta) {
                switch (op) {
                case WT_OP_SUM: emu_delta<WT_OP_SUM>(R); break;
                case WT_OP_MEAN: emu_delta<WT_OP_MEAN>(R); break;
                case WT_OP_VAR: wt_delta_kernel<WT_OP_VAR>(R, P); break;
                case WT_OP_CV: wt_delta_kernel<WT_OP_CV>(R, P); break;
                case WT_OP_TTEST: wt_delta_kernel<WT_OP_TTEST>(R, P); break;
                case WT_OP_MAX: wt_delta_kernel<WT_OP_MAX>(R, P); break;
                case WT_OP_MIN: wt_delta_kernel<WT_OP_MIN>(R, P); break;
                default: wt_delta_kernel<WT_OP_STDDEV>(R, P); break;
                }
            } else if (R.plan.walk_S && R.plan.walk_mwu) {
                wt_mwalk_kernel<256>(R, P);
            } else if (R.plan.walk_S) {
                if (P.walk_pair) wt_walk_kernel<256, true>(R, P); else wt_walk_kernel<256, false>(R, P);
            } else {
                EmuReduce run{R, patching ? &Q : nullptr};
                if (!wt_dispatch(op, value_is_f64 != 0, s32, R.plan.ppt, R.plan.n_chunks > 1 || R.plan.scratch_slab > 0, run, R.plan.regcol)) return -11;
            }
        }
        if (R.plan.walk_S) { walk_used = 1; walk_rounds = R.n_rounds; walk_fallback = R.n_fallback; }
        if (info && !patching) { info[0] = R.plan.W; info[1] = R.plan.T; info[2] = R.plan.lds_bytes; info[3] = tab.n_windows; info[6] = R.plan.n_chunks; info[7] = R.plan.scratch_slab;
                    info[4] = (long long) counters[WT_CTR_BP]; info[5] = (long long) counters[WT_CTR_INTERVALS]; }
        if (delta) {
            n_redo_total = R.n_redo;
            delta_bad = (long long) counters[WT_CTR_DELTA_BAD];
            used_delta = delta_bad == 0;
            if (used_delta) break;
            delta_tab = tab;
            delta_W = R.plan.W;
            delta_counters = counters;
        } else if (patching) {
            counters = delta_counters;          // run count, covered bp, ... are the difference-array launch's
            used_delta = 1;
        }
    }
    if (info) { info[8] = used_delta; info[9] = delta_bad; info[10] = n_redo_total; info[11] = patched; }
    if (info) { info[12] = walk_used; info[13] = walk_rounds; info[14] = walk_fallback; }
    if (counters[WT_CTR_ERROR] & WT_ERR_CAPACITY) return -1;
    if (counters[WT_CTR_ERROR]) return -2;
    return (long long) counters[WT_CTR_RUNS];
}

// the device's form of the t-test's tail (wt_core.h wt_tdist_2Q_fast: the device reducers' wt_ttest_tail) and the oracle's form
// beside it, for tests/test_tdist_fast.py
double wtemu_tdist_2q_fast(double t, double nu) { return wt_tdist_2Q_fast(t, nu); }
double wtemu_tdist_2q(double t, double nu) { return 2 * wt_tdist_Q(t, nu); }
double wtemu_lgamma_half_diff(double a) { return wt_lgamma_half_diff(a); }
// wt_div_n (csrc/wt_delta.h) against the division it stands in for: `cases` quotients per count n in [n_lo, n_hi], chosen to sit on and beside
// the doubles' rounding boundaries (s = RN(n (m + h ulp)) for h in {0, 1/2} -+ a few ulp) and at random; returns the mismatches
long long wtemu_div_n_mismatches(int n_lo, int n_hi, int cases, unsigned long long seed) {
    long long bad = 0;
    unsigned long long x = seed * 0x9E3779B97F4A7C15ull + 1;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (int n = n_lo; n <= n_hi; n++) {
        const double dn = (double) n, y = 1.0 / dn;
        for (int c = 0; c < cases; c++) {
            const unsigned long long r = rnd();
            const unsigned long long mant = (r & ((1ull << 52) - 1)) | (c % 7 == 0 ? ((1ull << 52) - 1) & ~((r >> 52) & 0xff) : 0ull) ;
            const int e = (int) (rnd() % 300) - 150;
            double m = ldexp(1.0 + (double) (mant & ((1ull << 52) - 1)) * 0x1p-52, e);
            double s;
            switch (c % 4) {
            case 0: s = m; break;                                                   // any double
            case 1: s = m * dn; break;                                              // a quotient next to a double
            case 2: s = (m + ldexp(1.0, e - 53)) * dn; break;                       // ... next to a midpoint
            default: s = (double) (long long) (rnd() >> 11) * ldexp(1.0, e - 60); break;    // an integer sum times a unit
            }
            for (int d = -2; d <= 2; d++) {
                double t = s;
                for (int q = 0; q < (d < 0 ? -d : d); q++) t = nextafter(t, d < 0 ? -INFINITY : INFINITY);
                for (int sg = 0; sg < 2; sg++) {
                    const double v = sg ? -t : t;
                    const double a = wt_div_n(v, dn, y), b = v / dn;
                    if (!(a == b) || std::signbit(a) != std::signbit(b)) bad++;
                }
            }
        }
    }
    return bad;
}

}  // extern "C"
