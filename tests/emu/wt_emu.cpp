// wt_emu.cpp -- TEST INFRASTRUCTURE ONLY (never linked into the product).
//
// CPU emulation of the HIP kernels in wiggletools_amd/csrc (wt_reduce_kernel.h, wt_patch_kernels.hip, wt_delta_kernel.h,
// wt_walk.hip; their logic: wt_core.h, wt_delta.h, wt_walk.h, wt_mwalk.h): one emulated workgroup, windows in ticket order.  It
// exists so that the alignment / reducer / look-back logic can be checked against the oracle in the build container, which has
// no GPU.  Built by tests/emu/build.py
// into tests/emu/libwt_emu.so.
//
// ONE LOOP OVER THE LANES = ONE __syncthreads() INTERVAL OF THE KERNEL, no more and no fewer: the drivers below (EmuRun::run,
// run_patch, run_delta, run_walk, run_mwalk) carry the kernels' phase calls and barriers in the kernels' order, and
// tests/test_emu_skeleton.py compares the two texts.  Inside an interval the wavefronts run in the order WTEMU_WAVE_ORDER asks
// for (forward | reverse | rotate:<k> | shuffle:<seed>, WaveSched below); tests/test_emu_wave_order.py holds every order to the
// same bits.  An interval in which shared device code lets two wavefronts touch one LDS word, one of them writing, shows there.
//
// Intervals per kernel, by phase name (tests/test_emu_skeleton.py holds them to the kernels' text; `a | b`: a loop boundary INSIDE
// the substitute of one device call, see below; (c): only under the condition c):
//
//  wt_reduce_kernel (wt_reduce_kernel.h) = run()
//   1  ticket by lane 0, (NR) dflt32;  2  header by lane 0, zero
//   3+ per chunk, a barrier after each: (MULTI, not the first) zero; [eval_init,] load; count_a; count_b; (FUSE) eval_chunk
//   4  (FUSE, two passes) eval_mid, emask;  5  escan
//   6  publish by lane 0, (MULTIPLEX: complete by wave 0, barrier), every eval_chunk pass -- MULTI: zero, load,
//       count_a, count_b, eval_chunk with a barrier after each --, eval_mid, eval_finish, (MWU without register columns:
//       barrier, mwu_rank, barrier, mwu_tail), complete by wave 0
//   7  write;  8  stats + next ticket by lane 0
//  wt_patch_kernel (wt_patch_kernels.hip) = run_patch(): as 2-7 with a barrier in front of the header, without ticket, look-back
//   and statistics; n_emit / goffset set by lane 0 at the head of 6, a barrier between eval_finish and write, none after write
//  wt_delta_kernel (wt_delta_kernel.h) = run_delta(); Sum / Mean follow the kernel's `else` branches, not EP (below)
//   1  ticket + header by lane 0, zero (WT_DELTA_ZERO_EARLY)
//   2+ per chunk, a barrier after each: ranges_w1 -> ranges1; ranges_w2 -> ranges2 | ranges3; pass_mm / pass1 / pass2.
//       The verdicts (wt_delta_verdict, wt_delta_window_verdict) are read once, by the driver, where every lane reads
//       them; mark_bad by lane 0 shares the interval that follows.  Redone window: barrier, rezero, barrier, passes again
//   3  scan_w1[_tt|_mm] -> scan1 | scan2, barrier, scan3[_tt|_mm], barrier, (TT) combine_tt, barrier
//   4  (TT) mark_bad by lane 0 on risk; escan_wave -> wt_phase_escan over wave 0's lanes + publish by lane 0; nextw by all
//   5  complete + note_offset by wave 0; (TT) tail_tt by the other waves; not TT: this is interval 7
//   6  (TT) load_res_tt                      <- the barrier after it is this file's first finding
//   7  stage;  8  copy_out;  9  stats + ticket + header by lane 0, zero by all
//  wt_walk_kernel (wt_walk.hip) = run_walk()
//   1  ticket + header by lane 0, defaults;  2  walk_zero, ranges_w1 -> ranges1;  3  walk_ranges_w2 -> walk_ranges3
//   4  walk_pass;  5  emits, scan_a;  6  scan_b
//   7  publish by lane 0, walk_lane          (fallback: a barrier after each of offsets1, scan_b, offsets2, per
//       round walk_pass and walk_lane, then scan_a and scan_b)
//   8  complete by wave 0;  9  walk_write;  10  stats + ticket + header by lane 0
//  wt_mwalk_kernel (wt_walk.hip) = run_mwalk(): 1-4 as above; 5 mwalk_events, mwalk_lane (fallback as above);
//   6 scan_a; 7 scan_b; 8 publish by lane 0, complete by wave 0; 9 mwalk_write; 10 as above
//
// SUBSTITUTED (device-only wave code, `#ifndef WT_EMU`; what stands here instead is NOT vouched for by the wave-order tests -- only
// the -m gpu parity tests cover the device flavour): wt_delta_ranges_w1 / _w2, wt_walk_ranges_w2, wt_delta_scan_w1 / _tt / _mm,
// wt_delta_escan_wave (-> emu_escan_wave), wt_waves_before32 / 64 inside scan3*, the ballots of wt_delta_combine_tt, the wave
// reductions of wt_delta_copy_out and its WT_DELTA_COPY2 form, wt_lookback_publish / _complete (restated below for one lane), and the
// whole early-publish route of Sum / Mean (EP: wt_delta_scan3_cov / _val, wt_delta_stage_ep, wt_delta_note_offset_ep).
// NOT PERMUTED: the stretch-walking rounds (emu_walk_lanes / emu_mwalk_lanes: wt_walk_lane / wt_mwalk_lane, the two lanes of a pair
// as two real threads); they run after the other fragments of their interval, pairs ascending.  No interval is pinned to `forward`.
#define WT_EMU 1
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>
#include <thread>

#include "../../wiggletools_amd/csrc/wt_core.h"
#include "../../wiggletools_amd/csrc/wt_plan.h"

namespace {

// ---------------------------------------------------------------------------
// The workgroup scheduler.  A driver below is written like the kernel it restates: ph(...) hands over what every lane does
// next (a "fragment": one phase call, with the kernel's own `if (tid ...)` around it), barrier() stands where the kernel has
// __syncthreads().  Nothing runs until the barrier: then the interval's fragments are run wave by wave in the order the run
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

// The wave flavour of the look-back (wt_core.h, device only: ballots) restated for one lane: publish is the same two stores;
// complete is the sequential walk over the predecessors' status words (wt_phase_lookback: windows run in ticket order here, so
// every predecessor has its inclusive prefix out and the walk is one step).
void wt_lookback_publish(const WtParams &P, WtCtx &c, long long k, unsigned long long mine) {
    c.sh->n_emit = (int32_t) mine;
    if (k > 0) wt_status_store(&P.status[k], WT_FLAG_AGG | mine);
}
void wt_lookback_publish(const WtParams &P, WtCtx &c, long long k) { wt_lookback_publish(P, c, k, (unsigned long long) c.epfx[P.n_words]); }
void wt_lookback_complete(const WtParams &P, WtCtx &c, long long k, int lane, unsigned long long mine) {
    if (lane == 0) wt_phase_lookback(P, c, k, mine);
}
void wt_lookback_complete(const WtParams &P, WtCtx &c, long long k, int lane) { wt_lookback_complete(P, c, k, lane, (unsigned long long) c.epfx[P.n_words]); }
// wt_delta_escan_wave (device only: wave scans) for one lane of wave 0: the LDS-only scan over the 64 lanes
void emu_escan_wave(const WtParams &P, WtCtx &c, int lane) { wt_phase_escan(P, c, lane, 64); }

struct EmuRun {
    WtParams P;
    WtPlan plan;
    std::vector<char> lds;
    int T_lanes = 0;
    long long n_redo = 0;
    // patch mode (wt_patch_kernel): only these windows, run offsets given instead of looked back
    struct PatchGroup { long long goff; std::vector<long long> wins; };
    bool patch = false;
    std::vector<PatchGroup> groups;
    WaveSched S;

    template <class F> void ph(int n, F f) { S.pend.push_back(WaveSched::Frag{n, std::function<void(int)>(f)}); }
    void barrier() { S.run(); }             // where the kernel has __syncthreads()
    void sub_barrier() { S.run(); }         // a loop boundary inside the substitute of ONE device call (see the table above)
    void flush() { S.run(); }               // before a piece that the scheduler does not run (the stretch-walking rounds)

    // wt_reduce_kernel
    template <int OP, class ValT, class ScrT, int K, bool MULTI, int NR = 0>
    void run() {
        if (patch) { run_patch<OP, ValT, ScrT, K, MULTI, NR>(); return; }
        WtCtx c;
        wt_ctx_init(c, P, lds.data());
        std::vector<char> slab((size_t) (P.g_scratch_slab + P.g_attr_slab));
        if (P.g_scratch_slab) c.scratch = slab.data();      // one emulated workgroup: one slab
        if (P.g_attr_slab) c.attr = slab.data() + P.g_scratch_slab;
        const int T = plan.T, nt = T;
        std::vector<WtLane<K>> L(T);
        std::vector<WtAcc<K, NR>> A(T);
        ph(T, [&](int tid) { if (tid == 0) c.sh->ticket = (long long) wt_glb_add64(&P.counters[WT_CTR_TICKET], 1ull); });
        if (NR > 0)
            ph(T, [&](int tid) { for (int i = tid; i < P.n_tracks; i += nt) c.dflt32[i] = (float) P.defaults[i]; });
        barrier();
        for (;;) {
            const long long k = c.sh->ticket;
            if (k >= P.n_windows) break;
            ph(T, [&, k](int tid) { if (tid == 0) wt_phase_header(P, c, k); });
            ph(T, [&](int tid) { wt_phase_zero(P, c, true, tid, nt); });
            barrier();
            const int N = P.n_tracks, NC = MULTI ? P.chunk_tracks : N, n_chunks = MULTI ? P.n_chunks : 1;
            constexpr bool FUSE = MULTI && OP != WT_OP_MULTIPLEX;
            constexpr int npass = wt_eval_passes(OP);
            ph(T, [&](int tid) { wt_eval_init<OP, K>(A[tid]); });
            for (int ch = 0; ch < n_chunks; ch++) {
                const int t_lo = ch * NC, t_hi = (t_lo + NC < N) ? t_lo + NC : N;
                if (MULTI && ch > 0) {
                    ph(T, [&](int tid) { wt_phase_zero(P, c, false, tid, nt); });
                    barrier();
                }
                ph(T, [&, t_lo, t_hi](int tid) { wt_phase_load<ValT>(P, c, t_lo, t_hi, true, tid, nt); });
                barrier();
                ph(T, [&, t_lo, t_hi](int tid) { wt_phase_count_a(P, c, t_lo, t_hi, tid, nt); });
                barrier();
                ph(T, [&, t_lo, t_hi](int tid) { wt_phase_count_b(P, c, t_lo, t_hi, tid, nt); });
                barrier();
                if (FUSE) {
                    ph(T, [&, t_lo, t_hi](int tid) { wt_phase_eval_chunk<OP, ValT, ScrT, K>(P, c, A[tid], 0, t_lo, t_hi, true, tid, nt); });
                    barrier();
                }
            }
            if (FUSE && npass == 2) ph(T, [&](int tid) { wt_eval_mid<OP, K>(P, A[tid]); });
            ph(T, [&](int tid) { wt_phase_emask(P, c, OP == WT_OP_TTEST || OP == WT_OP_MWU, tid, nt); });
            barrier();
            ph(T, [&](int tid) { wt_phase_escan(P, c, tid, nt); });
            barrier();
            ph(T, [&, k](int tid) { if (tid == 0) wt_lookback_publish(P, c, k); });
            if (OP == WT_OP_MULTIPLEX) {
                ph(T, [&, k](int tid) { if (tid < 64) wt_lookback_complete(P, c, k, tid); });
                barrier();
            }
            for (int pass = FUSE ? 1 : 0; pass < npass; pass++) {
                for (int ch = 0; ch < n_chunks; ch++) {
                    const int t_lo = ch * NC, t_hi = (t_lo + NC < N) ? t_lo + NC : N;
                    if (MULTI) {
                        ph(T, [&](int tid) { wt_phase_zero(P, c, false, tid, nt); });
                        barrier();
                        ph(T, [&, t_lo, t_hi](int tid) { wt_phase_load<ValT>(P, c, t_lo, t_hi, false, tid, nt); });
                        barrier();
                        ph(T, [&, t_lo, t_hi](int tid) { wt_phase_count_a(P, c, t_lo, t_hi, tid, nt); });
                        barrier();
                        ph(T, [&, t_lo, t_hi](int tid) { wt_phase_count_b(P, c, t_lo, t_hi, tid, nt); });
                        barrier();
                    }
                    ph(T, [&, pass, t_lo, t_hi](int tid) { wt_phase_eval_chunk<OP, ValT, ScrT, K>(P, c, A[tid], pass, t_lo, t_hi, false, tid, nt); });
                    if (MULTI) barrier();
                }
                if (pass == 0 && npass == 2) ph(T, [&](int tid) { wt_eval_mid<OP, K>(P, A[tid]); });
            }
            ph(T, [&](int tid) { wt_phase_eval_finish<OP, ValT, ScrT, K>(P, c, A[tid], L[tid], tid, nt); });
            if (OP == WT_OP_MWU && NR == 0) {
                barrier();
                ph(T, [&](int tid) { wt_phase_mwu_rank<ScrT>(P, c, tid, nt); });
                barrier();
                ph(T, [&](int tid) { wt_phase_mwu_tail<K>(P, c, A[tid], L[tid], tid, nt); });
            }
            ph(T, [&, k](int tid) { if (OP != WT_OP_MULTIPLEX && tid < 64) wt_lookback_complete(P, c, k, tid); });
            barrier();
            ph(T, [&](int tid) { wt_phase_write<OP, ValT, K>(P, c, L[tid], tid, nt); });
            barrier();
            ph(T, [&](int tid) {
                if (tid == 0) {
                    wt_window_stats(P, c);
                    c.sh->ticket = (long long) wt_glb_add64(&P.counters[WT_CTR_TICKET], 1ull);
                }
            });
            barrier();
        }
    }

    // wt_patch_kernel (one emulated workgroup takes the items one after the other)
    template <int OP, class ValT, class ScrT, int K, bool MULTI, int NR>
    void run_patch() {
        WtCtx c;
        wt_ctx_init(c, P, lds.data());
        const int T = plan.T, nt = T;
        std::vector<WtLane<K>> L(T);
        std::vector<WtAcc<K, NR>> A(T);
        if (NR > 0)
            for (int i = 0; i < P.n_tracks; i++) c.dflt32[i] = (float) P.defaults[i];
        const int N = P.n_tracks, NC = MULTI ? P.chunk_tracks : N, n_chunks = MULTI ? P.n_chunks : 1;
        for (const PatchGroup &g : groups) {
            const long long goff = g.goff;
            for (const long long k : g.wins) {
                barrier();
                ph(T, [&, k](int tid) { if (tid == 0) wt_phase_header(P, c, k); });
                ph(T, [&](int tid) { wt_phase_zero(P, c, true, tid, nt); });
                barrier();
                constexpr int npass = wt_eval_passes(OP);
                ph(T, [&](int tid) { wt_eval_init<OP, K>(A[tid]); });
                for (int cc = 0; cc < n_chunks; cc++) {
                    const int t_lo = cc * NC, t_hi = (t_lo + NC < N) ? t_lo + NC : N;
                    if (MULTI && cc > 0) {
                        ph(T, [&](int tid) { wt_phase_zero(P, c, false, tid, nt); });
                        barrier();
                    }
                    ph(T, [&, t_lo, t_hi](int tid) { wt_phase_load<ValT>(P, c, t_lo, t_hi, false, tid, nt); });
                    barrier();
                    ph(T, [&, t_lo, t_hi](int tid) { wt_phase_count_a(P, c, t_lo, t_hi, tid, nt); });
                    barrier();
                    ph(T, [&, t_lo, t_hi](int tid) { wt_phase_count_b(P, c, t_lo, t_hi, tid, nt); });
                    barrier();
                    if (MULTI) {
                        ph(T, [&, t_lo, t_hi](int tid) { wt_phase_eval_chunk<OP, ValT, ScrT, K>(P, c, A[tid], 0, t_lo, t_hi, true, tid, nt); });
                        barrier();
                    }
                }
                if (MULTI && npass == 2) ph(T, [&](int tid) { wt_eval_mid<OP, K>(P, A[tid]); });
                ph(T, [&](int tid) { wt_phase_emask(P, c, OP == WT_OP_TTEST, tid, nt); });
                barrier();
                ph(T, [&](int tid) { wt_phase_escan(P, c, tid, nt); });
                barrier();
                ph(T, [&, goff](int tid) {
                    const long long n_emit = (long long) c.epfx[P.n_words];
                    if (tid == 0) { c.sh->n_emit = (int32_t) n_emit; c.sh->goffset = goff; }
                });
                for (int pass = MULTI ? 1 : 0; pass < npass; pass++) {
                    for (int cc = 0; cc < n_chunks; cc++) {
                        const int t_lo = cc * NC, t_hi = (t_lo + NC < N) ? t_lo + NC : N;
                        if (MULTI) {
                            ph(T, [&](int tid) { wt_phase_zero(P, c, false, tid, nt); });
                            barrier();
                            ph(T, [&, t_lo, t_hi](int tid) { wt_phase_load<ValT>(P, c, t_lo, t_hi, false, tid, nt); });
                            barrier();
                            ph(T, [&, t_lo, t_hi](int tid) { wt_phase_count_a(P, c, t_lo, t_hi, tid, nt); });
                            barrier();
                            ph(T, [&, t_lo, t_hi](int tid) { wt_phase_count_b(P, c, t_lo, t_hi, tid, nt); });
                            barrier();
                        }
                        ph(T, [&, pass, t_lo, t_hi](int tid) { wt_phase_eval_chunk<OP, ValT, ScrT, K>(P, c, A[tid], pass, t_lo, t_hi, false, tid, nt); });
                        if (MULTI) barrier();
                    }
                    if (pass == 0 && npass == 2) ph(T, [&](int tid) { wt_eval_mid<OP, K>(P, A[tid]); });
                }
                ph(T, [&](int tid) { wt_phase_eval_finish<OP, ValT, ScrT, K>(P, c, A[tid], L[tid], tid, nt); });
                barrier();
                ph(T, [&](int tid) { wt_phase_write<OP, ValT, K>(P, c, L[tid], tid, nt); });
            }
        }
        flush();        // (the kernel ends here: the last window's write)
    }

    // the stretch-walking rounds: the two lanes of a stretch run side by side as two real threads (they exchange values:
    // wt_pair_xchg), one pair at a time, lanes ascending -- not the scheduler's
    template <bool FIXED>
    void emu_walk_lanes(WtCtx &c, WtWalkCtx &w, std::vector<WtWalkLane> &L, int l0, int l1, uint32_t ev0) {
        const int T = plan.T;
        if (!w.pair) {
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
    void emu_mwalk_lanes(WtCtx &c, WtWalkCtx &w, std::vector<WtWalkLane> &L, int l0, int l1, uint32_t ev0) {
        const int T = plan.T;
        for (int q = l0; q < l1; q++) {
            std::thread odd([&, q] { wt_mwalk_lane<FIXED>(P, c, w, L[2 * q + 1], ev0, 2 * q + 1, T); });
            wt_mwalk_lane<FIXED>(P, c, w, L[2 * q], ev0, 2 * q, T);
            odd.join();
        }
    }

    // wt_walk_kernel
    void run_walk() {
        WtCtx c{};
        c.sh = (WtShared *) (lds.data() + P.off_shared);
        WtDeltaCtx d;
        wt_delta_ctx_init(d, P, lds.data());
        std::vector<char> slab((size_t) P.g_scratch_slab + 64);
        WtWalkCtx w;
        wt_walk_ctx_init(w, P, lds.data(), slab.data());
        const int T = plan.T, nt = T;
        std::vector<WtWalkLane> L(T);
        ph(T, [&](int tid) {
            if (tid == 0) {
                const long long k0 = (long long) wt_glb_add64(&P.counters[WT_CTR_TICKET], 1ull);
                c.sh->ticket = k0;
                if (k0 < P.n_windows) wt_phase_header(P, c, k0);
            }
        });
        ph(T, [&](int tid) { wt_walk_defaults(P, w, tid, nt); });
        barrier();
        for (;;) {
            const long long k = c.sh->ticket;
            if (k >= P.n_windows) break;
            ph(T, [&](int tid) { wt_walk_zero(P, c, w, tid, nt); });
            ph(T, [&](int tid) { wt_delta_ranges1(P, c, d, 0, tid, nt); });
            barrier();
            ph(T, [&](int tid) { wt_walk_ranges3(d, tid, nt); });
            barrier();
            ph(T, [&](int tid) { wt_walk_pass<false>(P, c, w, d, 0u, 0u, tid, nt); });
            barrier();
            ph(T, [&](int tid) { wt_walk_emits(P, c, w, L[tid], tid, nt); });
            ph(T, [&](int tid) { wt_walk_scan_a(w, wt_walk_emit_count(w, L[tid], tid), tid, nt); });
            barrier();
            ph(T, [&](int tid) { wt_walk_scan_b(w, tid, nt); });
            barrier();
            const unsigned long long mine = w.base[nt];
            ph(T, [&, k, mine](int tid) { if (tid == 0) wt_lookback_publish(P, c, k, mine); });
            if (w.novf[0] <= w.ov_cap) {
                n_rounds++;
                flush();
                emu_walk_lanes<true>(c, w, L, 0, w.nstr, 0u);
                barrier();
            } else {
                n_fallback++;
                barrier();
                ph(T, [&](int tid) { wt_walk_offsets1(P, w, tid, nt); });
                barrier();
                ph(T, [&](int tid) { wt_walk_scan_b(w, tid, nt); });
                barrier();
                ph(T, [&](int tid) { wt_walk_offsets2(P, w, tid, nt); });
                barrier();
                for (int l0 = 0; l0 < w.nstr;) {
                    const int l1 = wt_walk_round_end(w, l0, nt);
                    const uint32_t ev0 = w.base[l0 << w.pair], ev1 = w.base[l1 << w.pair];
                    if (ev1 > ev0) {
                        n_rounds++;
                        ph(T, [&, ev0, ev1](int tid) { wt_walk_pass<true>(P, c, w, d, ev0, ev1, tid, nt); });
                        barrier();
                        emu_walk_lanes<false>(c, w, L, l0, l1, ev0);
                        barrier();
                    }
                    l0 = l1;
                }
                ph(T, [&](int tid) { wt_walk_scan_a(w, wt_walk_emit_count(w, L[tid], tid), tid, nt); });
                barrier();
                ph(T, [&](int tid) { wt_walk_scan_b(w, tid, nt); });
                barrier();
            }
            if ((unsigned long long) w.base[T] != mine) { fprintf(stderr, "wtemu: walking kernel: run count changed\n"); abort(); }
            ph(T, [&, k, mine](int tid) { if (tid < 64) wt_lookback_complete(P, c, k, tid, mine); });
            barrier();
            ph(T, [&](int tid) { wt_walk_write(P, c, w, L[tid], tid, nt); });
            barrier();
            ph(T, [&](int tid) {
                if (tid == 0) {
                    wt_window_stats(P, c);
                    const long long kn = (long long) wt_glb_add64(&P.counters[WT_CTR_TICKET], 1ull);
                    c.sh->ticket = kn;
                    if (kn < P.n_windows) wt_phase_header(P, c, kn);
                }
            });
            barrier();
        }
    }

    // wt_mwalk_kernel
    void run_mwalk() {
        WtCtx c{};
        c.sh = (WtShared *) (lds.data() + P.off_shared);
        WtDeltaCtx d;
        wt_delta_ctx_init(d, P, lds.data());
        std::vector<char> slab((size_t) P.g_scratch_slab + 64);
        WtWalkCtx w;
        wt_walk_ctx_init(w, P, lds.data(), slab.data());
        const int T = plan.T, nt = T;
        std::vector<WtWalkLane> L(T);
        ph(T, [&](int tid) {
            if (tid == 0) {
                const long long k0 = (long long) wt_glb_add64(&P.counters[WT_CTR_TICKET], 1ull);
                c.sh->ticket = k0;
                if (k0 < P.n_windows) wt_phase_header(P, c, k0);
            }
        });
        ph(T, [&](int tid) { wt_walk_defaults(P, w, tid, nt); });
        barrier();
        for (;;) {
            const long long k = c.sh->ticket;
            if (k >= P.n_windows) break;
            ph(T, [&](int tid) { wt_walk_zero(P, c, w, tid, nt); });
            ph(T, [&](int tid) { wt_delta_ranges1(P, c, d, 0, tid, nt); });
            barrier();
            ph(T, [&](int tid) { wt_walk_ranges3(d, tid, nt); });
            barrier();
            ph(T, [&](int tid) { wt_walk_pass<false>(P, c, w, d, 0u, 0u, tid, nt); });
            barrier();
            ph(T, [&](int tid) { wt_mwalk_events(P, c, w, L[tid], tid, nt); });
            if (w.novf[0] <= w.ov_cap) {
                n_rounds++;
                flush();
                emu_mwalk_lanes<true>(c, w, L, 0, w.nstr, 0u);
                barrier();
            } else {
                n_fallback++;
                barrier();
                ph(T, [&](int tid) { wt_walk_offsets1(P, w, tid, nt); });
                barrier();
                ph(T, [&](int tid) { wt_walk_scan_b(w, tid, nt); });
                barrier();
                ph(T, [&](int tid) { wt_walk_offsets2(P, w, tid, nt); });
                barrier();
                for (int l0 = 0; l0 < w.nstr;) {
                    const int l1 = wt_walk_round_end(w, l0, nt);
                    const uint32_t ev0 = w.base[l0 << 1], ev1 = w.base[l1 << 1];
                    if (ev1 > ev0) {
                        n_rounds++;
                        ph(T, [&, ev0, ev1](int tid) { wt_walk_pass<true>(P, c, w, d, ev0, ev1, tid, nt); });
                        barrier();
                        emu_mwalk_lanes<false>(c, w, L, l0, l1, ev0);
                        barrier();
                    }
                    l0 = l1;
                }
            }
            ph(T, [&](int tid) { wt_walk_scan_a(w, wt_walk_emit_count(w, L[tid], tid), tid, nt); });
            barrier();
            ph(T, [&](int tid) { wt_walk_scan_b(w, tid, nt); });
            barrier();
            const unsigned long long mine = w.base[nt];
            ph(T, [&, k, mine](int tid) { if (tid == 0) wt_lookback_publish(P, c, k, mine); });
            ph(T, [&, k, mine](int tid) { if (tid < 64) wt_lookback_complete(P, c, k, tid, mine); });
            barrier();
            ph(T, [&](int tid) { wt_mwalk_write(P, c, w, L[tid], tid, nt); });
            barrier();
            ph(T, [&](int tid) {
                if (tid == 0) {
                    wt_window_stats(P, c);
                    const long long kn = (long long) wt_glb_add64(&P.counters[WT_CTR_TICKET], 1ull);
                    c.sh->ticket = kn;
                    if (kn < P.n_windows) wt_phase_header(P, c, kn);
                }
            });
            barrier();
        }
    }
    long long n_rounds = 0, n_fallback = 0;

    // wt_delta_kernel (Sum / Mean: its `else` branches -- the early publish of the device, EP, is wave code throughout)
    template <int OP, bool DF = false>
    void run_delta() {
        constexpr bool TT = OP == WT_OP_TTEST;      // two sets per position (wt_delta_scan3_tt)
        constexpr bool MM = OP == WT_OP_MAX || OP == WT_OP_MIN;     // range updates of a segment tree (wt_delta_apply_mm)
        constexpr bool QQ = OP == WT_OP_VAR || OP == WT_OP_STDDEV || OP == WT_OP_ENTROPY || OP == WT_OP_CV || TT;
        WtCtx c;
        wt_ctx_init(c, P, lds.data());
        WtDeltaCtx d;
        wt_delta_ctx_init(d, P, lds.data());
        const int T = plan.T, nt = T;
        std::vector<WtDeltaLane> DL(T);
        std::vector<WtDeltaLane2> DL2(T);
        std::vector<int32_t> wc_mm(T, 0);
        std::vector<WtLane<WT_DELTA_K>> L(T);
        const int nts = QQ ? P.W / WT_DELTA_K : nt;
        int guess = 0;      // the workgroup's unit exponent (0: none yet)
        unsigned long long mine = 0;        // (wave 0's, uniform)
        auto scan_lane = [&](int tid) { return !QQ || tid < nts; };     // WT_SCAN_LANE
        ph(T, [&](int tid) {
            if (tid == 0) {
                const long long k0 = (long long) wt_glb_add64(&P.counters[WT_CTR_TICKET], 1ull);
                c.sh->ticket = k0;
                if (k0 < P.n_windows) wt_phase_header(P, c, k0);
            }
        });
        if constexpr (MM) ph(T, [&](int tid) { wt_delta_zero_mm<OP == WT_OP_MAX>(P, c, d, tid, nt); });
        else ph(T, [&](int tid) { wt_delta_zero<QQ, TT>(P, c, d, tid, nt); });
        barrier();
        for (;;) {
            const long long k = c.sh->ticket;
            if (k >= P.n_windows) break;
            const int nchunks = (P.n_tracks + nt - 1) / nt;
            auto ntr = [&](int ch) { const int r = P.n_tracks - ch * nt; return r < nt ? r : nt; };     // tracks of chunk ch
            int scale = 1;
            if constexpr (MM) {
                for (int ch = 0; ch < nchunks; ch++) {
                    ph(T, [&, ch](int tid) { wt_delta_ranges1(P, c, d, ch * nt, tid, nt); });
                    barrier();
                    ph(T, [&](int tid) { wt_delta_ranges2(P, c, d, tid, nt); });
                    sub_barrier();
                    ph(T, [&](int tid) { wt_delta_ranges3(P, c, d, tid, nt); });
                    barrier();
                    ph(T, [&](int tid) { wt_delta_pass_mm<OP == WT_OP_MAX>(P, c, d, tid, nt); });
                    barrier();
                }
                ph(T, [&, k](int tid) { if (tid == 0 && d.dsh->bad) wt_delta_mark_bad(P, c, k); });
            } else if (guess == 0) {
                for (int ch = 0; ch < nchunks; ch++) {
                    ph(T, [&, ch](int tid) { wt_delta_ranges1(P, c, d, ch * nt, tid, nt); });
                    barrier();
                    ph(T, [&](int tid) { wt_delta_ranges2(P, c, d, tid, nt); });
                    sub_barrier();
                    ph(T, [&](int tid) { wt_delta_ranges3(P, c, d, tid, nt); });
                    barrier();
                    ph(T, [&](int tid) { wt_delta_pass1(P, c, d, tid, nt); });
                    barrier();
                }
                const bool any = d.dsh->emin <= d.dsh->emax;
                const bool ok = wt_delta_verdict(P, d, scale);
                ph(T, [&, k, ok](int tid) { if (!ok && tid == 0) wt_delta_mark_bad(P, c, k); });
                for (int ch = 0; ch < nchunks; ch++) {
                    if (nchunks > 1) {
                        ph(T, [&, ch](int tid) { wt_delta_ranges1(P, c, d, ch * nt, tid, nt); });
                        barrier();
                        ph(T, [&](int tid) { wt_delta_ranges2(P, c, d, tid, nt); });
                        sub_barrier();
                        ph(T, [&](int tid) { wt_delta_ranges3(P, c, d, tid, nt); });
                        barrier();
                    }
                    const int ntr_ch = ntr(ch);
                    ph(T, [&, scale, ok, ch, ntr_ch](int tid) { wt_delta_pass2<QQ, DF, TT>(P, c, d, scale, ok, false, true, tid, nt, ntr_ch, ch * nt); });
                    barrier();
                }
                if (any && ok) guess = scale;
            } else {
                for (int ch = 0; ch < nchunks; ch++) {
                    ph(T, [&, ch](int tid) { wt_delta_ranges1(P, c, d, ch * nt, tid, nt); });
                    barrier();
                    ph(T, [&](int tid) { wt_delta_ranges2(P, c, d, tid, nt); });
                    sub_barrier();
                    ph(T, [&](int tid) { wt_delta_ranges3(P, c, d, tid, nt); });
                    barrier();
                    const int ntr_ch = ntr(ch);
                    ph(T, [&, guess, ch, ntr_ch](int tid) { wt_delta_pass2<QQ, DF, TT>(P, c, d, guess, true, true, true, tid, nt, ntr_ch, ch * nt); });
                    barrier();
                }
                int lo;
                bool ok;
                scale = guess;
                if (!wt_delta_window_verdict(P, d, guess, lo, ok)) {
                    if (!ok) {
                        ph(T, [&, k](int tid) { if (tid == 0) wt_delta_mark_bad(P, c, k); });
                    } else {
                        n_redo++;
                        barrier();
                        ph(T, [&](int tid) { wt_delta_rezero<QQ, TT>(P, c, d, tid, nt); });
                        barrier();
                        for (int ch = 0; ch < nchunks; ch++) {
                            if (nchunks > 1) {
                                ph(T, [&, ch](int tid) { wt_delta_ranges1(P, c, d, ch * nt, tid, nt); });
                                barrier();
                                ph(T, [&](int tid) { wt_delta_ranges2(P, c, d, tid, nt); });
                                sub_barrier();
                                ph(T, [&](int tid) { wt_delta_ranges3(P, c, d, tid, nt); });
                                barrier();
                            }
                            const int ntr_ch = ntr(ch);
                            ph(T, [&, lo, ok, ch, ntr_ch](int tid) { wt_delta_pass2<QQ, DF, TT>(P, c, d, lo, ok, false, false, tid, nt, ntr_ch, ch * nt); });
                            barrier();
                        }
                        scale = lo;
                        guess = lo;
                    }
                }
            }
            if constexpr (TT) {
                ph(T, [&](int tid) { if (tid < 2 * nts) wt_delta_scan1_tt(P, c, d, DL2[tid], tid, nts); });
                sub_barrier();
                ph(T, [&](int tid) { if (tid < 2 * nts) wt_delta_scan2_tt(P, c, d, tid, nts); });
                barrier();
                ph(T, [&, scale](int tid) { if (tid < 2 * nts) wt_delta_scan3_tt(P, c, d, DL2[tid], scale, tid, nts); });
                barrier();
                ph(T, [&](int tid) { wt_delta_combine_tt(P, c, d, tid, nt); });
                barrier();
                ph(T, [&, k](int tid) { if (tid == 0 && d.dsh->risk && c.sh->bad_slot < 0) wt_delta_mark_bad(P, c, k); });
            } else if constexpr (MM) {
                ph(T, [&](int tid) { wt_delta_scan1_mm(P, c, d, wc_mm[tid], tid, nt); });
                sub_barrier();
                ph(T, [&](int tid) { wt_delta_scan2_mm(P, c, d, tid, nt); });
                barrier();
                ph(T, [&](int tid) { wt_delta_scan3_mm<OP == WT_OP_MAX>(P, c, d, 0, L[tid], tid, nt); });
                barrier();
            } else {
                ph(T, [&](int tid) { if (scan_lane(tid)) wt_delta_scan1<QQ>(P, c, d, DL[tid], tid, nts); });
                sub_barrier();
                ph(T, [&](int tid) { if (scan_lane(tid)) wt_delta_scan2<QQ>(P, c, d, tid, nts); });
                barrier();
                ph(T, [&, scale](int tid) { if (scan_lane(tid)) wt_delta_scan3<OP>(P, c, d, DL[tid], L[tid], scale, tid, nts); });
                barrier();
            }
            ph(T, [&](int tid) { if (tid < 64) emu_escan_wave(P, c, tid); });
            ph(T, [&, k](int tid) {
                if (tid < 64) {
                    mine = (unsigned long long) c.epfx[P.n_words];
                    if (tid == 0) wt_lookback_publish(P, c, k, mine);
                }
            });
            ph(T, [&](int tid) { wt_delta_nextw(P, c, tid, nt); });
            barrier();
            ph(T, [&, k](int tid) {
                if (tid < 64) {
                    wt_lookback_complete(P, c, k, tid, mine);
                    wt_delta_note_offset(P, c, tid);
                }
            });
            if constexpr (TT) {
                ph(T, [&](int tid) { if (tid >= 64) wt_delta_tail_tt(P, d, tid - 64, nt - 64); });
                barrier();
                ph(T, [&](int tid) { if (tid < nts) wt_delta_load_res_tt(P, d, L[tid], tid); });
                barrier();
            }
            ph(T, [&](int tid) { if (scan_lane(tid)) wt_delta_stage<OP>(P, c, d, L[tid], tid, nts); });
            barrier();
            ph(T, [&](int tid) { wt_delta_copy_out(P, c, d, tid, nt); });
            barrier();
            ph(T, [&](int tid) {
                if (tid == 0) {
                    wt_window_stats(P, c);
                    const long long kn = (long long) wt_glb_add64(&P.counters[WT_CTR_TICKET], 1ull);
                    c.sh->ticket = kn;
                    if (kn < P.n_windows) wt_phase_header(P, c, kn);
                }
            });
            if constexpr (MM) ph(T, [&](int tid) { wt_delta_zero_mm<OP == WT_OP_MAX>(P, c, d, tid, nt); });
            else ph(T, [&](int tid) { wt_delta_zero<QQ, TT>(P, c, d, tid, nt); });
            barrier();
        }
    }
};

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
        const bool patching = !delta && attempt == 1 && delta_bad > 0 && wt_few_enough_to_patch(delta_bad, delta_tab.n_windows) &&
                              wt_patch_compatible(R.plan, delta_W, s32, value_is_f64 != 0);
        if (patching) {
            const int ratio = delta_W / R.plan.W;
            R.patch = true;
            for (long long j = 0; j < delta_bad; j++) {
                const long long kd = bad_list[j];
                const int ch = delta_tab.win_chrom[kd];
                const long long m = kd - delta_tab.c_first_win[ch];
                // (as the patch kernel: every narrower window is an item of its own, at the offset the difference-array
                //  kernel recorded for its sub-range)
                for (int h = 0; h < ratio; h++) {
                    const long long mg = m * ratio + h;
                    if (mg >= tab.c_nwin[ch]) continue;
                    EmuRun::PatchGroup g;
                    g.goff = bad_goff[j * WT_BAD_SUB + h * (WT_BAD_SUB / ratio)];
                    g.wins.push_back(tab.c_first_win[ch] + mg);
                    R.groups.push_back(g);
                }
            }
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
        if (total > 0) {
            if (delta) {
                switch (op) {
                case WT_OP_SUM: if (P.delta_df) R.run_delta<WT_OP_SUM, true>(); else R.run_delta<WT_OP_SUM>(); break;
                case WT_OP_MEAN: if (P.delta_df) R.run_delta<WT_OP_MEAN, true>(); else R.run_delta<WT_OP_MEAN>(); break;
                case WT_OP_VAR: R.run_delta<WT_OP_VAR>(); break;
                case WT_OP_CV: R.run_delta<WT_OP_CV>(); break;
                case WT_OP_TTEST: R.run_delta<WT_OP_TTEST>(); break;
                case WT_OP_MAX: R.run_delta<WT_OP_MAX>(); break;
                case WT_OP_MIN: R.run_delta<WT_OP_MIN>(); break;
                default: R.run_delta<WT_OP_STDDEV>(); break;
                }
            } else if (R.plan.walk_S && R.plan.walk_mwu) {
                R.run_mwalk();
            } else if (R.plan.walk_S) {
                R.run_walk();
            } else if (!wt_dispatch(op, value_is_f64 != 0, s32, R.plan.ppt, R.plan.n_chunks > 1 || R.plan.scratch_slab > 0, R, R.plan.regcol)) {
                return -11;
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
