// wt_walk_kernel.h -- wt_walk_kernel and wt_mwalk_kernel: MedianReduction / MWUReduction by walking (logic in wt_walk.h,
// wt_mwalk.h).  One text (wt_exec.h): wt_walk.hip compiles it for gfx950 and holds the launcher, tests/emu/wt_emu.cpp runs the
// same bodies on the CPU.
#ifndef WT_WALK_KERNEL_H_
#define WT_WALK_KERNEL_H_

#include "wt_core.h"
#include "wt_exec.h"

// The stretch-walking rounds: wt_walk_lane / wt_mwalk_lane over the lanes of the stretches [l0, l1) (FIXED: every stretch).
// The two lanes of a stretch exchange values (wt_pair_xchg), so the emulator runs them as two real threads, one pair at a
// time, after the other fragments of their interval (emu_walk_lanes / emu_mwalk_lanes, wt_emu.cpp) -- not the scheduler's.
#ifdef WT_EMU
#define WT_WALK_ROUND(FIXED, l0, l1, ev0) do { R.n_rounds++; R.flush(); emu_walk_lanes<FIXED, PAIR>(R, c, w, L, l0, l1, ev0); } while (0)
#define WT_MWALK_ROUND(FIXED, l0, l1, ev0) do { R.n_rounds++; R.flush(); emu_mwalk_lanes<FIXED>(R, c, w, L, l0, l1, ev0); } while (0)
#else
#ifdef WT_PROFILE
#define WT_WALK_ROUND_true(l0, l1, ev0) do { wt_walk_lane<true, PAIR>(P, c, w, L, 0u, tid, nt, tid == 0 ? prof : nullptr); \
        if (tid == 0) t_last = __builtin_readcyclecounter(); } while (0)
#else
#define WT_WALK_ROUND_true(l0, l1, ev0) wt_walk_lane<true, PAIR>(P, c, w, L, 0u, tid, nt)
#endif
#define WT_WALK_ROUND_false(l0, l1, ev0) if ((tid >> w.pair) >= l0 && (tid >> w.pair) < l1) wt_walk_lane<false, PAIR>(P, c, w, L, ev0, tid, nt)
#define WT_WALK_ROUND(FIXED, l0, l1, ev0) WT_WALK_ROUND_##FIXED(l0, l1, ev0)
#define WT_MWALK_ROUND_true(l0, l1, ev0) wt_mwalk_lane<true>(P, c, w, L, 0u, tid, nt)
#define WT_MWALK_ROUND_false(l0, l1, ev0) if ((tid >> 1) >= l0 && (tid >> 1) < l1) wt_mwalk_lane<false>(P, c, w, L, ev0, tid, nt)
#define WT_MWALK_ROUND(FIXED, l0, l1, ev0) WT_MWALK_ROUND_##FIXED(l0, l1, ev0)
#endif

// MedianReduction by walking (wt_walk.h): a lane carries its column of current values from one position to the next.
// T lanes (128: two workgroups per CU at 100 tracks) x S positions each; persistent workgroups, window tickets, ordered
// output through the look-back chain like the other kernels.
// (-DWT_PROFILE: cycles of wave 0: 0 zero + ranges, 1 count pass, 2 offsets, 3 scatter pass, 4 events, 5 first median, 6 moves
//  of the median (4-6: lane 0's view inside the walk), 7 everything else (run-count scan, look-back, write, ticket))
template <int MAXT, bool PAIR>
WT_KERNEL(wt_walk_kernel, (MAXT, 1), const WtParams P) {
    WT_LDS(wt_lds);
    WtCtx c{};
    c.sh = (WtShared *) (wt_lds + P.off_shared);
    WtDeltaCtx d;
    wt_delta_ctx_init(d, P, wt_lds);
    WtWalkCtx w;
    wt_walk_ctx_init(w, P, wt_lds, P.g_scratch + (size_t) WT_WG * (size_t) P.g_scratch_slab);
    w.pair = PAIR ? 1 : 0;                      // (== P.walk_pair: a constant of this instantiation from here on)
    w.mwu = 0;                                  // (... and so is this: the MWU branches of the shared phases fold away)
    WT_THREAD_IDS;
    WT_PROF_BEGIN;
    WT_DO() {
        if (tid == 0) {
            const long long k0 = (long long) wt_glb_add64(&P.counters[WT_CTR_TICKET], 1ull);
            c.sh->ticket = k0;
            if (k0 < P.n_windows) wt_phase_header(P, c, k0);
        }
    } WT_END
    WT_DO() { wt_walk_defaults(P, w, tid, nt); } WT_END
    WT_SYNC;
    for (;;) {
        const long long k = c.sh->ticket;
        if (k >= P.n_windows) break;
        WT_DO() { wt_walk_zero(P, c, w, tid, nt); } WT_END
        WT_DO() { wt_delta_ranges_w1(P, c, d, 0, tid, nt); } WT_END
        WT_SYNC;
        WT_DO() { wt_walk_ranges_w2(d, tid, nt); } WT_END
        WT_SYNC;
        WT_TICK(0);
        WT_DO() { wt_walk_pass<false>(P, c, w, d, 0u, 0u, tid, nt); } WT_END
        WT_SYNC;                                // the events are in the slab, the counts in cnt[]
        WT_TICK(1);
        WT_REG(L, WtWalkLane);
        // positions with events / emitted runs per lane, the window's run count: published before the walk
        WT_DO() { wt_walk_emits(P, c, w, WT_R(L), tid, nt); } WT_END
        WT_DO() { wt_walk_scan_a(w, wt_walk_emit_count(w, WT_R(L), tid), tid, nt); } WT_END
        WT_SYNC;
        WT_DO() { wt_walk_scan_b(w, tid, nt); } WT_END
        WT_SYNC;
        const unsigned long long mine = w.base[nt];
        WT_DO(k, mine) { if (tid == 0) wt_lookback_publish(P, c, k, mine); } WT_END
        if (w.novf[0] <= w.ov_cap) {            // (uniform) every position's events fit its slots + the overflow list
            WT_WALK_ROUND(true, 0, w.nstr, 0u);
            WT_SYNC;
            WT_TICK(7);
        } else {
            // a window denser than that: its events sorted by position into the same memory (a second pass over the
            // runs), as many lanes' worth at a time as fit
            WT_EMU_ONLY(R.n_fallback++;)
            WT_SYNC;                            // (base[] is about to hold the lanes' event offsets)
            WT_DO() { wt_walk_offsets1(P, w, tid, nt); } WT_END
            WT_SYNC;
            WT_DO() { wt_walk_scan_b(w, tid, nt); } WT_END
            WT_SYNC;
            WT_DO() { wt_walk_offsets2(P, w, tid, nt); } WT_END
            WT_SYNC;
            WT_TICK(2);
            for (int l0 = 0; l0 < w.nstr;) {        // (stretches)
                const int l1 = wt_walk_round_end(w, l0, nt);
                const uint32_t ev0 = w.base[l0 << w.pair], ev1 = w.base[l1 << w.pair];
                if (ev1 > ev0) {                    // (uniform)
                    WT_DO(ev0, ev1) { wt_walk_pass<true>(P, c, w, d, ev0, ev1, tid, nt); } WT_END
                    WT_SYNC;
                    WT_TICK(3);
                    WT_WALK_ROUND(false, l0, l1, ev0);
                    WT_SYNC;                        // before the next round reuses the slab
                    WT_TICK(7);
                }
                l0 = l1;
            }
            // the lanes' run offsets again (base[] held the event offsets meanwhile)
            WT_DO() { wt_walk_scan_a(w, wt_walk_emit_count(w, WT_R(L), tid), tid, nt); } WT_END
            WT_SYNC;
            WT_DO() { wt_walk_scan_b(w, tid, nt); } WT_END
            WT_SYNC;
        }
        WT_EMU_ONLY(if ((unsigned long long) w.base[nt] != mine) { fprintf(stderr, "wtemu: walking kernel: run count changed\n"); abort(); })
        WT_TICK(7);
        WT_DO(k, mine) { if (tid < 64) wt_lookback_complete(P, c, k, tid, mine); } WT_END
        WT_SYNC;
#ifdef WT_PROFILE_LB
        WT_TICK(2);                             // (experiment: the look-back's wait alone, in the "offsets" slot)
#endif
        WT_DO() { wt_walk_write(P, c, w, WT_R(L), tid, nt); } WT_END
        WT_SYNC;
#ifdef WT_PROFILE_LB
        WT_TICK(3);                             // (experiment: the write, in the "scatter" slot)
#endif
        WT_DO() {
            if (tid == 0) {
                wt_window_stats(P, c);
                const long long kn = (long long) wt_glb_add64(&P.counters[WT_CTR_TICKET], 1ull);
                c.sh->ticket = kn;
                if (kn < P.n_windows) wt_phase_header(P, c, kn);
            }
        } WT_END
        WT_SYNC;
        WT_TICK(7);
    }
    WT_PROF_END;
    WT_KERNEL_END;
}

// MWUReduction by walking (wt_mwalk.h): the same window machinery; the two lanes of a stretch hold one SET each.  Which
// positions emit a run is only known once the events have been applied (tracks in play per set), so the window's run count
// goes to the look-back chain after the walk.
template <int MAXT>
WT_KERNEL(wt_mwalk_kernel, (MAXT, 1), const WtParams P) {
    WT_LDS(wt_lds);
    WtCtx c{};
    c.sh = (WtShared *) (wt_lds + P.off_shared);
    WtDeltaCtx d;
    wt_delta_ctx_init(d, P, wt_lds);
    WtWalkCtx w;
    wt_walk_ctx_init(w, P, wt_lds, P.g_scratch + (size_t) WT_WG * (size_t) P.g_scratch_slab);
    w.pair = 1; w.mwu = 1;
    WT_THREAD_IDS;
    WT_DO() {
        if (tid == 0) {
            const long long k0 = (long long) wt_glb_add64(&P.counters[WT_CTR_TICKET], 1ull);
            c.sh->ticket = k0;
            if (k0 < P.n_windows) wt_phase_header(P, c, k0);
        }
    } WT_END
    WT_DO() { wt_walk_defaults(P, w, tid, nt); } WT_END
    WT_SYNC;
    for (;;) {
        const long long k = c.sh->ticket;
        if (k >= P.n_windows) break;
        WT_DO() { wt_walk_zero(P, c, w, tid, nt); } WT_END
        WT_DO() { wt_delta_ranges_w1(P, c, d, 0, tid, nt); } WT_END
        WT_SYNC;
        WT_DO() { wt_walk_ranges_w2(d, tid, nt); } WT_END
        WT_SYNC;
        WT_DO() { wt_walk_pass<false>(P, c, w, d, 0u, 0u, tid, nt); } WT_END
        WT_SYNC;                                // the events are in the slab, the counts in cnt[]
        WT_REG(L, WtWalkLane);
        WT_DO() { wt_mwalk_events(P, c, w, WT_R(L), tid, nt); } WT_END
        if (w.novf[0] <= w.ov_cap) {            // (uniform) every position's events fit its slots + the overflow list
            WT_MWALK_ROUND(true, 0, w.nstr, 0u);
            WT_SYNC;
        } else {
            // a window denser than that: its events sorted by position into the same memory, as many stretches at a time as fit
            WT_EMU_ONLY(R.n_fallback++;)
            WT_SYNC;
            WT_DO() { wt_walk_offsets1(P, w, tid, nt); } WT_END
            WT_SYNC;
            WT_DO() { wt_walk_scan_b(w, tid, nt); } WT_END
            WT_SYNC;
            WT_DO() { wt_walk_offsets2(P, w, tid, nt); } WT_END
            WT_SYNC;
            for (int l0 = 0; l0 < w.nstr;) {
                const int l1 = wt_walk_round_end(w, l0, nt);
                const uint32_t ev0 = w.base[l0 << 1], ev1 = w.base[l1 << 1];
                if (ev1 > ev0) {                    // (uniform)
                    WT_DO(ev0, ev1) { wt_walk_pass<true>(P, c, w, d, ev0, ev1, tid, nt); } WT_END
                    WT_SYNC;
                    WT_MWALK_ROUND(false, l0, l1, ev0);
                    WT_SYNC;                        // before the next round reuses the slab
                }
                l0 = l1;
            }
        }
        // the lanes' run offsets, the window's run count
        WT_DO() { wt_walk_scan_a(w, wt_walk_emit_count(w, WT_R(L), tid), tid, nt); } WT_END
        WT_SYNC;
        WT_DO() { wt_walk_scan_b(w, tid, nt); } WT_END
        WT_SYNC;
        const unsigned long long mine = w.base[nt];
        WT_DO(k, mine) { if (tid == 0) wt_lookback_publish(P, c, k, mine); } WT_END
        WT_DO(k, mine) { if (tid < 64) wt_lookback_complete(P, c, k, tid, mine); } WT_END
        WT_SYNC;
        WT_DO() { wt_mwalk_write(P, c, w, WT_R(L), tid, nt); } WT_END
        WT_SYNC;
        WT_DO() {
            if (tid == 0) {
                wt_window_stats(P, c);
                const long long kn = (long long) wt_glb_add64(&P.counters[WT_CTR_TICKET], 1ull);
                c.sh->ticket = kn;
                if (kn < P.n_windows) wt_phase_header(P, c, kn);
            }
        } WT_END
        WT_SYNC;
    }
    WT_KERNEL_END;
}

#endif  // WT_WALK_KERNEL_H_
