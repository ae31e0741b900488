// wt_delta_kernel.h -- wt_delta_kernel as a template (logic in wt_delta.h), instantiated by wt_delta_kernels.hip and, one at a
// time, by tools/kernel_asm.py.  One text (wt_exec.h): hipcc compiles it for gfx950, tests/emu/wt_emu.cpp runs the same body on
// the CPU -- there with WT_DELTA_EARLY_PUBLISH 0: Sum / Mean follow the body's other branch, not EP (wave code throughout).
#ifndef WT_DELTA_KERNEL_H_
#define WT_DELTA_KERNEL_H_

#include "wt_reduce_kernel.h"       // (the device's includes, wt_exec.h)

// Exact difference-array path for Sum / Mean over float tracks (wt_delta.h): O(intervals) work
// instead of O(tracks x runs); LDS independent of the track count.
// (var / stddev / CV also accumulate the sum of squares: 512 lanes, one workgroup per CU)
#define WT_DELTA_SQ(OP) ((OP) == WT_OP_VAR || (OP) == WT_OP_STDDEV || (OP) == WT_OP_ENTROPY || (OP) == WT_OP_CV || (OP) == WT_OP_TTEST)
#ifndef WT_DELTA_MIN_WAVES
#define WT_DELTA_MIN_WAVES 4     // waves per SIMD the register allocation aims at (experiments: 6 spills, see DESIGN A.1)
#endif
#ifndef WT_DELTA_SQ_BLOCK
#define WT_DELTA_SQ_BLOCK WT_DELTA_SQ_T0   // workgroup of the launches that also accumulate squares (768: three wavefronts per SIMD, 168 registers; the scans: the first 512 lanes, see wt_make_delta_plan)
#endif
#ifndef WT_DELTA_ZERO_EARLY
#define WT_DELTA_ZERO_EARLY 1      // the accumulators are zeroed beside lane 0's ticket + header chain (0: at the window's start, rounds 1-5): -2 % at every density
#endif
#ifndef WT_DELTA_EARLY_PUBLISH
#define WT_DELTA_EARLY_PUBLISH 1
#endif
#ifndef WT_DELTA_BLOCK
#define WT_DELTA_BLOCK 1024     // (launch bound; the plan's default, see wt_make_delta_plan)
#endif
// DF: some track's default is non-zero (Sum / Mean; P.delta_df)
// U: runs per lane and tile of the pass (round 6: 4, or 2 for launches whose windows hold few tiles per wavefront -- wt_delta_launch)
template <int OP, bool DF = false, int U = WT_DELTA_U>
WT_KERNEL(wt_delta_kernel, (WT_DELTA_SQ(OP) ? WT_DELTA_SQ_BLOCK : WT_DELTA_BLOCK, WT_DELTA_SQ(OP) ? 3 : WT_DELTA_MIN_WAVES), const WtParams P) {
    WT_LDS(wt_lds);
    WtCtx c;
    wt_ctx_init(c, P, wt_lds);
    WtDeltaCtx d;
    wt_delta_ctx_init(d, P, wt_lds);
    constexpr bool QQ = WT_DELTA_SQ(OP);
    constexpr bool TT = OP == WT_OP_TTEST;      // two sets per position (wt_delta_scan3_tt)
    constexpr bool MM = OP == WT_OP_MAX || OP == WT_OP_MIN;     // range updates of a segment tree (wt_delta_apply_mm)
    constexpr bool EP = WT_DELTA_EARLY_PUBLISH && (OP == WT_OP_SUM || OP == WT_OP_MEAN);       // the run count is published before the values are computed (wt_delta_scan3_cov / _val)
    WT_REG(DL, WtDeltaLane);
    WT_REG(DL2, WtDeltaLane2);
    (void) DL; (void) DL2;
    WT_REG(L, WtLane<WT_DELTA_K>);
    WT_REG_INIT(ep_rank, 0, uint32_t); WT_REG_INIT(ep_em, 0, uint32_t);     // EP: the lane's first rank among the window's emitted runs, its emitted byte
    (void) ep_rank; (void) ep_em;
    WT_THREAD_IDS;              // (below the lane registers: above them the Sum / Mean kernels come out with another scalar register assignment)
    // lanes of the scans and the staging (8 positions each): all of them -- or, with squares, the first 512 of 1024.  (Sum / Mean must not
    // see a run-time bound here: the guard alone cost wt_delta_kernel<mean> 31 more spilled registers and a quarter more HBM traffic.)
    const int nts = QQ ? P.W / WT_DELTA_K : nt;
#define WT_SCAN_LANE (!QQ || tid < nts)
    int guess = 0;              // the workgroup's unit exponent (0: none yet); uniform across the lanes
    long long k_dbg = -1;
    (void) k_dbg;
    WT_PROF_BEGIN;
    // ticket handling: see wt_reduce_kernel; lane 0 also prepares the next window's header there,
    // so that the first phase of a window needs no barrier of its own
    WT_DO() {
        if (tid == 0) {
            const long long k0 = (long long) wt_glb_add64(&P.counters[WT_CTR_TICKET], 1ull);
            c.sh->ticket = k0;
            if (k0 < P.n_windows) wt_phase_header(P, c, k0);
        }
    } WT_END
#if WT_DELTA_ZERO_EARLY
    // (experiment: the accumulators are zeroed beside lane 0's ticket + header chain, before the barrier that publishes the header)
    if constexpr (MM) WT_DO() { wt_delta_zero_mm<OP == WT_OP_MAX>(P, c, d, tid, nt); } WT_END
    else WT_DO() { wt_delta_zero<QQ, TT>(P, c, d, tid, nt); } WT_END
#endif
    WT_SYNC;
    for (;;) {
        WT_MARK(101);
        const long long k = c.sh->ticket;
        k_dbg = k;
        if (k >= P.n_windows) break;
        const int nchunks = (P.n_tracks + nt - 1) / nt;
        auto ntr = [&](int ch) { const int r = P.n_tracks - ch * nt; return r < nt ? r : nt; };     // tracks of chunk ch
#if !WT_DELTA_ZERO_EARLY
        if constexpr (MM) WT_DO() { wt_delta_zero_mm<OP == WT_OP_MAX>(P, c, d, tid, nt); } WT_END
        else WT_DO() { wt_delta_zero<QQ, TT>(P, c, d, tid, nt); } WT_END
#endif
        WT_TICK(0);
        WT_MARK(102);
        int scale = 1;
        if constexpr (MM) {
            // one pass, no unit exponent: a float's order-preserving key needs none
            for (int ch = 0; ch < nchunks; ch++) {
                WT_DO(ch) { wt_delta_ranges_w1(P, c, d, ch * nt, tid, nt); } WT_END
                WT_SYNC;
                WT_DELTA_RANGES_W2(P, c, d, tid, nt, 64u * U);
                WT_SYNC;
                WT_TICK(1);
                WT_DO() { wt_delta_pass_mm<OP == WT_OP_MAX>(P, c, d, tid, nt); } WT_END
                WT_SYNC;
                WT_TICK(3);
            }
            WT_DO(k) { if (tid == 0 && d.dsh->bad) wt_delta_mark_bad(P, c, k); } WT_END   // a NaN or a -0.0: the general kernel's window
        } else if (guess == 0) {
            // no unit exponent known to this workgroup yet: exponent-range pass, then the delta pass
            for (int ch = 0; ch < nchunks; ch++) {
                WT_DO(ch) { wt_delta_ranges_w1(P, c, d, ch * nt, tid, nt); } WT_END
                WT_SYNC;
                WT_DELTA_RANGES_W2(P, c, d, tid, nt, 64u * U);
                WT_SYNC;
                WT_TICK(1);
                WT_DO() { wt_delta_pass1<U>(P, c, d, tid, nt); } WT_END
                WT_SYNC;
                WT_TICK(2);
            }
            const bool any = d.dsh->emin <= d.dsh->emax;
            const bool ok = wt_delta_verdict(P, d, scale);
            WT_DO(k, ok) { if (!ok && tid == 0) wt_delta_mark_bad(P, c, k); } WT_END
            for (int ch = 0; ch < nchunks; ch++) {
                if (nchunks > 1) {
                    WT_DO(ch) { wt_delta_ranges_w1(P, c, d, ch * nt, tid, nt); } WT_END
                    WT_SYNC;
                    WT_DELTA_RANGES_W2(P, c, d, tid, nt, 64u * U);
                    WT_SYNC;
                }
                WT_DO(scale, ok, ch) { wt_delta_pass2<QQ, DF, TT, U>(P, c, d, scale, ok, false, true, tid, nt, ntr(ch), ch * nt); } WT_END
                WT_SYNC;
                WT_TICK(3);
            }
            if (any && ok) guess = scale;
        } else {
            // speculative single pass with the workgroup's unit (wt_delta_window_verdict)
            for (int ch = 0; ch < nchunks; ch++) {
                WT_DO(ch) { wt_delta_ranges_w1(P, c, d, ch * nt, tid, nt); } WT_END
                WT_SYNC;
                WT_DELTA_RANGES_W2(P, c, d, tid, nt, 64u * U);
                WT_SYNC;
                WT_TICK(1);
                WT_DO(guess, ch) { wt_delta_pass2<QQ, DF, TT, U>(P, c, d, guess, true, true, true, tid, nt, ntr(ch), ch * nt); } WT_END
                WT_SYNC;
                WT_TICK(3);
            }
            int lo;
            bool ok;
            scale = guess;
            if (!wt_delta_window_verdict(P, d, guess, lo, ok)) {      // workgroup-uniform
              if (!ok) {
                // not provably exact whatever the unit: the patch kernel rewrites this window's values, and everything
                // else about it -- breakpoints, coverage, run count -- is in place after the speculative pass.  (It used
                // to be redone like the windows below: twice the time of a window, during which every later window sat
                // in its look-back; 5 % such windows cost the kernel a third more time, round 4.)
                WT_DO(k) { if (tid == 0) wt_delta_mark_bad(P, c, k); } WT_END
              } else {
                WT_EMU_ONLY(R.n_redo++;)
                WT_SYNC;            // every lane has read the verdict fields
                WT_DO() { wt_delta_rezero<QQ, TT>(P, c, d, tid, nt); } WT_END
                WT_SYNC;
                for (int ch = 0; ch < nchunks; ch++) {
                    if (nchunks > 1) {
                        WT_DO(ch) { wt_delta_ranges_w1(P, c, d, ch * nt, tid, nt); } WT_END
                        WT_SYNC;
                        WT_DELTA_RANGES_W2(P, c, d, tid, nt, 64u * U);
                        WT_SYNC;
                    }
                    WT_DO(lo, ok, ch) { wt_delta_pass2<QQ, DF, TT, U>(P, c, d, lo, ok, false, false, tid, nt, ntr(ch), ch * nt); } WT_END
                    WT_SYNC;
                }
                scale = lo;
                guess = lo;
              }
            }
        }
        WT_MARK(105);
        if constexpr (TT) {
            // the scans split by set over 2 nts lanes, then one lane per position (wt_delta.h: phases A - C)
            WT_DELTA_SCAN_W1_TT(if (tid < 2 * nts), P, c, d, WT_R(DL2), tid, nts);
            WT_SYNC;
            WT_MARK(107);
            WT_DO(scale) { if (tid < 2 * nts) wt_delta_scan3_tt(P, c, d, WT_R(DL2), scale, tid, nts); } WT_END
            WT_SYNC;
            WT_DO() { wt_delta_combine_tt(P, c, d, tid, nt); } WT_END
            WT_SYNC;
            // a position whose variance cancels too much for the exact sums (wt_delta_scan3_tt): the window's values are the general kernel's
            WT_DO(k) { if (tid == 0 && d.dsh->risk && c.sh->bad_slot < 0) wt_delta_mark_bad(P, c, k); } WT_END
        } else if constexpr (MM) {
            WT_REG_INIT(wc_mm, 0, int32_t);
            WT_DELTA_SCAN_W1_MM(P, c, d, WT_R(wc_mm), tid, nt);
            WT_SYNC;
            WT_MARK(107);
            WT_DO() { wt_delta_scan3_mm<OP == WT_OP_MAX>(P, c, d, WT_R(wc_mm), WT_R(L), tid, nt); } WT_END
            WT_SYNC;
        } else if constexpr (EP) {
            // Sum / Mean: the bytes of the breakpoint / emitted bitmaps first ...
            WT_DELTA_SCAN_W1(, QQ, P, c, d, WT_R(DL), tid, nts);
            WT_SYNC;
            WT_MARK(107);
            WT_DO() { WT_R(ep_rank) = wt_delta_scan3_cov(P, c, d, WT_R(DL), WT_R(ep_em), tid, nts); } WT_END
            WT_SYNC;
        } else {
            WT_DELTA_SCAN_W1(if (WT_SCAN_LANE), QQ, P, c, d, WT_R(DL), tid, nts);
            WT_SYNC;
            WT_MARK(107);
            WT_DO(scale) { if (WT_SCAN_LANE) wt_delta_scan3<OP>(P, c, d, WT_R(DL), WT_R(L), scale, tid, nts); } WT_END
            WT_SYNC;
        }
        WT_TICK(4);
        WT_MARK(108);
        // wave 0: run-count scan and look-back back to back (it owns the counts); the last lanes
        // build the breakpoint jump table meanwhile
        WT_REG_INIT(mine, 0, unsigned long long);
        if constexpr (EP) {
            // the wavefronts' run counts are in epfx[0 .. nwaves): this one's first rank, and -- wave 0 -- the window's count, published at once
            WT_DO(k, scale) {
                const int lane_ = tid & 63;
                if (tid < 64) {
                    WT_R(mine) = wt_waves_before32(c.epfx, 0, nt >> 6, lane_);
                    WT_TICK(5);
                    if (tid == 0) wt_lookback_publish(P, c, k, WT_R(mine));
                }
                WT_R(ep_rank) += wt_waves_before32(c.epfx, 0, tid >> 6, lane_);
                // ... the count is out; now the values (wt_delta_scan3_val: nobody waits for them but this window's own staging)
                wt_delta_scan3_val<OP>(P, c, d, WT_R(DL), WT_R(L), scale, tid, nts);
            } WT_END
        } else {
            WT_DO(k) {
                if (tid < 64) {
                    WT_R(mine) = wt_delta_escan_wave(P, c, tid);
                    WT_TICK(5);
                    if (tid == 0) wt_lookback_publish(P, c, k, WT_R(mine));
                }
            } WT_END
        }
        WT_DO() { wt_delta_nextw(P, c, tid, nt); } WT_END
        WT_SYNC;
        WT_MARK(110);
        // the look-back's round trips to the status words overlap the staging of the other waves
        // (and the predecessors get that much longer to publish)
        WT_DO(k) {
            if (tid < 64) {
                wt_lookback_complete(P, c, k, tid, WT_R(mine));
                if constexpr (!EP) wt_delta_note_offset(P, c, tid);     // (lane 0 set the offset in the look-back: same wave, LDS in order)
            }
        } WT_END
        WT_TICK(6);
        if constexpr (TT) {
            // two-sample launches: the Student tail of every emitted position is what the look-back of wave 0 overlaps -- the other
            // wavefronts share the window's positions.  Two barriers before the staging: the first, because a scan lane's 8 results
            // were written by other wavefronts' lanes (wt_delta_tail_tt); the second, because the staging reuses what the results
            // lie in -- with the spare entries of WT_STAGE_AT, run number 1986 and later of a 2048-bp window are staged at
            // acc[W ..], the results of the window's first positions, which their own lanes must have loaded by then
            WT_DO() { if (tid >= 64) wt_delta_tail_tt(P, d, tid - 64, nt - 64); } WT_END
            WT_SYNC;
            WT_TICK(2);             // (profile builds: the tail, less the look-back, in the slot of the exponent-range pass)
            WT_DO() { if (tid < nts) wt_delta_load_res_tt(P, d, WT_R(L), tid); } WT_END
            WT_SYNC;
        }
        if constexpr (EP) WT_DO() { wt_delta_stage_ep<OP>(P, c, d, WT_R(L), WT_R(ep_em), WT_R(DL).evmask, WT_R(ep_rank), tid, nts); } WT_END
        else WT_DO() { if (WT_SCAN_LANE) wt_delta_stage<OP>(P, c, d, WT_R(L), tid, nts); } WT_END
        WT_SYNC;
        if constexpr (EP) WT_DO() { if (tid < 64) wt_delta_note_offset_ep(P, c, tid); } WT_END
#ifdef WT_PROFILE_TAIL
        WT_TICK(2);                 // (experiment: the tail of a window apart -- staging here, copy-out in "write", ticket + header in "zero")
#endif
        WT_DO() { wt_delta_copy_out(P, c, d, tid, nt); } WT_END
        WT_SYNC;
#ifdef WT_PROFILE_TAIL
        WT_TICK(7);
#endif
        WT_MARK(111);
        WT_DO() {
            if (tid == 0) {
                wt_window_stats(P, c);
                const long long kn = (long long) wt_glb_add64(&P.counters[WT_CTR_TICKET], 1ull);
                c.sh->ticket = kn;
                if (kn < P.n_windows) wt_phase_header(P, c, kn);
            }
        } WT_END
#if WT_DELTA_ZERO_EARLY
        if constexpr (MM) WT_DO() { wt_delta_zero_mm<OP == WT_OP_MAX>(P, c, d, tid, nt); } WT_END
        else WT_DO() { wt_delta_zero<QQ, TT>(P, c, d, tid, nt); } WT_END
#endif
        WT_SYNC;
#ifdef WT_PROFILE_TAIL
        WT_TICK(0);
#else
        WT_TICK(7);
#endif
    }
    WT_PROF_END;
    WT_KERNEL_END;
}

#undef WT_SCAN_LANE

#endif  // WT_DELTA_KERNEL_H_
