// wt_delta_kernel.h -- wt_delta_kernel as a template (logic in wt_delta.h), instantiated by wt_delta_kernels.hip and, one at a
// time, by tools/kernel_asm.py.  Compiled only by hipcc --offload-arch=gfx950.
#ifndef WT_DELTA_KERNEL_H_
#define WT_DELTA_KERNEL_H_

#include "wt_reduce_kernel.h"       // WT_MARK, WT_TICK

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
__global__ void __launch_bounds__(WT_DELTA_SQ(OP) ? WT_DELTA_SQ_BLOCK : WT_DELTA_BLOCK, WT_DELTA_SQ(OP) ? 3 : WT_DELTA_MIN_WAVES) wt_delta_kernel(const WtParams P) {
    extern __shared__ __attribute__((aligned(16))) char wt_lds[];
    WtCtx c;
    wt_ctx_init(c, P, wt_lds);
    WtDeltaCtx d;
    wt_delta_ctx_init(d, P, wt_lds);
    constexpr bool QQ = WT_DELTA_SQ(OP);
    constexpr bool TT = OP == WT_OP_TTEST;      // two sets per position (wt_delta_scan3_tt)
    constexpr bool MM = OP == WT_OP_MAX || OP == WT_OP_MIN;     // range updates of a segment tree (wt_delta_apply_mm)
    constexpr bool EP = WT_DELTA_EARLY_PUBLISH && (OP == WT_OP_SUM || OP == WT_OP_MEAN);       // the run count is published before the values are computed (wt_delta_scan3_cov / _val)
    WtDeltaLane DL;
    WtDeltaLane2 DL2;
    (void) DL; (void) DL2;
    WtLane<WT_DELTA_K> L;
    uint32_t ep_rank = 0, ep_em = 0;        // EP: the lane's first rank among the window's emitted runs, its emitted byte
    (void) ep_rank; (void) ep_em;
    const int tid = threadIdx.x, nt = blockDim.x;
    // lanes of the scans and the staging (8 positions each): all of them -- or, with squares, the first 512 of 1024.  (Sum / Mean must not
    // see a run-time bound here: the guard alone cost wt_delta_kernel<mean> 31 more spilled registers and a quarter more HBM traffic.)
    const int nts = QQ ? P.W / WT_DELTA_K : nt;
#define WT_SCAN_LANE (!QQ || tid < nts)
    int guess = 0;              // the workgroup's unit exponent (0: none yet); uniform across the lanes
    long long k_dbg = -1;
    (void) k_dbg;
#ifdef WT_PROFILE
    unsigned long long prof[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long t_last = __builtin_readcyclecounter();
#endif
    // ticket handling: see wt_reduce_kernel; lane 0 also prepares the next window's header there,
    // so that the first phase of a window needs no barrier of its own
    if (tid == 0) {
        const long long k0 = (long long) wt_glb_add64(&P.counters[WT_CTR_TICKET], 1ull);
        c.sh->ticket = k0;
        if (k0 < P.n_windows) wt_phase_header(P, c, k0);
    }
#if WT_DELTA_ZERO_EARLY
    // (experiment: the accumulators are zeroed beside lane 0's ticket + header chain, before the barrier that publishes the header)
    if constexpr (MM) wt_delta_zero_mm<OP == WT_OP_MAX>(P, c, d, tid, nt);
    else wt_delta_zero<QQ, TT>(P, c, d, tid, nt);
#endif
    __syncthreads();
    for (;;) {
        WT_MARK(101);
        const long long k = c.sh->ticket;
        k_dbg = k;
        if (k >= P.n_windows) break;
        const int nchunks = (P.n_tracks + nt - 1) / nt;
        auto ntr = [&](int ch) { const int r = P.n_tracks - ch * nt; return r < nt ? r : nt; };     // tracks of chunk ch
#if !WT_DELTA_ZERO_EARLY
        if constexpr (MM) wt_delta_zero_mm<OP == WT_OP_MAX>(P, c, d, tid, nt);
        else wt_delta_zero<QQ, TT>(P, c, d, tid, nt);
#endif
        WT_TICK(0);
        WT_MARK(102);
        int scale = 1;
        if constexpr (MM) {
            // one pass, no unit exponent: a float's order-preserving key needs none
            for (int ch = 0; ch < nchunks; ch++) {
                wt_delta_ranges_w1(P, c, d, ch * nt, tid, nt);
                __syncthreads();
                wt_delta_ranges_w2(P, c, d, tid, nt, 64u * U);
                __syncthreads();
                WT_TICK(1);
                wt_delta_pass_mm<OP == WT_OP_MAX>(P, c, d, tid, nt);
                __syncthreads();
                WT_TICK(3);
            }
            if (tid == 0 && d.dsh->bad) wt_delta_mark_bad(P, c, k);     // a NaN or a -0.0: the general kernel's window
        } else if (guess == 0) {
            // no unit exponent known to this workgroup yet: exponent-range pass, then the delta pass
            for (int ch = 0; ch < nchunks; ch++) {
                wt_delta_ranges_w1(P, c, d, ch * nt, tid, nt);
                __syncthreads();
                wt_delta_ranges_w2(P, c, d, tid, nt, 64u * U);
                __syncthreads();
                WT_TICK(1);
                wt_delta_pass1<U>(P, c, d, tid, nt);
                __syncthreads();
                WT_TICK(2);
            }
            const bool any = d.dsh->emin <= d.dsh->emax;
            const bool ok = wt_delta_verdict(P, d, scale);
            if (!ok && tid == 0) wt_delta_mark_bad(P, c, k);
            for (int ch = 0; ch < nchunks; ch++) {
                if (nchunks > 1) {
                    wt_delta_ranges_w1(P, c, d, ch * nt, tid, nt);
                    __syncthreads();
                    wt_delta_ranges_w2(P, c, d, tid, nt, 64u * U);
                    __syncthreads();
                }
                wt_delta_pass2<QQ, DF, TT, U>(P, c, d, scale, ok, false, true, tid, nt, ntr(ch), ch * nt);
                __syncthreads();
                WT_TICK(3);
            }
            if (any && ok) guess = scale;
        } else {
            // speculative single pass with the workgroup's unit (wt_delta_window_verdict)
            for (int ch = 0; ch < nchunks; ch++) {
                wt_delta_ranges_w1(P, c, d, ch * nt, tid, nt);
                __syncthreads();
                wt_delta_ranges_w2(P, c, d, tid, nt, 64u * U);
                __syncthreads();
                WT_TICK(1);
                wt_delta_pass2<QQ, DF, TT, U>(P, c, d, guess, true, true, true, tid, nt, ntr(ch), ch * nt);
                __syncthreads();
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
                if (tid == 0) wt_delta_mark_bad(P, c, k);
              } else {
                __syncthreads();            // every lane has read the verdict fields
                wt_delta_rezero<QQ, TT>(P, c, d, tid, nt);
                __syncthreads();
                for (int ch = 0; ch < nchunks; ch++) {
                    if (nchunks > 1) {
                        wt_delta_ranges_w1(P, c, d, ch * nt, tid, nt);
                        __syncthreads();
                        wt_delta_ranges_w2(P, c, d, tid, nt, 64u * U);
                        __syncthreads();
                    }
                    wt_delta_pass2<QQ, DF, TT, U>(P, c, d, lo, ok, false, false, tid, nt, ntr(ch), ch * nt);
                    __syncthreads();
                }
                scale = lo;
                guess = lo;
              }
            }
        }
        WT_MARK(105);
        if constexpr (TT) {
            // the scans split by set over 2 nts lanes, then one lane per position (wt_delta.h: phases A - C)
            if (tid < 2 * nts) wt_delta_scan_w1_tt(P, c, d, DL2, tid, nts);
            __syncthreads();
            WT_MARK(107);
            if (tid < 2 * nts) wt_delta_scan3_tt(P, c, d, DL2, scale, tid, nts);
            __syncthreads();
            wt_delta_combine_tt(P, c, d, tid, nt);
            __syncthreads();
            // a position whose variance cancels too much for the exact sums (wt_delta_scan3_tt): the window's values are the general kernel's
            if (tid == 0 && d.dsh->risk && c.sh->bad_slot < 0) wt_delta_mark_bad(P, c, k);
        } else if constexpr (MM) {
            int32_t wc_mm = 0;
            wt_delta_scan_w1_mm(P, c, d, wc_mm, tid, nt);
            __syncthreads();
            WT_MARK(107);
            wt_delta_scan3_mm<OP == WT_OP_MAX>(P, c, d, wc_mm, L, tid, nt);
            __syncthreads();
        } else if constexpr (EP) {
            // Sum / Mean: the bytes of the breakpoint / emitted bitmaps first ...
            wt_delta_scan_w1<QQ>(P, c, d, DL, tid, nts);
            __syncthreads();
            WT_MARK(107);
            ep_rank = wt_delta_scan3_cov(P, c, d, DL, ep_em, tid, nts);
            __syncthreads();
        } else {
            if (WT_SCAN_LANE) wt_delta_scan_w1<QQ>(P, c, d, DL, tid, nts);
            __syncthreads();
            WT_MARK(107);
            if (WT_SCAN_LANE) wt_delta_scan3<OP>(P, c, d, DL, L, scale, tid, nts);
            __syncthreads();
        }
        WT_TICK(4);
        WT_MARK(108);
        // wave 0: run-count scan and look-back back to back (it owns the counts); the last lanes
        // build the breakpoint jump table meanwhile
        unsigned long long mine = 0;
        if constexpr (EP) {
            // the wavefronts' run counts are in epfx[0 .. nwaves): this one's first rank, and -- wave 0 -- the window's count, published at once
            const int lane_ = tid & 63;
            if (tid < 64) {
                mine = wt_waves_before32(c.epfx, 0, nt >> 6, lane_);
                WT_TICK(5);
                if (tid == 0) wt_lookback_publish(P, c, k, mine);
            }
            ep_rank += wt_waves_before32(c.epfx, 0, tid >> 6, lane_);
            // ... the count is out; now the values (wt_delta_scan3_val: nobody waits for them but this window's own staging)
            wt_delta_scan3_val<OP>(P, c, d, DL, L, scale, tid, nts);
        } else if (tid < 64) {
            mine = wt_delta_escan_wave(P, c, tid);
            WT_TICK(5);
            if (tid == 0) wt_lookback_publish(P, c, k, mine);
        }
        wt_delta_nextw(P, c, tid, nt);
        __syncthreads();
        WT_MARK(110);
        // the look-back's round trips to the status words overlap the staging of the other waves
        // (and the predecessors get that much longer to publish)
        if (tid < 64) {
            wt_lookback_complete(P, c, k, tid, mine);
            if constexpr (!EP) wt_delta_note_offset(P, c, tid);     // (lane 0 set the offset in the look-back: same wave, LDS in order)
        }
        WT_TICK(6);
        if constexpr (TT) {
            // two-sample launches: the Student tail of every emitted position is what the look-back of wave 0 overlaps -- the other
            // wavefronts share the window's positions.  Two barriers before the staging: the first, because a scan lane's 8 results
            // were written by other wavefronts' lanes (wt_delta_tail_tt); the second, because the staging reuses what the results
            // lie in -- with the spare entries of WT_STAGE_AT, run number 1986 and later of a 2048-bp window are staged at
            // acc[W ..], the results of the window's first positions, which their own lanes must have loaded by then
            if (tid >= 64) wt_delta_tail_tt(P, d, tid - 64, nt - 64);
            __syncthreads();
            WT_TICK(2);             // (profile builds: the tail, less the look-back, in the slot of the exponent-range pass)
            if (tid < nts) wt_delta_load_res_tt(P, d, L, tid);
            __syncthreads();
        }
        if constexpr (EP) wt_delta_stage_ep<OP>(P, c, d, L, ep_em, DL.evmask, ep_rank, tid, nts);
        else if (WT_SCAN_LANE) wt_delta_stage<OP>(P, c, d, L, tid, nts);
        __syncthreads();
        if constexpr (EP) { if (tid < 64) wt_delta_note_offset_ep(P, c, tid); }
#ifdef WT_PROFILE_TAIL
        WT_TICK(2);                 // (experiment: the tail of a window apart -- staging here, copy-out in "write", ticket + header in "zero")
#endif
        wt_delta_copy_out(P, c, d, tid, nt);
        __syncthreads();
#ifdef WT_PROFILE_TAIL
        WT_TICK(7);
#endif
        WT_MARK(111);
        if (tid == 0) {
            wt_window_stats(P, c);
            const long long kn = (long long) wt_glb_add64(&P.counters[WT_CTR_TICKET], 1ull);
            c.sh->ticket = kn;
            if (kn < P.n_windows) wt_phase_header(P, c, kn);
        }
#if WT_DELTA_ZERO_EARLY
        if constexpr (MM) wt_delta_zero_mm<OP == WT_OP_MAX>(P, c, d, tid, nt);
        else wt_delta_zero<QQ, TT>(P, c, d, tid, nt);
#endif
        __syncthreads();
#ifdef WT_PROFILE_TAIL
        WT_TICK(0);
#else
        WT_TICK(7);
#endif
    }
#ifdef WT_PROFILE
    if (tid == 0)
        for (int q = 0; q < 8; q++) wt_glb_add64(&P.counters[WT_CTR_PROF + q], prof[q]);
#endif
}

#undef WT_SCAN_LANE

#endif  // WT_DELTA_KERNEL_H_
