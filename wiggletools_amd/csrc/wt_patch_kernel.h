// wt_patch_kernel.h -- wt_patch_kernel as a template (logic in wt_core.h).  One text (wt_exec.h): wt_patch_kernels.hip compiles
// it for gfx950 and holds its launch entry, tests/emu/wt_emu.cpp runs the same body on the CPU.
#ifndef WT_PATCH_KERNEL_H_
#define WT_PATCH_KERNEL_H_

#include "wt_reduce_kernel.h"       // WT_MAX_BLOCK, WT_MIN_WAVES

// Patch kernel: the general bitmap multiplexer over just the windows the difference-array kernel
// could not prove exact (a NaN, an Inf, too wide a dynamic range).  That kernel has already emitted
// those windows' runs -- coordinates, run count, position in the output -- so this one only has
// to recompute their values in the reference's own summation order and store them at the recorded
// offsets: no ticket, no look-back, no statistics.  One difference-array window (8192 bp) is
// `ratio` general windows; the difference-array kernel recorded the run offset of 16 sub-ranges of
// every such window, so every (window, sub-window) pair is a work item of its own.

template <int OP, int K, bool MULTI>
WT_KERNEL(wt_patch_kernel, (WT_MAX_BLOCK, WT_MIN_WAVES(K)), const WtParams P, const WtPatchArgs Q) {
    typedef float ValT;
    typedef float ScrT;
    WT_LDS(wt_lds);
    WtCtx c;
    wt_ctx_init(c, P, wt_lds);
    WT_REG(L, WtLane<K>);
    WT_THREAD_IDS;
    const long long n_bad = (long long) *Q.n_bad;
    const int N = P.n_tracks, NC = MULTI ? P.chunk_tracks : N, n_chunks = MULTI ? P.n_chunks : 1;
    // work items = (window the difference-array kernel recorded, narrower window h inside it): independent of one
    // another -- the recording kernel left the run offset of every sub-range (wt_delta_note_offset)
    const long long n_items = n_bad * Q.ratio;
    for (long long item = WT_WG; item < n_items; item += WT_NWG) {
        const long long j = item / Q.ratio;
        const int h = (int) (item - j * Q.ratio);
        const long long kd = Q.bad_list[j];
        const int ch = Q.d_win_chrom[kd];
        const long long m = kd - Q.d_c_first_win[ch];
        const long long goff = Q.bad_goff[j * WT_BAD_SUB + h * (WT_BAD_SUB / Q.ratio)];
        {
            const long long mg = m * Q.ratio + h;
            if (mg >= P.c_nwin[ch]) continue;               // workgroup-uniform
            const long long k = P.c_first_win[ch] + mg;
            WT_SYNC;                                        // the previous window is done with the shared block
            WT_DO(k) { if (tid == 0) wt_phase_header(P, c, k); } WT_END
            WT_DO() { wt_phase_zero(P, c, true, tid, nt); } WT_END
            WT_SYNC;
            // same sweeps as wt_reduce_kernel (chunked tracks: the first evaluation pass rides on the
            // sweep that builds the bitmaps; var / stddev / CV take a second one)
            constexpr int npass = wt_eval_passes(OP);
            WT_REG(A, WtAcc<K>);
            WT_DO() { wt_eval_init<OP, K>(WT_R(A)); } WT_END
            for (int cc = 0; cc < n_chunks; cc++) {
                const int t_lo = cc * NC, t_hi = (t_lo + NC < N) ? t_lo + NC : N;
                if (MULTI && cc > 0) {
                    WT_DO() { wt_phase_zero(P, c, false, tid, nt); } WT_END
                    WT_SYNC;
                }
                WT_DO(t_lo, t_hi) { wt_phase_load<ValT>(P, c, t_lo, t_hi, false, tid, nt); } WT_END
                WT_SYNC;
                WT_DO(t_lo, t_hi) { wt_phase_count_a(P, c, t_lo, t_hi, tid, nt); } WT_END
                WT_SYNC;
                WT_DO(t_lo, t_hi) { wt_phase_count_b(P, c, t_lo, t_hi, tid, nt); } WT_END
                WT_SYNC;
                if (MULTI) {
                    WT_DO(t_lo, t_hi) { wt_phase_eval_chunk<OP, ValT, ScrT, K>(P, c, WT_R(A), 0, t_lo, t_hi, true, tid, nt); } WT_END
                    WT_SYNC;
                }
            }
            if (MULTI && npass == 2) WT_DO() { wt_eval_mid<OP, K>(P, WT_R(A)); } WT_END
            WT_DO() { wt_phase_emask(P, c, OP == WT_OP_TTEST, tid, nt); } WT_END
            WT_SYNC;
            WT_DO() { wt_phase_escan(P, c, tid, nt); } WT_END
            WT_SYNC;
            WT_DO(goff) {
                const long long n_emit = (long long) c.epfx[P.n_words];
                if (tid == 0) { c.sh->n_emit = (int32_t) n_emit; c.sh->goffset = goff; }
            } WT_END
#pragma unroll
            for (int pass = MULTI ? 1 : 0; pass < npass; pass++) {
                for (int cc = 0; cc < n_chunks; cc++) {
                    const int t_lo = cc * NC, t_hi = (t_lo + NC < N) ? t_lo + NC : N;
                    if (MULTI) {
                        WT_DO() { wt_phase_zero(P, c, false, tid, nt); } WT_END
                        WT_SYNC;
                        WT_DO(t_lo, t_hi) { wt_phase_load<ValT>(P, c, t_lo, t_hi, false, tid, nt); } WT_END
                        WT_SYNC;
                        WT_DO(t_lo, t_hi) { wt_phase_count_a(P, c, t_lo, t_hi, tid, nt); } WT_END
                        WT_SYNC;
                        WT_DO(t_lo, t_hi) { wt_phase_count_b(P, c, t_lo, t_hi, tid, nt); } WT_END
                        WT_SYNC;
                    }
                    WT_DO(pass, t_lo, t_hi) { wt_phase_eval_chunk<OP, ValT, ScrT, K>(P, c, WT_R(A), pass, t_lo, t_hi, false, tid, nt); } WT_END
                    if (MULTI) WT_SYNC;
                }
                if (pass == 0 && npass == 2) WT_DO() { wt_eval_mid<OP, K>(P, WT_R(A)); } WT_END
            }
            WT_DO() { wt_phase_eval_finish<OP, ValT, ScrT, K>(P, c, WT_R(A), WT_R(L), tid, nt); } WT_END
            WT_SYNC;
            WT_DO() { wt_phase_write<OP, ValT, K>(P, c, WT_R(L), tid, nt); } WT_END
        }
    }
    WT_KERNEL_END;
}

#endif  // WT_PATCH_KERNEL_H_
