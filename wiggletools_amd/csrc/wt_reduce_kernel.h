// wt_reduce_kernel.h -- wt_reduce_kernel as a template (logic in wt_core.h): persistent workgroups, one alignment window per
// ticket: bitmap multiplexer + per-run reducer + ordered output -- every reducer, any track count.  wt_reduce_stream.hip,
// wt_reduce_moments.hip and wt_reduce_order.hip instantiate it for their ops.  One text (wt_exec.h): hipcc compiles it for gfx950,
// tests/emu/wt_emu.cpp runs the same body on the CPU; the launch functor below is the device's alone.  WT_MAX_BLOCK and
// WT_MIN_WAVES also serve wt_patch_kernel.
#ifndef WT_REDUCE_KERNEL_H_
#define WT_REDUCE_KERNEL_H_

#ifndef WT_EMU
#include "../../include/wiggletools_amd.h"
#include "wt_plan.h"
#include "wt_kernels.h"
#include "wt_launch.h"
#endif
#include "wt_exec.h"

#define WT_MAX_BLOCK 512
// minimum waves per SIMD the register allocator must leave room for (MI355X_MICROARCH:
// w = k*T/256).  Measured on MI355X: the K=4 kernels sit at 129 VGPRs unconstrained -- one
// register over the limit for two 512-lane workgroups per CU -- so they are held to 128
// (w = 4: 2.35 vs 3.14 ms on the bench kernel); the K=1 kernels fit anyway and schedule
// better unconstrained (var/500 tracks: 71 vs 93 ms).
#ifndef WT_MIN_WAVES
#define WT_MIN_WAVES(K) ((K) == 4 ? 4 : 3)
#endif

template <int OP, class ValT, class ScrT, int K, bool MULTI, int NR>
// (register columns, NR > 0: 256 lanes; the column + the exchange network's temporaries need more
//  than the 168 VGPRs three waves per SIMD leave -- with that bound the compiler spilled 250
//  registers into the middle of the network -- so NR = 128 runs two waves per SIMD, NR = 64 three)
WT_KERNEL(wt_reduce_kernel, (NR > 0 ? 256 : WT_MAX_BLOCK, NR > 0 ? (NR > 64 ? 2 : (NR > 32 ? 3 : 4)) : WT_MIN_WAVES(K)), const WtParams P) {
    WT_LDS(wt_lds);
    WtCtx c;
    wt_ctx_init(c, P, wt_lds);
    // global slab of this workgroup: [value columns, if they do not fit LDS][MWU attributes]
    const size_t slab = (size_t) P.g_scratch_slab + (size_t) P.g_attr_slab;
    if (MULTI && (OP == WT_OP_MEDIAN || OP == WT_OP_MWU) && P.g_scratch_slab)
        c.scratch = P.g_scratch + (size_t) WT_WG * slab;
    if (OP == WT_OP_MWU) c.attr = P.g_scratch + (size_t) WT_WG * slab + (size_t) P.g_scratch_slab;
    WT_REG(L, WtLane<K>);
    WT_THREAD_IDS;
    WT_PROF_BEGIN;
    long long k_dbg = -1;
    (void) k_dbg;
    // Window tickets.  The lane-0 work at the end of one iteration (statistics) and at the start of
    // the next (ticket) must NOT be left adjacent across the loop back-edge: hipcc (ROCm 7.2) merges
    // the two `tid == 0` regions into a divergent exit of an inner loop, whose header -- including
    // its s_barrier -- the other 63 lanes of wave 0 then re-enter before lane 0 has fetched the next
    // ticket: every wave re-reads the stale ticket and the workgroup never terminates (observed on
    // MI355X; any instruction between the two regions hides it).  So the next ticket is taken in the
    // same lane-0 block as the statistics, followed by the barrier that publishes it.
    WT_DO() { if (tid == 0) c.sh->ticket = (long long) wt_glb_add64(&P.counters[WT_CTR_TICKET], 1ull); } WT_END
    if (NR > 0)
        WT_DO() { for (int i = tid; i < P.n_tracks; i += nt) c.dflt32[i] = (float) P.defaults[i]; } WT_END
    WT_SYNC;
    for (;;) {
        WT_MARK(1);
        const long long k = c.sh->ticket;
        k_dbg = k;
        WT_MARK(2);
        if (k >= P.n_windows) break;
        WT_DO(k) { if (tid == 0) wt_phase_header(P, c, k); } WT_END
        WT_DO() { wt_phase_zero(P, c, true, tid, nt); } WT_END
        WT_SYNC;
        WT_TICK(0);
        // pass A: every track's breakpoints and coverage enter U / cover[]; with one chunk the
        // per-track bitmaps stay resident for the evaluation
        const int N = P.n_tracks, NC = MULTI ? P.chunk_tracks : N, n_chunks = MULTI ? P.n_chunks : 1;
        // Chunked tracks: every sweep over the chunks rebuilds their bitmaps, so the first
        // evaluation pass is fused into the sweep that builds U / the coverage summaries (one
        // sweep saved: sum-like ops 2 -> 1, var / stddev / CV 3 -> 2).  Not for the Multiplexer
        // tile, whose rows need the look-back offset first.
        constexpr bool FUSE = MULTI && OP != WT_OP_MULTIPLEX;
        constexpr int npass = wt_eval_passes(OP);
        WT_REG(A, WtAcc<K, NR>);
        WT_DO() { wt_eval_init<OP, K>(WT_R(A)); } WT_END
        for (int ch = 0; ch < n_chunks; ch++) {
            const int t_lo = ch * NC, t_hi = (t_lo + NC < N) ? t_lo + NC : N;
            if (MULTI && ch > 0) {
                WT_DO() { wt_phase_zero(P, c, false, tid, nt); } WT_END
                WT_SYNC;
            }
            WT_MARK(3);
            WT_DO(t_lo, t_hi) { wt_phase_load<ValT>(P, c, t_lo, t_hi, true, tid, nt); } WT_END
            WT_SYNC;
            WT_TICK(1);
            WT_MARK(4);
            WT_DO(t_lo, t_hi) { wt_phase_count_a(P, c, t_lo, t_hi, tid, nt); } WT_END
            WT_SYNC;
            WT_MARK(5);
            WT_DO(t_lo, t_hi) { wt_phase_count_b(P, c, t_lo, t_hi, tid, nt); } WT_END
            WT_SYNC;
            WT_TICK(2);
            if (FUSE) {     // first evaluation pass rides on this sweep (every position: E is not known yet)
                WT_DO(t_lo, t_hi) { wt_phase_eval_chunk<OP, ValT, ScrT, K>(P, c, WT_R(A), 0, t_lo, t_hi, true, tid, nt); } WT_END
                WT_SYNC;
                WT_TICK(4);
            }
        }
        if (FUSE && npass == 2) WT_DO() { wt_eval_mid<OP, K>(P, WT_R(A)); } WT_END
        WT_MARK(6);
        WT_DO() { wt_phase_emask(P, c, OP == WT_OP_TTEST || OP == WT_OP_MWU, tid, nt); } WT_END
        WT_SYNC;
        WT_MARK(7);
        WT_DO() { wt_phase_escan(P, c, tid, nt); } WT_END
        WT_SYNC;
        WT_TICK(3);
        // the window's run count is known before the reducers run: publish it now, so that no
        // successor ever waits for our evaluation
        WT_MARK(8);
        WT_DO(k) { if (tid == 0) wt_lookback_publish(P, c, k); } WT_END
        if (OP == WT_OP_MULTIPLEX) {     // the tile rows are written by the evaluation: offset first
            WT_DO(k) { if (tid < 64) wt_lookback_complete(P, c, k, tid); } WT_END
            WT_SYNC;
        }
        WT_MARK(9);
#pragma unroll
        for (int pass = FUSE ? 1 : 0; pass < npass; pass++) {
            for (int ch = 0; ch < n_chunks; ch++) {
                const int t_lo = ch * NC, t_hi = (t_lo + NC < N) ? t_lo + NC : N;
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
                if (MULTI) WT_SYNC;     // the next chunk overwrites the bitmaps
            }
            if (pass == 0 && npass == 2) WT_DO() { wt_eval_mid<OP, K>(P, WT_R(A)); } WT_END
        }
        WT_DO() { wt_phase_eval_finish<OP, ValT, ScrT, K>(P, c, WT_R(A), WT_R(L), tid, nt); } WT_END
        if (OP == WT_OP_MWU && NR == 0) {      // the value columns are complete: rank with every lane, then the tie scan
            WT_SYNC;
            WT_DO() { wt_phase_mwu_rank<ScrT>(P, c, tid, nt); } WT_END
            WT_SYNC;
            WT_DO() { wt_phase_mwu_tail<K>(P, c, WT_R(A), WT_R(L), tid, nt); } WT_END
        }
        WT_TICK(4);
        WT_MARK(10);
        WT_DO(k) { if (OP != WT_OP_MULTIPLEX && tid < 64) wt_lookback_complete(P, c, k, tid); } WT_END
        WT_SYNC;
        WT_TICK(5);
        WT_MARK(11);
        WT_DO() { wt_phase_write<OP, ValT, K>(P, c, WT_R(L), tid, nt); } WT_END
        WT_SYNC;
        WT_MARK(12);
        WT_DO() {
            if (tid == 0) {
                wt_window_stats(P, c);
                c.sh->ticket = (long long) wt_glb_add64(&P.counters[WT_CTR_TICKET], 1ull);
            }
        } WT_END
        WT_SYNC;
        WT_TICK(6);
    }
    WT_PROF_END;
    WT_KERNEL_END;
}

#ifndef WT_EMU
// Launch functor of the general kernel for wt_dispatch_ops (wt_plan.h)
struct WtReduceRun {
    WtLaunch &L;
    template <int OP, class ValT, class ScrT, int K, bool MULTI, int NR = 0>
    void run() {
        auto kern = wt_reduce_kernel<OP, ValT, ScrT, K, MULTI, NR>;
        int per_cu = 0;
        L.err = wt_blocks_per_cu((const void *) kern, L.T, L.lds, &per_cu);
        if (L.err != hipSuccess) return;
        long long g = (long long) L.num_cu * per_cu;
        if (g > L.P.n_windows) g = L.P.n_windows;
        if (g < 1) g = 1;
        if (L.P.g_scratch_slab || L.P.g_attr_slab) {    // one global slab per resident workgroup
            if (L.P.g_scratch_slab && g > 2ll * L.num_cu) g = 2ll * L.num_cu;
            L.err = wt_reserve_slab(L.gscratch, L.gscratch_bytes, (size_t) g * (size_t) (L.P.g_scratch_slab + L.P.g_attr_slab));
            if (L.err != hipSuccess) return;
            L.P.g_scratch = *L.gscratch;
        }
        L.grid = (int) g;
        hipLaunchKernelGGL(kern, dim3((unsigned) L.grid), dim3((unsigned) L.T), (size_t) L.lds, L.stream, L.P);
        L.err = hipGetLastError();
    }
};

#endif  // WT_EMU

#endif  // WT_REDUCE_KERNEL_H_
