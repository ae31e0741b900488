// wt_patch_kernels.hip -- wt_patch_kernel, wt_patch_index_kernel (this unit alone needs them: no header) and their launch
// entry.  Compiled only by hipcc --offload-arch=gfx950.
#include "wt_reduce_kernel.h"

// Patch kernel: the general bitmap multiplexer over just the windows the difference-array kernel
// could not prove exact (a NaN, an Inf, too wide a dynamic range).  That kernel has already emitted
// those windows' runs -- coordinates, run count, position in the output -- so this one only has
// to recompute their values in the reference's own summation order and store them at the recorded
// offsets: no ticket, no look-back, no statistics.  One difference-array window (8192 bp) is
// `ratio` general windows; the difference-array kernel recorded the run offset of 16 sub-ranges of
// every such window, so every (window, sub-window) pair is a work item of its own.

// The narrow-window index rows the patch kernel is going to read, and only those: for every window the
// difference-array kernel recorded, the ratio + 1 boundaries inside it, per track, by binary search.  (Round 3 built the
// WHOLE index at the patch kernel's window width whenever a launch had a window to patch -- 4 x the rows of the
// 8192-bp index, a third of a millisecond per chromosome for a few hundred windows.)
__global__ void __launch_bounds__(256) wt_patch_index_kernel(const WtParams P, const WtPatchArgs Q) {
    const long long n_bad = (long long) *Q.n_bad;
    const int N = P.n_tracks, R1 = Q.ratio + 1;
    const long long total = n_bad * R1 * N;
    for (long long t = (long long) blockIdx.x * 256 + threadIdx.x; t < total; t += (long long) gridDim.x * 256) {
        const long long j = t / ((long long) R1 * N);
        const int rem = (int) (t - j * R1 * N), r = rem / N, i = rem - r * N;
        const long long kd = Q.bad_list[j];
        const int ch = Q.d_win_chrom[kd];
        const long long m = (kd - Q.d_c_first_win[ch]) * Q.ratio + r;
        if (m > P.c_nwin[ch]) continue;             // (row c_nwin is the chromosome's last boundary)
        const long long seg = (long long) ch * N + i;
        const long long s0 = P.seg_off[seg], n = P.seg_off[seg + 1] - s0;
        const long long b = (long long) P.cbase[ch] + (m << P.logW);
        P.widx[(P.c_first_win[ch] + ch + m) * N + i] = (uint32_t) wt_lane_lower_bound(P.finish + s0, 0, n, n >> 1, b);
    }
}

template <int OP, int K, bool MULTI>
__global__ void __launch_bounds__(WT_MAX_BLOCK, WT_MIN_WAVES(K)) wt_patch_kernel(const WtParams P, const WtPatchArgs Q) {
    typedef float ValT;
    typedef float ScrT;
    extern __shared__ __attribute__((aligned(16))) char wt_lds[];
    WtCtx c;
    wt_ctx_init(c, P, wt_lds);
    WtLane<K> L;
    const int tid = threadIdx.x, nt = blockDim.x;
    const long long n_bad = (long long) *Q.n_bad;
    const int N = P.n_tracks, NC = MULTI ? P.chunk_tracks : N, n_chunks = MULTI ? P.n_chunks : 1;
    // work items = (window the difference-array kernel recorded, narrower window h inside it): independent of one
    // another -- the recording kernel left the run offset of every sub-range (wt_delta_note_offset)
    const long long n_items = n_bad * Q.ratio;
    for (long long item = blockIdx.x; item < n_items; item += gridDim.x) {
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
            __syncthreads();                                // the previous window is done with the shared block
            if (tid == 0) wt_phase_header(P, c, k);
            wt_phase_zero(P, c, true, tid, nt);
            __syncthreads();
            // same sweeps as wt_reduce_kernel (chunked tracks: the first evaluation pass rides on the
            // sweep that builds the bitmaps; var / stddev / CV take a second one)
            constexpr int npass = wt_eval_passes(OP);
            WtAcc<K> A;
            wt_eval_init<OP, K>(A);
            for (int cc = 0; cc < n_chunks; cc++) {
                const int t_lo = cc * NC, t_hi = (t_lo + NC < N) ? t_lo + NC : N;
                if (MULTI && cc > 0) {
                    wt_phase_zero(P, c, false, tid, nt);
                    __syncthreads();
                }
                wt_phase_load<ValT>(P, c, t_lo, t_hi, false, tid, nt);
                __syncthreads();
                wt_phase_count_a(P, c, t_lo, t_hi, tid, nt);
                __syncthreads();
                wt_phase_count_b(P, c, t_lo, t_hi, tid, nt);
                __syncthreads();
                if (MULTI) {
                    wt_phase_eval_chunk<OP, ValT, ScrT, K>(P, c, A, 0, t_lo, t_hi, true, tid, nt);
                    __syncthreads();
                }
            }
            if (MULTI && npass == 2) wt_eval_mid<OP, K>(P, A);
            wt_phase_emask(P, c, OP == WT_OP_TTEST, tid, nt);
            __syncthreads();
            wt_phase_escan(P, c, tid, nt);
            __syncthreads();
            const long long n_emit = (long long) c.epfx[P.n_words];
            if (tid == 0) { c.sh->n_emit = (int32_t) n_emit; c.sh->goffset = goff; }
#pragma unroll
            for (int pass = MULTI ? 1 : 0; pass < npass; pass++) {
                for (int cc = 0; cc < n_chunks; cc++) {
                    const int t_lo = cc * NC, t_hi = (t_lo + NC < N) ? t_lo + NC : N;
                    if (MULTI) {
                        wt_phase_zero(P, c, false, tid, nt);
                        __syncthreads();
                        wt_phase_load<ValT>(P, c, t_lo, t_hi, false, tid, nt);
                        __syncthreads();
                        wt_phase_count_a(P, c, t_lo, t_hi, tid, nt);
                        __syncthreads();
                        wt_phase_count_b(P, c, t_lo, t_hi, tid, nt);
                        __syncthreads();
                    }
                    wt_phase_eval_chunk<OP, ValT, ScrT, K>(P, c, A, pass, t_lo, t_hi, false, tid, nt);
                    if (MULTI) __syncthreads();
                }
                if (pass == 0 && npass == 2) wt_eval_mid<OP, K>(P, A);
            }
            wt_phase_eval_finish<OP, ValT, ScrT, K>(P, c, A, L, tid, nt);
            __syncthreads();
            wt_phase_write<OP, ValT, K>(P, c, L, tid, nt);
        }
    }
}

template <int OP, int K>
static void wt_patch_launch_t(WtLaunch &L, const WtPatchArgs &Q, bool multi, long long n_bad) {
    auto kern = multi ? wt_patch_kernel<OP, K, true> : wt_patch_kernel<OP, K, false>;
    int per_cu = 0;
    L.err = wt_blocks_per_cu((const void *) kern, L.T, L.lds, &per_cu);
    if (L.err != hipSuccess) return;
    long long g = (long long) L.num_cu * per_cu;
    if (g > n_bad * Q.ratio) g = n_bad * Q.ratio;
    if (g < 1) g = 1;
    L.grid = (int) g;
    hipLaunchKernelGGL(kern, dim3((unsigned) g), dim3((unsigned) L.T), (size_t) L.lds, L.stream, L.P, Q);
    L.err = hipGetLastError();
}

bool wt_patch_launch(WtLaunch &L, const WtPatchArgs &Q, int op, int ppt, bool multi, long long n_bad, bool fill_index) {
    if (fill_index) {
        long long blocks = (n_bad * (Q.ratio + 1) * L.P.n_tracks + 255) / 256;
        if (blocks > 4ll * L.num_cu) blocks = 4ll * L.num_cu;
        if (blocks < 1) blocks = 1;
        hipLaunchKernelGGL(wt_patch_index_kernel, dim3((unsigned) blocks), dim3(256), 0, L.stream, L.P, Q);
        if ((L.err = hipGetLastError()) != hipSuccess) return true;
    }
    // Sum / Mean exist with 1 and 4 positions per lane, every other op with 4 only (what the plans pick unless forced)
    const bool k4 = ppt == 4;
    if (!k4 && op != WT_OP_SUM && op != WT_OP_MEAN) return false;
    switch (op) {
    case WT_OP_SUM: if (k4) wt_patch_launch_t<WT_OP_SUM, 4>(L, Q, multi, n_bad); else wt_patch_launch_t<WT_OP_SUM, 1>(L, Q, multi, n_bad); break;
    case WT_OP_MEAN: if (k4) wt_patch_launch_t<WT_OP_MEAN, 4>(L, Q, multi, n_bad); else wt_patch_launch_t<WT_OP_MEAN, 1>(L, Q, multi, n_bad); break;
    case WT_OP_MAX: wt_patch_launch_t<WT_OP_MAX, 4>(L, Q, multi, n_bad); break;
    case WT_OP_MIN: wt_patch_launch_t<WT_OP_MIN, 4>(L, Q, multi, n_bad); break;
    case WT_OP_TTEST: wt_patch_launch_t<WT_OP_TTEST, 4>(L, Q, multi, n_bad); break;
    case WT_OP_VAR: wt_patch_launch_t<WT_OP_VAR, 4>(L, Q, multi, n_bad); break;
    case WT_OP_CV: wt_patch_launch_t<WT_OP_CV, 4>(L, Q, multi, n_bad); break;
    default: wt_patch_launch_t<WT_OP_STDDEV, 4>(L, Q, multi, n_bad); break;      // stddev, entropy (reducers.c:665)
    }
    return true;
}
