// wt_patch_kernels.hip -- wt_patch_kernel (wt_patch_kernel.h), wt_patch_index_kernel (this unit alone needs it: no header) and
// their launch entry.  Compiled only by hipcc --offload-arch=gfx950.
#include "wt_patch_kernel.h"

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
