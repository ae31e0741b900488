// wt_delta_kernels.hip -- wt_delta_kernel (wt_delta_kernel.h) for every op it has, and its launch entry.
#include "wt_delta_kernel.h"

const int wt_delta_block = WT_DELTA_BLOCK, wt_delta_sq_block = WT_DELTA_SQ_BLOCK;

template <int OP, bool DF = false>
static void wt_delta_launch_t(WtLaunch &L) {
    // 128-run tiles when a window holds fewer than 8 of the 256-run ones per wavefront (round 6: the last round of tiles
    // leaves wavefronts idle -- mean run 64: 50 tiles over 16 wavefronts, -6.5 % with the small ones; mean run 200 -2.5 %; mean run 16,
    // 12.5 per wavefront: +1 %, so the large ones stay there).  WTAMD_DELTA_U=2 / 4 forces one.
    // (the t-test's 2048-bp windows: 50 tiles over 12 wavefronts, -6 % with the small ones; the variance family measured +-0 at mean run 16
    //  and +2.5 % at 200 with them and keeps the large ones; Max / Min have a pass of their own, wt_delta_pass_mm)
    constexpr bool TWO = OP == WT_OP_SUM || OP == WT_OP_MEAN || OP == WT_OP_TTEST;
    auto kern = (TWO && L.small_tiles) ? wt_delta_kernel<OP, DF, TWO ? 2 : WT_DELTA_U> : wt_delta_kernel<OP, DF, WT_DELTA_U>;
    int per_cu = 0;
    L.err = wt_blocks_per_cu((const void *) kern, L.T, L.lds, &per_cu);
    if (L.err != hipSuccess) return;
    long long g = (long long) L.num_cu * per_cu;
    if (g > L.P.n_windows) g = L.P.n_windows;
    if (g < 1) g = 1;
    L.grid = (int) g;
    hipLaunchKernelGGL(kern, dim3((unsigned) L.grid), dim3((unsigned) L.T), (size_t) L.lds, L.stream, L.P);
    L.err = hipGetLastError();
}

void wt_delta_launch(WtLaunch &L, int op) {
    switch (op) {
    case WT_OP_SUM: if (L.P.delta_df) wt_delta_launch_t<WT_OP_SUM, true>(L); else wt_delta_launch_t<WT_OP_SUM>(L); break;
    case WT_OP_MEAN: if (L.P.delta_df) wt_delta_launch_t<WT_OP_MEAN, true>(L); else wt_delta_launch_t<WT_OP_MEAN>(L); break;
    case WT_OP_VAR: wt_delta_launch_t<WT_OP_VAR>(L); break;
    case WT_OP_CV: wt_delta_launch_t<WT_OP_CV>(L); break;
    case WT_OP_TTEST: wt_delta_launch_t<WT_OP_TTEST>(L); break;
    case WT_OP_MAX: wt_delta_launch_t<WT_OP_MAX>(L); break;
    case WT_OP_MIN: wt_delta_launch_t<WT_OP_MIN>(L); break;
    default: wt_delta_launch_t<WT_OP_STDDEV>(L); break;      // stddev, entropy (reducers.c:665)
    }
}
