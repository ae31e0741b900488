// wt_walk.hip -- gfx950 kernels of MedianReduction / MWUReduction by walking (wt_walk_kernel.h; logic in wt_walk.h, wt_mwalk.h)
// and their launcher (wt_kernels.h), one of the kernel units next to wt_engine.hip.  Compiled only by hipcc --offload-arch=gfx950.
#include <hip/hip_runtime.h>
#include <cstdio>

#include "../../include/wiggletools_amd.h"
#include "wt_core.h"
#include "wt_kernels.h"
#include "wt_launch.h"
#include "wt_walk_kernel.h"

hipError_t wt_walk_launch(WtParams &P, int nr, int T, int lds, int num_cu, char **gscratch, size_t *gscratch_bytes, hipStream_t s, int *grid) {
    (void) nr;
    auto kern = P.walk_mwu ? wt_mwalk_kernel<256> : (P.walk_pair ? (T > 256 ? wt_walk_kernel<512, true> : wt_walk_kernel<256, true>) : wt_walk_kernel<256, false>);
    int per_cu = 0;
    hipError_t e = wt_blocks_per_cu((const void *) kern, T, lds, &per_cu);
    if (e != hipSuccess) return e;
    long long g = (long long) num_cu * per_cu;
    if (g > P.n_windows) g = P.n_windows;
    if (g < 1) g = 1;
    e = wt_reserve_slab(gscratch, gscratch_bytes, (size_t) g * (size_t) P.g_scratch_slab);     // one slab of events per resident workgroup
    if (e != hipSuccess) return e;
    P.g_scratch = *gscratch;
    *grid = (int) g;
    hipLaunchKernelGGL(kern, dim3((unsigned) g), dim3((unsigned) T), (size_t) lds, s, P);
    return hipGetLastError();
}
