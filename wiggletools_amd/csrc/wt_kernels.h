// wt_kernels.h -- what the engine (wt_engine.hip; the pipeline reaches the kernels through it, wt_trackset.h) needs of the
// kernel units: the launch record (the patch kernel's arguments: WtPatchArgs, wt_core.h), the kernels' launch bounds and one launch entry per kernel family.  The kernels are templates in
// wt_reduce_kernel.h / wt_patch_kernel.h / wt_delta_kernel.h / wt_walk_kernel.h (wt_exec.h), instantiated in wt_reduce_stream.hip,
// wt_reduce_moments.hip, wt_reduce_order.hip, wt_patch_kernels.hip, wt_delta_kernels.hip and wt_walk.hip.
#ifndef WT_KERNELS_H_
#define WT_KERNELS_H_

#include <hip/hip_runtime.h>
#include "wt_core.h"

// One launch: filled in by the host; `grid` and `err` are the launch entry's answer
struct WtLaunch {
    WtParams P;
    int T = 0, lds = 0, grid = 0;
    bool small_tiles = false;           // difference-array Sum / Mean: the pass in 128-run tiles (wt_delta_launch)
    hipStream_t stream = nullptr;
    int num_cu = 256;
    char **gscratch = nullptr;
    size_t *gscratch_bytes = nullptr;
    hipError_t err = hipSuccess;
};

// launch bounds of the kernels, as compiled into the units that own them
extern const int wt_reduce_max_block, wt_delta_block, wt_delta_sq_block;

// General kernel: each unit launches its own ops (stream: sum, product, mean, min, max, multiplex; moments: var, stddev /
// entropy, cv, ttest; order: median, mwu and their register-column forms) and returns false for the others
bool wt_reduce_stream_launch(WtLaunch &L, int op, bool value_f64, bool scratch_f32, int ppt, bool multi, int regcol);
bool wt_reduce_moments_launch(WtLaunch &L, int op, bool value_f64, bool scratch_f32, int ppt, bool multi, int regcol);
bool wt_reduce_order_launch(WtLaunch &L, int op, bool value_f64, bool scratch_f32, int ppt, bool multi, int regcol);
static inline bool wt_reduce_launch(WtLaunch &L, int op, bool value_f64, bool scratch_f32, int ppt, bool multi, int regcol) {
    return wt_reduce_stream_launch(L, op, value_f64, scratch_f32, ppt, multi, regcol) || wt_reduce_moments_launch(L, op, value_f64, scratch_f32, ppt, multi, regcol) ||
           wt_reduce_order_launch(L, op, value_f64, scratch_f32, ppt, multi, regcol);
}
// Patch kernel over the n_bad windows of Q (fill_index: wt_patch_index_kernel first); false: no instantiation for (op, ppt)
bool wt_patch_launch(WtLaunch &L, const WtPatchArgs &Q, int op, int ppt, bool multi, long long n_bad, bool fill_index);
// Difference-array kernel of `op` (L.P.delta_df and L.small_tiles select among its forms)
void wt_delta_launch(WtLaunch &L, int op);
// Walking kernels (nr: the register-column slots the bitmap kernel would use for this track count -- eligibility only)
hipError_t wt_walk_launch(WtParams &P, int nr, int T, int lds, int num_cu, char **gscratch, size_t *gscratch_bytes, hipStream_t s, int *grid);
// -DWT_PROFILE builds: wt_prof2 (wt_core.h), read and cleared by the unit whose kernels write it; false: nothing counted
bool wt_prof2_take(unsigned long long (&p2)[8]);

#endif  // WT_KERNELS_H_
