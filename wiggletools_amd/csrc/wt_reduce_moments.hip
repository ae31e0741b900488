// wt_reduce_moments.hip -- wt_reduce_kernel (wt_reduce_kernel.h) for the moment reducers (var, stddev / entropy, cv, t-test).
#include "wt_reduce_kernel.h"

bool wt_reduce_moments_launch(WtLaunch &L, int op, bool value_f64, bool scratch_f32, int ppt, bool multi, int regcol) {
    WtReduceRun f{L};
    return wt_dispatch_ops<WT_OP_VAR, WT_OP_STDDEV, WT_OP_CV, WT_OP_TTEST>(op, value_f64, scratch_f32, ppt, multi, f, regcol);
}
