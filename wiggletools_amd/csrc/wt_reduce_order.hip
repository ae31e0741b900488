// wt_reduce_order.hip -- wt_reduce_kernel (wt_reduce_kernel.h) for the order statistics (median, Mann-Whitney U), register-column forms included.
#include "wt_reduce_kernel.h"

#ifdef WT_PROFILE
bool wt_prof2_take(unsigned long long (&p2)[8]) {
    const unsigned long long z[8] = {0};
    if (hipMemcpyFromSymbol(p2, HIP_SYMBOL(wt_prof2), sizeof p2) != hipSuccess || !(p2[0] | p2[4])) return false;
    return (void) hipMemcpyToSymbol(HIP_SYMBOL(wt_prof2), z, sizeof z), true;
}
#endif

bool wt_reduce_order_launch(WtLaunch &L, int op, bool value_f64, bool scratch_f32, int ppt, bool multi, int regcol) {
    WtReduceRun f{L};
    return wt_dispatch_ops<WT_OP_MEDIAN, WT_OP_MWU>(op, value_f64, scratch_f32, ppt, multi, f, regcol);
}
