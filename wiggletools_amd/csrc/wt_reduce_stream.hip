// wt_reduce_stream.hip -- wt_reduce_kernel (wt_reduce_kernel.h) for the streaming reducers (sum, product, mean, min, max) and the Multiplexer tile.
#include "wt_reduce_kernel.h"

const int wt_reduce_max_block = WT_MAX_BLOCK;

bool wt_reduce_stream_launch(WtLaunch &L, int op, bool value_f64, bool scratch_f32, int ppt, bool multi, int regcol) {
    WtReduceRun f{L};
    return wt_dispatch_ops<WT_OP_SUM, WT_OP_PRODUCT, WT_OP_MEAN, WT_OP_MIN, WT_OP_MAX, WT_OP_MULTIPLEX>(op, value_f64, scratch_f32, ppt, multi, f, regcol);
}
