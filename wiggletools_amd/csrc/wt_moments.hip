// wt_moments.hip -- the integrators: genome-wide statistics of a device run list, each behind an asynchronous entry
// (wt_host.h) that the bulk doors (wt_engine.hip) and the streaming pipeline (wt_pipe.hip) launch with their own block
// counts.  Further down: wt_auc_kernel (AUC, meanI) and wt_pearson_kernel (Pearson of a 2-track Multiplexer tile).  First
// the statistics that need more than a sum, in ONE pass:
// varI / stddevI / CVI, maxI / minI and the span (reference src/statistics.c:129-326).  One launch yields
//
//     { sum = S L v,  span = S L,  T = S L (v - sum/span)^2,  min,  max,  spare }      L = finish - start,
//
// over the runs whose value is not NaN; min and max are NaN when there is none.  T is the reference's
// VarianceData.T (statistics.c:232-252), which it updates run by run with a weighted Welford step; here
//
//   * consecutive lanes take consecutive runs (two per lane and load where the arrays are aligned for it), so a
//     wavefront reads whole cache lines -- the kernel streams 16 bytes per run and does no division per run:
//     a lane accumulates S L, S L (v - k), S L (v - k)^2 about a pivot k of its own (its first value, so that the
//     one subtraction T = S2 - S1^2 / S0 per lane cancels next to nothing), then restates its sum about the
//     LAUNCH's pivot K (the first value of the list's first 256 runs: every block reads the same one);
//   * partials {n, d = S L (v - K), T} are merged with the pairwise (Chan) form of the reference's step, in a fixed
//     order: across the wavefront with shuffles, across the block's wavefronts through LDS, across blocks in a
//     one-block kernel.  All of it about K: the term (mean_b - mean_a)^2 n_a n_b / n then loses digits with
//     ((mean - K) / deviation)^2 instead of (mean / deviation)^2.  No atomics: a run list always gives the same bits;
//   * min / max carry the index of the run that set them and the merge keeps the EARLIER run of two that compare
//     equal: the reference keeps the first run that reaches the extreme (statistics.c:176,206, strict > / <), which
//     decides the sign of a zero result.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "wt_host.h"
#include "wt_devscope.h"
#include "wt_moments_merge.h"      // WmAcc, wm_merge, WmLane, wm_add, wm_lane_acc: shared with csrc/wt_apply.h

namespace {

#define WM_BLOCK 256
#ifndef WM_MAX_BLOCKS
#define WM_MAX_BLOCKS 2048          // of the bulk door: 8 blocks per CU (the pipeline launches WT_INTEG_BLOCKS per batch)
#endif

struct WmPartial {          // 64 bytes
    double n, d, T, mn, mx;
    long long imn, imx;     // index of the run that set mn / mx, WM_NONE: unset
    double K;               // the launch's pivot (written by block 0)
};

__device__ __forceinline__ long long wm_shfl_down(long long x, int s) {
    const int lo = __shfl_down((int) (x & 0xffffffffll), s), hi = __shfl_down((int) (x >> 32), s);
    return ((long long) hi << 32) | (unsigned int) lo;
}

// lane 0 ends up with the wavefront's aggregate (lanes merged pairwise, lower lane first)
__device__ __forceinline__ void wm_wave_reduce(WmAcc &a) {
    for (int s = 1; s < 64; s <<= 1) {
        WmAcc b;
        b.n = __shfl_down(a.n, s); b.d = __shfl_down(a.d, s); b.T = __shfl_down(a.T, s);
        b.mn = __shfl_down(a.mn, s); b.mx = __shfl_down(a.mx, s);
        b.imn = wm_shfl_down(a.imn, s); b.imx = wm_shfl_down(a.imx, s);
        wm_merge(a, b);                     // (lanes whose partner lies past the wavefront read their own value back and are
    }                                       //  never read again: lane 0's tree only has partners inside the wavefront)
}

__global__ void __launch_bounds__(WM_BLOCK) wt_moments_kernel(const int32_t *__restrict__ start, const int32_t *__restrict__ finish,
                                                              const double *__restrict__ value, long long n,
                                                              const unsigned long long *n_dev, WmPartial *partial) {
    __shared__ int first[WM_BLOCK / 64];
    __shared__ WmAcc red[WM_BLOCK / 64];
    if (n_dev && (long long) *n_dev < n) n = (long long) *n_dev;       // (pipeline: the run count only exists on the device)
    const int t = threadIdx.x, w = t >> 6;

    // the launch's pivot: the first value among the list's first 256 runs (0 when they are all NaN)
    const double v0 = t < n ? value[t] : __builtin_nan("");
    const unsigned long long m = __ballot(v0 == v0);
    if ((t & 63) == 0) first[w] = m ? w * 64 + __ffsll((long long) m) - 1 : -1;
    __syncthreads();
    int fi0 = -1;
    for (int k = WM_BLOCK / 64 - 1; k >= 0; k--) if (first[k] >= 0) fi0 = first[k];
    const double K = fi0 >= 0 ? value[fi0] : 0.0;

    WmLane a = {0, 0, 0, 0, 0, 0, WM_NONE, WM_NONE, false};
    const long long lanes = (long long) gridDim.x * WM_BLOCK, me = (long long) blockIdx.x * WM_BLOCK + t;
    const bool wide = ((((uintptr_t) start | (uintptr_t) finish) & 7) | ((uintptr_t) value & 15)) == 0;
    long long done = 0;
    if (wide) {                             // two runs per lane and load: int2 / int2 / double2
        const long long pairs = n >> 1;
        const int2 *s2 = (const int2 *) start, *f2 = (const int2 *) finish;
        const double2 *v2 = (const double2 *) value;
#pragma unroll 2
        for (long long q = me; q < pairs; q += lanes) {
            const int2 s = s2[q], f = f2[q];
            const double2 v = v2[q];
            wm_add(a, 2 * q, s.x, f.x, v.x);
            wm_add(a, 2 * q + 1, s.y, f.y, v.y);
        }
        done = pairs << 1;
    }
    for (long long r = done + me; r < n; r += lanes) wm_add(a, r, start[r], finish[r], value[r]);

    WmAcc c = wm_lane_acc(a, K);
    wm_wave_reduce(c);
    if ((t & 63) == 0) red[w] = c;
    __syncthreads();
    if (t == 0) {
        for (int k = 1; k < WM_BLOCK / 64; k++) wm_merge(c, red[k]);
        WmPartial p;
        p.n = c.n; p.d = c.d; p.T = c.T; p.mn = c.mn; p.mx = c.mx; p.imn = c.imn; p.imx = c.imx; p.K = K;
        partial[blockIdx.x] = p;
    }
}

// one block: lane l merges its contiguous share of the block partials in order, then lanes and wavefronts as above
__global__ void __launch_bounds__(WM_BLOCK) wt_moments_final_kernel(const WmPartial *partial, int n_blocks, double *out6) {
    __shared__ WmAcc red[WM_BLOCK / 64];
    const int l = threadIdx.x, per = (n_blocks + WM_BLOCK - 1) / WM_BLOCK;
    WmAcc c = {0, 0, 0, 0, 0, WM_NONE, WM_NONE};
    for (int i = l * per; i < (l + 1) * per && i < n_blocks; i++) {
        const WmPartial p = partial[i];
        WmAcc b = {p.n, p.d, p.T, p.mn, p.mx, p.imn, p.imx};
        wm_merge(c, b);
    }
    wm_wave_reduce(c);
    if ((l & 63) == 0) red[l >> 6] = c;
    __syncthreads();
    if (l == 0) {
        for (int k = 1; k < WM_BLOCK / 64; k++) wm_merge(c, red[k]);
        const double K = partial[0].K;
        out6[0] = c.n > 0 ? K * c.n + c.d : 0.0;
        out6[1] = c.n;
        out6[2] = c.T;
        out6[3] = c.imn != WM_NONE ? c.mn : __builtin_nan("");
        out6[4] = c.imx != WM_NONE ? c.mx : __builtin_nan("");
        out6[5] = 0.0;
    }
}

}  // namespace

// AUC: statistics.c:103-120.  Deterministic two-level sum.
__global__ void __launch_bounds__(256) wt_auc_kernel(const int32_t *start, const int32_t *finish, const double *value,
                                                      long long n, double *partial, double *partial_span,
                                                      const unsigned long long *n_dev = nullptr) {
    __shared__ double red[256];
    double acc = 0, span = 0;
    if (n_dev && (long long) *n_dev < n) n = (long long) *n_dev;       // (pipeline: the run count only exists on the device)
    const long long stride = (long long) gridDim.x * blockDim.x;
    for (long long r = (long long) blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
        const double v = value[r];
        if (v == v) {                                   // NaN runs are skipped (statistics.c:78, 110)
            const double len = (double) (finish[r] - start[r]);
            acc += len * v;
            span += len;
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int) threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
    if (partial_span) {                                 // MeanIntegrator also needs the non-NaN span
        __syncthreads();
        red[threadIdx.x] = span;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if ((int) threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
            __syncthreads();
        }
        if (threadIdx.x == 0) partial_span[blockIdx.x] = red[0];
    }
}

__global__ void wt_auc_final_kernel(const double *partial, int n, double *out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double acc = 0;
        for (int i = 0; i < n; i++) acc += partial[i];
        *out = acc;
    }
}

// ---------------------------------------------------------------------------
// Pearson correlation of two tracks over the Multiplexer tile (reference PearsonIntegrator,
// statistics.c:414-465).  The reference updates {count, sum, T_XX, T_XY, T_YY} run by run with the
// weighted Welford / Chan step (its `new_mean` is old sum / new count; expanding
// n*L/(n+L) * (X - mean)^2 gives exactly its expression).  Here every lane applies that step IN ITS
// UNEXPANDED FORM, n*L/(n+L) * (X - mean)^2, to a contiguous slice of runs, and slices are merged
// pairwise in genome order with the same formula for two aggregates -- mathematically identical.
// The expanded form sums terms of size mean^2 to get one of size deviation^2; in the reference's one long
// pass that costs (mean/deviation)^2 of the digits with errors of either sign, but at the start of
// every slice -- 65 536 of them, n / (n + L) far from 1 -- the errors are biased: on a track of
// relative variance 1e-10 (70 001 runs) T_XX came out 2.1e-8 off where the reference's own pass is
// 4.9e-10 off; unexpanded it is 2.9e-13 off (tests/test_side_kernels.py::test_gpu_pearson_constant_track_rule,
// against exact rational arithmetic; the other tests hold 1e-9 against the oracle).
// ---------------------------------------------------------------------------
struct WtMoments {
    double n, sx, sy, txx, txy, tyy;
};

__device__ inline void wt_moments_add_run(WtMoments &m, double X, double Y, double L) {
    if (m.n > 0) {
        const double dx = X - m.sx / m.n, dy = Y - m.sy / m.n;
        const double w = m.n * L / (m.n + L);
        m.txx += dx * dx * w;
        m.txy += dx * dy * w;
        m.tyy += dy * dy * w;
    }
    m.n += L;
    m.sx += X * L;
    m.sy += Y * L;
}

// a := a (+) b, b following a in genome order
__device__ inline void wt_moments_merge(WtMoments &a, const WtMoments &b) {
    if (b.n == 0) return;
    if (a.n == 0) { a = b; return; }
    const double n = a.n + b.n;
    const double dx = b.sx / b.n - a.sx / a.n, dy = b.sy / b.n - a.sy / a.n;
    const double w = a.n * b.n / n;
    a.txx += b.txx + dx * dx * w;
    a.txy += b.txy + dx * dy * w;
    a.tyy += b.tyy + dy * dy * w;
    a.n = n;
    a.sx += b.sx;
    a.sy += b.sy;
}

__global__ void __launch_bounds__(256) wt_pearson_kernel(const int32_t *start, const int32_t *finish, const double *tile,
                                                          const uint8_t *inplay, double dx, double dy, long long n,
                                                          WtMoments *partial, const unsigned long long *n_dev = nullptr) {
    __shared__ WtMoments red[256];
    if (n_dev && (long long) *n_dev < n) n = (long long) *n_dev;
    const long long total_lanes = (long long) gridDim.x * blockDim.x;
    const long long per = (n + total_lanes - 1) / total_lanes;          // contiguous slice per lane
    const long long lane_id = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    long long lo = lane_id * per, hi = lo + per;
    if (hi > n) hi = n;
    WtMoments m = {0, 0, 0, 0, 0, 0};
    for (long long r = lo; r < hi; r++) {
        const double X = inplay[2 * r] ? tile[2 * r] : dx;
        const double Y = inplay[2 * r + 1] ? tile[2 * r + 1] : dy;
        wt_moments_add_run(m, X, Y, (double) (finish[r] - start[r]));
    }
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = 1; s < 256; s <<= 1) {                                 // ordered pairwise merge
        if ((threadIdx.x & (2 * s - 1)) == 0) wt_moments_merge(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

__global__ void wt_pearson_final_kernel(const WtMoments *partial, int n, double *out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        WtMoments m = {0, 0, 0, 0, 0, 0};
        for (int i = 0; i < n; i++) wt_moments_merge(m, partial[i]);
        double txx = m.txx, tyy = m.tyy;                               // (constant track: see wtamd_pearson_finish)
        if (m.n > 0) {
            const double mx = m.sx / m.n, my = m.sy / m.n;
            if (txx <= m.n * mx * mx * 1e-14) txx = 0;
            if (tyy <= m.n * my * my * 1e-14) tyy = 0;
        }
        const double den = txx * tyy;
        out[0] = den ? m.txy / sqrt(den) : __builtin_nan("");          // statistics.c:421-423
        out[1] = m.n; out[2] = m.sx; out[3] = m.sy; out[4] = m.txx; out[5] = m.txy; out[6] = m.tyy;
    }
}

size_t wt_auc_partial_bytes(int blocks) { return sizeof(double) * 2 * (size_t) blocks; }

int wt_auc_async(const int32_t *start, const int32_t *finish, const double *value, long long n, const unsigned long long *n_dev,
                 int blocks, void *d_partial, double *d_out, bool with_span, hipStream_t st) {
    double *part = (double *) d_partial;
    hipLaunchKernelGGL(wt_auc_kernel, dim3(blocks), dim3(256), 0, st, start, finish, value, n, part, with_span ? part + blocks : nullptr, n_dev);
    hipLaunchKernelGGL(wt_auc_final_kernel, dim3(1), dim3(64), 0, st, part, blocks, d_out);
    if (with_span) hipLaunchKernelGGL(wt_auc_final_kernel, dim3(1), dim3(64), 0, st, part + blocks, blocks, d_out + 1);
    WT_HIP(hipGetLastError());
    return WTAMD_OK;
}

size_t wt_pearson_partial_bytes(int blocks) { return sizeof(WtMoments) * (size_t) blocks; }

int wt_pearson_async(const int32_t *start, const int32_t *finish, const double *tile, const uint8_t *inplay, double dx, double dy, long long n,
                     const unsigned long long *n_dev, int blocks, void *d_partial, double *d_out7, hipStream_t st) {
    hipLaunchKernelGGL(wt_pearson_kernel, dim3(blocks), dim3(256), 0, st, start, finish, tile, inplay, dx, dy, n, (WtMoments *) d_partial, n_dev);
    hipLaunchKernelGGL(wt_pearson_final_kernel, dim3(1), dim3(64), 0, st, (const WtMoments *) d_partial, blocks, d_out7);
    WT_HIP(hipGetLastError());
    return WTAMD_OK;
}

// Moments of the run list -> d_out6 (device), on `st`.  d_partial: wt_moments_partial_bytes(blocks) bytes of device memory.
size_t wt_moments_partial_bytes(int blocks) { return sizeof(WmPartial) * (size_t) blocks; }

int wt_moments_async(const int32_t *start, const int32_t *finish, const double *value, long long cap, const unsigned long long *n_dev,
                     int blocks, void *d_partial, double *d_out6, hipStream_t st) {
    hipLaunchKernelGGL(wt_moments_kernel, dim3((unsigned) blocks), dim3(WM_BLOCK), 0, st, start, finish, value, cap, n_dev,
                       (WmPartial *) d_partial);
    hipLaunchKernelGGL(wt_moments_final_kernel, dim3(1), dim3(WM_BLOCK), 0, st, (const WmPartial *) d_partial, blocks, d_out6);
    return hipGetLastError() == hipSuccess ? WTAMD_OK : wt_fail(WTAMD_ERR_HIP, "moments kernel launch failed");
}

extern "C" int wtamd_runs_moments(const wtamd_runs *runs, int64_t n_runs, double *moments6, void *stream) {
    if (!runs || !moments6 || n_runs < 0) return wt_fail(WTAMD_ERR_ARG, "wtamd_runs_moments: bad argument");
    hipStream_t st = (hipStream_t) stream;
    // enough lanes to keep every CU's loads in flight, few enough that the ordered tail stays short
    long long want = (n_runs + 2 * WM_BLOCK * 4 - 1) / (2 * WM_BLOCK * 4);
    const int blocks = (int) (want < 1 ? 1 : want > WM_MAX_BLOCKS ? WM_MAX_BLOCKS : want);
    char *d = nullptr;
    WtDevScope scope;
    if (scope.alloc(&d, wt_moments_partial_bytes(blocks) + sizeof(double) * 6) != hipSuccess)
        return wt_fail(WTAMD_ERR_HIP, "wtamd_runs_moments: out of device memory");
    double *d_out = (double *) (d + wt_moments_partial_bytes(blocks));
    const int rc = wt_moments_async(runs->start, runs->finish, runs->value, (long long) n_runs, nullptr, blocks, d, d_out, st);
    if (rc != WTAMD_OK) return rc;
    if (hipMemcpyAsync(moments6, d_out, sizeof(double) * 6, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return wt_fail(WTAMD_ERR_HIP, "wtamd_runs_moments: copy failed");
    return WTAMD_OK;
}
