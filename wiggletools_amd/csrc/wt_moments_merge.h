// wt_moments_merge.h -- the pivoted run moments and their ordered pairwise merge, shared by the genome-wide integrator
// (csrc/wt_moments.hip) and the per-region statistics (csrc/wt_apply.h).  Compiled by hipcc for the device and, with
// -DWT_EMU, by g++ for the CPU emulation of the apply passes: the same expressions in the same order, so the same bits
// (both are built with -ffp-contract=off).
//
//   * a lane accumulates S L, S L (v - k), S L (v - k)^2 about a pivot k of its own (its first value, so that the one
//     subtraction T = S2 - S1^2 / S0 per lane cancels next to nothing), then restates its sum about the pivot K its
//     partial is merged under (wm_lane_acc);
//   * partials {n, d = S L (v - K), T} are merged with the pairwise (Chan) form of the reference's weighted Welford step
//     (statistics.c:232-252), all of them about K: the term (mean_b - mean_a)^2 n_a n_b / n then loses digits with
//     ((mean - K) / deviation)^2 instead of (mean / deviation)^2;
//   * min / max carry the index of the run that set them and the merge keeps the EARLIER run of two that compare equal:
//     the reference keeps the first run that reaches the extreme (statistics.c:176,206, strict > / <), which decides the
//     sign of a zero result.
#ifndef WT_MOMENTS_MERGE_H_
#define WT_MOMENTS_MERGE_H_

#ifdef WT_EMU
#define WM_DEV inline
#else
#include <hip/hip_runtime.h>
#define WM_DEV __device__ __forceinline__
#endif

#define WM_NONE 0x7fffffffffffffffll

struct WmAcc {
    double n, d, T, mn, mx;
    long long imn, imx;     // index of the run that set mn / mx, WM_NONE: unset
};

// a := a (+) b, both about the same pivot
WM_DEV void wm_merge(WmAcc &a, const WmAcc &b) {
    if (b.n > 0) {
        if (a.n > 0) {
            const double n = a.n + b.n;
            const double dm = b.d / b.n - a.d / a.n;
            a.T += b.T + dm * dm * (a.n * b.n / n);
            a.d += b.d;
            a.n = n;
        } else {
            a.n = b.n; a.d = b.d; a.T = b.T;
        }
    }
    if (b.imn != WM_NONE && (a.imn == WM_NONE || b.mn < a.mn || (b.mn == a.mn && b.imn < a.imn))) { a.mn = b.mn; a.imn = b.imn; }
    if (b.imx != WM_NONE && (a.imx == WM_NONE || b.mx > a.mx || (b.mx == a.mx && b.imx < a.imx))) { a.mx = b.mx; a.imx = b.imx; }
}

struct WmLane {
    double s0, s1, s2, k, mn, mx;
    long long imn, imx;
    bool have;
};

WM_DEV WmLane wm_lane_zero() {
    WmLane a = {0, 0, 0, 0, 0, 0, WM_NONE, WM_NONE, false};
    return a;
}

WM_DEV void wm_add(WmLane &a, long long r, int st, int fi, double v) {
    if (v == v) {                           // NaN runs are skipped
        if (!a.have) { a.k = v; a.have = true; }
        const double L = (double) (fi - st), e = v - a.k, Le = L * e;
        a.s0 += L;
        a.s1 += Le;
        a.s2 += Le * e;
        if (a.imn == WM_NONE || v < a.mn) { a.mn = v; a.imn = r; }
        if (a.imx == WM_NONE || v > a.mx) { a.mx = v; a.imx = r; }
    }
}

// the lane's sums as a partial about the pivot K
WM_DEV WmAcc wm_lane_acc(const WmLane &a, double K) {
    WmAcc c;
    c.n = a.s0;
    c.T = a.s0 > 0 ? a.s2 - a.s1 * a.s1 / a.s0 : 0.0;
    c.d = a.s1 + (a.k - K) * a.s0;
    c.mn = a.mn; c.mx = a.mx; c.imn = a.imn; c.imx = a.imx;
    return c;
}

#endif  // WT_MOMENTS_MERGE_H_
