// wt_isearch.h -- the lane search of the window index (wt_engine.hip wt_index_coarse_kernel / wt_index_search_kernel, the patch
// kernels' index rows): the lower bound of a boundary b in a track's finish[].  Plain C++ wherever WT_DEV is defined the way the
// emulator build defines it (`inline`), so a host program can include it on its own (tests/test_isearch_host.py does).
#ifndef WT_ISEARCH_H_
#define WT_ISEARCH_H_

#include <math.h>
#include <stdint.h>

#ifndef WT_DEV
#if defined(__HIPCC__) && !defined(WT_EMU)
#define WT_DEV __device__ __forceinline__
#else
#define WT_DEV inline
#endif
#endif

// what the searches read finish[] through: a plain array on the device, a counting accessor in the host test
struct WtFinArray {
    const int32_t *p;
    WT_DEV long long operator()(long long x) const { return (long long) p[x]; }
};

// first x in [lo, hi) with fin(x) >= b (hi if none), starting from a guess g in [lo, hi): gallop from the guess, then bisect.
// At most 1 + 2 floor(log2(hi - lo)) reads.
template <class Fin>
WT_DEV long long wt_gallop_lower_bound(Fin fin, long long lo, long long hi, long long g, long long b) {
    if (lo >= hi) return lo;
    if (fin(g) >= b) {
        hi = g;
        for (long long d = 1;; d <<= 1) {
            const long long q = hi - d;
            if (q < lo) break;
            if (fin(q) < b) { lo = q + 1; break; }
            hi = q;
        }
    } else {
        lo = g + 1;
        for (long long d = 1;; d <<= 1) {
            const long long q = lo + d - 1;
            if (q >= hi) break;
            if (fin(q) >= b) { hi = q; break; }
            lo = q + 1;
        }
    }
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (fin(mid) < b) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The same lower bound by interpolation first.  `density` is the bracket's runs per base pair, (B - A) / (b_B - b_A) of the
// two boundaries whose answers A and B bracket this one (0 or less: not known, no interpolation).  Up to WT_ISEARCH_STEPS
// times the guess moves by (b - fin(g)) * density: every probe tightens the bracket [lo, hi) and the new guess is clamped into
// it, so a probe is never repeated and the bracket only shrinks.  The gallop and the bisection above then run from the improved
// guess inside the tightened bracket: they are the guarantee (the exact lower bound on every input, whatever the density says),
// the interpolation only moves the starting point.  At most WT_ISEARCH_STEPS + 1 + 2 floor(log2(hi - lo)) reads.
// The step is float arithmetic, limited to the bracket's length BEFORE it becomes an integer: (b - fin(g)) is below 2^32 in
// magnitude and hi - lo below 2^33, so nothing overflows at coordinates near WTAMD_MAX_COORD; a NaN (inf * 0) leaves the limit.
#define WT_ISEARCH_STEPS 2
template <class Fin>
WT_DEV long long wt_interp_lower_bound(Fin fin, long long lo, long long hi, long long g, long long b, float density) {
    if (lo >= hi) return lo;
    if (density > 0.0f) {
        for (int step = 0; step < WT_ISEARCH_STEPS; step++) {
            const long long f = fin(g);
            if (f >= b) hi = g; else lo = g + 1;
            if (lo >= hi) return lo;
            const float span = (float) (hi - lo);
            const float move = fminf(fmaxf((float) (b - f) * density, -span), span);
            g += (long long) move;
            if (g < lo) g = lo;
            if (g > hi - 1) g = hi - 1;
        }
    }
    return wt_gallop_lower_bound(fin, lo, hi, g, b);
}

// first x in [lo, hi) with fin[x] >= b (hi if none), starting from a guess g in [lo, hi)
WT_DEV long long wt_lane_lower_bound(const int32_t *fin, long long lo, long long hi, long long g, long long b) {
    return wt_gallop_lower_bound(WtFinArray{fin}, lo, hi, g, b);
}

#endif  // WT_ISEARCH_H_
