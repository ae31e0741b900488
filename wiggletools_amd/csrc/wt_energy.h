// wt_energy.h -- energy spectra of whole run lists (device + -DWT_EMU): the reference's EnergyIntegrator (src/statistics.c:345-391;
// the parser's `energy (wavelength) (iterator)`), for any number of wavelengths in one pass.  This header is the single source of
// the logic.  It is compiled
//   * by hipcc for gfx950 inside csrc/wt_energy.hip (the product),
//   * by g++ with -DWT_EMU inside tests/energy_emu.cpp, which runs the workgroups of every pass one after the other in any order
//     on the CPU, and
//   * as plain C++ inside the drop-in layer (csrc/wt_abi_energy.h), which uses the host sweep at the end.
//
// Input (the layout of wtamd_runs_histogram): n_seg segments, seg_off[n_seg + 1], start / finish / value, and one int64 base per
// segment that is added to its coordinates.  Inside a segment the runs are sorted and disjoint (start[i] >= finish[i - 1]) and
// start < finish.
//
// THE RULE.  For a run (s, f, v) of a segment with base B, a = B + s (int64), L = f - s, and a wavelength lam >= 2:
//     sum over p = a .. a + L - 1 of e^(-2 pi i p / lam)  =  D (cos(pi m / lam) - i sin(pi m / lam))
//     D = sin(pi q / lam) / sin(pi / lam),     m = (2 a + L - 1) mod 2 lam  (floor modulus),     q = L mod 2 lam
// and real += v D cos(pi m / lam), im -= v D sin(pi m / lam).  For lam == 1 the sum is L.  The phase is reduced in integers: m and
// q are exact, and the trigonometric functions see only (double) m / lam and (double) q / lam, arguments in [0, 2), through
// sincospi / sinpi.  No position goes through a double.  f32 values are widened first.  A NaN or infinite value makes every
// output NaN (a flag, not arithmetic: inf * 0 would depend on the phase).
//
// THE MODULUS.  2 a + L - 1 = 2 B + (s + f - 1).  bm = 2 (B mod lam) is in [0, 2 lam) and congruent to 2 B; s + f - 1 is in
// [-2^32, 2^32); off = 2 lam ceil(2^32 / (2 lam)) < 2^33 is a multiple of 2 lam.  So u = bm + (s + f - 1) + off is in [0, 2^35)
// and congruent to 2 a + L - 1.  wen_mod(u, d, 1 / d) takes qh = (u64) ((double) u * inv_d): u is exact in a double, the product
// carries two roundings of 2^-53, and (u / d + 1) 2^-52 < 2^-16 / d < 1 / d, so qh is floor(u / d) or one less and u - qh d is
// in [0, 2 d): one correction.  B mod lam is one 64-bit division per (segment, wavelength): per workgroup where its share lies in
// one segment, per run otherwise.  tests/test_energy_mod.py checks the whole chain against integer arithmetic.
//
// FIXED ORDER.  A lane takes the runs r0 + j WEN_BLOCK + l of its workgroup's share, j rising, and adds them in that order; the
// workgroup merges its lanes by a halving tree in LDS and writes one {re, im} per wavelength to part[block]; the final pass has
// one workgroup per output, whose lane l adds part[l], part[l + WEN_BLOCK], ... in that order, then the same tree.  No
// floating-point atomic anywhere: the same list gives the same bits on every call and under any order of workgroups.
//
//   last    one lane per segment: the finish of its last run (0 for an empty one), for the offset rule
//   main    WEN_SHARE runs per workgroup.  Wavelengths are served WEN_KCHUNK at a time: a lane loads WEN_BATCH runs (the loads
//           in flight together), then walks the chunk's wavelengths -- a uniform loop, the wavelength's constants scalar -- with
//           its accumulators (2 WEN_KCHUNK doubles) in its own LDS column.  A later chunk reads the share again (from L2).  The
//           first chunk also validates: start < finish, start >= the finish before it inside a segment (counted in WEN_S_ERR),
//           and raises WEN_S_POISON on a value that is not finite.
//   final   the workgroups' partials into out[2 n_lam]; NaN when poisoned
#ifndef WT_ENERGY_H_
#define WT_ENERGY_H_

#include <math.h>
#include <string.h>

#include <vector>

#include "wt_cover.h"

#define WEN_BLOCK WCV_BLOCK
#define WEN_RUNS_PER_LANE 64                    // runs one lane of the main pass takes
#define WEN_SHARE (WEN_BLOCK * WEN_RUNS_PER_LANE)       // a workgroup's share of runs
#define WEN_BATCH 4                             // runs a lane loads before it uses the first
#define WEN_KCHUNK 8                            // wavelengths served from one load of a batch (2 doubles of LDS per lane each)
#define WEN_MAX_WAVELENGTHS 1024                // of one call
static_assert(WEN_RUNS_PER_LANE % WEN_BATCH == 0, "a lane's runs are whole batches");
#define WEN_MAX_BASE ((1ll << 62) - (1ll << 31))        // |base| of a segment with runs: base + coordinate stays inside +-2^62
#ifndef WEN_PROBE
#define WEN_PROBE 0                             // 1 / 2: variants that leave a part of wen_add out, for tools/energy_time.py --lib (build.py: build_source_variant)
#endif

enum { WEN_K_LAST = 0, WEN_K_MAIN, WEN_K_FINAL, WEN_K_COUNT_ };
enum { WEN_S_ERR = 0, WEN_S_POISON = 1, WEN_S_N = 2 };

// a wavelength and what the host derives from it
struct WenLam {
    unsigned int lam, d;                        // d = 2 lam
    unsigned long long off;                     // the multiple of d that makes the numerator non-negative
    double inv_d;                               // 1 / d rounded
    double inv_sin;                             // 1 / sin(pi / lam) (lam >= 2)
};

#define WEN_LDS_DOUBLES (2 * WEN_KCHUNK * WEN_BLOCK)
struct WenLds {
    double w[WEN_LDS_DOUBLES];                  // main: row 2 k the lanes' real sums of wavelength k, row 2 k + 1 the imaginary; final: row 0
    unsigned int bm[WEN_KCHUNK];                // main: 2 (base mod lam) of the share's first segment
};

struct WenArgs {
    const int32_t *start, *finish;
    const void *value;
    int value_is_f64;
    long long n, n_seg;
    const int64_t *seg_off;                     // [n_seg + 1] (device)
    const int64_t *base;                        // [n_seg]
    int32_t *lastfin;                           // [n_seg]
    const WenLam *lam;                          // [n_lam]
    int n_lam;
    long long blocks;                           // workgroups of the main pass
    double *part;                               // [blocks][2 n_lam]
    double *out;                                // [2 n_lam], then WEN_S_N 64-bit scalars
    long long *scalars;
};

WCV_DEV double wen_value(const WenArgs &a, long long i) {
    return a.value_is_f64 ? ((const double *) a.value)[i] : (double) ((const float *) a.value)[i];
}

// x mod d for x < 2^35 and inv_d = 1 / d rounded (the proof stands at the top)
WCV_DEV unsigned int wen_mod(unsigned long long x, unsigned int d, double inv_d) {
    const unsigned long long qh = (unsigned long long) ((double) x * inv_d);
    unsigned long long r = x - qh * (unsigned long long) d;
    if (r >= d) r -= d;
    return (unsigned int) r;
}

// 2 (base mod lam), floor modulus: congruent to 2 base modulo 2 lam
WCV_DEV unsigned int wen_bm(long long base, unsigned int lam) {
    long long r = base % (long long) lam;
    if (r < 0) r += (long long) lam;
    return 2u * (unsigned int) r;
}

// m and q of a run
WCV_DEV void wen_phase(const WenLam &w, unsigned int bm, int32_t s, int32_t f, unsigned int *m, unsigned int *q) {
    const unsigned long long u = (unsigned long long) ((long long) bm + (long long) w.off + (long long) s + (long long) f - 1);
    *m = wen_mod(u, w.d, w.inv_d);
    *q = wen_mod((unsigned long long) ((long long) f - (long long) s), w.d, w.inv_d);
}

// sin(pi x) and cos(pi x), x in [0, 2)
#ifdef WT_EMU
WCV_DEV void wen_sincospi(double x, double *sn, double *cs) {
    const int n = (int) (2.0 * x + 0.5);        // the nearest multiple of 1/2; x - n / 2 is exact and at most 1/4 in size
    const double r = x - 0.5 * (double) n;
    const double s0 = sin(3.14159265358979323846 * r), c0 = cos(3.14159265358979323846 * r);
    switch (n & 3) {
    case 0: *sn = s0; *cs = c0; break;
    case 1: *sn = c0; *cs = -s0; break;
    case 2: *sn = -s0; *cs = -c0; break;
    default: *sn = -c0; *cs = s0; break;
    }
}
WCV_DEV double wen_sinpi(double x) { double s, c; wen_sincospi(x, &s, &c); return s; }
#else
WCV_DEV void wen_sincospi(double x, double *sn, double *cs) { sincospi(x, sn, cs); }
WCV_DEV double wen_sinpi(double x) { return sinpi(x); }
#endif

// one run into the sums of one wavelength
WCV_DEV void wen_add(const WenLam &w, unsigned int bm, int32_t s, int32_t f, double v, double *re, double *im) {
    if (w.lam == 1) { *re += v * (double) ((long long) f - (long long) s); return; }
    unsigned int m, q;
#if WEN_PROBE == 2                              // (timing probe: the trigonometry without the phase reduction -- wrong sums)
    m = (unsigned int) s % 16u; q = (unsigned int) (f - s) % 16u;
#else
    wen_phase(w, bm, s, f, &m, &q);
#endif
#if WEN_PROBE == 1                              // (timing probe: the phase reduction without the trigonometry -- wrong sums)
    *re += v * (double) m; *im -= v * (double) q;
    return;
#endif
    double sn, cs;
    wen_sincospi((double) m / (double) w.lam, &sn, &cs);
    const double t = v * (wen_sinpi((double) q / (double) w.lam) * w.inv_sin);
    *re += t * cs;
    *im -= t * sn;
}

// ---- last: the finish of every segment's last run ----
WCV_DEV void wen_last_block(const WenArgs &a, long long block) {
    WCV_LANES(l) {
        const long long g = block * WEN_BLOCK + l;
        if (g >= a.n_seg) continue;
        const long long e = a.seg_off[g + 1];
        a.lastfin[g] = e > (long long) a.seg_off[g] ? a.finish[e - 1] : 0;
    }
}

// the halving tree over the lanes of `rows` rows of w
WCV_DEV void wen_tree(double *w, int rows) {
    for (int s = WEN_BLOCK / 2; s > 0; s >>= 1) {
        WCV_SYNC();
        WCV_LANES(l) {
            if (l < s)
                for (int j = 0; j < rows; j++) w[j * WEN_BLOCK + l] += w[j * WEN_BLOCK + l + s];
        }
    }
    WCV_SYNC();
}

// ---- main: one workgroup, WEN_SHARE runs, every wavelength ----
WCV_DEV void wen_main_block(const WenArgs &a, long long block, double *w, unsigned int *bmk) {
    const long long r0 = block * WEN_SHARE, r1 = r0 + WEN_SHARE < a.n ? r0 + WEN_SHARE : a.n;
    const long long g0 = wcv_seg_of(a.seg_off, a.n_seg, r0);
    const bool one = g0 == wcv_seg_of(a.seg_off, a.n_seg, r1 - 1);      // the share lies in one segment (uniform)
    const long long seg0 = a.seg_off[g0], base0 = a.base[g0];
    for (int k0 = 0; k0 < a.n_lam; k0 += WEN_KCHUNK) {
        const int kn = a.n_lam - k0 < WEN_KCHUNK ? a.n_lam - k0 : WEN_KCHUNK;
        WCV_LANES(l) {
            if (l < kn) bmk[l] = wen_bm(base0, a.lam[k0 + l].lam);
            for (int j = 0; j < 2 * kn; j++) w[j * WEN_BLOCK + l] = 0.0;
        }
        WCV_SYNC();
        WCV_LANES(l) {
            long long bad = 0;
            bool poison = false;
            for (int j0 = 0; j0 < WEN_RUNS_PER_LANE; j0 += WEN_BATCH) {
                if (r0 + (long long) j0 * WEN_BLOCK >= r1) break;       // (uniform over the workgroup)
                int32_t s[WEN_BATCH], f[WEN_BATCH];
                double v[WEN_BATCH];
                long long bs[WEN_BATCH];
                bool live[WEN_BATCH];
#pragma unroll
                for (int b = 0; b < WEN_BATCH; b++) {                   // (past the end: the last run again, not used)
                    const long long i = r0 + (long long) (j0 + b) * WEN_BLOCK + l;
                    live[b] = i < r1;
                    const long long ii = live[b] ? i : r1 - 1;
                    s[b] = a.start[ii]; f[b] = a.finish[ii]; v[b] = wen_value(a, ii);
                    bs[b] = base0;
                    long long first = seg0;
                    if (!one) {
                        const long long g = wcv_seg_of(a.seg_off, a.n_seg, ii);
                        bs[b] = a.base[g];
                        first = a.seg_off[g];
                    }
                    if (k0 == 0 && live[b]) {
                        if (s[b] >= f[b]) bad++;
                        if (ii > first && s[b] < a.finish[ii - 1]) bad++;
                        if (v[b] - v[b] != 0.0) poison = true;
                    }
                    if (v[b] - v[b] != 0.0) v[b] = 0.0;                 // (the flag speaks for it)
                }
                for (int k = 0; k < kn; k++) {
                    const WenLam lam = a.lam[k0 + k];
                    double re = w[(2 * k) * WEN_BLOCK + l], im = w[(2 * k + 1) * WEN_BLOCK + l];
#pragma unroll
                    for (int b = 0; b < WEN_BATCH; b++)
                        if (live[b]) wen_add(lam, one ? bmk[k] : wen_bm(bs[b], lam.lam), s[b], f[b], v[b], &re, &im);
                    w[(2 * k) * WEN_BLOCK + l] = re; w[(2 * k + 1) * WEN_BLOCK + l] = im;
                }
            }
            if (bad) wcv_add64(&a.scalars[WEN_S_ERR], bad);
            if (poison) wcv_or64((unsigned long long *) &a.scalars[WEN_S_POISON], 1ull);
        }
        wen_tree(w, 2 * kn);
        WCV_LANES(l) {
            if (l < 2 * kn) a.part[block * (2ll * a.n_lam) + 2 * k0 + l] = w[l * WEN_BLOCK];
        }
        WCV_SYNC();
    }
}

// ---- final: output j = block; the partials of the workgroups in a fixed order ----
WCV_DEV void wen_final_block(const WenArgs &a, long long block, double *w) {
    WCV_LANES(l) {
        double sum = 0.0;
        for (long long b = l; b < a.blocks; b += WEN_BLOCK) sum += a.part[b * (2ll * a.n_lam) + block];
        w[l] = sum;
    }
    wen_tree(w, 1);
    WCV_LANES(l) {
        if (l == 0) a.out[block] = a.scalars[WEN_S_POISON] ? (double) NAN : w[0];
    }
}

// pass `kernel`, one workgroup
WCV_DEV void wen_run_words(int kernel, const WenArgs &a, long long block, double *w, unsigned int *bm) {
    switch (kernel) {
    case WEN_K_LAST: wen_last_block(a, block); break;
    case WEN_K_MAIN: wen_main_block(a, block, w, bm); break;
    case WEN_K_FINAL: wen_final_block(a, block, w); break;
    default: break;
    }
}
WCV_DEV void wen_run_block(int kernel, const WenArgs &a, long long block, WenLds *lds) { wen_run_words(kernel, a, block, lds->w, lds->bm); }

// ---- host side: checks, the wavelengths' table, the offset rule ----

// what every entry checks before it touches anything; "" when fine
static inline const char *wen_check(long long n_seg, const int64_t *seg_off, const int32_t *start, const int32_t *finish, const void *value,
                                    int n_lam, const int32_t *wavelength, const double *reim) {
    if (n_seg < 0 || (n_seg > 0 && !seg_off) || !reim) return "bad argument";
    if (n_lam < 1 || !wavelength) return "there must be a wavelength";
    if (n_lam > WEN_MAX_WAVELENGTHS) return "more than WEN_MAX_WAVELENGTHS (1024) wavelengths";
    for (int k = 0; k < n_lam; k++)
        if (wavelength[k] < 1) return "a wavelength below 1";
    if (n_seg > 0 && seg_off[0] != 0) return "bad argument";
    for (long long g = 0; g < n_seg; g++)
        if (seg_off[g + 1] < seg_off[g]) return "segment offsets decrease";
    const long long n = n_seg ? (long long) seg_off[n_seg] : 0;
    if (n >= (1ll << 31) || (n > 0 && (!start || !finish || !value))) return "bad argument";
    return "";
}

static inline void wen_table(int n_lam, const int32_t *wavelength, std::vector<WenLam> *tab) {
    for (int k = 0; k < n_lam; k++) {
        WenLam w;
        w.lam = (unsigned int) wavelength[k];
        w.d = 2u * w.lam;
        w.off = (unsigned long long) w.d * (((1ull << 32) + w.d - 1) / w.d);
        w.inv_d = 1.0 / (double) w.d;
        w.inv_sin = w.lam >= 2 ? 1.0 / sin(3.14159265358979323846 / (double) w.lam) : 0.0;
        tab->push_back(w);
    }
}

// The bases of the segments -- seg_base, or the reference's rule from 0 over the last finishes -- and the base a following
// segment would get.  false: a segment with runs has a base beyond WEN_MAX_BASE.
static inline bool wen_bases(long long n_seg, const int64_t *seg_off, const int64_t *seg_base, const int32_t *lastfin, std::vector<int64_t> *base,
                             int64_t *end_base) {
    base->assign((size_t) (n_seg ? n_seg : 1), 0);
    int64_t run = 0, end = n_seg > 0 && seg_base ? seg_base[n_seg - 1] : 0;
    for (long long g = 0; g < n_seg; g++) {
        const bool any = seg_off[g + 1] > seg_off[g];
        const int64_t b = seg_base ? seg_base[g] : run;
        (*base)[(size_t) g] = b;
        if (!any) continue;
        if (b > WEN_MAX_BASE || b < -WEN_MAX_BASE) return false;
        end = run = b + (int64_t) lastfin[g];
    }
    *end_base = end;
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------
// The door, written once over a Launcher: the one of wt_cover.h (alloc, release, zero, to_host, to_device) with
//     bool run_energy(int kernel, long long blocks, const WenArgs &a)     and     bool sync()
// Return value: 0 fine, 1 bad argument, 2 launcher failure.  Nothing is written to reim or end_base unless the value is 0.
// Temporary memory: 16 n_lam bytes per workgroup of the main pass (one per WEN_SHARE runs), 48 n_lam + 16 bytes of table,
// outputs and scalars, 20 bytes per segment.
// ---------------------------------------------------------------------------------------------------------------------
#ifndef WCV_NO_HOST

template <class L>
static int wen_door(L &l, long long n_seg, const int64_t *seg_off, const int64_t *seg_base, const int32_t *start, const int32_t *finish,
                    const void *value, int value_is_f64, int n_lam, const int32_t *wavelength, double *reim, int64_t *end_base, const char **why) {
    *why = wen_check(n_seg, seg_off, start, finish, value, n_lam, wavelength, reim);
    if (**why) return 1;
    WenArgs a = {};
    a.start = start; a.finish = finish; a.value = value; a.value_is_f64 = value_is_f64;
    a.n = n_seg ? (long long) seg_off[n_seg] : 0;
    a.n_seg = n_seg; a.n_lam = n_lam;
    a.blocks = wcv_blocks(a.n, WEN_SHARE);
    std::vector<int32_t> lastfin((size_t) (n_seg ? n_seg : 1), 0);
    std::vector<int64_t> base;
    std::vector<double> out((size_t) (2 * n_lam + WEN_S_N), 0.0);
    int64_t end = 0;
    WcvScope<L> sc(l);
    if (a.n > 0) {
        int64_t *d_seg = nullptr;
        if (!sc.get(&d_seg, (size_t) n_seg + 1) || !sc.get(&a.lastfin, (size_t) n_seg)) { *why = "device memory"; return 2; }
        a.seg_off = d_seg;
        if (!l.to_device(d_seg, seg_off, sizeof(int64_t) * ((size_t) n_seg + 1)) || !l.run_energy(WEN_K_LAST, wcv_blocks(n_seg, WEN_BLOCK), a) ||
            !l.to_host(lastfin.data(), a.lastfin, sizeof(int32_t) * (size_t) n_seg)) { *why = "last pass"; return 2; }
    }
    if (!wen_bases(n_seg, seg_off, seg_base, lastfin.data(), &base, &end)) { *why = "a segment's base puts its coordinates outside +-2^62"; return 1; }
    if (a.n > 0) {
        // one blob: the bases, then the table
        std::vector<WenLam> tab;
        wen_table(n_lam, wavelength, &tab);
        static_assert(sizeof(WenLam) == 32, "the table's entries are 32 bytes");
        std::vector<unsigned char> blob(sizeof(int64_t) * (size_t) n_seg + sizeof(WenLam) * tab.size());
        memcpy(blob.data(), base.data(), sizeof(int64_t) * (size_t) n_seg);
        memcpy(blob.data() + sizeof(int64_t) * (size_t) n_seg, tab.data(), sizeof(WenLam) * tab.size());
        int64_t *d_blob = nullptr;
        if (!sc.get(&d_blob, blob.size() / 8) || !sc.get(&a.part, (size_t) a.blocks * 2 * (size_t) n_lam) || !sc.get(&a.out, out.size()))
            { *why = "device memory"; return 2; }
        a.base = d_blob;
        a.lam = (const WenLam *) (d_blob + n_seg);
        a.scalars = (long long *) (a.out + 2 * n_lam);
        if (!l.to_device(d_blob, blob.data(), blob.size()) || !l.zero(a.scalars, sizeof(long long) * WEN_S_N) ||
            !l.run_energy(WEN_K_MAIN, a.blocks, a) || !l.run_energy(WEN_K_FINAL, 2 * n_lam, a) ||
            !l.to_host(out.data(), a.out, sizeof(double) * out.size())) { *why = "main pass"; return 2; }
        long long sc2[WEN_S_N];
        memcpy(sc2, out.data() + 2 * n_lam, sizeof sc2);
        if (sc2[WEN_S_ERR]) { *why = "a run with start >= finish, or a segment that is not sorted and disjoint"; return 1; }
    }
    memcpy(reim, out.data(), sizeof(double) * 2 * (size_t) n_lam);
    if (end_base) *end_base = end;
    return 0;
}

#endif  // WCV_NO_HOST

// The same rule on the host, without a device (a translation unit compiled with -DWT_EMU): one sweep, every wavelength's sums in
// run order.  The same arguments and refusals as the door's with the run arrays in host memory; equal to the door to rounding,
// not bit for bit (another order of additions, the host's libm).
#ifdef WT_EMU

static int wen_host(long long n_seg, const int64_t *seg_off, const int64_t *seg_base, const int32_t *start, const int32_t *finish,
                    const double *value, int n_lam, const int32_t *wavelength, double *reim, int64_t *end_base) {
    if (*wen_check(n_seg, seg_off, start, finish, value, n_lam, wavelength, reim)) return 1;
    std::vector<int32_t> lastfin((size_t) (n_seg ? n_seg : 1), 0);
    bool poison = false;
    for (long long g = 0; g < n_seg; g++)
        for (long long i = seg_off[g]; i < (long long) seg_off[g + 1]; i++) {
            if (start[i] >= finish[i] || (i > (long long) seg_off[g] && start[i] < finish[i - 1])) return 1;
            if (value[i] - value[i] != 0.0) poison = true;
            lastfin[(size_t) g] = finish[i];
        }
    std::vector<int64_t> base;
    int64_t end = 0;
    if (!wen_bases(n_seg, seg_off, seg_base, lastfin.data(), &base, &end)) return 1;
    std::vector<WenLam> tab;
    wen_table(n_lam, wavelength, &tab);
    for (int k = 0; k < n_lam; k++) {
        double re = 0.0, im = 0.0;
        for (long long g = 0; g < n_seg && !poison; g++) {
            const unsigned int bm = wen_bm(base[(size_t) g], tab[(size_t) k].lam);
            for (long long i = seg_off[g]; i < (long long) seg_off[g + 1]; i++) wen_add(tab[(size_t) k], bm, start[i], finish[i], value[i], &re, &im);
        }
        reim[2 * k] = poison ? (double) NAN : re;
        reim[2 * k + 1] = poison ? (double) NAN : im;
    }
    if (end_base) *end_base = end;
    return 0;
}
#endif  // WT_EMU

#endif  // WT_ENERGY_H_
