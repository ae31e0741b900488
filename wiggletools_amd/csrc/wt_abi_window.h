// wt_abi_window.h -- part of the DROP-IN LAYER (csrc/wt_iter_abi.cpp includes it after wt_abi_profile.h): the reference's
// BinningWiggleIterator (src/unaryOps.c:963-1036; `bin`) and SmoothWiggleIterator (:1039-1162; `smooth`) as wtamd_BinIterator
// and wtamd_SmoothIterator.  Either drains its child one chromosome at a time (reg_drain_chrom: blocks from this library's
// sources and reducers, pop() otherwise), puts the union in front when child->overlaps, computes the chromosome through the
// device door (wtamd_runs_bin_host / wtamd_runs_smooth_host, csrc/wt_window.hip) and serves the finished run list as a
// ServedRuns (csrc/wt_abi_runs.h).  Smooth is served in clip slices of WIN_SLICE positions: the chromosome's runs stay, its
// output never takes more than 16 bytes x WIN_SLICE of host memory at once.
//
// The doors are reached through WEAK references: a build of this layer without the HIP units has none and sweeps on the host by
// the same rules -- wwn_bin_host / wwn_smooth_host of csrc/wt_window.h, compiled here as plain C++ (the same bits) --, as does
// WTAMD_NO_DEVICE_WINDOW=1.
//
// A chromosome with a start below 1 is outside the doors' input: it is served by the reference's own per-pop loops, restated
// below (C's division towards zero at :994, the prefill of :1118-1124).  One departure: the reference's smooth carries its
// running sum from one chromosome to the next; here every chromosome starts from 0.
#ifndef WT_ABI_WINDOW_H_
#define WT_ABI_WINDOW_H_

#ifndef WT_EMU
#define WT_EMU 1
#endif
#ifndef WCV_NO_HOST
#define WCV_NO_HOST 1
#endif
#include "wt_window.h"

extern "C" int wtamd_runs_bin_host(int64_t n, const int32_t *start, const int32_t *finish, const double *value, int32_t width, double default_value,
                                   int64_t capacity, int32_t *o_start, int32_t *o_finish, double *o_value, int64_t *n_out) __attribute__((weak));
extern "C" int wtamd_runs_smooth_host(int64_t n, const int32_t *start, const int32_t *finish, const double *value, int32_t width, int32_t clip_lo,
                                      int32_t clip_hi, int64_t capacity, int32_t *o_start, int32_t *o_finish, double *o_value, int64_t *n_out)
    __attribute__((weak));

namespace {

const long long WIN_SLICE = 1ll << 20;     // positions of one smooth slice

// WTAMD_WINDOW_SLICE=<positions>: the slice of wtamd_SmoothIterator; the tests force it small
long long win_slice() {
    const char *e = getenv("WTAMD_WINDOW_SLICE");
    const long long b = e ? atoll(e) : 0;
    return b > 0 ? b : WIN_SLICE;
}

struct WinIter : ServedRuns {      // (csrc/wt_abi_runs.h: BulkSource hdr stays first)
    WiggleIterator *child = nullptr;
    Interner names;
    RegRuns in;                     // the chromosome's runs, after the union
    int width = 2;
    bool smooth = false;
    bool slicing = false;           // smooth: slices of the chromosome in `in` are still to come, from position `next`
    long long next = 0, end = 0;
};

// UnionWiggleIterator (:60-92) over one chromosome: a run joins the group while group.finish > start
void win_union(RegRuns &r) {
    size_t k = 0;
    for (size_t i = 0; i < r.s.size(); i++) {
        if (k > 0 && r.f[k - 1] > r.s[i]) { if (r.f[i] > r.f[k - 1]) r.f[k - 1] = r.f[i]; continue; }
        r.s[k] = r.s[i]; r.f[k] = r.f[i]; r.v[k] = r.v[i];
        k++;
    }
    r.s.resize(k); r.f.resize(k); r.v.resize(k);
}

// BinningWiggleIteratorPop (:978-1025) over one chromosome, pop by pop
void win_bin_literal(const RegRuns &in, int width, double dflt, RegRuns &o) {
    const size_t n = in.s.size();
    size_t j = 0;
    bool have = false;
    long long wfinish = 0;
    while (j < n) {
        const long long start = have && in.s[j] < wfinish + width ? wfinish : (long long) ((in.s[j] - 1) / width) * width + 1;
        have = true;
        wfinish = start + width;
        double value = 0;
        long long total = 0;
        while (j < n && in.s[j] < wfinish) {
            const long long a = in.s[j] < start ? start : in.s[j], b = in.f[j] > wfinish ? wfinish : in.f[j];
            value += (double) (int) (b - a) * in.v[j];
            total += b - a;
            if (in.f[j] > wfinish) break;
            j++;
        }
        if (dflt != 0.0 && total < width) value += (double) (width - total) * dflt;
        o.push((int32_t) start, (int32_t) wfinish, value);
    }
}

// SmoothWiggleIteratorPop (:1102-1136) with its helpers (:1053-1100) over one chromosome, pop by pop
void win_smooth_literal(const RegRuns &in, int width, RegRuns &o) {
    const size_t n = in.s.size();
    std::vector<double> buffer((size_t) width, 0.0);
    double sum = 0;
    int latest = 0, oldest = 0, count = 0;
    long long last_position = 0, start = 0;
    size_t j = 0;
    auto read_one = [&](long long position) {
        while (j < n && in.f[j] <= position) j++;
        if (j >= n) return;
        if (in.s[j] <= position) { buffer[(size_t) latest] = in.v[j]; sum += in.v[j]; }
        else buffer[(size_t) latest] = 0;
        count++;
        last_position = position;
        if (++latest >= width) latest = 0;
    };
    for (;;) {
        if (j >= n && count == 0) return;
        if (count == 0) {
            start = (long long) in.s[j] - width / 2;
            if (start < 1) {
                start = 1;
                for (int i = 0; i < width / 2; i++) read_one(start + i);
            }
        } else {
            start++;
        }
        read_one(start + width / 2);
        o.push((int32_t) start, (int32_t) (start + 1), sum / width);
        if (count == width || last_position < start + width / 2) {
            if (buffer[(size_t) oldest] != buffer[(size_t) oldest]) {
                sum = 0;
                for (int q = 1; q < count; q++) sum += buffer[(size_t) ((oldest + q) % width)];
            } else {
                sum -= buffer[(size_t) oldest];
            }
            count--;
            if (++oldest >= width) oldest = 0;
        }
    }
}

[[noreturn]] void win_refuse(const WinIter *c, const char *what) {
    fprintf(stderr, "wiggletools_amd: wtamd_%sIterator: %s: %s\n", c->smooth ? "Smooth" : "Bin", c->chrom, what);
    exit(1);
}

// one call of a door (or of its host sweep) into c->out, which holds `cap` entries
void win_call(WinIter *c, long long cap, long long clip_lo, long long clip_hi) {
    RegRuns &o = c->out;
    const RegRuns &in = c->in;
    const int64_t n = (int64_t) in.s.size();
    o.s.resize((size_t) cap); o.f.resize((size_t) cap); o.v.resize((size_t) cap);
    int rc;
    long long got = 0;
    if (wt_use_device(c->smooth ? (const void *) wtamd_runs_smooth_host : (const void *) wtamd_runs_bin_host, "WTAMD_NO_DEVICE_WINDOW")) {
        int64_t n_out = 0;
        rc = c->smooth ? wtamd_runs_smooth_host(n, in.s.data(), in.f.data(), in.v.data(), c->width, (int32_t) clip_lo, (int32_t) clip_hi, cap, o.s.data(),
                                                o.f.data(), o.v.data(), &n_out)
                       : wtamd_runs_bin_host(n, in.s.data(), in.f.data(), in.v.data(), c->width, c->child->default_value, cap, o.s.data(), o.f.data(),
                                             o.v.data(), &n_out);
        if (rc != WTAMD_OK && rc != WTAMD_ERR_ARG) die(c->smooth ? "wtamd_runs_smooth" : "wtamd_runs_bin");
        got = n_out;
    } else {
        rc = c->smooth ? wwn_smooth_host(n, in.s.data(), in.f.data(), in.v.data(), c->width, clip_lo, clip_hi, cap, o.s.data(), o.f.data(), o.v.data(), &got)
                       : wwn_bin_host(n, in.s.data(), in.f.data(), in.v.data(), c->width, c->child->default_value, cap, o.s.data(), o.f.data(), o.v.data(), &got);
    }
    if (rc != 0) win_refuse(c, "an output coordinate would pass INT32_MAX");         // (the runs themselves were checked by win_load)
    o.s.resize((size_t) got); o.f.resize((size_t) got); o.v.resize((size_t) got);
}

// The next stretch of output: the next slice of the chromosome being smoothed, or the next chromosome(s) of the child until
// one has a result; done when the child is exhausted.
void win_load(ServedRuns *r) {
    WinIter *c = (WinIter *) r;
    WiggleIterator *it = c->child;
    for (;;) {
        if (!c->slicing) {
            if (it->done) { c->done = true; return; }
            c->chrom = c->names.get(it->chrom);
            c->in.clear();
            reg_drain_chrom(it, c->chrom, &c->in);
            if (it->overlaps) win_union(c->in);
            const RegRuns &in = c->in;
            const size_t n = in.s.size();
            for (size_t q = 0; q < n; q++)
                if (in.s[q] >= in.f[q] || (q > 0 && in.f[q - 1] > in.s[q]))
                    win_refuse(c, "not sorted, an interval with start >= finish, or runs that overlap from a child that does not say so");
            if (n == 0) continue;
            if (in.s[0] < 1) {                                  // outside the doors' input: the reference's own loops
                if (c->smooth) win_smooth_literal(in, c->width, c->out);
                else win_bin_literal(in, c->width, it->default_value, c->out);
                if (!c->out.s.empty()) return;
                continue;
            }
            if (!c->smooth) {
                long long cap = 0;
                for (size_t q = 0; q < n; q++) cap += ((long long) in.f[q] - 2) / c->width - ((long long) in.s[q] - 1) / c->width + 1;
                win_call(c, cap, 0, 0);
                return;                                         // (a run always has a bin)
            }
            const WwnSeg isl = wwn_island(0, (long long) n, in.s[0], in.f[n - 1], c->width, 0, 0);
            if (isl.pend + 1 > (long long) INT32_MAX) win_refuse(c, "an output coordinate would pass INT32_MAX");
            c->next = isl.p0; c->end = isl.pend + 1;
            c->slicing = true;
        }
        const long long slice = win_slice(), lo = c->next, hi = c->end - lo > slice ? lo + slice : c->end;
        win_call(c, hi - lo, lo, hi);
        c->next = hi;
        if (hi >= c->end) c->slicing = false;
        if (!c->out.s.empty()) return;
    }
}

void win_seek(WiggleIterator *wi, const char *chrom, int start, int finish) {
    WinIter *c = (WinIter *) (ServedRuns *) wi->data;
    seek(c->child, chrom, start, finish);
    c->slicing = false;
    srv_restart(c, wi);
}

WiggleIterator *win_iterator(WiggleIterator *child, int width, bool smooth) {
    if (width < 2) {
        fprintf(stderr, "Cannot %s over a window of width %i, must be 2 or more\n", smooth ? "smooth" : "bin", width);     // :1030, :1155
        exit(1);
    }
    WinIter *c = new (calloc(1, sizeof(WinIter))) WinIter();
    c->load = &win_load;
    c->child = child;
    c->width = width;
    c->smooth = smooth;
    return srv_iterator(c, &win_seek, 0, smooth ? child->default_value : child->default_value * width);          // :1035, :1161
}

}  // namespace

#endif  // WT_ABI_WINDOW_H_
