// wt_abi_hist.h -- part of the DROP-IN LAYER (csrc/wt_iter_abi.cpp includes it after wt_abi_runs.h): the reference's
// histogram(), normalize_histogram() and print_histogram() (src/plots.c:167-223; `histogram`, commandParser.c readHistogram) as
// wtamd_histogram, wtamd_normalize_histogram and wtamd_print_histogram.  Row r is wigs[r].  Every child is drained whole
// (reg_drain_chrom: blocks from this library's sources and reducers, pop() otherwise).  The range is known only when the last
// child is exhausted, so the runs of all rows are held until then: 16 bytes per run (start, finish, the value as a double) of
// host memory, which the door's host entry stages on the device in one piece.  Then one call of wtamd_runs_histogram_host
// (csrc/wt_hist.hip), one segment per row.
//
// The door is reached through a WEAK reference: a build of this layer without the HIP units has none and sweeps on the host by
// the same rule -- whs_host of csrc/wt_hist.h, compiled here as plain C++ (the same bits) --, as does WTAMD_NO_DEVICE_HIST=1.
//
// Departures from the reference, which streams with a provisional range and re-bins whenever a value leaves it:
//  1. its re-binning smears mass by linear interpolation (raiseMaxNRows, plots.c:137-146); here bins are exact over the final
//     range.  Lengths 4, values 0, 1, 0.5, 2, 0.25, width 4: the reference gives 8 8 0 4, the exact answer is 8 4 4 4;
//  2. its lowering re-bin reads and writes one column past each row (plots.c:108): it has no defined result;
//  3. at width 1 it loses all earlier mass when the second distinct value is lower (plots.c:113-116); here width 1 gives the
//     total span;
//  4. it keeps the sign of the run that set a zero extreme; here a zero extreme is +0.0 (seen only in the printed centre of an
//     all -0.0 input).
// The two are equal, bit for bit, exactly when no value lies outside the interval spanned by the stream's first two distinct
// non-NaN values and either width >= 2 or the second of them is higher.  A first row without a non-NaN value, on which the
// reference does not return, gives a NaN range and zeros.
#ifndef WT_ABI_HIST_H_
#define WT_ABI_HIST_H_

#ifndef WT_EMU
#define WT_EMU 1
#endif
#ifndef WCV_NO_HOST
#define WCV_NO_HOST 1
#endif
#include "wt_hist.h"

extern "C" int wtamd_runs_histogram_host(int64_t n_seg, const int64_t *seg_off, const int32_t *seg_row, int32_t n_rows, const int32_t *start,
                                         const int32_t *finish, const double *value, int32_t width, uint32_t flags, double *range2, double *hist)
    __attribute__((weak));

struct wtamd_histogram_st {
    int width = 0, count = 0;
    std::vector<double> values;         // count x width
    double lo = NAN, hi = NAN;
};

namespace {

[[noreturn]] void hist_refuse(const char *what) {
    fprintf(stderr, "wiggletools_amd: wtamd_histogram: %s\n", what);
    exit(1);
}

}  // namespace

extern "C" {

wtamd_Histogram *wtamd_histogram(WiggleIterator **wigs, int count, int width) {
    if (width < 1) hist_refuse("the width must be 1 or more");
    if (count < 1 || !wigs) hist_refuse("there must be an iterator");
    RegRuns runs;
    Interner names;
    std::vector<int64_t> seg((size_t) count + 1, 0);
    std::vector<int32_t> row((size_t) count);
    for (int r = 0; r < count; r++) {
        WiggleIterator *it = wigs[r];
        while (!it->done) reg_drain_chrom(it, names.get(it->chrom), &runs);
        seg[(size_t) r + 1] = (int64_t) runs.s.size();
        row[(size_t) r] = r;
    }
    if (runs.s.size() >= (size_t) 1 << 31) hist_refuse("2^31 runs or more");
    wtamd_Histogram *h = new wtamd_Histogram();
    h->width = width; h->count = count;
    h->values.assign((size_t) count * (size_t) width, 0.0);
    double range2[2] = {NAN, NAN};
    int rc;
    if (wt_use_device((const void *) wtamd_runs_histogram_host, "WTAMD_NO_DEVICE_HIST")) {
        rc = wtamd_runs_histogram_host(count, seg.data(), row.data(), count, runs.s.data(), runs.f.data(), runs.v.data(), width, 0, range2, h->values.data());
        if (rc != WTAMD_OK && rc != WTAMD_ERR_ARG) die("wtamd_runs_histogram");
    } else {
        rc = whs_host(count, seg.data(), row.data(), count, runs.s.data(), runs.f.data(), runs.v.data(), width, 0, range2, h->values.data());
    }
    if (rc != 0) hist_refuse("an interval with start >= finish, or an infinite value");
    h->lo = range2[0]; h->hi = range2[1];
    return h;
}

// plots.c:196-208
void wtamd_normalize_histogram(wtamd_Histogram *h) {
    for (int r = 0; r < h->count; r++) {
        double *v = h->values.data() + (size_t) r * (size_t) h->width;
        double sum = 0;
        for (int c = 0; c < h->width; c++) sum += v[c];
        for (int c = 0; c < h->width; c++) v[c] /= sum;
    }
}

// plots.c:210-223
void wtamd_print_histogram(wtamd_Histogram *h, FILE *file) {
    const double step = (h->hi - h->lo) / h->width;
    double position = h->lo;
    for (int c = 0; c < h->width; c++) {
        fprintf(file, "%f", position + step / 2);
        for (int r = 0; r < h->count; r++) fprintf(file, "\t%f", h->values[(size_t) r * (size_t) h->width + (size_t) c]);
        fprintf(file, "\n");
        position += step;
    }
}

int wtamd_histogram_width(const wtamd_Histogram *h) { return h->width; }
int wtamd_histogram_count(const wtamd_Histogram *h) { return h->count; }
const double *wtamd_histogram_row(const wtamd_Histogram *h, int row) {
    return row >= 0 && row < h->count ? h->values.data() + (size_t) row * (size_t) h->width : nullptr;
}
void wtamd_histogram_range(const wtamd_Histogram *h, double *lo_hi2) { lo_hi2[0] = h->lo; lo_hi2[1] = h->hi; }
void wtamd_destroy_histogram(wtamd_Histogram *h) { delete h; }

}  // extern "C"

#endif  // WT_ABI_HIST_H_
