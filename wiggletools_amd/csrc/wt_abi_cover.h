// wt_abi_cover.h -- part of the DROP-IN LAYER (csrc/wt_iter_abi.cpp includes it; one translation unit, one anonymous namespace):
// overlapping input.  wtamd_OverlappingArrayReader is the array-backed reader with `overlaps = true` (intervals sorted by
// start only, as the reference's BED / BAM / bigBed readers deliver them); wtamd_CoverageIterator is the reference's
// CoverageWiggleIterator (src/unaryOps.c:303-375) as a bulk source: it drains its child one chromosome at a time, computes
// the chromosome's depth track through the device door (wtamd_runs_coverage, csrc/wt_cover.hip) and serves the finished run
// list as a ServedRuns (csrc/wt_abi_runs.h).
//
// The door is reached through a WEAK reference: a build of this layer without the HIP units (the emulated drop-in library of
// the CPU tests) has no door and sweeps on the host instead, as does WTAMD_NO_DEVICE_COVERAGE=1.  Either way the result is
// the same list of integers.
//
// One deviation from the reference, on purpose: when its child runs dry the reference reads the exhausted child's stale
// start (:333-334) and emits one run with start == finish per stream; this iterator does not.
#ifndef WT_ABI_COVER_H_
#define WT_ABI_COVER_H_

extern "C" int wtamd_runs_coverage_host(int64_t n, const int32_t *start, const int32_t *finish, int64_t capacity, int32_t *o_start,
                                        int32_t *o_finish, double *o_value, int64_t *n_out) __attribute__((weak));

namespace {

// ---------------------------------------------------------------------------
// Array-backed reader of OVERLAPPING intervals (bulk-capable child iterator)
// ---------------------------------------------------------------------------
struct OvlReader {
    BulkSource hdr;                 // must stay first (see wt_bulk_pop)
    int n_chrom = 0;
    char **names = nullptr;         // own copies
    int64_t *seg_off = nullptr;     // own copy
    const int32_t *start = nullptr, *finish = nullptr;
    const float *value = nullptr;
    int c = 0;                      // current chromosome
    int64_t j = 0, end = 0;         // current interval, end of what this chromosome delivers (indices into cs / cf / cv)
    const int32_t *cs = nullptr, *cf = nullptr;     // what is being delivered: the caller's arrays, or the window's copy
    const float *cv = nullptr;
    bool windowed = false, done = false;
    std::vector<int32_t> ws, wf;    // after seek(): the intervals that intersect the window, clipped
    std::vector<float> wv;

    void settle(WiggleIterator *wi) {
        while (!done && j >= end) {
            if (windowed) { done = true; break; }
            c++;
            if (c >= n_chrom) { done = true; break; }
            j = seg_off[c]; end = seg_off[c + 1];
        }
        if (done) { wi->done = 1; return; }
        wi->chrom = names[c];
        wi->start = cs[j]; wi->finish = cf[j];
        wi->value = (double) cv[j];
    }
};

int64_t ovl_peek(BulkSource *b, const int32_t **s, const int32_t **f, const float **v) {
    OvlReader *a = (OvlReader *) b;
    if (a->done || a->j >= a->end) return 0;
    *s = a->cs + a->j; *f = a->cf + a->j; *v = a->cv + a->j;
    return a->end - a->j;
}

void ovl_advance(BulkSource *b, WiggleIterator *wi, int64_t k) {
    OvlReader *a = (OvlReader *) b;
    if (a->done) { wi->done = 1; return; }
    a->j += k;
    a->settle(wi);
}

void ovl_seek(WiggleIterator *wi, const char *chrom, int start, int finish) {
    // what the reference's readers deliver after seek: only that chromosome, the intervals that intersect [start, finish),
    // clipped.  The finishes are in no order, so the window is a filtered copy (the clipped starts stay sorted).
    OvlReader *a = (OvlReader *) wi->data;
    a->windowed = true;
    a->ws.clear(); a->wf.clear(); a->wv.clear();
    for (int c = 0; c < a->n_chrom; c++)
        if (strcmp(a->names[c], chrom) == 0) {
            a->c = c;
            for (int64_t g = a->seg_off[c]; g < a->seg_off[c + 1] && a->start[g] < finish; g++) {
                if (a->finish[g] <= start) continue;
                a->ws.push_back(a->start[g] < start ? start : a->start[g]);
                a->wf.push_back(a->finish[g] > finish ? finish : a->finish[g]);
                a->wv.push_back(a->value[g]);
            }
            break;
        }
    a->cs = a->ws.data(); a->cf = a->wf.data(); a->cv = a->wv.data();
    a->j = 0; a->end = (int64_t) a->ws.size();
    a->done = a->end == 0;
    wi->done = 0;
    if (a->done) { wi->done = 1; return; }
    a->settle(wi);
}

// ---------------------------------------------------------------------------
// Coverage
// ---------------------------------------------------------------------------
// The depth track of one chromosome on the host: starts in order, finishes sorted, one merge.
void cov_host_sweep(const std::vector<int32_t> &s, const std::vector<int32_t> &f, std::vector<int32_t> &os, std::vector<int32_t> &of,
                    std::vector<double> &ov) {
    std::vector<int32_t> fs(f);
    std::sort(fs.begin(), fs.end());
    const size_t n = s.size();
    size_t i = 0, k = 0;
    long long depth = 0;
    while (k < n) {
        const int32_t p = (i < n && s[i] < fs[k]) ? s[i] : fs[k];
        while (i < n && s[i] == p) { depth++; i++; }
        while (k < n && fs[k] == p) { depth--; k++; }
        if (depth > 0) {
            const int32_t nx = (i < n && s[i] < fs[k]) ? s[i] : fs[k];      // (depth > 0: a finish is still to come)
            os.push_back(p); of.push_back(nx); ov.push_back((double) depth);
        }
    }
}

struct CovIter : ServedRuns {      // (csrc/wt_abi_runs.h: BulkSource hdr stays first)
    WiggleIterator *child = nullptr;
    Interner names;
    RegRuns in;                     // the chromosome's intervals (no values: the depth counts them)
};

// Drains the next chromosome(s) of the child until one has a depth track (float32 holds it exactly up to a depth of 2^24);
// done when the child is exhausted.
void cov_load(ServedRuns *r) {
    CovIter *c = (CovIter *) r;
    WiggleIterator *it = c->child;
    while (!it->done) {
        c->chrom = c->names.get(it->chrom);
        c->in.clear();
        reg_drain_chrom(it, c->chrom, &c->in, false);
        const size_t n = c->in.s.size();
        for (size_t q = 0; q < n; q++)
            if (c->in.s[q] >= c->in.f[q] || (q > 0 && c->in.s[q] < c->in.s[q - 1])) {
                fprintf(stderr, "wiggletools_amd: wtamd_CoverageIterator: %s is not sorted by start, or holds an interval with start >= finish\n", c->chrom);
                exit(1);
            }
        RegRuns &o = c->out;
        if (wt_use_device((const void *) wtamd_runs_coverage_host, "WTAMD_NO_DEVICE_COVERAGE")) {
            const int64_t cap = 2 * (int64_t) n - 1;
            o.s.resize((size_t) cap); o.f.resize((size_t) cap); o.v.resize((size_t) cap);
            int64_t n_out = 0;
            if (wtamd_runs_coverage_host((int64_t) n, c->in.s.data(), c->in.f.data(), cap, o.s.data(), o.f.data(), o.v.data(), &n_out) != WTAMD_OK)
                die("wtamd_runs_coverage");
            o.s.resize((size_t) n_out); o.f.resize((size_t) n_out); o.v.resize((size_t) n_out);
        } else {
            cov_host_sweep(c->in.s, c->in.f, o.s, o.f, o.v);
        }
        if (!o.s.empty()) return;
    }
    c->done = true;
}

void cov_seek(WiggleIterator *wi, const char *chrom, int start, int finish) {
    CovIter *c = (CovIter *) (ServedRuns *) wi->data;
    seek(c->child, chrom, start, finish);
    srv_restart(c, wi);
}

}  // namespace

#endif  // WT_ABI_COVER_H_
