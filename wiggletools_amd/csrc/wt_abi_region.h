// wt_abi_region.h -- part of the DROP-IN LAYER (csrc/wt_iter_abi.cpp includes it; one translation unit, one anonymous
// namespace): the reference's region operators OverlapWiggleIterator, NoverlapWiggleIterator, TrimWiggleIterator and
// NearestWiggleIterator (src/unaryOps.c:437-639; the parser's `overlaps`, `noverlaps`, `trim`, `nearest`,
// commandParser.c:813-819) as ONE bulk source, wtamd_RegionIterator(op, source, mask).  It drains source and mask one
// chromosome at a time (in blocks where the child is a bulk source of this library), pairs chromosomes by name in strcmp
// order as the reference does, computes the chromosome's result through the device door (wtamd_runs_region, csrc/wt_region.hip)
// and serves the finished run list as a ServedRuns (csrc/wt_abi_runs.h).
//
// The door is reached through a WEAK reference: a build of this layer without the HIP units (the emulated drop-in library of
// the CPU tests) has no door and sweeps on the host by the same rules (csrc/wt_region.h), as does WTAMD_NO_DEVICE_REGION=1.
// Either way the result is the same list.
//
// One combination never goes to the door: a trim whose SOURCE overlaps itself.  What the reference puts out then depends on
// the order of its pops (it loses intersections), so the door refuses such a source and this iterator follows the
// reference's own per-interval protocol on the host.
#ifndef WT_ABI_REGION_H_
#define WT_ABI_REGION_H_

extern "C" int wtamd_runs_region_host(int op, int64_t n, const int32_t *start, const int32_t *finish, const double *value, int64_t m,
                                      const int32_t *m_start, const int32_t *m_finish, int64_t capacity, int32_t *o_start,
                                      int32_t *o_finish, double *o_value, int64_t *n_out) __attribute__((weak));

namespace {

// the union of a mask sorted by start: an interval joins the group while group.finish > start (touching ones stay apart)
void reg_union(const RegRuns &m, std::vector<int32_t> &gs, std::vector<int32_t> &gf) {
    for (size_t k = 0; k < m.s.size(); k++) {
        if (gs.empty() || m.s[k] >= gf.back()) { gs.push_back(m.s[k]); gf.push_back(m.f[k]); }
        else if (m.f[k] > gf.back()) gf.back() = m.f[k];
    }
}

// The rules of csrc/wt_region.h over one chromosome, on the host.
void reg_host_sweep(int op, const RegRuns &src, const RegRuns &mask, RegRuns &out) {
    const size_t n = src.s.size(), m = mask.s.size();
    if (op == WTAMD_REGION_NEAREST) {
        size_t k = 0;                       // masks with start <= the run's start (starts are sorted on both sides)
        for (size_t i = 0; i < n; i++) {
            while (k < m && mask.s[k] <= src.s[i]) k++;
            bool set = false;
            int32_t best = 0;
            if (k > 0) { best = (int32_t) ((uint32_t) src.s[i] - (uint32_t) mask.f[k - 1] + 1u); set = true; }
            if (k < m) {
                const int32_t c = (int32_t) ((uint32_t) mask.s[k] - (uint32_t) src.f[i] + 1u);
                if (!set || best > c) best = c;
                set = true;
            }
            out.push(src.s[i], src.f[i], !set ? (double) NAN : best < 0 ? 0.0 : (double) best);
        }
        return;
    }
    std::vector<int32_t> gs, gf;
    reg_union(mask, gs, gf);
    size_t lo = 0;                          // the first group with finish > the run's start
    for (size_t i = 0; i < n; i++) {
        while (lo < gs.size() && gf[lo] <= src.s[i]) lo++;
        size_t hi = lo;                     // the first group with start >= the run's finish (finishes need not be sorted)
        while (hi < gs.size() && gs[hi] < src.f[i]) hi++;
        if (op == WTAMD_REGION_TRIM) {
            for (size_t g = lo; g < hi; g++) out.push(std::max(src.s[i], gs[g]), std::min(src.f[i], gf[g]), src.v[i]);
        } else if ((op == WTAMD_REGION_OVERLAPS) == (hi > lo)) {
            out.push(src.s[i], src.f[i], src.v[i]);
        }
    }
}

// TrimWiggleIterator's pops (unaryOps.c:485-516) over one chromosome: after an output, whichever side ends first moves on.
void reg_trim_protocol(const RegRuns &src, const RegRuns &mask, RegRuns &out) {
    std::vector<int32_t> gs, gf;
    reg_union(mask, gs, gf);
    size_t i = 0, g = 0;
    while (i < src.s.size() && g < gs.size()) {
        if (gf[g] <= src.s[i]) g++;
        else if (src.f[i] <= gs[g]) i++;
        else {
            out.push(std::max(src.s[i], gs[g]), std::min(src.f[i], gf[g]), src.v[i]);
            if (src.f[i] <= gf[g]) i++; else g++;
        }
    }
}

struct RegIter : ServedRuns {      // (csrc/wt_abi_runs.h: BulkSource hdr stays first)
    int op = 0;
    WiggleIterator *source = nullptr, *mask = nullptr;
    Interner names;
    RegRuns in, msk;
};

void reg_check_sorted(const RegRuns &r, const char *chrom, const char *side) {
    for (size_t q = 0; q < r.s.size(); q++)
        if (r.s[q] >= r.f[q] || (q > 0 && r.s[q] < r.s[q - 1])) {
            fprintf(stderr, "wiggletools_amd: wtamd_RegionIterator: the %s's %s is not sorted by start, or holds an interval with start >= finish\n", side, chrom);
            exit(1);
        }
}

// Drains the next chromosome(s) of the source, with the mask's chromosome of the same name, until one has a result.
void reg_load(ServedRuns *r) {
    RegIter *c = (RegIter *) r;
    WiggleIterator *src = c->source, *mask = c->mask;
    while (!src->done) {
        // the reference ends an overlaps / trim with its mask (unaryOps.c:456, :504)
        if (mask->done && (c->op == WTAMD_REGION_OVERLAPS || c->op == WTAMD_REGION_TRIM)) break;
        c->chrom = c->names.get(src->chrom);
        while (!mask->done && strcmp(mask->chrom, c->chrom) < 0) {           // chromosomes only the mask has
            const char *skip = c->names.get(mask->chrom);
            reg_drain_chrom(mask, skip, nullptr);
        }
        c->in.clear(); c->msk.clear();
        reg_drain_chrom(src, c->chrom, &c->in);
        if (!mask->done && strcmp(mask->chrom, c->chrom) == 0) reg_drain_chrom(mask, c->chrom, &c->msk);
        reg_check_sorted(c->in, c->chrom, "source");
        reg_check_sorted(c->msk, c->chrom, "mask");
        const size_t n = c->in.s.size(), m = c->msk.s.size();
        bool disjoint = true;
        for (size_t q = 1; q < n && disjoint; q++) disjoint = c->in.s[q] >= c->in.f[q - 1];
        if (c->op == WTAMD_REGION_TRIM && !disjoint) {
            reg_trim_protocol(c->in, c->msk, c->out);
        } else if (wt_use_device((const void *) wtamd_runs_region_host, "WTAMD_NO_DEVICE_REGION")) {
            const int64_t cap = (int64_t) (c->op == WTAMD_REGION_TRIM ? n + m : n);
            c->out.s.resize((size_t) cap); c->out.f.resize((size_t) cap); c->out.v.resize((size_t) cap);
            int64_t n_out = 0;
            if (wtamd_runs_region_host(c->op, (int64_t) n, c->in.s.data(), c->in.f.data(), c->in.v.data(), (int64_t) m, c->msk.s.data(),
                                       c->msk.f.data(), cap, c->out.s.data(), c->out.f.data(), c->out.v.data(), &n_out) != WTAMD_OK)
                die("wtamd_runs_region");
            c->out.s.resize((size_t) n_out); c->out.f.resize((size_t) n_out); c->out.v.resize((size_t) n_out);
        } else {
            reg_host_sweep(c->op, c->in, c->msk, c->out);
        }
        if (!c->out.s.empty()) return;
    }
    c->done = true;
}

void reg_seek(WiggleIterator *wi, const char *chrom, int start, int finish) {
    RegIter *c = (RegIter *) (ServedRuns *) wi->data;
    seek(c->source, chrom, start, finish);
    seek(c->mask, chrom, start, finish);
    srv_restart(c, wi);
}

}  // namespace

#endif  // WT_ABI_REGION_H_
