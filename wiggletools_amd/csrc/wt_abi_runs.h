// wt_abi_runs.h -- part of the DROP-IN LAYER (csrc/wt_iter_abi.cpp includes it before wt_abi_cover.h, wt_abi_region.h,
// wt_abi_apply.h and wt_abi_profile.h): what the iterators over the run-list doors share.  A chromosome's run list drained from a
// child (RegRuns, reg_drain_chrom); the choice between a device door and the host sweep (wt_use_device); ServedRuns, a finished
// per-chromosome run list served to the library's Multiplexer in blocks, to wtamd_iterator_next_block, and to a foreign pop()
// one run at a time (wtamd_CoverageIterator, wtamd_RegionIterator); RegionMux, one region of a chromosome per popMultiplexer
// (wtamd_ApplyMultiplexer, wtamd_ProfileMultiplexer).
#ifndef WT_ABI_RUNS_H_
#define WT_ABI_RUNS_H_

namespace {

struct RegRuns {
    std::vector<int32_t> s, f;
    std::vector<double> v;
    void clear() { s.clear(); f.clear(); v.clear(); }
    void push(int32_t a, int32_t b, double x) { s.push_back(a); f.push_back(b); v.push_back(x); }
};

// the device door (a weak reference: absent in a build of this layer without the HIP units), unless <no_device_var>=1
bool wt_use_device(const void *door, const char *no_device_var) {
    const char *e = getenv(no_device_var);
    return door != nullptr && !(e && atoi(e) != 0);
}

// ---------------------------------------------------------------------------
// A finished run list per chromosome, served
// ---------------------------------------------------------------------------
struct ServedRuns {
    BulkSource hdr;                 // must stay first (see wt_bulk_pop)
    // Drains the next chromosome(s) of the children until one has a result: its interned name to `chrom`, its runs to `out`
    // (found empty); done = true when the children are exhausted.  Called once per chromosome.
    void (*load)(ServedRuns *) = nullptr;
    const char *chrom = nullptr;    // interned name of the chromosome being served
    RegRuns out;
    std::vector<float> vf;          // the values as float32 for the Multiplexer's blocks: only where f32_exact
    bool f32_exact = false;         // every value of `out` is a float32 (or NaN): decided once per load
    int64_t j = 0;
    bool done = false;
    bool block_out = false;         // wtamd_iterator_next_block handed out [j, end): the next call moves past it
};

void srv_settle(ServedRuns *c, WiggleIterator *wi) {
    if (!c->done && c->j >= (int64_t) c->out.s.size()) {
        c->out.clear(); c->vf.clear();
        c->j = 0;
        c->load(c);
        // What a consumer sees is what pop() delivers, a double.  The float32 blocks are offered only for a chromosome whose
        // values all are float32; any other goes run by run (srv_peek returns 0), or through its f64 arrays (reg_drain_chrom).
        c->vf.assign(c->out.v.begin(), c->out.v.end());
        c->f32_exact = true;
        for (size_t q = 0; q < c->vf.size() && c->f32_exact; q++) {
            const double v = c->out.v[q];
            c->f32_exact = (double) c->vf[q] == v || v != v;
        }
        if (!c->f32_exact) c->vf.clear();
    }
    if (c->done) { wi->done = 1; return; }
    wi->chrom = (char *) c->chrom;
    wi->start = c->out.s[(size_t) c->j]; wi->finish = c->out.f[(size_t) c->j];
    wi->value = c->out.v[(size_t) c->j];
}

int64_t srv_peek(BulkSource *b, const int32_t **s, const int32_t **f, const float **v) {
    ServedRuns *c = (ServedRuns *) b;
    if (c->done || c->block_out || !c->f32_exact || c->j >= (int64_t) c->out.s.size()) return 0;
    *s = c->out.s.data() + c->j; *f = c->out.f.data() + c->j; *v = c->vf.data() + c->j;
    return (int64_t) c->out.s.size() - c->j;
}

void srv_advance(BulkSource *b, WiggleIterator *wi, int64_t k) {
    ServedRuns *c = (ServedRuns *) b;
    if (c->done) { wi->done = 1; return; }
    if (c->block_out) { c->block_out = false; c->j = (int64_t) c->out.s.size(); }      // the block's runs have been taken
    else c->j += k;
    srv_settle(c, wi);
}

// after the children have been sought: nothing is held, the first element of the window is fetched
void srv_restart(ServedRuns *c, WiggleIterator *wi) {
    c->done = false;
    c->block_out = false;
    c->out.clear(); c->vf.clear();
    c->j = 0;
    wi->done = 0;
    srv_settle(c, wi);
}

// The iterator over a fresh ServedRuns (c->load set): it already holds its first element (wiggleIterator.c:32).
WiggleIterator *srv_iterator(ServedRuns *c, void (*seek_fn)(WiggleIterator *, const char *, int, int), wt_bool overlaps, double default_value) {
    c->hdr.peek = &srv_peek;
    c->hdr.advance = &srv_advance;
    c->hdr.stable = false;                     // the run list is replaced chromosome by chromosome
    WiggleIterator *wi = (WiggleIterator *) calloc(1, sizeof(WiggleIterator));
    wi->data = c;
    wi->pop = &wt_bulk_pop;
    wi->seek = seek_fn;
    wi->value = 1;
    wi->overlaps = overlaps;
    wi->default_value = default_value;
    srv_settle(c, wi);
    return wi;
}

bool srv_is(WiggleIterator *wi) { return wi && wi->pop == &wt_bulk_pop && wi->data && ((BulkSource *) wi->data)->peek == &srv_peek; }

// wtamd_iterator_next_block over a served run list: the runs from the current element to the end of its chromosome
int64_t srv_next_block(WiggleIterator *wi, const char **chrom, const int32_t **start, const int32_t **finish, const double **value) {
    ServedRuns *c = (ServedRuns *) wi->data;
    if (c->block_out) srv_advance(&c->hdr, wi, 0);
    if (wi->done) return 0;
    const int64_t n = (int64_t) c->out.s.size() - c->j;
    if (chrom) *chrom = c->chrom;
    *start = c->out.s.data() + c->j; *finish = c->out.f.data() + c->j; *value = c->out.v.data() + c->j;
    c->block_out = true;
    return n;
}

// Every interval of the chromosome `it` stands on, in blocks where it is a bulk source (a served run list: its f64 arrays, the
// doubles its pop() delivers); keep == NULL: skipped; values: false leaves keep->v alone.
void reg_drain_chrom(WiggleIterator *it, const char *chrom, RegRuns *keep, bool values = true) {
    BulkSource *bulk = it->pop == &wt_bulk_pop ? (BulkSource *) it->data : nullptr;
    ServedRuns *served = srv_is(it) ? (ServedRuns *) it->data : nullptr;
    while (!it->done && strcmp(it->chrom, chrom) == 0) {
        if (served && !served->block_out && served->j < (int64_t) served->out.s.size()) {
            const RegRuns &o = served->out;
            const int64_t cnt = (int64_t) o.s.size() - served->j;
            if (keep) {
                keep->s.insert(keep->s.end(), o.s.begin() + served->j, o.s.end());
                keep->f.insert(keep->f.end(), o.f.begin() + served->j, o.f.end());
                if (values) keep->v.insert(keep->v.end(), o.v.begin() + served->j, o.v.end());
            }
            srv_advance(&served->hdr, it, cnt);
            continue;
        }
        const int32_t *bs, *bf;
        const float *bv;
        const int64_t cnt = bulk ? bulk->peek(bulk, &bs, &bf, &bv) : 0;
        if (cnt > 0) {
            if (keep) {
                keep->s.insert(keep->s.end(), bs, bs + cnt);
                keep->f.insert(keep->f.end(), bf, bf + cnt);
                if (values) keep->v.insert(keep->v.end(), bv, bv + cnt);
            }
            bulk->advance(bulk, it, cnt);
        } else {
            if (keep) {
                keep->s.push_back(it->start); keep->f.push_back(it->finish);
                if (values) keep->v.push_back(it->value);
            }
            it->pop(it);
        }
    }
}

// ---------------------------------------------------------------------------
// One region of a chromosome per popMultiplexer
// ---------------------------------------------------------------------------
struct RegionMux {
    const char *name;               // "Apply" / "Profile": the reference's multiplexer this one stands for, for the messages
    WiggleIterator *regions = nullptr, *dataset = nullptr;
    Interner names;
    const char *chrom = nullptr;    // interned name of the chromosome being served
    RegRuns reg, dat;
    std::vector<double> res;        // the door's output for the regions of the chromosome
    size_t j = 0;                   // the next region to serve
    explicit RegionMux(const char *name_) : name(name_) {}
};

void rmx_seek(Multiplexer *m, const char *chrom, int start, int finish) {
    RegionMux *a = (RegionMux *) m->data;
    seek(a->regions, chrom, start, finish);
    seek(a->dataset, chrom, start, finish);
    a->reg.clear(); a->dat.clear(); a->res.clear();
    a->j = 0;
    m->done = 0;
    m->pop(m);
}

[[noreturn]] void rmx_refuse(const RegionMux *a) {
    fprintf(stderr, "wiggletools_amd: wtamd_%sMultiplexer: on %s the dataset overlaps itself, or a side is not sorted by start or holds an "
                    "interval with start >= finish; keep the reference's %sMultiplexer for such input\n", a->name, a->chrom, a->name);
    exit(1);
}

}  // namespace

#endif  // WT_ABI_RUNS_H_
