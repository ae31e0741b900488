// wt_abi_apply.h -- part of the DROP-IN LAYER (csrc/wt_iter_abi.cpp includes it): the reference's ApplyMultiplexer
// (src/apply.c:293-353; the parser's `apply` / `apply_paste`) as wtamd_ApplyMultiplexer(regions, stats, count, dataset,
// strict).  It drains regions and dataset one chromosome at a time -- in blocks where the child is a bulk source of this
// library or one of its reducers (wtamd_iterator_next_block), by pop() otherwise --, pairs chromosomes by name in strcmp
// order, computes six moments per region of the chromosome through the device door (wtamd_runs_apply_host,
// csrc/wt_apply.hip) and serves one region per popMultiplexer: values[i] = wtamd_apply_finish(m6, stats[i]).
//
// The door is reached through a WEAK reference: a build of this layer without the HIP units (the emulated drop-in library of
// the CPU tests) has no door and sweeps on the host by the same rules -- wap_apply_host of csrc/wt_apply.h, compiled here as
// plain C++ --, as does WTAMD_NO_DEVICE_APPLY=1.
//
// Refused with a message and exit(1): a dataset with `overlaps` set or one that turns out not to be disjoint, regions that are
// not sorted, an unknown statistic.  Such callers keep the reference's ApplyMultiplexer.
#ifndef WT_ABI_APPLY_H_
#define WT_ABI_APPLY_H_

// the arithmetic of csrc/wt_apply.h as plain C++ (its passes and its door are not needed here)
#ifndef WT_EMU
#define WT_EMU 1
#endif
#ifndef WCV_NO_HOST
#define WCV_NO_HOST 1
#endif
#include "wt_apply.h"

extern "C" int wtamd_runs_apply_host(int64_t n, const int32_t *start, const int32_t *finish, const double *value, int64_t n_regions,
                                     const int32_t *r_start, const int32_t *r_finish, double default_value, uint32_t flags,
                                     double *moments6) __attribute__((weak));

namespace {

struct ApplyMux : RegionMux {       // (csrc/wt_abi_runs.h; res: 6 moments per region of the chromosome)
    std::vector<int> stats;
    bool strict = true;
    ApplyMux() : RegionMux("Apply") {}
};

// Every interval of the chromosome `it` stands on: whole batches of a reducer of this library, blocks of a bulk source,
// pop() for anything else; keep == NULL: skipped.
void apm_drain_chrom(WiggleIterator *it, const char *chrom, RegRuns *keep) {
    if (it->pop == &red_pop) {
        while (!it->done && strcmp(it->chrom, chrom) == 0) {
            const int32_t *bs, *bf;
            const double *bv;
            const int64_t cnt = wtamd_iterator_next_block(it, nullptr, &bs, &bf, &bv);
            if (cnt <= 0) break;
            if (keep) {
                keep->s.insert(keep->s.end(), bs, bs + cnt);
                keep->f.insert(keep->f.end(), bf, bf + cnt);
                keep->v.insert(keep->v.end(), bv, bv + cnt);
            }
            it->pop(it);                    // the first element of the next batch
        }
        return;
    }
    reg_drain_chrom(it, chrom, keep);
}

// Drains the next chromosome of the regions and the dataset's chromosome of the same name (wt_abi_profile.h shares it); false
// when there is none.
bool apm_drain_pair(WiggleIterator *reg, WiggleIterator *dat, Interner &names, const char **chrom, RegRuns *reg_runs, RegRuns *dat_runs) {
    reg_runs->clear(); dat_runs->clear();
    if (reg->done) return false;
    *chrom = names.get(reg->chrom);
    apm_drain_chrom(reg, *chrom, reg_runs);
    while (!dat->done && strcmp(dat->chrom, *chrom) < 0) {                  // chromosomes only the dataset has
        const char *skip = names.get(dat->chrom);
        apm_drain_chrom(dat, skip, nullptr);
    }
    if (!dat->done && strcmp(dat->chrom, *chrom) == 0) apm_drain_chrom(dat, *chrom, dat_runs);
    return true;
}

bool apm_load(ApplyMux *a) {
    WiggleIterator *dat = a->dataset;
    a->res.clear();
    a->j = 0;
    if (!apm_drain_pair(a->regions, dat, a->names, &a->chrom, &a->reg, &a->dat)) return false;
    const size_t n = a->dat.s.size(), m = a->reg.s.size();
    a->res.resize(6 * m);
    const uint32_t flags = a->strict ? WTAMD_APPLY_STRICT : 0u;
    int rc;
    if (wt_use_device((const void *) wtamd_runs_apply_host, "WTAMD_NO_DEVICE_APPLY")) {
        rc = wtamd_runs_apply_host((int64_t) n, a->dat.s.data(), a->dat.f.data(), a->dat.v.data(), (int64_t) m, a->reg.s.data(), a->reg.f.data(),
                                   dat->default_value, flags, a->res.data());
        if (rc != WTAMD_OK && rc != WTAMD_ERR_ARG) die("wtamd_runs_apply");
    } else {
        rc = wap_apply_host((long long) n, a->dat.s.data(), a->dat.f.data(), a->dat.v.data(), (long long) m, a->reg.s.data(), a->reg.f.data(),
                            dat->default_value, flags, a->res.data());
    }
    if (rc != 0) rmx_refuse(a);
    return true;
}

void apm_pop(Multiplexer *m) {
    ApplyMux *a = (ApplyMux *) (RegionMux *) m->data;
    if (a->j >= a->reg.s.size() && !apm_load(a)) { m->done = 1; return; }
    m->chrom = (char *) a->chrom;
    m->start = a->reg.s[a->j]; m->finish = a->reg.f[a->j];
    for (int i = 0; i < m->count; i++) m->values[i] = wtamd_apply_finish(a->res.data() + 6 * a->j, a->stats[(size_t) i]);
    a->j++;
}

}  // namespace

#endif  // WT_ABI_APPLY_H_
