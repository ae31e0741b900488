// wt_abi_profile.h -- part of the DROP-IN LAYER (csrc/wt_iter_abi.cpp includes it after wt_abi_apply.h): the reference's
// ProfileMultiplexer (src/apply.c:355-366; the parser's `profile` / `profiles`) as wtamd_ProfileMultiplexer(regions, width,
// dataset).  It drains regions and dataset one chromosome at a time with the code of wt_abi_apply.h (apm_drain_pair: blocks
// from this library's sources and reducers, pop() otherwise; chromosomes paired by name in strcmp order), computes the rows of
// the chromosome's regions through the device door (wtamd_runs_profile_host, csrc/wt_profile.hip) and serves one region per
// popMultiplexer: values = the region's `width` bins.
//
// The door is reached through a WEAK reference: a build of this layer without the HIP units has no door and sweeps on the host
// by the same rules -- wpr_profile_host of csrc/wt_profile.h, compiled here as plain C++ (the same bits) --, as does
// WTAMD_NO_DEVICE_PROFILE=1.
//
// Refused with a message and exit(1), as wtamd_ApplyMultiplexer does: a dataset with `overlaps` set or one that turns out not
// to be disjoint, regions that are not sorted; and width < 1.
#ifndef WT_ABI_PROFILE_H_
#define WT_ABI_PROFILE_H_

#include "wt_abi_apply.h"
#include "wt_profile.h"

extern "C" int wtamd_runs_profile_host(int64_t n, const int32_t *start, const int32_t *finish, const double *value, int64_t n_regions,
                                       const int32_t *r_start, const int32_t *r_finish, int32_t width, double default_value, uint32_t flags,
                                       double *profile) __attribute__((weak));

namespace {

struct ProfileMux {
    WiggleIterator *regions = nullptr, *dataset = nullptr;
    int width = 1;
    Interner names;
    const char *chrom = nullptr;    // interned name of the chromosome being served
    RegRuns reg, dat;
    std::vector<double> rows;       // width per region of the chromosome
    size_t j = 0;                   // the next region to serve
};

bool prm_use_device() {
    const char *e = getenv("WTAMD_NO_DEVICE_PROFILE");
    return wtamd_runs_profile_host != nullptr && !(e && atoi(e) != 0);
}

bool prm_load(ProfileMux *a) {
    WiggleIterator *dat = a->dataset;
    a->rows.clear();
    a->j = 0;
    if (!apm_drain_pair(a->regions, dat, a->names, &a->chrom, &a->reg, &a->dat)) return false;
    const size_t n = a->dat.s.size(), m = a->reg.s.size();
    a->rows.resize(m * (size_t) a->width);
    int rc;
    if (prm_use_device()) {
        rc = wtamd_runs_profile_host((int64_t) n, a->dat.s.data(), a->dat.f.data(), a->dat.v.data(), (int64_t) m, a->reg.s.data(), a->reg.f.data(),
                                     (int32_t) a->width, dat->default_value, 0u, a->rows.data());
        if (rc != WTAMD_OK && rc != WTAMD_ERR_ARG) die("wtamd_runs_profile");
    } else {
        rc = wpr_profile_host((long long) n, a->dat.s.data(), a->dat.f.data(), a->dat.v.data(), (long long) m, a->reg.s.data(), a->reg.f.data(),
                              (long long) a->width, dat->default_value, 0u, a->rows.data());
    }
    if (rc != 0) {
        fprintf(stderr, "wiggletools_amd: wtamd_ProfileMultiplexer: on %s the dataset overlaps itself, or a side is not sorted by start or holds an "
                        "interval with start >= finish; keep the reference's ProfileMultiplexer for such input\n", a->chrom);
        exit(1);
    }
    return true;
}

void prm_pop(Multiplexer *m) {
    ProfileMux *a = (ProfileMux *) m->data;
    if (a->j >= a->reg.s.size() && !prm_load(a)) { m->done = 1; return; }
    m->chrom = (char *) a->chrom;
    m->start = a->reg.s[a->j]; m->finish = a->reg.f[a->j];
    memcpy(m->values, a->rows.data() + a->j * (size_t) a->width, sizeof(double) * (size_t) a->width);
    a->j++;
}

void prm_seek(Multiplexer *m, const char *chrom, int start, int finish) {
    ProfileMux *a = (ProfileMux *) m->data;
    seek(a->regions, chrom, start, finish);
    seek(a->dataset, chrom, start, finish);
    a->reg.clear(); a->dat.clear(); a->rows.clear();
    a->j = 0;
    m->done = 0;
    prm_pop(m);
}

}  // namespace

#endif  // WT_ABI_PROFILE_H_
