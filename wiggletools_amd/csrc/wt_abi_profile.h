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

struct ProfileMux : RegionMux {     // (csrc/wt_abi_runs.h; res: width bins per region of the chromosome)
    int width = 1;
    ProfileMux() : RegionMux("Profile") {}
};

bool prm_load(ProfileMux *a) {
    WiggleIterator *dat = a->dataset;
    a->res.clear();
    a->j = 0;
    if (!apm_drain_pair(a->regions, dat, a->names, &a->chrom, &a->reg, &a->dat)) return false;
    const size_t n = a->dat.s.size(), m = a->reg.s.size();
    a->res.resize(m * (size_t) a->width);
    int rc;
    if (wt_use_device((const void *) wtamd_runs_profile_host, "WTAMD_NO_DEVICE_PROFILE")) {
        rc = wtamd_runs_profile_host((int64_t) n, a->dat.s.data(), a->dat.f.data(), a->dat.v.data(), (int64_t) m, a->reg.s.data(), a->reg.f.data(),
                                     (int32_t) a->width, dat->default_value, 0u, a->res.data());
        if (rc != WTAMD_OK && rc != WTAMD_ERR_ARG) die("wtamd_runs_profile");
    } else {
        rc = wpr_profile_host((long long) n, a->dat.s.data(), a->dat.f.data(), a->dat.v.data(), (long long) m, a->reg.s.data(), a->reg.f.data(),
                              (long long) a->width, dat->default_value, 0u, a->res.data());
    }
    if (rc != 0) rmx_refuse(a);
    return true;
}

void prm_pop(Multiplexer *m) {
    ProfileMux *a = (ProfileMux *) (RegionMux *) m->data;
    if (a->j >= a->reg.s.size() && !prm_load(a)) { m->done = 1; return; }
    m->chrom = (char *) a->chrom;
    m->start = a->reg.s[a->j]; m->finish = a->reg.f[a->j];
    memcpy(m->values, a->res.data() + a->j * (size_t) a->width, sizeof(double) * (size_t) a->width);
    a->j++;
}

}  // namespace

#endif  // WT_ABI_PROFILE_H_
