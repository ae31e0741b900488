// wt_abi_energy.h -- part of the DROP-IN LAYER (csrc/wt_iter_abi.cpp includes it after wt_abi_runs.h): the reference's
// EnergyIntegrator (src/statistics.c:345-391; `energy`, commandParser.c:677-681) as wtamd_EnergyIntegrator, and
// wtamd_EnergySpectrum, any number of wavelengths from one drain.  The child is drained a chromosome at a time (reg_drain_chrom:
// blocks from this library's sources and reducers, pop() otherwise); an overlapping child's chromosome goes through the
// reference's union rule (unaryOps.c:60-86) on the host first; then one call of wtamd_runs_energy_host (csrc/wt_energy.hip) with
// the running offset as the segment's base, and the chromosome's sums are added to the integrator's in genome order.
//
// The door is reached through a WEAK reference: a build of this layer without the HIP units has none and sweeps on the host by
// the same rule -- wen_host of csrc/wt_energy.h, compiled here as plain C++ --, as does WTAMD_NO_DEVICE_ENERGY=1.  A wavelength
// below 1, which the door refuses, is served by the reference's own per-position expression.
//
// Departures from the reference: positions are exact beyond 2^30 and the offset is 64-bit; the sums are correctly reduced closed
// forms, equal to the reference's to its error bound and not bit for bit; an infinite value gives NaN; one pop serves one
// chromosome, not one run (wi->finish is the last finish served either way, which is what the offset rule reads).
#ifndef WT_ABI_ENERGY_H_
#define WT_ABI_ENERGY_H_

#ifndef WT_EMU
#define WT_EMU 1
#endif
#ifndef WCV_NO_HOST
#define WCV_NO_HOST 1
#endif
#include <new>

#include "wt_energy.h"

extern "C" int wtamd_runs_energy_host(int64_t n_seg, const int64_t *seg_off, const int64_t *seg_base, const int32_t *start, const int32_t *finish,
                                      const double *value, int32_t n_wavelengths, const int32_t *wavelength, double *reim, int64_t *end_base)
    __attribute__((weak));

namespace {

struct EnergyData {
    double res;                 // must stay first: the consumer prints *(double *) wi->data (statistics.c:579)
    double real, im;            // where the reference's EnergyData has them: the sums of wavelength 0
    int wavelength;
    int chrom_offset;           // the reference's field: the offset's low 32 bits
    WiggleIterator *source;
    // what the reference has not
    bool overlaps = false;      // the source's chromosomes go through the union rule
    int64_t offset = 0;
    std::vector<int> lam;       // every wavelength served
    std::vector<double> reim;   // 2 per wavelength
    Interner names;
    RegRuns runs, merged;
};

[[noreturn]] void energy_refuse(const char *chrom) {
    fprintf(stderr, "wiggletools_amd: wtamd_EnergyIntegrator: on %s the child is not sorted, or holds an interval with start >= finish\n", chrom);
    exit(1);
}

// the reference's per-position sums (statistics.c:377-381), int arithmetic as it stands, for a wavelength the door refuses
void energy_by_position(const RegRuns &r, int chrom_offset, int wavelength, double *re, double *im) {
    const double PI = 3.141592653589793;
    for (size_t i = 0; i < r.s.size(); i++)
        for (int position = (int) ((unsigned) chrom_offset + (unsigned) r.s[i]); position < (int) ((unsigned) chrom_offset + (unsigned) r.f[i]); position++) {
            const int p2 = (int) ((0u - (unsigned) position) * 2u);
            *re += cos(p2 * PI / wavelength) * r.v[i];
            *im += sin(p2 * PI / wavelength) * r.v[i];
        }
}

// one chromosome of the source into the sums
void energy_absorb(WiggleIterator *wi, EnergyData *d) {
    WiggleIterator *src = d->source;
    const char *chrom = d->names.get(src->chrom);
    if (!wi->chrom || strcmp(wi->chrom, chrom) != 0) d->offset += wi->finish;          // statistics.c:369-370
    d->chrom_offset = (int) d->offset;
    d->runs.clear();
    reg_drain_chrom(src, chrom, &d->runs);
    const RegRuns *r = &d->runs;
    if (d->overlaps) {                                                                  // unaryOps.c:70-83
        d->merged.clear();
        for (size_t i = 0; i < r->s.size(); i++) {
            if (!d->merged.s.empty() && d->merged.f.back() > r->s[i]) { if (r->f[i] > d->merged.f.back()) d->merged.f.back() = r->f[i]; }
            else d->merged.push(r->s[i], r->f[i], r->v[i]);
        }
        r = &d->merged;
    }
    if (r->s.empty()) return;
    wi->chrom = (char *) chrom;
    wi->start = r->s.back(); wi->finish = r->f.back(); wi->value = r->v.back();
    std::vector<int32_t> good;
    std::vector<size_t> where;
    for (size_t k = 0; k < d->lam.size(); k++) {
        if (d->lam[k] >= 1) { good.push_back(d->lam[k]); where.push_back(k); }
        else energy_by_position(*r, d->chrom_offset, d->lam[k], &d->reim[2 * k], &d->reim[2 * k + 1]);
    }
    if (!good.empty()) {
        const int64_t seg[2] = {0, (int64_t) r->s.size()}, base[1] = {d->offset};
        std::vector<double> part(2 * good.size());
        int rc;
        if (wt_use_device((const void *) wtamd_runs_energy_host, "WTAMD_NO_DEVICE_ENERGY")) {
            rc = wtamd_runs_energy_host(1, seg, base, r->s.data(), r->f.data(), r->v.data(), (int32_t) good.size(), good.data(), part.data(), nullptr);
            if (rc != WTAMD_OK && rc != WTAMD_ERR_ARG) die("wtamd_runs_energy");
        } else {
            rc = wen_host(1, seg, base, r->s.data(), r->f.data(), r->v.data(), (int) good.size(), good.data(), part.data(), nullptr);
        }
        if (rc != 0) energy_refuse(chrom);
        for (size_t j = 0; j < good.size(); j++) { d->reim[2 * where[j]] += part[2 * j]; d->reim[2 * where[j] + 1] += part[2 * j + 1]; }
    }
    d->real = d->reim[0]; d->im = d->reim[1];
}

void energy_pop(WiggleIterator *wi) {
    if (wi->done) return;
    EnergyData *d = (EnergyData *) wi->data;
    if (d->source->done) {
        wi->done = 1;
        d->res = d->real * d->real + d->im * d->im;                                    // statistics.c:365
        return;
    }
    energy_absorb(wi, d);
}

void energy_seek(WiggleIterator *wi, const char *chrom, int start, int finish) {
    EnergyData *d = (EnergyData *) wi->data;
    seek(d->source, chrom, start, finish);                                              // statistics.c:354-358
    wi->done = 0;
    energy_pop(wi);
}

WiggleIterator *energy_make(WiggleIterator *child, int n, const int *wavelengths) {
    EnergyData *d = new (calloc(1, sizeof(EnergyData))) EnergyData();       // (calloc: destroyWiggleIterator frees `data`)
    d->res = NAN;
    d->real = d->im = 0.0;
    d->wavelength = wavelengths[0];
    d->chrom_offset = 0;
    d->source = child;
    d->overlaps = child->overlaps != 0;
    d->lam.assign(wavelengths, wavelengths + n);
    d->reim.assign(2 * (size_t) n, 0.0);
    WiggleIterator *wi = newWiggleIterator(d, &energy_pop, &energy_seek, child->default_value, 0);
    wi->append = child;
    return wi;
}

}  // namespace

extern "C" {

WiggleIterator *wtamd_EnergyIntegrator(WiggleIterator *child, int wavelength) { return energy_make(child, 1, &wavelength); }

int wtamd_EnergySpectrum(WiggleIterator *child, int n, const int *wavelengths, double *reim) {
    if (!child || n < 1 || n > WEN_MAX_WAVELENGTHS || !wavelengths || !reim) return WTAMD_ERR_ARG;
    WiggleIterator *wi = energy_make(child, n, wavelengths);
    while (!wi->done) wi->pop(wi);
    EnergyData *d = (EnergyData *) wi->data;
    memcpy(reim, d->reim.data(), sizeof(double) * 2 * (size_t) n);
    d->~EnergyData();
    free(d);
    free(wi);
    return WTAMD_OK;
}

double wtamd_energy_finish(const double *reim2) { return reim2[0] * reim2[0] + reim2[1] * reim2[1]; }

}  // extern "C"

#endif  // WT_ABI_ENERGY_H_
