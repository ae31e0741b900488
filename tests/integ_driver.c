/* integ_driver.c -- drives a genome-wide integrator of ONE library that exports the WiggleTools iterator C API: the
 * compiled reference (VarianceIntegrator, MaxIntegrator, ...), this project's library or its emulated drop-in
 * (wtamd_VarianceIntegrator, ...).  Everything is looked up by name, so one driver serves the three.
 *
 * The library is opened RTLD_LAZY | RTLD_LOCAL: the compiled reference leaves the symbols of its file readers
 * unresolved on purpose, and the tested libraries export the same unprefixed names (pop, seek, ...).
 *
 * The children are array-backed iterators over the [chromosome][track] layout the tests use everywhere
 * (seg_off[c * n_tracks + i] .. seg_off[c * n_tracks + i + 1]); every pop loop is capped, so an integrator that
 * stops advancing its source returns an error instead of spinning. */
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "wiggletools_amd.h"

typedef struct {
    int32_t n_chrom, n_tracks;
    const int64_t *seg_off;
    const int32_t *start, *finish;
    const double *value;
    const double *defaults;
} idrv_tracks;

typedef struct {
    void *lib;
    WiggleIterator *(*new_iter)(void *, void (*)(WiggleIterator *), void (*)(WiggleIterator *, const char *, int, int), double, wt_bool);
    Multiplexer *(*new_mux)(WiggleIterator **, int, wt_bool);
    void (*pop)(WiggleIterator *);
    void (*seek)(WiggleIterator *, const char *, int, int);
    int (*pipe_stats)(WiggleIterator *, wtamd_pipe_stats *);    /* NULL in the compiled reference */
} idrv;

void *idrv_open(const char *path) {
    idrv *d = (idrv *) calloc(1, sizeof(idrv));
    d->lib = dlopen(path, RTLD_LAZY | RTLD_LOCAL);
    if (!d->lib) { fprintf(stderr, "integ_driver: %s\n", dlerror()); free(d); return NULL; }
    *(void **) &d->new_iter = dlsym(d->lib, "newWiggleIterator");
    *(void **) &d->new_mux = dlsym(d->lib, "newMultiplexer");
    *(void **) &d->pop = dlsym(d->lib, "pop");
    *(void **) &d->seek = dlsym(d->lib, "seek");
    *(void **) &d->pipe_stats = dlsym(d->lib, "wtamd_iterator_pipe_stats");
    if (!d->new_iter || !d->new_mux || !d->pop || !d->seek) { free(d); return NULL; }
    return d;
}

/* ---- one track as an iterator ---- */
typedef struct {
    const idrv_tracks *t;
    char **names;
    int track, chrom;
    int64_t next;                   /* next interval of (chrom, track), -1: at the segment's beginning */
    int windowed, lo, hi;           /* after a seek: only `chrom`, clipped to [lo, hi) */
} child;

static void child_pop(WiggleIterator *wi) {
    child *c = (child *) wi->data;
    const idrv_tracks *t = c->t;
    while (c->chrom < t->n_chrom) {
        const int64_t seg = (int64_t) c->chrom * t->n_tracks + c->track;
        if (c->next < t->seg_off[seg]) c->next = t->seg_off[seg];
        if (c->next >= t->seg_off[seg + 1]) {
            if (c->windowed) break;
            c->chrom++; c->next = -1;
            continue;
        }
        const int64_t j = c->next++;
        int s = t->start[j], f = t->finish[j];
        if (c->windowed) {
            if (f <= c->lo) continue;
            if (s >= c->hi) break;
            if (s < c->lo) s = c->lo;
            if (f > c->hi) f = c->hi;
        }
        wi->chrom = c->names[c->chrom]; wi->start = s; wi->finish = f; wi->value = t->value[j];
        return;
    }
    wi->done = 1;
}

static void child_seek(WiggleIterator *wi, const char *chrom, int start, int finish) {
    child *c = (child *) wi->data;
    c->windowed = 1; c->lo = start; c->hi = finish; c->next = -1;
    c->chrom = c->t->n_chrom;
    for (int k = 0; k < c->t->n_chrom; k++)
        if (!strcmp(c->names[k], chrom)) c->chrom = k;
    wi->done = 0;
    child_pop(wi);
}

typedef struct {
    WiggleIterator *reducer, *integ;
    char **names;
    int64_t cap;                    /* pops allowed in all */
} chain;

static int build(idrv *d, const idrv_tracks *t, const char *reducer, int strict, const char *integrator, chain *out) {
    WiggleIterator *(*red)(Multiplexer *);
    WiggleIterator *(*integ)(WiggleIterator *);
    *(void **) &red = dlsym(d->lib, reducer);
    *(void **) &integ = dlsym(d->lib, integrator);
    if (!red || !integ) return -2;
    out->names = (char **) calloc((size_t) t->n_chrom + 1, sizeof(char *));
    for (int c = 0; c < t->n_chrom; c++) {
        out->names[c] = (char *) malloc(16);
        snprintf(out->names[c], 16, "k%06d", c);            /* sorted by name == sorted by index */
    }
    WiggleIterator **kids = (WiggleIterator **) calloc((size_t) t->n_tracks, sizeof(WiggleIterator *));
    for (int i = 0; i < t->n_tracks; i++) {
        child *c = (child *) calloc(1, sizeof(child));
        c->t = t; c->names = out->names; c->track = i; c->next = -1;
        kids[i] = d->new_iter(c, child_pop, child_seek, t->defaults[i], 0);
    }
    Multiplexer *m = d->new_mux(kids, t->n_tracks, (wt_bool) (strict != 0));
    out->reducer = red(m);
    out->integ = integ(out->reducer);
    out->cap = 4 * (t->seg_off[(int64_t) t->n_chrom * t->n_tracks] + 16);
    return 0;
}

/* pops to the end; < 0 past the cap */
static int64_t drain(idrv *d, chain *c) {
    int64_t pops = 0;
    while (!c->integ->done) {
        if (pops >= c->cap) return -1;
        d->pop(c->integ);
        pops++;
    }
    c->cap -= pops;
    return pops;
}

/* info[0] pops, info[1] bytes device -> host, info[2] runs the reducer computed (-1 where the library keeps no counters).
 * Returns 0, -2 for a missing symbol, -4 when the integrator was still not done at the cap. */
int idrv_run(void *h, const idrv_tracks *t, const char *reducer, int strict, const char *integrator, double *result, int64_t *info) {
    idrv *d = (idrv *) h;
    chain c;
    info[0] = info[1] = info[2] = -1;
    const int rc = build(d, t, reducer, strict, integrator, &c);
    if (rc) return rc;
    info[0] = drain(d, &c);
    *result = *(double *) c.integ->data;
    if (info[0] < 0) return -4;
    wtamd_pipe_stats st;
    memset(&st, 0, sizeof st);
    if (d->pipe_stats && d->pipe_stats(c.reducer, &st) == 0) { info[1] = st.d2h_bytes; info[2] = st.runs; }
    return 0;
}

/* pre_pops pops, then per region (chromosome index, start, finish): seek, pop to the end.  out[0]: the value before the
 * first seek, out[1 + k]: after region k. */
int idrv_run_seek(void *h, const idrv_tracks *t, const char *reducer, int strict, const char *integrator, int pre_pops,
                  int n_regions, const int32_t *regions, double *out) {
    idrv *d = (idrv *) h;
    chain c;
    const int rc = build(d, t, reducer, strict, integrator, &c);
    if (rc) return rc;
    c.cap *= 1 + n_regions;
    for (int k = 0; k < pre_pops && !c.integ->done; k++) d->pop(c.integ);
    out[0] = *(double *) c.integ->data;
    for (int k = 0; k < n_regions; k++) {
        d->seek(c.integ, c.names[regions[3 * k]], regions[3 * k + 1], regions[3 * k + 2]);
        if (drain(d, &c) < 0) return -4;
        out[1 + k] = *(double *) c.integ->data;
    }
    return 0;
}
