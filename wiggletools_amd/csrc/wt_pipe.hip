// wt_pipe.hip -- the streaming pipeline's unit: the gather and export kernels, every wtamd_pipe_* entry and
// wtamd_host_* (overview: wt_pipe.h; the pools themselves and wtamd_pool_*: wt_pool.hip).  The kernels of a batch are the engine's and the side
// units': this file stages, orders and ships.  Compiled only by hipcc --offload-arch=gfx950.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "wt_host.h"
#include "wt_trackset.h"
#include "wt_core.h"
#include "wt_plan.h"
#include "wt_bwdev_core.h"
#include "wt_pipe.h"
#include "wt_pool.h"

__global__ void __launch_bounds__(256) wt_gather_kernel(const WtGatherSeg *segs, int n_segs, long long n_chunks,
                                                         int32_t *d_start, int32_t *d_finish, float *d_value) {
    // the table lies in pinned HOST memory: every block pulls it into LDS once (one coalesced read
    // through the link) instead of a separate H2D copy ahead of the launch
    __shared__ WtGatherSeg tab[WT_GATHER_MAX_SEGS];
    {
        const long long *src = (const long long *) segs;
        long long *dst = (long long *) tab;
        const int words = n_segs * (int) (sizeof(WtGatherSeg) / 8);
        for (int i = threadIdx.x; i < words; i += 256) dst[i] = __builtin_nontemporal_load(src + i);
    }
    __syncthreads();
    for (long long ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
        int lo = 0, hi = n_segs - 1;                    // last segment with chunk_first <= ch
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (tab[mid].chunk_first <= ch) lo = mid; else hi = mid - 1;
        }
        const WtGatherSeg g = tab[lo];
        const long long a = (ch - g.chunk_first) * WT_GATHER_CHUNK;
        long long b = a + WT_GATHER_CHUNK;
        if (b > g.count) b = g.count;
        // issue every load of the chunk before the first store: the link's latency is microseconds
        int32_t vs[WT_GATHER_CHUNK / 256], vf[WT_GATHER_CHUNK / 256];
        float vv[WT_GATHER_CHUNK / 256];
#pragma unroll
        for (int q = 0; q < WT_GATHER_CHUNK / 256; q++) {
            const long long i = a + threadIdx.x + 256ll * q;
            if (i < b) { vs[q] = __builtin_nontemporal_load(g.start + i); vf[q] = __builtin_nontemporal_load(g.finish + i); vv[q] = __builtin_nontemporal_load(g.value + i); }
        }
#pragma unroll
        for (int q = 0; q < WT_GATHER_CHUNK / 256; q++) {
            const long long i = a + threadIdx.x + 256ll * q;
            if (i < b) { d_start[g.dst + i] = vs[q]; d_finish[g.dst + i] = vf[q]; d_value[g.dst + i] = vv[q]; }
        }
    }
}

// Export: the emitted runs (their count is read on the device) and the launch counters go to the
// slot's PINNED host output, written through the link by the kernel itself.
#define WT_CTR_EXPORTED 6            // h_counters slot: runs the export kernel shipped (== WT_CTR_RUNS unless compressed)
__global__ void __launch_bounds__(256) wt_export_kernel(const unsigned long long *d_counters, unsigned long long *h_counters,
                                                         const unsigned long long *n_src, long long capacity, int n_tracks,
                                                         const int32_t *d_os, const int32_t *d_of, const double *d_ov,
                                                         const double *d_tile, const uint8_t *d_ip,
                                                         int32_t *h_os, int32_t *h_of, double *h_ov, double *h_tile, uint8_t *h_ip) {
    long long n = (long long) *n_src;
    if (n > capacity) n = capacity;
    const long long stride = (long long) gridDim.x * 256, t = (long long) blockIdx.x * 256 + threadIdx.x;
    {   // coordinates: 16 bytes per lane
        const long long n4 = n >> 2;
        const int4 *a = (const int4 *) d_os, *b = (const int4 *) d_of;
        int4 *ha = (int4 *) h_os, *hb = (int4 *) h_of;
        for (long long i = t; i < n4; i += stride) { ha[i] = a[i]; hb[i] = b[i]; }
        for (long long i = (n4 << 2) + t; i < n; i += stride) { h_os[i] = d_os[i]; h_of[i] = d_of[i]; }
        const long long n2 = n >> 1;
        const double2 *v = (const double2 *) d_ov;
        double2 *hv = (double2 *) h_ov;
        for (long long i = t; i < n2; i += stride) hv[i] = v[i];
        if (t == 0 && (n & 1)) h_ov[n - 1] = d_ov[n - 1];
    }
    if (d_tile) {
        const long long m = n * n_tracks;
        for (long long i = t; i < m; i += stride) { h_tile[i] = d_tile[i]; h_ip[i] = d_ip[i]; }
    }
    if (t < WT_CTR_N) h_counters[t] = t == WT_CTR_EXPORTED ? (unsigned long long) n : d_counters[t];
}

static void wt_slot_free(WtSlot &s) {
    if (s.h_seg) wt_host_free(s.h_seg);
    if (s.h_start) wt_host_free(s.h_start);
    if (s.h_finish) wt_host_free(s.h_finish);
    if (s.h_v32) wt_host_free(s.h_v32);
    if (s.h_v64) wt_host_free(s.h_v64);
    (void) wt_dev_free(s.d_start); (void) wt_dev_free(s.d_finish); (void) wt_dev_free(s.d_value);
    (void) wt_dev_free(s.d_os); (void) wt_dev_free(s.d_of); (void) wt_dev_free(s.d_ov); (void) wt_dev_free(s.d_tile); (void) wt_dev_free(s.d_ip);
    (void) wt_dev_free(s.d_cro);
    (void) wt_dev_free(s.d_cs); (void) wt_dev_free(s.d_cf); (void) wt_dev_free(s.d_cv); (void) wt_dev_free(s.d_cscratch); (void) wt_dev_free(s.d_cn);
    if (s.h_segs) wt_host_free(s.h_segs);
    (void) wt_dev_free(s.d_mstart); (void) wt_dev_free(s.d_mfinish); (void) wt_dev_free(s.d_mvalue); (void) wt_dev_free(s.d_mseg); (void) wt_dev_free(s.d_mscratch);
    if (s.h_os) wt_host_free(s.h_os);
    if (s.h_of) wt_host_free(s.h_of);
    if (s.h_ov) wt_host_free(s.h_ov);
    if (s.h_tile) wt_host_free(s.h_tile);
    if (s.h_ip) wt_host_free(s.h_ip);
    if (s.h_bw) wt_host_free(s.h_bw);
    if (s.h_integ) wt_host_free(s.h_integ);
    (void) wt_dev_free(s.d_integ);
    if (s.h_bw_status) wt_host_free(s.h_bw_status);
    (void) wt_dev_free(s.d_bw);
    for (hipEvent_t e : {s.e_bwc, s.e_bw0, s.e_bw1})
        if (e) (void) hipEventDestroy(e);
    if (s.ts) {
        s.ts->d_start = s.ts->d_finish = nullptr; s.ts->d_value = nullptr;      // the slot's, freed above
        wtamd_trackset_destroy(s.ts);
    }
    for (hipEvent_t e : {s.e_h0, s.e_h1, s.e_k0, s.e_cnt, s.e_patch, s.e_d0, s.e_d1})
        if (e) (void) hipEventDestroy(e);
    s = WtSlot();
}

template <class T>
static hipError_t wt_pinned_grow(T **p, int64_t old_n, int64_t used, int64_t new_n) {
    T *q = nullptr;
    const hipError_t e = wt_host_alloc((void **) &q, sizeof(T) * (size_t) (new_n > 0 ? new_n : 1));
    if (e != hipSuccess) return e;
    if (*p) {
        if (used > 0) memcpy(q, *p, sizeof(T) * (size_t) (used < old_n ? used : old_n));
        wt_host_free(*p);
    }
    *p = q;
    return hipSuccess;
}

static int wt_slot_grow_input(WtSlot &s, int64_t used, int64_t min_cap, bool want64) {
    if (min_cap > s.cap) {
        WT_HIP(wt_pinned_grow(&s.h_start, s.cap, used, min_cap));
        WT_HIP(wt_pinned_grow(&s.h_finish, s.cap, used, min_cap));
        WT_HIP(wt_pinned_grow(&s.h_v32, s.cap, used, min_cap));
        if (s.has64) WT_HIP(wt_pinned_grow(&s.h_v64, s.cap, used, min_cap));
        s.cap = min_cap;
    }
    if (want64 && !s.has64) {
        WT_HIP(wt_pinned_grow(&s.h_v64, 0, 0, s.cap));
        s.has64 = true;
    }
    return WTAMD_OK;
}

// Bounded wait (wt_host.h) for an event of the pipe
static int wt_wait_event(hipEvent_t ev, const char *what) {
    return wt_bounded_wait([ev] { return hipEventQuery(ev); }, "hipEventQuery", what, 0.0005, 50, [what](double limit_s) {
        char buf[160];
        snprintf(buf, sizeof buf, "pipeline %s did not finish within %.0f s", what, limit_s);
        return std::string(buf);
    });
}

static int wt_pipe_enqueue_export(wtamd_pipe *p, WtSlot &s, hipEvent_t after) {
    WT_HIP(hipStreamWaitEvent(p->s_out, after, 0));
    WT_HIP(hipEventRecord(s.e_d0, p->s_out));
    long long blocks = (s.ocap + 256 * 16 - 1) / (256 * 16);
    if (blocks > 2ll * s.ts->num_cu) blocks = 2ll * s.ts->num_cu;
    if (blocks < 1) blocks = 1;
    const bool cz = s.compressed;
    hipLaunchKernelGGL(wt_export_kernel, dim3((unsigned) blocks), dim3(256), 0, p->s_out, s.ts->d_counters, s.ts->h_counters,
                       cz ? (const unsigned long long *) s.d_cn : (const unsigned long long *) (s.ts->d_counters + WT_CTR_RUNS),
                       (long long) s.ocap, p->cfg.n_tracks, cz ? s.d_cs : s.d_os, cz ? s.d_cf : s.d_of, cz ? s.d_cv : s.d_ov, p->tile ? s.d_tile : nullptr,
                       p->tile ? s.d_ip : nullptr, s.h_os, s.h_of, s.h_ov, p->tile ? s.h_tile : nullptr, p->tile ? s.h_ip : nullptr);
    WT_HIP(hipGetLastError());
    WT_HIP(hipEventRecord(s.e_d1, p->s_out));
    return WTAMD_OK;
}

// Integrals of the slot's (uncompressed) device runs -> s.h_integ, on `st`: {sum len * value, span} over the non-NaN
// runs (statistics.c:62-120), or the Pearson moments of the 2-track tile (:414-465).  The run count is read on
// the device.
// mode 2: all six run moments {sum, span, T, min, max, 0} of wt_moments.hip (varI / stddevI / CVI / maxI / minI / span).
#define WT_INTEG_BLOCKS 256
#define WT_INTEG_PARTIAL 64         // bytes per block, enough for every integrator (wt_*_partial_bytes: 16, 48 and 64 per block)
static int wt_pipe_enqueue_integ(wtamd_pipe *p, WtSlot &s, hipStream_t st, int mode) {
    const size_t part = (size_t) WT_INTEG_PARTIAL * WT_INTEG_BLOCKS, need = part + sizeof(double) * 16;
    if (wt_moments_partial_bytes(WT_INTEG_BLOCKS) > part || wt_pearson_partial_bytes(WT_INTEG_BLOCKS) > part || wt_auc_partial_bytes(WT_INTEG_BLOCKS) > part)
        return wt_fail(WTAMD_ERR_INTERNAL, "partials of the integrators");
    if (!s.d_integ) WT_HIP(wt_dev_alloc((void **) &s.d_integ, need));
    if (!s.h_integ) { WT_HIP(wt_host_alloc((void **) &s.h_integ, sizeof(double) * 8)); }
    const unsigned long long *n_dev = s.ts->d_counters + WT_CTR_RUNS;
    double *d_out = (double *) (s.d_integ + part);
    s.integ_mode = mode;
    int rc;
    if (mode == 2) {
        if (p->tile) return wt_fail(WTAMD_ERR_ARG, "the run moments are those of a reducer's output, not of a Multiplexer tile");
        rc = wt_moments_async(s.d_os, s.d_of, s.d_ov, (long long) s.ocap, n_dev, WT_INTEG_BLOCKS, s.d_integ, d_out, st);
    } else if (p->tile) {
        if (p->cfg.n_tracks != 2) return wt_fail(WTAMD_ERR_ARG, "the fused Pearson integrator needs a Multiplexer of exactly two tracks");
        rc = wt_pearson_async(s.d_os, s.d_of, s.d_tile, s.d_ip, p->defaults[0], p->defaults[1], (long long) s.ocap, n_dev, WT_INTEG_BLOCKS, s.d_integ, d_out, st);
    } else {
        rc = wt_auc_async(s.d_os, s.d_of, s.d_ov, (long long) s.ocap, n_dev, WT_INTEG_BLOCKS, s.d_integ, d_out, true, st);
    }
    if (rc != WTAMD_OK) return rc;
    // (the Pearson entry puts the correlation in front of its six moments; {sum, span} are two doubles)
    WT_HIP(hipMemcpyAsync(s.h_integ, d_out + (mode != 2 && p->tile ? 1 : 0), sizeof(double) * (mode == 2 || p->tile ? 6 : 2), hipMemcpyDeviceToHost, st));
    return WTAMD_OK;
}

// The device buffers of the slot's output as the engine's launches take them
static wtamd_runs wt_slot_runs(const WtSlot &s) {
    wtamd_runs runs{};
    runs.capacity = s.ocap; runs.start = s.d_os; runs.finish = s.d_of; runs.value = s.d_ov; runs.chrom_run_off = s.d_cro;
    return runs;
}

// Compute stage, last part: the slot's runs merged on the device (buffers grow-only, with the output buffers)
static int wt_pipe_compress(wtamd_pipe *p, WtSlot &s) {
    if (!s.d_cs) {
        WT_HIP(wt_dev_alloc(&s.d_cs, sizeof(int32_t) * s.ocap));
        WT_HIP(wt_dev_alloc(&s.d_cf, sizeof(int32_t) * s.ocap));
        WT_HIP(wt_dev_alloc(&s.d_cv, sizeof(double) * s.ocap));
        WT_HIP(wt_dev_alloc(&s.d_cscratch, sizeof(unsigned long long) * (size_t) wt_compress_scratch_words((long long) s.ocap)));
    }
    if (!s.d_cn) WT_HIP(wt_dev_alloc(&s.d_cn, sizeof(unsigned long long)));
    const int rc = wt_compress_async(s.d_os, s.d_of, s.d_ov, s.ts->d_counters + WT_CTR_RUNS, (long long) s.ocap, s.d_cscratch, s.d_cs, s.d_cf,
                                     s.d_cv, s.d_cn, p->s_comp);
    return rc == WTAMD_OK ? rc : wt_fail(rc, "run compression launch failed");
}

// Ship stage: what goes home once the compute stream is through, which `done` marks.  Fused integrator: the integrals (and
// the counters), the runs stay.  Runs that travel by copy engine (export_pending): the counters, the runs are asked for when
// the batch is collected.  Else the export kernel, behind `done`.  counters = false: the host has them (a patched batch).
static int wt_pipe_ship(wtamd_pipe *p, WtSlot &s, hipEvent_t done, int integ_mode, bool counters) {
    wtamd_trackset *ts = s.ts;
    if (s.integrated) {
        const int rc = wt_pipe_enqueue_integ(p, s, p->s_comp, integ_mode);
        if (rc != WTAMD_OK) return rc;
    }
    if (counters && (s.integrated || s.export_pending)) {
        WT_HIP(hipMemcpyAsync(ts->h_counters, ts->d_counters, sizeof(unsigned long long) * WT_CTR_N, hipMemcpyDeviceToHost, p->s_comp));
        if (s.export_pending && s.compressed)
            WT_HIP(hipMemcpyAsync(ts->h_counters + WT_CTR_EXPORTED, s.d_cn, sizeof(unsigned long long), hipMemcpyDeviceToHost, p->s_comp));
    }
    WT_HIP(hipEventRecord(done, p->s_comp));
    return (s.integrated || s.export_pending) ? WTAMD_OK : wt_pipe_enqueue_export(p, s, done);
}

// The batch's export has landed: read the counters; patch, then compress and ship again if the difference-array
// launch left windows it could not prove exact.
static int wt_pipe_finish(wtamd_pipe *p, WtSlot &s) {
    wtamd_trackset *ts = s.ts;
    const unsigned long long *hc = ts->h_counters;
    if (hc[WT_CTR_ERROR] & WT_ERR_LOOKBACK) return wt_fail(WTAMD_ERR_INTERNAL, "look-back timed out");
    if (hc[WT_CTR_ERROR] & WT_ERR_CAPACITY) return wt_fail(WTAMD_ERR_CAPACITY, "batch emitted more runs than the slot's output capacity (max_runs)");
    const long long n_bad = (long long) hc[WT_CTR_DELTA_BAD];
    if (s.used_delta && n_bad > 0) {
        wtamd_runs runs = wt_slot_runs(s);
        int rc = wt_launch_patch(ts, s.delta_W, p->cfg.desc.op, p->cfg.desc.flags, p->cfg.desc.n_set0, &runs, n_bad, p->s_comp);
        if (rc == WTAMD_OK && s.compressed) rc = wt_pipe_compress(p, s);
        if (rc == WTAMD_OK) rc = wt_pipe_ship(p, s, s.e_patch, s.integ_mode, false);
        if (rc == WTAMD_OK) rc = s.integrated ? wt_wait_event(s.e_patch, "patched integrals") : wt_wait_event(s.e_d1, "patched result");
        if (rc != WTAMD_OK) return rc;
        s.patched = true;
        if (!wt_few_enough_to_patch(n_bad, ts->stats.n_windows)) p->delta_failed = true;     // this data: general kernel from now on
    }
    s.n_runs = (int64_t) hc[WT_CTR_EXPORTED];
    s.covered = (int64_t) hc[WT_CTR_BP];
    return WTAMD_OK;
}

extern "C" {

int wtamd_pipe_create(const wtamd_pipe_config *cfg, wtamd_pipe **out) {
    if (!cfg || !out || cfg->n_tracks <= 0 || !cfg->defaults || cfg->max_runs <= 0)
        return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_create: bad configuration");
    if (cfg->flags & ~0u & ~WTAMD_PIPE_COMPRESS) return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_create: unknown flag");
    const bool tile = cfg->desc.op == WTAMD_OP_MULTIPLEX;
    if ((cfg->flags & WTAMD_PIPE_COMPRESS) && tile) return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_create: the Multiplexer tile cannot be compressed");
    wt_warmup_join();           // (wtamd_warmup_async: the runtime's start-up, if a helper thread is at it)
    if (wtamd_device_count() <= 0) return wt_fail(WTAMD_ERR_NODEVICE, "no HIP device visible");
    wtamd_pipe *p = new wtamd_pipe();
    (void) hipGetDevice(&p->device);
    p->cfg = *cfg;
    p->defaults.assign(cfg->defaults, cfg->defaults + cfg->n_tracks);
    p->cfg.defaults = p->defaults.data();
    p->tile = tile;
    p->compress = (cfg->flags & WTAMD_PIPE_COMPRESS) != 0;
    if (getenv("WTAMD_PIPE_GATHER")) p->gather = atoi(getenv("WTAMD_PIPE_GATHER")) != 0;
    if (getenv("WTAMD_GATHER_BLOCKS") && atoi(getenv("WTAMD_GATHER_BLOCKS")) > 0) p->gather_blocks = atoi(getenv("WTAMD_GATHER_BLOCKS"));
    int ns = cfg->n_slots ? cfg->n_slots : 3;
    if (ns < 2) ns = 2;
    if (ns > 8) ns = 8;
    p->st.n_slots = ns;
    // streams, slots and their track sets; any failure lets go of the half-built pipe (below)
    auto build = [&]() -> int {
        if (!tile) {
            wtamd_trackset probe;       // argument check of the descriptor (same messages as wtamd_reduce)
            probe.n_tracks = cfg->n_tracks;
            const int rc = wt_check_desc(&probe, &cfg->desc);
            if (rc != WTAMD_OK) return rc;
        }
        // (Confining the PCIe-facing kernels to a few CUs with hipExtStreamCreateWithCUMask was tried: the inflate kernel
        // got slower -- fewer CUs, 21 ms against 13.5 ms per batch -- and the masked streams crashed the process in the
        // drop-in tests; tools/probes/cumask_probe.hip shows how the mask bits map to CUs on this GPU.)
        WT_HIP(hipStreamCreateWithFlags(&p->s_copy, hipStreamNonBlocking));
        WT_HIP(hipStreamCreateWithFlags(&p->s_comp, hipStreamNonBlocking));
        WT_HIP(hipStreamCreateWithFlags(&p->s_out, hipStreamNonBlocking));
        p->slots.resize((size_t) ns);
        const int64_t cap0 = cfg->max_intervals > 0 ? cfg->max_intervals : 4096;
        const int N = cfg->n_tracks;
        std::vector<int64_t> seg0((size_t) N + 1, 0);
        for (auto &s : p->slots) {
            WT_HIP(wt_host_alloc((void **) &s.h_seg, sizeof(int64_t) * ((size_t) N + 1)));
            memset(s.h_seg, 0, sizeof(int64_t) * ((size_t) N + 1));
            int rc = wt_slot_grow_input(s, 0, cap0, false);
            if (rc != WTAMD_OK) return rc;
            for (hipEvent_t *e : {&s.e_h0, &s.e_h1, &s.e_k0, &s.e_cnt, &s.e_patch, &s.e_d0, &s.e_d1}) WT_HIP(hipEventCreate(e));
            // the slot's track set: one chromosome, device arrays bound per batch
            wtamd_tracks t;
            memset(&t, 0, sizeof(t));
            t.n_chrom = 1; t.n_tracks = N; t.seg_off = seg0.data(); t.defaults = p->defaults.data();
            s.ts = new wtamd_trackset();
            rc = wt_trackset_common(&t, s.ts);
            if (rc != WTAMD_OK) return rc;
            s.ts->pipe_mode = true;
            s.ts->owns = false;
            s.ts->first_start.assign((size_t) N, 0);
            s.ts->last_finish.assign((size_t) N, 0);
            s.ts->range_lo.assign(1, 0);
            s.ts->range_hi.assign(1, INT32_MAX);
            WT_HIP(wt_dev_alloc(&s.d_cro, sizeof(int64_t) * 2));
        }
        return WTAMD_OK;
    };
    const int rc = build();
    if (rc != WTAMD_OK) { wtamd_pipe_destroy(p); return rc; }
    *out = p;
    return WTAMD_OK;
}

void wtamd_pipe_destroy(wtamd_pipe *p) {
    WtDevGuard dev_guard_(p ? p->device : -1);
    if (!p) return;
    // everything still in flight must have left the buffers before they are freed
    if (p->s_copy) (void) hipStreamSynchronize(p->s_copy);
    if (p->s_comp) (void) hipStreamSynchronize(p->s_comp);
    for (int k = 0; k < 2; k++)
        if (p->s_decs[k]) (void) hipStreamSynchronize(p->s_decs[k]);
    if (p->s_out) (void) hipStreamSynchronize(p->s_out);
    for (auto &s : p->slots) wt_slot_free(s);
    if (p->s_copy) (void) hipStreamDestroy(p->s_copy);
    if (p->s_comp) (void) hipStreamDestroy(p->s_comp);
    if (p->s_out) (void) hipStreamDestroy(p->s_out);
    if (p->d_chains) (void) wt_dev_free(p->d_chains);
    for (int k = 0; k < 2; k++) {
        (void) wt_dev_free(p->d_bw_scratches[k]);
        if (p->s_decs[k]) (void) hipStreamDestroy(p->s_decs[k]);
    }
    for (void *q : p->dead_dev) (void) wt_dev_free(q);
    for (void *q : p->dead_host) wt_host_free(q);
    delete p;
}

static void wt_fill_batch(const WtSlot &s, wtamd_pipe_batch *b) {
    b->capacity = s.cap;
    b->seg_off = s.h_seg;
    b->start = s.h_start; b->finish = s.h_finish;
    b->value32 = s.h_v32;
    b->value64 = s.has64 ? s.h_v64 : nullptr;
}

int wtamd_pipe_acquire(wtamd_pipe *p, wtamd_pipe_batch *out) {
    if (!p || !out) return wt_fail(WTAMD_ERR_ARG, "NULL argument");
    if (p->acquired >= 0) return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_acquire: a slot is already acquired");
    WtSlot &s = p->slots[(size_t) p->head];
    if (s.state != 0) return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_acquire: every slot is in flight or unreleased");
    s.state = 1;
    p->acquired = p->head;
    wt_fill_batch(s, out);
    return WTAMD_OK;
}

int wtamd_pipe_grow(wtamd_pipe *p, int64_t used, int64_t min_capacity, int want_f64, wtamd_pipe_batch *out) {
    WtDevGuard dev_guard_(p ? p->device : -1);
    if (!p || !out || p->acquired < 0) return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_grow: no acquired slot");
    WtSlot &s = p->slots[(size_t) p->acquired];
    if (used > s.cap || used < 0) return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_grow: used > capacity");
    const int rc = wt_slot_grow_input(s, used, min_capacity, want_f64 != 0);
    if (rc != WTAMD_OK) return rc;
    wt_fill_batch(s, out);
    return WTAMD_OK;
}

int wtamd_pipe_put_direct(wtamd_pipe *p, int64_t at, int64_t count, const int32_t *start, const int32_t *finish,
                          const float *value) {
    WtDevGuard dev_guard_(p ? p->device : -1);
    if (!p || p->acquired < 0) return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_put_direct: no acquired slot");
    if (count <= 0) return WTAMD_OK;
    if (at < 0 || !start || !finish || !value) return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_put_direct: bad arguments");
    WtSlot &s = p->slots[(size_t) p->acquired];
    if (!s.direct.empty() && s.direct.back().at + s.direct.back().count > at)
        return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_put_direct: ranges must be added in ascending order");
    if (s.direct.empty()) s.direct_pinned = true;
    if (p->gather && s.direct_pinned && !(wt_is_pinned(start) && wt_is_pinned(finish) && wt_is_pinned(value))) s.direct_pinned = false;
    s.direct.push_back({at, count, start, finish, value});
    return WTAMD_OK;
}

int wtamd_pipe_cancel(wtamd_pipe *p) {
    if (!p || p->acquired < 0) return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_cancel: no acquired slot");
    p->slots[(size_t) p->acquired].direct.clear();
    p->slots[(size_t) p->acquired].bw_res_bytes = p->slots[(size_t) p->acquired].bw_res_secs = -1;
    p->slots[(size_t) p->acquired].state = 0;
    p->acquired = -1;
    return WTAMD_OK;
}

// bw_tracks != NULL: the batch came as BigWig file bytes (wtamd_pipe_submit_bw) -- the run lists are produced
// on the device, the host only knows upper bounds of their sizes and extents.
static int wt_pipe_submit_impl(wtamd_pipe *p, int value_is_f64, int32_t range_lo, int32_t range_hi,
                               const wtamd_bw_track *bw_tracks = nullptr, int64_t bw_bytes = 0, int64_t bw_secs = 0, WtSlot *redo = nullptr);

int wtamd_pipe_submit(wtamd_pipe *p, int value_is_f64, int32_t range_lo, int32_t range_hi) {
    WtDevGuard dev_guard_(p ? p->device : -1);
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = wt_pipe_submit_impl(p, value_is_f64, range_lo, range_hi);
    if (p) p->st.host_submit_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

static int64_t wt_align256(int64_t x) { return (x + 255) & ~(int64_t) 255; }

unsigned wtamd_pipe_bw_error(const wtamd_pipe *p) { return p ? p->last_bw_err : 0u; }

int64_t wtamd_pipe_bw_redone(const wtamd_pipe *p) { return p ? p->bw_redone : 0; }

int64_t wtamd_pipe_bw_fill_sections(const wtamd_pipe *p) {
    if (!p || p->slots.empty() || !p->slots[0].ts) return 0;
    return (int64_t) wt_bw_fill_sections(p->slots[0].ts->num_cu);
}

int wtamd_pipe_bw_reserve(wtamd_pipe *p, int64_t n_bytes, int64_t n_sections, uint8_t **bytes, wtamd_bw_section **sections) {
    WtDevGuard dev_guard_(p ? p->device : -1);
    if (!p || p->acquired < 0) return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_bw_reserve: no acquired slot");
    if (n_bytes < 0 || n_sections < 0 || !bytes || !sections) return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_bw_reserve: bad arguments");
    WtSlot &s = p->slots[(size_t) p->acquired];
    const int N = p->cfg.n_tracks;
    s.bw_off_sec = wt_align256((int64_t) sizeof(wtamd_bw_track) * N);
    s.bw_off_bytes = s.bw_off_sec + wt_align256((int64_t) sizeof(wtamd_bw_section) * n_sections);
    const int64_t need = s.bw_off_bytes + wt_align256(n_bytes + 64);
    if (s.h_bw_cap < need) {
        if (s.h_bw) p->dead_host.push_back(s.h_bw);
        s.h_bw = nullptr; s.h_bw_cap = 0;
        const int64_t c = need + need / 4;
        WT_HIP(wt_host_alloc((void **) &s.h_bw, (size_t) c));
        s.h_bw_cap = c;
    }
    s.bw_res_bytes = n_bytes; s.bw_res_secs = n_sections;
    *bytes = s.h_bw + s.bw_off_bytes;
    *sections = (wtamd_bw_section *) (s.h_bw + s.bw_off_sec);
    return WTAMD_OK;
}

int wtamd_pipe_submit_bw(wtamd_pipe *p, int64_t n_bytes, int64_t n_sections, const wtamd_bw_track *tracks,
                         int32_t range_lo, int32_t range_hi) {
    WtDevGuard dev_guard_(p ? p->device : -1);
    const auto t0 = std::chrono::steady_clock::now();
    if (!p || p->acquired < 0) return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_submit_bw: no acquired slot");
    if (!tracks) return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_submit_bw: tracks == NULL");
    const int rc = wt_pipe_submit_impl(p, 0, range_lo, range_hi, tracks, n_bytes, n_sections);
    p->st.host_submit_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

// Host-side bounds of a batch that arrives as file bytes: seg_off[] (piece counts), per-track extents.
static int wt_pipe_bw_bounds(wtamd_pipe *p, WtSlot &s, const wtamd_bw_track *tk, int64_t n_bytes, int64_t n_secs, int64_t *plain_stride) {
    const int N = p->cfg.n_tracks;
    if (s.bw_res_bytes < 0 || n_bytes > s.bw_res_bytes || n_secs > s.bw_res_secs || n_bytes < 0 || n_secs < 0)
        return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_submit_bw: more bytes / sections than reserved");
    if (p->tile) return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_submit_bw: not available for the Multiplexer tile");
    const wtamd_bw_section *sec = (const wtamd_bw_section *) (s.h_bw + s.bw_off_sec);
    int64_t at = 0, next_sec = 0, stride = 64;
    for (int i = 0; i < N; i++) {
        const wtamd_bw_track &t = tk[i];
        if (t.first_section != next_sec || t.n_sections < 0 || (int64_t) t.first_section + t.n_sections > n_secs)
            return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_submit_bw: sections must be listed track by track");
        s.h_seg[i] = at;
        int32_t fs = 0, lf = 0;
        for (int64_t q = t.first_section; q < (int64_t) t.first_section + t.n_sections; q++) {
            const wtamd_bw_section &c = sec[q];
            if (c.track != i || c.comp_off < 0 || c.comp_off + (int64_t) c.comp_size > n_bytes || c.leaf_end < c.leaf_start)
                return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_submit_bw: bad section entry");
            if (q > t.first_section && c.leaf_start < sec[q - 1].leaf_end)
                return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_submit_bw: a track's sections must be sorted and disjoint");
            if (!t.compressed && c.comp_size > t.plain_bytes) return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_submit_bw: raw section larger than plain_bytes");
            at += wt_bw_section_bound(t.plain_bytes, c.leaf_start, c.leaf_end, t.box);
        }
        if (t.n_sections > 0) {
            const int64_t a = (int64_t) sec[t.first_section].leaf_start + 1, b = (int64_t) sec[t.first_section + t.n_sections - 1].leaf_end + 1;
            fs = (int32_t) std::max<int64_t>(a, t.clip_lo);
            lf = (int32_t) std::min<int64_t>(std::min<int64_t>(b, t.clip_hi), INT32_MAX);
            if (lf <= fs) lf = fs + 1;
            if ((int64_t) t.plain_bytes + 16 > stride) stride = (int64_t) t.plain_bytes + 16;
        }
        s.ts->first_start[(size_t) i] = fs;
        s.ts->last_finish[(size_t) i] = lf;
        next_sec += t.n_sections;
    }
    if (next_sec != n_secs) return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_submit_bw: section count does not match the tracks");
    s.h_seg[N] = at;
    *plain_stride = (stride + 15) & ~(int64_t) 15;
    return WTAMD_OK;
}

// One batch on its way through wt_pipe_submit_impl's stages
struct WtBatch {
    bool bw, f64, redo;                 // came as file bytes / float64 values / a file-byte batch decoded once more
    int64_t n;                          // intervals (file bytes: the host's upper bound)
    int32_t range_lo, range_hi;
    const wtamd_bw_track *bw_tracks;
    int64_t bw_bytes, bw_secs, bw_stride;
    bool mapped, map_f32, compacted;    // operator chains: any / their output stays float32 / they drop runs
};

// Check stage: the batch as the caller staged it
static int wt_pipe_check(wtamd_pipe *p, WtSlot &s, WtBatch &b) {
    const int N = p->cfg.n_tracks;
    if (b.bw && !b.redo) {
        if (!s.direct.empty()) return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_submit_bw: the slot holds direct ranges");
        const int rcb = wt_pipe_bw_bounds(p, s, b.bw_tracks, b.bw_bytes, b.bw_secs, &b.bw_stride);
        if (rcb != WTAMD_OK) return rcb;
    }
    const int64_t n = b.n = s.h_seg[N];
    if (s.h_seg[0] != 0 || n < 0) return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_submit: bad seg_off");
    // staged ranges = [0, n) minus the direct ranges; they must lie inside the staging arrays
    if (!b.bw) {
        int64_t staged_end = 0, pos = 0;
        for (const auto &d : s.direct) {
            if (d.at + d.count > n) return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_submit: a direct range lies beyond seg_off[n_tracks]");
            if (d.at > pos) staged_end = d.at;
            pos = d.at + d.count;
        }
        if (pos < n) staged_end = n;
        if (staged_end > s.cap) return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_submit: staged intervals beyond the staging capacity");
        if (b.f64 && !s.direct.empty()) return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_submit: direct ranges are float32");
    }
    for (int i = 0; i < N; i++)
        if (s.h_seg[i + 1] < s.h_seg[i]) return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_submit: seg_off not monotone");
    if (b.f64 && !s.has64) return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_submit: float64 values were never staged");
    return WTAMD_OK;
}

// Reserve stage: the slot's device buffers (and the pinned output), grow-only
static int wt_pipe_reserve(wtamd_pipe *p, WtSlot &s, const WtBatch &b) {
    const int N = p->cfg.n_tracks;
    const int64_t n = b.n;
    // device twin of the staging
    int64_t need_in = n > 0 ? n : 1;
    if (b.bw && !b.redo && p->bw_density >= 0.0 && p->bw_density < 1.0) {
        const int64_t by_density = (int64_t) ((double) n * p->bw_density * 1.125) + 65536;
        if (by_density < need_in) need_in = by_density;
    }
    if (s.dcap < need_in || (b.f64 && !s.d_has64)) {
        // an eighth of slack, not a doubling: the batches of a run settle on one size and wobble by a fraction of a
        // percent around it (63 220 sections, then 63 502), and "twice the old capacity" answered the first batch that
        // was a hair larger with three more arrays of 1.5 GB per slot -- 27.6 of the 37.6 GB a pipe of 100 BigWig tracks
        // held, and most of the time its first run spent in hipMalloc (round 3, WTAMD_TRACE_POOL=1).  The ramp at the
        // start of a run grows by factors anyway.
        int64_t c = need_in + need_in / 8;
        if (c < s.cap) c = s.cap;
        for (void *q : {(void *) s.d_start, (void *) s.d_finish, s.d_value}) if (q) p->dead_dev.push_back(q);
        s.d_start = s.d_finish = nullptr; s.d_value = nullptr; s.dcap = 0;
        const bool w64 = b.f64 || s.d_has64 || s.has64;
        WT_HIP(wt_dev_alloc(&s.d_start, sizeof(int32_t) * c));
        WT_HIP(wt_dev_alloc(&s.d_finish, sizeof(int32_t) * c));
        WT_HIP(wt_dev_alloc(&s.d_value, (w64 ? 8 : 4) * (size_t) c));
        s.dcap = c; s.d_has64 = w64;
    }
    if (b.mapped && (s.mcap < s.dcap || (p->map_drops && !s.m_has_coords))) {
        for (void *q : {(void *) s.d_mstart, (void *) s.d_mfinish, (void *) s.d_mvalue, (void *) s.d_mscratch}) if (q) p->dead_dev.push_back(q);
        s.d_mstart = s.d_mfinish = nullptr; s.d_mvalue = nullptr; s.d_mscratch = nullptr; s.mcap = 0; s.m_has_coords = false;
        WT_HIP(wt_dev_alloc(&s.d_mvalue, sizeof(double) * (size_t) s.dcap));
        if (p->map_drops) {
            WT_HIP(wt_dev_alloc(&s.d_mstart, sizeof(int32_t) * (size_t) s.dcap));
            WT_HIP(wt_dev_alloc(&s.d_mfinish, sizeof(int32_t) * (size_t) s.dcap));
            WT_HIP(wt_dev_alloc(&s.d_mscratch, sizeof(unsigned long long) * (size_t) wt_map_scratch_words((long long) s.dcap)));
            if (!s.d_mseg) WT_HIP(wt_dev_alloc(&s.d_mseg, sizeof(int64_t) * ((size_t) N + 1)));
            s.m_has_coords = true;
        }
        s.mcap = s.dcap;
    }
    // output (bounded by max_runs): a run is at least 1 bp and starts at an interval edge
    int64_t need_out = 2 * n;
    const int64_t span = (int64_t) b.range_hi - (int64_t) b.range_lo;
    if (b.range_hi != INT32_MAX && span < need_out) need_out = span > 0 ? span : 0;
    if (need_out > p->cfg.max_runs) need_out = p->cfg.max_runs;
    if (need_out < 1) need_out = 1;
    if (s.ocap < need_out) {
        int64_t c = need_out + need_out / 8;        // (slack, not a doubling: see the device twins above)
        if (c > p->cfg.max_runs) c = p->cfg.max_runs;
        if (c < need_out) c = need_out;
        for (void *q : {(void *) s.d_os, (void *) s.d_of, (void *) s.d_ov, (void *) s.d_tile, (void *) s.d_ip}) if (q) p->dead_dev.push_back(q);
        s.d_os = s.d_of = nullptr; s.d_ov = s.d_tile = nullptr; s.d_ip = nullptr;
        for (void *q : {(void *) s.h_os, (void *) s.h_of, (void *) s.h_ov, (void *) s.h_tile, (void *) s.h_ip}) if (q) p->dead_host.push_back(q);
        s.h_os = s.h_of = nullptr; s.h_ov = s.h_tile = nullptr; s.h_ip = nullptr; s.ocap = 0;
        WT_HIP(wt_dev_alloc(&s.d_os, sizeof(int32_t) * c));
        WT_HIP(wt_dev_alloc(&s.d_of, sizeof(int32_t) * c));
        WT_HIP(wt_dev_alloc(&s.d_ov, sizeof(double) * c));
        WT_HIP(wt_host_alloc((void **) &s.h_os, sizeof(int32_t) * c));
        WT_HIP(wt_host_alloc((void **) &s.h_of, sizeof(int32_t) * c));
        WT_HIP(wt_host_alloc((void **) &s.h_ov, sizeof(double) * c));
        for (void *q : {(void *) s.d_cs, (void *) s.d_cf, (void *) s.d_cv, (void *) s.d_cscratch}) if (q) p->dead_dev.push_back(q);
        s.d_cs = s.d_cf = nullptr; s.d_cv = nullptr; s.d_cscratch = nullptr;
        if (p->tile) {
            WT_HIP(wt_dev_alloc(&s.d_tile, sizeof(double) * c * N));
            WT_HIP(wt_dev_alloc(&s.d_ip, sizeof(uint8_t) * c * N));
            WT_HIP(wt_host_alloc((void **) &s.h_tile, sizeof(double) * c * N));
            WT_HIP(wt_host_alloc((void **) &s.h_ip, sizeof(uint8_t) * c * N));
        }
        s.ocap = c;
    }
    return WTAMD_OK;
}

// Rebind stage: the slot's track set takes on this batch
static int wt_pipe_rebind(wtamd_pipe *p, WtSlot &s, const WtBatch &b) {
    wtamd_trackset *ts = s.ts;
    if (!b.bw) {
        // the direct range that holds entry g of the batch; NULL: g lies in the staging arrays (file bytes: wt_pipe_bw_bounds)
        auto direct_of = [&](int64_t g) -> const WtSlot::Direct * {
            size_t lo = 0, hi = s.direct.size();
            while (lo < hi) { const size_t m = (lo + hi) / 2; if (s.direct[m].at + s.direct[m].count <= g) lo = m + 1; else hi = m; }
            return (lo < s.direct.size() && s.direct[lo].at <= g) ? &s.direct[lo] : nullptr;
        };
        for (int i = 0; i < p->cfg.n_tracks; i++) {
            const int64_t a = s.h_seg[i], z = s.h_seg[i + 1] - 1;
            const WtSlot::Direct *da = z >= a ? direct_of(a) : nullptr, *dz = z >= a ? direct_of(z) : nullptr;
            ts->first_start[(size_t) i] = z < a ? 0 : (da ? da->start[a - da->at] : s.h_start[a]);
            ts->last_finish[(size_t) i] = z < a ? 0 : (dz ? dz->finish[z - dz->at] : s.h_finish[z]);
        }
    }
    // mapped batches: the kernels read the operator chains' output (the host-side seg_off[] / extents stay those
    // of the raw lists: upper bounds, which is all the planning needs)
    return wt_trackset_rebind(ts, b.n, s.h_seg, b.range_lo, b.range_hi, b.f64 || (b.mapped && !b.map_f32), b.compacted ? s.d_mstart : s.d_start,
                              b.compacted ? s.d_mfinish : s.d_finish, b.mapped ? (void *) s.d_mvalue : s.d_value, p->delta_failed);
}

// Upload stage, file bytes: file bytes + tables in one copy; inflate / count / scan / scatter on the decode stream write the
// run lists and the device-side seg_off[] (the authority downstream: the host's are upper bounds)
// (on the COMPUTE stream: HIP maps its streams onto 4 hardware queues, and a fourth stream of the pipe landed
// on the copy stream's queue -- the next batch's copy then waited behind this batch's inflate kernel)
static int wt_pipe_upload_bw(wtamd_pipe *p, WtSlot &s, const WtBatch &b) {
    const int N = p->cfg.n_tracks;
    {
        if (p->n_decs == 0) {
            const char *e = getenv("WTAMD_BW_DECODE_STREAMS");
            p->n_decs = (e && atoi(e) == 2) ? 2 : -1;
            for (int k = 0; k < 2 && p->n_decs == 2; k++) WT_HIP(hipStreamCreateWithFlags(&p->s_decs[k], hipStreamNonBlocking));
        }
        const int k = p->n_decs == 2 ? (int) (p->bw_batches & 1) : 0;
        p->bw_batches++;
        p->s_dec = p->n_decs == 2 ? p->s_decs[k] : p->s_comp;
        // the slot's run lists and outputs were last touched by the kernels of its previous batch on the compute
        // stream (long collected); the scratch is per decode stream
        p->d_bw_scratch = p->d_bw_scratches[k]; p->bw_scratch_cap = p->bw_scratch_caps[k];
        s.bw_dec = k;
    }
    if (!s.e_bwc) { WT_HIP(hipEventCreate(&s.e_bwc)); WT_HIP(hipEventCreate(&s.e_bw0)); WT_HIP(hipEventCreate(&s.e_bw1)); }
    if (!s.h_bw_status) WT_HIP(wt_host_alloc((void **) &s.h_bw_status, 64));
    const int64_t total = s.bw_off_bytes + wt_align256(b.bw_bytes + 64);
    if (s.d_bw_cap < total) {
        if (s.d_bw) p->dead_dev.push_back(s.d_bw);
        s.d_bw = nullptr; s.d_bw_cap = 0;
        const int64_t c = total + total / 4;
        WT_HIP(wt_dev_alloc((void **) &s.d_bw, (size_t) c));
        s.d_bw_cap = c;
    }
    const int64_t need_scr = wt_bw_scratch_bytes(b.bw_secs, b.bw_stride);
    if (p->bw_scratch_cap < need_scr) {
        if (p->d_bw_scratch) p->dead_dev.push_back(p->d_bw_scratch);
        p->d_bw_scratch = nullptr; p->bw_scratch_cap = 0;
        const int64_t c = need_scr + need_scr / 4;
        WT_HIP(wt_dev_alloc(&p->d_bw_scratch, (size_t) c));
        p->bw_scratch_cap = c;
        p->d_bw_scratches[s.bw_dec] = p->d_bw_scratch; p->bw_scratch_caps[s.bw_dec] = c;
    }
    if (!b.redo) memcpy(s.h_bw, b.bw_tracks, sizeof(wtamd_bw_track) * (size_t) N);
    s.h_bw_status[0] = ~0ull; s.h_bw_status[1] = 0;
    WT_HIP(hipEventRecord(s.e_bw0, p->s_dec));
    const int rc = wt_bw_decode_async(s.h_bw, s.d_bw, total, s.d_bw + s.bw_off_bytes, s.d_bw + s.bw_off_sec, s.d_bw, N, b.bw_secs, b.bw_stride, p->d_bw_scratch,
                                      (long long) s.dcap, s.d_start, s.d_finish, (float *) s.d_value, b.compacted ? s.d_mseg : s.ts->d_seg_off,
                                      s.h_bw_status, p->gather_blocks, p->s_copy, s.e_bwc, p->s_dec);
    if (rc != WTAMD_OK) return rc;
    WT_HIP(hipEventRecord(s.e_bw1, p->s_dec));
    s.bw_secs = b.bw_secs; s.bw_bytes = b.bw_bytes; s.bw_stride = b.bw_stride; s.bw_bound = b.n;
    s.bw_res_bytes = s.bw_res_secs = -1;
    return WTAMD_OK;
}

// Upload stage, gather kernel: one table, one kernel for the whole batch
static int wt_pipe_upload_gather(wtamd_pipe *p, WtSlot &s, const WtBatch &b) {
    const int64_t max_segs = 2 * (int64_t) s.direct.size() + 1;
    if (s.seg_cap < max_segs) {
        if (s.h_segs) wt_host_free(s.h_segs);
        s.h_segs = nullptr; s.seg_cap = 0;
        const int64_t c = 2 * max_segs;
        WT_HIP(wt_host_alloc((void **) &s.h_segs, sizeof(WtGatherSeg) * c));
        s.seg_cap = c;
    }
    int ns = 0;
    long long chunks = 0;
    auto add = [&](const int32_t *ps, const int32_t *pf, const float *pv, int64_t dst, int64_t count) {
        if (count <= 0) return;
        s.h_segs[ns++] = WtGatherSeg{ps, pf, pv, dst, count, chunks};
        chunks += (count + WT_GATHER_CHUNK - 1) / WT_GATHER_CHUNK;
    };
    int64_t pos = 0;
    for (const auto &d : s.direct) {
        add(s.h_start + pos, s.h_finish + pos, s.h_v32 + pos, pos, d.at - pos);       // staged gap before it
        add(d.start, d.finish, d.value, d.at, d.count);
        pos = d.at + d.count;
    }
    add(s.h_start + pos, s.h_finish + pos, s.h_v32 + pos, pos, b.n - pos);
    // Few blocks on purpose: every block keeps 48 KB of reads in flight, and whatever is queued
    // on the link delays every OTHER host read by queue / bandwidth -- kernel arguments and the
    // small tables of the compute kernels of the previous batch included (measured with 768
    // blocks = 37 MB in flight: those kernels started ~1.7 ms late, right at the gather's tail).
    // The bandwidth-delay product of the link is well below 1 MB.
    long long grid = p->gather_blocks;
    if (grid > chunks) grid = chunks;
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(wt_gather_kernel, dim3((unsigned) grid), dim3(256), 0, p->s_copy, s.h_segs, ns, chunks,
                       s.d_start, s.d_finish, (float *) s.d_value);
    WT_HIP(hipGetLastError());
    return WTAMD_OK;
}

// Upload stage, copies: three hipMemcpyAsync per range, staged or the caller's (no staging copy)
static int wt_pipe_upload_copies(wtamd_pipe *p, WtSlot &s, const WtBatch &b) {
    auto staged = [&](int64_t a, int64_t e) -> int {        // staging [a, e) -> HBM
        if (e <= a) return WTAMD_OK;
        WT_HIP(hipMemcpyAsync(s.d_start + a, s.h_start + a, sizeof(int32_t) * (e - a), hipMemcpyHostToDevice, p->s_copy));
        WT_HIP(hipMemcpyAsync(s.d_finish + a, s.h_finish + a, sizeof(int32_t) * (e - a), hipMemcpyHostToDevice, p->s_copy));
        if (b.f64) WT_HIP(hipMemcpyAsync((double *) s.d_value + a, s.h_v64 + a, sizeof(double) * (e - a), hipMemcpyHostToDevice, p->s_copy));
        else WT_HIP(hipMemcpyAsync((float *) s.d_value + a, s.h_v32 + a, sizeof(float) * (e - a), hipMemcpyHostToDevice, p->s_copy));
        return WTAMD_OK;
    };
    int64_t pos = 0;
    for (const auto &d : s.direct) {
        const int rc = staged(pos, d.at);
        if (rc != WTAMD_OK) return rc;
        WT_HIP(hipMemcpyAsync(s.d_start + d.at, d.start, sizeof(int32_t) * d.count, hipMemcpyHostToDevice, p->s_copy));
        WT_HIP(hipMemcpyAsync(s.d_finish + d.at, d.finish, sizeof(int32_t) * d.count, hipMemcpyHostToDevice, p->s_copy));
        WT_HIP(hipMemcpyAsync((float *) s.d_value + d.at, d.value, sizeof(float) * d.count, hipMemcpyHostToDevice, p->s_copy));
        pos = d.at + d.count;
    }
    return staged(pos, b.n);
}

// Upload stage: pinned staging (or file bytes) -> the slot's device run lists, on the copy stream; e_h1 marks them complete
static int wt_pipe_upload(wtamd_pipe *p, WtSlot &s, const WtBatch &b) {
    const int N = p->cfg.n_tracks;
    int rc = WTAMD_OK;
    WT_HIP(hipEventRecord(s.e_h0, p->s_copy));
    s.bw = b.bw;
    if (b.bw) {
        rc = wt_pipe_upload_bw(p, s, b);
    } else {
        WT_HIP(hipMemcpyAsync(b.compacted ? s.d_mseg : s.ts->d_seg_off, s.h_seg, sizeof(int64_t) * ((size_t) N + 1), hipMemcpyHostToDevice, p->s_copy));
        if (b.n > 0 && p->gather && !b.f64 && !s.direct.empty() && s.direct_pinned && 2 * (int64_t) s.direct.size() + 1 <= WT_GATHER_MAX_SEGS)
            rc = wt_pipe_upload_gather(p, s, b);
        else if (b.n > 0)
            rc = wt_pipe_upload_copies(p, s, b);
    }
    if (rc != WTAMD_OK) return rc;
    s.direct.clear();
    WT_HIP(hipEventRecord(s.e_h1, b.bw ? p->s_dec : p->s_copy));    // (file bytes: the run lists exist once the decode stream is through)
    p->st.h2d_bytes += b.bw ? s.bw_off_bytes + b.bw_bytes : (int64_t) sizeof(int64_t) * (N + 1) + b.n * (b.f64 ? 16 : 12);
    return WTAMD_OK;
}

// Compute stage, on the compute stream behind the upload: operator chains, window index + fused multiplex / reduce, compression
static int wt_pipe_compute(wtamd_pipe *p, WtSlot &s, const WtBatch &b) {
    wtamd_trackset *ts = s.ts;
    WT_HIP(hipStreamWaitEvent(p->s_comp, s.e_h1, 0));
    WT_HIP(hipEventRecord(s.e_k0, p->s_comp));
    if (b.mapped) {
        const int rc = wt_map_chain_async(p->d_chains, p->cfg.n_tracks, p->map_drops, b.compacted ? s.d_mseg : ts->d_seg_off, (long long) b.n, s.d_start, s.d_finish,
                                          s.d_value, b.f64, s.d_mscratch, s.d_mstart, s.d_mfinish, s.d_mvalue, ts->d_seg_off, p->s_comp, b.map_f32);
        if (rc != WTAMD_OK) return wt_fail(rc, "operator chain launch failed");
    }
    wtamd_runs runs = wt_slot_runs(s);
    s.patched = false;
    const int rc = wt_reduce_enqueue(ts, p->cfg.desc, &runs, p->tile ? s.d_tile : nullptr, p->tile ? s.d_ip : nullptr, p->s_comp, &s.used_delta, &s.delta_W);
    if (rc != WTAMD_OK) return rc;
    s.integrated = p->integrate != 0;
    s.compressed = p->compress && !s.integrated;
    return s.compressed ? wt_pipe_compress(p, s) : WTAMD_OK;
}

// redo != NULL: the file-byte batch of that (submitted) slot once more, its run lists at the size of the host's bound
// -- everything the first submit staged (tables, file bytes, seg_off bounds) is still in place.
static int wt_pipe_submit_impl(wtamd_pipe *p, int value_is_f64, int32_t range_lo, int32_t range_hi,
                               const wtamd_bw_track *bw_tracks, int64_t bw_bytes, int64_t bw_secs, WtSlot *redo) {
    if (!p || (!redo && p->acquired < 0)) return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_submit: no acquired slot");
    WtSlot &s = redo ? *redo : p->slots[(size_t) p->acquired];
    const bool bw = bw_tracks != nullptr, f64 = value_is_f64 != 0, mapped = p->d_chains != nullptr;
    WtBatch b = {bw, f64, redo != nullptr, 0, range_lo, range_hi, bw_tracks, bw_bytes, bw_secs, redo ? s.bw_stride : 0,
                 mapped, mapped && p->map_f32 && !f64, mapped && p->map_drops};
    // File-byte batches: the runs go home through the COPY ENGINE, not the export kernel.  Next to a kernel whose
    // wavefronts wait on the PCIe link the per-lane inflate kernel of the following batch (a serial, latency-bound
    // lane per stream) took 13.5 ms instead of 9.5; the copy engine costs no CU anything.  It needs the run count on
    // the host: the counters travel first (128 bytes), the runs are requested when the batch is collected.
    static const bool sdma_out = !(getenv("WTAMD_BW_EXPORT") && !strcmp(getenv("WTAMD_BW_EXPORT"), "kernel"));
    int rc = wt_pipe_check(p, s, b);
    if (rc == WTAMD_OK) rc = wt_pipe_reserve(p, s, b);
    if (rc == WTAMD_OK) rc = wt_pipe_rebind(p, s, b);
    if (rc == WTAMD_OK) rc = wt_pipe_upload(p, s, b);
    if (rc == WTAMD_OK) rc = wt_pipe_compute(p, s, b);
    if (rc != WTAMD_OK) return rc;
    s.export_pending = bw && sdma_out && !p->tile && !s.integrated;
    rc = wt_pipe_ship(p, s, s.e_cnt, p->integrate, true);
    if (rc != WTAMD_OK) return rc;

    s.n_int = b.n; s.f64 = f64; s.err = WTAMD_OK;
    if (redo) return WTAMD_OK;
    s.state = 2;
    p->acquired = -1;
    p->head = (p->head + 1) % (int) p->slots.size();
    p->in_flight++;
    p->st.batches++;
    if (!bw) p->st.intervals += b.n;    // (file-byte batches: counted when collected, the device knows)
    if (s.used_delta) p->st.delta_batches++;
    return WTAMD_OK;
}

// Waits for the submitted batch of slot s (and, for file-byte batches whose runs travel by copy engine, asks for them
// once their count is known).
static int wt_pipe_wait_slot(wtamd_pipe *p, WtSlot &s) {
    int rc = WTAMD_OK;
    if (s.integrated) {
        rc = wt_wait_event(s.e_cnt, "batch kernels");
        if (rc == WTAMD_OK) s.ts->h_counters[WT_CTR_EXPORTED] = s.ts->h_counters[WT_CTR_RUNS];
    } else if (s.export_pending) {
        s.export_pending = false;
        rc = wt_wait_event(s.e_cnt, "batch kernels");
        if (rc == WTAMD_OK) {
            unsigned long long *hc = s.ts->h_counters;
            if (!s.compressed) hc[WT_CTR_EXPORTED] = hc[WT_CTR_RUNS];
            if ((int64_t) hc[WT_CTR_EXPORTED] > s.ocap) hc[WT_CTR_EXPORTED] = (unsigned long long) s.ocap;
            const size_t nr = (size_t) hc[WT_CTR_EXPORTED];
            const bool cz = s.compressed;
            hipError_t e = hipEventRecord(s.e_d0, p->s_out);
            if (e == hipSuccess && nr > 0) {
                e = hipMemcpyAsync(s.h_os, cz ? s.d_cs : s.d_os, sizeof(int32_t) * nr, hipMemcpyDeviceToHost, p->s_out);
                if (e == hipSuccess) e = hipMemcpyAsync(s.h_of, cz ? s.d_cf : s.d_of, sizeof(int32_t) * nr, hipMemcpyDeviceToHost, p->s_out);
                if (e == hipSuccess) e = hipMemcpyAsync(s.h_ov, cz ? s.d_cv : s.d_ov, sizeof(double) * nr, hipMemcpyDeviceToHost, p->s_out);
            }
            if (e == hipSuccess) e = hipEventRecord(s.e_d1, p->s_out);
            if (e != hipSuccess) rc = wt_fail(WTAMD_ERR_HIP, std::string("copy-engine export: ") + hipGetErrorString(e));
        }
    }
    if (rc == WTAMD_OK && !s.integrated) rc = wt_wait_event(s.e_d1, "batch");
    return rc;
}

int wtamd_pipe_collect(wtamd_pipe *p, wtamd_pipe_result *out) {
    WtDevGuard dev_guard_(p ? p->device : -1);
    if (!p || !out) return wt_fail(WTAMD_ERR_ARG, "NULL argument");
    if (p->in_flight <= 0) return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_collect: nothing in flight");
    if (p->held) return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_collect: the previous result was not released");
    WtSlot &s = p->slots[(size_t) p->tail];
    if (s.state != 2) return wt_fail(WTAMD_ERR_INTERNAL, "wtamd_pipe_collect: slot order corrupted");
    const auto t_wait0 = std::chrono::steady_clock::now();
    int rc = wt_pipe_wait_slot(p, s);
    if (rc == WTAMD_OK && s.bw && s.h_bw_status[0] == WT_BW_ERR_CAPACITY && s.dcap < s.bw_bound) {
        // more intervals than the run lists sized by density hold (the device wrote nothing): once more, at the bound
        p->bw_density = 2.0;
        p->bw_redone++;
        rc = wt_pipe_submit_impl(p, 0, s.ts->range_lo[0], s.ts->range_hi[0], (const wtamd_bw_track *) s.h_bw, s.bw_bytes, s.bw_secs, &s);
        if (rc == WTAMD_OK) rc = wt_pipe_wait_slot(p, s);
    }
    s.state = 3;
    p->in_flight--;
    p->held = 1;
    if (rc != WTAMD_OK) return rc;
    p->last_bw_err = 0;
    if (s.bw) {
        const unsigned long long e = s.h_bw_status[0];
        if (e) {
            p->last_bw_err = e == ~0ull ? ~0u : (unsigned) e;
            std::string why = "BigWig sections could not be decoded on the device:";
            if (e == ~0ull) why += " decode kernels did not report";
            else {
                if (e & WT_BW_ERR_INFLATE) why += " corrupt zlib stream;";
                if (e & WT_BW_ERR_SECTION) why += " malformed section;";
                if (e & WT_BW_ERR_EXTENT) why += " items outside their index leaf / out of order (WTAMD_BW_DEVICE=0 selects the host decoder);";
                if (e & WT_BW_ERR_COORD) why += " coordinate above the supported maximum;";
                if (e & WT_BW_ERR_CAPACITY) why += " more intervals than the host's bound;";
            }
            return wt_fail(WTAMD_ERR_INTERNAL, why);
        }
        s.n_int = (int64_t) s.h_bw_status[1];
        if (s.bw_bound > 0 && p->bw_density < 1.0) {
            const double d = (double) s.n_int / (double) s.bw_bound;
            if (d > p->bw_density) p->bw_density = d;
        }
        p->st.intervals += s.n_int;
        p->st.bw_sections += s.bw_secs;
        float msb = 0;
        if (hipEventElapsedTime(&msb, s.e_bw0, s.e_bw1) == hipSuccess) p->st.bw_decode_ms += msb;
    }
    rc = wt_pipe_finish(p, s);
    if (rc != WTAMD_OK) return rc;
    p->st.host_wait_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_wait0).count();
    float ms = 0;
    if (hipEventElapsedTime(&ms, s.e_h0, s.e_h1) == hipSuccess) p->st.h2d_ms += ms;
    if (hipEventElapsedTime(&ms, s.e_k0, s.e_cnt) == hipSuccess) p->st.kernel_ms += ms;
    if (!s.integrated && hipEventElapsedTime(&ms, s.e_d0, s.e_d1) == hipSuccess) p->st.d2h_ms += ms;
    p->st.runs += s.n_runs;
    p->st.covered_bp += s.covered;
    p->st.d2h_bytes += s.integrated ? (int64_t) (sizeof(unsigned long long) * WT_CTR_N + 48) : s.n_runs * (16 + (p->tile ? 9 * (int64_t) p->cfg.n_tracks : 0));
    out->n_runs = s.n_runs;
    out->integ_valid = s.integrated ? 1 : 0;
    out->reserved = 0;
    for (int k = 0; k < 6; k++) out->integ[k] = s.integrated ? s.h_integ[k] : 0.0;
    if (s.integrated && !p->tile && s.integ_mode != 2) { out->integ[2] = out->integ[3] = out->integ[4] = out->integ[5] = 0.0; }
    out->start = s.integrated ? nullptr : s.h_os; out->finish = s.integrated ? nullptr : s.h_of; out->value = s.integrated ? nullptr : s.h_ov;
    out->tile = (p->tile && !s.integrated) ? s.h_tile : nullptr;
    out->inplay = (p->tile && !s.integrated) ? s.h_ip : nullptr;
    out->covered_bp = s.covered;
    out->n_intervals = s.n_int;
    return WTAMD_OK;
}

int wtamd_pipe_release(wtamd_pipe *p) {
    if (!p || !p->held) return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_release: nothing to release");
    p->slots[(size_t) p->tail].state = 0;
    p->held = 0;
    p->tail = (p->tail + 1) % (int) p->slots.size();
    return WTAMD_OK;
}

int wtamd_pipe_in_flight(const wtamd_pipe *p) { return p ? p->in_flight : 0; }

int wtamd_pipe_set_compress(wtamd_pipe *p, int on) {
    if (!p) return wt_fail(WTAMD_ERR_ARG, "NULL argument");
    if (on && p->tile) return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_set_compress: the Multiplexer tile cannot be compressed");
    p->compress = on != 0;
    return WTAMD_OK;
}

int wtamd_pipe_set_integrate(wtamd_pipe *p, int on) {
    if (!p) return wt_fail(WTAMD_ERR_ARG, "NULL argument");
    if (on && p->tile && p->cfg.n_tracks != 2) return wt_fail(WTAMD_ERR_ARG, "the fused Pearson integrator needs a Multiplexer of exactly two tracks");
    if (on == 2 && p->tile) return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_set_integrate: mode 2 (run moments) needs a reducer, not a Multiplexer tile");
    p->integrate = on == 2 ? 2 : on != 0;
    return WTAMD_OK;
}

int wtamd_pipe_integrate_modes(const wtamd_pipe *p) {
    if (!p) return 0;
    return p->tile ? 1 : 2;
}

int wtamd_pipe_integrate_held(wtamd_pipe *p, double *integ) {
    WtDevGuard dev_guard_(p ? p->device : -1);
    if (!p || !integ) return wt_fail(WTAMD_ERR_ARG, "NULL argument");
    if (!p->held) return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_integrate_held: no collected batch");
    WtSlot &s = p->slots[(size_t) p->tail];
    for (int k = 0; k < 6; k++) integ[k] = 0.0;
    const int mode = p->integrate == 2 ? 2 : 1;
    if (!s.integrated || s.integ_mode != mode) {
        // the device still holds the batch's runs (d_os / d_of / d_ov, the tile): integrate them there, now
        int rc = wt_pipe_enqueue_integ(p, s, p->s_comp, mode);
        if (rc != WTAMD_OK) return rc;
        WT_HIP(hipEventRecord(s.e_patch, p->s_comp));
        rc = wt_wait_event(s.e_patch, "integrals of the held batch");
        if (rc != WTAMD_OK) return rc;
    }
    for (int k = 0; k < (p->tile || mode == 2 ? 6 : 2); k++) integ[k] = s.h_integ[k];
    return WTAMD_OK;
}

int wtamd_pipe_set_map(wtamd_pipe *p, const wtamd_map_chain *chains) {
    WtDevGuard dev_guard_(p ? p->device : -1);
    if (!p) return wt_fail(WTAMD_ERR_ARG, "NULL argument");
    if (p->in_flight > 0 || p->acquired >= 0) return wt_fail(WTAMD_ERR_ARG, "wtamd_pipe_set_map: batches in flight");
    if (p->d_chains) { (void) wt_dev_free(p->d_chains); p->d_chains = nullptr; p->map_drops = false; p->map_f32 = false; }
    if (!chains) return WTAMD_OK;
    bool any = false;
    for (int t = 0; t < p->cfg.n_tracks; t++) any = any || chains[t].n_ops != 0;
    if (!any) return WTAMD_OK;
    return wt_map_upload_chains(chains, p->cfg.n_tracks, &p->d_chains, &p->map_drops, &p->map_f32);
}

void *wtamd_host_alloc(size_t bytes) {
    void *q = nullptr;
    if (wt_host_alloc(&q, bytes ? bytes : 1) != hipSuccess) return nullptr;
    return q;
}

void wtamd_host_free(void *q) {
    if (q) wt_host_free(q);
}

// (wtamd_pool_trim / wtamd_pool_stats: wt_pool.hip, with the pools)

int wtamd_pipe_get_stats(const wtamd_pipe *p, wtamd_pipe_stats *out) {
    if (!p || !out) return wt_fail(WTAMD_ERR_ARG, "NULL argument");
    *out = p->st;
    return WTAMD_OK;
}

}  // extern "C"
