// wt_mtext.hip -- multi-column wig, bedGraph and paste text on the device: the reference's Multiplexer writer (printBlock,
// src/mWigWriter.c:56-133; `mwrite`, `mwrite_bg`, `apply_paste`) over a tile in HBM.  The passes and the door are written once
// in csrc/wt_mtext.h (which tests/mtext_emu.cpp also compiles for the CPU); this unit gives every pass its kernel; the launcher
// of the door, the report of its result and the staging of the *_host entries are those of csrc/wt_runs_host.h.  Temporary
// device memory comes from the pool (wt_pool.h).  wtamd_trackset_mtext materialises the tile through the engine's entry
// wt_multiplex_device (wt_trackset.h) and prints it where it lies.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "wt_runs_host.h"
#include "wt_trackset.h"
#include "wt_mtext.h"

namespace {

template <int K>
__global__ void __launch_bounds__(WTM_BLOCK) wt_mtext_kernel(WtmArgs a) {
    __shared__ WtmLds lds;
    wtm_run_block(K, a, (long long) blockIdx.x, &lds);
}

struct HipMtextLauncher : WtRunsLauncher {
    template <int K> bool launch(long long blocks, const WtmArgs &a) { return WtRunsLauncher::launch(wt_mtext_kernel<K>, WTM_BLOCK, blocks, a); }
    bool run_mtext(int kernel, long long blocks, const WtmArgs &a) {
        switch (kernel) {
        case WTM_K_CELLS: return launch<WTM_K_CELLS>(blocks, a);
        case WTM_K_MODE: return launch<WTM_K_MODE>(blocks, a);
        case WTM_K_SCAN: return launch<WTM_K_SCAN>(blocks, a);
        case WTM_K_EMIT: return launch<WTM_K_EMIT>(blocks, a);
        default: return false;
        }
    }
};

static_assert(sizeof(wtamd_text_state) == sizeof(WtxState), "wtamd_text_state is WtxState");
static_assert(WTAMD_MTEXT_MAX_WIDTH == WTM_MAX_WIDTH && WTAMD_MTEXT_BEDGRAPH == WTX_BEDGRAPH && WTAMD_MTEXT_STRICT == WTM_STRICT, "the header's constants");

int mtext_report(const char *door, int rc, const char *why) {
    if (rc == 3) return wt_fail(WTAMD_ERR_CAPACITY, std::string(door) + ": the text buffer is too small (*n_bytes holds the size needed)");
    return wt_runs_report(door, rc, why);
}

}  // namespace

extern "C" {

int wtamd_tile_text(int64_t n_seg, const int64_t *seg_off, const char *const *seg_name, const int32_t *start, const int32_t *finish,
                    const double *values, int32_t width, const char *prefix, const int64_t *prefix_off, uint32_t flags, wtamd_text_state *state,
                    char *text, int64_t capacity, int64_t *n_bytes, int64_t *n_wide, void *stream) {
    HipMtextLauncher l{{(hipStream_t) stream, __FILE__}};
    const char *why = "";
    const int rc = wtm_door(l, (long long) n_seg, seg_off, seg_name, start, finish, values, (int) width, prefix, prefix_off, (unsigned int) flags,
                            (WtxState *) state, text, (long long) capacity, n_bytes, n_wide, &why);
    return mtext_report("wtamd_tile_text", rc, why);
}

// Everything in HOST memory: device memory from the pool, copies and the call on the null stream.
int wtamd_tile_text_host(int64_t n_seg, const int64_t *seg_off, const char *const *seg_name, const int32_t *start, const int32_t *finish,
                         const double *values, int32_t width, const char *prefix, const int64_t *prefix_off, uint32_t flags,
                         wtamd_text_state *state, char *text, int64_t capacity, int64_t *n_bytes, int64_t *n_wide) {
    const char *bad = wtm_check((long long) n_seg, seg_off, seg_name, start, finish, values, (int) width, prefix, prefix_off, (unsigned int) flags,
                                (const WtxState *) state, text, (long long) capacity, n_bytes, n_wide);
    if (*bad) return wt_fail(WTAMD_ERR_ARG, std::string("wtamd_tile_text_host: ") + bad);
    HipMtextLauncher l{{nullptr, __FILE__}};
    WcvScope<HipMtextLauncher> sc(l);
    WtDevRuns in;
    char *d_text = nullptr, *d_prefix = nullptr;
    double *d_values = nullptr;
    int64_t *d_poff = nullptr;
    const int64_t n = n_seg ? seg_off[n_seg] : 0;
    if (const int e = wt_stage_runs("wtamd_tile_text_host", sc, n, start, finish, nullptr, false, &in)) return e;
    const int64_t n_pre = prefix && n > 0 ? prefix_off[n] : 0;
    if (prefix && n > 0) {
        if (prefix_off[0] < 0) return wt_fail(WTAMD_ERR_ARG, "wtamd_tile_text_host: prefix offsets start below 0");
        for (int64_t i = 0; i < n; i++)
            if (prefix_off[i + 1] < prefix_off[i]) return wt_fail(WTAMD_ERR_ARG, "wtamd_tile_text_host: prefix offsets decrease");
    }
    if (!sc.get(&d_text, (size_t) capacity) || !sc.get(&d_values, (size_t) (n * width)) || (prefix && (!sc.get(&d_prefix, (size_t) n_pre) || !sc.get(&d_poff, (size_t) n + 1))))
        return wt_fail(WTAMD_ERR_HIP, "wtamd_tile_text_host: out of device memory");
    if (n > 0) {
        WT_HIP(hipMemcpy(d_values, values, sizeof(double) * (size_t) (n * width), hipMemcpyHostToDevice));
        if (prefix) {
            if (n_pre > 0) WT_HIP(hipMemcpy(d_prefix, prefix, (size_t) n_pre, hipMemcpyHostToDevice));
            WT_HIP(hipMemcpy(d_poff, prefix_off, sizeof(int64_t) * ((size_t) n + 1), hipMemcpyHostToDevice));
        }
    }
    const int rc = wtamd_tile_text(n_seg, seg_off, seg_name, in.start, in.finish, d_values, width, d_prefix, d_poff, flags, state, d_text, capacity,
                                   n_bytes, n_wide, nullptr);
    if (rc != WTAMD_OK) return rc;
    if (*n_bytes > 0) WT_HIP(hipMemcpy(text, d_text, (size_t) *n_bytes, hipMemcpyDeviceToHost));
    l.quiet = true;             // (the call waited for its stream and the copy home for the device: the buffers are idle)
    return WTAMD_OK;
}

int wtamd_trackset_mtext(wtamd_trackset *ts, const char *const *chrom_name, uint32_t flags, wtamd_text_state *state, char *text, int64_t capacity,
                         int64_t *n_bytes, int64_t *n_wide, int64_t *n_runs, void *stream) {
    if (!ts || !chrom_name || !n_bytes || !n_wide) return wt_fail(WTAMD_ERR_ARG, "wtamd_trackset_mtext: NULL argument");
    if (flags & ~(WTAMD_MTEXT_BEDGRAPH | WTAMD_MTEXT_STRICT)) return wt_fail(WTAMD_ERR_ARG, "wtamd_trackset_mtext: unknown flag");
    if (ts->n_tracks < 1 || ts->n_tracks > WTAMD_MTEXT_MAX_WIDTH) return wt_fail(WTAMD_ERR_ARG, "wtamd_trackset_mtext: more tracks than WTAMD_MTEXT_MAX_WIDTH");
    hipStream_t s = (hipStream_t) stream;
    HipMtextLauncher l{{s, __FILE__}};
    WcvScope<HipMtextLauncher> sc(l);
    const int64_t cap = wtamd_trackset_max_runs(ts), alloc = cap > 0 ? cap : 1;
    const int N = ts->n_tracks;
    wtamd_runs d{};
    d.capacity = cap;
    double *d_tile = nullptr;
    uint8_t *d_inplay = nullptr;
    if (!sc.get(&d.start, (size_t) alloc) || !sc.get(&d.finish, (size_t) alloc) || !sc.get(&d.value, (size_t) alloc) ||
        !sc.get(&d.chrom_run_off, (size_t) ts->n_chrom + 1) || !sc.get(&d_tile, (size_t) alloc * N) || !sc.get(&d_inplay, (size_t) alloc * N))
        return wt_fail(WTAMD_ERR_HIP, "wtamd_trackset_mtext: out of device memory");
    int64_t n = 0;
    l.quiet = false;
    const int rc = wt_multiplex_device(ts, (flags & WTAMD_MTEXT_STRICT) ? WTAMD_STRICT_SET0 : 0u, &d, d_tile, d_inplay, &n, s);
    if (rc != WTAMD_OK) return rc;
    std::vector<int64_t> seg((size_t) ts->n_chrom + 1, 0);
    WT_HIP(hipMemcpyAsync(seg.data(), d.chrom_run_off, sizeof(int64_t) * seg.size(), hipMemcpyDeviceToHost, s));
    WT_HIP(hipStreamSynchronize(s));
    if (n_runs) *n_runs = n;
    return wtamd_tile_text(ts->n_chrom, seg.data(), chrom_name, d.start, d.finish, d_tile, N, nullptr, nullptr, flags & WTAMD_MTEXT_BEDGRAPH, state, text,
                           capacity, n_bytes, n_wide, stream);
}

int wtamd_trackset_mtext_host(wtamd_trackset *ts, const char *const *chrom_name, uint32_t flags, wtamd_text_state *state, char *text, int64_t capacity,
                              int64_t *n_bytes, int64_t *n_wide, int64_t *n_runs) {
    if (!n_bytes || capacity < 0 || (capacity > 0 && !text)) return wt_fail(WTAMD_ERR_ARG, "wtamd_trackset_mtext_host: bad argument");
    HipMtextLauncher l{{nullptr, __FILE__}};
    WcvScope<HipMtextLauncher> sc(l);
    char *d_text = nullptr;
    if (!sc.get(&d_text, (size_t) capacity)) return wt_fail(WTAMD_ERR_HIP, "wtamd_trackset_mtext_host: out of device memory");
    const int rc = wtamd_trackset_mtext(ts, chrom_name, flags, state, d_text, capacity, n_bytes, n_wide, n_runs, nullptr);
    if (rc != WTAMD_OK) return rc;
    if (*n_bytes > 0) WT_HIP(hipMemcpy(text, d_text, (size_t) *n_bytes, hipMemcpyDeviceToHost));
    l.quiet = true;
    return WTAMD_OK;
}

}  // extern "C"
