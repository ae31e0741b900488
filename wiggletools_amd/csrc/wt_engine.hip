// wt_engine.hip -- the bulk C ABI (wtamd_*) of include/wiggletools_amd.h: planner glue, launches, the patch / probe state
// machine and the small kernels below.  Its internal interface is wt_trackset.h: the streaming pipeline (wt_pipe.hip) is a
// unit of its own built on it.  The reducing kernels live in units of their own behind wt_kernels.h, the integrators
// (AUC, Pearson, run moments) in wt_moments.hip.  Compiled only by hipcc --offload-arch=gfx950.
//
// Kernels
//   wt_index_kernel     window index (widx): contiguous span of input runs per block, 4 per lane
//   wt_index_coarse_kernel / wt_index_search_kernel   the same index by search
//   wt_extents_kernel   first start / last finish per (chrom, track) segment
//   wt_win_chrom_kernel / wt_clear_kernel   the window -> chromosome table; what a launch clears first
//   wt_validate_kernel  input contract (sorted, non-overlapping, positive length)
#include <hip/hip_runtime.h>

#include <cstdio>
#include <thread>
#include <atomic>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "wt_host.h"
#include "wt_trackset.h"
#include "wt_core.h"
#include "wt_plan.h"
#include "wt_kernels.h"
#include "wt_devscope.h"
#include "wt_pool.h"

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------
// Each block owns ONE contiguous span of intervals: a single binary search finds the
// (chrom,track) segment of its first interval, every lane then walks its cursor forward.  The
// finish[] reads of the next sub-chunk are in flight while the current one is applied.
#ifndef WT_INDEX_UNROLL
#define WT_INDEX_UNROLL 2
#endif
#define WT_INDEX_CHUNK (256 * 4 * WT_INDEX_UNROLL)
__global__ void __launch_bounds__(256) wt_index_kernel(const WtParams P, long long total, long long span) {
    // a batch whose run lists were compacted on device (operator chains that drop runs) holds fewer
    // intervals than the host counted: the device's seg_off[] is the authority
    const long long dev_total = P.seg_off[(long long) P.n_chrom * P.n_tracks];
    if (total > dev_total) total = dev_total;
    const long long begin0 = (long long) blockIdx.x * span;
    long long end0 = begin0 + span;
    if (end0 > total) end0 = total;
    if (begin0 >= end0) return;
    WtIndexCursor cur;
    wt_index_cursor_set(P, cur, wt_index_find_segment(P, begin0));
    // Every lane takes 4 CONSECUTIVE runs per sub-chunk: one 16-byte load of finish[] plus the
    // predecessor's finish (the kernel was instruction-bound on per-element 64-bit addressing).
    // begin0 is a multiple of WT_INDEX_CHUNK, so the vectors never straddle `total` unguarded.
    struct __attribute__((packed, aligned(4))) V4 { int32_t x[4]; };
    V4 f[WT_INDEX_UNROLL], nf[WT_INDEX_UNROLL];
    int32_t pf[WT_INDEX_UNROLL], npf[WT_INDEX_UNROLL];
    // FULL sub-chunks: unconditional loads.  (Round 3, read off the ISA: with `if (more) fetch(next)` and the
    // per-lane tail guards around the loads, the compiler could not count the loads in flight and waited for
    // ALL of them before applying the current sub-chunk -- the prefetch overlapped nothing, and 1, 2 or 4
    // vectors per lane made no difference.)  A prefetch past the last full sub-chunk re-reads that one.
    const long long n_full = (end0 - begin0) / WT_INDEX_CHUNK;
    auto fetch = [&](long long base, V4 (&v)[WT_INDEX_UNROLL], int32_t (&p)[WT_INDEX_UNROLL]) {
#pragma unroll
        for (int u = 0; u < WT_INDEX_UNROLL; u++) {
            const long long g = base + 4ll * (threadIdx.x + 256 * u);
            v[u] = *(const V4 *) (P.finish + g);
            p[u] = P.finish[g > 0 ? g - 1 : 0];
        }
    };
    if (n_full > 0) {
        const long long last_full = begin0 + (n_full - 1) * WT_INDEX_CHUNK;
        fetch(begin0, f, pf);
        for (long long begin = begin0; begin <= last_full; begin += WT_INDEX_CHUNK) {
            const long long nb = begin + WT_INDEX_CHUNK;
            fetch(nb <= last_full ? nb : last_full, nf, npf);
#pragma unroll
            for (int u = 0; u < WT_INDEX_UNROLL; u++) {
                const long long g = begin + 4ll * (threadIdx.x + 256 * u);
                int32_t prev = pf[u];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    wt_index_apply(P, cur, g + q, f[u].x[q], prev);
                    prev = f[u].x[q];
                }
            }
#pragma unroll
            for (int u = 0; u < WT_INDEX_UNROLL; u++) { f[u] = nf[u]; pf[u] = npf[u]; }
        }
    }
    // the partial sub-chunk at the end of the span (only the last block of a launch has one)
    const long long begin = begin0 + n_full * WT_INDEX_CHUNK;
    if (begin < end0) {
#pragma unroll
        for (int u = 0; u < WT_INDEX_UNROLL; u++) {
            const long long g = begin + 4ll * (threadIdx.x + 256 * u);
            int32_t prev = (g < end0 && g > 0) ? P.finish[g - 1] : 0;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                if (g + q < end0) {
                    const int32_t fq = P.finish[g + q];
                    wt_index_apply(P, cur, g + q, fq, prev);
                    prev = fq;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Window index by SEARCH (round 3).  widx[row(b)][track] is the lower bound of the boundary b = cbase + m * W
// in the track's finish[] (wt_index_apply's claims, restated), so nothing obliges the kernel to read every
// finish: at a mean run of 16 bp the scan above reads 256 entries (1 KB) per boundary and stays near
// 3.3 TB/s whatever its loads look like (1, 2 or 4 vectors in flight, long or short spans per block).
//   coarse  every 64th row of every track by an interpolation search over the track's whole segment
//           (one lane each; ~1 % of the boundaries);
//   fine    a wave owns the 64 rows between two coarse rows of ONE track: each lane interpolates its boundary
//           between the two coarse answers, corrects the guess twice by the bracket's density (the linear guess is
//           ~90 runs off at a mean run of 16 bp, the corrected one a few) and gallops / bisects from there
//           (wt_isearch.h) -- 5 dependent probes on average where the gallop alone took 11, almost all inside one
//           or two 128-byte lines; the 16 waves of a workgroup (16 neighbouring tracks, same rows) exchange
//           through LDS so that a row is written as one 64-byte piece.
// (A first version found the bracket with a cooperative 64-ary search per wave: 17.7 ms against the scan's
// 22-27 -- its 64 probes per step were 64 cache lines per step.)  Same result as the scan by construction;
// WTAMD_INDEX=scan selects the scan, WTAMD_INDEX_CHECK=1 runs both and compares (tests).
// ---------------------------------------------------------------------------
#define WT_ISEARCH_ROWS 64
#define WT_ISEARCH_TRACKS 16

// chromosome of an index row: the rows of chromosome ch start at c_first_win[ch] + ch
__device__ __forceinline__ int wt_index_row_chrom(const WtParams &P, long long row) {
    int lo = 0;
    for (int hi = P.n_chrom; hi - lo > 1;) {
        const int mid = (lo + hi) >> 1;
        if (P.c_first_win[mid] + mid <= row) lo = mid; else hi = mid;
    }
    return lo;
}

// the chromosome of an index row, its boundary and the track's finish[] segment.  One chromosome (wave-uniform branch): no
// search, and the tables' entries are loads at a uniform address
struct WtIndexRow { int ch; long long b, s0, n; };
__device__ __forceinline__ WtIndexRow wt_index_row(const WtParams &P, long long row, int i) {
    WtIndexRow r;
    r.ch = P.n_chrom == 1 ? 0 : wt_index_row_chrom(P, row);
    const long long m = row - (P.c_first_win[r.ch] + r.ch);
    const long long seg = (long long) r.ch * P.n_tracks + i;
    r.s0 = P.seg_off[seg];
    r.n = P.seg_off[seg + 1] - r.s0;
    r.b = (long long) P.cbase[r.ch] + (m << P.logW);
    return r;
}

// coarse[strip][track]: the index entry of row strip * 64.  An interpolation search (wt_isearch.h) from the segment's end
// points: the density is the segment's, the first guess linear between its first and last finish -- 2 + up to ~8 dependent
// probes where the plain binary search took log2(n) = 21 to 24, on a grid far too small to hide them.
__global__ void __launch_bounds__(256) wt_index_coarse_kernel(const WtParams P, long long n_strips, uint32_t *coarse) {
    const long long t = (long long) blockIdx.x * 256 + threadIdx.x;
    const int N = P.n_tracks;
    if (t >= n_strips * N) return;
    const long long strip = t / N;
    const int i = (int) (t - strip * N);
    const WtIndexRow r = wt_index_row(P, strip * WT_ISEARCH_ROWS, i);
    const int32_t *fin = P.finish + r.s0;
    long long g = r.n >> 1;
    float density = 0.0f;
    if (r.n > 1) {
        const long long f0 = fin[0], f1 = fin[r.n - 1];
        if (f1 > f0) {
            density = (float) (r.n - 1) / (float) (f1 - f0);
            const float guess = fminf(fmaxf((float) (r.b - f0) * density, 0.0f), (float) (r.n - 1));
            g = (long long) guess;
            if (g > r.n - 1) g = r.n - 1;
        }
    }
    coarse[t] = (uint32_t) wt_interp_lower_bound(WtFinArray{fin}, 0, r.n, g, r.b, density);
}

__global__ void __launch_bounds__(WT_ISEARCH_ROWS * WT_ISEARCH_TRACKS) wt_index_search_kernel(const WtParams P, long long n_rows, long long n_strips,
                                                                                              const uint32_t *coarse) {
    __shared__ uint32_t out[WT_ISEARCH_ROWS][WT_ISEARCH_TRACKS + 1];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // (told to the compiler: what hangs on the track alone is scalar)
    const int N = P.n_tracks;
    const long long strip = blockIdx.x;
    const long long r0 = strip * WT_ISEARCH_ROWS;
    const int i = (int) blockIdx.y * WT_ISEARCH_TRACKS + wave;
    if (i < N) {                                    // (wave-uniform)
        long long row = r0 + lane;
        if (row > n_rows - 1) row = n_rows - 1;     // the last strip: duplicates of the last row, not stored
        const WtIndexRow r = wt_index_row(P, row, i);
        const int32_t *fin = P.finish + r.s0;
        // the bracket: the coarse answers of this strip's and the next strip's first rows (wave-uniform loads), where they
        // belong to the lane's chromosome (a strip may straddle a chromosome edge)
        const bool have_next = strip + 1 < n_strips;
        const long long cA = (long long) coarse[strip * N + i];
        const long long cB = have_next ? (long long) coarse[(strip + 1) * N + i] : 0;
        bool real_a = true, real_b = have_next;
        if (P.n_chrom != 1) {
            const int ch_first = __shfl(r.ch, 0);
            const int ch_next = have_next ? wt_index_row_chrom(P, r0 + WT_ISEARCH_ROWS) : -1;
            real_a = r.ch == ch_first; real_b = r.ch == ch_next;
        }
        const long long A = real_a ? cA : 0;
        const long long B = real_b ? cB : r.n;
        long long g = (real_a && real_b) ? A + (((B - A) * lane) >> 6) : (A + B) >> 1;
        if (g > B - 1) g = B - 1;
        // both ends real: the bracket's B - A runs lie between two boundaries 64 windows apart -- its density moves the guess
        // (wt_interp_lower_bound) before the gallop; at a chromosome's edge the gallop runs alone, as it always did
        const float density = (real_a && real_b) ? (float) (B - A) / (float) ((long long) WT_ISEARCH_ROWS << P.logW) : 0.0f;
        out[lane][wave] = (uint32_t) wt_interp_lower_bound(WtFinArray{fin}, A, B, g, r.b, density);
    }
    __syncthreads();
    const int orow = tid / WT_ISEARCH_TRACKS, ocol = tid % WT_ISEARCH_TRACKS;
    const long long row = r0 + orow;
    const int track = (int) blockIdx.y * WT_ISEARCH_TRACKS + ocol;
    if (row < n_rows && track < N) P.widx[(size_t) row * N + track] = out[orow][ocol];
}

// check mode: number of entries in which two indices differ
__global__ void __launch_bounds__(256) wt_index_compare_kernel(const uint32_t *a, const uint32_t *b, long long n, unsigned long long *diff) {
    const long long t = (long long) blockIdx.x * 256 + threadIdx.x;
    if (t < n && a[t] != b[t]) atomicAdd(diff, 1ull);
}

__global__ void __launch_bounds__(256) wt_extents_kernel(const int64_t *seg_off, const int32_t *start,
                                                          const int32_t *finish, long long n_seg,
                                                          int32_t *first_start, int32_t *last_finish) {
    const long long s = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seg) return;
    const long long lo = seg_off[s], hi = seg_off[s + 1];
    first_start[s] = hi > lo ? start[lo] : 0;
    last_finish[s] = hi > lo ? finish[hi - 1] : 0;
}

// win_chrom[k]: the chromosome of window k, from c_first_win[] (strictly increasing: every chromosome has a window).  The
// table is filled where it is read: a track set of several chromosomes uploads n_chrom entries instead of n_windows.
__global__ void __launch_bounds__(256) wt_win_chrom_kernel(const int64_t *c_first_win, int n_chrom, long long n_windows, int32_t *win_chrom) {
    const long long k = (long long) blockIdx.x * 256 + threadIdx.x;
    if (k >= n_windows) return;
    int lo = 0;
    for (int hi = n_chrom; hi - lo > 1;) {
        const int mid = (lo + hi) >> 1;
        if (c_first_win[mid] <= k) lo = mid; else hi = mid;
    }
    win_chrom[k] = lo;
}

// What every launch clears first -- the counters, the per-chromosome run offsets, the look-back words -- in ONE kernel: as
// three hipMemsetAsync calls they stood between the index and the reducing kernel for 30 us of every launch (13 us of fill
// kernels, the rest the gaps between them; profiles/fresh_step.md).
__global__ void __launch_bounds__(256) wt_clear_kernel(unsigned long long *counters, int n_counters, int64_t *chrom_run_off, int n_cro,
                                                        unsigned long long *status, long long n_status) {
    const long long t = (long long) blockIdx.x * 256 + threadIdx.x, stride = (long long) gridDim.x * 256;
    for (long long q = t; q < n_status; q += stride) status[q] = 0ull;
    for (long long q = t; q < n_counters; q += stride) counters[q] = 0ull;
    for (long long q = t; q < n_cro; q += stride) chrom_run_off[q] = 0;
}

// Input contract check (sorted, non-overlapping, positive-length runs inside every (chrom, track)
// segment -- anything else is undefined behaviour in the reference's Multiplexer too,
// multiplexer.c:76-96, and bedReader.c:46-49 checks it for text input).  One lane per run.
__global__ void __launch_bounds__(256) wt_validate_kernel(const int32_t *start, const int32_t *finish, const int64_t *seg_off,
                                                           long long n_seg, long long total, unsigned long long *out) {
    const long long g = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    bool bad = finish[g] <= start[g];
    if (!bad && g > 0 && start[g] < finish[g - 1]) {
        long long lo = 0, hi = n_seg;                   // is g the first run of its segment?
        while (hi - lo > 1) {
            const long long mid = (lo + hi) >> 1;
            if (seg_off[mid] <= g) lo = mid; else hi = mid;
        }
        bad = seg_off[lo] != g;
    }
    if (bad) {
        atomicAdd(&out[0], 1ull);
        atomicMin(&out[1], (unsigned long long) g);
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
static thread_local std::string g_last_error;

int wt_fail(int code, const std::string &msg) {
    g_last_error = msg;
    return code;
}

// Device tables come from the device pool and return to it (wt_pool.h).  The pool waits for nothing, so a table that is
// outgrown waits for the device before it returns: once per growth (*quiet: the caller's growth has waited already).
template <class T>
static hipError_t wt_grow(T **p, int64_t *cap, int64_t need, bool *quiet) {
    if (*cap >= need && *p) return hipSuccess;
    int64_t c = *cap * 2;
    if (c < need) c = need;
    if (c < 1) c = 1;
    if (*p) {
        if (!*quiet) {
            const hipError_t eq = wt_pool_quiesce();
            if (eq != hipSuccess) return eq;
            *quiet = true;
        }
        (void) wt_dev_free(*p);
    }
    *p = nullptr; *cap = 0;
    const hipError_t e = wt_dev_alloc(p, sizeof(T) * (size_t) c);
    if (e == hipSuccess) *cap = c;
    return e;
}

// (the caller has waited for the device: wtamd_trackset_destroy)
static void wt_free_windows(WtWindows &w) {
    (void) wt_dev_free(w.d_tabs);          // (d_cbase, d_cnwin, d_chi, d_cfirst, d_win_chrom point into it)
    (void) wt_dev_free(w.d_widx); (void) wt_dev_free(w.d_cidx); (void) wt_dev_free(w.d_status); (void) wt_dev_free(w.d_bad_list); (void) wt_dev_free(w.d_bad_goff);
    if (w.h_tab) wt_host_free(w.h_tab);
    if (w.ev_tab) (void) hipEventDestroy(w.ev_tab);
    w = WtWindows();
}

// (the wtamd_* entries below and, among them, the wt_* functions of wt_trackset.h: those are marked extern "C++")
extern "C" {

const char *wtamd_last_error(void) { return g_last_error.c_str(); }
const char *wtamd_version(void) { return "wiggletools_amd 0.1 (gfx950)"; }

int wtamd_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// The first HIP call of a process brings the runtime up (device discovery, the library's code object, the first hardware
// queues): 170 ms between newMultiplexer and the first batch in the trace of a fresh `mean *.bw` process (round 5,
// tools/cli_cold.py) -- spent AFTER the 100 files had been opened, although neither needs the other.  The callers that
// know GPU work is coming (wtamd_BigWiggleReaders: it opens the files on worker threads) start it on a helper thread
// first; wtamd_pipe_create waits for the helper.  The helper works on the default device (a process that selects another
// one has called into HIP already: the runtime is up and this costs nothing).
__global__ void wt_warm_kernel(int *p) { if (p && threadIdx.x == 4096) *p = 0; }

static std::mutex g_warm_mu;
static std::thread *g_warm_thread = nullptr;
static bool g_warm_started = false;

extern "C++" void wt_warmup_join() {
    std::thread *t = nullptr;
    { std::lock_guard<std::mutex> lk(g_warm_mu); t = g_warm_thread; g_warm_thread = nullptr; }
    if (t) { t->join(); delete t; }
}

// The helper is a new thread: HIP's current device is per thread, so it is told which device to warm -- the one the caller
// selected (wtamd_set_device, or the calling thread's current device when that was set through the runtime, e.g. by
// torch.cuda.set_device in a one-process-per-GPU job).  With several devices visible and none selected the warm-up is skipped:
// a context on GPU 0 from every rank would help nobody.
static std::atomic<int> g_device_chosen{-1};

void wtamd_warmup_async(void) {
    std::lock_guard<std::mutex> lk(g_warm_mu);
    if (g_warm_started || getenv("WTAMD_NO_WARMUP")) return;
    int n = 0, cur = -1;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { (void) hipGetLastError(); return; }
    int ordinal = g_device_chosen.load();
    if (ordinal < 0 && hipGetDevice(&cur) == hipSuccess && (n == 1 || cur > 0)) ordinal = cur;     // (cur == 0 of several: nobody chose yet)
    if (ordinal < 0 || ordinal >= n) return;                    // (not started: a later call, after wtamd_set_device, may)
    g_warm_started = true;
    g_warm_thread = new std::thread([ordinal] {
        if (hipSetDevice(ordinal) != hipSuccess) { (void) hipGetLastError(); return; }
        hipStream_t st[3] = {nullptr, nullptr, nullptr};
        for (auto &s : st)
            if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) s = nullptr;
        for (auto &s : st)
            if (s) hipLaunchKernelGGL(wt_warm_kernel, dim3(1), dim3(64), 0, s, (int *) nullptr);
        for (auto &s : st)
            if (s) { (void) hipStreamSynchronize(s); (void) hipStreamDestroy(s); }
        (void) hipGetLastError();
    });
    atexit(wt_warmup_join);         // (a process that exits before it ever built a pipe must not leave the helper inside the runtime)
}

int wtamd_set_device(int ordinal) {
    wt_warmup_join();               // (a helper still warming another device finishes first)
    WT_HIP(hipSetDevice(ordinal));
    g_device_chosen.store(ordinal);
    return WTAMD_OK;
}

int wtamd_current_device(void) {
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess) { (void) hipGetLastError(); return -1; }
    return d;
}

extern "C++" int wt_trackset_common(const wtamd_tracks *t, wtamd_trackset *ts) {
    if (!t || t->n_chrom < 0 || t->n_tracks <= 0 || !t->seg_off || !t->defaults)
        return wt_fail(WTAMD_ERR_ARG, "wtamd_trackset_create: bad tracks descriptor");
    if (wtamd_device_count() <= 0) return wt_fail(WTAMD_ERR_NODEVICE, "no HIP device visible");
    ts->n_chrom = t->n_chrom;
    ts->n_tracks = t->n_tracks;
    ts->value_f64 = t->value_is_f64 != 0;
    const int64_t n_seg = (int64_t) t->n_chrom * t->n_tracks;
    ts->seg_off.assign(t->seg_off, t->seg_off + n_seg + 1);
    for (int64_t s = 0; s < n_seg; s++)
        if (ts->seg_off[s + 1] < ts->seg_off[s]) return wt_fail(WTAMD_ERR_ARG, "seg_off not monotone");
    ts->n_intervals = ts->seg_off[n_seg] - ts->seg_off[0];
    if (ts->seg_off[0] != 0) return wt_fail(WTAMD_ERR_ARG, "seg_off[0] must be 0");
    ts->defaults.assign(t->defaults, t->defaults + t->n_tracks);
    if (t->range_lo && t->range_hi) {
        ts->range_lo.assign(t->range_lo, t->range_lo + t->n_chrom);
        ts->range_hi.assign(t->range_hi, t->range_hi + t->n_chrom);
    }
    ts->scratch_f32 = !ts->value_f64 && wt_defaults_fit_f32(ts->defaults.data(), ts->n_tracks);
    WT_HIP(hipGetDevice(&ts->device));
    hipDeviceProp_t prop;
    WT_HIP(hipGetDeviceProperties(&prop, ts->device));
    ts->num_cu = prop.multiProcessorCount;
    WT_HIP(wt_dev_alloc(&ts->d_seg_off, sizeof(int64_t) * (n_seg + 1)));
    WT_HIP(hipMemcpy(ts->d_seg_off, ts->seg_off.data(), sizeof(int64_t) * (n_seg + 1), hipMemcpyHostToDevice));
    WT_HIP(wt_dev_alloc(&ts->d_defaults, sizeof(double) * t->n_tracks));
    WT_HIP(hipMemcpy(ts->d_defaults, ts->defaults.data(), sizeof(double) * t->n_tracks, hipMemcpyHostToDevice));
    WT_HIP(wt_dev_alloc(&ts->d_counters, sizeof(unsigned long long) * WT_CTR_N));
    WT_HIP(wt_host_alloc((void **) &ts->h_counters, sizeof(unsigned long long) * WT_CTR_N));
    WT_HIP(wt_host_alloc((void **) &ts->h_debug, sizeof(unsigned long long) * 16));
    memset(ts->h_debug, 0, sizeof(unsigned long long) * 16);
    WT_HIP(wt_dev_alloc(&ts->d_chrom_run_off, sizeof(int64_t) * (t->n_chrom + 1)));
    WT_HIP(hipEventCreate(&ts->ev_i0));
    WT_HIP(hipEventCreate(&ts->ev_i1));
    WT_HIP(hipEventCreate(&ts->ev_r0));
    WT_HIP(hipEventCreate(&ts->ev_r1));
    return WTAMD_OK;
}

// The window arithmetic (w0 + W, look-ahead sentinels) is 32-bit: keep a margin below INT32_MAX.
// Loud, at creation -- a run that close to 2^31 would otherwise be silently lost.
extern "C++" int wt_check_extents(wtamd_trackset *ts) {
    for (size_t q = 0; q < ts->last_finish.size(); q++)
        if (ts->seg_off[q + 1] > ts->seg_off[q] && ts->last_finish[q] > WTAMD_MAX_COORD) {
            const int64_t bad = ts->last_finish[q];
            return wt_fail(WTAMD_ERR_ARG, "run finish " + std::to_string(bad) + " above the supported maximum " +
                           std::to_string((long long) WTAMD_MAX_COORD) + " (2^31 - 65537)");
        }
    return WTAMD_OK;
}

// Device-side (first start, last finish) of every (chrom, track) segment into the host copies: one kernel on the caller's
// stream, one asynchronous copy of both arrays into the track set's pinned buffer, one synchronisation of that stream.
static int wt_refresh_extents_device(wtamd_trackset *ts, hipStream_t s) {
    const int64_t n_seg = (int64_t) ts->n_chrom * ts->n_tracks;
    ts->first_start.assign(n_seg, 0);
    ts->last_finish.assign(n_seg, 0);
    if (n_seg > 0 && ts->n_intervals > 0) {
        const size_t bytes = sizeof(int32_t) * 2 * (size_t) n_seg;
        if (!ts->d_extents) WT_HIP(wt_dev_alloc(&ts->d_extents, bytes));
        if (!ts->h_extents) WT_HIP(wt_host_alloc((void **) &ts->h_extents, bytes));
        hipLaunchKernelGGL(wt_extents_kernel, dim3((unsigned) ((n_seg + 255) / 256)), dim3(256), 0, s,
                           ts->d_seg_off, ts->d_start, ts->d_finish, (long long) n_seg, ts->d_extents, ts->d_extents + n_seg);
        WT_HIP(hipGetLastError());
        WT_HIP(hipMemcpyAsync(ts->h_extents, ts->d_extents, bytes, hipMemcpyDeviceToHost, s));
        WT_HIP(hipStreamSynchronize(s));
        ts->first_start.assign(ts->h_extents, ts->h_extents + n_seg);
        ts->last_finish.assign(ts->h_extents + n_seg, ts->h_extents + 2 * n_seg);
    }
    return WTAMD_OK;
}

static int wt_create_host_impl(const wtamd_tracks *t, wtamd_trackset *ts) {
    int rc = wt_trackset_common(t, ts);
    if (rc != WTAMD_OK) return rc;
    ts->owns = true;
    const int64_t n = ts->n_intervals;
    const size_t vsz = ts->value_f64 ? 8 : 4;
    const int64_t n_alloc = n > 0 ? n : 1;
    WT_HIP(hipMalloc(&ts->d_start, sizeof(int32_t) * n_alloc));
    WT_HIP(hipMalloc(&ts->d_finish, sizeof(int32_t) * n_alloc));
    WT_HIP(hipMalloc(&ts->d_value, vsz * n_alloc));
    if (n > 0) {
        if (!t->start || !t->finish || !t->value) return wt_fail(WTAMD_ERR_ARG, "NULL arrays");
        WT_HIP(hipMemcpy(ts->d_start, t->start, sizeof(int32_t) * n, hipMemcpyHostToDevice));
        WT_HIP(hipMemcpy(ts->d_finish, t->finish, sizeof(int32_t) * n, hipMemcpyHostToDevice));
        WT_HIP(hipMemcpy(ts->d_value, t->value, vsz * n, hipMemcpyHostToDevice));
    }
    const int64_t n_seg = (int64_t) ts->n_chrom * ts->n_tracks;
    ts->first_start.assign(n_seg, 0);
    ts->last_finish.assign(n_seg, 0);
    for (int64_t s = 0; s < n_seg; s++)
        if (ts->seg_off[s + 1] > ts->seg_off[s]) {
            ts->first_start[s] = t->start[ts->seg_off[s]];
            ts->last_finish[s] = t->finish[ts->seg_off[s + 1] - 1];
        }
    return wt_check_extents(ts);
}

int wtamd_trackset_create_host(const wtamd_tracks *t, wtamd_trackset **out) {
    if (!out) return wt_fail(WTAMD_ERR_ARG, "out == NULL");
    wtamd_trackset *ts = new wtamd_trackset();
    const int rc = wt_create_host_impl(t, ts);
    if (rc != WTAMD_OK) { wtamd_trackset_destroy(ts); return rc; }     // every failing path releases what was allocated
    *out = ts;
    return WTAMD_OK;
}

static int wt_create_device_impl(const wtamd_tracks *t, wtamd_trackset *ts) {
    int rc = wt_trackset_common(t, ts);
    if (rc != WTAMD_OK) return rc;
    ts->owns = false;
    ts->d_start = const_cast<int32_t *>(t->start);
    ts->d_finish = const_cast<int32_t *>(t->finish);
    ts->d_value = const_cast<void *>(t->value);
    rc = wt_refresh_extents_device(ts, nullptr);
    if (rc != WTAMD_OK) return rc;
    return wt_check_extents(ts);
}

int wtamd_trackset_create_device(const wtamd_tracks *t, wtamd_trackset **out) {
    if (!out) return wt_fail(WTAMD_ERR_ARG, "out == NULL");
    wtamd_trackset *ts = new wtamd_trackset();
    const int rc = wt_create_device_impl(t, ts);
    if (rc != WTAMD_OK) { wtamd_trackset_destroy(ts); return rc; }
    *out = ts;
    return WTAMD_OK;
}

void wtamd_trackset_destroy(wtamd_trackset *ts) {
    if (!ts) return;
    // The pools' rule (wt_pool.h): a buffer returns only after the device has finished with it.  A launch of this track set may
    // be in flight on any stream (wtamd_reduce without n_runs returns at once), and the first hipFree used to wait for it: the
    // wait is explicit now, once, before the first buffer goes back.
    (void) wt_pool_quiesce();
    if (ts->owns) { (void) hipFree(ts->d_start); (void) hipFree(ts->d_finish); (void) hipFree(ts->d_value); }
    (void) wt_dev_free(ts->d_seg_off); (void) wt_dev_free(ts->d_defaults); (void) wt_dev_free(ts->d_counters); (void) wt_dev_free(ts->d_chrom_run_off);
    (void) wt_dev_free(ts->d_extents);
    (void) hipFree(ts->d_gscratch); (void) hipFree(ts->d_mwu_table);
    for (double *q : ts->mwu_retired) (void) hipFree(q);
    if (ts->h_counters) wt_host_free(ts->h_counters);
    if (ts->h_debug) wt_host_free(ts->h_debug);
    if (ts->h_extents) wt_host_free(ts->h_extents);
    for (auto &kv : ts->windows) wt_free_windows(kv.second);
    if (ts->ev_i0) (void) hipEventDestroy(ts->ev_i0);
    if (ts->ev_i1) (void) hipEventDestroy(ts->ev_i1);
    if (ts->ev_r0) (void) hipEventDestroy(ts->ev_r0);
    if (ts->ev_r1) (void) hipEventDestroy(ts->ev_r1);
    delete ts;
}

static int64_t wt_span(const wtamd_trackset *ts) {
    // sum over chromosomes of (max finish - min start)
    int64_t span = 0;
    for (int c = 0; c < ts->n_chrom; c++) {
        int64_t lo = INT64_MAX, hi = INT64_MIN;
        for (int i = 0; i < ts->n_tracks; i++) {
            const int64_t s = (int64_t) c * ts->n_tracks + i;
            if (ts->seg_off[s + 1] > ts->seg_off[s]) {
                lo = std::min<int64_t>(lo, ts->first_start[s]);
                hi = std::max<int64_t>(hi, ts->last_finish[s]);
            }
        }
        if (lo <= hi) span += hi - lo;
    }
    return span;
}

int64_t wtamd_trackset_max_runs(const wtamd_trackset *ts) {
    if (!ts) return 0;
    // every run starts at an interval start or finish, and no two runs start at the same position
    return std::min<int64_t>(2 * ts->n_intervals, wt_span(ts));
}

// Window tables of width W for the track set's current data.  The device tables come from the device pool, are kept and
// reused (they only ever grow).  The per-chromosome tables travel in ONE asynchronous copy on `s` from this WtWindows' pinned
// staging, packed as they lie at the head of d_tabs; win_chrom[] is filled on the device (all zeros for one chromosome: a
// memset; wt_win_chrom_kernel otherwise).
static int wt_get_windows(wtamd_trackset *ts, int W, WtWindows **out, hipStream_t s = nullptr) {
    WtWindows &w = ts->windows[W];
    *out = &w;
    if (w.tab_valid) return WTAMD_OK;
    wt_make_windows(ts->n_chrom, ts->n_tracks, ts->seg_off.data(), ts->first_start.data(), ts->last_finish.data(), W, w.tab,
                    ts->range_lo.empty() ? nullptr : ts->range_lo.data(),
                    ts->range_hi.empty() ? nullptr : ts->range_hi.data(), false);
    w.indexed = false;
    const int64_t nc = ts->n_chrom > 0 ? ts->n_chrom : 1;
    const int64_t nwin = w.tab.n_windows > 0 ? w.tab.n_windows : 1;
    const int64_t nwidx = (w.tab.n_rows > 0 ? w.tab.n_rows : 1) * (int64_t) ts->n_tracks;
    // layout of the combined table allocation (8-byte aligned pieces)
    auto up8 = [](int64_t x) { return (x + 7) & ~(int64_t) 7; };
    bool quiet = false;         // this growth has waited for the device (once, before the first table returns to the pool)
    if (w.cap_chrom < nc || w.cap_win < nwin || !w.d_tabs) {
        // (growing: twice the old capacity at least, as wt_grow does -- a pipeline slot's batches creep up)
        const int64_t cc = w.cap_chrom < nc ? std::max<int64_t>(nc, 2 * w.cap_chrom) : w.cap_chrom;
        const int64_t cw = w.cap_win < nwin ? std::max<int64_t>(nwin, 2 * w.cap_win) : w.cap_win;
        const int64_t o_cnwin = up8(4 * cc), o_chi = o_cnwin + up8(4 * cc), o_cfirst = o_chi + up8(4 * cc), o_win = o_cfirst + 8 * (cc + 1);
        const int64_t total = o_win + up8(4 * cw);
        if (w.d_tabs || w.d_status) { WT_HIP(wt_pool_quiesce()); quiet = true; }
        (void) wt_dev_free(w.d_tabs);
        w.d_tabs = nullptr; w.cap_tabs = 0;
        w.d_cbase = w.d_cnwin = w.d_chi = w.d_win_chrom = nullptr; w.d_cfirst = nullptr;
        if (w.cap_win < cw) { (void) wt_dev_free(w.d_status); w.d_status = nullptr; }      // (cleared before every launch: its own allocation)
        w.cap_chrom = 0; w.cap_win = 0;
        WT_HIP(wt_dev_alloc(&w.d_tabs, (size_t) total));
        if (!w.d_status) WT_HIP(wt_dev_alloc(&w.d_status, sizeof(unsigned long long) * (size_t) cw));
        w.cap_tabs = total;
        w.d_cbase = (int32_t *) w.d_tabs; w.d_cnwin = (int32_t *) (w.d_tabs + o_cnwin); w.d_chi = (int32_t *) (w.d_tabs + o_chi);
        w.d_cfirst = (int64_t *) (w.d_tabs + o_cfirst); w.d_win_chrom = (int32_t *) (w.d_tabs + o_win);
        w.cap_chrom = cc; w.cap_win = cw;
    }
    WT_HIP(wt_grow(&w.d_widx, &w.cap_widx, nwidx, &quiet));
    WT_HIP(wt_grow(&w.d_cidx, &w.cap_cidx, ((w.tab.n_rows > 0 ? w.tab.n_rows : 1) + WT_ISEARCH_ROWS - 1) / WT_ISEARCH_ROWS * (int64_t) ts->n_tracks, &quiet));
    if (ts->n_chrom > 0) {
        if (ts->pipe_mode && ts->n_chrom != 1) return wt_fail(WTAMD_ERR_INTERNAL, "pipeline slots hold one chromosome");
        // the staging is rewritten only after the event behind its previous upload has completed
        if (!w.ev_tab) WT_HIP(hipEventCreateWithFlags(&w.ev_tab, hipEventDisableTiming));
        if (w.tab_in_flight) { WT_HIP(hipEventSynchronize(w.ev_tab)); w.tab_in_flight = false; }
        const int64_t head = (char *) w.d_win_chrom - w.d_tabs;         // the per-chromosome tables at this capacity
        if (w.h_tab_bytes < head) {
            if (w.h_tab) wt_host_free(w.h_tab);
            w.h_tab = nullptr; w.h_tab_bytes = 0;
            WT_HIP(wt_host_alloc((void **) &w.h_tab, (size_t) head));
            w.h_tab_bytes = head;
        }
        const int64_t o_cfirst = (char *) w.d_cfirst - w.d_tabs;
        const int64_t used = o_cfirst + (int64_t) sizeof(int64_t) * (ts->n_chrom + 1);
        memset(w.h_tab, 0, (size_t) used);
        memcpy(w.h_tab + ((char *) w.d_cbase - w.d_tabs), w.tab.cbase.data(), sizeof(int32_t) * ts->n_chrom);
        memcpy(w.h_tab + ((char *) w.d_cnwin - w.d_tabs), w.tab.c_nwin.data(), sizeof(int32_t) * ts->n_chrom);
        memcpy(w.h_tab + ((char *) w.d_chi - w.d_tabs), w.tab.c_hi.data(), sizeof(int32_t) * ts->n_chrom);
        memcpy(w.h_tab + o_cfirst, w.tab.c_first_win.data(), sizeof(int64_t) * (ts->n_chrom + 1));
        WT_HIP(hipMemcpyAsync(w.d_tabs, w.h_tab, (size_t) used, hipMemcpyHostToDevice, s));
        WT_HIP(hipEventRecord(w.ev_tab, s));
        w.tab_in_flight = true;
        if (w.tab.n_windows > 0) {
            if (ts->n_chrom == 1) {
                WT_HIP(hipMemsetAsync(w.d_win_chrom, 0, sizeof(int32_t) * (size_t) w.tab.n_windows, s));
            } else {
                hipLaunchKernelGGL(wt_win_chrom_kernel, dim3((unsigned) ((w.tab.n_windows + 255) / 256)), dim3(256), 0, s,
                                   (const int64_t *) w.d_cfirst, ts->n_chrom, (long long) w.tab.n_windows, w.d_win_chrom);
                WT_HIP(hipGetLastError());
            }
        }
    }
    w.tab_valid = true;
    return WTAMD_OK;
}

static void wt_fill_params(const wtamd_trackset *ts, const WtWindows *w, const WtPlan &plan, WtParams &P) {
    memset(&P, 0, sizeof(P));
    P.start = ts->d_start; P.finish = ts->d_finish; P.value = ts->d_value;
    P.seg_off = ts->d_seg_off; P.defaults = ts->d_defaults;
    P.n_chrom = ts->n_chrom; P.n_tracks = ts->n_tracks; P.n_total = ts->n_intervals;
    P.cbase = w->d_cbase; P.c_nwin = w->d_cnwin; P.c_hi = w->d_chi; P.c_first_win = w->d_cfirst;
    P.n_windows = w->tab.n_windows; P.win_chrom = w->d_win_chrom; P.widx = w->d_widx;
    P.status = w->d_status; P.counters = ts->d_counters; P.debug = ts->h_debug;
    wt_plan_to_params(plan, P);
}

static int wt_build_index(wtamd_trackset *ts, WtWindows *w, const WtPlan &plan, hipStream_t s) {
    WtParams P;
    wt_fill_params(ts, w, plan, P);
    WT_HIP(hipEventRecord(ts->ev_i0, s));
    static const int mode = [] {            // 0: search (default), 1: scan, 2: both + compare
        const char *e = getenv("WTAMD_INDEX"), *c = getenv("WTAMD_INDEX_CHECK");
        if (c && atoi(c) > 0) return 2;
        return (e && !strcmp(e, "scan")) ? 1 : 0;
    }();
    const size_t n_widx = (size_t) w->tab.n_rows * ts->n_tracks;
    auto scan = [&](uint32_t *dst) -> int {
        WtParams Q = P;
        Q.widx = dst;
        WT_HIP(hipMemsetAsync(dst, 0, sizeof(uint32_t) * n_widx, s));
        if (ts->n_intervals > 0) {
            const long long total = ts->n_intervals;
            long long blocks = (total + WT_INDEX_CHUNK - 1) / WT_INDEX_CHUNK;
            const long long cap = (long long) ts->num_cu * 8;      // 8 x 256 lanes = a full CU
            if (blocks > cap) blocks = cap;
            // contiguous span per block, a whole number of sub-chunks
            long long span = (total + blocks - 1) / blocks;
            span = (span + WT_INDEX_CHUNK - 1) / WT_INDEX_CHUNK * WT_INDEX_CHUNK;
            blocks = (total + span - 1) / span;
            hipLaunchKernelGGL(wt_index_kernel, dim3((unsigned) blocks), dim3(256), 0, s, Q, total, span);
            WT_HIP(hipGetLastError());
        }
        return WTAMD_OK;
    };
    auto search = [&](uint32_t *dst) -> int {
        WtParams Q = P;
        Q.widx = dst;
        const long long n_rows = w->tab.n_rows;
        if (n_rows > 0 && ts->n_tracks > 0) {
            const long long n_strips = (n_rows + WT_ISEARCH_ROWS - 1) / WT_ISEARCH_ROWS;
            if (w->cap_cidx < n_strips * ts->n_tracks) return wt_fail(WTAMD_ERR_INTERNAL, "coarse window index not allocated");
            hipLaunchKernelGGL(wt_index_coarse_kernel, dim3((unsigned) ((n_strips * ts->n_tracks + 255) / 256)), dim3(256), 0, s, Q, n_strips, w->d_cidx);
            WT_HIP(hipGetLastError());
            const dim3 grid((unsigned) n_strips, (unsigned) ((ts->n_tracks + WT_ISEARCH_TRACKS - 1) / WT_ISEARCH_TRACKS));
            hipLaunchKernelGGL(wt_index_search_kernel, grid, dim3(WT_ISEARCH_ROWS * WT_ISEARCH_TRACKS), 0, s, Q, n_rows, n_strips, (const uint32_t *) w->d_cidx);
            WT_HIP(hipGetLastError());
        }
        return WTAMD_OK;
    };
    if (mode == 1) {
        if (int rc = scan(w->d_widx)) return rc;
    } else {
        if (int rc = search(w->d_widx)) return rc;
    }
    if (mode == 2 && n_widx > 0) {
        uint32_t *other = nullptr;
        unsigned long long *d_diff = nullptr, h_diff = 0;
        WT_HIP(hipMalloc(&other, sizeof(uint32_t) * n_widx));
        WT_HIP(hipMalloc(&d_diff, sizeof(unsigned long long)));
        WT_HIP(hipMemsetAsync(d_diff, 0, sizeof(unsigned long long), s));
        if (int rc = scan(other)) return rc;
        hipLaunchKernelGGL(wt_index_compare_kernel, dim3((unsigned) ((n_widx + 255) / 256)), dim3(256), 0, s, w->d_widx, other, (long long) n_widx, d_diff);
        WT_HIP(hipMemcpyAsync(&h_diff, d_diff, sizeof(h_diff), hipMemcpyDeviceToHost, s));
        WT_HIP(hipStreamSynchronize(s));
        (void) hipFree(other); (void) hipFree(d_diff);
        if (h_diff) {
            fprintf(stderr, "wiggletools_amd: WTAMD_INDEX_CHECK: the searched window index differs from the scanned one in %llu of %zu entries\n", h_diff, n_widx);
            return wt_fail(WTAMD_ERR_INTERNAL, "window index check failed");
        }
    }
    WT_HIP(hipEventRecord(ts->ev_i1, s));
    ts->have_index_time = true;
    w->indexed = true;
    return WTAMD_OK;
}

// The plan a reduction of `op` will run with first: the exact difference-array plan for Sum /
// Mean over float tracks with zero defaults (until a window of this data proved inexact), else the
// general bitmap plan.
static inline int wt_delta_class(int op) { return op == WT_OP_TTEST ? 1 : ((op == WT_OP_MAX || op == WT_OP_MIN) ? 2 : 0); }
static bool wt_wants_delta(const wtamd_trackset *ts, int op) {
    return !ts->delta_failed_[wt_delta_class(op)] && wt_delta_eligible(op, ts->value_f64, ts->n_tracks, ts->defaults.data());
}

// Events (run starts, plus a finish wherever a gap follows) per base pair the track set is expected to hold: the walking
// kernel sizes its per-position slots from it.  Contiguous runs assumed for a quarter of them to be followed by a gap.
static double wt_events_per_bp(const wtamd_trackset *ts) {
    const int64_t span = wt_span(ts);
    return span > 0 ? 1.25 * (double) ts->n_intervals / (double) span : 0.0;
}

// MWUReduction has two kernels, and which one is faster is a matter of the VALUES (round 6; chromosome 21, 50 v 50): the register
// columns of the bitmap kernel sort every position from scratch, 35.8 ms whatever the values are; the walking kernel (wt_mwalk.h)
// keeps its state from position to position and pays for every group of equal values across the two sets -- 28.5 ms on
// full-mantissa values (no position has one), 43.8 ms on the generator's 800 levels (nearly every position has one).  So the
// track set's values are SAMPLED once (4096 of them, evenly strided over the value column; one strided copy and a stream
// synchronisation per track set and index epoch): when nearly all of the sample's values are distinct, equal values at one position are
// rare and the walk is taken.  Real coverage signal with its many exact zeros and small integers stays on the register columns.
// WTAMD_MWALK=1 / 0: always / never.  Both kernels are bit-identical on every input (tests/test_gpu_parity.py::test_gpu_mwu_walk_paths).
static bool wt_mwu_few_ties(wtamd_trackset *ts, hipStream_t stream) {
    if (ts->mwu_few_ties >= 0) return ts->mwu_few_ties != 0;
    ts->mwu_few_ties = 0;
    if (hipStreamSynchronize(stream) != hipSuccess) { (void) hipGetLastError(); return false; }      // (the values may still be on their way on this stream)
    const int64_t n = ts->n_intervals;
    if (n < 1024 || ts->value_f64 || !ts->d_value) return false;      // (a small sample says little: the register columns)
    const int64_t S = std::min<int64_t>(4096, n), stride = n / S;
    std::vector<uint32_t> v((size_t) S);
    if (hipMemcpy2D(v.data(), 4, ts->d_value, (size_t) stride * 4, 4, (size_t) S, hipMemcpyDeviceToHost) != hipSuccess) { (void) hipGetLastError(); return false; }
    std::sort(v.begin(), v.end());
    const int64_t distinct = (int64_t) (std::unique(v.begin(), v.end()) - v.begin());
    ts->mwu_few_ties = distinct * 100 >= S * 97 ? 1 : 0;
    return ts->mwu_few_ties != 0;
}

// The general (non difference-array) plan (wt_plan.h wt_pick_general_plan), with what the engine knows: the switches and the data.
// MWUReduction by walking (wt_mwalk.h): when the values say so (wt_mwu_few_ties) -- on the generator's 800 levels it needs
// 284 wave-wide VALU instructions per output run where the bitmap kernel's register columns need 253 (chromosome 21:
// 43.9 against 35.6 ms; profiles/r05_mwu_walk_vs_bitmap.json).  WTAMD_NO_WALK=1: the bitmap kernel for both.
static bool wt_pick_plan(wtamd_trackset *ts, int op, int n_set0, WtPlan &plan, std::string &err, hipStream_t stream = nullptr) {
    static const int mwalk = getenv("WTAMD_MWALK") ? (atoi(getenv("WTAMD_MWALK")) != 0 ? 1 : 0) : -1;      // (-1: by the data)
    const bool walk = !getenv("WTAMD_NO_WALK");
    const bool mwu_walk = op == WT_OP_MWU && mwalk != 0 && !ts->value_f64 && walk && (mwalk == 1 || wt_mwu_few_ties(ts, stream));
    const double events_per_bp = (op == WT_OP_MEDIAN || op == WT_OP_MWU) ? wt_events_per_bp(ts) : 0.0;
    return wt_pick_general_plan(ts->n_tracks, op, ts->value_f64, ts->scratch_f32, n_set0, walk, mwu_walk, events_per_bp, plan, err);
}

// What was learnt about the track set's data is void: the difference-array launches verify again (delta_failed: they are
// not to be tried at all) and every width's window index describes the old run lists.
static void wt_trackset_forget(wtamd_trackset *ts, bool delta_failed) {
    for (int q = 0; q < 3; q++) { ts->delta_verified_[q] = false; ts->delta_failed_[q] = delta_failed; ts->delta_n_bad_[q] = 0; }
    for (auto &kv : ts->windows) kv.second.indexed = false;
}

extern "C++" int wt_trackset_rebind(wtamd_trackset *ts, int64_t n, const int64_t *seg_off, int32_t range_lo, int32_t range_hi, bool value_f64,
                                    int32_t *d_start, int32_t *d_finish, void *d_value, bool delta_failed) {
    ts->n_intervals = n;
    ts->seg_off.assign(seg_off, seg_off + (int64_t) ts->n_chrom * ts->n_tracks + 1);
    ts->range_lo[0] = range_lo;
    ts->range_hi[0] = range_hi;
    ts->value_f64 = value_f64;
    ts->scratch_f32 = !ts->value_f64 && wt_defaults_fit_f32(ts->defaults.data(), ts->n_tracks);
    ts->d_start = d_start; ts->d_finish = d_finish; ts->d_value = d_value;
    // mwu_few_ties is KEPT: the sample of the pipe's first MWU batch decides for all its batches (ADVICE.md lists this as an
    // open item; sampling per batch would put a stream synchronisation and a copy into every one).  wtamd_trackset_index clears it.
    wt_trackset_forget(ts, delta_failed);
    for (auto &kv : ts->windows) kv.second.tab_valid = false;       // other extents: every width's window tables are rebuilt
    return wt_check_extents(ts);
}

int wtamd_trackset_index(wtamd_trackset *ts, int op, void *stream) {
    if (!ts) return wt_fail(WTAMD_ERR_ARG, "ts == NULL");
    // an explicit re-index means the run lists may have been rewritten in place (zero-copy track
    // sets): what was learnt about their values is void, the next Sum / Mean verifies again
    wt_trackset_forget(ts, false);
    ts->mwu_few_ties = -1;
    if (!ts->owns && !ts->pipe_mode) {
        // zero-copy track set rewritten in place: its runs may start earlier / end later than
        // before, so the extents, their check and every width's window tables are rebuilt too
        int rce = wt_refresh_extents_device(ts, (hipStream_t) stream);
        if (rce != WTAMD_OK) return rce;
        rce = wt_check_extents(ts);
        if (rce != WTAMD_OK) return rce;
        for (auto &kv : ts->windows) kv.second.tab_valid = false;
    }
    WtPlan plan;
    std::string err;
    if (wt_wants_delta(ts, op)) wt_make_delta_plan_for(plan, ts->n_tracks, op);
    // (two-sample ops: the index only depends on the window width; the usual even split is assumed)
    else if (!wt_pick_plan(ts, op, ts->n_tracks / 2, plan, err, (hipStream_t) stream)) return wt_fail(WTAMD_ERR_ARG, err);
    WtWindows *w = nullptr;
    int rc = wt_get_windows(ts, plan.W, &w, (hipStream_t) stream);
    if (rc != WTAMD_OK) return rc;
    return wt_build_index(ts, w, plan, (hipStream_t) stream);
}

extern "C++" int wt_check_desc(const wtamd_trackset *ts, const wtamd_reduce_desc *d) {
    if (!ts || !d) return wt_fail(WTAMD_ERR_ARG, "NULL argument");
    if (d->op < 0 || d->op >= WTAMD_OP_COUNT_) return wt_fail(WTAMD_ERR_ARG, "unknown op");
    if (d->op == WTAMD_OP_TTEST) {
        // message + precondition of reference setComparisons.c:123-128
        if (d->n_set0 < 3 || ts->n_tracks - d->n_set0 < 3)
            return wt_fail(WTAMD_ERR_ARG, "The t-test function only works for two sets with enough elements to compute variance");
    } else if (d->op == WTAMD_OP_MWU) {
        // reference setComparisons.c:374-377
        if (d->n_set0 < 1 || ts->n_tracks - d->n_set0 < 1)
            return wt_fail(WTAMD_ERR_ARG, "The Mann-Whitney U function only works for two non-empty sets");
    }
    return WTAMD_OK;
}

static int wt_reduce_plan(wtamd_trackset *ts, const WtPlan &plan, int op, uint32_t flags, int n_set0, wtamd_runs *runs,
                          double *d_tile, uint8_t *d_inplay, int64_t *n_runs, hipStream_t s);

// The general kernel over the `n_bad` windows the difference-array launch (window width delta_W,
// just finished or still running on `s`) recorded as not provably exact.
extern "C++" int wt_launch_patch(wtamd_trackset *ts, int delta_W, int op, uint32_t flags, int n_set0, wtamd_runs *runs, long long n_bad,
                                 hipStream_t s) {
    WtPlan plan;
    std::string err;
    if (!wt_make_plan(ts->n_tracks, op, ts->scratch_f32, plan, err)) return wt_fail(WTAMD_ERR_INTERNAL, err);
    if (!wt_patch_compatible(plan, delta_W, ts->scratch_f32, ts->value_f64))
        return wt_fail(WTAMD_ERR_INTERNAL, "no general plan compatible with the difference-array windows (general W " + std::to_string(plan.W) + ", difference-array W " +
                       std::to_string(delta_W) + ", slab " + std::to_string((long long) plan.scratch_slab) + ", float staging " + std::to_string((int) ts->scratch_f32) + ", f64 values " +
                       std::to_string((int) ts->value_f64) + ")");
    WtWindows *dw = nullptr, *w = nullptr;
    int rc = wt_get_windows(ts, delta_W, &dw, s);
    if (rc != WTAMD_OK) return rc;
    rc = wt_get_windows(ts, plan.W, &w, s);
    if (rc != WTAMD_OK) return rc;
    WtLaunch L;
    WtParams &P = L.P;
    wt_fill_params(ts, w, plan, P);
    P.op = op; P.flags = flags; P.n_set0 = op == WT_OP_TTEST ? n_set0 : 0;
    P.capacity = runs->capacity;
    P.o_start = runs->start; P.o_finish = runs->finish; P.o_value = runs->value;
    P.chrom_run_off = runs->chrom_run_off ? runs->chrom_run_off : ts->d_chrom_run_off;
    L.T = plan.T; L.lds = plan.lds_bytes; L.stream = s; L.num_cu = ts->num_cu;
    WtPatchArgs Q;
    Q.bad_list = dw->d_bad_list; Q.bad_goff = dw->d_bad_goff;
    Q.n_bad = ts->d_counters + WT_CTR_DELTA_BAD;
    Q.d_win_chrom = dw->d_win_chrom; Q.d_c_first_win = dw->d_cfirst;
    Q.ratio = delta_W / plan.W;
    // (no index at this window width yet: only the rows of the recorded windows are filled in, w->indexed stays false)
    if (!wt_patch_launch(L, Q, op, plan.ppt, plan.n_chunks > 1, n_bad, !w->indexed))
        return wt_fail(WTAMD_ERR_INTERNAL, "no general plan compatible with the difference-array windows");
    if (L.err != hipSuccess) return wt_fail(WTAMD_ERR_HIP, std::string("patch kernel launch: ") + hipGetErrorString(L.err));
    WT_HIP(hipEventRecord(ts->ev_r1, s));       // the reduction's time includes its patches
    ts->stats.patched_windows = (int32_t) n_bad;
    return WTAMD_OK;
}

static int wt_reduce_impl(wtamd_trackset *ts, int op, uint32_t flags, int n_set0, wtamd_runs *runs,
                          double *d_tile, uint8_t *d_inplay, int64_t *n_runs, hipStream_t s) {
    if (!runs || !runs->start || !runs->finish || !runs->value)
        return wt_fail(WTAMD_ERR_ARG, "wtamd_reduce: output arrays missing");
    WtPlan plan;
    std::string err;
    // Sum / Mean: exact difference-array kernel first.  It verifies every window.  A few windows
    // it cannot prove exact (NaN, Inf, too wide a dynamic range) keep their coordinates and get
    // their values from the general kernel restricted to them (the patch kernel); if they are many
    // the whole launch is redone by the general kernel and this data stays on it.  The verdict
    // depends on the data and the windows only (not on the op or its flags), so it is established
    // once per track set -- that first launch is waited for even when the caller asked for an
    // asynchronous one -- and later launches (patch included) need no host round trip.
    if (!d_tile && wt_wants_delta(ts, op)) {
        wt_make_delta_plan_for(plan, ts->n_tracks, op);
        const int dc = wt_delta_class(op);
        int64_t n_probe = 0;
        const bool probe = !ts->delta_verified_[dc];
        const int rc = wt_reduce_plan(ts, plan, op, flags, n_set0, runs, d_tile, d_inplay,
                                      (probe && !n_runs) ? &n_probe : n_runs, s);
        if (!probe) {
            if (ts->delta_n_bad_[dc] > 0 && (rc == WTAMD_OK || rc == WTAMD_ERR_CAPACITY)) {
                const int rp = wt_launch_patch(ts, plan.W, op, flags, n_set0, runs, ts->delta_n_bad_[dc], s);
                if (rp != WTAMD_OK) return rp;
                if (n_runs) WT_HIP(hipStreamSynchronize(s));
            }
            return rc;
        }
        if (rc != WTAMD_OK && rc != WTAMD_ERR_CAPACITY) return rc;
        const long long n_bad = (long long) ts->h_counters[WT_CTR_DELTA_BAD];
        if (n_bad == 0) { ts->delta_verified_[dc] = true; ts->delta_n_bad_[dc] = 0; return rc; }
        if (wt_few_enough_to_patch(n_bad, ts->stats.n_windows) && !getenv("WTAMD_NO_PATCH")) {
            const int rp = wt_launch_patch(ts, plan.W, op, flags, n_set0, runs, n_bad, s);
            if (rp == WTAMD_OK) {
                WT_HIP(hipStreamSynchronize(s));
                ts->delta_verified_[dc] = true;
                ts->delta_n_bad_[dc] = n_bad;
                return rc;
            }
            if (rp != WTAMD_ERR_INTERNAL) return rp;        // INTERNAL: no compatible general plan -> full redo
        }
        ts->delta_failed_[dc] = true;
    }
    if (!wt_pick_plan(ts, op, n_set0, plan, err, s)) return wt_fail(WTAMD_ERR_ARG, err);
    return wt_reduce_plan(ts, plan, op, flags, n_set0, runs, d_tile, d_inplay, n_runs, s);
}

extern "C++" int wt_reduce_enqueue(wtamd_trackset *ts, const wtamd_reduce_desc &desc, wtamd_runs *runs, double *d_tile, uint8_t *d_inplay,
                                   hipStream_t s, bool *used_delta, int *delta_W) {
    WtPlan plan;
    std::string err;
    *used_delta = !d_tile && wt_wants_delta(ts, desc.op);
    if (*used_delta) {
        wt_make_delta_plan_for(plan, ts->n_tracks, desc.op);
        *delta_W = plan.W;
    } else if (!wt_pick_plan(ts, desc.op, desc.n_set0, plan, err, s)) {
        return wt_fail(WTAMD_ERR_ARG, err);
    }
    return wt_reduce_plan(ts, plan, desc.op, desc.flags, desc.n_set0, runs, d_tile, d_inplay, nullptr, s);
}

static int wt_reduce_plan(wtamd_trackset *ts, const WtPlan &plan, int op, uint32_t flags, int n_set0, wtamd_runs *runs,
                          double *d_tile, uint8_t *d_inplay, int64_t *n_runs, hipStream_t s) {
    if (plan.T > (plan.delta ? ((wt_op_is_var_family(op) || op == WT_OP_TTEST) ? wt_delta_sq_block : wt_delta_block) : wt_reduce_max_block)) return wt_fail(WTAMD_ERR_ARG, "workgroup size above the kernel's launch bound");
    WtWindows *w = nullptr;
    int rc = wt_get_windows(ts, plan.W, &w, s);
    if (rc != WTAMD_OK) return rc;
    if (!w->indexed) {
        rc = wt_build_index(ts, w, plan, s);
        if (rc != WTAMD_OK) return rc;
    }
    WtLaunch L;
    wt_fill_params(ts, w, plan, L.P);
    L.P.op = op; L.P.flags = flags; L.P.n_set0 = n_set0;
    L.P.capacity = runs->capacity;
    L.P.o_start = runs->start; L.P.o_finish = runs->finish; L.P.o_value = runs->value;
    L.P.chrom_run_off = runs->chrom_run_off ? runs->chrom_run_off : ts->d_chrom_run_off;
    L.P.o_tile = d_tile; L.P.o_inplay = d_inplay;
    L.T = plan.T; L.lds = plan.lds_bytes; L.stream = s; L.num_cu = ts->num_cu;
    L.gscratch = &ts->d_gscratch; L.gscratch_bytes = &ts->gscratch_bytes;
    if (op == WT_OP_MWU && !getenv("WTAMD_MWU_DEVICE_ERF")) {
        const int n1 = n_set0, n2 = ts->n_tracks - n_set0;
        if (ts->mwu_n1 != n1 || ts->mwu_n2 != n2) {
            // (a table per pair of set sizes; the previous pair's table may still be read by a launch in flight on ANY stream of
            //  this track set: it is retired, not freed -- wtamd_trackset_destroy frees them all)
            std::vector<double> t;
            const bool have = wt_mwu_make_table(n1, n2, t);
            if (ts->d_mwu_table) { ts->mwu_retired.push_back(ts->d_mwu_table); ts->d_mwu_table = nullptr; }
            if (have) {
                WT_HIP(hipMalloc((void **) &ts->d_mwu_table, sizeof(double) * t.size()));
                WT_HIP(hipMemcpyAsync(ts->d_mwu_table, t.data(), sizeof(double) * t.size(), hipMemcpyHostToDevice, s));
                WT_HIP(hipStreamSynchronize(s));                // (t is a local)
            }
            ts->mwu_n1 = n1; ts->mwu_n2 = n2; ts->mwu_kmax = have ? (int) t.size() - 1 : 0;
        }
        L.P.mwu_table = ts->d_mwu_table;
        L.P.mwu_kmax = ts->mwu_kmax;
    }
    if (plan.delta) {
        const int64_t nwin = w->tab.n_windows > 0 ? w->tab.n_windows : 1;
        if (w->cap_bad < nwin) {
            int64_t c1 = w->cap_bad, c2 = w->cap_bad;
            bool quiet = false;
            WT_HIP(wt_grow(&w->d_bad_list, &c1, nwin, &quiet));
            WT_HIP(wt_grow(&w->d_bad_goff, &c2, nwin * WT_BAD_SUB, &quiet));
            w->cap_bad = c1 < c2 / WT_BAD_SUB ? c1 : c2 / WT_BAD_SUB;
        }
        L.P.bad_list = w->d_bad_list;
        L.P.bad_goff = w->d_bad_goff;
        wt_delta_defaults_params(ts->defaults.data(), ts->n_tracks, L.P);
    }

    // the counters, the run offsets and (where a kernel follows) the look-back words, cleared by one kernel
    const bool launches = w->tab.n_windows > 0 && ts->n_intervals > 0;
    {
        const long long n_status = launches ? (long long) w->tab.n_windows : 0;
        const long long most = std::max<long long>(std::max<long long>(n_status, WT_CTR_N), ts->n_chrom + 1);
        const unsigned blocks = (unsigned) std::min<long long>((most + 255) / 256, 1024);
        hipLaunchKernelGGL(wt_clear_kernel, dim3(blocks), dim3(256), 0, s, ts->d_counters, (int) WT_CTR_N, L.P.chrom_run_off, ts->n_chrom + 1,
                           w->d_status, n_status);
        WT_HIP(hipGetLastError());
    }
    if (launches) {
        if (plan.delta) {
            // (tiles of 256 runs per wavefront and window, on average)
            static const int force_u = getenv("WTAMD_DELTA_U") ? atoi(getenv("WTAMD_DELTA_U")) : 0;
            const double tiles_per_wave = (double) ts->n_intervals / (double) w->tab.n_windows / 256.0 / (double) std::max(1, L.T / 64);
            L.small_tiles = force_u == 2 || (force_u != 4 && tiles_per_wave < 8.0);
        }
        WT_HIP(hipEventRecord(ts->ev_r0, s));
        if (plan.delta) {
            wt_delta_launch(L, op);
        } else if (plan.walk_S) {
            L.err = wt_walk_launch(L.P, plan.regcol, L.T, L.lds, L.num_cu, L.gscratch, L.gscratch_bytes, L.stream, &L.grid);
        } else if (!wt_reduce_launch(L, op, ts->value_f64, ts->scratch_f32, plan.ppt, plan.n_chunks > 1 || plan.scratch_slab > 0, plan.regcol)) {
            return wt_fail(WTAMD_ERR_ARG, "op not dispatchable");
        }
        if (L.err != hipSuccess) return wt_fail(WTAMD_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(L.err));
        WT_HIP(hipEventRecord(ts->ev_r1, s));
        ts->have_reduce_time = true;
    }
    ts->stats.n_windows = w->tab.n_windows;
    ts->stats.window_bp = plan.W;
    ts->stats.lds_bytes = plan.lds_bytes;
    ts->stats.kernel = plan.delta ? 1 : (plan.walk_S ? (plan.walk_mwu ? 3 : 2) : 0);     // (2: median by walking, csrc/wt_walk.h; 3: MWU by walking, csrc/wt_mwalk.h)
    ts->stats.patched_windows = 0;
    if (n_runs) {
        WT_HIP(hipMemcpyAsync(ts->h_counters, ts->d_counters, sizeof(unsigned long long) * WT_CTR_N, hipMemcpyDeviceToHost, s));
        const int rcw = wt_bounded_wait([s] { return hipStreamQuery(s); }, "hipStreamQuery", nullptr, 0.002, 200, [ts](double limit_s) {
            char buf[320];
            snprintf(buf, sizeof buf, "kernel did not finish within %.0f s (debug marker %llu, window %lld; per wave %llu %llu %llu %llu %llu %llu %llu %llu)",
                     limit_s, ts->h_debug[0], (long long) ts->h_debug[1], ts->h_debug[2], ts->h_debug[3], ts->h_debug[4],
                     ts->h_debug[5], ts->h_debug[6], ts->h_debug[7], ts->h_debug[8], ts->h_debug[9]);
            return std::string(buf);
        });
        if (rcw != WTAMD_OK) return rcw;
        ts->stats.n_runs = (int64_t) ts->h_counters[WT_CTR_RUNS];
        ts->stats.covered_bp = (int64_t) ts->h_counters[WT_CTR_BP];
        ts->stats.n_intervals = (int64_t) ts->h_counters[WT_CTR_INTERVALS];
        *n_runs = ts->stats.n_runs;
        if (plan.walk_S) {      // (-DWT_PROFILE builds of wt_walk.hip: cycles of wave 0 per phase, summed over the workgroups)
            static const bool show = getenv("WTAMD_WALK_PROF") != nullptr;
            if (show) {
                static const char *names_w[8] = {"zero+ranges", "count", "offsets", "scatter", "events", "first-median", "moves", "rest"};
                unsigned long long tot = 0;
                for (int q = 0; q < 8; q++) tot += ts->h_counters[WT_CTR_PROF + q];
                fprintf(stderr, "[wt_walk_profile]");
                for (int q = 0; q < 8; q++) fprintf(stderr, " %s %.1f%%", names_w[q], tot ? 100.0 * ts->h_counters[WT_CTR_PROF + q] / tot : 0.0);
                fprintf(stderr, " (total %.3g cycles)\n", (double) tot);
            }
        }
#ifdef WT_PROFILE
        {
            static const char *names_g[8] = {"zero", "load", "count", "emask+escan", "eval", "lookback", "write", "-"};
            static const char *names_d[8] = {"zero", "ranges", "pass1", "pass2", "scan", "escan", "lookback", "write"};
            const char **names = plan.delta ? names_d : names_g;
            unsigned long long tot = 0;
            for (int q = 0; q < 8; q++) tot += ts->h_counters[WT_CTR_PROF + q];
            fprintf(stderr, "[wt_profile] op %d:", op);
            for (int q = 0; q < 8; q++)
                fprintf(stderr, " %s %.1f%%", names[q], tot ? 100.0 * ts->h_counters[WT_CTR_PROF + q] / tot : 0.0);
            fprintf(stderr, " (total %.3g cycles over all workgroups)\n", (double) tot);
            unsigned long long p2[8] = {0};
            if (wt_prof2_take(p2))
                fprintf(stderr, "[wt_profile] register column, cycles summed over waves: gather %.3g  sort/park %.3g  count loop %.3g  erf %.3g  median sort+select %.3g\n",
                        (double) p2[0], (double) p2[1], (double) p2[2], (double) p2[3], (double) p2[4]);
        }
#endif
        if (ts->h_counters[WT_CTR_ERROR] & WT_ERR_LOOKBACK) return wt_fail(WTAMD_ERR_INTERNAL, "look-back timed out");
        if (ts->h_counters[WT_CTR_ERROR] & WT_ERR_CAPACITY) return wt_fail(WTAMD_ERR_CAPACITY, "output capacity too small");
    }
    return WTAMD_OK;
}

int wtamd_reduce(wtamd_trackset *ts, const wtamd_reduce_desc *desc, wtamd_runs *runs, int64_t *n_runs, void *stream) {
    int rc = wt_check_desc(ts, desc);
    if (rc != WTAMD_OK) return rc;
    return wt_reduce_impl(ts, desc->op, desc->flags, desc->n_set0, runs, nullptr, nullptr, n_runs, (hipStream_t) stream);
}

static int wt_reduce_host_impl(wtamd_trackset *ts, int op, uint32_t flags, int n_set0, wtamd_runs *runs,
                               double *h_tile, uint8_t *h_inplay, int64_t *n_runs) {
    if (!runs) return wt_fail(WTAMD_ERR_ARG, "runs == NULL");
    int64_t cap = wtamd_trackset_max_runs(ts);
    if (cap > runs->capacity) cap = runs->capacity;     // never write past the caller's arrays
    const int64_t alloc = cap > 0 ? cap : 1;
    const int N = ts->n_tracks;
    WtDevScope scope;
    wtamd_runs d{};
    d.capacity = cap;
    double *d_tile = nullptr;
    uint8_t *d_inplay = nullptr;
    WT_HIP(scope.alloc(&d.start, sizeof(int32_t) * alloc));
    WT_HIP(scope.alloc(&d.finish, sizeof(int32_t) * alloc));
    WT_HIP(scope.alloc(&d.value, sizeof(double) * alloc));
    WT_HIP(scope.alloc(&d.chrom_run_off, sizeof(int64_t) * (ts->n_chrom + 1)));
    if (op == WT_OP_MULTIPLEX) {
        WT_HIP(scope.alloc(&d_tile, sizeof(double) * alloc * N));
        WT_HIP(scope.alloc(&d_inplay, sizeof(uint8_t) * alloc * N));
    }
    int64_t n = 0;
    int rc = wt_reduce_impl(ts, op, flags, n_set0, &d, d_tile, d_inplay, &n, nullptr);
    if (rc == WTAMD_OK) {
        if (n > 0) {
            WT_HIP(hipMemcpy(runs->start, d.start, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
            WT_HIP(hipMemcpy(runs->finish, d.finish, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
            if (runs->value) WT_HIP(hipMemcpy(runs->value, d.value, sizeof(double) * n, hipMemcpyDeviceToHost));
            if (h_tile) WT_HIP(hipMemcpy(h_tile, d_tile, sizeof(double) * n * N, hipMemcpyDeviceToHost));
            if (h_inplay) WT_HIP(hipMemcpy(h_inplay, d_inplay, sizeof(uint8_t) * n * N, hipMemcpyDeviceToHost));
        }
        if (runs->chrom_run_off)
            WT_HIP(hipMemcpy(runs->chrom_run_off, d.chrom_run_off, sizeof(int64_t) * (ts->n_chrom + 1), hipMemcpyDeviceToHost));
        if (n_runs) *n_runs = n;
    }
    return rc;
}

int wtamd_reduce_host(wtamd_trackset *ts, const wtamd_reduce_desc *desc, wtamd_runs *runs, int64_t *n_runs) {
    int rc = wt_check_desc(ts, desc);
    if (rc != WTAMD_OK) return rc;
    return wt_reduce_host_impl(ts, desc->op, desc->flags, desc->n_set0, runs, nullptr, nullptr, n_runs);
}

int wtamd_multiplex_host(wtamd_trackset *ts, uint32_t flags, wtamd_runs *runs, double *values, uint8_t *inplay,
                         int64_t *n_runs) {
    if (!ts || !values || !inplay) return wt_fail(WTAMD_ERR_ARG, "NULL argument");
    return wt_reduce_host_impl(ts, WT_OP_MULTIPLEX, flags, 0, runs, values, inplay, n_runs);
}

// the Multiplexer tile of the track set's current data into device arrays, on `s` (csrc/wt_mtext.hip prints it)
extern "C++" int wt_multiplex_device(wtamd_trackset *ts, uint32_t flags, wtamd_runs *runs, double *d_tile, uint8_t *d_inplay, int64_t *n_runs,
                                     hipStream_t s) {
    return wt_reduce_impl(ts, WT_OP_MULTIPLEX, flags, 0, runs, d_tile, d_inplay, n_runs, s);
}

static int wt_runs_auc_span(const wtamd_runs *runs, int64_t n_runs, double *auc, double *span, void *stream) {
    hipStream_t s = (hipStream_t) stream;
    const int blocks = 512;
    double *d_partial = nullptr, h[2] = {0, 0};
    WtDevScope scope;
    WT_HIP(scope.alloc(&d_partial, wt_auc_partial_bytes(blocks) + sizeof(double) * 2));
    const int rc = wt_auc_async(runs->start, runs->finish, runs->value, (long long) n_runs, nullptr, blocks, d_partial, d_partial + 2 * blocks, span != nullptr, s);
    if (rc != WTAMD_OK) return rc;
    WT_HIP(hipMemcpyAsync(h, d_partial + 2 * blocks, sizeof(double) * (span ? 2 : 1), hipMemcpyDeviceToHost, s));
    WT_HIP(hipStreamSynchronize(s));
    *auc = h[0];
    if (span) *span = h[1];
    return WTAMD_OK;
}

int wtamd_runs_auc(const wtamd_runs *runs, int64_t n_runs, double *auc, void *stream) {
    if (!runs || !auc) return wt_fail(WTAMD_ERR_ARG, "NULL argument");
    return wt_runs_auc_span(runs, n_runs, auc, nullptr, stream);
}

int wtamd_runs_mean(const wtamd_runs *runs, int64_t n_runs, double *mean, void *stream) {
    if (!runs || !mean) return wt_fail(WTAMD_ERR_ARG, "NULL argument");
    double sum = 0, span = 0;
    const int rc = wt_runs_auc_span(runs, n_runs, &sum, &span, stream);
    if (rc != WTAMD_OK) return rc;
    *mean = span > 0 ? sum / span : __builtin_nan("");      // statistics.c:66-68, res initialised to NAN :98
    return WTAMD_OK;
}

// result[0] = correlation, result[1..6] = {n, sum_X, sum_Y, T_XX, T_XY, T_YY}
static int wt_pearson_impl(wtamd_trackset *ts, double *result7) {
    if (ts->n_tracks != 2) return wt_fail(WTAMD_ERR_ARG, "wtamd_pearson: the track set must hold exactly two tracks");
    int64_t cap = wtamd_trackset_max_runs(ts);
    const int64_t alloc = cap > 0 ? cap : 1;
    wtamd_runs d{};
    d.capacity = cap;
    double *d_tile = nullptr;
    uint8_t *d_inplay = nullptr;
    char *d_partial = nullptr;
    double *d_out = nullptr;
    const int blocks = 256;
    WtDevScope scope;
    WT_HIP(scope.alloc(&d.start, sizeof(int32_t) * alloc));
    WT_HIP(scope.alloc(&d.finish, sizeof(int32_t) * alloc));
    WT_HIP(scope.alloc(&d.value, sizeof(double) * alloc));
    WT_HIP(scope.alloc(&d.chrom_run_off, sizeof(int64_t) * (ts->n_chrom + 1)));
    WT_HIP(scope.alloc(&d_tile, sizeof(double) * alloc * 2));
    WT_HIP(scope.alloc(&d_inplay, sizeof(uint8_t) * alloc * 2));
    WT_HIP(scope.alloc(&d_partial, wt_pearson_partial_bytes(blocks)));
    WT_HIP(scope.alloc(&d_out, sizeof(double) * 7));
    int64_t n = 0;
    int rc = wt_reduce_impl(ts, WT_OP_MULTIPLEX, 0, 0, &d, d_tile, d_inplay, &n, nullptr);
    if (rc == WTAMD_OK) {
        rc = wt_pearson_async(d.start, d.finish, d_tile, d_inplay, ts->defaults[0], ts->defaults[1], (long long) n, nullptr, blocks, d_partial, d_out, nullptr);
        if (rc != WTAMD_OK || hipMemcpy(result7, d_out, sizeof(double) * 7, hipMemcpyDeviceToHost) != hipSuccess)
            rc = wt_fail(WTAMD_ERR_HIP, "wtamd_pearson: kernel launch / copy failed");
    }
    return rc;
}

int wtamd_pearson(wtamd_trackset *ts, double *result) {
    if (!ts || !result) return wt_fail(WTAMD_ERR_ARG, "NULL argument");
    double r[7];
    const int rc = wt_pearson_impl(ts, r);
    if (rc == WTAMD_OK) *result = r[0];
    return rc;
}

int wtamd_pearson_moments(wtamd_trackset *ts, double *moments) {
    if (!ts || !moments) return wt_fail(WTAMD_ERR_ARG, "NULL argument");
    double r[7];
    const int rc = wt_pearson_impl(ts, r);
    if (rc == WTAMD_OK) memcpy(moments, r + 1, sizeof(double) * 6);
    return rc;
}

// (wtamd_pearson_merge / wtamd_pearson_finish: host-only, csrc/wt_defaults.cpp)

int wtamd_trackset_validate(wtamd_trackset *ts, int64_t *n_bad, int64_t *first_bad) {
    if (!ts || !n_bad) return wt_fail(WTAMD_ERR_ARG, "NULL argument");
    *n_bad = 0;
    if (first_bad) *first_bad = -1;
    if (ts->n_intervals <= 0) return WTAMD_OK;
    unsigned long long h[2] = {0ull, ~0ull}, *d = nullptr;
    WtDevScope scope;
    WT_HIP(scope.alloc(&d, sizeof h));
    WT_HIP(hipMemcpy(d, h, sizeof h, hipMemcpyHostToDevice));
    const long long total = ts->n_intervals;
    hipLaunchKernelGGL(wt_validate_kernel, dim3((unsigned) ((total + 255) / 256)), dim3(256), 0, nullptr, ts->d_start,
                       ts->d_finish, ts->d_seg_off, (long long) ts->n_chrom * ts->n_tracks, total, d);
    const hipError_t e = hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return wt_fail(WTAMD_ERR_HIP, "wtamd_trackset_validate: kernel / copy failed");
    *n_bad = (int64_t) h[0];
    if (first_bad && h[0]) *first_bad = (int64_t) h[1];
    return WTAMD_OK;
}

int wtamd_get_stats(const wtamd_trackset *ts_c, wtamd_stats *out) {
    if (!ts_c || !out) return wt_fail(WTAMD_ERR_ARG, "NULL argument");
    wtamd_trackset *ts = const_cast<wtamd_trackset *>(ts_c);
    if (ts->have_index_time && hipEventSynchronize(ts->ev_i1) == hipSuccess)
        (void) hipEventElapsedTime(&ts->stats.index_ms, ts->ev_i0, ts->ev_i1);
    if (ts->have_reduce_time && hipEventSynchronize(ts->ev_r1) == hipSuccess)
        (void) hipEventElapsedTime(&ts->stats.reduce_ms, ts->ev_r0, ts->ev_r1);
    *out = ts->stats;
    return WTAMD_OK;
}

}  // extern "C"

