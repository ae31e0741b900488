// wt_host.h -- what the host side of every HIP unit shares: the error record, the return-on-HIP-error macro, the bounded
// wait, and the entries one unit offers to another (the unit that defines them and the unit that calls them both include this).
#ifndef WT_HOST_H_
#define WT_HOST_H_

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <unistd.h>

#include "../../include/wiggletools_amd.h"

// records msg for wtamd_last_error (per thread) and returns code (wt_engine.hip)
int wt_fail(int code, const std::string &msg);

#define WT_HIP(expr)                                                                           \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return wt_fail(WTAMD_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));  \
    } while (0)

// Bounded wait: a kernel that does not finish is reported, never waited for forever.  A kernel that never finishes cannot
// be cancelled and every later HIP call of this process (even hipFree) would block behind it: after WTAMD_TIMEOUT_S
// (default 120) the process reports fatal(limit) and terminates.  query() is hipStreamQuery / hipEventQuery of what is waited
// for (`call`, `what`: its name in the error message); the wait spins for nap_after_s, then sleeps between queries -- for 1/64
// of the time already waited, nap_us at the most: a wait of a few milliseconds ends within 2 % of the kernel's end instead of
// up to a whole nap_us quantum behind it, and a long one still leaves the core alone.
template <class Query, class Fatal>
static inline int wt_bounded_wait(Query query, const char *call, const char *what, double nap_after_s, int nap_us, Fatal fatal) {
    const double limit_s = getenv("WTAMD_TIMEOUT_S") ? atof(getenv("WTAMD_TIMEOUT_S")) : 120.0;
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t q = query();
        if (q == hipSuccess) return WTAMD_OK;
        if (q != hipErrorNotReady) return wt_fail(WTAMD_ERR_HIP, std::string(call) + (what ? std::string(" (") + what + ")" : std::string()) + ": " + hipGetErrorString(q));
        const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (el > limit_s) {
            fprintf(stderr, "wiggletools_amd: FATAL: %s\n", fatal(limit_s).c_str());
            fflush(stderr);
            _exit(70);
        }
        if (el > nap_after_s) {
            const double nap = el * (1e6 / 64.0);
            std::this_thread::sleep_for(std::chrono::nanoseconds((long long) (1e3 * (nap < (double) nap_us ? nap : (double) nap_us))));
        }
    }
}

// wt_map.hip
long long wt_map_scratch_words(long long capacity);
int wt_map_upload_chains(const wtamd_map_chain *chains, int n_tracks, void **d_out, bool *drops, bool *f32_exact);
int wt_map_chain_async(const void *d_chains, int n_tracks, bool drops, const int64_t *d_seg_in, long long n, const int32_t *start,
                       const int32_t *finish, const void *value, bool value_is_f64, unsigned long long *scratch,
                       int32_t *o_start, int32_t *o_finish, double *o_value, int64_t *d_seg_out, hipStream_t stream, bool out_f32);
// wt_bwdev.hip
long long wt_bw_scratch_bytes(long long n_sec, long long plain_stride);
long long wt_bw_fill_sections(int num_cu);
int wt_bw_decode_async(const void *h_bytes, void *d_bytes, long long n_bytes, const void *d_comp, const void *d_secs, const void *d_tracks, int n_tracks,
                       long long n_sec, long long plain_stride, void *scratch, long long capacity, int32_t *o_start, int32_t *o_finish,
                       float *o_value, int64_t *d_seg_off, unsigned long long *h_status, int copy_blocks, hipStream_t s_copy,
                       hipEvent_t e_copied, hipStream_t s_dec);
// wt_compress.hip
long long wt_compress_scratch_words(long long capacity);
int wt_compress_async(const int32_t *start, const int32_t *finish, const double *value, const unsigned long long *d_n,
                      long long capacity, unsigned long long *scratch, int32_t *o_start, int32_t *o_finish, double *o_value,
                      unsigned long long *d_n_out, hipStream_t s);
// wt_moments.hip: integrals of a device run list on `st`.  n_dev (may be NULL): the run count where only the device knows
// it; d_partial: wt_*_partial_bytes(blocks) bytes of device memory; results stay on the device.
size_t wt_moments_partial_bytes(int blocks);
int wt_moments_async(const int32_t *start, const int32_t *finish, const double *value, long long cap, const unsigned long long *n_dev,
                     int blocks, void *d_partial, double *d_out6, hipStream_t st);
size_t wt_auc_partial_bytes(int blocks);
// d_out[0] = sum (finish - start) * value over the non-NaN runs; with_span: d_out[1] = their span
int wt_auc_async(const int32_t *start, const int32_t *finish, const double *value, long long n, const unsigned long long *n_dev,
                 int blocks, void *d_partial, double *d_out, bool with_span, hipStream_t st);
size_t wt_pearson_partial_bytes(int blocks);
// d_out7[0] = correlation of the two tracks of the tile, d_out7[1..6] = {n, sum_X, sum_Y, T_XX, T_XY, T_YY}
int wt_pearson_async(const int32_t *start, const int32_t *finish, const double *tile, const uint8_t *inplay, double dx, double dy, long long n,
                     const unsigned long long *n_dev, int blocks, void *d_partial, double *d_out7, hipStream_t st);

#endif  // WT_HOST_H_
