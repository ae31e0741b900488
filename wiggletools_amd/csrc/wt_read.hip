// wt_read.hip -- wig, bedGraph and BED text into run lists on the device: the reference's WiggleReader (src/wigReader.c) and
// BedReader (src/bedReader.c) over the bytes of a file in HBM.  The passes and the door are written once in csrc/wt_read.h (which
// tests/read_emu.cpp also compiles for the CPU); this unit gives every pass its kernel; the launcher of the door and the report
// of its result are those of csrc/wt_runs_host.h.  Temporary device memory comes from the pool (wt_pool.h).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "wt_runs_host.h"
#include "wt_read.h"

namespace {

template <int K>
__global__ void __launch_bounds__(WTR_BLOCK) wt_read_kernel(WtrArgs a) {
    __shared__ WtrLds lds;
    wtr_run_block(K, a, (long long) blockIdx.x, &lds);
}

struct HipReadLauncher : WtRunsLauncher {
    template <int K> bool launch(long long blocks, const WtrArgs &a) { return WtRunsLauncher::launch(wt_read_kernel<K>, WTR_BLOCK, blocks, a); }
    bool run_read(int kernel, long long blocks, const WtrArgs &a) {
        switch (kernel) {
        case WTR_K_LINES: return launch<WTR_K_LINES>(blocks, a);
        case WTR_K_SCAN: return launch<WTR_K_SCAN>(blocks, a);
        case WTR_K_COUNT: return launch<WTR_K_COUNT>(blocks, a);
        case WTR_K_SCAN2: return launch<WTR_K_SCAN2>(blocks, a);
        case WTR_K_WRITE: return launch<WTR_K_WRITE>(blocks, a);
        case WTR_K_STATE: return launch<WTR_K_STATE>(blocks, a);
        default: return false;
        }
    }
};

static_assert(sizeof(wtamd_read_state) == sizeof(WtrState) && sizeof(WtrState) == 544, "wtamd_read_state is WtrState");
static_assert(sizeof(wtamd_read_counts) == sizeof(WtrCounts) && sizeof(WtrCounts) == 64, "wtamd_read_counts is WtrCounts");
static_assert(sizeof(WtrTile) == 112, "the scratch per tile, as documented");

}  // namespace

extern "C" {

int wtamd_text_runs(const char *text, int64_t n_bytes, uint32_t flags, wtamd_read_state *state, int32_t *start, int32_t *finish, double *value,
                    int64_t capacity, int64_t *seg_off, int64_t *seg_name_off, int32_t *seg_name_len, int64_t seg_capacity, int64_t *slow_rec,
                    int64_t *slow_off, int64_t slow_capacity, wtamd_read_counts *counts, void *stream) {
    HipReadLauncher l{{(hipStream_t) stream, __FILE__}};
    const char *why = "";
    const int rc = wtr_door(l, text, (long long) n_bytes, (unsigned int) flags, (WtrState *) state, start, finish, value, (long long) capacity, seg_off,
                            seg_name_off, seg_name_len, (long long) seg_capacity, slow_rec, slow_off, (long long) slow_capacity, (WtrCounts *) counts, &why);
    if (rc == 3) return wt_fail(WTAMD_ERR_CAPACITY, "wtamd_text_runs: the output arrays are too small (counts holds n_runs, n_seg and n_slow needed)");
    return wt_runs_report("wtamd_text_runs", rc, why);
}

// The text and the outputs in HOST memory: device memory from the pool, copies and the call on the null stream; the slow
// values by strtod, the names copied out.
int wtamd_text_runs_host(const char *text, int64_t n_bytes, uint32_t flags, wtamd_read_state *state, int32_t *start, int32_t *finish, double *value,
                         int64_t capacity, int64_t *seg_off, int64_t *seg_name_off, int32_t *seg_name_len, int64_t seg_capacity, char *seg_name,
                         int64_t seg_name_cap, wtamd_read_counts *counts) {
    if (!state || !counts || n_bytes < 0 || capacity < 0 || seg_capacity < 0 || seg_name_cap < 0 || (n_bytes > 0 && !text) || (seg_name_cap > 0 && !seg_name))
        return wt_fail(WTAMD_ERR_ARG, "wtamd_text_runs_host: bad argument");
    HipReadLauncher l{{nullptr, __FILE__}};
    WcvScope<HipReadLauncher> sc(l);
    char *d_text = nullptr;
    int32_t *d_start = nullptr, *d_len = nullptr;
    double *d_value = nullptr;
    int64_t *d_seg = nullptr, *d_noff = nullptr, *d_slow = nullptr;
    const size_t cap = (size_t) capacity, scap = (size_t) seg_capacity;
    if (!sc.get(&d_text, (size_t) n_bytes) || !sc.get(&d_start, 2 * cap) || !sc.get(&d_value, cap) || !sc.get(&d_seg, 2 * scap + 1) || !sc.get(&d_len, scap))
        return wt_fail(WTAMD_ERR_HIP, "wtamd_text_runs_host: out of device memory");
    d_noff = d_seg + scap + 1;
    if (n_bytes > 0) WT_HIP(hipMemcpy(d_text, text, (size_t) n_bytes, hipMemcpyHostToDevice));
    const wtamd_read_state before = *state;
    int64_t slow_cap = 1024;
    int rc = WTAMD_OK;
    for (int attempt = 0; attempt < 2; attempt++) {
        if (!sc.get(&d_slow, (size_t) (2 * slow_cap))) return wt_fail(WTAMD_ERR_HIP, "wtamd_text_runs_host: out of device memory");
        rc = wtamd_text_runs(d_text, n_bytes, flags, state, d_start, d_start + cap, d_value, capacity, d_seg, d_noff, d_len, seg_capacity, d_slow,
                             d_slow + slow_cap, slow_cap, counts, nullptr);
        if (rc != WTAMD_ERR_CAPACITY || counts->n_runs > capacity || counts->n_seg > seg_capacity || counts->n_slow <= slow_cap) break;
        slow_cap = counts->n_slow;              // (only the slow list was too small: once more with the count needed)
    }
    if (rc != WTAMD_OK) return rc;
    const size_t n = (size_t) counts->n_runs, ns = (size_t) counts->n_seg, nw = (size_t) counts->n_slow;
    std::vector<int64_t> h_seg(ns + 1), h_noff(ns), h_slow(2 * nw);
    std::vector<int32_t> h_len(ns);
    if (n > 0) {
        WT_HIP(hipMemcpy(h_seg.data(), d_seg, sizeof(int64_t) * (ns + 1), hipMemcpyDeviceToHost));
        WT_HIP(hipMemcpy(h_noff.data(), d_noff, sizeof(int64_t) * ns, hipMemcpyDeviceToHost));
        WT_HIP(hipMemcpy(h_len.data(), d_len, sizeof(int32_t) * ns, hipMemcpyDeviceToHost));
    }
    size_t need = 0;
    for (size_t g = 0; g < ns; g++) need += (size_t) h_len[g] + 1;
    if (seg_name && need > (size_t) seg_name_cap) {
        *state = before;
        return wt_fail(WTAMD_ERR_CAPACITY, "wtamd_text_runs_host: seg_name is too small for the names");
    }
    if (n > 0) {
        WT_HIP(hipMemcpy(start, d_start, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
        WT_HIP(hipMemcpy(finish, d_start + cap, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
        WT_HIP(hipMemcpy(value, d_value, sizeof(double) * n, hipMemcpyDeviceToHost));
        memcpy(seg_off, h_seg.data(), sizeof(int64_t) * (ns + 1));
        memcpy(seg_name_off, h_noff.data(), sizeof(int64_t) * ns);
        memcpy(seg_name_len, h_len.data(), sizeof(int32_t) * ns);
    }
    if (nw > 0) {
        WT_HIP(hipMemcpy(h_slow.data(), d_slow + slow_cap, sizeof(int64_t) * nw, hipMemcpyDeviceToHost));
        WT_HIP(hipMemcpy(h_slow.data() + nw, d_slow, sizeof(int64_t) * nw, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < nw; k++) {
            const char *p = text + h_slow[k], *e = p;
            while (e < text + n_bytes && *e != '\n') e++;
            value[h_slow[nw + k]] = wtr_strtod(std::string(p, (size_t) (e - p)).c_str());
        }
    }
    if (seg_name) {
        char *o = seg_name;
        for (size_t g = 0; g < ns; g++) {
            const char *src = h_noff[g] == WTR_STATE_NAME ? before.chrom : h_noff[g] == WTR_STATE_REC ? before.rec_name : text + h_noff[g];
            memcpy(o, src, (size_t) h_len[g]);
            o[h_len[g]] = 0;
            o += h_len[g] + 1;
        }
    }
    l.quiet = true;             // (the call waited for its stream and the copies home for the device: the buffers are idle)
    return WTAMD_OK;
}

}  // extern "C"
