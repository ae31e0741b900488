// wt_pool.hip -- the library's ONE instance of the two process-wide pools declared in wt_pool.h: page-locked host memory
// (hipHostMalloc, or anonymous mappings registered by the page) and device buffers, kept when their user lets go of them.
// The engine's track sets (wt_engine.hip), the temporary buffers of a host entry point (wt_devscope.h) and the pipes
// (wt_pipe.hip) all draw on them; wtamd_pool_stats / wtamd_pool_trim speak for all of them.
#include <sys/mman.h>

#include <atomic>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "wt_pool.h"

// Page-locked (hipHostMalloc / hipHostRegister) host memory is readable by kernels; pageable memory
// is not -- such ranges go through hipMemcpyAsync, which stages them.
static bool wt_is_registered(const void *q);
bool wt_is_pinned(const void *q) {
    if (wt_is_registered(q)) return true;       // (this library's own mmap + hipHostRegister buffers, below)
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, q) != hipSuccess) { (void) hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}

// Page-locked host memory is expensive to get (hipHostMalloc pins pages at ~6 GB/s: the three slots of a pipe that
// streams 300 MB batches cost ~0.25 s) and to give back (hipHostFree waits for the device).  Buffers of 1 MB and more
// are therefore kept in a process-wide pool when a pipe lets go of them and handed to the next pipe that asks for
// the same size -- the Multiplexer a reducer takes over, the next reducer of a long-lived process.  Smaller buffers rest
// there too (a track set's counters and table staging: hipHostMalloc + hipHostFree of a few bytes cost 0.25 ms per track
// set), but only those of 1 MB and more are counted as misses.  Bounded by
// WTAMD_PINNED_POOL_MB (default 8192: a pipe of 100 BigWig tracks holds 3.7 GB; 0 switches the pool off).
struct WtPinnedPool {
    std::mutex mu;
    std::multimap<size_t, void *> free_list;        // by (rounded) size
    std::map<void *, size_t> size_of;               // every live buffer that came through here
    size_t pooled = 0;
    size_t misses = 0, miss_bytes = 0;              // buffers of 1 MB and more that had to be page-locked afresh
    size_t limit() const {
        const char *e = getenv("WTAMD_PINNED_POOL_MB");
        return (size_t) (e ? atoll(e) : 8192) << 20;
    }
};
static WtPinnedPool g_pinned_pool;

// Sizes of 1 MB and more are rounded up to eighths of their power of two before they reach the pool or the runtime:
// the staging of a file-byte batch is sized by the batch (306 995 195 bytes, then 308 322 053, ...), so the next run
// of the same job never asked for exactly what the previous one had returned and page-locked everything afresh --
// 0.8 s of hipHostMalloc on hosts where that runs at 1.5 GB/s (round 3; seen as a second run SLOWER than the first).
size_t wt_pool_round(size_t bytes) {
    if (bytes < (1u << 20)) return (bytes + 255) / 256 * 256;      // (small buffers: a few size classes, so that they meet again)
    int lg = 63;
    while (!((bytes >> lg) & 1u)) lg--;
    const size_t step = (size_t) 1 << (lg - 3);
    return (bytes + step - 1) / step * step;
}

// Page-locking by the page.  hipHostMalloc allocates AND faults AND pins from one thread: 176-229 ms per GiB on the
// MI355X hosts measured (tools/probes/cold_probe.hip; 4.3 GB of staging = 0.3-0.8 s of a cold file-byte run, round 4's
// "pinned_afresh").  The same GiB as an anonymous mapping with transparent huge pages, faulted in by 16 threads
// (4 ms) and then registered (hipHostRegister: 2 ms -- 512 huge pages to pin instead of 262 144 small ones) costs 6 ms,
// and the copy engine reads it at the same 57 GB/s.  Buffers of 2 MB and more take that route (WTAMD_PIN=malloc: the
// old one); anything the runtime refuses falls back to hipHostMalloc.
struct WtRegistered { void *base; size_t map_len; size_t len; };   // the mapping (for munmap) and the page-locked bytes from the pointer handed out
static std::mutex g_reg_mu;
static std::map<void *, WtRegistered> g_registered;        // registered mappings, by the pointer handed out
static std::atomic<int> g_reg_state{0};                      // 0 untried, 1 works, -1 does not (hipHostMalloc from then on)
static std::atomic<int> g_reg_failures{0};                   // hipHostRegister refusals in a row (a transient one -- RLIMIT_MEMLOCK on one large buffer -- does not end the route)

static bool wt_is_registered(const void *q) {
    std::lock_guard<std::mutex> lk(g_reg_mu);
    auto it = g_registered.upper_bound((void *) q);
    if (it == g_registered.begin()) return false;
    --it;
    return (const char *) q < (const char *) it->first + it->second.len;       // (the mapping's alignment slack behind it is NOT page-locked)
}

static int wt_pin_threads() {
    static const int n = [] {
        int c = (int) std::thread::hardware_concurrency();
        if (FILE *fp = fopen("/sys/fs/cgroup/cpu.max", "r")) {       // (the container's CPU quota: the GPU boxes show 256 CPUs and grant 16)
            char q[64]; long long period = 0;
            if (fscanf(fp, "%63s %lld", q, &period) == 2 && period > 0 && strcmp(q, "max") != 0) {
                const long long k = atoll(q) / period;
                if (k >= 1 && k < c) c = (int) k;
            }
            fclose(fp);
        }
        return c < 1 ? 1 : (c > 16 ? 16 : c);
    }();
    return n;
}

static bool wt_pin_by_register(void **out, size_t bytes) {
    static const bool off = getenv("WTAMD_PIN") && !strcmp(getenv("WTAMD_PIN"), "malloc");
    if (off || g_reg_state.load() < 0 || bytes < ((size_t) 2 << 20)) return false;
    const size_t huge = (size_t) 2 << 20;
    const size_t len = (bytes + huge - 1) / huge * huge;
    void *base = mmap(nullptr, len + huge, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (base == MAP_FAILED) return false;
    char *p = (char *) (((uintptr_t) base + huge - 1) & ~(uintptr_t) (huge - 1));
#ifdef MADV_HUGEPAGE
    (void) madvise(p, len, MADV_HUGEPAGE);
#endif
    // fault the pages in from several threads (one touch per 4 KB: right with and without huge pages)
    int T = wt_pin_threads();
    const size_t per_thread_min = (size_t) 32 << 20;
    if ((size_t) T > len / per_thread_min) T = (int) (len / per_thread_min);
    if (T < 1) T = 1;
    const size_t slice = (len / (size_t) T + huge - 1) / huge * huge;
    auto touch = [p, len, slice](int t) {
        const size_t a = slice * (size_t) t, b = a + slice < len ? a + slice : len;
        for (size_t q = a; q < b; q += 4096) ((volatile char *) p)[q] = 0;
    };
    std::vector<std::thread> th;
    for (int t = 1; t < T; t++) th.emplace_back(touch, t);
    touch(0);
    for (auto &t : th) t.join();
    void *dp = nullptr;
    const bool registered = hipHostRegister(p, len, hipHostRegisterDefault) == hipSuccess;
    if (!registered || hipHostGetDevicePointer(&dp, p, 0) != hipSuccess || dp != (void *) p) {
        // (kernels of the pipe read and write the staging through the HOST address: it must be the device's too)
        (void) hipGetLastError();
        // a host pointer that is not the device's: this runtime cannot do it, ever; a refused registration: maybe just this size, now
        const bool never = registered;
        if (registered) (void) hipHostUnregister(p);
        munmap(base, len + huge);
        if (never || g_reg_failures.fetch_add(1) + 1 >= 3) g_reg_state.store(-1);
        return false;
    }
    g_reg_state.store(1);
    g_reg_failures.store(0);
    { std::lock_guard<std::mutex> lk(g_reg_mu); g_registered[p] = WtRegistered{base, len + huge, len}; }
    *out = p;
    return true;
}

static hipError_t wt_pin_raw_alloc(void **out, size_t bytes) {
    if (wt_pin_by_register(out, bytes)) return hipSuccess;
    return hipHostMalloc(out, bytes, hipHostMallocDefault);
}

static void wt_pin_raw_free(void *q) {
    WtRegistered r{nullptr, 0};
    {
        std::lock_guard<std::mutex> lk(g_reg_mu);
        auto it = g_registered.find(q);
        if (it != g_registered.end()) { r = it->second; g_registered.erase(it); }
    }
    if (r.base) { (void) hipHostUnregister(q); munmap(r.base, r.map_len); }
    else (void) hipHostFree(q);
}

hipError_t wt_host_alloc(void **out, size_t bytes) {
    if (bytes < 1) bytes = 1;
    bytes = wt_pool_round(bytes);
    {
        std::lock_guard<std::mutex> lk(g_pinned_pool.mu);
        // the smallest resting buffer that is large enough and at most a quarter larger (slot capacities grow by
        // doubling from whatever the first batches needed, so two runs of one job rarely end on identical sizes)
        auto it = g_pinned_pool.free_list.lower_bound(bytes);
        if (it != g_pinned_pool.free_list.end() && it->first <= bytes + bytes / 4) {
            *out = it->second;
            g_pinned_pool.pooled -= it->first;
            g_pinned_pool.free_list.erase(it);
            return hipSuccess;
        }
    }
    const auto t_alloc0 = std::chrono::steady_clock::now();
    hipError_t e = wt_pin_raw_alloc(out, bytes);
    if (e != hipSuccess) {
        // the host refuses to page-lock more while buffers rest in the pool: give them all back and try once more
        std::vector<void *> idle;
        {
            std::lock_guard<std::mutex> lk(g_pinned_pool.mu);
            for (auto &kv : g_pinned_pool.free_list) { idle.push_back(kv.second); g_pinned_pool.size_of.erase(kv.second); }
            g_pinned_pool.free_list.clear();
            g_pinned_pool.pooled = 0;
        }
        if (!idle.empty()) {
            (void) hipGetLastError();
            for (void *x : idle) wt_pin_raw_free(x);
            e = wt_pin_raw_alloc(out, bytes);
        }
    }
    if (e == hipSuccess && bytes < (1u << 20)) {
        std::lock_guard<std::mutex> lk(g_pinned_pool.mu);
        g_pinned_pool.size_of[*out] = bytes;
    } else if (e == hipSuccess) {
        std::lock_guard<std::mutex> lk(g_pinned_pool.mu);
        g_pinned_pool.size_of[*out] = bytes;
        g_pinned_pool.misses++;
        g_pinned_pool.miss_bytes += bytes;
        static const bool trace = getenv("WTAMD_TRACE_POOL") != nullptr;
        bool by_register = false;
        if (trace) { std::lock_guard<std::mutex> lk2(g_reg_mu); by_register = g_registered.count(*out) != 0; }
        if (trace) fprintf(stderr, "[pool] page-locked %.1f MB (%s) in %.1f ms\n", bytes / 1048576.0, by_register ? "mmap + hipHostRegister" : "hipHostMalloc",
                           std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_alloc0).count());
    }
    return e;
}

void wt_host_free(void *q) {
    if (!q) return;
    {
        std::lock_guard<std::mutex> lk(g_pinned_pool.mu);
        auto it = g_pinned_pool.size_of.find(q);
        if (it != g_pinned_pool.size_of.end()) {
            if (g_pinned_pool.pooled + it->second <= g_pinned_pool.limit()) {
                g_pinned_pool.free_list.emplace(it->second, q);
                g_pinned_pool.pooled += it->second;
                return;
            }
            g_pinned_pool.size_of.erase(it);
        }
    }
    wt_pin_raw_free(q);
}

// Device buffers, the same way: a pipe frees everything it holds when its reducer reaches the end of the data
// (35 hipFree calls, each of which synchronises the device and unmaps gigabytes), and the next reducer of the process
// maps it all again -- on some hosts that made the SECOND run of a job 2 x slower than the first (0.9 s inside
// wtamd_pipe_submit_bw for 27 batches; round 3).  Released buffers rest in a process-wide pool keyed by (device,
// rounded size); a pipe is destroyed only after its streams have been synchronised, so nothing in the pool is still
// in use.  Bounded by WTAMD_DEVICE_POOL_MB per process (default 65536 -- a pipe of 100 tracks holds 38 GB; 0 switches the pool off).
struct WtDevPool {
    std::mutex mu;
    std::multimap<std::pair<int, size_t>, void *> free_list;
    std::map<void *, std::pair<int, size_t>> size_of;
    size_t pooled = 0, misses = 0, miss_bytes = 0;
    size_t limit() const {
        const char *e = getenv("WTAMD_DEVICE_POOL_MB");
        return (size_t) (e ? atoll(e) : 65536) << 20;
    }
};
static WtDevPool g_dev_pool;

hipError_t wt_dev_alloc_bytes(void **out, size_t bytes, const char *file, int line) {
    if (bytes < 1) bytes = 1;
    bytes = wt_pool_round(bytes);
    int dev = 0;
    (void) hipGetDevice(&dev);
    {
        std::lock_guard<std::mutex> lk(g_dev_pool.mu);
        auto it = g_dev_pool.free_list.lower_bound({dev, bytes});       // (same rule as the pinned pool)
        if (it != g_dev_pool.free_list.end() && it->first.first == dev && it->first.second <= bytes + bytes / 4) {
            *out = it->second;
            g_dev_pool.pooled -= it->first.second;
            g_dev_pool.free_list.erase(it);
            return hipSuccess;
        }
    }
    void *q = nullptr;
    const auto t_alloc0 = std::chrono::steady_clock::now();
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) {
        // out of device memory with buffers resting in the pool: give them all back and try once more
        std::vector<void *> idle;
        {
            std::lock_guard<std::mutex> lk(g_dev_pool.mu);
            for (auto &kv : g_dev_pool.free_list) { idle.push_back(kv.second); g_dev_pool.size_of.erase(kv.second); }
            g_dev_pool.free_list.clear();
            g_dev_pool.pooled = 0;
        }
        if (!idle.empty()) {
            (void) hipGetLastError();
            for (void *x : idle) (void) hipFree(x);
            e = hipMalloc(&q, bytes);
        }
    }
    *out = q;
    if (e == hipSuccess) {
        std::lock_guard<std::mutex> lk(g_dev_pool.mu);
        g_dev_pool.size_of[q] = {dev, bytes};
        g_dev_pool.misses++;
        g_dev_pool.miss_bytes += bytes;
        static const bool trace = getenv("WTAMD_TRACE_POOL") != nullptr;
        if (trace && bytes >= (1u << 20)) fprintf(stderr, "[pool] hipMalloc %.1f MB in %.1f ms (device %d, %s:%d)\n", bytes / 1048576.0,
                                                  std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_alloc0).count(), dev, file, line);
    }
    return e;
}

hipError_t wt_dev_free(void *q) {
    if (!q) return hipSuccess;
    {
        std::lock_guard<std::mutex> lk(g_dev_pool.mu);
        auto it = g_dev_pool.size_of.find(q);
        if (it != g_dev_pool.size_of.end()) {
            if (g_dev_pool.pooled + it->second.second <= g_dev_pool.limit()) {
                g_dev_pool.free_list.emplace(it->second, q);
                g_dev_pool.pooled += it->second.second;
                return hipSuccess;
            }
            g_dev_pool.size_of.erase(it);
        }
    }
    return hipFree(q);
}


// The rule of both pools: they hand a resting buffer to the next caller at once and wait for nothing, so A BUFFER RETURNS
// TO A POOL ONLY AFTER THE DEVICE HAS FINISHED WITH IT.  hipFree / hipHostFree used to provide that wait for every single
// buffer; the owner now provides it once for all it is about to return -- wtamd_trackset_destroy and WtDevScope's
// destructor before their first buffer, a growing table (wt_grow, wt_get_windows) once per growth, a pipe by synchronising
// its streams before it is destroyed.  Work may be in flight on any stream of the caller's, so the wait is for the device.
hipError_t wt_pool_quiesce() { return hipDeviceSynchronize(); }

extern "C" {

void wtamd_pool_trim(void) {
    std::vector<void *> host, dev;
    {
        std::lock_guard<std::mutex> lk(g_pinned_pool.mu);
        for (auto &kv : g_pinned_pool.free_list) { host.push_back(kv.second); g_pinned_pool.size_of.erase(kv.second); }
        g_pinned_pool.free_list.clear();
        g_pinned_pool.pooled = 0;
    }
    {
        std::lock_guard<std::mutex> lk(g_dev_pool.mu);
        for (auto &kv : g_dev_pool.free_list) { dev.push_back(kv.second); g_dev_pool.size_of.erase(kv.second); }
        g_dev_pool.free_list.clear();
        g_dev_pool.pooled = 0;
    }
    for (void *x : host) wt_pin_raw_free(x);
    for (void *x : dev) (void) hipFree(x);
}

void wtamd_pool_stats(int64_t out[6]) {
    if (!out) return;
    {
        std::lock_guard<std::mutex> lk(g_pinned_pool.mu);
        out[0] = (int64_t) g_pinned_pool.misses; out[1] = (int64_t) g_pinned_pool.miss_bytes; out[2] = (int64_t) g_pinned_pool.pooled;
    }
    std::lock_guard<std::mutex> lk(g_dev_pool.mu);
    out[3] = (int64_t) g_dev_pool.misses; out[4] = (int64_t) g_dev_pool.miss_bytes; out[5] = (int64_t) g_dev_pool.pooled;
}

}  // extern "C"
