// wt_pipe.h -- the streaming pipeline (wtamd_pipe_*, include/wiggletools_amd.h): its slots and the pipe itself.  The code is
// wt_pipe.hip, built on the engine's track sets (wt_trackset.h) and the pools of wt_pool.h.
//
// The reference overlaps its readers with the evaluation through producer threads and
// 10 000-entry SoA blocks, at most 3 blocks ahead (bufferedReader.c:17-28,41-55,99-109).  Here
// the same role is played across host, PCIe and GPU by `n_slots` batch slots and three HIP streams:
//
//      host (Drainer)     fill k+2 | fill k+3 | ...
//      copy stream        H2D k+1  | H2D k+2  | ...          hipMemcpyAsync from PINNED staging
//      compute stream     index + multiplex/reduce kernels k | k+1 | ...
//      result stream      D2H k-1 (exactly the emitted runs) | D2H k | ...   into PINNED output
//
// Events order the three streams per slot; nothing is allocated, freed or synchronised per batch
// (staging, device buffers and window tables only ever grow) and the host never has to learn a
// run count before the result can travel: the export kernel reads it on the device and writes
// exactly the emitted runs (and the counters) into the slot's pinned output through the link.
// All three legs are KERNELS -- gather (reads the page-locked run lists over PCIe), the
// multiplex/reduce kernels, export (writes over PCIe) -- so consecutive batches overlap on the
// GPU's queues without SDMA hand-offs in between (measured: with hipMemcpyAsync legs the next
// batch's H2D did not start before the previous batch's D2H had finished).  A batch whose
// difference-array launch reported windows it could not prove exact (rare: NaN, Inf, huge dynamic
// range) is patched and exported again when it is collected.
#ifndef WT_PIPE_H_
#define WT_PIPE_H_

#include <string>
#include <vector>

#include "wt_trackset.h"

// Gather: ONE kernel pulls every range of a batch -- the caller's pinned SoA blocks (bulk side
// door) and the staged ranges alike -- from host memory into the slot's device arrays.  The copy
// engine needs three hipMemcpyAsync per track and batch (~10 us of launch overhead each: 300 calls
// for 100 tracks, more than the transfer itself at 4 M intervals per batch); a kernel reading the
// page-locked host arrays through the PCIe link has no per-range cost and keeps thousands of reads
// in flight.  Host bandwidth is the bound either way (12 B per interval).
struct WtGatherSeg {
    const int32_t *start, *finish;
    const float *value;
    long long dst;                  // first interval of the range in the device arrays
    long long count;
    long long chunk_first;          // prefix sum of ceil(count / WT_GATHER_CHUNK)
};
#define WT_GATHER_CHUNK 4096

#define WT_GATHER_MAX_SEGS 1024      // table entries one launch caches in LDS (48 KB)

struct WtSlot {
    int state = 0;                  // 0 free, 1 acquired, 2 submitted, 3 collected
    // input staging (pinned) and its device twin
    int64_t cap = 0;
    bool has64 = false;
    int64_t *h_seg = nullptr;
    int32_t *h_start = nullptr, *h_finish = nullptr;
    float *h_v32 = nullptr;
    double *h_v64 = nullptr;
    int64_t dcap = 0;
    bool d_has64 = false;
    int32_t *d_start = nullptr, *d_finish = nullptr;
    void *d_value = nullptr;
    // output: device + pinned
    int64_t ocap = 0;
    int32_t *d_os = nullptr, *d_of = nullptr;
    double *d_ov = nullptr, *d_tile = nullptr;
    uint8_t *d_ip = nullptr;
    int64_t *d_cro = nullptr;
    int32_t *h_os = nullptr, *h_of = nullptr;
    double *h_ov = nullptr, *h_tile = nullptr;
    uint8_t *h_ip = nullptr;
    wtamd_trackset *ts = nullptr;
    hipEvent_t e_h0 = nullptr, e_h1 = nullptr, e_k0 = nullptr, e_cnt = nullptr, e_patch = nullptr, e_d0 = nullptr, e_d1 = nullptr;
    // the batch in flight
    int64_t n_int = 0, n_runs = 0, covered = 0;
    bool f64 = false, used_delta = false, patched = false;
    int err = WTAMD_OK;
    std::string err_msg;
    int delta_W = 0;
    // bulk side door: ranges of the batch that are copied to HBM straight from the caller's arrays
    struct Direct { int64_t at, count; const int32_t *start, *finish; const float *value; };
    std::vector<Direct> direct;
    WtGatherSeg *h_segs = nullptr;  // gather table, pinned (the kernel reads it where it lies)
    // device-side run compression (WTAMD_PIPE_COMPRESS): merged runs + scratch bitmaps, sized with the output
    int32_t *d_cs = nullptr, *d_cf = nullptr;
    double *d_cv = nullptr;
    unsigned long long *d_cscratch = nullptr, *d_cn = nullptr;
    bool compressed = false;        // this batch's output went through the compression
    // operator chains (wtamd_pipe_set_map): mapped f64 values, compacted coordinates, raw offsets, scratch
    int64_t mcap = 0;
    bool m_has_coords = false;
    int32_t *d_mstart = nullptr, *d_mfinish = nullptr;
    double *d_mvalue = nullptr;
    int64_t *d_mseg = nullptr;
    unsigned long long *d_mscratch = nullptr;
    int64_t seg_cap = 0;
    bool direct_pinned = true;      // every direct range of this batch lies in page-locked memory
    // BigWig sections decoded on device (wtamd_pipe_submit_bw): pinned staging [track table | section table | file
    // bytes] and its device twin (ONE copy kernel moves all three), decode scratch, status words
    uint8_t *h_bw = nullptr, *d_bw = nullptr;
    int64_t h_bw_cap = 0, d_bw_cap = 0;
    int64_t bw_off_sec = 0, bw_off_bytes = 0;       // layout of the reserved staging
    int64_t bw_res_bytes = -1, bw_res_secs = -1;     // what wtamd_pipe_bw_reserve was asked for (-1: nothing reserved)
    int64_t bw_bytes = 0, bw_stride = 0;             // of the batch in flight (a batch that overflowed its run lists is decoded again)
    int64_t bw_bound = 0;                            // the host's upper bound of its intervals
    int bw_dec = 0;                                  // decode stream (and scratch) of the batch
    unsigned long long *h_bw_status = nullptr;       // pinned: error bits, pieces
    hipEvent_t e_bwc = nullptr, e_bw0 = nullptr, e_bw1 = nullptr;
    bool bw = false;                                 // the batch in flight came as file bytes
    int64_t bw_secs = 0;
    bool export_pending = false;                     // the runs travel by copy engine once the host knows their count (collect)
    // fused integrators (wtamd_pipe_set_integrate): partial sums / moments on device, the batch's integrals in pinned memory
    char *d_integ = nullptr;
    double *h_integ = nullptr;
    bool integrated = false;
    int integ_mode = 0;             // what s.h_integ holds: 1 {sum, span} / the Pearson moments, 2 the run moments (wt_moments.hip)
};

// HIP's current device is per thread; a pipe lives on the device that was current when it was created, and the drop-in
// layer drives several pipes (one per GPU: WTAMD_DEVICES) from one thread.
struct WtDevGuard {
    int prev = -1;
    explicit WtDevGuard(int dev) {
        int cur = -1;
        if (hipGetDevice(&cur) == hipSuccess && cur != dev && dev >= 0) { prev = cur; (void) hipSetDevice(dev); }
    }
    ~WtDevGuard() { if (prev >= 0) (void) hipSetDevice(prev); }
};

struct wtamd_pipe {
    wtamd_pipe_config cfg;
    int device = -1;
    std::vector<double> defaults;
    std::vector<WtSlot> slots;
    int head = 0, tail = 0, acquired = -1, in_flight = 0, held = 0;
    hipStream_t s_copy = nullptr, s_comp = nullptr, s_out = nullptr, s_dec = nullptr;
    // File-byte batches are inflated / decoded on the compute stream.  WTAMD_BW_DECODE_STREAMS=2: on two streams of their
    // own taking turns, so that the next batch's inflate kernel takes the lanes the part-filled last batch of a
    // chromosome leaves idle (a launch costs ~12 ms however few sections it holds).  Measured (round 4, 100 files x 24
    // chromosomes at GRCh38 x 0.2): SLOWER, 0.75 s against 0.68 s -- the workgroups of inflate(k + 1) hold their CUs for
    // 12 ms and the reduce kernels of batch k, which need whole CUs, wait behind them; the host then waits longer for
    // batch k and, with two batches in flight, submits k + 2 later.  Kept as a switch, off.
    hipStream_t s_decs[2] = {nullptr, nullptr};
    int n_decs = 0;
    int64_t bw_batches = 0;
    bool delta_failed = false;      // a batch had many inexact windows: Sum / Mean stay on the general kernel
    bool tile = false;
    bool compress = false;          // WTAMD_PIPE_COMPRESS: batches submitted from now on are merged on device before they travel
    int integrate = 0;              // wtamd_pipe_set_integrate (0 off, 1 sums / Pearson, 2 run moments): batches submitted from now on are integrated on device, no runs travel
    bool gather = true;             // WTAMD_PIPE_GATHER=0: hipMemcpyAsync per range instead of the gather kernel
    int gather_blocks = 64;         // WTAMD_GATHER_BLOCKS
    // buffers a slot outgrew: released when the pipe is destroyed -- hipFree / hipHostFree wait for the
    // whole device, i.e. for the batches in flight on the other slots (measured: 6-8 ms per growing
    // submit while the pipeline ramps up)
    std::vector<void *> dead_dev, dead_host;
    void *d_chains = nullptr;       // wtamd_pipe_set_map: per-track operator chains on device
    bool map_drops = false;         // ... some operator drops runs: batches are compacted
    bool map_f32 = false;           // ... every operator is float32-exact: float32 batches stay float32 (and on the exact kernels)
    int num_cu = 256;
    // File-byte batches: the inflate scratch is ONE per pipe -- every decode runs on the compute stream, in order, and
    // is through with the scratch before the next one starts (round 3 kept 0.8 GB of it in each of four slots).
    void *d_bw_scratch = nullptr;   // (the scratch of the decode stream in use: d_bw_scratches[k])
    int64_t bw_scratch_cap = 0;
    void *d_bw_scratches[2] = {nullptr, nullptr};
    int64_t bw_scratch_caps[2] = {0, 0};
    // ... and their run lists are sized from the densest batch seen so far (intervals / host bound), not from the bound:
    // the bound must assume 4-byte fixedStep items because the item type is inside the compressed stream, three times
    // what bedGraph sections hold.  A batch that does not fit reports WT_BW_ERR_CAPACITY and is decoded again at full
    // size when it is collected (wt_pipe_bw_redo); from then on the pipe sizes by the bound.  < 0: nothing seen yet.
    double bw_density = -1.0;
    int64_t bw_redone = 0;
    unsigned last_bw_err = 0;       // wtamd_pipe_bw_error
    wtamd_pipe_stats st{};
};

#endif  // WT_PIPE_H_
