// wt_trackset.h -- the engine's internal interface (wt_engine.hip): the track set, its window tables and the engine
// functions the streaming pipeline (wt_pipe.hip) is built on.  Host side only.  Every device and pinned buffer named here
// comes from the pools of wt_pool.h and returns to them (d_gscratch and the MWU tables excepted: hipMalloc / hipFree).
#ifndef WT_TRACKSET_H_
#define WT_TRACKSET_H_

#include <map>
#include <vector>

#include "wt_host.h"
#include "wt_plan.h"

struct WtWindows {
    WtPlan plan_geom;        // only W matters for the tables
    WtWindowTables tab;
    int32_t *d_cbase = nullptr, *d_cnwin = nullptr, *d_chi = nullptr, *d_win_chrom = nullptr;
    int64_t *d_cfirst = nullptr;
    uint32_t *d_widx = nullptr;
    uint32_t *d_cidx = nullptr;         // coarse index of the searched window index (every 64th row)
    unsigned long long *d_status = nullptr;
    int32_t *d_bad_list = nullptr;      // difference-array launches: windows not provably exact ...
    long long *d_bad_goff = nullptr;    // ... and where their runs start (both [n_windows])
    bool indexed = false;
    // capacities of the device tables (entries); the tables are reused and only ever grow
    int64_t cap_chrom = 0, cap_win = 0, cap_widx = 0, cap_bad = 0, cap_cidx = 0;
    bool tab_valid = false;             // tab / device tables describe the track set's current data
    // Pinned staging of the per-chromosome tables, packed as they lie at the head of d_tabs: ONE asynchronous copy on the launch
    // stream uploads them (win_chrom[] is filled on the device).  The staging is this WtWindows' own and is rewritten only after
    // the event behind its previous upload has completed.
    char *h_tab = nullptr;
    int64_t h_tab_bytes = 0;
    hipEvent_t ev_tab = nullptr;        // recorded behind every upload
    bool tab_in_flight = false;         // an upload was enqueued since ev_tab was last waited for
    // round 6: cbase | cnwin | chi | cfirst | win_chrom live in ONE allocation (d_tabs) and travel in ONE copy -- a NEW track set's first
    // index paid five hipMallocs and five blocking copies for them, 0.1 ms of host time per chromosome of a resident pass
    char *d_tabs = nullptr;
    int64_t cap_tabs = 0;               // bytes
};

struct wtamd_trackset {
    int n_chrom = 0, n_tracks = 0;
    bool value_f64 = false;
    bool owns = false;
    int64_t n_intervals = 0;
    std::vector<int64_t> seg_off;
    std::vector<double> defaults;
    std::vector<int32_t> first_start, last_finish;
    std::vector<int32_t> range_lo, range_hi;     // optional run-start ranges (empty = none)
    int32_t *d_start = nullptr, *d_finish = nullptr;
    void *d_value = nullptr;
    int64_t *d_seg_off = nullptr;
    double *d_defaults = nullptr;
    unsigned long long *d_counters = nullptr;
    unsigned long long *h_counters = nullptr;   // pinned
    unsigned long long *h_debug = nullptr;      // pinned, device-visible (debug builds)
    int64_t *d_chrom_run_off = nullptr;         // scratch when the caller passes none
    // zero-copy track sets: (first start | last finish) of every segment as the device reads them off the run lists, and the
    // pinned buffer one asynchronous copy brings them to (wt_refresh_extents_device)
    int32_t *d_extents = nullptr, *h_extents = nullptr;
    char *d_gscratch = nullptr;                 // median / MWU columns of very many tracks (grown on demand)
    size_t gscratch_bytes = 0;
    double *d_mwu_table = nullptr;              // MWUReduction's last step as a table (wt_mwu_make_table), for set sizes mwu_n1 / mwu_n2
    int mwu_n1 = -1, mwu_n2 = -1, mwu_kmax = 0;
    int mwu_few_ties = -1;                      // MWUReduction's kernel by the data (wt_mwu_few_ties): -1 not looked at yet, 1 walk (wt_mwalk.h), 0 register columns
    std::vector<double *> mwu_retired;          // tables of earlier set sizes (freed with the track set)
    std::map<int, WtWindows> windows;           // keyed by W
    hipEvent_t ev_i0 = nullptr, ev_i1 = nullptr, ev_r0 = nullptr, ev_r1 = nullptr;
    bool have_index_time = false, have_reduce_time = false;
    wtamd_stats stats{};
    int device = 0;
    int num_cu = 256;
    bool scratch_f32 = false;
    // Sum / Mean over float tracks: what a completed difference-array launch found out about this data
    // the difference-array launches' verdict on this data, per class of reducer -- [0] Sum / Mean / the var family (exponent range
    // of a window), [1] TTestReduction (its own, narrower windows, and positions whose variance cancels: wt_delta_scan3_tt)
    // [2] Max / Min (only a NaN or a -0.0 sends a window to the general kernel)
    bool delta_failed_[3] = {false, false, false};      // many windows are not provably exact: the class uses the general kernel
    bool delta_verified_[3] = {false, false, false};    // verdict known: delta_n_bad windows (few) get patched by the general kernel
    long long delta_n_bad_[3] = {0, 0, 0};
    // pipeline slot (wt_pipe.hip): the run lists are rebound per batch, device tables are reused,
    // every upload is asynchronous on the launch stream from pinned staging
    bool pipe_mode = false;
};

void wt_warmup_join();          // waits for the helper thread of wtamd_warmup_async, if one is at it
// what both constructors share: the descriptor's check, the host copies, the small device tables, the events
int wt_trackset_common(const wtamd_tracks *t, wtamd_trackset *ts);
int wt_check_extents(wtamd_trackset *ts);
int wt_check_desc(const wtamd_trackset *ts, const wtamd_reduce_desc *d);

// A pipeline slot's track set takes on the next batch: `n` intervals in device run lists that are (or will be, on the
// stream the reduction is enqueued on) bound here, seg_off[n_tracks + 1] and ts->first_start / last_finish (upper bounds
// will do) as the host knows them.  Nothing that was learnt about the previous batch's data survives; delta_failed: the
// exact kernels are not to be tried on this one.
int wt_trackset_rebind(wtamd_trackset *ts, int64_t n, const int64_t *seg_off, int32_t range_lo, int32_t range_hi, bool value_f64,
                       int32_t *d_start, int32_t *d_finish, void *d_value, bool delta_failed);

// Plans the reduction of the track set's current data as wtamd_reduce would plan its first launch and enqueues it (window
// index included) on `s`; nothing is waited for, the counters stay on the device.  *used_delta: the difference-array kernel
// runs, with windows of *delta_W bp -- the caller reads WT_CTR_DELTA_BAD when the launch is through and patches
// (wt_launch_patch) what it reports.
int wt_reduce_enqueue(wtamd_trackset *ts, const wtamd_reduce_desc &desc, wtamd_runs *runs, double *d_tile, uint8_t *d_inplay,
                      hipStream_t s, bool *used_delta, int *delta_W);

// The general kernel over the `n_bad` windows the difference-array launch (window width delta_W,
// just finished or still running on `s`) recorded as not provably exact.
int wt_launch_patch(wtamd_trackset *ts, int delta_W, int op, uint32_t flags, int n_set0, wtamd_runs *runs, long long n_bad,
                    hipStream_t s);

// The Multiplexer tile of the track set's current data (the route of wtamd_multiplex_host) into DEVICE arrays, on `s`:
// runs (start, finish, value = the in-play count, chrom_run_off), d_tile[capacity * n_tracks], d_inplay likewise; *n_runs is
// written when the launch is through.  flags: WTAMD_STRICT_SET0 or 0.
int wt_multiplex_device(wtamd_trackset *ts, uint32_t flags, wtamd_runs *runs, double *d_tile, uint8_t *d_inplay, int64_t *n_runs,
                        hipStream_t s);

#endif  // WT_TRACKSET_H_
