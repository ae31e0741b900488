/*
 * wiggletools_amd.h -- C ABI of the MI355X-native multiplexer / reducer engine.
 *
 * Two layers are declared here:
 *
 *  (1) DROP-IN LAYER.  The symbols the reference's own callers bind
 *      (reference src/commandParser.c:500-569,635-651 call them; they are
 *      declared in reference src/wiggletools.h:80-103 and
 *      src/multiplexer.h:38-41, src/multiSet.h:32-33).  Same names, same C
 *      signatures, same struct layouts (reference src/wiggleIterator.h:21-35,
 *      src/multiplexer.h:21-36, src/multiSet.h:20-30), so that
 *      libwiggletools_amd.so can be linked in place of multiplexer.o /
 *      multiSet.o / reducers.o / setComparisons.o.  See INTEGRATION.md.
 *
 *  (2) BULK LAYER (wtamd_*).  Plain pointers + sizes.  This is what the
 *      drop-in layer itself calls once it has drained the child iterators
 *      into SoA batches, and what a bulk reader (BigWig section decoder)
 *      or bench.py binds directly when the tracks are already resident
 *      in HBM.
 *
 * No torch / C++ types appear in any signature.
 */
#ifndef WIGGLETOOLS_AMD_H_
#define WIGGLETOOLS_AMD_H_

#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ */
/* (1) DROP-IN LAYER                                                   */
/* ------------------------------------------------------------------ */

/* The reference spells its booleans `#define bool char`
 * (reference src/wiggletools.h:18-22).  We cannot #define bool in a header
 * that C++ also includes, so the ABI type is named explicitly. */
typedef char wt_bool;

typedef struct wiggleIterator_st WiggleIterator;
typedef struct multiplexer_st Multiplexer;
typedef struct multiset_st Multiset;

/* Layout == reference src/wiggleIterator.h:21-35 (88 bytes on LP64). */
struct wiggleIterator_st {
    char *chrom;
    int start;              /* 1-based, inclusive  */
    int finish;             /* exclusive           */
    double value;
    void *valuePtr;
    wt_bool done;
    int strand;
    void *data;
    void (*pop)(WiggleIterator *);
    void (*seek)(WiggleIterator *, const char *, int, int);
    wt_bool overlaps;
    double default_value;
    WiggleIterator *append;
};

/* Layout == reference src/multiplexer.h:21-36.  `starts`/`finishes` are the
 * reference's FibHeap pointers; this engine has no heaps and keeps them NULL. */
struct multiplexer_st {
    char *chrom;
    int start;
    int finish;
    double *values;
    double *default_values;
    int count, inplay_count;
    wt_bool *inplay;
    WiggleIterator **iters;
    wt_bool done;
    wt_bool strict;
    void (*pop)(Multiplexer *);
    void (*seek)(Multiplexer *, const char *, int, int);
    void *starts, *finishes;
    void *data;
};

/* Layout == reference src/multiSet.h:20-30. */
struct multiset_st {
    char *chrom;
    int start;
    int finish;
    double **values;
    int count, inplay_count;
    wt_bool *inplay;
    Multiplexer **multis;
    wt_bool done;
    void *starts, *finishes;
};

/* Iterator core -- replaces reference src/wiggleIterator.c:20-70.
 * (Provided so the library is self-contained; when linked into the reference
 * build the reference's wiggleIterator.o may be kept instead -- the semantics
 * are identical: ctor primes the first element, pop() guards on done.) */
WiggleIterator *newWiggleIterator(void *data, void (*pop)(WiggleIterator *),
                                  void (*seek)(WiggleIterator *, const char *, int, int),
                                  double default_value, wt_bool overlapping);
void pop(WiggleIterator *);
void seek(WiggleIterator *, const char *, int, int);
void runWiggleIterator(WiggleIterator *);
void destroyWiggleIterator(WiggleIterator *);

/* Multiplexer -- replaces reference src/multiplexer.c:22-169. */
Multiplexer *newMultiplexer(WiggleIterator **iters, int count, wt_bool strict);
Multiplexer *newCoreMultiplexer(void *data, int count, void (*pop)(Multiplexer *),
                                void (*seek)(Multiplexer *, const char *, int, int));
void popMultiplexer(Multiplexer *);
void seekMultiplexer(Multiplexer *, const char *chrom, int start, int finish);
void runMultiplexer(Multiplexer *);

/* Multiset -- replaces reference src/multiSet.c:80-128. */
Multiset *newMultiset(Multiplexer **multis, int count);
void popMultiset(Multiset *);
void seekMultiset(Multiset *, const char *chrom, int start, int finish);

/* Reducers -- replace reference src/reducers.c (ctor lines in brackets). */
WiggleIterator *SumReduction(Multiplexer *);      /* reducers.c:294-307 */
WiggleIterator *ProductReduction(Multiplexer *);  /* reducers.c:348-361 */
WiggleIterator *MeanReduction(Multiplexer *);     /* reducers.c:404-422 */
WiggleIterator *VarianceReduction(Multiplexer *); /* reducers.c:481-505 */
WiggleIterator *StdDevReduction(Multiplexer *);   /* reducers.c:565-590 */
WiggleIterator *EntropyReduction(Multiplexer *);  /* reducers.c:640-666 */
WiggleIterator *CVReduction(Multiplexer *);       /* reducers.c:727-751 */
WiggleIterator *MedianReduction(Multiplexer *);   /* reducers.c:815-834 */
WiggleIterator *MinReduction(Multiplexer *);      /* reducers.c:237-253 */
WiggleIterator *MaxReduction(Multiplexer *);      /* reducers.c:170-186 */
WiggleIterator *SelectReduction(Multiplexer *, int);      /* reducers.c:67-72, host */
WiggleIterator *FillInReduction(Multiplexer *, wt_bool);  /* reducers.c:108-119, host */

/* Two-sample tests -- replace reference src/setComparisons.c. */
WiggleIterator *TTestReduction(Multiset *);  /* setComparisons.c:123-131 */
WiggleIterator *MWUReduction(Multiset *);    /* setComparisons.c:372-390 */
/* setComparisons.c:232-243.  The reference's F-test pop is broken (its inner loops advance
 * `index` instead of `index2`, :183,199 -- undefined behaviour) and is out of scope:
 * exported so that the link change of INTEGRATION.md links (commandParser.c:642-644 calls it);
 * prints a message and exit(1)s, the reference's own error convention. */
WiggleIterator *FTestReduction(Multiset *);

/* Behavioural difference at this boundary (documented, loud): the reference accepts any C `int`
 * coordinate; this engine refuses run finishes above WTAMD_MAX_COORD = 2^31 - 65537 (message +
 * exit(1) from the drop-in layer, WTAMD_ERR_ARG from the bulk layer) because its 32-bit window
 * arithmetic keeps a margin below INT32_MAX.  No genome assembly comes near it. */

/* ------------------------------------------------------------------ */
/* (2) BULK LAYER                                                      */
/* ------------------------------------------------------------------ */

/* Reducer selector.  One code per reference ...ReductionPop. */
enum wtamd_op {
    WTAMD_OP_SUM = 0,      /* SumReductionPop       reducers.c:259-292 */
    WTAMD_OP_PRODUCT = 1,  /* ProductReductionPop   reducers.c:313-346 */
    WTAMD_OP_MEAN = 2,     /* MeanReductionPop      reducers.c:367-402 */
    WTAMD_OP_VAR = 3,      /* VarianceReductionPop  reducers.c:428-479 */
    WTAMD_OP_STDDEV = 4,   /* StdDevReductionPop    reducers.c:511-563 */
    WTAMD_OP_ENTROPY = 5,  /* == STDDEV pop (reducers.c:665 installs StdDevReductionPop) */
    WTAMD_OP_CV = 6,       /* CVReductionPop        reducers.c:672-725 */
    WTAMD_OP_MIN = 7,      /* MinReductionPop       reducers.c:192-235 */
    WTAMD_OP_MAX = 8,      /* MaxReductionPop       reducers.c:125-168 */
    WTAMD_OP_MEDIAN = 9,   /* MedianReductionPop    reducers.c:780-813 */
    WTAMD_OP_TTEST = 10,   /* TTestReductionPop     setComparisons.c:35-121 */
    WTAMD_OP_MWU = 11,     /* MWUReductionPop       setComparisons.c:269-370 */
    WTAMD_OP_COUNT_ = 12
};

/* Flags for wtamd_reduce_desc.flags */
#define WTAMD_STRICT_SET0 1u   /* Multiplexer `strict` (set 0, or the only set) */
#define WTAMD_STRICT_SET1 2u   /* `strict` of the second Multiplexer (two-sample ops) */

/* Status codes (every wtamd_* function returning int). */
#define WTAMD_OK 0
#define WTAMD_ERR_ARG 1        /* bad argument                         */
#define WTAMD_ERR_HIP 2        /* HIP runtime error (see wtamd_last_error) */
#define WTAMD_ERR_CAPACITY 3   /* output buffers too small             */
#define WTAMD_ERR_NODEVICE 4   /* no gfx950 device visible             */
#define WTAMD_ERR_INTERNAL 5   /* kernel reported an internal fault    */

typedef struct wtamd_trackset wtamd_trackset; /* opaque: N tracks resident in HBM */

/*
 * Track storage ("run lists"): for chromosome c (0..n_chrom-1, already in
 * strcmp order, cf. reference multiplexer.c:56) and track i (0..n_tracks-1)
 * the intervals of that track on that chromosome are the slice
 *     [seg_off[c*n_tracks+i], seg_off[c*n_tracks+i+1])
 * of the three parallel arrays start[] (1-based inclusive), finish[]
 * (exclusive) and value[].  Within a slice intervals are sorted and
 * non-overlapping (the Multiplexer's precondition, multiplexer.c:163).
 * value[] is float32 (BigWig payload type) or float64.
 */
typedef struct {
    int32_t n_chrom;
    int32_t n_tracks;
    const int64_t *seg_off;   /* HOST pointer, n_chrom*n_tracks+1 entries */
    const int32_t *start;     /* host or device, see create function */
    const int32_t *finish;
    const void *value;        /* float* or double* */
    int32_t value_is_f64;     /* 0: float32, 1: float64 */
    const double *defaults;   /* HOST pointer, n_tracks default_values */
    /* Optional (NULL = whole chromosome): per chromosome, only runs whose START lies in
     * [range_lo[c], range_hi[c]) are produced.  This is how one chromosome is cut into
     * batches (drop-in layer) or shards (multi-GPU): a run spanning a cut belongs to the
     * piece that holds its start and keeps its true finish, so pieces concatenate to the
     * unsharded output.  INT32_MAX as range_hi = "to the end".  HOST pointers, n_chrom entries. */
    const int32_t *range_lo;
    const int32_t *range_hi;
} wtamd_tracks;

typedef struct {
    int32_t op;        /* enum wtamd_op */
    uint32_t flags;    /* WTAMD_STRICT_* */
    int32_t n_set0;    /* two-sample ops: tracks [0,n_set0) = set 0, rest = set 1; else 0 */
    int32_t reserved;
} wtamd_reduce_desc;

/* Output of one reduction: R runs in (chrom, start) order. All DEVICE pointers
 * unless the _host entry point is used. */
typedef struct {
    int64_t capacity;        /* in: entries available in the arrays below */
    int32_t *start;          /* out: run start  (1-based inclusive)  */
    int32_t *finish;         /* out: run finish (exclusive)          */
    double *value;           /* out: reducer value                   */
    int64_t *chrom_run_off;  /* out: n_chrom+1 entries, runs of chrom c = [off[c],off[c+1]) */
} wtamd_runs;

/* Aggregate statistics of the last reduce on a trackset (for metrics). */
typedef struct {
    int64_t n_runs;          /* emitted runs                                   */
    int64_t covered_bp;      /* sum(finish-start) of emitted runs              */
    int64_t n_intervals;     /* input intervals examined                       */
    int64_t n_windows;       /* alignment windows processed                    */
    int32_t window_bp;       /* window width used                              */
    int32_t lds_bytes;       /* LDS per workgroup                              */
    float index_ms;          /* last window-index kernel time (HIP events)     */
    float reduce_ms;         /* last multiplex+reduce kernel time (HIP events) */
    int32_t kernel;          /* kernel of the last reduction: 0 general bitmap multiplexer (wt_reduce_kernel),
                                1 exact difference array for Sum / Mean (wt_delta_kernel),
                                2 median by walking (wt_walk_kernel)                                  */
    int32_t patched_windows; /* difference-array windows whose values the general kernel rewrote (NaN, Inf, wide range) */
} wtamd_stats;

int wtamd_device_count(void);
int wtamd_set_device(int ordinal);
int wtamd_current_device(void);     /* the calling thread's device (-1: none); HIP devices are per thread */
/* Starts the HIP runtime (device discovery, code object, first hardware queues: ~0.2 s in a fresh process) on a helper thread,
 * once per process; returns at once.  wtamd_BigWiggleReaders calls it before it opens its files; the first pipe waits for it. */
void wtamd_warmup_async(void);
const char *wtamd_last_error(void);
const char *wtamd_version(void);

/* Largest run finish a track set may hold (the 32-bit window arithmetic keeps a margin below
 * INT32_MAX; creation fails with WTAMD_ERR_ARG above it).  The reference's coordinates are C `int`
 * as well (wiggleIterator.h:23-24). */
#define WTAMD_MAX_COORD (2147483647 - 65536)

/* Copies the SoA arrays from HOST memory into HBM. */
int wtamd_trackset_create_host(const wtamd_tracks *tracks, wtamd_trackset **out);
/* Zero-copy: start/finish/value are DEVICE pointers owned by the caller and
 * must stay valid until wtamd_trackset_destroy. */
int wtamd_trackset_create_device(const wtamd_tracks *tracks, wtamd_trackset **out);
void wtamd_trackset_destroy(wtamd_trackset *);

/* Input contract check, on device: inside every (chrom, track) segment the runs must be sorted,
 * non-overlapping and of positive length (finish > start).  Anything else is undefined behaviour
 * here as it is in the reference's Multiplexer (multiplexer.c:76-96; its text readers check it,
 * bedReader.c:46-49).  *n_bad = number of offending runs, *first_bad (optional) = global index of
 * the first one or -1.  Not called implicitly: one pass over start[] / finish[]. */
int wtamd_trackset_validate(wtamd_trackset *ts, int64_t *n_bad, int64_t *first_bad);

/* Upper bound on the number of runs any reduction over `ts` can emit. */
int64_t wtamd_trackset_max_runs(const wtamd_trackset *ts);

/* Build (or rebuild) the window index `op` (enum wtamd_op) would use, on `stream`
 * (hipStream_t as void*).  wtamd_reduce() calls this itself when the index is
 * missing; it is exposed so callers can time / amortise it separately, and it is what a caller of
 * a zero-copy track set must call after rewriting the run lists in place (same segment sizes):
 * it also voids what earlier reductions learnt about the values -- the next Sum / Mean verifies
 * again that its exact difference-array kernel applies and therefore waits for its launch. */
int wtamd_trackset_index(wtamd_trackset *ts, int op, void *stream);

/* Multiplex + reduce, everything on device. `runs` arrays are DEVICE memory.
 * *n_runs is written on the host after the stream has been synchronised iff
 * n_runs != NULL (otherwise the call is fully asynchronous and the count can be
 * read from chrom_run_off[n_chrom]). */
int wtamd_reduce(wtamd_trackset *ts, const wtamd_reduce_desc *desc, wtamd_runs *runs,
                 int64_t *n_runs, void *stream);

/* Convenience: same, but `runs` arrays are HOST memory (internally staged). */
int wtamd_reduce_host(wtamd_trackset *ts, const wtamd_reduce_desc *desc, wtamd_runs *runs,
                      int64_t *n_runs);

/* Multiplexer "materialise": emits the aligned tile the reference exposes per
 * popMultiplexer (multiplexer.h:21-36): for each run r, values[r*n_tracks+i]
 * and inplay[r*n_tracks+i]; runs->value[r] receives the run's inplay_count.  HOST output.
 * Used by the drop-in layer when a Multiplexer* escapes to code that reads its fields. */
int wtamd_multiplex_host(wtamd_trackset *ts, uint32_t flags, wtamd_runs *runs,
                         double *values, uint8_t *inplay, int64_t *n_runs);

/* Genome-wide scalar over the output of a reduction, computed on device:
 * AUC = sum over runs of (finish-start)*value skipping NaN
 * (reference statistics.c:103-120).  Result written to *auc (host). */
int wtamd_runs_auc(const wtamd_runs *runs, int64_t n_runs, double *auc, void *stream);
/* meanI: sum of (finish-start)*value over the non-NaN runs divided by their span; NaN when that
 * span is 0 (reference MeanIntegrator, statistics.c:62-100; its NonOverlapping wrapper is the
 * identity on reducer output, which never overlaps). */
int wtamd_runs_mean(const wtamd_runs *runs, int64_t n_runs, double *mean, void *stream);

/* Pearson correlation of the two tracks of `ts` over their Multiplexer tile, on device
 * (reference PearsonIntegrator over a 2-track Multiplexer: statistics.c:414-465,
 * commandParser.c:683-694).  Non-strict Multiplexer, absent tracks read as their defaults.
 * NaN when T_XX*T_YY == 0 (statistics.c:421-423).  Slices of runs are merged with the reference's
 * own update formula, so the result agrees to rounding (not bit-for-bit). */
int wtamd_pearson(wtamd_trackset *ts, double *result);
/* The same as six moments {n, sum_X, sum_Y, T_XX, T_XY, T_YY} of this track set's part of the genome,
 * so that shards (chromosomes on different GPUs) can be combined: gather the 6 doubles per shard
 * (RCCL all_gather), then merge IN GENOME ORDER with wtamd_pearson_merge -- the reference's update is
 * sequential (statistics.c:442-456), a pairwise merge agrees to rounding -- and finish. */
int wtamd_pearson_moments(wtamd_trackset *ts, double *moments6);
void wtamd_pearson_merge(double *a6, const double *b6);     /* a := a (+) b, b after a in genome order; HOST */
double wtamd_pearson_finish(const double *m6);               /* T_XY / sqrt(T_XX T_YY), NaN if 0 (statistics.c:421-423) */

/* The reference's other genome-wide statistics over a device run list -- varI / stddevI / CVI, maxI / minI and the
 * span (statistics.c:129-326) -- from ONE pass:
 *     moments6 = { sum of L v, span = sum of L, T = sum of L (v - sum / span)^2, min, max, 0 },  L = finish - start,
 * over the runs whose value is not NaN (min and max are NaN when there is none).  T is the reference's
 * VarianceData.T (:232-252): it updates T run by run, here lanes' partial {span, sum, T} are merged pairwise in a
 * fixed order, so T and sum agree to rounding (the same run list always gives the same bits); span is exact,
 * min / max bit for bit (the earlier run wins between -0.0 and 0.0, as in the reference). */
int wtamd_runs_moments(const wtamd_runs *runs, int64_t n_runs, double *moments6, void *stream);
/* a := a (+) b, b after a in genome order (chromosomes on different GPUs, batches of a pipeline); HOST */
void wtamd_moments_merge(double *a6, const double *b6);
/* The reference's closing arithmetic in its own order (statistics.c:259,288-289,312-314): whatever that gives for
 * an empty or one-base-pair input (-0.0, NaN, inf) is what comes back; HOST */
#define WTAMD_STAT_VAR 0    /* T / (span - 1) */
#define WTAMD_STAT_STDDEV 1 /* sqrt of that */
#define WTAMD_STAT_CV 2     /* that / (sum / span) */
#define WTAMD_STAT_MAX 3
#define WTAMD_STAT_MIN 4
#define WTAMD_STAT_SPAN 5
double wtamd_moments_finish(const double *m6, int kind);

/* The reference's `map`-able unary operators (src/unaryOps.c: scale :650-664, offset :722-734,
 * ln / log :760-813, exp :823-866, pow :873-899, abs :934-949; commandParser.c:115-211) applied to
 * whole run lists on device before they are multiplexed. */
enum wtamd_map_op {
    WTAMD_MAP_SCALE = 0,    /* param * value                                   */
    WTAMD_MAP_OFFSET = 1,   /* param + value                                   */
    WTAMD_MAP_LN = 2,       /* log(value); runs with value <= 0 are DROPPED    */
    WTAMD_MAP_LOG = 3,      /* log(value) / log(param); same                   */
    WTAMD_MAP_EXP = 4,      /* exp(value)                                      */
    WTAMD_MAP_EXPB = 5,     /* exp(value * log(param))                         */
    WTAMD_MAP_POW = 6,      /* pow(value, param); NaN if param < 0 && value <= 0 */
    WTAMD_MAP_ABS = 7,
    WTAMD_MAP_GT = 8,       /* runs with value > param, value 1; the others and NaN runs are DROPPED */
    WTAMD_MAP_GTE = 9,      /*   (HighPassFilterWiggleIterator, unaryOps.c:386-419; default 0)      */
    WTAMD_MAP_LT = 10,      /* value < param (the reference builds it as scale -1, gt -param)       */
    WTAMD_MAP_LTE = 11,
    WTAMD_MAP_COUNT_
};
/* start / finish / value and the o_* arrays are DEVICE memory (o_* sized for all input runs),
 * seg_off / o_seg_off HOST arrays of n_seg + 1 offsets (n_seg = n_chrom * n_tracks).  Output
 * values are f64.  For the operators that drop nothing o_start / o_finish may be NULL or alias
 * the inputs.  Synchronous on `stream`. */
int wtamd_runs_map(int map_op, double param, int64_t n_seg, const int64_t *seg_off, const int32_t *start,
                   const int32_t *finish, const void *value, int value_is_f64, int32_t *o_start, int32_t *o_finish,
                   double *o_value, int64_t *o_seg_off, void *stream);
/* default_value of the operator iterator the reference would build around a track whose default is
 * `default_value`, including the `float` truncation several constructors apply. */
double wtamd_map_default(int map_op, double param, double default_value);

/* The same operators INSIDE the streaming pipeline: one chain of up to WTAMD_MAP_CHAIN_MAX operators per
 * track (applied first to last), run on device on every batch between its arrival in HBM and the
 * Multiplexer -- `sum map ln a.bw b.bw` (README idiom; commandParser.c:115-211) without N host operator
 * iterators in front of the engine.  The pipe's default values must already be the mapped ones
 * (wtamd_map_default).  chains == NULL switches it off.  Mapped batches are f64. */
#define WTAMD_MAP_CHAIN_MAX 4
typedef struct wtamd_map_chain {
    int32_t n_ops;
    int32_t op[WTAMD_MAP_CHAIN_MAX];
    double param[WTAMD_MAP_CHAIN_MAX];
} wtamd_map_chain;
struct wtamd_pipe;
int wtamd_pipe_set_map(struct wtamd_pipe *p, const wtamd_map_chain *chains /* n_tracks entries */);
/* Drop-in side: the operator iterator the reference's parser builds around a track (ScaleWiggleIterator,
 * NaturalLogWiggleIterator, ... unaryOps.c:650-949, HighPassFilterWiggleIterator :386-419) as ONE
 * constructor.  Handed to newMultiplexer / newMultiset of this library it is unwrapped: the child is
 * drained raw (in blocks when it is bulk-capable) and the chain runs on device (wtamd_pipe_set_map);
 * popped by anything else it follows the reference's per-interval protocol on the host.
 * default_value = wtamd_map_default(op, param, child's).  Unknown operator or a chain deeper than
 * WTAMD_MAP_CHAIN_MAX: message and exit(1). */
WiggleIterator *wtamd_MapIterator(WiggleIterator *child, int map_op, double param);

/* Coverage and union of OVERLAPPING intervals on device (csrc/wt_cover.hip): what turns reads and regions (BED, BAM,
 * bigBed: the reference's readers with `overlaps = true`) into the non-overlapping tracks everything else here consumes.
 * Input in the layout of wtamd_runs_map: start / finish (and value, f32 or f64) are DEVICE arrays, seg_off / o_seg_off HOST
 * arrays of n_seg + 1 offsets; inside a segment the intervals are sorted by start (finishes in any order) and
 * start < finish -- anything else: WTAMD_ERR_ARG, nothing written (wtamd_runs_coverage_flags takes a segment's intervals in any
 * order).  The o_* arrays are DEVICE memory of `capacity` runs;
 * when the result does not fit: WTAMD_ERR_CAPACITY with *n_out = the count needed.  Synchronous on `stream`.
 *
 * wtamd_runs_coverage -- the reference's CoverageWiggleIterator (src/unaryOps.c:303-375, the `coverage` command): per
 * segment, with B the sorted distinct starts and finishes, one run [B[k], B[k+1]) of value #(start <= B[k]) -
 * #(finish <= B[k]) wherever that is > 0.  Runs are not merged where the depth stays the same (touching intervals give two
 * runs of equal value), input values are ignored, depth 0 emits nothing; at most 2n - 1 runs from n intervals; values are
 * exact integers in f64.  ONE DEVIATION: when its child runs dry the reference reads the exhausted child's stale start
 * (:333-334) and emits one run with start == finish per stream; this library does not emit it.  Scratch: 12 bytes per 64 bp
 * of a segment's extent plus 16 bytes per interval, in passes of at most WTAMD_COVER_SCRATCH_MB (default 256) MiB of the
 * former; a larger segment is cut at positions.
 *
 * wtamd_runs_union -- the reference's UnionWiggleIterator (:60-92, what NonOverlappingWiggleIterator puts in front of every
 * Multiplexer child): an interval joins the current group while group.finish > start (touching intervals do not merge); the
 * group has the first member's start and value (carried bit for bit, widened to f64) and the largest finish; at most n runs. */
int wtamd_runs_coverage(int64_t n_seg, const int64_t *seg_off, const int32_t *start, const int32_t *finish,
                        int64_t capacity, int32_t *o_start, int32_t *o_finish, double *o_value,
                        int64_t *o_seg_off, int64_t *n_out, void *stream);
/* wtamd_runs_coverage with flags; flags 0 is wtamd_runs_coverage itself, results and errors alike.  A bit that is not listed
 * here: WTAMD_ERR_ARG.
 *   WTAMD_COVER_ANY_ORDER   the intervals of a segment may come in any order (the covering components of spliced reads in file
 *                           order: after 50M1000N50M at 100 the next read's start at 120 follows an interval that starts at
 *                           1150).  start >= finish is still refused.  The result is the coverage of the same intervals sorted
 *                           by start, byte for byte, whole segments and segments cut at positions alike: a segment's extent is
 *                           the integer minimum of its starts and maximum of its finishes, and every pass places an interval by
 *                           its own start and finish alone.  Same scratch, same passes, no sort. */
#define WTAMD_COVER_ANY_ORDER 1u
int wtamd_runs_coverage_flags(int64_t n_seg, const int64_t *seg_off, const int32_t *start, const int32_t *finish,
                              int64_t capacity, int32_t *o_start, int32_t *o_finish, double *o_value,
                              int64_t *o_seg_off, int64_t *n_out, uint32_t flags, void *stream);
int wtamd_runs_union(int64_t n_seg, const int64_t *seg_off, const int32_t *start, const int32_t *finish,
                     const void *value, int value_is_f64, int64_t capacity,
                     int32_t *o_start, int32_t *o_finish, double *o_value,
                     int64_t *o_seg_off, int64_t *n_out, void *stream);
/* wtamd_runs_coverage of ONE segment held in HOST arrays, result in HOST arrays (what wtamd_CoverageIterator calls per
 * chromosome): device memory, copies and the call on the null stream. */
int wtamd_runs_coverage_host(int64_t n, const int32_t *start, const int32_t *finish, int64_t capacity, int32_t *o_start,
                             int32_t *o_finish, double *o_value, int64_t *n_out);
/* The same over wtamd_runs_coverage_flags. */
int wtamd_runs_coverage_host_flags(int64_t n, const int32_t *start, const int32_t *finish, int64_t capacity, int32_t *o_start,
                                   int32_t *o_finish, double *o_value, int64_t *n_out, uint32_t flags);

/* Region operators on device (csrc/wt_region.hip): the reference's OverlapWiggleIterator, NoverlapWiggleIterator,
 * TrimWiggleIterator and NearestWiggleIterator (src/unaryOps.c:437-639; the parser's `overlaps`, `noverlaps`, `trim`,
 * `nearest`, commandParser.c:813-819) over whole run lists: a source restricted to, or measured against, a mask.  Source and
 * mask come in the layout of wtamd_runs_map with the SAME n_seg, segment g of one pairing with segment g of the other:
 * start / finish (and the source's value, f32 or f64) are DEVICE arrays, the seg_off arrays HOST arrays of n_seg + 1
 * offsets; inside a segment both are sorted by start with start < finish, and either may overlap itself, except the source
 * of a trim.  Per segment, with S the source, M the mask, G = the union of M as wtamd_runs_union defines it (touching
 * intervals stay apart), lo(i) = the first group with G.finish > S.start[i], hi(i) = the first group with
 * G.start >= S.finish[i]:
 *   OVERLAPS    run i iff hi(i) > lo(i); start, finish and value carried unchanged
 *   NOVERLAPS   run i iff hi(i) <= lo(i) (every run where the mask is empty)
 *   TRIM        for g in [lo(i), hi(i)), in that order: [max(S.start, G.start[g]), min(S.finish, G.finish[g])) with the
 *               value of run i; at most n + |G| - 1 runs per segment; two touching mask intervals cut a run in two
 *   NEAREST     exactly the source's runs; with k = #(M.start <= S.start[i]) over the RAW mask the value is the smaller of
 *               S.start[i] - M.finish[k-1] + 1 (if k > 0) and M.start[k] - S.finish[i] + 1 (if k < m), in int32
 *               arithmetic, 0 where that is negative, NaN where there is no candidate.  The reference's quirks are kept:
 *               the + 1; the "previous" mask is the one that started last, not the one that ends last; an earlier mask
 *               that encloses the run is not seen.
 * Values are carried bit for bit and widened to f64.  WTAMD_ERR_ARG with nothing written: an unknown op, a segment that is
 * not sorted by start or holds start >= finish (either side), a TRIM source with start[i] < finish[i-1] (the reference's
 * output then depends on the order of its pops and loses intersections; wtamd_RegionIterator serves that case by the
 * reference's protocol on the host).  The o_* arrays are DEVICE memory of `capacity` runs, o_seg_off a HOST array; when the
 * result does not fit: WTAMD_ERR_CAPACITY with *n_out = the count needed, nothing written.  Synchronous on `stream`.
 * Scratch: 8 bytes per mask interval (the union), 8 bytes per 1024 source runs. */
enum wtamd_region_op { WTAMD_REGION_OVERLAPS = 0, WTAMD_REGION_NOVERLAPS = 1, WTAMD_REGION_TRIM = 2, WTAMD_REGION_NEAREST = 3 };
int wtamd_runs_region(int op, int64_t n_seg,
                      const int64_t *seg_off, const int32_t *start, const int32_t *finish, const void *value, int value_is_f64,
                      const int64_t *m_seg_off, const int32_t *m_start, const int32_t *m_finish,
                      int64_t capacity, int32_t *o_start, int32_t *o_finish, double *o_value,
                      int64_t *o_seg_off, int64_t *n_out, void *stream);
/* wtamd_runs_region of ONE segment pair held in HOST arrays, result in HOST arrays (what wtamd_RegionIterator calls per
 * chromosome): device memory, copies and the call on the null stream. */
int wtamd_runs_region_host(int op, int64_t n, const int32_t *start, const int32_t *finish, const double *value,
                           int64_t m, const int32_t *m_start, const int32_t *m_finish,
                           int64_t capacity, int32_t *o_start, int32_t *o_finish, double *o_value, int64_t *n_out);

/* Per-region statistics on device (csrc/wt_apply.hip): what the reference's ApplyMultiplexer (src/apply.c; the parser's
 * `apply` / `apply_paste`, commandParser.c:266-320, 917-936) computes -- AUC meanI varI stddevI CVI maxI minI of a dataset
 * inside every region -- as six moments per region.  Dataset and regions come in the layout of wtamd_runs_map with the SAME
 * n_seg, segment g of one pairing with segment g of the other: start / finish (and the dataset's value, f32 or f64) are DEVICE
 * arrays, the seg_off arrays HOST arrays of n_seg + 1 offsets.  The dataset is sorted, start < finish and DISJOINT
 * (start[i] >= finish[i-1]: the Multiplexer's own precondition); the regions are sorted by start with start < finish and may
 * overlap, nest or repeat -- each is evaluated on its own, as the reference does.  Anything else: WTAMD_ERR_ARG, nothing
 * written.  Fewer than 2^31 dataset runs per call.
 * For region [rs, rf): lo = the first run of its segment with finish > rs, hi = the first with start >= rf; the pieces are
 * [max(s, rs), min(f, rf)) of the runs in [lo, hi).  With L the piece lengths and v the values widened to f64,
 *     moments6 = { sum of L v, span = sum of L, T = sum of L (v - sum / span)^2, min, max, covered },
 * the first five over the pieces whose value is not NaN, exactly as wtamd_runs_moments defines them (min / max NaN when there
 * is none), covered = sum of L over ALL pieces, NaN-valued ones included.
 *   WTAMD_APPLY_STRICT (`apply` without `fillIn`, the parser's default): exactly the above.
 *   without it (`fillIn`): the (rf - rs) - covered uncovered base pairs also enter with value default_value, unless that is
 *   NaN, as one partial {sum U d, span U, T 0, min d, max d} merged after the data; covered stays the data's.
 * span, covered, min and max are exact; sum and T agree with exact arithmetic to rounding (pivoted sums merged pairwise in a
 * fixed order: the same input always gives the same bits), and a region's six doubles depend on that region, its dataset
 * segment, default_value and flags alone -- not on the other regions of the call.  moments6 is DEVICE memory, 6 doubles per
 * region in region order.  Synchronous on `stream`; temporary memory comes from the device pool.
 * Scratch: 16 bytes per region + 64 bytes per chunk + 8 bytes per 1024 regions + device copies of the two seg_off arrays; a
 * region with more than 32 runs under it is cut into chunks of 2048 runs.  No start may be negative (WTAMD_ERR_ARG).
 * Departures from the reference:
 *   - NaN runs are skipped for varI / stddevI / CVI as for the others (the reference's VarianceCorePop never terminates on
 *     one): the library's existing departure.
 *   - The reference truncates the dataset's default to `float` on its buffered path (apply.c:42) but not on its long-region
 *     path; here the double given is used.
 *   - For regions of 10^6 bp and more (apply.c:197) the reference feeds the statistics whatever the dataset's own seek
 *     delivers; here the runs are always clipped to the region.
 *   - The reference buffers regions in groups and seeks the dataset to the finish of the LAST region of a group (apply.c:311):
 *     with a reader that clips at the seek's finish, a region that reaches past it (one nested inside it follows) loses the
 *     data beyond.  Here every region sees its dataset whole.
 *   - A min / max tie between the default and a data value that compare equal (+-0) goes to the data. */
#define WTAMD_APPLY_STRICT 1u
int wtamd_runs_apply(int64_t n_seg,
                     const int64_t *seg_off, const int32_t *start, const int32_t *finish, const void *value, int value_is_f64,
                     const int64_t *r_seg_off, const int32_t *r_start, const int32_t *r_finish,
                     double default_value, uint32_t flags, double *moments6, void *stream);
/* wtamd_runs_apply of ONE segment pair held in HOST arrays, 6 doubles per region into a HOST array: device memory, copies
 * and the call on the null stream. */
int wtamd_runs_apply_host(int64_t n, const int32_t *start, const int32_t *finish, const double *value,
                          int64_t n_regions, const int32_t *r_start, const int32_t *r_finish,
                          double default_value, uint32_t flags, double *moments6);
/* The reference's closing arithmetic over one region's six moments; HOST.  AUC is m6[0]; meanI is m6[0] / m6[1], NaN when the
 * span is 0 (statistics.c:66-67); the rest go through wtamd_moments_finish (statistics.c:259,288-289,312-314: whatever that
 * order gives for an empty or one-base-pair region).  NaN for an unknown statistic. */
enum wtamd_apply_stat { WTAMD_APPLY_AUC = 0, WTAMD_APPLY_MEAN = 1, WTAMD_APPLY_VAR = 2, WTAMD_APPLY_STDDEV = 3, WTAMD_APPLY_CV = 4,
                        WTAMD_APPLY_MAX = 5, WTAMD_APPLY_MIN = 6 };
double wtamd_apply_finish(const double *m6, int stat);

/* Region profiles on device (csrc/wt_profile.hip): what the reference's ProfileMultiplexer (src/apply.c:355-366; the parser's
 * `profile` / `profiles`, commandParser.c:862-905) computes through regionProfile (src/plots.c:27-64) -- the dataset under
 * every region squeezed or stretched onto `width` bins.  Dataset and regions exactly as for wtamd_runs_apply (same layout, the
 * SAME n_seg, dataset sorted, start < finish and DISJOINT, regions sorted by start and free to overlap, nest or repeat, no
 * negative start, fewer than 2^31 runs) and width >= 1; anything else, or an unknown flag bit: WTAMD_ERR_ARG, nothing written.
 * The rule, never strict.  Region [rs, rf), L = rf - rs, W = width, c = W / (double) L, positions relative to rs.  The
 * reference serves one run [i, i + 1) with the dataset's value for every covered position i, and ONE run [a, b) with
 * default_value for every maximal uncovered stretch (before the first run and after the last included).  A run [a, b) with
 * value v: a NaN v is skipped; start = round(a c), finish = round(b c) (C's round on the double product); finish <= start
 * becomes start + 1, finish > W becomes W; every bin of [start, finish) gets v / (finish - start).
 * Consequences (the reference's, reproduced):
 *   - c <= 1: every covered position lands in the one bin round(i c) with its full value; bins are centred, so bin 0 collects
 *     about half as many positions as the others, and with L >= 2 W the last positions have round(i c) == W and are dropped
 *     (L = 20, W = 4, value 1 everywhere: 3 5 5 5).
 *   - c > 1: every bin has exactly one contributor and holds v / n, bit for bit.
 *   - An uncovered stretch counts as ONE sample of the default, spread over its bins, however long it is (L = 20, W = 4, runs
 *     [2,5) = 2 and [10,18) = 1, default 0.5: 2.5 4.5 3 5 -- the trailing stretch [18,20) starts at bin 4 and vanishes).
 * profile is DEVICE memory: width doubles per region, row-major in region order -- or, with WTAMD_PROFILE_SUM (`profile`),
 * width doubles: the column sums of all rows of all segments, merged pairwise, the lower region first, in ONE tree over the
 * region index whatever the batch.  A bin's terms are added in position order (a bin with more than 32 runs under it: 64
 * contiguous shares merged pairwise): the same input always gives the same bits, and a region's row depends on that region,
 * its dataset segment, default_value and width alone.  Synchronous on `stream`; temporary memory from the device pool.
 * Regions are processed in batches (a power of two of regions, at most 2^22 bins, at least one region; WTAMD_PROFILE_BATCH=<n>
 * sets the regions per batch).  Scratch: 16 bytes per region + 40 bytes per 256 bins of a batch + device copies of the two
 * seg_off arrays; with WTAMD_PROFILE_SUM also 8 bytes x (bins of a batch + width x (2 + log2 of the number of batches)).
 * Departures from the reference, as for wtamd_runs_apply:
 *   - The reference truncates the dataset's default to `float` (apply.c:42); here the double given is used.
 *   - The reference seeks the dataset to the finish of the LAST region of a buffered group (apply.c:311), so a region reaching
 *     past a nested one loses data; here every region sees its dataset whole.
 *   - Regions of 10^6 bp and more (apply.c:197) take the reference's unbuffered path, which feeds regionProfile absolute
 *     coordinates; here the rule above holds at every length. */
#define WTAMD_PROFILE_SUM 1u
int wtamd_runs_profile(int64_t n_seg,
                       const int64_t *seg_off, const int32_t *start, const int32_t *finish, const void *value, int value_is_f64,
                       const int64_t *r_seg_off, const int32_t *r_start, const int32_t *r_finish,
                       int32_t width, double default_value, uint32_t flags, double *profile, void *stream);
/* wtamd_runs_profile of ONE segment pair held in HOST arrays, the rows (or their sum) into a HOST array: device memory, copies
 * and the call on the null stream. */
int wtamd_runs_profile_host(int64_t n, const int32_t *start, const int32_t *finish, const double *value,
                            int64_t n_regions, const int32_t *r_start, const int32_t *r_finish,
                            int32_t width, double default_value, uint32_t flags, double *profile);

/* The window operators on device (csrc/wt_window.hip): the reference's BinningWiggleIterator (src/unaryOps.c:963-1036; the
 * parser's `bin`) and SmoothWiggleIterator (:1039-1162; `smooth`) over whole run lists.  The layout of wtamd_runs_map: n_seg
 * segments, seg_off / o_seg_off HOST arrays of n_seg + 1 offsets, start / finish / value (f32 or f64) DEVICE arrays; outputs
 * o_start / o_finish / o_value (f64) DEVICE arrays of `capacity` entries, *n_out on the host.  Inside a segment the runs are
 * sorted, start < finish, DISJOINT (the reference puts its union in front of both operators) and start >= 1; fewer than 2^31 runs.
 * WTAMD_ERR_CAPACITY: *n_out holds the count needed, nothing written.  WTAMD_ERR_ARG, nothing written: width < 2, a segment
 * that breaks those rules, or an output coordinate that would pass INT32_MAX.
 * BIN, width w.  The grid bins of a segment are [1 + k w, 1 + (k + 1) w); a bin is emitted, in order, if and only if a run
 * intersects it (the reference's "continue at the last finish" and "realign" rules land on the same grid); adjacent bins are
 * not merged.  A bin's value starts at 0.0 and takes (double) (int) covered * value of every intersecting run in order; then,
 * if default_value is not zero -- NaN counts as not zero, the reference tests `if (iter->default_value && ...)` -- and the
 * covered length is below w, (w - covered) * default_value.  An all -0.0 bin gives +0.0.  The default of the result is
 * default_value * w.  The output count is at most the sum over the runs of the bins each touches.  A bin with more than 32
 * runs under it is summed as 64 contiguous shares merged pairwise, lower share first, the default's term last.
 * SMOOTH, width w, h = w / 2.  One run [p, p + 1) per position; every segment is ONE island.  With s the first start and F the
 * last finish: it starts at p0 = max(1, s - h), after a prefill that reads positions 1 .. h when s - h < 1; the value at p is
 * (sum of the buffer) / w, the buffer holding the last <= w positions read up to p + h.  A position inside the segment that no
 * run covers reads as 0, NOT as the default.  Nothing is read from position F on (even when it is asked for during the
 * prefill); from then on every pop drops exactly one value, the oldest, and the island ends when none is left -- so a
 * chromosome shorter than w shrinks from its first read position, not by the window formula.  A window holding a NaN gives NaN;
 * once the NaN has left, the sum is that of the remaining values (the NaN positions are counted apart from the sum).  Zero
 * sums are +0.0.  The default of the result is the child's.  The output count is at most (F - p0) + w per segment, 16 bytes
 * per position: [clip_lo, clip_hi) restricts the positions DELIVERED, in every segment (0, 0: no clip), and the bits of a
 * position do not depend on it.  The sum of a position is formed over a strip of 16 outputs aligned to p0: the first window
 * from the runs under it as len * value in run order, the following ones by adding the value that enters and subtracting the
 * one that leaves -- the reference's running sum carries its whole history instead, so values that are not exact sums differ
 * from it by rounding (within (m + 2) 2^-53 x the largest window sum of |values| / w, m <= runs under a window + 30).
 * The bits of either result depend only on the segment's runs, the width and the default.  Synchronous on `stream`; temporary
 * memory from the device pool: bin 8 bytes per run + 40 bytes per 256 output bins, smooth 96 bytes per segment. */
int wtamd_runs_bin(int64_t n_seg, const int64_t *seg_off, const int32_t *start, const int32_t *finish, const void *value, int value_is_f64,
                   int32_t width, double default_value,
                   int64_t capacity, int32_t *o_start, int32_t *o_finish, double *o_value, int64_t *o_seg_off, int64_t *n_out, void *stream);
int wtamd_runs_smooth(int64_t n_seg, const int64_t *seg_off, const int32_t *start, const int32_t *finish, const void *value, int value_is_f64,
                      int32_t width, int32_t clip_lo, int32_t clip_hi,
                      int64_t capacity, int32_t *o_start, int32_t *o_finish, double *o_value, int64_t *o_seg_off, int64_t *n_out, void *stream);
/* Either door over ONE segment held in HOST arrays, result in HOST arrays (what wtamd_BinIterator / wtamd_SmoothIterator call
 * per chromosome, smooth per clip slice): device memory, copies and the call on the null stream. */
int wtamd_runs_bin_host(int64_t n, const int32_t *start, const int32_t *finish, const double *value, int32_t width, double default_value,
                        int64_t capacity, int32_t *o_start, int32_t *o_finish, double *o_value, int64_t *n_out);
int wtamd_runs_smooth_host(int64_t n, const int32_t *start, const int32_t *finish, const double *value, int32_t width,
                           int32_t clip_lo, int32_t clip_hi,
                           int64_t capacity, int32_t *o_start, int32_t *o_finish, double *o_value, int64_t *n_out);

/* Value histograms on device (csrc/wt_hist.hip): the reference's histogram() (src/plots.c:77-223; the parser's `histogram`)
 * over whole run lists.  The layout of wtamd_runs_map: n_seg segments, seg_off a HOST array of n_seg + 1 offsets, start / finish
 * / value (f32 or f64) DEVICE arrays; seg_row a HOST array of n_seg entries, the histogram row (0 .. n_rows - 1) of every
 * segment, so chromosome-major and track-major lists both work; hist a DEVICE matrix of n_rows x width doubles, range2 two
 * doubles on the HOST.  The runs need be neither sorted nor disjoint (the reference histograms raw iterators and counts
 * overlapping intervals once each); the only rule per run is start < finish; fewer than 2^31 runs.
 * THE RULE.  lo and hi are the minimum and maximum of all non-NaN values of all rows.  A run with a NaN value is skipped.  A
 * run of value v and length L = finish - start adds L to column c of its row: c = 0 when lo == hi, otherwise
 * c = (int) ((v - lo) * width / (hi - lo)) computed in double in exactly that order -- subtract, multiply by (double) width, one
 * IEEE division --, and c == width becomes width - 1 (any quotient not below width lands there).  f32 values are widened
 * first, so the same values in either width give the same bits.  The counters are unsigned 64-bit integers in LDS and in global
 * memory, converted to double at the end (exact below 2^53): the result does not depend on the order of addition and is
 * bit-reproducible.  A zero extreme comes back as +0.0.  When no non-NaN value exists, range2 comes back NaN, NaN and hist all
 * zeros.
 * flags.  WTAMD_HIST_RANGE_GIVEN: range2 is INPUT (lo, hi) and is not written; the range pass still validates.
 * WTAMD_HIST_ACCUMULATE (needs RANGE_GIVEN): hist holds whole numbers below 2^53 from an earlier call over the same range; they
 * are read back into the integer counters and added to.  So batches, and chromosomes on different GPUs, compose exactly:
 * compute a range per part, take the min / max on the host, run every part with the range given, add the parts -- counts are
 * integers, so any split gives the bits of the single call.
 * WTAMD_ERR_ARG, NOTHING written to hist or range2: width < 1 or n_rows < 1 (or n_rows x width above 2^40); a seg_row outside
 * [0, n_rows); a run with start >= finish; an infinite value (the reference's cast is undefined there); an unknown flag bit;
 * ACCUMULATE without RANGE_GIVEN; with RANGE_GIVEN a NaN, infinite or inverted range or a non-NaN value outside it; with
 * ACCUMULATE a cell of hist that is not a whole number in [0, 2^53).
 * Departures from the reference, which streams with a provisional range and re-bins whenever a value leaves it:
 *  1. Its re-binning smears mass by linear interpolation (raiseMaxNRows, plots.c:137-146); here bins are exact over the final
 *     range.  Lengths 4, values 0, 1, 0.5, 2, 0.25, width 4: the reference gives 8 8 0 4, the exact answer, given here, is 8 4 4 4.
 *  2. Its lowering re-bin reads and writes one column past each row (lowerMinNRows, plots.c:108) and has no defined result.
 *  3. At width 1 it loses all earlier mass when the second distinct value is lower (plots.c:113-116); here width 1 gives the
 *     total span.
 *  4. It keeps the sign of the run that set a zero extreme; here a zero extreme is +0.0 (seen only in the printed centre of an
 *     all -0.0 input).
 * The two are equal, bit for bit, exactly when no value lies outside the interval spanned by the stream's first two distinct
 * non-NaN values and either width >= 2 or the second of them is higher (the stream runs row 0 first, in order).
 * Synchronous on `stream`; temporary memory from the device pool: 8 bytes per cell of hist, 16 bytes per 16384 runs (per stretch
 * of consecutive segments of one row), 32 bytes of scalars. */
#define WTAMD_HIST_RANGE_GIVEN 1u   /* range2 is INPUT: lo, hi */
#define WTAMD_HIST_ACCUMULATE  2u   /* hist already holds a histogram over the same range: add to it */
int wtamd_runs_histogram(int64_t n_seg, const int64_t *seg_off, const int32_t *seg_row, int32_t n_rows,
                         const int32_t *start, const int32_t *finish, const void *value, int value_is_f64,
                         int32_t width, uint32_t flags, double *range2, double *hist, void *stream);
/* The same over run lists and a matrix held in HOST arrays (what wtamd_histogram calls): device memory, copies and the call on
 * the null stream. */
int wtamd_runs_histogram_host(int64_t n_seg, const int64_t *seg_off, const int32_t *seg_row, int32_t n_rows,
                              const int32_t *start, const int32_t *finish, const double *value,
                              int32_t width, uint32_t flags, double *range2, double *hist);

/* Energy spectra on device (csrc/wt_energy.hip): the reference's EnergyIntegrator (src/statistics.c:345-391; the parser's
 * `energy (wavelength) (iterator)`) over whole run lists, for any number of wavelengths from ONE read of the list.  The layout
 * of wtamd_runs_histogram: n_seg segments, seg_off a HOST array of n_seg + 1 offsets, start / finish / value (f32 or f64) DEVICE
 * arrays; wavelength a HOST array of n_wavelengths entries; reim a HOST array of 2 n_wavelengths doubles (real0, im0, real1,
 * ...); the energy of a wavelength is real^2 + im^2 (wtamd_energy_finish).  seg_base: a HOST array of n_seg int64 offsets
 * added to a segment's coordinates, or NULL for the reference's rule from 0 -- a segment's base is the sum of the last
 * finishes of the non-empty segments before it; an empty segment adds nothing (its seg_base entry is not looked at).  end_base
 * (HOST, may be NULL): the base a following segment would get -- the base of the last non-empty segment plus its last finish;
 * without one, the last entry of seg_base, or 0 --, so batches, chromosomes served one at a time and shards on other GPUs
 * chain: partial sums add, and a split agrees with the single call to rounding, not bit for bit.
 * THE RULE.  Every position p = base + start .. base + finish - 1 of a run of value v adds v cos(-2 pi p / lam) to real and
 * v sin(-2 pi p / lam) to im; gaps add nothing.  A run's sum is taken in closed form: with a = base + start (int64),
 * L = finish - start, m = (2 a + L - 1) mod 2 lam (floor modulus) and q = L mod 2 lam, both exact integers,
 * D = sinpi(q / lam) / sin(pi / lam): real += v D cospi(m / lam), im -= v D sinpi(m / lam); for lam == 1, real += v L.  f32 values
 * are widened first, so the same values in either width give the same bits.  Against the exact value of the rule, real and
 * im each lie within 2^-53 (48 + n) S, n the runs of the call and S = sum |v| L (DESIGN.md counts it).
 * FIXED ORDER.  A lane adds its runs in index order, a workgroup merges its lanes in a fixed tree, a final pass merges the
 * workgroups' partials in a fixed order; no floating-point atomics: the same list gives the same bits on every call.
 * WTAMD_ERR_ARG, NOTHING written to reim or end_base: n_wavelengths < 1 or above 1024 (WEN_MAX_WAVELENGTHS); a wavelength
 * < 1; a run with start >= finish; a segment that is not sorted and disjoint (start[i] < finish[i - 1]: put wtamd_runs_union in
 * front, as the reference does); a segment with runs whose |base| exceeds 2^62 - 2^31 (base + coordinate outside +-2^62).
 * DEPARTURES from the reference.  1. Positions are exact: no position goes through a double or an int product, so the result
 * is defined beyond position 2^30 (where the reference's `-position * 2` overflows) and offsets are 64-bit (its int
 * chrom_offset overflows on a human genome).  2. The values are correctly reduced closed forms, not running sums of libm calls
 * on large arguments: agreement with the reference is to its own error bound, 2^-53 S (16 P / lam + B + 8) for largest
 * position P and B base pairs, not bit for bit.  3. A NaN OR INFINITE value makes every real and im NaN (the reference can
 * return +-inf for an infinity).
 * Synchronous on `stream`; temporary memory from the device pool: 16 n_wavelengths bytes per 16384 runs, 48 n_wavelengths + 16
 * bytes of table, outputs and scalars, 20 bytes per segment. */
int wtamd_runs_energy(int64_t n_seg, const int64_t *seg_off, const int64_t *seg_base,
                      const int32_t *start, const int32_t *finish, const void *value, int value_is_f64,
                      int32_t n_wavelengths, const int32_t *wavelength, double *reim, int64_t *end_base, void *stream);
/* The same over run lists held in HOST arrays (what wtamd_EnergyIntegrator calls): device memory, copies and the call on the
 * null stream. */
int wtamd_runs_energy_host(int64_t n_seg, const int64_t *seg_off, const int64_t *seg_base,
                           const int32_t *start, const int32_t *finish, const double *value,
                           int32_t n_wavelengths, const int32_t *wavelength, double *reim, int64_t *end_base);
/* real^2 + im^2 of one wavelength's pair (statistics.c:365). */
double wtamd_energy_finish(const double *reim2);

/* Wig and bedGraph text on device (csrc/wt_text.hip): the reference's writer, printBlock of TeeWiggleIterator
 * (src/wigWriter.c:55-119; the parser's `write` and `write_bg`), over whole run lists: from a run list to the bytes of the
 * file, byte for byte what the reference prints.  The layout of wtamd_runs_histogram: n_seg segments, seg_off a HOST array of
 * n_seg + 1 offsets, start / finish / value (f32 or f64) DEVICE arrays; seg_name a HOST array of n_seg C strings of 1 to 255
 * bytes, copied verbatim; text DEVICE memory of `capacity` bytes at any alignment.  The door prints the list it is given: it
 * does not compress, sort or merge (wtamd_runs_compress is the writer's compression).
 * THE RULE.  The writer numbers the runs it receives from 0, across chromosomes, and prints them in blocks of
 * WTAMD_TEXT_BLOCK = 10000 consecutive entries (BLOCK_LENGTH).  Every block starts with pointByPoint = false, lastChrom = NULL,
 * lastFinish = -1: nothing about the mode crosses a block boundary.  L = finish - start.  With WTAMD_TEXT_BEDGRAPH no entry
 * is point-by-point; otherwise an entry is point-by-point iff the latest entry at or before it in its block with L < 2 or L > 5
 * exists and has L < 2 (wigWriter.c:69-74 as a "last setter" scan: entries with 2 <= L <= 5 hold the mode).  A point-by-point
 * entry prints L lines "%lf\n"; before them "fixedStep chrom=%s start=%i step=1\n" (start itself, 1-based) iff it is the
 * first entry of its block, or the previous entry of the block is not point-by-point, or lies in another segment, or
 * start > the previous entry's finish.  Any other entry prints "%s\t%i\t%i\t%lf\n" with start - 1 and finish - 1.
 * "%lf" is glibc's in round-to-nearest: sign, integer digits, '.', six digits -- the decimal expansion of the exact binary
 * value (f32 widened first), rounded half to even at the sixth decimal, computed in integers (csrc/wt_text.h);
 * '-' whenever the sign bit is set (-0.0 prints -0.000000, and so does -1e-9); nan / -nan by the sign bit, inf / -inf.
 * DEPARTURE: chromosome identity is the SEGMENT (the reference compares name pointers): two segments are two chromosomes
 * even where their names are equal.
 * WIDE VALUES.  Finite |v| >= 2^64 needs multi-word decimal conversion and is not printed on the device: the door counts them
 * in *n_wide and, if there is any, returns WTAMD_ERR_ARG with nothing written; the caller prints that batch on the host.
 * state (HOST, may be NULL: a fresh writer, nothing returned) chains the batches of one writer.
 * WTAMD_ERR_ARG, NOTHING written to text and state untouched: an unknown flag bit; a name outside 1 .. 255 bytes; in_block
 * outside 0 .. 9999; a run with start >= finish or start == INT32_MIN; fewer than 0 or at least 2^31 runs; any wide value.
 * WTAMD_ERR_CAPACITY when the text needs more than `capacity`: *n_bytes receives the size needed, not one byte of text is
 * written, state is untouched.  *n_bytes is always written on success; an empty call returns 0 bytes and leaves state untouched.
 * One workgroup per block of the reference, two passes (measure, emit) around a scan of the blocks' sizes; no atomics on
 * global memory: the same list gives the same bytes on every call.  Synchronous on `stream`; temporary memory from the device
 * pool: 32 bytes per 10000 runs, 12 bytes and the name per segment, 64 bytes of scalars. */
#define WTAMD_TEXT_BLOCK 10000
#define WTAMD_TEXT_BEDGRAPH 1u
typedef struct {            /* HOST, in / out: chains batches of one writer; all zero = a fresh writer            */
    int32_t in_block;       /* entries already in the current block, 0 .. 9999; 0: the three below are ignored */
    int32_t point_by_point; /* mode after the last entry                                                       */
    int32_t last_finish;    /* finish of the last entry                                                        */
    int32_t continues;      /* in: this call's first non-empty segment is the chromosome of the last entry;    */
} wtamd_text_state;         /* out: 1 after a call with runs -- the caller clears it before a new chromosome   */
int wtamd_runs_text(int64_t n_seg, const int64_t *seg_off, const char *const *seg_name,
                    const int32_t *start, const int32_t *finish, const void *value, int value_is_f64,
                    uint32_t flags, wtamd_text_state *state, char *text, int64_t capacity,
                    int64_t *n_bytes, int64_t *n_wide, void *stream);
/* The same over run lists held in HOST arrays, double values and a HOST text buffer: device memory, copies and the call on
 * the null stream. */
int wtamd_runs_text_host(int64_t n_seg, const int64_t *seg_off, const char *const *seg_name,
                         const int32_t *start, const int32_t *finish, const double *value,
                         uint32_t flags, wtamd_text_state *state, char *text, int64_t capacity,
                         int64_t *n_bytes, int64_t *n_wide);

/* Multi-column wig, bedGraph and paste text on device (csrc/wt_mtext.hip): the reference's Multiplexer writer, printBlock of
 * TeeMultiplexer / PasteMultiplexer (src/mWigWriter.c:56-133; the parser's `mwrite`, `mwrite_bg`, `apply_paste`), byte for
 * byte.  The layout of wtamd_runs_text plus a tile: values is a DEVICE array of n * width doubles, row r at values + r * width
 * (a track that is not in play holds its default in the tile, as the materialising kernel writes it; inplay is not read).
 * ROW(r) is, for every column, "\t" and "%lf" of the cell (wtamd_runs_text's "%lf"), then "\n".  Blocks of WTAMD_TEXT_BLOCK
 * entries, the mode and the header rule are those of wtamd_runs_text.  A point-by-point entry prints its header (if any) and
 * ROW(r) L times; any other entry prints "%s\t%i\t%i" (name, start - 1, finish - 1) and ROW(r): at width 1 the line
 * wtamd_runs_text prints.  PASTE: with prefix (DEVICE bytes) and prefix_off (DEVICE, n + 1 offsets; both or neither) entry r
 * prints its prefix bytes verbatim (0 bytes is legal) and ROW(r); the mode is bedGraph.  Chromosome identity is the segment.
 * width runs from 1 to WTAMD_MTEXT_MAX_WIDTH.  A finite cell of 2^64 or more is counted in *n_wide and refused, as there.
 * WTAMD_ERR_ARG, NOTHING written and state untouched: what wtamd_runs_text refuses (WTAMD_MTEXT_STRICT is an unknown flag
 * here); a width outside the limits; one of prefix / prefix_off without the other; prefix offsets that decrease.
 * WTAMD_ERR_CAPACITY, the state, the empty call and determinism: as wtamd_runs_text.  Four passes (cells, mode, scan, emit), no
 * floating-point and no global atomics.  Synchronous on `stream`; temporary memory from the device pool: 4 bytes per entry, 8
 * per 256 entries, 8 per 10000 entries, 4 per max(1, 2048 / width) entries, 12 bytes and the name per segment, 64 of scalars. */
#define WTAMD_MTEXT_BEDGRAPH 1u
#define WTAMD_MTEXT_STRICT 2u       /* wtamd_trackset_mtext only */
#define WTAMD_MTEXT_MAX_WIDTH 65536
int wtamd_tile_text(int64_t n_seg, const int64_t *seg_off, const char *const *seg_name,
                    const int32_t *start, const int32_t *finish, const double *values, int32_t width,
                    const char *prefix, const int64_t *prefix_off,
                    uint32_t flags, wtamd_text_state *state, char *text, int64_t capacity,
                    int64_t *n_bytes, int64_t *n_wide, void *stream);
/* The same over HOST arrays (prefix and prefix_off included) and a HOST text buffer: device memory from the pool, copies and
 * the call on the null stream. */
int wtamd_tile_text_host(int64_t n_seg, const int64_t *seg_off, const char *const *seg_name,
                         const int32_t *start, const int32_t *finish, const double *values, int32_t width,
                         const char *prefix, const int64_t *prefix_off,
                         uint32_t flags, wtamd_text_state *state, char *text, int64_t capacity,
                         int64_t *n_bytes, int64_t *n_wide);
/* `mwrite` / `mwrite_bg` of a resident track set: the Multiplexer tile is materialised on the device (the route of
 * wtamd_multiplex_host; WTAMD_MTEXT_STRICT asks for WTAMD_STRICT_SET0) and printed by the passes above with the chromosomes
 * as segments (chrom_name: HOST, n_chrom names of 1 .. 255 bytes); the tile never leaves HBM.  text: DEVICE memory.  *n_runs
 * (may be NULL) receives the number of entries.  Device memory: what wtamd_multiplex_host allocates (16 bytes per run of
 * wtamd_trackset_max_runs, 9 bytes per run and track, 8 per chromosome) plus the text passes' scratch.  A genome that does not
 * fit is cut by the caller into track sets with range_lo / range_hi; `state` (HOST, may be NULL) chains the pieces' texts as
 * in wtamd_runs_text -- the caller clears `continues` where a piece starts a new chromosome.  Synchronous. */
int wtamd_trackset_mtext(wtamd_trackset *ts, const char *const *chrom_name, uint32_t flags, wtamd_text_state *state,
                         char *text, int64_t capacity, int64_t *n_bytes, int64_t *n_wide, int64_t *n_runs, void *stream);
/* The same into a HOST text buffer. */
int wtamd_trackset_mtext_host(wtamd_trackset *ts, const char *const *chrom_name, uint32_t flags, wtamd_text_state *state,
                              char *text, int64_t capacity, int64_t *n_bytes, int64_t *n_wide, int64_t *n_runs);

/* Wig, bedGraph and BED text INTO run lists on the device (csrc/wt_read.hip; csrc/wt_read.h is the single source of the rule):
 * the inverse of wtamd_runs_text, the reference's WiggleReader (src/wigReader.c) and BedReader (src/bedReader.c) over the bytes
 * of a file.  text: DEVICE memory, n_bytes of WHOLE LINES at any alignment: the last byte is '\n', unless WTAMD_READ_EOF is set
 * for a file's unterminated last line; anything else is WTAMD_ERR_ARG.  state (HOST, in / out, all zero at the start of a file)
 * carries from one chunk to the next: the reading mode, span, step and the start of the next fixedStep line, the last record's
 * start, the latest header's chromosome and -- DEPARTURE from one name: a header may name a chromosome no record has yet, so
 * `continues` needs its own -- the last record's name (each: length and up to 255 bytes).
 * THE RULE.  Every line is one of
 *   skipped  the first byte is '#', or the line begins with "track" (wigReader.c:153-165); any bytes may follow.
 *   header   "fixedStep" or "variableStep", then key=value tokens, each after a single space or tab.  fixedStep takes chrom,
 *            start, step (all three compulsory) and optionally span; variableStep takes chrom and optionally span; a key at most
 *            once; span restarts at 1 with every header (wigReader.c:47).  A header sets the mode, the chromosome and, for
 *            fixedStep, the position of the first data line.  A chrom value holds no '=' (the reference's strtok cuts there);
 *            one that ENDS the header line keeps the line's '\n' in the name, as the reference's strtok leaves it: the name's
 *            length includes it ("variableStep chrom=chr1\n" names "chr1\n"), and 255 bytes is the limit with it.
 *   data     fields separated by exactly one space or tab, nothing leading or trailing (the reference's countWords: 1 + the
 *            separator bytes).  4 fields `name int int number`: the record (name, a + 1, b + 1, v); it sets the mode to
 *            bedGraph.  2 fields `int number`: (chrom, p, p + span, v), regular only while the latest mode setter is a
 *            variableStep header.  1 field `number`: the k-th data line after a fixedStep header (k from 0) is (chrom, start +
 *            k step, that + span, v), regular only while the latest setter is a fixedStep header.  Skipped lines do not count.
 * With WTAMD_READ_BED (bedReader.c:41-52) every line that is not "#..." is name, blanks (spaces or tabs, one or more), int,
 * blanks, int, then anything, and gives (name, a + 1, b + 1, 1.0); a record that sorts before its predecessor (strcmp of the
 * names below zero, or equal names and a lower start) is counted in n_unsorted and the call is refused.
 * An `int` is an optional '-', then 0 or a decimal without a leading zero, inside int32 after the + 1 / + span (the reference's
 * %i reads 010 as 8 and 0x10 as 16: those are irregular).  A `number` is an optional '-', digits with an optional '.' and
 * digits (or '.' digits), an optional e|E[+-] and 1 to 3 digits; or exactly nan, -nan, inf, -inf.  A name is 1 to 255 bytes
 * above 0x20.  Everything else is IRREGULAR: a '\r', an empty line, a line of 4999 bytes or more (fgets(5000) would split it),
 * a double separator, an unknown or repeated header key, step or span below 1, a keyword followed by something else than a
 * space or tab, a coordinate outside int32.  Irregular lines are counted and the byte offset of the first is reported; if there
 * is any the call returns WTAMD_ERR_ARG, writes nothing to the arrays and leaves the state untouched (with irregular lines only
 * n_lines, n_irregular and first_irregular of counts are defined); the host sweep (wtr_host) reads the same rule on the host.
 * VALUES, bit for bit strtod's.  W = the number's digits without leading zeros and without the fraction's trailing zeros, E
 * the decimal exponent that goes with it.  W = 0 gives +-0.  W <= 2^53 and |E| <= 22: (double) W * 10^E or (double) W / 10^-E
 * from a table of the 23 exact powers, ONE correctly rounded operation (Clinger's fast path) -- every line wtamd_runs_text
 * prints for |v| < 9.0e9 ("%lf" has six decimals: beyond that W passes 2^53 unless they end in zeros).
 * Any other regular number is SLOW: its record index and the byte offset of its number go to slow_rec /
 * slow_off in record order, its value is written as NaN and the caller patches it with strtod (the _host door does).
 * SEGMENTS.  Records come out in line order, one per data line.  A record opens a segment when it is the call's first or its
 * name differs bytewise from the previous record's.  seg_off (DEVICE, seg_capacity + 1 entries; seg_off[n_seg] = n_runs)
 * holds each segment's first record, seg_name_off / seg_name_len (seg_capacity entries) the name's byte offset in text and its
 * length; an offset of -1 is the chromosome of the state that came in (a header of an earlier chunk); no other negative
 * offset is ever written (the state's last record's name is compared inside the passes only).  counts->continues: the
 * first record's name is the name of the incoming state's last record.  The door does not compress, merge or sort.
 * WTAMD_ERR_CAPACITY: counts holds what is needed (n_runs, n_seg, n_slow); nothing written, state untouched.  An empty call
 * leaves the state alone.  Unknown flag bits: WTAMD_ERR_ARG.  Six passes (lines, scan, count, scan2, write, state) of one
 * kernel, no atomics on global memory, no floating-point reduction: the same text gives the same bytes.  Synchronous on
 * `stream`; temporary memory from the device pool: 112 bytes per 4096 bytes of text, 1088 of states, 128 of scalars. */
#define WTAMD_READ_BED 1u
#define WTAMD_READ_EOF 2u
#define WTAMD_READ_BEDGRAPH_MODE 0
#define WTAMD_READ_FIXED_MODE 1
#define WTAMD_READ_VARIABLE_MODE 2
typedef struct {            /* HOST, in / out: chains the chunks of one file; all zero = the start of a file  */
    int32_t mode;           /* WTAMD_READ_*_MODE: the latest mode setter                                       */
    int32_t span, step;     /* of the latest header                                                            */
    int32_t last_start;     /* of the last record                                                              */
    int64_t next;           /* the start of the next fixedStep line                                            */
    int32_t chrom_len;      /* bytes of chrom                                                                  */
    int32_t rec_len;        /* bytes of rec_name; 0: no record yet                                             */
    char chrom[256];        /* the latest header's chromosome                                                  */
    char rec_name[256];     /* the last record's name                                                          */
} wtamd_read_state;         /* 544 bytes                                                                       */
typedef struct {
    int64_t n_lines, n_runs, n_seg, n_slow, n_irregular, first_irregular /* -1: none */, n_unsorted, continues;
} wtamd_read_counts;
int wtamd_text_runs(const char *text, int64_t n_bytes, uint32_t flags, wtamd_read_state *state,
                    int32_t *start, int32_t *finish, double *value, int64_t capacity,
                    int64_t *seg_off, int64_t *seg_name_off, int32_t *seg_name_len, int64_t seg_capacity,
                    int64_t *slow_rec, int64_t *slow_off, int64_t slow_capacity,
                    wtamd_read_counts *counts, void *stream);
/* The same over a HOST text buffer and HOST outputs, the slow values patched by strtod; seg_name (may be NULL) receives the
 * names one after the other, seg_name_cap bytes in all, each closed by a 0 byte (a name taken from the incoming state
 * included): WTAMD_ERR_CAPACITY when they do not fit.  Device memory from the pool, copies and the call on the null stream. */
int wtamd_text_runs_host(const char *text, int64_t n_bytes, uint32_t flags, wtamd_read_state *state,
                         int32_t *start, int32_t *finish, double *value, int64_t capacity,
                         int64_t *seg_off, int64_t *seg_name_off, int32_t *seg_name_len, int64_t seg_capacity,
                         char *seg_name, int64_t seg_name_cap, wtamd_read_counts *counts);

/* Run compression on device (reference CompressionWiggleIterator, unaryOps.c:235-253, which the
 * default writer applies, wigWriter.c:263-267): adjacent runs of one chromosome merge while
 * start == previous finish and (both NaN or |value - value of the group's first run| < 1e-6).
 * `in` / `out` are DEVICE run lists (in->chrom_run_off required); *n_out is written on the host. */
int wtamd_runs_compress(const wtamd_runs *in, int64_t n_runs, int32_t n_chrom, wtamd_runs *out,
                        int64_t *n_out, void *stream);

int wtamd_get_stats(const wtamd_trackset *ts, wtamd_stats *out);

/* ---- Streaming pipeline (what the drop-in layer feeds; replaces the producer / consumer
 * overlap the reference gets from src/bufferedReader.c:41-55,99-109 -- 10 000-entry SoA blocks, a
 * producer up to 3 blocks ahead -- and the per-run evaluation behind it).
 *
 * A pipe owns `n_slots` batch slots.  Each slot has PINNED host staging for one batch of run lists
 * (one chromosome, run starts in [lo, hi)), device buffers allocated once, and pinned host output.
 * submit() enqueues  H2D (copy stream) -> window index + multiplex/reduce kernels (compute
 * stream) -> D2H of exactly the emitted runs (third stream)  and returns at once, so the caller
 * fills slot k+1 while slot k computes and slot k-1 is being read.  Values stay float32 end to end
 * when the source's values are float32-exact.  Nothing is allocated or freed per batch.
 *
 *   acquire -> fill the staging arrays (grow if needed) -> submit     (repeat, up to n_slots deep)
 *   collect -> read the result arrays -> release                       (in submission order)      */
#define WTAMD_OP_MULTIPLEX 12   /* pipe only: the aligned tile values[]/inplay[] per run (multiplexer.h:21-36) */
#define WTAMD_PIPE_COMPRESS 1u  /* apply CompressionWiggleIterator's merge rule on device before D2H (unaryOps.c:235-253) */

typedef struct wtamd_pipe wtamd_pipe;

typedef struct {
    int32_t n_tracks;
    int32_t n_slots;            /* 2..8 batches in flight; 0 = 3 */
    const double *defaults;     /* HOST, n_tracks default_values */
    wtamd_reduce_desc desc;     /* op may also be WTAMD_OP_MULTIPLEX */
    int64_t max_intervals;      /* initial input capacity of a slot (wtamd_pipe_grow enlarges it) */
    int64_t max_runs;           /* output capacity of a slot, fixed: keep hi - lo <= max_runs (a run is >= 1 bp) */
    uint32_t flags;             /* WTAMD_PIPE_* */
    int32_t reserved;
} wtamd_pipe_config;

typedef struct {                /* pinned staging of the slot being filled */
    int64_t capacity;           /* intervals the arrays below hold */
    int64_t *seg_off;           /* n_tracks + 1 offsets into the arrays (seg_off[0] = 0) */
    int32_t *start, *finish;
    float *value32;             /* always present */
    double *value64;            /* NULL until wtamd_pipe_grow(.., want_f64 = 1) */
} wtamd_pipe_batch;

typedef struct {                /* pinned output of the oldest submitted batch, valid until release */
    int64_t n_runs;
    const int32_t *start, *finish;
    const double *value;        /* reducer value; WTAMD_OP_MULTIPLEX: the run's inplay_count */
    const double *tile;         /* WTAMD_OP_MULTIPLEX: n_runs * n_tracks values, else NULL */
    const uint8_t *inplay;      /* WTAMD_OP_MULTIPLEX: n_runs * n_tracks flags, else NULL */
    int64_t covered_bp;         /* sum (finish - start) of the runs the kernels emitted (before compression) */
    int64_t n_intervals;        /* input intervals of the batch */
    int32_t integ_valid;        /* the batch was integrated on device (wtamd_pipe_set_integrate): start / finish / value are NULL */
    int32_t reserved;
    double integ[6];            /* reducers: {sum of (finish - start) * value, span} over the non-NaN runs (statistics.c:62-120);
                                   WTAMD_OP_MULTIPLEX over 2 tracks: the Pearson moments {n, sum_X, sum_Y, T_XX, T_XY, T_YY} (:414-465) */
} wtamd_pipe_result;

typedef struct {
    int64_t batches, intervals, runs, covered_bp;
    int64_t h2d_bytes, d2h_bytes;
    double kernel_ms;           /* sum over batches of index + reduce kernel time (HIP events on the compute stream) */
    double h2d_ms, d2h_ms;      /* same for the copies (events on their streams) */
    int32_t delta_batches;      /* batches the exact difference-array kernel evaluated */
    int32_t n_slots;
    double host_submit_ms;      /* host time inside wtamd_pipe_submit (enqueueing; nothing there waits for the GPU) */
    double host_wait_ms;        /* host time wtamd_pipe_collect spent waiting for a batch to finish */
    int64_t bw_sections;        /* BigWig sections inflated on device (wtamd_pipe_submit_bw) */
    double bw_decode_ms;        /* ... and the summed duration of their inflate / count / scan / scatter kernels (HIP events) */
} wtamd_pipe_stats;

int wtamd_pipe_create(const wtamd_pipe_config *cfg, wtamd_pipe **out);
void wtamd_pipe_destroy(wtamd_pipe *);
/* Staging of the next free slot.  WTAMD_ERR_ARG when every slot is in flight or unreleased. */
int wtamd_pipe_acquire(wtamd_pipe *, wtamd_pipe_batch *out);
/* Enlarges the acquired slot's staging to >= min_capacity intervals (and adds the float64 value
 * array if want_f64), preserving the first `used` entries of every array; *out is refreshed. */
int wtamd_pipe_grow(wtamd_pipe *, int64_t used, int64_t min_capacity, int want_f64, wtamd_pipe_batch *out);
/* Bulk side door: `count` float32-valued intervals of the acquired slot, at interval offset `at`
 * of its arrays, are NOT staged -- the pipe copies them to HBM straight from the caller's arrays at
 * submit (hipMemcpyAsync).  The arrays must stay valid and unchanged until the batch has been
 * collected and should be pinned (wtamd_host_alloc); pageable memory still works but the copy is
 * then staged by the runtime.  The staging arrays need not cover such ranges. */
int wtamd_pipe_put_direct(wtamd_pipe *, int64_t at, int64_t count, const int32_t *start, const int32_t *finish,
                          const float *value);
/* Ships the acquired slot: seg_off[n_tracks] intervals of one chromosome, runs whose start lies in
 * [range_lo, range_hi) are produced (same meaning as wtamd_tracks.range_lo/hi).  Asynchronous. */
int wtamd_pipe_submit(wtamd_pipe *, int value_is_f64, int32_t range_lo, int32_t range_hi);
/* Abandons the acquired slot without shipping it. */
int wtamd_pipe_cancel(wtamd_pipe *);
/* Result of the oldest submitted batch (waits for it). */
int wtamd_pipe_collect(wtamd_pipe *, wtamd_pipe_result *out);
/* Returns the oldest collected batch's slot to the pipe. */
int wtamd_pipe_release(wtamd_pipe *);
/* Turns the device-side run compression on / off for the batches submitted from now on: the
 * reference's CompressionWiggleIterator rule (unaryOps.c:235-253) inside every batch, from the batch's
 * first run that leads a group whatever came before it (the runs ahead of it may belong to the
 * previous batch's last group -- only a consumer that knows that group's leader can tell -- and are
 * passed through one by one).  Applying the reference's own wrapper to this output, as the default
 * writer always does (wigWriter.c:263-267), yields exactly what it yields on the uncompressed runs. */
int wtamd_pipe_set_compress(wtamd_pipe *, int on);
/* Genome-wide integrators fused into the pipeline (reference AUCIntegrator / MeanIntegrator over a reducer,
 * PearsonIntegrator over a 2-track Multiplexer: statistics.c:62-127,414-465): batches submitted from now on are
 * integrated ON THE DEVICE and their runs never cross PCIe -- a result carries 2 (6) doubles instead of 16 bytes
 * per run.  Sums are two-level (per lane slice, then ordered merge): agreement with the reference's sequential
 * accumulation to rounding.  Not together with WTAMD_PIPE_COMPRESS. */
int wtamd_pipe_set_integrate(wtamd_pipe *, int on);
/* on == 2 (reducers only): the batch's six run moments of wtamd_runs_moments come home in integ[0..5] instead, for
 * varI / stddevI / CVI / maxI / minI / span; merge batches in order with wtamd_moments_merge.  on == 1 is unchanged
 * (integ[2..5] zero for a reducer).  wtamd_pipe_integrate_modes: the highest `on` this pipe serves (2 for a reducer,
 * 1 for the Multiplexer tile) -- a pipeline that predates mode 2 does not export it. */
int wtamd_pipe_integrate_modes(const wtamd_pipe *);
/* The same integrals of the batch currently held (collected, not released) when it travelled the ordinary way
 * -- the batch a reducer's constructor primed with before an integrator took it over.  integ[6] as above. */
int wtamd_pipe_integrate_held(wtamd_pipe *, double *integ);
/* Submitted batches not yet collected. */
int wtamd_pipe_in_flight(const wtamd_pipe *);
int wtamd_pipe_get_stats(const wtamd_pipe *, wtamd_pipe_stats *out);

/* ---- BigWig sections decoded ON THE DEVICE (csrc/wt_bwdev.hip, csrc/wt_inflate.h).  A batch may be handed
 * over as the FILE BYTES of the BigWig data sections that overlap it instead of as run lists: the pipe
 * ships the compressed bytes (2.5 x fewer than the run lists), inflates every section on the GPU -- one
 * lane per zlib stream -- and expands the items into the slot's run lists with the reference reader's
 * conventions (1-based starts, 10 000-bp boxing, seek window: src/bigWiggleReader.c:36-83,125-145).  This
 * replaces the host-side inflate the reference gets from libBigWig; wtamd_BigWiggleReader children of a
 * reducer of this library take this route on their own (WTAMD_BW_DEVICE=0 keeps the host decoder).
 *
 *   acquire -> wtamd_pipe_bw_reserve -> fill bytes[] and sections[] -> wtamd_pipe_submit_bw -> collect ...
 *
 * Sections are listed track by track (track-major, ascending position inside a track); a track's
 * intervals must come out sorted and non-overlapping (checked on device: the batch fails otherwise). */
typedef struct {
    int64_t comp_off;               /* first byte of the section in bytes[] (any alignment) */
    uint32_t comp_size;             /* its size there */
    int32_t track;
    uint32_t leaf_start, leaf_end;  /* extents of the section in the file's R-tree leaf, 0-based half-open: every item must
                                       lie inside (checked on device) */
} wtamd_bw_section;

typedef struct {
    uint32_t chrom_id;              /* the file's id of the batch's chromosome (sections of other ids yield nothing) */
    uint32_t chrom_len;             /* its length in that file (bounds the boxing, bigWiggleReader.c:76) */
    int32_t box;                    /* != 0: cut intervals at the reader's 10 000-bp stretch edges (:42-44,73-83) */
    int32_t compressed;             /* != 0: sections are zlib streams (header uncompressBufSize != 0) */
    int32_t clip_lo, clip_hi;       /* pieces are clipped to [clip_lo, clip_hi) (1-based) and dropped when empty */
    int32_t first_section;          /* this track's slice of sections[]: [first_section, first_section + n_sections); */
    int32_t n_sections;             /*   first_section of a track without sections = that of the next track           */
    uint32_t plain_bytes;           /* upper bound of a section's inflated size (the file's uncompressBufSize; raw: its largest section) */
    int32_t reserved;
} wtamd_bw_track;

/* Pinned staging of the acquired slot for `n_bytes` file bytes and `n_sections` table entries (grown on
 * demand, contents undefined).  Pointers stay valid until the slot is submitted or cancelled. */
int wtamd_pipe_bw_reserve(wtamd_pipe *, int64_t n_bytes, int64_t n_sections, uint8_t **bytes, wtamd_bw_section **sections);
/* Ships the acquired slot as file bytes: tracks[n_tracks] describe the tracks, the tables / bytes are the
 * reserved ones; runs whose start lies in [range_lo, range_hi) are produced, as for wtamd_pipe_submit.
 * A malformed stream / section fails the batch at collect (WTAMD_ERR_INTERNAL with the cause). */
int wtamd_pipe_submit_bw(wtamd_pipe *, int64_t n_bytes, int64_t n_sections, const wtamd_bw_track *tracks,
                         int32_t range_lo, int32_t range_hi);
/* How many sections one launch of the inflate kernel keeps resident on the device (wavefronts the GPU holds at
 * once x 64 lanes): a batch of about that many sections fills the GPU exactly once -- fewer leave SIMDs idle, a
 * few more cost a whole second round. */
int64_t wtamd_pipe_bw_fill_sections(const wtamd_pipe *);
/* Why the last wtamd_pipe_collect of a file-byte batch failed: the device decoder's error bits (1 corrupt zlib stream or
 * Adler-32 mismatch, 2 malformed section, 4 items outside their index leaf's extents / out of order, 8 coordinate above
 * the maximum, 16 more intervals than the bound); 0: it did not fail there.  The drop-in layer answers 1 / 2 / 4 by going
 * back to the host decoder from that batch on -- libBigWig, which the reference reads through, checks none of these
 * extents (src/bigWiggleReader.c:52-83). */
unsigned wtamd_pipe_bw_error(const wtamd_pipe *);
/* File-byte batches decoded a second time at collect because they held more intervals than the run lists sized from the
 * earlier batches' density (WT_BW_ERR_CAPACITY on the first pass), since the pipe was created. */
int64_t wtamd_pipe_bw_redone(const wtamd_pipe *);

/* Pinned (page-locked, DMA-able) host memory for bulk sources. */
void *wtamd_host_alloc(size_t bytes);
void wtamd_host_free(void *);
/* The process-wide pools behind the pipes, the track sets (their window tables, counters and staging) and the scratch of
 * the host entry points: page-locked memory (also wtamd_host_alloc; WTAMD_PINNED_POOL_MB) and
 * device buffers (WTAMD_DEVICE_POOL_MB).  out[0..2]: pinned buffers of 1 MB and more that had to be page-locked afresh
 * so far (count, bytes) and the bytes resting in the pool now; out[3..5]: the same for device buffers (hipMalloc).  A
 * second run of the same job in a process should add no misses. */
void wtamd_pool_stats(int64_t out[6]);
/* Gives every buffer resting in the two pools back to the runtime (a process that wants its device memory or its
 * lockable pages for something else; the pools also do this on their own when an allocation of theirs fails). */
void wtamd_pool_trim(void);

/* ---- Bulk doors of the drop-in layer ------------------------------------------------------
 * The reference's iterator protocol moves ONE interval per indirect call (wiggleIterator.c:57-60);
 * its own readers soften that with 10 000-entry SoA blocks between threads (bufferedReader.c:21-28).
 * A child iterator built by this library exposes such blocks to the Multiplexer directly (producer
 * side), and a reducer hands its runs over in blocks (consumer side -- what TeeWiggleIterator copies
 * into its 10 000-entry blocks one pop at a time, wigWriter.c:164-203).  Both stay ordinary
 * WiggleIterators: pop() / seek() work as always, foreign iterators are drained with pop(). */

/* Array-backed reader: one track as SoA run lists in host memory (chromosomes in strcmp order,
 * chromosome c = slice [seg_off[c], seg_off[c+1]) of the arrays; 1-based start, exclusive finish,
 * float32 value).  The arrays are borrowed (and read by DMA when pinned).  Bulk-capable. */
WiggleIterator *wtamd_ArrayReader(int n_chrom, const char *const *chrom_names, const int64_t *seg_off,
                                  const int32_t *start, const int32_t *finish, const float *value,
                                  double default_value);
/* The same arrays holding OVERLAPPING intervals: sorted by start only (finishes in any order), `overlaps` set -- what the
 * reference's BED / BAM / bigBed readers deliver.  seek() delivers the intervals that intersect the window, clipped, from a
 * filtered copy.  A Multiplexer puts the union in front of it (NonOverlappingWiggleIterator); wtamd_CoverageIterator turns
 * it into a depth track.  Bulk-capable. */
WiggleIterator *wtamd_OverlappingArrayReader(int n_chrom, const char *const *chrom_names, const int64_t *seg_off,
                                             const int32_t *start, const int32_t *finish, const float *value,
                                             double default_value);
/* The reference's CoverageWiggleIterator (src/unaryOps.c:303-375; the parser's `coverage`) on the device: returns `child`
 * itself when it does not overlap; otherwise drains it one chromosome at a time (in blocks when it is bulk-capable, by pop()
 * otherwise), computes the chromosome's depth track with wtamd_runs_coverage and serves it as a bulk source -- the
 * library's Multiplexer takes it in blocks, wtamd_iterator_next_block hands out the rest of the current chromosome, a
 * foreign pop() walks it run by run.  default_value 0, `overlaps` false; seek() seeks the child, then recomputes.  Values
 * are doubles for pop() / next_block and float32 inside Multiplexer blocks: exact up to a depth of 2^24.  WITHOUT the
 * reference's run of start == finish at the last distinct start of every stream (it reads the exhausted child's stale
 * start, :333-334).  WTAMD_NO_DEVICE_COVERAGE=1 (or a build of the drop-in layer without the HIP units) computes the same
 * list with a host sweep.  A child that is not sorted by start: message and exit(1). */
WiggleIterator *wtamd_CoverageIterator(WiggleIterator *child);
/* The reference's OverlapWiggleIterator / NoverlapWiggleIterator / TrimWiggleIterator / NearestWiggleIterator
 * (src/unaryOps.c:437-639) as one constructor; op is a wtamd_region_op (anything else: message and exit(1)).  Drains source
 * and mask one chromosome at a time (in blocks where the child is bulk-capable, by pop() otherwise), pairing chromosomes by
 * name in strcmp order as the reference does, computes the chromosome's result with wtamd_runs_region and serves it as a
 * bulk source: the library's Multiplexer takes it in blocks, wtamd_iterator_next_block hands out the rest of the current
 * chromosome, a foreign pop() walks it run by run.  default_value and `overlaps` are the source's; seek() seeks both
 * children, then recomputes.  Values are doubles for pop() / next_block and float32 inside Multiplexer blocks, where a
 * `nearest` distance above 2^24 is rounded.  A TRIM whose source overlaps itself is served by the reference's own
 * per-interval protocol on the host.  WTAMD_NO_DEVICE_REGION=1 (or a build of the drop-in layer without the HIP units)
 * computes the same lists with a host sweep.  A child that is not sorted by start: message and exit(1). */
WiggleIterator *wtamd_RegionIterator(int op, WiggleIterator *source, WiggleIterator *mask);

/* The reference's ApplyMultiplexer (apply.c:293-353; `apply` / `apply_paste`, commandParser.c readApply / readApplyPaste) on
 * wtamd_runs_apply: `count` values per region, values[i] = wtamd_apply_finish(moments, stats[i]) with stats[i] a
 * WTAMD_APPLY_* code; default_values NaN; chrom / start / finish the current region; primed with the first region, done after
 * the last; strict as the reference's flag (0: fill-in with the dataset's default_value).  It drains regions and dataset a
 * chromosome at a time -- in blocks from a bulk source or a reducer of this library, by pop() from anything else --, pairs
 * chromosomes by name in strcmp order and computes the chromosome's regions in one call.  seekMultiplexer seeks both
 * children and recomputes.  It works under SelectReduction and the reference's PasteMultiplexer.  WTAMD_NO_DEVICE_APPLY=1
 * (or a build of the drop-in layer without the HIP units) computes the same values with a host sweep by the same rules.
 * Refused with a message and exit(1): a dataset with `overlaps` set or one that is not disjoint, regions that are not sorted,
 * an unknown statistic -- keep the reference's ApplyMultiplexer for those.  The departures
 * listed at wtamd_runs_apply hold. */
Multiplexer *wtamd_ApplyMultiplexer(WiggleIterator *regions, const int *stats, int count, WiggleIterator *dataset, wt_bool strict);
/* The reference's ProfileMultiplexer (apply.c:355-366; `profile` / `profiles`, commandParser.c readProfile / readProfiles) on
 * wtamd_runs_profile: count = width values per region, the region's row; default_values NaN; never strict.  It drains, pairs
 * chromosomes, serves one region per popMultiplexer and seeks exactly as wtamd_ApplyMultiplexer does (the same code).
 * WTAMD_NO_DEVICE_PROFILE=1 (or a build of the drop-in layer without the HIP units) computes the same bits with a host sweep.
 * Refused with a message and exit(1): width < 1, a dataset with `overlaps` set or one that is not disjoint, regions that are not
 * sorted.  The departures listed at wtamd_runs_profile hold. */
Multiplexer *wtamd_ProfileMultiplexer(WiggleIterator *regions, int width, WiggleIterator *dataset);
/* The reference's BinningWiggleIterator (unaryOps.c:1027-1036; `bin`) and SmoothWiggleIterator (:1152-1162; `smooth`) on
 * wtamd_runs_bin / wtamd_runs_smooth: they drain the child one chromosome at a time (in blocks where it is a bulk source), put
 * the union in front when child->overlaps, compute the chromosome through the device door and serve the finished run list --
 * smooth in clip slices of 2^20 positions (WTAMD_WINDOW_SLICE=<n>: of n), so a chromosome never needs 16 bytes per base pair of host memory at once.  Bulk
 * sources themselves (a Multiplexer of this library and wtamd_iterator_next_block take them in blocks).  Defaults: child's x
 * width, child's.  seek seeks the child and recomputes.  WTAMD_NO_DEVICE_WINDOW=1 (or a build of the drop-in layer without the
 * HIP units) computes the same bits with a host sweep.  A chromosome with a start below 1 is served by the reference's own
 * per-pop protocol on the host (C's division towards zero, the prefill from position 1).  A width below 2: the reference's
 * message and exit(1).  A child that is not sorted, or overlaps without saying so: a message and exit(1).  Unlike the
 * reference's smooth, whose running sum carries over from one chromosome to the next, every chromosome starts from 0. */
WiggleIterator *wtamd_BinIterator(WiggleIterator *child, int width);
WiggleIterator *wtamd_SmoothIterator(WiggleIterator *child, int width);
/* The reference's histogram(), normalize_histogram() and print_histogram() (plots.c:167-223; `histogram`, commandParser.c
 * readHistogram) on wtamd_runs_histogram: row r is wigs[r].  Every child is drained whole (in blocks where it is a bulk source,
 * pop by pop otherwise) and its runs are held, 16 bytes per run of host memory, until the range is known; then one call of
 * wtamd_runs_histogram_host.  WTAMD_NO_DEVICE_HIST=1 (or a build of the drop-in layer without the HIP units) computes the same
 * bits with a host sweep.  normalize: the row sum over the columns in order, then the divisions; an empty row gives NaN.
 * print: "%f" of position + step / 2, "\t%f" per row, position += step iteratively, as the reference does.  width < 1,
 * count < 1, a run with start >= finish or an infinite value: a message and exit(1).  A first row without a non-NaN value, on
 * which the reference does not return, gives a NaN range and zeros.  The departures listed at wtamd_runs_histogram hold. */
typedef struct wtamd_histogram_st wtamd_Histogram;
wtamd_Histogram *wtamd_histogram(WiggleIterator **wigs, int count, int width);
void wtamd_normalize_histogram(wtamd_Histogram *hist);
void wtamd_print_histogram(wtamd_Histogram *hist, FILE *file);
int wtamd_histogram_width(const wtamd_Histogram *hist);
int wtamd_histogram_count(const wtamd_Histogram *hist);
const double *wtamd_histogram_row(const wtamd_Histogram *hist, int row);
void wtamd_histogram_range(const wtamd_Histogram *hist, double *lo_hi2);
void wtamd_destroy_histogram(wtamd_Histogram *hist);
/* The reference's EnergyIntegrator (statistics.c:345-391; called where the parser calls it, commandParser.c:677-681) on
 * wtamd_runs_energy, with the contract of the library's other integrators: pop it to the end, *(double *) data is then the
 * result real^2 + im^2 (NaN before the end, statistics.c:389), `append` is the source, the default is the child's; behind the
 * leading res, `data` keeps real and im where the reference's EnergyData has them.  The child is drained a chromosome at a time
 * (in blocks where it is a bulk source, pop by pop otherwise; an overlapping child goes through the reference's union rule
 * first), one wtamd_runs_energy_host call per chromosome with the running offset -- which grows by the last finish served when
 * the chromosome changes, the priming pop adding 0 --, and the chromosomes' sums are added in genome order.  One pop serves one
 * chromosome.  A seek carries the sums and the offset on, as the reference's does.  WTAMD_NO_DEVICE_ENERGY=1 (or a build of
 * the drop-in layer without the HIP units) sweeps on the host by the same rule (equal to rounding).  A wavelength < 1, which
 * the door refuses, is served by the reference's own per-position expression on the host: 0 gives NaN, a negative one what
 * the reference gives.  A child that is not sorted or holds a run with start >= finish: a message and exit(1).  The
 * departures listed at wtamd_runs_energy hold. */
WiggleIterator *wtamd_EnergyIntegrator(WiggleIterator *child, int wavelength);
/* n wavelengths from ONE drain of the child: reim[2 k], reim[2 k + 1] are what n integrators would hold as real and im, bit
 * for bit.  WTAMD_OK, or WTAMD_ERR_ARG for n < 1 or n above 1024. */
int wtamd_EnergySpectrum(WiggleIterator *child, int n, const int *wavelengths, double *reim);
/* The reference's writers, TeeWiggleIterator, toFile and toStdout (wigWriter.c:261-289; `write`, `write_bg`), on
 * wtamd_runs_text: the same bytes in the file.  The iterator passes the runs it prints on, one per pop() and in blocks through
 * wtamd_iterator_next_block.  bedGraph mode is forced for an overlapping child; otherwise the compression rule
 * (unaryOps.c:235-253) goes in front -- a reducer of this library is asked for it (wtamd_iterator_compress_output), and the
 * same rule runs on the host over every batch anyway, the open group carried across batches (the rule is idempotent) --, and
 * the runs passed on are the compressed ones.  A batch (one block of a reducer, one chromosome of any other child) is
 * formatted by wtamd_runs_text_host with a wtamd_text_state chaining the batches; a batch with a wide value,
 * WTAMD_NO_DEVICE_TEXT=1 and a build of the drop-in layer without the HIP units use the host sweep (the same bytes).
 * The text of a batch is written when all of its runs have been handed on (the next batch is fetched, or the child is
 * exhausted), the block of 10000 entries it leaves open when that block is full or at the end.  holdFire: nothing is written
 * before the first seek.  SEEK: the reference kills its writer thread and loses whatever it had not yet printed -- a race that
 * cannot be reproduced; here the complete 10000-entry blocks of what was handed on are written, the open block is dropped
 * (what the reference does when its thread keeps up), then fflush, the child is sought and the entry count restarts at 0.
 * wtamd_toFile closes the file it opened (the reference leaves it to exit()). */
WiggleIterator *wtamd_TeeWiggleIterator(WiggleIterator *wi, FILE *out, wt_bool bedGraph, wt_bool holdFire);
void wtamd_toFile(WiggleIterator *wi, char *filename, wt_bool bedGraph, wt_bool holdFire);
void wtamd_toStdout(WiggleIterator *wi, wt_bool bedGraph, wt_bool holdFire);
/* The reference's Multiplexer writers, TeeMultiplexer, toStdoutMultiplexer and PasteMultiplexer (mWigWriter.c:179-327;
 * `mwrite`, `mwrite_bg`, `apply_paste`), on wtamd_tile_text: the same bytes in the file.  The returned Multiplexer shares
 * values / inplay / default_values with `in`, copies chrom / start / finish on every pop, records the entry and pops `in`; it
 * is primed by one pop and works over any `in` (this library's Multiplexer, wtamd_ApplyMultiplexer, wtamd_ProfileMultiplexer,
 * a foreign one).  Complete blocks of 10000 entries are formatted by wtamd_tile_text_host, several per call, and fwritten; the
 * open block at the end.  WTAMD_NO_DEVICE_MTEXT=1, a batch with a wide value and a build of the drop-in layer without the HIP
 * units use the host sweep (the same bytes).  Paste reads one line of `infile` per entry exactly as the reference does
 * (fgets of 5000 bytes, empty / `track` / `browser` lines skipped, trailing \n and \r stripped; a file that runs out: what was
 * recorded is written, then the reference's message and exit(1)).  SEEK and holdFire: as wtamd_TeeWiggleIterator -- complete
 * blocks of what was handed on are written, the open block is dropped, fflush, `in` is sought, the count restarts.  The tile
 * still comes home on this path (its callers read the struct); wtamd_trackset_mtext is the path on which it does not. */
Multiplexer *wtamd_TeeMultiplexer(Multiplexer *in, FILE *out, wt_bool bedGraph, wt_bool holdFire);
void wtamd_toStdoutMultiplexer(Multiplexer *in, wt_bool bedGraph, wt_bool holdFire);
Multiplexer *wtamd_PasteMultiplexer(Multiplexer *in, FILE *infile, FILE *outfile, wt_bool holdFire);

/* The reference's text readers (csrc/wt_abi_read.h): WiggleReader (src/wigReader.c: wig fixedStep / variableStep and bedGraph,
 * its compression rule behind it, overlaps false, default 0) and BedReader (src/bedReader.c: value 1, overlaps true).  Served
 * run lists: bulk sources to this library's Multiplexer and to wtamd_iterator_next_block, one run per pop() to anything else.
 * The file is read in chunks cut at the last newline (WTAMD_READ_CHUNK_MB, default 64) through wtamd_text_runs_host, a
 * wtamd_read_state chaining them; WTAMD_NO_DEVICE_READ=1, a build without the HIP units, and every chunk from the first one the
 * door refuses on (an irregular line, an unsorted BED record) are read as the reference reads them: sscanf / strtok, its
 * messages and exit(1) ("Badly formatted ...", "Invalid header ...", "Bed file ... is not sorted!"), fgets(5000) pieces.
 * seek follows WiggleReaderSeek / BedReaderSeek; the file is reopened for it.  "-" reads stdin forwards; DEPARTURE: any seek on
 * it ends as the reference's failed fopen does (the reference can seek stdin forwards). */
WiggleIterator *wtamd_WiggleReader(char *path);
WiggleIterator *wtamd_BedReader(char *path);
/* BigWig reader: the role of the reference's BigWiggleReader (src/bigWiggleReader.c:147-151) on this
 * library's own section decoder -- chromosomes in strcmp order, 1-based starts, box != 0: intervals
 * cut at the reference reader's 10 000-bp stretch edges (what `write_bg` parity needs); one producer
 * thread per file decodes the next chromosome while the current one is consumed.  Bulk-capable.
 * A file that is not BigWig: the reference's message and exit(1). */
WiggleIterator *wtamd_BigWiggleReader(const char *path, int box);
/* The same for n files at once, opened side by side on a few threads (every constructor reads its file's index and
 * primes: ~1-2 ms per file, which 100 tracks would otherwise pay one after the other before the first run). */
int wtamd_BigWiggleReaders(int n, const char *const *paths, int box, WiggleIterator **out);
/* Releases what destroyWiggleIterator (wiggleIterator.c:52-55) cannot know about: the file, the decode buffers and
 * the producer thread (joined).  The iterator stays the caller's to free; it must not be popped, sought or given to
 * a reducer afterwards.  A reader that is never closed keeps its file descriptor and, once its second part has been
 * asked for, one idle thread for the life of the process (the reference's reader thread is never joined either,
 * bigWiggleReader.c:147-151).  WTAMD_ERR_ARG for anything that is not an open wtamd_BigWiggleReader. */
int wtamd_BigWiggleReader_close(WiggleIterator *wi);
/* Fused integrators (reference AUCIntegrator / MeanIntegrator, statistics.c:62-127; PearsonIntegrator :414-465; built
 * by commandParser.c:653-704).  Same contract towards the consumer that prints the result: an iterator to be popped
 * to its end whose `data` starts with the double result and whose `append` is the source
 * (PrintStatisticsWiggleIteratorPop, statistics.c:574-590).  Handed a reducer / a 2-track Multiplexer of THIS library
 * that nothing else has popped yet, the integration happens on the device batch by batch and no per-position run
 * is exported: the iterator then yields ONE element per batch (the batch's window, value NaN) instead of one per run
 * -- use the reference's own integrators when something downstream reads the runs.  Anything else: the reference's
 * per-run pass-through on the host. */
WiggleIterator *wtamd_AUCIntegrator(WiggleIterator *wi);
WiggleIterator *wtamd_MeanIntegrator(WiggleIterator *wi);
WiggleIterator *wtamd_PearsonIntegrator(Multiplexer *multi);
/* varI / stddevI / CVI / maxI / minI (statistics.c:159-326, commandParser.c:653-704) and the SpanIntegrator the
 * reference's library exports (:129-157), under the same contract: fused over a reducer of this library (six doubles
 * per batch come home, wtamd_pipe_set_integrate mode 2), the reference's per-run pass-through otherwise.  One departure:
 * the reference's VarianceCorePop returns on a NaN run WITHOUT popping its source (:238-239), so its varI / stddevI / CVI
 * never end over a source with a NaN run; these skip NaN runs, as its min / max / span / mean / AUC do. */
WiggleIterator *wtamd_VarianceIntegrator(WiggleIterator *wi);
WiggleIterator *wtamd_StandardDeviationIntegrator(WiggleIterator *wi);
WiggleIterator *wtamd_CoefficientOfVariationIntegrator(WiggleIterator *wi);
WiggleIterator *wtamd_MaxIntegrator(WiggleIterator *wi);
WiggleIterator *wtamd_MinIntegrator(WiggleIterator *wi);
WiggleIterator *wtamd_SpanIntegrator(WiggleIterator *wi);
/* Consumer door, for reducers built by this library: the runs from the iterator's current element
 * to the end of the batch it belongs to (a wtamd_CoverageIterator: to the end of its chromosome), as arrays valid until
 * the next call on `wi`.  Returns the
 * number of runs (0 and wi->done at the end).  Mixes freely with pop(). */
int64_t wtamd_iterator_next_block(WiggleIterator *wi, const char **chrom, const int32_t **start,
                                  const int32_t **finish, const double **value);
/* Writer hand-off: asks a reducer of this library to merge its runs on the device before they
 * cross PCIe (wtamd_pipe_set_compress on its pipeline; batches already in flight are unaffected).
 * Meant for the iterator the default writer wraps in CompressionWiggleIterator anyway
 * (TeeWiggleIterator, wigWriter.c:261-267): the text written is byte-identical, the pops and the
 * D2H traffic shrink by the compression ratio.  Returns WTAMD_ERR_ARG for any other iterator. */
int wtamd_iterator_compress_output(WiggleIterator *wi, int on);
/* Counters of the pipeline behind a reducer of this library (bytes over PCIe, summed kernel / copy
 * durations from HIP events).  Returns WTAMD_ERR_ARG for any other iterator. */
int wtamd_iterator_pipe_stats(WiggleIterator *wi, wtamd_pipe_stats *out);
/* runWiggleIterator with counters: pops `wi` to the end one run at a time (the reference's own
 * protocol, wiggleIterator.c:62-65); returns the number of runs, their covered bp and value sum. */
int64_t wtamd_drain(WiggleIterator *wi, int64_t *covered_bp, double *value_sum);

/* ---- BigWig section decoder (bulk side door; replaces what the reference gets from libBigWig
 * through src/bigWiggleReader.c:52-83).  HOST only. ---- */
typedef struct wtamd_bw wtamd_bw;
int wtamd_bw_open(const char *path, wtamd_bw **out);    /* prints the reference's message on a non-BigWig file */
void wtamd_bw_close(wtamd_bw *);
int wtamd_bw_n_chrom(const wtamd_bw *);
const char *wtamd_bw_chrom_name(const wtamd_bw *, int i);
uint32_t wtamd_bw_chrom_length(const wtamd_bw *, int i);
/* All runs of one chromosome, 1-based start / exclusive finish, sorted.  box != 0 cuts runs at the
 * reference reader's 10 000-bp stretch edges (bigWiggleReader.c:42-44,73-83).  Returns the number
 * of runs; when that exceeds `capacity` nothing was written (call again with more room). */
int64_t wtamd_bw_read_chrom(wtamd_bw *, const char *chrom, int box, int64_t capacity,
                            int32_t *start, int32_t *finish, float *value);

/* Streaming form (what wtamd_BigWiggleReader's producer thread calls): the runs of the next `max_blocks`
 * data blocks of `chrom` from index-leaf position *cursor on (0: the chromosome's beginning), skipping
 * blocks that lie wholly outside 0-based [lo0, hi0).  Returns the number of runs and advances *cursor;
 * *last = 1 when no block of the chromosome (inside the window) is left.  More runs than `capacity`:
 * nothing written, *cursor unchanged, the decoded part is kept for the repeated call. */
int64_t wtamd_bw_read_part(wtamd_bw *, const char *chrom, int box, int64_t *cursor, int max_blocks, int32_t lo0, int32_t hi0,
                           int64_t capacity, int32_t *start, int32_t *finish, float *value, int *last);

/* ---- Drop-in for the reference's src/bufferedReader.c (same five functions as src/bufferedReader.h:27-31, the
 * struct opaque and free()-able as there): the producer / consumer block buffer of the binary-file readers
 * (bigWiggleReader.c, bamReader.c, bigBedReader.c, bcfReader.c).  Link this library INSTEAD of bufferedReader.o and
 * those readers, unchanged, hand their 10 000-entry blocks to a Multiplexer of this library whole (csrc/wt_bufreader.h). */
typedef struct bufferedReaderData_st BufferedReaderData;
void launchBufferedReader(void *(*readFileFunction)(void *), void *f_data, BufferedReaderData **buf_data);
wt_bool pushValuesToBuffer(BufferedReaderData *data, const char *chrom, int start, int finish, double value);
void endBufferedSignal(BufferedReaderData *data);
void killBufferedReader(BufferedReaderData *data);
void BufferedReaderPop(WiggleIterator *wi, BufferedReaderData *data);
int compare_chrom_lengths(const void *A, const void *B);
long long wtamd_bufreader_bulk_entries(void);      /* entries taken through the bulk door so far (tests) */
/* wtamd_ArrayReader's arrays behind a reader written like the reference's binary-file readers: a producer thread pushes
 * one interval at a time (pushValuesToBuffer), pop is BufferedReaderPop -- the buffered reader's protocol with a producer
 * that costs nothing else (tests, bench leg `e2e.buffered`). */
WiggleIterator *wtamd_BufferedArrayReader(int n_chrom, const char *const *chrom_names, const int64_t *seg_off,
                                          const int32_t *start, const int32_t *finish, const float *value,
                                          double default_value);

/* ---- BigWig WRITER (bench / test plumbing next to the synthetic generator; csrc/wt_bwwrite.cpp): bedGraph sections of
 * `items_per_block` records, one zlib stream each, an R-tree index of as many levels as needed.  Chromosome names in
 * strcmp order (= their ids).  Intervals use the engine's convention: 1-based start, exclusive finish. */
typedef struct wtamd_bw_writer wtamd_bw_writer;
int wtamd_bw_writer_open(const char *path, int n_chrom, const char *const *names, const uint32_t *lengths, int items_per_block,
                         int zlib_level, wtamd_bw_writer **out);
int wtamd_bw_writer_add(wtamd_bw_writer *, int chrom, int64_t n, const int32_t *start, const int32_t *finish, const float *value);
int64_t wtamd_bw_writer_close(wtamd_bw_writer *);      /* index + header; returns the number of sections or < 0 */
/* one chromosome of many files: track i = [seg_off[i], seg_off[i + 1]) of the arrays, dealt to `threads` workers */
int wtamd_bw_writers_add_chrom(wtamd_bw_writer *const *writers, int n_tracks, int chrom, const int64_t *seg_off, const int32_t *start,
                               const int32_t *finish, const float *value, int threads);

/* ---- Synthetic workload generator of SURVEY 8d, on device (bench / test plumbing; csrc/wt_synth.hip).
 * Counter-based: position x of (chromosome c, track t) is a breakpoint iff a hash of (seed, c, t, x)
 * falls below 2^32 / mean_run, the run starting there takes value k/8 (k < levels) and its gap flag
 * from a second hash -- any piece can be regenerated anywhere (wiggletools_amd/synthgen.py holds the
 * numpy mirror the CPU baseline uses).  Two passes with the caller's exclusive scan in between:
 * plan -> count (per 4096-position block) -> scan -> fill. */
int wtamd_synth_plan(int n_chrom, const int32_t *chrom_len, int n_tracks, int64_t *n_blocks, int64_t *seg_first_block);
int wtamd_synth_count(uint64_t seed, int n_chrom, const int32_t *chrom_len, int n_tracks, double mean_run, double gap_prob,
                      int levels, int64_t *counts, void *stream);
int wtamd_synth_fill(uint64_t seed, int n_chrom, const int32_t *chrom_len, int n_tracks, double mean_run, double gap_prob,
                     int levels, const int64_t *block_off, int32_t *start, int32_t *finish, float *value, void *stream);

/* Default value a reducer iterator advertises to its parent
 * (reference reducers.c ctor of each op, incl. float truncations). HOST only. */
double wtamd_reducer_default(int op, int n_tracks, const double *defaults);

#ifdef __cplusplus
}
#endif
#endif /* WIGGLETOOLS_AMD_H_ */
