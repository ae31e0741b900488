// wt_abi_text.h -- part of the DROP-IN LAYER (csrc/wt_iter_abi.cpp includes it after wt_abi_runs.h): the reference's writers,
// TeeWiggleIterator, toFile and toStdout (src/wigWriter.c:261-289; `write`, `write_bg`), as wtamd_TeeWiggleIterator,
// wtamd_toFile and wtamd_toStdout.  The iterator is a ServedRuns (wt_abi_runs.h): it passes the runs it prints on, one per pop()
// and in blocks through wtamd_iterator_next_block.
//
// bedGraph mode is forced for an overlapping child; otherwise the compression rule (unaryOps.c:235-253) goes in front: a
// reducer of this library is asked for it (wtamd_iterator_compress_output) and the same rule runs on the host over every batch
// anyway, the open group carried from batch to batch -- the rule is idempotent, a group keeps its first value.  A batch is one
// block of a reducer (wtamd_iterator_next_block) or one chromosome of any other child (reg_drain_chrom: blocks from this
// library's sources, pop() otherwise).  Every batch is formatted by wtamd_runs_text_host (csrc/wt_text.hip), a wtamd_text_state
// chaining the batches; a batch with a wide value (finite, 2^64 or more), WTAMD_NO_DEVICE_TEXT=1 and a build of this layer
// without the HIP units use the host sweep, wtx_host of csrc/wt_text.h compiled here as plain C++: the same bytes.
//
// WHEN THE TEXT IS WRITTEN.  The reference's writer thread prints a block of 10000 entries when the block is full, and the
// open block at the end.  Here the text of a batch is fwritten when all of its runs have been handed on -- when the next batch
// is fetched or the child is exhausted --, except for the block the batch leaves open, which waits for its end.  SEEK: the
// reference kills its thread and loses whatever the thread had not yet printed, a race; here the complete blocks of what was
// handed on are written, the open block is dropped (what the reference does when its thread keeps up), then fflush, the child
// is sought and the entry count restarts at 0.  holdFire: nothing is written before the first seek.
#ifndef WT_ABI_TEXT_H_
#define WT_ABI_TEXT_H_

#ifndef WT_EMU
#define WT_EMU 1
#endif
#ifndef WCV_NO_HOST
#define WCV_NO_HOST 1
#endif
#include "wt_text.h"

extern "C" int wtamd_runs_text_host(int64_t n_seg, const int64_t *seg_off, const char *const *seg_name, const int32_t *start, const int32_t *finish,
                                    const double *value, uint32_t flags, wtamd_text_state *state, char *text, int64_t capacity, int64_t *n_bytes,
                                    int64_t *n_wide) __attribute__((weak));

namespace {

struct TeeIter : ServedRuns {
    WiggleIterator *child = nullptr;
    FILE *file = nullptr;
    bool bed = false, compress = false, writing = false;
    Interner names;
    // the text
    WtxState st = {0, 0, 0, 0}, st0 = {0, 0, 0, 0};       // after / before the batch being served
    const char *last_chrom = nullptr, *last_chrom0 = nullptr;   // the chromosome of the last entry formatted, likewise
    std::string open0;                  // the open block's text before the batch
    std::string full, open;             // the batch: open0 + its text up to its last block boundary (empty: it has none); the rest
    int64_t boundary = 0;               // runs of the batch up to that boundary
    std::vector<char> buf;
    // the compression rule's open group, and a drained batch that has to wait for it
    bool g_open = false;
    const char *g_chrom = nullptr;
    int32_t g_s = 0, g_f = 0;
    double g_v = 0;
    RegRuns raw;
    const char *raw_chrom = nullptr;
    bool have_raw = false;
};

[[noreturn]] void tee_refuse(const char *what) {
    fprintf(stderr, "wiggletools_amd: wtamd_TeeWiggleIterator: %s\n", what);
    exit(1);
}

// the runs [a, b) of the batch as text, appended to *txt; *st and *last move on
void tee_format(TeeIter *T, int64_t a, int64_t b, WtxState *st, const char **last, std::string *txt) {
    if (b <= a) return;
    const int64_t n = b - a, seg[2] = {0, n};
    const char *name[1] = {T->chrom};
    const uint32_t flags = T->bed ? WTX_BEDGRAPH : 0u;
    const int32_t *s = T->out.s.data() + a, *f = T->out.f.data() + a;
    const double *v = T->out.v.data() + a;
    st->continues = *last == T->chrom;
    bool device = wt_use_device((const void *) wtamd_runs_text_host, "WTAMD_NO_DEVICE_TEXT");
    int64_t cap = n * 40 + 1024, nb = 0, nw = 0;
    for (int attempt = 0;; attempt++) {
        if ((int64_t) T->buf.size() < cap) T->buf.resize((size_t) cap);
        int rc;
        if (device) {
            rc = wtamd_runs_text_host(1, seg, name, s, f, v, flags, (wtamd_text_state *) st, T->buf.data(), cap, &nb, &nw);
            if (rc == WTAMD_ERR_ARG && nw > 0) { device = false; continue; }   // a wide value: this batch on the host
            if (rc != WTAMD_OK && rc != WTAMD_ERR_ARG && rc != WTAMD_ERR_CAPACITY) die("wtamd_runs_text");
        } else {
            rc = wtx_host(1, seg, name, s, f, v, flags, st, T->buf.data(), cap, &nb, &nw);
        }
        if (rc == WTAMD_ERR_CAPACITY && attempt < 4) { cap = nb; continue; }
        if (rc != 0) tee_refuse("an interval with start >= finish, or a chromosome name outside 1 .. 255 bytes");
        break;
    }
    txt->append(T->buf.data(), (size_t) nb);
    *last = T->chrom;
}

void tee_write(TeeIter *T, const std::string &txt) {
    if (!txt.empty() && fwrite(txt.data(), 1, txt.size(), T->file) != txt.size()) tee_refuse("could not write");
}

// every run of the batch has been handed on: its text up to its last block boundary goes out, the open block waits
void tee_retire(TeeIter *T) {
    if (!T->writing) return;
    if (T->boundary > 0) { tee_write(T, T->full); T->open0.clear(); }
    T->open0 += T->open;
    T->full.clear(); T->open.clear();
    T->boundary = 0;
}

// the batch in T->out (chromosome T->chrom) becomes text, held until tee_retire
void tee_compose(TeeIter *T) {
    if (!T->writing) return;
    T->st0 = T->st; T->last_chrom0 = T->last_chrom;
    const int64_t n = (int64_t) T->out.s.size(), total = T->st.in_block + n;
    T->boundary = total >= WTX_ENTRIES ? total / WTX_ENTRIES * WTX_ENTRIES - T->st.in_block : 0;
    if (T->boundary > 0) { T->full = T->open0; tee_format(T, 0, T->boundary, &T->st, &T->last_chrom, &T->full); }
    tee_format(T, T->boundary, n, &T->st, &T->last_chrom, &T->open);
}

// the child's next batch into T->raw / T->raw_chrom; false: the child is exhausted
bool tee_drain(TeeIter *T) {
    WiggleIterator *it = T->child;
    T->raw.clear();
    if (it->pop == &red_pop) {
        const char *chrom = nullptr;
        const int32_t *s, *f;
        const double *v;
        const int64_t n = wtamd_iterator_next_block(it, &chrom, &s, &f, &v);
        if (n <= 0) return false;
        T->raw.s.assign(s, s + n); T->raw.f.assign(f, f + n); T->raw.v.assign(v, v + n);
        T->raw_chrom = T->names.get(chrom);
        return true;
    }
    if (it->done) return false;
    T->raw_chrom = T->names.get(it->chrom);
    reg_drain_chrom(it, T->raw_chrom, &T->raw);
    return true;
}

void tee_load(ServedRuns *c) {
    TeeIter *T = (TeeIter *) c;
    tee_retire(T);
    for (;;) {
        if (!T->have_raw) {
            if (!tee_drain(T)) {
                if (T->g_open) {                            // the last group
                    T->chrom = T->g_chrom;
                    T->out.push(T->g_s, T->g_f, T->g_v);
                    T->g_open = false;
                    break;
                }
                T->done = true;                             // the end: the open block is printed as well
                if (T->writing) { tee_write(T, T->open0); T->open0.clear(); fflush(T->file); }
                return;
            }
            T->have_raw = true;
        }
        if (!T->compress) {
            T->chrom = T->raw_chrom;
            std::swap(T->out, T->raw);
            T->have_raw = false;
            if (!T->out.s.empty()) break;
            continue;
        }
        if (T->g_open && T->g_chrom != T->raw_chrom) {      // the group ends with its chromosome; the batch waits
            T->chrom = T->g_chrom;
            T->out.push(T->g_s, T->g_f, T->g_v);
            T->g_open = false;
            break;
        }
        T->chrom = T->raw_chrom;
        for (size_t i = 0; i < T->raw.s.size(); i++) {      // unaryOps.c:248
            const int32_t s = T->raw.s[i], f = T->raw.f[i];
            const double v = T->raw.v[i];
            if (T->g_open && s == T->g_f && ((std::isnan(v) && std::isnan(T->g_v)) || fabs(v - T->g_v) < 0.000001)) { T->g_f = f; continue; }
            if (T->g_open) T->out.push(T->g_s, T->g_f, T->g_v);
            T->g_open = true; T->g_chrom = T->raw_chrom; T->g_s = s; T->g_f = f; T->g_v = v;
        }
        T->have_raw = false;
        if (!T->out.s.empty()) break;                       // (otherwise everything lies in the open group: more is needed)
    }
    tee_compose(T);
}

void tee_seek(WiggleIterator *wi, const char *chrom, int start, int finish) {
    TeeIter *T = (TeeIter *) wi->data;
    if (T->writing && !T->done) {
        // the complete blocks of what was handed on: the runs before the current element, and that element
        const int64_t n = (int64_t) T->out.s.size();
        const int64_t handed = T->block_out ? n : std::min(n, T->j + 1);
        const int64_t total = T->st0.in_block + handed;
        const int64_t upto = total >= WTX_ENTRIES ? total / WTX_ENTRIES * WTX_ENTRIES - T->st0.in_block : 0;
        if (upto > 0 && upto == T->boundary) tee_write(T, T->full);
        else if (upto > 0) {
            std::string txt = T->open0;
            WtxState st = T->st0;
            const char *last = T->last_chrom0;
            tee_format(T, 0, upto, &st, &last, &txt);
            tee_write(T, txt);
        }
    }
    fflush(T->file);
    T->writing = true;                                      // (holdFire: the first seek opens fire)
    T->st = T->st0 = WtxState{0, 0, 0, 0};
    T->last_chrom = T->last_chrom0 = nullptr;
    T->open0.clear(); T->full.clear(); T->open.clear();
    T->boundary = 0;
    T->g_open = false; T->have_raw = false; T->raw.clear();
    seek(T->child, chrom, start, finish);
    srv_restart(T, wi);
}

}  // namespace

extern "C" {

WiggleIterator *wtamd_TeeWiggleIterator(WiggleIterator *wi, FILE *out, wt_bool bedGraph, wt_bool holdFire) {
    TeeIter *T = new (calloc(1, sizeof(TeeIter))) TeeIter();       // free()-able, like every iterator's data
    T->load = &tee_load;
    T->child = wi;
    T->file = out;
    T->bed = bedGraph || wi->overlaps;                              // wigWriter.c:269-270
    T->compress = !bedGraph && !wi->overlaps;                       // :263-267, unaryOps.c:256-257
    T->writing = !holdFire;
    if (T->compress && wi->pop == &red_pop) (void) wtamd_iterator_compress_output(wi, 1);
    return srv_iterator(T, &tee_seek, wi->overlaps, wi->default_value);
}

static void tee_run(WiggleIterator *tee) {
    const char *chrom;
    const int32_t *s, *f;
    const double *v;
    while (srv_next_block(tee, &chrom, &s, &f, &v) > 0) { }
}

void wtamd_toFile(WiggleIterator *wi, char *filename, wt_bool bedGraph, wt_bool holdFire) {
    FILE *file = fopen(filename, "w");
    if (!file) {
        fprintf(stderr, "Could not open file %s\n", filename);      // wigWriter.c:280-283
        exit(1);
    }
    tee_run(wtamd_TeeWiggleIterator(wi, file, bedGraph, holdFire));
    fclose(file);
}

void wtamd_toStdout(WiggleIterator *wi, wt_bool bedGraph, wt_bool holdFire) {
    tee_run(wtamd_TeeWiggleIterator(wi, stdout, bedGraph, holdFire));
    fflush(stdout);
}

}  // extern "C"

#endif  // WT_ABI_TEXT_H_
