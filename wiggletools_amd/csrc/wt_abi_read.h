// wt_abi_read.h -- part of the DROP-IN LAYER (csrc/wt_iter_abi.cpp includes it after wt_abi_runs.h): the reference's text readers,
// WiggleReader (src/wigReader.c) and BedReader (src/bedReader.c), as wtamd_WiggleReader and wtamd_BedReader.  Both are ServedRuns
// (wt_abi_runs.h): bulk sources to this library's Multiplexer and to wtamd_iterator_next_block, one run per pop() to anything else.
//
// The file is read in chunks cut at the last newline (WTAMD_READ_CHUNK_MB, default 64; WTAMD_READ_CHUNK_BYTES for tests) and
// every chunk goes through wtamd_text_runs_host (csrc/wt_read.hip), a wtamd_read_state chaining them.  With
// WTAMD_NO_DEVICE_READ=1, in a build of this layer without the HIP units, and from the first chunk the door refuses on (an
// irregular line, an unsorted BED record), the lines go through WtrRefReader of csrc/wt_read.h, compiled here as plain C++: the
// reference's own sscanf / strtok reading with its messages and exit(1), continuing from the door's state.
//
// Behind the raw records: the seek window (wigReader.c:192-203, bedReader.c:70-81), and for the wig reader the compression rule
// (unaryOps.c:235-253) with its group carried across chunks.  SEEK follows WiggleReaderSeek / BedReaderSeek under the
// compression iterator's seek.  The reference's reader stands one raw record ahead of what its consumer holds; the file is
// reopened, the raw records already consumed are passed over, and that record decides as it does there: a seek backwards (or
// after the end) starts again from the top, a seek forwards goes on from it; then records before the window are skipped, the
// first start is clipped, the stop clips the last finish and ends the iterator.  "-" reads stdin forwards; a seek on it cannot
// reopen and ends as the reference's failed fopen does.
#ifndef WT_ABI_READ_H_
#define WT_ABI_READ_H_

#ifndef WT_EMU
#define WT_EMU 1
#endif
#ifndef WCV_NO_HOST
#define WCV_NO_HOST 1
#endif
#include "wt_read.h"

extern "C" int wtamd_text_runs_host(const char *text, int64_t n_bytes, uint32_t flags, wtamd_read_state *state, int32_t *start, int32_t *finish,
                                    double *value, int64_t capacity, int64_t *seg_off, int64_t *seg_name_off, int32_t *seg_name_len,
                                    int64_t seg_capacity, char *seg_name, int64_t seg_name_cap, wtamd_read_counts *counts) __attribute__((weak));

namespace {

struct ReadIter : ServedRuns {
    std::string path;
    FILE *file = nullptr;
    bool bed = false, host = false, at_eof = false;
    Interner names;
    WtrState st;
    WtrRefReader ref;
    std::string carry;                          // the bytes after the last newline of the chunk before
    // raw records read and not yet taken
    std::vector<const char *> r_name;
    RegRuns raw;
    size_t r_at = 0;
    int64_t n_raw = 0;                          // raw records taken since the file was opened
    int32_t last_f = 0;
    double last_v = 1;
    // the seek window
    std::string w_chrom;
    int w_stop = -1;
    bool ended = false;                         // a record beyond the window was met
    // the compression rule's open group; what it has let go: (name, run, raw records in it)
    bool g_open = false;
    const char *g_chrom = nullptr;
    int32_t g_s = 0, g_f = 0;
    double g_v = 0;
    int64_t g_n = 0;
    std::vector<const char *> p_name;
    RegRuns pend;
    std::vector<int64_t> p_cnt;
    size_t p_at = 0;
    // raw records in the runs handed to `out` before the batch being served, and per run of the batch
    int64_t consumed = 0;
    std::vector<int64_t> out_cnt;
};

size_t read_chunk_bytes() {
    if (const char *e = getenv("WTAMD_READ_CHUNK_BYTES")) { const long long v = atoll(e); if (v > 0) return (size_t) v; }
    const char *e = getenv("WTAMD_READ_CHUNK_MB");
    const long long mb = e ? atoll(e) : 64;
    return (size_t) (mb > 0 ? mb : 64) << 20;
}

void read_open(ReadIter *R) {
    if (R->path == "-") { R->file = stdin; return; }
    if (!(R->file = fopen(R->path.c_str(), "r"))) {
        fprintf(stderr, R->bed ? "Could not open bed file %s\n" : "Could not open input file %s\n", R->path.c_str());
        exit(1);
    }
}

void read_reset(ReadIter *R) {
    memset(&R->st, 0, sizeof R->st);
    R->ref = WtrRefReader();
    R->ref.bed = R->bed; R->ref.filename = R->path;
    const char *e = getenv("WTAMD_NO_DEVICE_READ");
    R->host = wtamd_text_runs_host == nullptr || (e && atoi(e) != 0);
    R->at_eof = false; R->ended = false;
    R->carry.clear();
    R->r_name.clear(); R->raw.clear(); R->r_at = 0; R->n_raw = 0;
    R->last_f = 0; R->last_v = 1;
    R->g_open = false; R->g_n = 0;
    R->p_name.clear(); R->pend.clear(); R->p_cnt.clear(); R->p_at = 0;
    R->consumed = 0; R->out_cnt.clear();
}

void read_push_raw(ReadIter *R, const char *name, int32_t s, int32_t f, double v) {
    R->r_name.push_back(name); R->raw.push(s, f, v);
    R->last_f = f; R->last_v = v;
}

// the lines [p, e) the reference's way
void read_lines_host(ReadIter *R, const char *p, const char *e) {
    wtr_ref_pieces(p, e, [R](char *ln) {
        if (R->ref.line(ln)) read_push_raw(R, R->names.get(R->ref.chrom.c_str()), R->ref.start, R->ref.finish, R->ref.value);
    });
}

// one more chunk of the file into the raw records; false: the file has ended
bool read_fill(ReadIter *R) {
    if (R->at_eof || !R->file) return false;
    if (R->r_at > 0 && R->r_at == R->r_name.size()) { R->r_name.clear(); R->raw.clear(); R->r_at = 0; }
    std::string text = std::move(R->carry);
    R->carry.clear();
    const size_t want = read_chunk_bytes();
    size_t cut = std::string::npos;
    while (true) {
        const size_t old = text.size();
        text.resize(old + want);
        const size_t got = fread(&text[old], 1, want, R->file);
        text.resize(old + got);
        if (got < want) { R->at_eof = true; break; }
        cut = text.rfind('\n');
        if (cut != std::string::npos) break;    // (a chunk without a newline grows until it has one)
    }
    if (R->at_eof) {
        if (R->file != stdin) fclose(R->file);
        R->file = nullptr;
    } else {
        R->carry.assign(text, cut + 1, std::string::npos);
        text.resize(cut + 1);
    }
    if (text.empty()) return !R->at_eof;
    if (!R->host) {
        const uint32_t flags = (R->bed ? WTR_BED : 0u) | (text.back() != '\n' ? WTR_EOF : 0u);
        int64_t cap = 0;
        for (char c : text) cap += c == '\n';
        cap += 1;
        std::vector<int32_t> s((size_t) cap), f((size_t) cap), nl((size_t) cap);
        std::vector<double> v((size_t) cap);
        std::vector<int64_t> so((size_t) cap + 1), no((size_t) cap);
        std::vector<char> nm(text.size() + 2 * 257 + (size_t) cap);
        WtrState st = R->st;
        wtamd_read_counts cn;
        const int rc = wtamd_text_runs_host(text.data(), (int64_t) text.size(), flags, (wtamd_read_state *) &st, s.data(), f.data(), v.data(), cap, so.data(),
                                            no.data(), nl.data(), cap, nm.data(), (int64_t) nm.size(), &cn);
        if (rc == WTAMD_OK) {
            const char *p = nm.data();
            for (int64_t g = 0; g < cn.n_seg; g++) {
                const char *name = R->names.get(p);
                for (int64_t i = so[(size_t) g]; i < so[(size_t) g + 1]; i++) read_push_raw(R, name, s[(size_t) i], f[(size_t) i], v[(size_t) i]);
                p += nl[(size_t) g] + 1;
            }
            R->st = st;
            return true;
        }
        if (rc != WTAMD_ERR_ARG) die("wtamd_text_runs_host");
        // refused (an irregular line, an unsorted BED record): this chunk and the rest of the file as the reference reads them
        R->host = true;
        R->ref.resume(R->st, R->bed, R->last_f, R->last_v);
        R->ref.filename = R->path;
    }
    read_lines_host(R, text.data(), text.data() + text.size());
    return true;
}

// the next raw record behind the seek window: false at the end (of the file or of the window)
bool read_next_raw(ReadIter *R, const char **name, int32_t *s, int32_t *f, double *v) {
    if (R->ended) return false;
    while (R->r_at >= R->r_name.size()) if (!read_fill(R)) return false;
    *name = R->r_name[R->r_at]; *s = R->raw.s[R->r_at]; *f = R->raw.f[R->r_at]; *v = R->raw.v[R->r_at];
    R->r_at++;
    R->n_raw++;
    if (R->w_stop > 0) {
        const int d = strcmp(*name, R->w_chrom.c_str());
        if (d > 0 || (d == 0 && *s >= R->w_stop)) { R->ended = true; return false; }
        if (d == 0 && *f > R->w_stop) *f = R->w_stop;
    }
    return true;
}

void read_let_go(ReadIter *R) {
    if (!R->g_open) return;
    R->p_name.push_back(R->g_chrom); R->pend.push(R->g_s, R->g_f, R->g_v); R->p_cnt.push_back(R->g_n);
    R->g_open = false;
}

// one raw record through the compression rule (the BED reader: as it is)
void read_take(ReadIter *R, const char *name, int32_t s, int32_t f, double v) {
    if (!R->bed && R->g_open && name == R->g_chrom && s == R->g_f && ((v != v && R->g_v != R->g_v) || fabs(v - R->g_v) < 0.000001)) {
        R->g_f = f; R->g_n++;
        return;
    }
    read_let_go(R);
    R->g_open = true; R->g_chrom = name; R->g_s = s; R->g_f = f; R->g_v = v; R->g_n = 1;
    if (R->bed) read_let_go(R);
}

void read_load(ServedRuns *c) {
    ReadIter *R = (ReadIter *) c;
    for (int64_t k : R->out_cnt) R->consumed += k;
    R->out_cnt.clear();
    if (R->p_at > 0 && R->p_at == R->p_name.size()) { R->p_name.clear(); R->pend.clear(); R->p_cnt.clear(); R->p_at = 0; }
    // until the rule has let a run go; then whatever raw records are at hand, but no further chunk
    for (;;) {
        if (R->p_at < R->p_name.size() && R->r_at >= R->r_name.size()) break;
        const char *name; int32_t s, f; double v;
        if (!read_next_raw(R, &name, &s, &f, &v)) { read_let_go(R); break; }
        read_take(R, name, s, f, v);
    }
    if (R->p_at >= R->p_name.size()) { c->done = true; return; }
    c->chrom = R->p_name[R->p_at];
    while (R->p_at < R->p_name.size() && R->p_name[R->p_at] == c->chrom) {
        c->out.push(R->pend.s[R->p_at], R->pend.f[R->p_at], R->pend.v[R->p_at]);
        R->out_cnt.push_back(R->p_cnt[R->p_at]);
        R->p_at++;
    }
}

void read_seek(WiggleIterator *wi, const char *chrom, int start, int finish) {
    ReadIter *R = (ReadIter *) wi->data;
    if (R->path == "-") { fprintf(stderr, R->bed ? "Could not open input file %s\n" : "Cannot open input file %s\n", R->path.c_str()); exit(1); }
    // raw records in what the consumer has been given, the current element included
    int64_t used = R->consumed;
    if (!R->done && !R->block_out) for (int64_t q = 0; q <= R->j && q < (int64_t) R->out_cnt.size(); q++) used += R->out_cnt[(size_t) q];
    else for (int64_t k : R->out_cnt) used += k;
    const std::string target = chrom;
    for (int attempt = 0; attempt < 2; attempt++) {
        if (R->file && R->file != stdin) fclose(R->file);
        read_reset(R);
        read_open(R);
        R->w_chrom.clear(); R->w_stop = -1;
        const char *name = nullptr; int32_t s = 0, f = 0; double v = 0;
        bool have = true;
        for (int64_t k = 0; k <= used && have; k++) have = read_next_raw(R, &name, &s, &f, &v);      // the reader's own record is the last of these
        const bool back = !have || strcmp(target.c_str(), name) < 0 || (strcmp(target.c_str(), name) == 0 && start < s);
        if (attempt == 0 && back && used > 0) { used = 0; continue; }      // again from the top
        R->w_chrom = target; R->w_stop = finish;
        if (!have) break;
        R->r_at--; R->n_raw--;                  // (that record again, now behind the window)
        while (read_next_raw(R, &name, &s, &f, &v)) {
            const int d = strcmp(name, target.c_str());
            if (d < 0 || (d == 0 && (R->bed ? f < start : f <= start))) continue;
            if (d == 0 && s < start) s = start;
            R->consumed = R->n_raw - 1;
            read_take(R, name, s, f, v);
            break;
        }
        break;
    }
    srv_restart(R, wi);
}

WiggleIterator *read_new(const char *path, bool bed) {
    ReadIter *R = new ReadIter();
    R->path = path; R->bed = bed;
    R->load = &read_load;
    read_reset(R);
    read_open(R);
    return srv_iterator(R, &read_seek, bed, 0.0);
}

}  // namespace

extern "C" {

WiggleIterator *wtamd_WiggleReader(char *path) { return read_new(path, false); }
WiggleIterator *wtamd_BedReader(char *path) { return read_new(path, true); }

}  // extern "C"

#endif  // WT_ABI_READ_H_
