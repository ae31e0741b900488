// wt_abi_mtext.h -- part of the DROP-IN LAYER (csrc/wt_iter_abi.cpp includes it after wt_abi_text.h): the reference's
// Multiplexer writers, TeeMultiplexer, toStdoutMultiplexer and PasteMultiplexer (src/mWigWriter.c:179-327; `mwrite`,
// `mwrite_bg`, `apply_paste`), as wtamd_TeeMultiplexer, wtamd_toStdoutMultiplexer and wtamd_PasteMultiplexer.  No un-prefixed
// name: a program may link the reference's own mWigWriter.o beside this library.
//
// The returned Multiplexer shares values / inplay / default_values with `in`; a pop copies chrom / start / finish (and
// inplay_count) and records the entry on the host -- its row of values and, for paste, the next line of `infile` read exactly
// as mWigWriter.c:97-118 reads it; it is primed by one pop.  DEPARTURE: the reference pops `in` right after it has copied the
// coordinates, so what its caller reads through the shared `values` is the NEXT entry's row beside this entry's coordinates;
// here `in` is popped at the start of the following pop, so that the struct stays coherent: the rows a caller sees are the
// rows it would see without the writer.  The file is the same either way.  It works over any `in`: this library's
// Multiplexer, wtamd_ApplyMultiplexer, wtamd_ProfileMultiplexer, a foreign one.  THE TILE STILL COMES HOME here, because the
// callers of this API read the struct after every pop; the path on which it never leaves HBM is wtamd_trackset_mtext.
//
// Complete blocks of 10000 entries are formatted by wtamd_tile_text_host (csrc/wt_mtext.hip), several blocks per call -- about
// four million cells --, and written with fwrite; the open block is written at the end.  Every call starts at a block
// boundary, so no state has to be chained.  WTAMD_NO_DEVICE_MTEXT=1, a batch with a wide value (finite, 2^64 or more) and a
// build of this layer without the HIP units use the host sweep, wtm_host of csrc/wt_mtext.h compiled here as plain C++: the
// same bytes.  SEEK and holdFire follow wt_abi_text.h's policy: the complete blocks of what was handed on are written, the
// open block is dropped, then fflush, `in` is sought, the entry count restarts at 0 and the Multiplexer is primed again;
// holdFire: nothing is recorded or written before the first seek.  An infile that runs out of lines: the entries before it are
// written, then the reference's message and exit(1).  Departure: without a writer the reference's pop never sets `done`
// (mWigWriter.c:216); this one does.
#ifndef WT_ABI_MTEXT_H_
#define WT_ABI_MTEXT_H_

#include "wt_mtext.h"

extern "C" int wtamd_tile_text_host(int64_t n_seg, const int64_t *seg_off, const char *const *seg_name, const int32_t *start, const int32_t *finish,
                                    const double *values, int32_t width, const char *prefix, const int64_t *prefix_off, uint32_t flags,
                                    wtamd_text_state *state, char *text, int64_t capacity, int64_t *n_bytes, int64_t *n_wide) __attribute__((weak));

namespace {

struct MTee {
    Multiplexer *in = nullptr;
    FILE *infile = nullptr, *outfile = nullptr;
    bool bed = false, writing = false;
    bool fresh = true;                  // `in` was primed or sought and stands on an entry this Multiplexer has not shown yet
    Interner names;
    // the entries recorded and not yet written
    std::vector<const char *> chrom;
    std::vector<int32_t> s, f;
    std::vector<double> vals;
    std::string prefix;
    std::vector<int64_t> poff;
    std::vector<char> buf;
};

[[noreturn]] void mtee_refuse(const char *what) {
    fprintf(stderr, "wiggletools_amd: wtamd_TeeMultiplexer: %s\n", what);
    exit(1);
}

int64_t mtee_blocks_per_call(int width) {
    const int64_t b = 4000000 / ((int64_t) WTX_ENTRIES * width);
    return b < 1 ? 1 : b > 16 ? 16 : b;
}

// the first n recorded entries (n a multiple of 10000, or all of them) as text into the file; they are forgotten
void mtee_write(MTee *T, Multiplexer *m, int64_t n) {
    if (n <= 0) return;
    const int width = m->count;
    std::vector<int64_t> seg(1, 0);
    std::vector<const char *> name;
    for (int64_t i = 0; i < n; i++) {
        if (i == 0 || T->chrom[(size_t) i] != T->chrom[(size_t) i - 1]) { if (i) seg.push_back(i); name.push_back(T->chrom[(size_t) i]); }
    }
    seg.push_back(n);
    const bool paste = T->infile != nullptr;
    const char *pre = paste ? T->prefix.data() : nullptr;
    const int64_t *poff = paste ? T->poff.data() : nullptr;
    const uint32_t flags = T->bed ? WTX_BEDGRAPH : 0u;
    bool device = wt_use_device((const void *) wtamd_tile_text_host, "WTAMD_NO_DEVICE_MTEXT");
    int64_t cap = n * ((int64_t) width * 12 + 40) + (paste ? T->poff[(size_t) n] - T->poff[0] : 0) + 1024, nb = 0, nw = 0;
    for (int attempt = 0;; attempt++) {
        if ((int64_t) T->buf.size() < cap) T->buf.resize((size_t) cap);
        int rc;
        if (device) {
            rc = wtamd_tile_text_host((int64_t) name.size(), seg.data(), name.data(), T->s.data(), T->f.data(), T->vals.data(), width, pre, poff, flags, nullptr,
                                      T->buf.data(), cap, &nb, &nw);
            if (rc == WTAMD_ERR_ARG && nw > 0) { device = false; continue; }   // a wide value: this batch on the host
            if (rc != WTAMD_OK && rc != WTAMD_ERR_ARG && rc != WTAMD_ERR_CAPACITY) die("wtamd_tile_text");
        } else {
            rc = wtm_host((long long) name.size(), seg.data(), name.data(), T->s.data(), T->f.data(), T->vals.data(), width, pre, poff, flags, nullptr,
                          T->buf.data(), cap, &nb, &nw);
        }
        if (rc == WTAMD_ERR_CAPACITY && attempt < 4) { cap = nb; continue; }
        if (rc != 0) mtee_refuse("an entry with start >= finish, a chromosome name outside 1 .. 255 bytes, or more columns than WTAMD_MTEXT_MAX_WIDTH");
        break;
    }
    if (nb > 0 && fwrite(T->buf.data(), 1, (size_t) nb, T->outfile) != (size_t) nb) mtee_refuse("could not write");
    T->chrom.erase(T->chrom.begin(), T->chrom.begin() + n);
    T->s.erase(T->s.begin(), T->s.begin() + n);
    T->f.erase(T->f.begin(), T->f.begin() + n);
    T->vals.erase(T->vals.begin(), T->vals.begin() + n * width);
    if (paste) {
        const int64_t cut = T->poff[(size_t) n];
        T->prefix.erase(0, (size_t) cut);
        T->poff.erase(T->poff.begin(), T->poff.begin() + n);
        for (int64_t &o : T->poff) o -= cut;
    }
}

void mtee_forget(MTee *T) {
    T->chrom.clear(); T->s.clear(); T->f.clear(); T->vals.clear(); T->prefix.clear();
    T->poff.assign(1, 0);
}

// the next line of the infile as the entry's prefix (mWigWriter.c:97-118)
void mtee_paste_line(MTee *T, Multiplexer *m) {
    char buffer[5000];
    do {
        if (!fgets(buffer, 5000, T->infile)) {
            mtee_write(T, m, (int64_t) T->s.size());            // (what the reference printed before it found the file short)
            fflush(T->outfile);
            fprintf(stderr, "Could not paste data to file lines, inconsistent number of lines.\n");
            exit(1);
        }
    } while (!(strlen(buffer) && strncmp(buffer, "track", 5) && strncmp(buffer, "browser", 7)));
    for (int k = (int) strlen(buffer) - 1; k >= 0; k--) {
        if (buffer[k] == '\n' || buffer[k] == '\r') buffer[k] = '\0';
        else break;
    }
    T->prefix += buffer;
    T->poff.push_back((int64_t) T->prefix.size());
}

void mtee_pop(Multiplexer *m) {
    MTee *T = (MTee *) m->data;
    Multiplexer *in = T->in;
    if (!T->fresh) popMultiplexer(in);                          // (`in` stands on the entry this Multiplexer shows: see the header)
    T->fresh = false;
    if (in->done) {
        if (T->writing) { mtee_write(T, m, (int64_t) T->s.size()); fflush(T->outfile); }
        m->done = 1;
        return;
    }
    m->chrom = in->chrom; m->start = in->start; m->finish = in->finish; m->inplay_count = in->inplay_count;
    if (T->writing) {
        if (T->infile) mtee_paste_line(T, m);
        T->chrom.push_back(T->names.get(in->chrom));
        T->s.push_back(in->start); T->f.push_back(in->finish);
        T->vals.insert(T->vals.end(), in->values, in->values + m->count);
        const int64_t full = mtee_blocks_per_call(m->count) * WTX_ENTRIES;
        if ((int64_t) T->s.size() >= full) mtee_write(T, m, full);
    }
}

void mtee_seek(Multiplexer *m, const char *chrom, int start, int finish) {
    MTee *T = (MTee *) m->data;
    if (T->writing) mtee_write(T, m, (int64_t) T->s.size() / WTX_ENTRIES * WTX_ENTRIES);
    mtee_forget(T);
    fflush(T->outfile);
    T->writing = true;                                          // (holdFire: the first seek opens fire)
    seekMultiplexer(T->in, chrom, start, finish);
    T->fresh = true;
    m->done = 0;
    popMultiplexer(m);
}

Multiplexer *mtee_new(Multiplexer *in, FILE *infile, FILE *outfile, bool bed, bool holdFire) {
    if (in->count < 1 || in->count > WTM_MAX_WIDTH) mtee_refuse("more columns than WTAMD_MTEXT_MAX_WIDTH, or none");
    MTee *T = new MTee();
    T->in = in; T->infile = infile; T->outfile = outfile;
    T->bed = bed; T->writing = !holdFire;
    T->poff.assign(1, 0);
    Multiplexer *m = newCoreMultiplexer(T, in->count, &mtee_pop, &mtee_seek);
    free(m->values); free(m->inplay); free(m->default_values);
    m->values = in->values; m->inplay = in->inplay; m->default_values = in->default_values;     // mWigWriter.c:296-298
    m->strict = in->strict;
    popMultiplexer(m);
    return m;
}

}  // namespace

extern "C" {

Multiplexer *wtamd_TeeMultiplexer(Multiplexer *in, FILE *outfile, wt_bool bedGraph, wt_bool holdFire) {
    return mtee_new(in, nullptr, outfile, bedGraph != 0, holdFire != 0);
}

void wtamd_toStdoutMultiplexer(Multiplexer *in, wt_bool bedGraph, wt_bool holdFire) {
    runMultiplexer(mtee_new(in, nullptr, stdout, bedGraph != 0, holdFire != 0));
    fflush(stdout);
}

Multiplexer *wtamd_PasteMultiplexer(Multiplexer *in, FILE *infile, FILE *outfile, wt_bool holdFire) {
    return mtee_new(in, infile, outfile, true, holdFire != 0);                                  // mWigWriter.c:315
}

}  // extern "C"

#endif  // WT_ABI_MTEXT_H_
