// wt_inflate_emu.h -- TEST INFRASTRUCTURE ONLY: one zlib (or raw deflate) stream through the lane state machine of
// csrc/wt_inflate.h on the host, as one lane of the inflate kernel runs it.  Shared by the emulated pipeline
// (wt_pipe_emu.cpp) and the variant builds of the state machine (wt_inflate_variant.cpp).
#ifndef WT_INFLATE_EMU_H_
#define WT_INFLATE_EMU_H_

#include <cstdint>
#include <cstring>
#include <vector>

#include "../../wiggletools_amd/csrc/wt_inflate.h"

// Returns bytes produced or -(error).
template <int RING>
static long long emu_inflate_ring(const uint8_t *src, long long n, uint8_t *dst, long long cap, int raw_deflate, long long *steps, uint32_t *end_byte = nullptr) {
    std::vector<uint8_t> perm(WT_INF_PERM + 8, 0);
    std::vector<uint32_t> ring(RING, 0);
    WtInfMem m{perm.data(), ring.data(), 1};
    // the decoder reads whole aligned 16-byte chunks around the stream and writes whole words: private padded copies
    std::vector<uint8_t> in((size_t) n + 96, 0), out(((size_t) cap + 3) / 4 * 4 + 8, 0);
    const int mis = (int) (n % 16);             // any alignment must work
    if (n > 0) memcpy(in.data() + 32 + mis, src, (size_t) n);
    WtInflateT<RING> z;
    wt_inf_begin(z, in.data() + 32 + mis, (uint32_t) n, out.data(), (uint32_t) cap, raw_deflate != 0);
    long long rounds = 0;
    while (wt_inf_land(z, m)) {
        for (int r = 0; r < WT_INF_ROUND; r++) wt_inf_step(z, m);
        rounds++;
    }
    if (steps) *steps = rounds * WT_INF_ROUND;
    const long long r = (long long) wt_inf_finish(z);
    if (end_byte) *end_byte = wt_inf_end_byte(z);
    if (r > 0) memcpy(dst, out.data(), (size_t) r);
    return r;
}

#endif  // WT_INFLATE_EMU_H_
