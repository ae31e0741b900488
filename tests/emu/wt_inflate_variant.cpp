// wt_inflate_variant.cpp -- TEST INFRASTRUCTURE ONLY: the lane state machine of csrc/wt_inflate.h alone, for builds
// with compile-time switches that are not the default (-DWT_INF_ROUND=3, -DWT_INF_LEAD=0, ...): tests/emu/build.py
// build_inflate_variant, tests/test_bwdev_streams.py.
#include "wt_inflate_emu.h"

extern "C" {
long long wtemu_inflate(const uint8_t *src, long long n, uint8_t *dst, long long cap, int raw_deflate) {
    return emu_inflate_ring<WT_INF_RING>(src, n, dst, cap, raw_deflate, nullptr);
}

long long wtemu_inflate_ring(const uint8_t *src, long long n, uint8_t *dst, long long cap, int raw_deflate, int ring, long long *steps) {
    if (ring == 64) return emu_inflate_ring<64>(src, n, dst, cap, raw_deflate, steps);
    return emu_inflate_ring<8>(src, n, dst, cap, raw_deflate, steps);
}
}  // extern "C"
