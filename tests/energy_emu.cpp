// energy_emu.cpp -- the energy passes of csrc/wt_energy.h on the CPU (test infrastructure of tests/test_energy_emu.py and
// tests/test_energy_mod.py).  The header is compiled with -DWT_EMU: a pass is a function of (arguments, workgroup index), and the
// launcher of tests/emu/runs_launcher.h runs the workgroups of every pass one after the other, forwards, backwards or shuffled.
// The door is the product's own template over this launcher; energy_host is the product's host sweep; energy_mod_check holds
// the product's phase reduction against 128-bit integer arithmetic.
#define WT_EMU 1
#include "emu/runs_launcher.h"
#include "../wiggletools_amd/csrc/wt_energy.h"

namespace {

struct EnergyLauncher : CpuLauncher {
    using CpuLauncher::CpuLauncher;
    bool run_energy(int kernel, long long blocks, const WenArgs &a) { return run_blocks<WenLds>(wen_run_block, kernel, blocks, a); }
};

}  // namespace

extern "C" {

int energy_emu_door(int order, uint64_t seed, int64_t n_seg, const int64_t *seg_off, const int64_t *seg_base, const int32_t *start, const int32_t *finish,
                    const void *value, int value_is_f64, int32_t n_lam, const int32_t *wavelength, double *reim, int64_t *end_base, int64_t *launches) {
    EnergyLauncher l(order, seed);
    const char *why = "";
    const int rc = wen_door(l, (long long) n_seg, seg_off, seg_base, start, finish, value, value_is_f64, (int) n_lam, wavelength, reim, end_base, &why);
    if (launches) *launches = l.launches;
    return rc;
}

int energy_host(int64_t n_seg, const int64_t *seg_off, const int64_t *seg_base, const int32_t *start, const int32_t *finish, const double *value,
                int32_t n_lam, const int32_t *wavelength, double *reim, int64_t *end_base) {
    return wen_host((long long) n_seg, seg_off, seg_base, start, finish, value, (int) n_lam, wavelength, reim, end_base);
}

// m and q of the runs (base[i], start[i], finish[i]) at wavelength lam by the product's reduction (wen_bm, wen_phase over the
// host-made table) against (2 (base + start) + L - 1) mod 2 lam and L mod 2 lam in 128-bit integers: the mismatches.
int64_t energy_mod_check(int32_t lam, int64_t n, const int64_t *base, const int32_t *start, const int32_t *finish) {
    std::vector<WenLam> tab;
    wen_table(1, &lam, &tab);
    const __int128 d = 2 * (__int128) lam;
    int64_t wrong = 0;
    for (int64_t i = 0; i < n; i++) {
        unsigned int m, q;
        wen_phase(tab[0], wen_bm(base[i], tab[0].lam), start[i], finish[i], &m, &q);
        const __int128 len = (__int128) finish[i] - start[i];
        __int128 mm = (2 * ((__int128) base[i] + start[i]) + len - 1) % d;
        if (mm < 0) mm += d;
        if ((__int128) m != mm || (__int128) q != len % d) wrong++;
    }
    return wrong;
}

// wen_mod alone over raw numerators below 2^35: the mismatches
int64_t energy_rawmod_check(int32_t lam, int64_t n, const uint64_t *x) {
    std::vector<WenLam> tab;
    wen_table(1, &lam, &tab);
    int64_t wrong = 0;
    for (int64_t i = 0; i < n; i++) wrong += wen_mod(x[i], tab[0].d, tab[0].inv_d) != (unsigned int) (x[i] % tab[0].d);
    return wrong;
}

}  // extern "C"
