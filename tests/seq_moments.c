/* The run-by-run (sequential) f64 updates the integrators are usually compared with, compiled so that lists of 10^6 .. 10^7
 * runs cost milliseconds: tests/exact.py measures THEIR error against exact arithmetic and derives its bounds from it.
 *
 *   seq_moments   tests/test_integrator_moments.py::_sequential, operation for operation (checked bit for bit by
 *                 tests/test_side_kernels.py::test_compiled_sequential_is_the_python_one)
 *   seq_pearson   the weighted Welford step of the reference's PearsonIntegrator in its expanded form, run by run in
 *                 one pass (the form the oracle restates; the device applies the unexpanded one per slice)
 *
 * Build: gcc -O1 -std=c99 -ffp-contract=off (no fused multiply-add: the Python restatement has none). */
#include <stdint.h>

/* out5 = {T, total, count, min, max} over the runs whose value is not NaN */
void seq_moments(int64_t n, const int32_t *start, const int32_t *finish, const double *value, double *out5) {
    double T = 0, total = 0, count = 0, mn = 0, mx = 0;
    int have = 0;
    for (int64_t r = 0; r < n; r++) {
        const double x = value[r];
        if (x != x) continue;
        const double length = (double) ((int64_t) finish[r] - start[r]);
        if (count != 0) {
            const double old_mean = total / count, new_mean = total / (count + length);
            T += (old_mean * new_mean - new_mean * 2 * x + (count / (count + length)) * x * x) * length;
        }
        count += length;
        total += length * x;
        if (!have || x < mn) mn = x;
        if (!have || x > mx) mx = x;
        have = 1;
    }
    out5[0] = T; out5[1] = total; out5[2] = count;
    out5[3] = have ? mn : 0.0 / 0.0; out5[4] = have ? mx : 0.0 / 0.0;
}

/* out6 = {n, sum x, sum y, Txx, Txy, Tyy}, weights L = finish - start */
void seq_pearson(int64_t n, const int32_t *start, const int32_t *finish, const double *x, const double *y, double *out6) {
    double cnt = 0, sx = 0, sy = 0, txx = 0, txy = 0, tyy = 0;
    for (int64_t r = 0; r < n; r++) {
        const double X = x[r], Y = y[r], L = (double) ((int64_t) finish[r] - start[r]);
        if (cnt > 0) {
            const double nn = cnt + L;
            const double old_mx = sx / cnt, new_mx = sx / nn;
            const double old_my = sy / cnt, new_my = sy / nn;
            const double ratio = cnt / nn;
            txy += (new_mx * old_my + ratio * X * Y - new_mx * Y - new_my * X) * L;
            txx += (new_mx * (old_mx - 2 * X) + ratio * X * X) * L;
            tyy += (new_my * (old_my - 2 * Y) + ratio * Y * Y) * L;
        }
        cnt += L;
        sx += X * L;
        sy += Y * L;
    }
    out6[0] = cnt; out6[1] = sx; out6[2] = sy; out6[3] = txx; out6[4] = txy; out6[5] = tyy;
}
