// marl_dop853_ctl.h - the scalar part of the native DOP853 loop: scipy's DOP853 (scipy/integrate/_ivp/rk.py, class DOP853: Dormand-Prince
// 8(5,3), 12 stages, no FSAL use of the error estimate) as RungeKutta._step_impl (rk.py:111-176) drives it.  The coefficient tables
// (marl_dop853_tables.h, generated from scipy's), the error norm, the accept / reject and step-factor decision, the preparation of the next
// attempt, the dense-output weights and the count of the dense output's evaluations, on the controller record the RK45 and RK23 loops use
// (Rk45Ctrl, marl_rk_ctrl.h: its layout is the C ABI's and stays what it is).  Nothing but <math.h>: a host C++ compiler builds this
// header alone (tests/test_dop853_control_cpu.py pins it to scipy's DOP853 that way); under hipcc it follows <hip/hip_runtime.h>.
//
// Against RK45 / RK23: error_estimator_order = 7, so the step factor is SAFETY err^(-1/8); an attempt costs 12 evaluations - K2..K12 and
// f(y_new), which is K13 of the dense output and K1 of the next step; the error norm combines a fifth- and a third-order estimate
// (DOP853._estimate_error_norm) and so needs TWO sums over the grid; the dense output is a polynomial of degree 7 over 16 stage
// derivatives, three of which (K14..K16) cost an evaluation each - counted by scipy, once per accepted step that builds a dense output.
#pragma once
#include <math.h>

#include "marl_rk_ctrl.h"

#ifdef __HIPCC__
#define MARL_DOP853_FN __host__ __device__ __forceinline__
#else
#define MARL_DOP853_FN inline
#endif

namespace marl {

namespace dop853 {
#define MARL_DOP853_TABLE static constexpr
#include "marl_dop853_tables.h"
#undef MARL_DOP853_TABLE
constexpr double SAFETY = 0.9, MIN_FACTOR = 0.2, MAX_FACTOR = 10.0;
constexpr double ERROR_EXPONENT = -1.0 / (7 + 1);   // -1 / (error_estimator_order + 1), rk.py:92
constexpr int NFEV_PER_ATTEMPT = 12, NFEV_DENSE = 3, N_WEIGHTS = 16;
}  // namespace dop853

// Row s (1..15) of the extended tableau as the stage loops walk it: the coefficients a_sj, j < s, of
//   stage s + 1 = f(y + h sum_j a_sj K_j)   (rk_step, rk.py:14-76; DOP853._dense_output_impl, rk.py:520-535).
// s < 12: A[s];  s = 12: B - the "stage" whose state is y_new and whose derivative is f(y_new);  s = 13..15: A_EXTRA.
MARL_DOP853_FN const double* dop853_row(int s)
{
    return s < dop853::N_STAGES ? dop853::A[s] : (s == dop853::N_STAGES ? dop853::B : dop853::A_EXTRA[s - dop853::N_STAGES - 1]);
}

// RungeKutta.__init__ (rk.py:94-102) with first_step given: f(t0, y0) is the one evaluation counted.  The monitors g are the caller's.
MARL_DOP853_FN void dop853_init(Rk45Ctrl& c, double t0, double t1, double first_step, double rtol, double atol, int64_t n_total,
                                int64_t max_attempts)
{
    c = Rk45Ctrl{};
    c.t = t0; c.t_bound = t1; c.h_abs = first_step; c.rtol = rtol; c.atol = atol;
    c.t_old = t0; c.pause_t = INFINITY;
    c.n_total = n_total; c.max_attempts = max_attempts;
    c.nfev = 1;
    c.status = (t0 == t1) ? ST_DONE : ST_RUNNING;  // base.py:189-194
}

// Top of RungeKutta._step_impl: choose the step of the next attempt (rk.py:119-142).
MARL_DOP853_FN void dop853_prepare_attempt(Rk45Ctrl& c)
{
    const double min_step = 10.0 * fabs(nextafter(c.t, INFINITY) - c.t);
    if (!c.rejected) {
        if (c.h_abs < min_step) c.h_abs = min_step;
    } else if (c.h_abs < min_step) {
        c.status = ST_TOO_SMALL;
        return;
    }
    if (c.max_attempts > 0 && c.attempts >= c.max_attempts) {
        c.status = ST_BUDGET;
        return;
    }
    double t_new = c.t + c.h_abs;
    if (t_new - c.t_bound > 0.0) t_new = c.t_bound;
    c.t_new = t_new;
    c.h_try = t_new - c.t;
    c.h_abs = fabs(c.h_try);
    c.attempts++;
}

// DOP853._estimate_error_norm (rk.py:506-518): s5 = sum (err5 / scale)^2, s3 = sum (err3 / scale)^2 over the n components, where
// err5 = sum_j E5_j K_j, err3 = sum_j E3_j K_j (no factor h) and scale = atol + rtol max(|y|, |y_new|).
MARL_DOP853_FN double dop853_error_norm(double s5, double s3, double h, double n)
{
    if (s5 == 0.0 && s3 == 0.0) return 0.0;
    const double denom = s5 + 0.01 * s3;
    return fabs(h) * s5 / sqrt(denom * n);
}

// Bottom of _step_impl (rk.py:146-165): accept / reject and the next step size from the two sums.  A NaN norm is a rejection with
// factor MIN_FACTOR.  Counts the attempt's 12 evaluations.
MARL_DOP853_FN bool dop853_decide(Rk45Ctrl& c, double s5, double s3)
{
    const double err = dop853_error_norm(s5, s3, c.h_try, (double)c.n_total);
    c.err_norm = err;
    c.nfev += dop853::NFEV_PER_ATTEMPT;
    if (err < 1.0) {
        double factor = dop853::MAX_FACTOR;
        if (err != 0.0) {
            const double f = dop853::SAFETY * pow(err, dop853::ERROR_EXPONENT);
            factor = (f < dop853::MAX_FACTOR) ? f : dop853::MAX_FACTOR;
        }
        if (c.rejected && !(factor < 1.0)) factor = 1.0;
        c.h_abs *= factor;
        c.accepted_last = 1;
        c.rejected = 0;
        c.n_acc++;
        c.t_old = c.t;
        c.h_prev = c.h_try;
        c.t = c.t_new;
        c.cur ^= 1;
        return true;
    }
    const double f = dop853::SAFETY * pow(err, dop853::ERROR_EXPONENT);
    c.h_abs *= (f > dop853::MIN_FACTOR) ? f : dop853::MIN_FACTOR;
    c.accepted_last = 0;
    c.rejected = 1;
    c.n_rej++;
    return false;
}

// After an ACCEPTED step of a run without monitor pauses: end of the interval (base.py:203-204) or the sample pause; otherwise (and
// after a rejection) the next attempt.
MARL_DOP853_FN void dop853_status_after_accept(Rk45Ctrl& c)
{
    if (c.t - c.t_bound >= 0.0) c.status = ST_DONE;
    else if (c.t >= c.pause_t) c.status = ST_PAUSED;
}

// scipy builds the dense output of an accepted step at most once - when a monitor changed sign in it (ivp.py:673-676) or a t_eval sample
// falls into it (ivp.py:706-717) - and that costs the three evaluations K14..K16 (rk.py:520-535).  The one place they are counted:
// replays and root probes recompute stages freely and count nothing.  So  nfev = 1 + 12 attempts + 3 (such steps).
MARL_DOP853_FN void dop853_count_dense_output(Rk45Ctrl& c) { c.nfev += dop853::NFEV_DENSE; }

// Dense output (Dop853DenseOutput, rk.py:577-601, built by DOP853._dense_output_impl, rk.py:520-547) written out in the K's:
//   y(t_old + x h) = y_old + h sum_j w_j(x) K_j,  j = 0..15 (K_13 = f(y_new), K_14..16 the extra stages).
// With  F0 = h sum B_j K_j,  F1 = h K_1 - F0,  F2 = 2 F0 - h (K_13 + K_1),  F3..6 = h D K,  scipy evaluates
//   x (F0 + (1-x) (F1 + x (F2 + (1-x) (F3 + x (F4 + (1-x) (F5 + x F6))))))
// = sum_i p_i(x) F_i  with  p_0 = x, p_1 = p_0 (1-x), p_2 = p_1 x, p_3 = p_2 (1-x), ...;  w_j = sum_i p_i c_ij, c_ij the coefficient of
// h K_j in F_i.  Weights are summed and F is not stored, as the RK45 and RK23 loops do it: equal to scipy up to rounding.
MARL_DOP853_FN void dop853_dense_weights(double x, double (&w)[16])
{
    double p[7];
    p[0] = x;
    for (int i = 1; i < 7; i++) p[i] = p[i - 1] * ((i & 1) ? 1.0 - x : x);
    for (int j = 0; j < 16; j++) {
        const double b = j < dop853::N_STAGES ? dop853::B[j] : 0.0;
        double a = p[0] * b;
        a += p[1] * ((j == 0 ? 1.0 : 0.0) - b);
        a += p[2] * (2.0 * b - (j == 0 ? 1.0 : 0.0) - (j == dop853::N_STAGES ? 1.0 : 0.0));
        for (int m = 0; m < 4; m++) a += p[3 + m] * dop853::D[m][j];
        w[j] = a;
    }
}

}  // namespace marl
