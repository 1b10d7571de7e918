// marl_rk23_ctl.h - the scalar part of the native RK23 loop: scipy's RK23 (scipy/integrate/_ivp/rk.py, class RK23: Bogacki-Shampine
// 3(2), FSAL) as RungeKutta._step_impl (rk.py:111-176) drives it.  The tableau, the dense-output weights, the accept / reject and
// step-factor decision and the preparation of the next attempt, on the controller record the RK45 loops use (Rk45Ctrl, marl_rk_ctrl.h:
// its layout is the C ABI's).  Nothing but <math.h>: a host C++ compiler builds this header alone (tests/test_rk23_control_cpu.py pins
// it to scipy's RK23 that way); under hipcc it follows <hip/hip_runtime.h>.
//
// Against RK45 (rk45_decide, rk45_prepare_attempt in marl_kernels.h): error_estimator_order = 2, so the step factor is
// SAFETY err^(-1/3) instead of err^(-1/5), and an attempt costs 3 evaluations instead of 6 - K2, K3 and f(y_new), which is K4 of the
// error estimate and K1 of the next step.  SAFETY, MIN_FACTOR, MAX_FACTOR and everything else of _step_impl are the same.
// The power is the caller's: pow on the host, the table-driven exp(e log x) in the kernels (marl_rk23.h).
#pragma once
#include <math.h>

#include "marl_rk_ctrl.h"

#ifdef __HIPCC__
#define MARL_RK23_FN __host__ __device__ __forceinline__
#else
#define MARL_RK23_FN inline
#endif

namespace marl {

// rk.py, class RK23: C, A, B, E, P as written there
namespace bs23 {
constexpr double C2 = 1.0 / 2, C3 = 3.0 / 4;
constexpr double A21 = 1.0 / 2;
constexpr double A31 = 0.0, A32 = 3.0 / 4;
constexpr double B1 = 2.0 / 9, B2 = 1.0 / 3, B3 = 4.0 / 9;
constexpr double E1 = 5.0 / 72, E2 = -1.0 / 12, E3 = -1.0 / 9, E4 = 1.0 / 8;
constexpr double SAFETY = 0.9, MIN_FACTOR = 0.2, MAX_FACTOR = 10.0;
constexpr double ERROR_EXPONENT = -1.0 / (2 + 1);   // -1 / (error_estimator_order + 1), rk.py:92
constexpr int N_STAGES = 3, NFEV_PER_ATTEMPT = 3, N_WEIGHTS = 4;
constexpr double P[4][3] = {{1, -4.0 / 3, 5.0 / 9}, {0, 1, -2.0 / 3}, {0, 4.0 / 3, -8.0 / 9}, {0, -1, 1}};
}  // namespace bs23

// Dense output (RkDenseOutput, rk.py:560-574): y(t_old + x h) = y_old + h sum_j w_j(x) K_j,  w_j(x) = sum_m P[j][m] x^(m+1),
// summed in the order of m as the RK45 weights are (dense_weights, marl_kernels.h).
MARL_RK23_FN void rk23_dense_weights(double x, double (&w)[4])
{
    const double pw[3] = {x, x * x, x * x * x};
    for (int j = 0; j < 4; j++) {
        double a = 0;
        for (int m = 0; m < 3; m++) a += bs23::P[j][m] * pw[m];
        w[j] = a;
    }
}

// RungeKutta.__init__ (rk.py:94-102) with first_step given: f(t0, y0) is the one evaluation counted.  The monitors g are the caller's.
MARL_RK23_FN void rk23_init(Rk45Ctrl& c, double t0, double t1, double first_step, double rtol, double atol, int64_t n_total,
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
MARL_RK23_FN void rk23_prepare_attempt(Rk45Ctrl& c)
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

// The same with the minimum-step test (10 ulp(t)) behind a cheap sufficient condition, for the controller that every wave of a
// one-workgroup sweep replicates (as rk45_prepare_attempt_lean): h_abs > |t| 2^-48 > 10 ulp(t) on every attempt of a healthy run.
MARL_RK23_FN void rk23_prepare_attempt_lean(Rk45Ctrl& c)
{
    if (!(c.h_abs > fabs(c.t) * 0x1p-48) || c.t == 0.0) {   // (t = 0: nextafter gives the smallest subnormal)
        rk23_prepare_attempt(c);
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

// rk.py:149-165 once the error norm (or anything with the same ordering against 1 and the same zero) and the raw factor
// f = SAFETY err^(-1/3) are known.  A NaN norm is a rejection with factor MIN_FACTOR.
MARL_RK23_FN bool rk23_apply_factor(Rk45Ctrl& c, bool below_one, bool is_zero, double f)
{
    c.nfev += bs23::NFEV_PER_ATTEMPT;
    if (below_one) {
        double factor = is_zero ? bs23::MAX_FACTOR : ((f < bs23::MAX_FACTOR) ? f : bs23::MAX_FACTOR);
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
    c.h_abs *= (f > bs23::MIN_FACTOR) ? f : bs23::MIN_FACTOR;
    c.accepted_last = 0;
    c.rejected = 1;
    c.n_rej++;
    return false;
}

// Bottom of _step_impl: sumsq = sum (err / scale)^2 over the n_total components -> accept / reject and the next step size.
// power(x, e) returns x^e.
template <class Pow>
MARL_RK23_FN bool rk23_decide(Rk45Ctrl& c, double sumsq, Pow&& power)
{
    const double err = sqrt(sumsq) / sqrt((double)c.n_total);  // common.py:63-65
    c.err_norm = err;
    return rk23_apply_factor(c, err < 1.0, err == 0.0, bs23::SAFETY * power(err, bs23::ERROR_EXPONENT));
}

// The same decision from the MEAN square error for the replicated controller (as rk45_decide_lean): err < 1 <=> err^2 < 1 and
// err^(-1/3) = (err^2)^(-1/6); no square roots, no division (inv_n = 1 / n_total).  c.err_norm holds err^2 until the kernel leaves.
template <class Pow>
MARL_RK23_FN bool rk23_decide_lean(Rk45Ctrl& c, double sumsq, double inv_n, Pow&& power)
{
    const double e2 = sumsq * inv_n;
    c.err_norm = e2;
    return rk23_apply_factor(c, e2 < 1.0, e2 == 0.0, bs23::SAFETY * power(e2, 0.5 * bs23::ERROR_EXPONENT));
}

// After an ACCEPTED step of a run without monitor pauses: end of the interval (base.py:203-204) or the sample pause.
MARL_RK23_FN void rk23_status_after_accept(Rk45Ctrl& c)
{
    if (c.t - c.t_bound >= 0.0) c.status = ST_DONE;
    else if (c.t >= c.pause_t) c.status = ST_PAUSED;
}

}  // namespace marl
