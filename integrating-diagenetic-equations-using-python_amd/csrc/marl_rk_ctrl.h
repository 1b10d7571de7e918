// marl_rk_ctrl.h - the step controller record of the explicit adaptive Runge-Kutta loops (RK45, RK23, DOP853) and their status codes.
// Plain data and nothing but <stdint.h>: marl_kernels.h (device) and marl_rk23_ctl.h / marl_dop853_ctl.h (host-compilable) share it.
#pragma once
#include <stdint.h>

namespace marl {

// (ST_TERMINAL: a terminal monitor ended the run, marl_set_terminal - marl_stats.status = 1, scipy's code, which ST_RUNNING occupies here)
enum : int { ST_DONE = 0, ST_RUNNING = 1, ST_BUDGET = 2, ST_PAUSED = 3, ST_TERMINAL = 4, ST_TOO_SMALL = -1 };

// Device-resident step controller: the scalar state of scipy's RungeKutta._step_impl
// (rk.py:111-176) plus the driver's event bookkeeping (ivp.py:673-694).  One per instance.
// Plain data; its layout is pinned by the ctypes mirror of tests/test_rk23_control_cpu.py.
struct Rk45Ctrl {
    double t, h_abs, t_bound, rtol, atol;
    double h_try, t_new;     // the attempt in flight (h_try = t_new - t, clipped at t_bound)
    double t_old, h_prev;    // last accepted step [t_old, t_old + h_prev] (dense output)
    double err_norm;         // error norm of the last attempt
    double pause_t;          // pause (ST_PAUSED) after the accepted step that reaches this time; +inf = never
    double g[7];             // monitors at the last accepted state (ivp.py:645, :694)
    double ev_first[7];      // first / latest sign change per monitor, located by linear interpolation
    double ev_last[7];       //   inside the bracketing step (the host refines with dense output + Brent)
    int64_t n_events[7];
    int64_t nfev, n_acc, n_rej, attempts, max_attempts;
    int64_t n_total;         // 5 * N of the global grid: size of the RMS norm (common.py:63-65)
    int32_t status;          // ST_*
    int32_t cur;             // which of the two state / FSAL buffers holds (y, f) at time t
    int32_t rejected;        // a rejection happened in the step in progress (rk.py:128,163-165)
    int32_t accepted_last;   // the last attempt was accepted
    int32_t pause_on_event;  // pause after an accepted step in which a monitor changed sign
    int32_t event_fired;     // set with ST_PAUSED when that was the reason
};

}  // namespace marl
