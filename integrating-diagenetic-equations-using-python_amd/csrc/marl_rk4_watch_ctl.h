// marl_rk4_watch_ctl.h - the scalar side of the monitored fixed-step RK4 loop (marl_rk4_watch.h; host driver: marl_api.hip): the
// per-instance record, the step epilogue that ONE lane of the workgroup runs after every step, and the host's check of the frame
// list.  Kernel and host use the SAME functions.  Nothing but <stdint.h>: a host C++ compiler builds this header alone
// (tests/test_rk4_watch_control_cpu.py pins it to a Python restatement, tests/rk4_watch_ref.py, that way).
//
// The rules (the fixed-step counterpart of what the adaptive sweeps do):
//   * step s (0-based) goes from t0 + s dt to t0 + (s + 1) dt; times are formed by that multiplication, never accumulated;
//   * after a step the reduction record of the new state arrives: slot 0 counts the cells with a non-finite field, slots 1..7 are the
//     monitor extrema in the order of monitors_kernel; monitor e is read from it by rk45_monitor_of_record's slot map;
//   * a non-zero (or NaN) slot 0 ends the instance at once with RK4W_NONFINITE: no monitor is processed for that step (g keeps the
//     monitors of the last finite state), no frame is written at it, the counters include it;
//   * a sign change is rk45_event_one's:  go <= 0 && gn >= 0  or the reverse; its time is  t_s + dt (go / (go - gn)),  and t_(s+1)
//     when go == gn.  There is NO dense output and NO Brent: a fixed step takes no partial steps, and this secant estimate is O(dt^2)
//     away from the root of the solution's monitor.  n_events[e] counts every occurrence; the time is stored while a slot is free
//     (max_events per monitor) and only when the caller passed a buffer;
//   * terminal monitors (marl_set_terminal's limits k[e]): the run ends at the END of the step in which monitor e has its k[e]-th
//     occurrence - RK4W_TERMINAL, t = that step's end, the state that step's result, NOT interpolated to the root (a deliberate
//     difference from marl_terminal.h's rule, which cuts the step at the root: there is no dense output to cut it with).  All sign
//     changes of that step are counted and stored;
//   * frame j is the state after frame_steps[j] steps (strictly ascending, in [0, nsteps]; 0 is the initial state); a frame due at a
//     terminal step is written.
// The epilogue's floating-point expressions are kept uncontracted (no fused multiply-add), so that the kernel, a host build of this
// header and the Python restatement form the same numbers.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define MARL_RK4W_FN __host__ __device__ __forceinline__
#else
#define MARL_RK4W_FN inline
#endif
#if defined(__clang__)
#define MARL_RK4W_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define MARL_RK4W_NO_CONTRACT
#endif

namespace marl {

enum : int32_t { RK4W_DONE = 0, RK4W_TERMINAL = 1, RK4W_NONFINITE = -2 };   // marl_stats.status of a watched run
enum : int { RK4W_FRAME = 1, RK4W_STOP = 2 };                               // what rk4_watch_step returns (bits)

struct Rk4WatchRec {
    double t0, dt;          // in: the instance's start time and step
    double t;               // out: t0 + steps * dt
    double g[7];            // the monitors of the last processed state (marl_stats.event_value)
    int64_t n_events[7];    // sign changes counted
    int64_t steps;          // steps done
    int64_t next_frame;     // frames written so far = index of the next one (n_done)
    int32_t status, pad;
};

// monitor e (the reference's order, Evolve_scenario.py:107-109) from a reduction record
// {count, min y, min CA, min CC, min U, max CA+CC, max Phi, max W}: rk45_monitor_of_record, restated for the host
MARL_RK4W_FN double rk4_watch_monitor(const double* rec, int e)
{
    const int slot = (e < 3) ? e + 1 : (e == 3 ? 5 : (e == 4 ? 6 : (e == 5 ? 4 : 7)));
    return (e == 3 || e == 4) ? rec[slot] - 1.0 : rec[slot];
}

// the time after s steps
MARL_RK4W_FN double rk4_watch_time(double t0, double dt, int64_t s)
{
    MARL_RK4W_NO_CONTRACT
    const double p = (double)s * dt;
    return t0 + p;
}

// The record before the first step, from the reduction record of the initial state; returns RK4W_FRAME when frame 0 is the initial
// state (frame_steps[0] == 0), which the caller then writes.
MARL_RK4W_FN int rk4_watch_begin(Rk4WatchRec& r, const double* rec, const int64_t* frame_steps, int64_t n_frames)
{
    r.t = r.t0;
    for (int e = 0; e < 7; e++) {
        r.g[e] = rk4_watch_monitor(rec, e);
        r.n_events[e] = 0;
    }
    r.steps = 0;
    r.next_frame = 0;
    r.status = RK4W_DONE;
    r.pad = 0;
    if (n_frames > 0 && frame_steps[0] == 0) {
        r.next_frame = 1;
        return RK4W_FRAME;
    }
    return 0;
}

// The epilogue of step r.steps (0-based), whose result's reduction record is `rec`.  lim: 7 limits or NULL; t_events: the instance's
// [7][max_events] slots or NULL.  Returns RK4W_FRAME (the new state is frame r.next_frame - 1) | RK4W_STOP (the instance ends here).
MARL_RK4W_FN int rk4_watch_step(Rk4WatchRec& r, const double* rec, const int64_t* frame_steps, int64_t n_frames, const int64_t* lim,
                                double* t_events, int64_t max_events)
{
    MARL_RK4W_NO_CONTRACT
    const int64_t s = r.steps;
    const double t_old = rk4_watch_time(r.t0, r.dt, s), t_new = rk4_watch_time(r.t0, r.dt, s + 1);
    r.steps = s + 1;
    r.t = t_new;
    if (!(rec[0] == 0.0)) {   // some cell holds a non-finite field: before anything else
        r.status = RK4W_NONFINITE;
        return RK4W_STOP;
    }
    int out = 0;
    for (int e = 0; e < 7; e++) {
        const double go = r.g[e], gn = rk4_watch_monitor(rec, e);
        const bool up = go <= 0.0 && gn >= 0.0, down = go >= 0.0 && gn <= 0.0;   // ivp.py:149-151
        if (up || down) {
            const double d = go - gn;
            double tc = t_new;
            if (d != 0.0) {
                const double frac = go / d;
                const double add = r.dt * frac;
                tc = t_old + add;
            }
            if (t_events && r.n_events[e] < max_events) t_events[e * max_events + r.n_events[e]] = tc;
            r.n_events[e]++;
            if (lim && lim[e] > 0 && r.n_events[e] == lim[e]) {
                r.status = RK4W_TERMINAL;
                out |= RK4W_STOP;
            }
        }
        r.g[e] = gn;
    }
    if (r.next_frame < n_frames && frame_steps[r.next_frame] == s + 1) {
        r.next_frame++;
        out |= RK4W_FRAME;
    }
    return out;
}

// The host's check of a frame list: strictly ascending step counts in [0, nsteps].  Returns the index of the first entry that breaks
// the rule, -1 when there is none (n_frames = 0 included).
MARL_RK4W_FN int64_t rk4_watch_check_frames(const int64_t* frame_steps, int64_t n_frames, int64_t nsteps)
{
    for (int64_t j = 0; j < n_frames; j++)
        if (frame_steps[j] < 0 || frame_steps[j] > nsteps || (j > 0 && frame_steps[j] <= frame_steps[j - 1])) return j;
    return -1;
}

}  // namespace marl
