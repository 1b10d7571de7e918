// marl_dop853_stop.h - terminal monitors in the native DOP853 loop: the scalar walk of ONE accepted step in which a monitor that changed
// sign meets its limit (marl_set_terminal).  The DOP853 loop (marl_dop853.h) replays an accepted step trip by trip - a PROBE of Brent's
// method, a t_eval SAMPLE - and thread 0 says between two trips what the next one is.  For a step that ends the run it asks this walk:
//   dop853_stop_begin   is this such a step (rk_terminal_any_met on the counts BEFORE the step)?  then which monitors need a root - all
//                       that changed sign, with or without a free slot;
//   dop853_stop_root    one root is known; which are left;
//   dop853_stop_rule    every root is known: what rk_terminal_step says - the kept mask, the counts, the slots, t_stop;
//   dop853_stop_next    the next trip: a probe while roots are missing, then the samples t_eval[k] <= t_stop, then the stop itself - one
//                       more replay at t_stop whose result becomes the state.
// The rule itself stays where it is stated (marl_terminal.h, through marl_rk_terminal.h).  Nothing but <stdint.h>, <math.h> and those
// two: a host C++ compiler builds this header alone (tests/test_dop853_stop_cpu.py holds it to scipy's handle_events that way); under
// hipcc it follows <hip/hip_runtime.h>.
#pragma once
#include <math.h>
#include <stdint.h>

#include "marl_rk_terminal.h"

namespace marl {

// the stage of the walk
enum : int32_t { DOP853_STOP_IDLE = 0, DOP853_STOP_ROOTS = 1, DOP853_STOP_SAMPLES = 2 };
// what dop853_stop_next answers: the numbers of the loop's trip kinds (DOP853_SAMPLE, DOP853_PROBE, DOP853_STOP of marl_dop853.h)
enum : int { DOP853_NEXT_SAMPLE = 1, DOP853_NEXT_PROBE = 2, DOP853_NEXT_STOP = 3 };

// Everything the stop adds to thread 0's state (LDS of the stop kernel only).
struct Dop853Stop {
    int64_t limit[7];   // marl_set_terminal's limits
    double root[7];     // the roots of the step's monitors, kept until the rule has said which of them happened
    double g_new[7];    // the monitors of y_new: the bookkeeping of the kept monitors needs them after the probes
    double t_stop;      // where the run ends
    uint32_t active;    // monitors that changed sign in the step (bit e)
    uint32_t locate;    // those still without a root
    uint32_t kept;      // after the rule: the sign changes that happened
    int32_t stage;      // DOP853_STOP_*
};

MARL_TERMINAL_FN void dop853_stop_init(Dop853Stop& s, const int64_t limit[7])
{
    s = Dop853Stop{};
    for (int e = 0; e < 7; e++) s.limit[e] = limit[e];
}

// An accepted step: `changed` (bit e = monitor e changed sign), n_events[e] the counts BEFORE the step.  True: the step ends the run -
// every monitor of `changed` is to be located (s.locate) and nothing of the step is booked yet.  False: s is untouched and the step
// runs as it does without limits.
MARL_TERMINAL_FN bool dop853_stop_begin(Dop853Stop& s, uint32_t changed, const int64_t n_events[7])
{
    if (!rk_terminal_any_met(changed, n_events, s.limit)) return false;
    s.active = changed;
    s.locate = changed;
    s.kept = 0;
    s.stage = DOP853_STOP_ROOTS;
    return true;
}

// Monitor e's root is known.  Returns the monitors still to be located.
MARL_TERMINAL_FN uint32_t dop853_stop_root(Dop853Stop& s, int e, double root)
{
    s.root[e] = root;
    s.locate &= ~(1u << e);
    return s.locate;
}

// Every root is known: rk_terminal_step on them.  n_events[e]: still the counts before the step; n_events_out[e], slot[e] as
// rk_terminal_step gives them (n_events_out may alias n_events).  Leaves s.kept and s.t_stop and moves on to the samples.
MARL_TERMINAL_FN void dop853_stop_rule(Dop853Stop& s, const int64_t n_events[7], int64_t max_events, int64_t n_events_out[7], int64_t slot[7])
{
    uint32_t keep = 0;
    double ts = 0.0;
    rk_terminal_step(s.active, s.root, n_events, s.limit, max_events, &keep, &ts, n_events_out, slot);   // (stops: dop853_stop_begin said so)
    s.kept = keep;
    s.t_stop = ts;
    s.stage = DOP853_STOP_SAMPLES;
}

// The next trip of a step that ends the run; ie: the next sample, t_eval[ie] (t_eval is not read when ie >= n_eval).
MARL_TERMINAL_FN int dop853_stop_next(const Dop853Stop& s, int64_t ie, int64_t n_eval, const double* t_eval)
{
    if (s.locate != 0) return DOP853_NEXT_PROBE;
    if (ie < n_eval && t_eval[ie] <= s.t_stop) return DOP853_NEXT_SAMPLE;
    return DOP853_NEXT_STOP;
}

}  // namespace marl
