// Terminal monitors in the explicit adaptive loops (RK45, RK23): what ONE accepted step does with the rule of marl_terminal.h
// (terminal_select, scipy's handle_events) - which sign changes happened, how the counts move and where the kept roots are stored.
// Called by the sweep kernels (rk45_sweep_body<..., TERM>, marl_kernels.h), by the host loop of the single runs (rk_run,
// marl_api.hip) and by the DOP853 loop's walk of a step that ends the run (marl_dop853_stop.h), so the rule and its bookkeeping stay
// stated once.  Nothing but <stdint.h>, <math.h> and marl_terminal.h: a host C++
// compiler builds this header alone (tests/test_rk_terminal_cpu.py holds it to scipy's handle_events that way); under hipcc it
// follows <hip/hip_runtime.h>.
#pragma once
#include <math.h>
#include <stdint.h>

#include "marl_terminal.h"

namespace marl {

// Does any monitor of `active` (bit e = monitor e changed sign in the step) meet its limit in this step?  n_events[e]: the count
// BEFORE the step, so this occurrence is number n_events[e] + 1.  False: the step runs as it does without limits.
MARL_TERMINAL_FN bool rk_terminal_any_met(uint32_t active, const int64_t n_events[7], const int64_t terminal[7])
{
    bool met = false;
    for (int e = 0; e < 7; e++)
        if (((active >> e) & 1) && terminal_met(n_events[e] + 1, terminal[e])) met = true;
    return met;
}

// One accepted step.  active, roots[e] (read for active monitors only), n_events[e] before the step, terminal[e], max_events (root
// slots per monitor; <= 0: none).  Returns 1 when the run stops in this step (*t_stop = the terminal monitor's root), else 0 (*t_stop
// untouched).  *keep: the sign changes that happened (all of `active` without a stop; with one, those up to and including the
// terminal monitor in the order of root times, equal roots in monitor order).  n_events_out[e]: n_events[e] + 1 for kept monitors,
// n_events[e] otherwise - "the sign changes after it never happened".  slot[e]: where a kept monitor's root is stored
// (its count before the step), or -1: not kept, or no free slot.  n_events_out may alias n_events.
MARL_TERMINAL_FN int rk_terminal_step(uint32_t active, const double roots[7], const int64_t n_events[7], const int64_t terminal[7],
                                      int64_t max_events, uint32_t* keep, double* t_stop, int64_t n_events_out[7], int64_t slot[7])
{
    int64_t counts[7];
    for (int e = 0; e < 7; e++) counts[e] = n_events[e] + (((active >> e) & 1) ? 1 : 0);
    uint32_t k = 0;
    const int stop = terminal_select(active, roots, counts, terminal, &k, t_stop);
    for (int e = 0; e < 7; e++) {
        const bool kept = (k >> e) & 1;
        const int64_t before = n_events[e];
        slot[e] = (kept && before < max_events) ? before : -1;
        n_events_out[e] = kept ? before + 1 : before;
    }
    *keep = k;
    return stop;
}

}  // namespace marl
