// Terminal monitors, the only statement of the rule in the project: scipy's handle_events (scipy/integrate/_ivp/ivp.py:79-130) for the
// seven monitors of one accepted step of a forward integration.  A monitor e with terminal[e] = k > 0 stops the run at its k-th
// occurrence (scipy >= 1.13: event.terminal may be an int; True is 1); terminal[e] = 0: it never does.  Called by the Radau sweeps'
// device-side controller (radau_control_step, marl_radau_batch.h), by the BDF sweep's (bdf_control_step, marl_bdf_ctl.h) and by the
// host's accepted_step_epilogue of the implicit single runs (marl_api.hip).  Nothing but <stdint.h> and <math.h>: a host C++ compiler builds this header alone (tests/test_terminal_select_cpu.py
// holds it to scipy's own handle_events that way); under hipcc it follows <hip/hip_runtime.h>, which defines __forceinline__.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define MARL_TERMINAL_FN __host__ __device__ __forceinline__
#else
#define MARL_TERMINAL_FN inline
#endif

namespace marl {

// Does monitor e, active with its count-th occurrence (this step's included: scipy's event_count after `+= 1`, ivp.py:680), meet its limit?
MARL_TERMINAL_FN bool terminal_met(int64_t count, int64_t limit) { return limit > 0 && count >= limit; }

// active: bit e = monitor e changed sign in the accepted step; roots[e]: its root time; counts[e]: its occurrences including this step;
// terminal[e]: its limit.  (Entries of inactive monitors are not read.)
// Returns 0 - no active monitor meets its limit: *keep = active, *t_stop untouched - or 1: the active monitors ordered by root time
// (equal roots stay in monitor order: what np.argsort leaves for arrays this short), the first in that order that meets its limit
// ends the run - *keep = the monitors up to and including it, *t_stop = its root; the sign changes after it never happened.
MARL_TERMINAL_FN int terminal_select(uint32_t active, const double roots[7], const int64_t counts[7], const int64_t terminal[7], uint32_t* keep,
                                     double* t_stop)
{
    bool any = false;
    for (int e = 0; e < 7; e++)
        if (((active >> e) & 1) && terminal_met(counts[e], terminal[e])) any = true;
    if (!any) { *keep = active; return 0; }
    int order[7], m = 0;
    for (int e = 0; e < 7; e++) {   // insertion sort, stable
        if (!((active >> e) & 1)) continue;
        int i = m++;
        while (i > 0 && roots[order[i - 1]] > roots[e]) { order[i] = order[i - 1]; i--; }
        order[i] = e;
    }
    uint32_t k = 0;
    for (int i = 0; i < m; i++) {
        const int e = order[i];
        k |= 1u << e;
        if (terminal_met(counts[e], terminal[e])) { *t_stop = roots[e]; break; }
    }
    *keep = k;
    return 1;
}

}  // namespace marl
