"""The reference of the DOP853 tests for everything no golden file holds: scipy's solve_ivp(method="DOP853", events=[7 monitors], t_eval=...)
on the CPU oracle's RHS and monitors (oracle.rhs / oracle.events), or on any small ODE - TEST INFRASTRUCTURE, the product never imports
this module.

scipy's solver is used unchanged; a subclass only notes, for every attempt, the two sums of the error norm, the norm itself and the step
size the solver holds afterwards, and for every accepted step whether its dense output was built (the three extra evaluations); it can
end the run after a budget of attempts the way the native loops do (status 2: the state, time and counts after the last attempt of the
budget; the samples and roots reached until then)."""
import numpy as np

from scipy.integrate import solve_ivp
from scipy.integrate._ivp.rk import DOP853


class _Budget(Exception):
    pass


class RecordingDOP853(DOP853):
    norms = None      # error norm of every attempt
    sums = None       # (|err5 / scale|^2, |err3 / scale|^2) of every attempt, as _estimate_error_norm forms them
    h_try = None      # the signed step of every attempt
    h_after = None    # h_abs after every attempt
    steps = None      # t0 and the end of every accepted step
    dense = None      # index (among the accepted steps) of every step whose dense output was built
    budget = 0
    last = None

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        type(self).last = self

    def _estimate_error_norm(self, K, h, scale):
        cls = type(self)
        if cls.budget > 0 and len(cls.norms) >= cls.budget:
            raise _Budget()
        err5 = np.dot(K.T, self.E5) / scale
        err3 = np.dot(K.T, self.E3) / scale
        cls.sums.append((float(np.linalg.norm(err5) ** 2), float(np.linalg.norm(err3) ** 2)))
        cls.h_try.append(float(h))
        n = super()._estimate_error_norm(K, h, scale)
        cls.norms.append(float(n))
        return n

    def _step_impl(self):
        cls = type(self)
        before = len(cls.norms)
        try:
            out = super()._step_impl()
        except _Budget:   # (nothing of the solver's state is assigned before an attempt is accepted)
            self.nfev -= 12   # the stages of the attempt beyond the budget, which the native loops never start
            cls.h_after.extend([None] * (len(cls.norms) - before))
            return False, "attempt budget"
        # _step_impl loops over rejected attempts itself: h_abs is visible after the accepted one only; the rejected ones' follow from it
        cls.h_after.extend([None] * (len(cls.norms) - before - 1) + [float(self.h_abs)])
        if out[0]:
            cls.steps.append(float(self.t))
        return out

    def _dense_output_impl(self):
        type(self).dense.append(len(type(self).steps) - 2)
        return super()._dense_output_impl()


class Dop853Ref:
    """status (0, or 2 after `max_attempts`), n_accepted, n_rejected, nfev (scipy's own count of calls), t, y_final, t_eval / y_eval (frames
    reached, (n, 5N)), t_events (7 arrays), accepted (flag per attempt), sums, h_try, h_after (per attempt), step_times (t0 and the end of
    every accepted step), dense_steps (accepted steps with a dense output), margin (min |error norm - 1| over the attempts)."""


def record(fun, y0, t_span, first_step, rtol, atol, t_eval=None, events=None, max_attempts=0):
    R = RecordingDOP853
    R.norms, R.sums, R.h_try, R.h_after, R.steps, R.dense, R.budget = [], [], [], [], [float(t_span[0])], [], int(max_attempts)
    with np.errstate(all="ignore"):
        sol = solve_ivp(fun, t_span, np.asarray(y0, float), method=R, first_step=first_step, rtol=rtol, atol=atol, t_eval=t_eval, events=events)
    norms = np.array(R.norms)
    solver = R.last
    r = Dop853Ref()
    r.accepted = norms < 1.0
    r.n_accepted, r.n_rejected, r.nfev = int(np.sum(r.accepted)), int(np.sum(~r.accepted)), int(solver.nfev)
    stopped = max_attempts > 0 and sol.status == -1
    assert sol.status == 0 or stopped, sol.message
    r.status = 2 if stopped else 0
    r.t, r.y_final = float(solver.t), np.array(solver.y)
    r.t_eval = None if t_eval is None else np.array(sol.t)
    r.y_eval = None if t_eval is None else np.array(sol.y).T.copy()
    r.t_events = None if events is None else [np.array(t) for t in sol.t_events]
    r.step_times = np.array(R.steps)
    r.sums, r.h_try, r.h_after = list(R.sums), list(R.h_try), list(R.h_after)
    r.dense_steps = sorted(set(R.dense))
    r.margin = float(np.min(np.abs(norms - 1.0))) if len(norms) else np.inf
    assert r.nfev == 1 + 12 * len(norms) + 3 * len(r.dense_steps), "scipy counts otherwise than 1 + 12 attempts + 3 dense outputs"
    return r


def scipy_dop853(oracle, P, N, y0, t_span, first_step, rtol, atol, t_eval=None, max_attempts=0):
    def fun(t, y):
        return oracle.rhs(P, N, y)

    seen = {}

    def monitor(e):   # (solve_ivp asks the seven monitors of a state one after the other: one oracle call serves them)
        def g(t, y):
            key = (float(t), float(y[0]), float(y[-1]))
            if key not in seen:
                seen.clear()
                seen[key] = oracle.events(P, N, y)
            return seen[key][e]
        return g

    return record(fun, y0, t_span, first_step, rtol, atol, t_eval=t_eval, events=[monitor(e) for e in range(7)], max_attempts=max_attempts)
