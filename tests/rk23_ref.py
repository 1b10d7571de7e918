"""The reference of the RK23 tests for everything no golden file holds: scipy's solve_ivp(method="RK23", events=[7 monitors], t_eval=...)
on the CPU oracle's RHS and monitors (oracle.rhs / oracle.events) - TEST INFRASTRUCTURE, the product never imports this module.

scipy's solver is used unchanged; a subclass only notes the error norm of every attempt (the attempt sequence and how close the
closest decision was) and can end the run after a budget of attempts the way the native loops do (status 2: the state, time and counts
after the last attempt of the budget; the samples and roots reached until then)."""
import numpy as np

from scipy.integrate import solve_ivp
from scipy.integrate._ivp.rk import RK23


class _Budget(Exception):
    pass


class RecordingRK23(RK23):
    norms = None
    steps = None
    budget = 0
    last = None

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        type(self).last = self

    def _estimate_error_norm(self, K, h, scale):
        cls = type(self)
        if cls.budget > 0 and len(cls.norms) >= cls.budget:
            raise _Budget()
        n = super()._estimate_error_norm(K, h, scale)
        cls.norms.append(float(n))
        return n

    def _step_impl(self):
        try:
            out = super()._step_impl()
            if out[0]:
                type(self).steps.append(float(self.t))
            return out
        except _Budget:   # (nothing of the solver's state is assigned before an attempt is accepted)
            return False, "attempt budget"


class Rk23Ref:
    """status (0, or 2 after `max_attempts`), n_accepted, n_rejected, nfev, t, y_final, t_eval / y_eval (frames reached, (n, 5N)), t_events (7
    arrays), accepted (flag per attempt), step_times (t0 and the end of every accepted step), margin (min |error norm - 1| over the attempts)."""


def scipy_rk23(oracle, P, N, y0, t_span, first_step, rtol, atol, t_eval=None, max_attempts=0):
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

    RecordingRK23.norms, RecordingRK23.steps, RecordingRK23.budget = [], [float(t_span[0])], int(max_attempts)
    with np.errstate(all="ignore"):
        sol = solve_ivp(fun, t_span, np.asarray(y0, float), method=RecordingRK23, first_step=first_step, rtol=rtol, atol=atol, t_eval=t_eval,
                        events=[monitor(e) for e in range(7)])
    norms = np.array(RecordingRK23.norms)
    solver = RecordingRK23.last
    r = Rk23Ref()
    r.accepted = norms < 1.0
    r.n_accepted, r.n_rejected, r.nfev = int(np.sum(r.accepted)), int(np.sum(~r.accepted)), 1 + 3 * len(norms)
    stopped = max_attempts > 0 and sol.status == -1
    assert sol.status == 0 or stopped, sol.message
    r.status = 2 if stopped else 0
    r.t, r.y_final = float(solver.t), np.array(solver.y)
    r.t_eval = None if t_eval is None else np.array(sol.t)
    r.y_eval = None if t_eval is None else np.array(sol.y).T.copy()
    r.t_events = [np.array(t) for t in sol.t_events]
    r.step_times = np.array(RecordingRK23.steps)
    r.margin = float(np.min(np.abs(norms - 1.0))) if len(norms) else np.inf
    return r
