#!/usr/bin/env python3
"""Generate the DOP853 golden vectors under tests/golden/ from the REAL reference: scipy's solve_ivp(method="DOP853") on the reference's
fun_numba, imported unmodified through oracle/stubs exactly as oracle/make_goldens.py imports it (that module is imported here for its
model construction; nothing under oracle/ is changed).  TEST INFRASTRUCTURE: it runs only where the reference lies
(oracle/make_goldens.py, REF); nothing in the product path or on a GPU machine imports this file.  The solver is scipy's, unchanged, under
the recording subclass of tests/dop853_ref.py (error norms, step times, which steps built a dense output).

Files written, with the keys of the rk23_* files of the same kind:

  dop853_traj_A_N64.npz          scenario A, N = 64, t1 = 0.01, rtol 1e-5, atol 1e-7, first_step 1e-6 (at rtol = atol = 1e-3, the tolerances
                                 of the RK23 file of this name, DOP853 overshoots its stability limit and a quarter of the attempts end
                                 in a NaN norm: no margin to speak of, so the scenario was replaced)
  dop853_traj_default_N200.npz   default scenario, N = 200, t1 = 0.002, rtol = atol = 1e-3, first_step 1e-6, a 5-point t_eval
  dop853_event_default_N400.npz  y0, t_span, rtol, atol, first_step of rk45_event_default_N400.npz: zeros_U fires once

Every run stores n_accepted, n_rejected, accepted (one flag per attempt, in order), dense_steps (the accepted steps whose dense output
scipy built: nfev = 1 + 12 attempts + 3 len(dense_steps), asserted) and err_margin = min |error norm - 1| over ALL its attempts.  The
generator asserts what the tests lean on: no attempt's error norm lies within 1e-4 of 1, and the event run fires zeros_U exactly once
and no other monitor.  A scenario that misses the margin is to be replaced, not the margin lowered.

Usage:  python tools/make_dop853_goldens.py
"""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from oracle import make_goldens as mg  # noqa: E402  (puts oracle/stubs and the reference on sys.path, imports marlpde)
from dop853_ref import record  # noqa: E402

OUT = mg.OUT
MARGIN = 1e-4


def run(eq, y0, t1, first_step, rtol, atol, t_eval):
    eq.last_t = 0.0
    args = [mg._Bar(), t1 / 1000, 0.0]
    events = [lambda t, y, name=name: getattr(eq, name)(t, y, *args) for name in mg.EVENTS]
    r = record(lambda t, y: eq.fun_numba(t, y, *args), y0, (0.0, t1), first_step, rtol, atol, t_eval=t_eval, events=events)
    assert r.status == 0 and r.t == t1
    assert r.margin > MARGIN, f"an attempt's error norm lies {r.margin:.2e} from 1: the run is no test of the decisions"
    return r


def save(name, r, y0, t1, first_step, rtol, atol, t_eval, N, extra):
    np.savez_compressed(os.path.join(OUT, name), y0=y0, t_span=np.array([0.0, t1]), rtol=rtol, atol=atol, first_step=first_step,
                        step_times=r.step_times, y_final=r.y_final, nfev=r.nfev, status=r.status,
                        t_eval=(np.array([]) if t_eval is None else r.t_eval), y_eval=(np.array([]) if t_eval is None else r.y_eval.T),
                        n_events=np.array([len(e) for e in r.t_events]), n_accepted=r.n_accepted, n_rejected=r.n_rejected,
                        err_margin=r.margin, accepted=r.accepted, dense_steps=np.array(r.dense_steps, dtype=np.int64), N=N, **extra)
    size = os.path.getsize(os.path.join(OUT, name))
    assert size <= 100 * 1024, (name, size)
    return size


def main():
    for s, N, t1, n_eval, rtol, atol in (("A", 64, 1e-2, None, 1e-5, 1e-7), ("default", 200, 2e-3, 5, 1e-3, 1e-3)):
        eq, y0, p, _ = mg.build_model(mg.SCENARIOS[s], N, 1)
        t_eval = None if n_eval is None else np.linspace(0.0, t1, n_eval)
        t_start = time.time()
        r = run(eq, y0, t1, 1e-6, rtol, atol, t_eval)
        name = f"dop853_traj_{s}_N{N}.npz"
        size = save(name, r, y0, t1, 1e-6, rtol, atol, t_eval, N, dict(scenario=s))
        print(f"dop853 {name}: {len(r.accepted)} attempts, {r.n_rejected} rejected, nfev {r.nfev}, dense outputs {len(r.dense_steps)}, "
              f"closest norm {r.margin:.1e} from 1, {size} bytes, {time.time() - t_start:.1f}s")
    g = np.load(os.path.join(OUT, "rk45_event_default_N400.npz"))
    N, y0, t1 = 400, g["y0"], float(g["t_span"][1])
    eq, _, p, _ = mg.build_model(mg.SCENARIOS["default"], N, 1)
    t_start = time.time()
    r = run(eq, y0, t1, float(g["first_step"]), float(g["rtol"]), float(g["atol"]), None)
    tev, nev = mg._pack_events(r.t_events)
    assert nev.tolist() == [0, 0, 0, 0, 0, 1, 0], f"zeros_U is to fire exactly once and nothing else: {nev.tolist()}"
    name = "dop853_event_default_N400.npz"
    size = save(name, r, y0, t1, float(g["first_step"]), float(g["rtol"]), float(g["atol"]), None, N, dict(t_events=tev))
    print(f"dop853 {name}: {len(r.accepted)} attempts, {r.n_rejected} rejected, nfev {r.nfev}, events {nev.tolist()}, roots {tev.tolist()}, "
          f"closest norm {r.margin:.1e} from 1, {size} bytes, {time.time() - t_start:.1f}s")


if __name__ == "__main__":
    main()
