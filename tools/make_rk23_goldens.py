#!/usr/bin/env python3
"""Generate the RK23 golden vectors under tests/golden/ from the REAL reference: scipy's solve_ivp(method="RK23") on the reference's
fun_numba, imported unmodified through oracle/stubs exactly as oracle/make_goldens.py imports it for gen_rk45 / gen_rk45_event
(that module is imported here for its model construction; nothing under oracle/ is changed).  TEST INFRASTRUCTURE: it runs only where
the reference lies (oracle/make_goldens.py, REF); nothing in the product path or on a GPU machine imports this file.

Files written, with the keys of the rk45_* files of the same kind:

  rk23_traj_A_N64.npz            scenario A, N = 64, t1 = 0.01,  rtol = atol = 1e-3, first_step 1e-6
  rk23_traj_A_N200.npz           scenario A, N = 200, t1 = 0.002, the same tolerances, a 5-point t_eval
  rk23_traj_default_N200.npz     default scenario, N = 200, t1 = 0.002, the same tolerances
  rk23_traj_A_N64_tight.npz      scenario A, N = 64, t1 = 0.005, rtol 1e-6, atol 1e-8, first_step 1e-6
  rk23_event_default_N400.npz    y0, t_span, rtol, atol, first_step of rk45_event_default_N400.npz: zeros_U fires once
  rk23_event_default_N1500.npz   the porosity dip of the large-grid event test (0.04 deep, centred, 0.08 L wide) at N = 1500 to
                                 t1 = 2200 dx^2 with rtol 1e-5, atol 1e-7, first_step 0.5 dx^2: zeros_U fires once (with --large)

Every run also stores n_accepted, n_rejected, accepted (one flag per attempt, in order: the attempt sequence) and err_margin =
min |error norm - 1| over ALL its attempts.  The generator asserts what
the tests lean on, so that a changed input cannot silently test nothing: no attempt's error norm lies within 1e-4 of 1 (the margin
tests/test_gpu_parity.py::test_rk45_decision_margins_of_the_golden_trajectories asks of RK45 - a native loop whose norm differs in
the last bits then takes the same decisions), and the event runs fire zeros_U exactly once and no other monitor.

Usage:  python tools/make_rk23_goldens.py [--large]
"""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import make_goldens as mg  # noqa: E402  (puts oracle/stubs and the reference on sys.path, imports marlpde)
from scipy.integrate import solve_ivp  # noqa: E402
from scipy.integrate._ivp.rk import RK23  # noqa: E402

OUT = mg.OUT
MARGIN = 1e-4


class RecordingRK23(RK23):
    """scipy's RK23, unchanged, noting the error norm of every attempt (solve_ivp takes a solver class for `method`)."""
    norms = None

    def _estimate_error_norm(self, K, h, scale):
        n = super()._estimate_error_norm(K, h, scale)
        type(self).norms.append(float(n))
        return n


def run(fun, y0, t1, first_step, rtol, atol, t_eval, events, args):
    RecordingRK23.norms = []
    sol = solve_ivp(fun, (0.0, t1), y0, method=RecordingRK23, first_step=first_step, rtol=rtol, atol=atol, t_eval=t_eval,
                    dense_output=True, args=args, events=events)
    norms = np.array(RecordingRK23.norms)
    n_acc = len(sol.sol.ts) - 1
    n_rej = int(np.sum(~(norms < 1.0)))
    assert sol.status == 0 and len(norms) == n_acc + n_rej and sol.nfev == 1 + 3 * len(norms), (sol.status, len(norms), n_acc, n_rej, sol.nfev)
    margin = float(np.min(np.abs(norms - 1.0)))
    assert margin > MARGIN, f"an attempt's error norm lies {margin:.2e} from 1: the run is no test of the decisions"
    return sol, n_acc, n_rej, margin, norms < 1.0


def gen_traj():
    runs = [("A", 64, 1e-2, 1e-3, 1e-3, None, ""),
            ("A", 200, 2e-3, 1e-3, 1e-3, 5, ""),
            ("default", 200, 2e-3, 1e-3, 1e-3, None, ""),
            ("A", 64, 5e-3, 1e-6, 1e-8, None, "_tight")]
    for s, N, t1, rtol, atol, n_eval, tag in runs:
        eq, y0, p, _ = mg.build_model(mg.SCENARIOS[s], N, 1)
        eq.last_t = 0.0
        t_eval = None if n_eval is None else np.linspace(0.0, t1, n_eval)
        t_start = time.time()
        sol, n_acc, n_rej, margin, accepted = run(eq.fun_numba, y0, t1, 1e-6, rtol, atol, t_eval, [getattr(eq, e) for e in mg.EVENTS],
                                        [mg._Bar(), t1 / 1000, 0.0])
        name = f"rk23_traj_{s}_N{N}{tag}.npz"
        np.savez_compressed(os.path.join(OUT, name), y0=y0, t_span=np.array([0.0, t1]), rtol=rtol, atol=atol, first_step=1e-6,
                            step_times=np.asarray(sol.sol.ts), y_final=sol.sol(t1), nfev=sol.nfev, status=sol.status,
                            t_eval=(np.array([]) if t_eval is None else sol.t), y_eval=(np.array([]) if t_eval is None else sol.y),
                            n_events=np.array([len(e) for e in sol.t_events]), n_accepted=n_acc, n_rejected=n_rej, err_margin=margin, accepted=accepted,
                            scenario=s, N=N)
        print(f"rk23 {name}: {n_acc + n_rej} attempts, {n_rej} rejected, nfev {sol.nfev}, closest norm {margin:.1e} from 1, "
              f"{time.time() - t_start:.1f}s")


def gen_event(N, y, t1, first_step, rtol, atol, name):
    eq, _, p, _ = mg.build_model(mg.SCENARIOS["default"], N, 1)
    eq.last_t = 0.0
    t_start = time.time()
    sol, n_acc, n_rej, margin, accepted = run(eq.fun_numba, y, t1, first_step, rtol, atol, None, [getattr(eq, e) for e in mg.EVENTS],
                                    [mg._Bar(), t1 / 1000, 0.0])
    tev, nev = mg._pack_events(sol.t_events)
    assert nev.tolist() == [0, 0, 0, 0, 0, 1, 0], f"zeros_U is to fire exactly once and nothing else: {nev.tolist()}"
    np.savez_compressed(os.path.join(OUT, name), y0=y, t_span=np.array([0.0, t1]), rtol=rtol, atol=atol, first_step=first_step,
                        step_times=np.asarray(sol.sol.ts), y_final=sol.y[:, -1], nfev=sol.nfev, status=sol.status, t_events=tev,
                        n_events=nev, n_accepted=n_acc, n_rejected=n_rej, err_margin=margin, accepted=accepted, N=N)
    print(f"rk23 {name}: {n_acc + n_rej} attempts, {n_rej} rejected, nfev {sol.nfev}, events {nev.tolist()}, roots {tev.tolist()}, "
          f"closest norm {margin:.1e} from 1, {time.time() - t_start:.1f}s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--large", action="store_true", help="also the N = 1500 event run (minutes: the reference's RHS is a Python loop here)")
    a = ap.parse_args()
    gen_traj()
    g = np.load(os.path.join(OUT, "rk45_event_default_N400.npz"))
    gen_event(400, g["y0"], float(g["t_span"][1]), float(g["first_step"]), float(g["rtol"]), float(g["atol"]), "rk23_event_default_N400.npz")
    if a.large:
        N = 1500
        eq, y0, p, depths = mg.build_model(mg.SCENARIOS["default"], N, 1)
        L = p["max_depth"] / p["Xstar"]
        x = depths._axes_coords[0]
        y = y0.reshape(5, N).copy()
        y[4] = p["PhiIni"] - 0.04 * np.exp(-((x - 0.5 * L) / (0.08 * L)) ** 2)
        dx2 = (L / N) ** 2
        gen_event(N, y.ravel(), 2200 * dx2, 0.5 * dx2, 1e-5, 1e-7, "rk23_event_default_N1500.npz")


if __name__ == "__main__":
    main()
