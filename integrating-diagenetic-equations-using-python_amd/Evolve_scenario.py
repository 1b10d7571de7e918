"""Driver - host-side mirror of ``marlpde/Evolve_scenario.py``.

``integrate_equations(solver_parms, tracker_parms, pde_parms)`` takes the same three dictionaries as the
reference (Evolve_scenario.py:19) and returns the same tuple
``(last (5, N) profile, covered_time [years], depths, Xstar, store_folder)`` (:183).

* ``solver_parms["backend"] == "hip"`` and ``method == "RK45"``: the whole adaptive loop
  (scipy-exact Dormand-Prince controller, the seven monitors with root finding, ``t_eval`` by dense
  output) runs on the GPU via ``marl_integrate_rk45``.
* ``backend == "hip"`` and ``method == "RK23"``: the same loop with scipy's Bogacki-Shampine 3(2) pair (3 RHS evaluations per
  attempt, step factor ``0.9 err^(-1/3)``, cubic dense output) via ``marl_integrate_rk23`` - no scipy in the loop.
* ``backend == "hip"`` and ``method == "DOP853"`` on a grid of up to 1024 cells, without terminal monitors: scipy's Dormand-Prince
  8(5,3) (12 evaluations per attempt, step factor ``0.9 err^(-1/8)``, the degree-7 dense output whose 3 extra evaluations scipy
  counts) via ``marl_integrate_dop853`` - no scipy in the loop.  Terminal monitors: ``native_terminal=True`` takes
  ``marl_integrate_dop853_stop``.  Larger grids: ``solver_parms["native_grid"] = True`` takes the large-grid loop, one launch per
  stage, via ``marl_integrate_dop853_grid`` (with a terminal monitor only together with ``native_terminal=True``) - no scipy in
  the loop either.  Without these keys larger grids and terminal monitors take the scipy route below.
* ``backend == "hip"`` and ``method == "RK4"`` (no counterpart in scipy or the reference): fixed-step classical RK4 with the whole driver
  inside one kernel via ``marl_integrate_rk4_watch`` - ``solver_parms["dt"]`` is required, ``t_span`` and every ``t_eval`` entry must lie
  on step ends, N <= 1024; the monitors' root times are secant estimates between step ends (no dense output), ``terminal`` ends the run
  at the end of the step of the occurrence, and a state that goes non-finite ends it with status -2 (:func:`rk4_schedule`).
* ``backend == "hip"`` and ``method == "Radau"`` (the reference's default, parameters.py:213): scipy's Radau IIA step
  logic restated natively, with the RHS, the finite-difference Jacobian (the reference's 27-diagonal pattern), the
  block-tridiagonal LU factorisations and every vector operation on the GPU via ``marl_integrate_radau`` - no scipy in the loop.
* ``backend == "hip"`` and ``method == "BDF"``: scipy's BDF step logic restated natively on the same Jacobian /
  factorisation kernels via ``marl_integrate_bdf`` - no scipy in the loop either.
* ``backend == "hip"`` and any other scipy method (LSODA with the reference's ``lband = uband = 1``; or any
  method with ``solver_parms["scipy_driver"] = True``; DOP853 where the native loop does not reach): scipy's ``solve_ivp`` drives, exactly as in the reference
  (:104-109), with the HIP RHS and HIP monitors as callables
  (``test_every_other_method_of_the_reference_solver_runs_through_scipy_on_the_hip_rhs``).
* other backends: rejected - this package has no CPU implementation.

Results are stored like the reference's (:156-178) with the same dataset names, as ``.npz`` (always) and
HDF5 (when h5py is importable).
"""
import os
import time
from datetime import datetime

import numpy as np

from .LHeureux_model import EVENT_NAMES, DepthGrid, LMAHeureuxPorosityDiff, terminal_counts

EVENT_TEXT = (
    "any field at any depth crossed zero", "CA at any depth crossed zero", "CC at any depth crossed zero",
    "CA + CC at any depth crossed one", "the porosity at any depth crossed one", "U at any depth crossed zero",
    "W at any depth crossed zero")


class _NoBar:
    n = 0

    def update(self, k):
        self.n += k


def _scipy_events(eq, limits):
    """The model's seven event callables for solve_ivp, each carrying its ``terminal`` as scipy reads it (False, or the count)."""
    def make(name, limit):
        bound = getattr(eq, name)

        def event(t, y, *args):
            return bound(t, y, *args)
        event.terminal = limit if limit else False
        return event
    return [make(name, limit) for name, limit in zip(EVENT_NAMES, limits)]


RK4_MAX_CELLS = 1024    # the monitored fixed-step loop runs grids of one workgroup
RK4_ON_GRID = 1e-6      # how far, in steps, a time may lie from a step end


def rk4_schedule(solver_parms, t_span, t_eval, N):
    """``(dt, nsteps, frame_steps)`` of an ``integrate_equations(method="RK4")`` run - a pure function, so that every complaint is
    raised before a model (and with it a GPU context) exists.  ``solver_parms["dt"]`` is required and positive;
    ``nsteps = (t1 - t0) / dt`` and every ``t_eval`` entry must lie on a step end, within 1e-6 of a step, the entries strictly
    ascending within ``t_span``; ``frame_steps`` (None without ``t_eval``) are their step counts.  N > 1024: ValueError."""
    if int(N) > RK4_MAX_CELLS:
        raise ValueError(f"method 'RK4': N = {int(N)} exceeds {RK4_MAX_CELLS} cells, the largest grid the monitored fixed-step loop runs "
                         "(marl_integrate_rk4_watch)")
    dt = solver_parms.get("dt")
    if dt is None:
        raise ValueError("method 'RK4' is a fixed-step method: the solver parameters need 'dt', the step")
    dt = float(dt)
    if not (dt > 0.0 and np.isfinite(dt)):
        raise ValueError(f"method 'RK4': dt = {dt!r} must be positive and finite")
    t0, t1 = float(t_span[0]), float(t_span[1])
    if not t1 >= t0:
        raise ValueError(f"method 'RK4': t_span = ({t0!r}, {t1!r}) must run forward")

    def steps_of(t, what):
        x = (float(t) - t0) / dt
        k = int(round(x))
        if not abs(x - k) <= RK4_ON_GRID:
            raise ValueError(f"method 'RK4': {what} = {float(t)!r} is not on a step end: (t - t0) / dt = {x!r} with t0 = {t0!r}, dt = {dt!r}")
        return k

    nsteps = steps_of(t1, "t_span[1]")
    if t_eval is None:
        return dt, nsteps, None
    frame_steps = []
    for i, t in enumerate(np.asarray(t_eval, dtype=float).ravel()):
        k = steps_of(t, f"t_eval[{i}]")
        if k < 0 or k > nsteps:
            raise ValueError(f"method 'RK4': t_eval[{i}] = {float(t)!r} lies outside t_span = ({t0!r}, {t1!r})")
        if frame_steps and k <= frame_steps[-1]:
            raise ValueError(f"method 'RK4': t_eval[{i}] = {float(t)!r} does not follow t_eval[{i - 1}]: the sample times must be strictly ascending")
        frame_steps.append(k)
    return dt, nsteps, np.array(frame_steps, dtype=np.int64)


def integrate_equations(solver_parms, tracker_parms, pde_parms, results_root="../Results/", verbose=True, device=0, terminal=None):
    """``terminal``: the reference's switch (LHeureux_model.py:113-122) - which monitors end the run at their root, as
    :func:`marlpde_amd.LHeureux_model.terminal_counts` reads it.  Native for Radau and BDF; for RK45 / RK23 the solver parameters
    choose: ``native_terminal=True`` - the native loop stops itself (marl_integrate_rk45_terminal / rk23_terminal) - or
    ``scipy_driver=True`` - solve_ivp drives the HIP RHS.  DOP853 with a terminal monitor: ``native_terminal=True`` and N <= 1024 - the
    native loop stops itself (marl_integrate_dop853_stop); ``native_terminal=True`` with ``native_grid=True`` and N > 1024 - the
    large-grid loop stops itself (marl_integrate_dop853_grid); otherwise solve_ivp drives the HIP RHS, as it does without the switch."""
    limits = terminal_counts(terminal)
    solver_parms = dict(solver_parms)
    Xstar, Tstar = pde_parms["Xstar"], pde_parms["Tstar"]
    N = int(pde_parms["N"])
    depths = DepthGrid(pde_parms["max_depth"] / Xstar, N)

    backend = solver_parms.pop("backend", "hip")
    if backend != "hip":
        raise ValueError(f"backend {backend!r} is not available here: only 'hip' (MI355X kernels) is implemented; "
                         "use the reference package for its 'numba'/'numpy' CPU backends")
    if solver_parms.get("method") == "RK4":   # (before the model exists: every complaint about the schedule needs no GPU)
        rk4_dt, rk4_nsteps, rk4_frames = rk4_schedule(solver_parms, tuple(solver_parms.get("t_span", (0, 1))), tracker_parms.get("t_eval"), N)
    eq = LMAHeureuxPorosityDiff.from_scenario(pde_parms, device=device)
    y0 = eq.get_state(pde_parms["CAIni"], pde_parms["CCIni"], pde_parms["cCaIni"], pde_parms["cCO3Ini"],
                      pde_parms["PhiIni"]).ravel()

    method = solver_parms.pop("method", "RK45")
    t_span = tuple(solver_parms.pop("t_span", (0, 1)))
    t_eval = tracker_parms.get("t_eval")
    no_progress_updates = tracker_parms.get("no_progress_updates", 100_000)
    start = time.time()
    scipy_driver = bool(solver_parms.pop("scipy_driver", False))
    native_terminal = bool(solver_parms.pop("native_terminal", False))
    native_grid = bool(solver_parms.pop("native_grid", False))
    # A native route is chosen here and run once below: (the model's method, its arguments after y0 - None: the adaptive methods'
    # (t_span, first_step, rtol, atol, t_eval=) -, further keyword arguments, whether the limits go to the library first, the statuses
    # let through - None: all; 1: a terminal monitor ended the run at t_reached -, whether njev / nlu come from the result)
    native = None
    can_stop, cannot_stop = (0, 1, -1), (0, -1)
    if method == "RK4":
        # fixed-step classical RK4, the driver inside the kernel (marl_integrate_rk4_watch): terminal monitors are honoured directly, at
        # the end of the step of the occurrence; status -2: the state went non-finite, dt is too large
        native = (eq.integrate_rk4_watch, (rk4_dt, rk4_nsteps), {"t0": t_span[0], "frame_steps": rk4_frames}, True, None, False)
    elif method in ("RK45", "RK23") and not scipy_driver:
        if any(limits) and not native_terminal:
            eq.close()
            raise ValueError(f"terminal monitors in the {method} loop are opt-in: pass native_terminal=True in the solver parameters for "
                             "the native loop (marl_integrate_rk45_terminal / rk23_terminal) or scipy_driver=True for solve_ivp on the "
                             "HIP RHS, or use method 'Radau' or 'BDF'")
        if any(limits):
            integrate = eq.integrate_rk45_terminal if method == "RK45" else eq.integrate_rk23_terminal
        else:
            integrate = eq.integrate_rk45 if method == "RK45" else eq.integrate_rk23
        native = (integrate, None, {}, any(limits), can_stop, False)
    elif method == "DOP853" and not scipy_driver and N <= 1024 and not any(limits):
        # the native loop covers grids of one workgroup; with a terminal monitor it is opt-in (the next branch), and everything else
        # keeps the scipy route below
        native = (eq.integrate_dop853, None, {}, False, cannot_stop, False)
    elif method == "DOP853" and not scipy_driver and N <= 1024 and native_terminal:
        # a terminal monitor and native_terminal=True: the native loop stops itself (marl_integrate_dop853_stop)
        native = (eq.integrate_dop853_stop, None, {}, True, can_stop, False)
    elif method == "DOP853" and not scipy_driver and N > 1024 and native_grid and (native_terminal or not any(limits)):
        # a grid above one workgroup and native_grid=True: the large-grid loop, one launch per stage (marl_integrate_dop853_grid); it
        # stops itself at a terminal monitor's root, which stays opt-in (native_terminal=True) as everywhere
        native = (eq.integrate_dop853_grid, None, {}, True, can_stop, False)
    elif method in ("Radau", "BDF") and not scipy_driver:
        # the reference's default: the whole implicit loop on the GPU (marl_integrate_radau).  The Jacobian pattern is the
        # reference's (parameters.py:150-199); when the caller's jac_sparsity has the matching shape its scipy column grouping
        # is used, otherwise a structured colouring - the Jacobian entries are the same either way.
        groups = None
        sp = solver_parms.get("jac_sparsity")
        if sp is not None and getattr(sp, "shape", None) == (5 * N, 5 * N):
            from scipy.optimize._numdiff import group_columns
            from scipy.sparse import csc_matrix
            groups = group_columns(csc_matrix(sp))
        integrate = eq.integrate_radau if method == "Radau" else eq.integrate_bdf   # (marl_integrate_bdf: the same machinery, scipy's BDF step logic)
        native = (integrate, None, {"groups": groups}, True, can_stop, True)   # (stopped without t_eval: the state at the root is the last profile)
    else:
        from scipy.integrate import solve_ivp
        # the reference forwards every remaining Solver key to solve_ivp; keep only what the method takes
        drop = {"jac_sparsity"} if method == "LSODA" else {"lband", "uband"}
        if method not in ("Radau", "BDF", "LSODA"):
            drop |= {"jac_sparsity"}
        opts = {k: v for k, v in solver_parms.items() if k not in drop and v is not None}
        bar = _NoBar()
        args = [bar, (t_span[1] - t_span[0]) / no_progress_updates, t_span[0]]
        sol = solve_ivp(eq.fun, t_span, y0, method=method, t_eval=t_eval, events=_scipy_events(eq, limits), args=args, **opts)
        t_out, y_out, t_events = sol.t, sol.y, sol.t_events
        nfev, njev, nlu, status, message = sol.nfev, sol.njev, sol.nlu, sol.status, sol.message
        if status == 1:   # a terminal monitor ended the run at its root: the latest of the roots kept (ivp.py:696-704)
            covered = Tstar * max(float(te[-1]) for te in t_events if len(te))
        else:
            covered = Tstar * t_span[1] if status == 0 else bar.n * Tstar * t_span[1] / no_progress_updates
    if native is not None:
        integrate, args, more, stops, allowed, implicit = native
        if stops:
            eq.set_terminal(limits)
        if args is None:
            args, more = (t_span, solver_parms["first_step"], solver_parms["rtol"], solver_parms["atol"]), {"t_eval": t_eval, **more}
        res = integrate(y0, *args, **more)
        t_out, y_out, t_events = res.t, res.y, res.t_events
        nfev, njev, nlu = res.nfev, res.njev if implicit else 0, res.nlu if implicit else 0
        status, message = res.status if allowed is None or res.status in allowed else -1, res.message
        covered = Tstar * (t_span[1] if status == 0 else res.t_reached)
    wall = time.time() - start

    if verbose:
        print(f"rhs evaluations {nfev}, Jacobian evaluations {njev}, LU decompositions {nlu}, status {status}")
        for text, te in zip(EVENT_TEXT, t_events):
            print(f"times [years] at which {text}: " + ", ".join(f"{Tstar * x:.2f}" for x in te))
        print(f"solver message: {message}\nwall time {wall:.2e} s")

    field_solutions = np.asarray(y_out).reshape(5, N, -1)
    store_folder = None
    if results_root is not None:
        store_folder = os.path.join(results_root, datetime.now().strftime("%d_%m_%Y_%H_%M_%S") + "/")
        os.makedirs(store_folder, exist_ok=True)
        meta = {k: v for k, v in (solver_parms | {"method": method, "backend": backend, "t_span": t_span}
                                  | tracker_parms | pde_parms).items() if k != "jac_sparsity"}
        arrays = {"solutions": field_solutions, "times": np.asarray(t_out)}
        arrays |= {f"event_{i}": np.asarray(te) for i, te in enumerate(t_events)}
        np.savez(store_folder + "LMAHeureuxPorosityDiff.npz", **arrays,
                 **{"attr_" + k: np.asarray(v) for k, v in meta.items() if v is not None})
        try:
            import h5py
        except ImportError:
            h5py = None
        if h5py is not None:
            with h5py.File(store_folder + "LMAHeureuxPorosityDiff.hdf5", "w") as stored:
                for k, v in arrays.items():
                    stored.create_dataset(k, data=v)
                stored.attrs.update({k: v for k, v in meta.items() if v is not None})
    eq.close()
    return field_solutions[:, :, -1], covered, depths, Xstar, store_folder


def Plot_results(last_field_sol, covered_time, depths, Xstar, store_folder):
    """Final profiles against depth (reference :185-205); needs matplotlib."""
    import matplotlib
    matplotlib.use("AGG")
    import matplotlib.pyplot as plt
    fig, ax = plt.subplots()
    fig.suptitle(f"Distributions after {covered_time:.2e} years")
    x_cm = depths.axes_coords[0] * Xstar
    for row, marker, label in zip(last_field_sol, "v^><o", ("CA", "CC", "cCa", "cCO3", "Phi")):
        ax.plot(x_cm, row, marker, ms=5, label=label)
    ax.set_xlabel("Depth (cm)")
    ax.set_ylabel("Compositions and concentrations (dimensionless)")
    ax.legend(loc="upper right")
    fig.savefig((store_folder or "./") + "Final_distributions.pdf", bbox_inches="tight")


if __name__ == "__main__":
    from dataclasses import asdict, replace

    from .parameters import Map_Scenario, Solver, Tracker
    Plot_results(*integrate_equations(asdict(replace(Solver(), method="RK45")), asdict(Tracker()), asdict(Map_Scenario())))
