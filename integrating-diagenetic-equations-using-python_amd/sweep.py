"""Batched parameter sweeps: many independent model instances, sharded over the GPUs of a node.

Not in the reference (one scenario per process); BASELINE configs 3-4.  Instances are independent - own
parameters, own step-size controller - so ranks take contiguous index ranges and never communicate in the
data path ("replicas of the kernel").  On each GPU one workgroup integrates one instance
entirely on-chip (marl_kernels.h, rk45_sweep_kernel).  Results can be gathered to every rank afterwards
(control plane only).
"""
import os

import numpy as np


def shard(n_instances, rank, world):
    """Contiguous near-even split: the (begin, end) instance range of ``rank``."""
    return (n_instances * rank) // world, (n_instances * (rank + 1)) // world


def assign(n_instances, rank, world, mode="contiguous", cost=None):
    """The instance indices of ``rank`` (ascending) under one of three assignments - the same on every rank, no communication:

    ``contiguous``   the near-even index ranges of :func:`shard` (fixed-budget explicit sweeps: every instance costs the same)
    ``round_robin``  rank r takes r, r + world, r + 2 world, ...: a cost that varies smoothly along the axes of a parameter grid
                     (implicit solvers: the evaluations per scenario spread 20x, slowest where Phi0 and PhiIni are high) is spread
                     over all ranks instead of landing on the rank that owns that end of the grid
    ``cost``         longest-processing-time-first on the given per-instance cost estimates (largest first, each to the least
                     loaded rank; ties by lower rank, then by lower index): for callers who know their stragglers
    """
    if mode == "contiguous":
        lo, hi = shard(n_instances, rank, world)
        return list(range(lo, hi))
    if mode == "round_robin":
        return list(range(rank, n_instances, world))
    if mode == "cost":
        c = np.asarray(cost, dtype=float)
        if c.shape != (n_instances,):
            raise ValueError("assign: `cost` needs one estimate per instance")
        load = [0.0] * world
        mine = []
        for i in sorted(range(n_instances), key=lambda i: (-c[i], i)):
            r = min(range(world), key=lambda r: (load[r], r))
            load[r] += c[i]
            if r == rank:
                mine.append(i)
        return sorted(mine)
    raise ValueError(f"assign: unknown mode {mode!r}")


def implicit_cost_proxy(base_parms, instances):
    """A-priori cost estimate of an implicit (Radau / BDF) run of each scenario: the evaluations scipy's Radau needs on the reference's
    own cases grow from ~390 (Phi0 0.6 / PhiIni 0.5) to ~32 000 (Phi0 = PhiIni = 0.8, where the porosity passes its pole and W changes
    sign hundreds of times) - steeply in the larger of the two porosities.  A monotone guess, good enough to
    keep the heavy end of a grid from landing on one rank."""
    out = []
    for inst in instances:
        p = base_parms | inst
        out.append(1.0 + 80.0 * max(0.0, max(float(p["Phi0"]), float(p["PhiIni"])) - 0.7) ** 2 * 100.0)
    return np.array(out)


def product_grid(**axes):
    """Cartesian product of named parameter axes -> list of override dicts (last axis fastest)."""
    names = list(axes)
    grids = np.meshgrid(*[np.asarray(axes[k], dtype=float) for k in names], indexing="ij")
    return [dict(zip(names, (float(g.flat[i]) for g in grids))) for i in range(grids[0].size)]


def _sweep_with_frames(engine, sweep, y0, args, terminal, events, max_events, samples=None, names=("t_eval", "y_eval_dev_ptr"), **fixed):
    """The frame plumbing of every engine method: set ``terminal`` on the engine's model, upload ``y0`` ((n_local, 5N), already
    converted by the caller), call the model's ``sweep`` once - ``events`` / ``max_events`` are handed on only when roots are asked
    for, ``samples`` and a device buffer [n_local][max(len(samples), 1)][5N] for the frames under ``names`` only when samples are -
    and attach to every result the frames it reached, ``y`` (5N, len(t)).  Returns (y_final (n_local, 5N), the results).  Uses the
    engine's ``model``, ``torch`` and ``device`` only."""
    engine.model.set_terminal(terminal)
    sweep = getattr(engine.model, sweep)
    yd = engine.torch.from_numpy(y0).to(engine.device)
    more = dict(fixed, events=True, max_events=max_events) if events else dict(fixed)
    frames = None
    if samples is not None:
        frames = engine.torch.empty((yd.shape[0], max(int(np.size(samples)), 1), yd.shape[1]), dtype=yd.dtype, device=engine.device)
        more |= {names[0]: samples, names[1]: frames.data_ptr()}
    res = sweep(yd.data_ptr(), *args, **more)
    if frames is not None:
        frames = frames.cpu().numpy()
        for b, r in enumerate(res):
            r.y = frames[b, :len(r.t)].T.copy()
    return yd.cpu().numpy(), res


class HipSweepEngine:
    """The product engine: LMAHeureuxPorosityDiff with a batch of instances on one GPU."""

    def __init__(self, base_parms, instances, device):
        import torch
        self.torch = torch
        self.device = torch.device("cuda", device)
        self.base_parms, self.instances = dict(base_parms), [dict(i) for i in instances]
        self._model = None

    @property
    def model(self):
        """The batched model (device constants, controllers, arenas for all instances): built on first use - integrate_bdf without
        ``batched`` runs single-instance contexts and never needs it."""
        if self._model is None:
            from .LHeureux_model import LMAHeureuxPorosityDiff
            self._model = LMAHeureuxPorosityDiff.from_scenario(self.base_parms, device=self.device.index, instances=self.instances)
            self._model.use_stream(self.torch.cuda.current_stream(self.device).cuda_stream)
        return self._model

    def integrate_rk45(self, y0, t_span, first_step, rtol, atol, max_attempts, t_eval=None, events=False, max_events=64, terminal=None):
        """y0: (n_local, 5N) host array.  Returns (y_final (n_local, 5N), list of RK45Result).  With ``t_eval`` every result carries
        the samples that instance reached, as a single run's does: ``t`` (n_t,) and ``y`` (5N, n_t).  With ``events`` every result
        carries ``t_events``, the root times of the seven monitors located inside the sweep (at most ``max_events`` each).
        ``terminal`` as for :meth:`integrate_radau`: an instance whose terminal monitor occurs ends at that root inside the sweep
        kernel (marl_sweep_rk45_terminal_dev) - status 1, ``t_reached`` the root; None: none, whatever an earlier call set."""
        return self._integrate_rk("sweep_rk45_device", y0, t_span, first_step, rtol, atol, max_attempts, t_eval, events, max_events, terminal)

    def integrate_rk23(self, y0, t_span, first_step, rtol, atol, max_attempts, t_eval=None, events=False, max_events=64, terminal=None):
        """:meth:`integrate_rk45` with RK23 (marl_sweep_rk23_dev / _eval_dev / _events_dev / _terminal_dev): the same arguments and results."""
        return self._integrate_rk("sweep_rk23_device", y0, t_span, first_step, rtol, atol, max_attempts, t_eval, events, max_events, terminal)

    def integrate_dop853(self, y0, t_span, first_step, rtol, atol, max_attempts, t_eval=None, events=False, max_events=64, terminal=None):
        """:meth:`integrate_rk45` with DOP853 (marl_sweep_dop853_dev / _eval_dev / _events_dev; N <= 1024): the same arguments and
        results.  These entries do not stop: with ``terminal`` set the sweep is refused (:class:`marlpde_amd._abi.MarlError`);
        :meth:`integrate_dop853_stop` runs the entry that does (marl_sweep_dop853_stop_dev)."""
        return self._integrate_rk("sweep_dop853_device", y0, t_span, first_step, rtol, atol, max_attempts, t_eval, events, max_events, terminal)

    def integrate_dop853_stop(self, y0, t_span, first_step, rtol, atol, max_attempts, t_eval=None, events=False, max_events=64, terminal=None):
        """:meth:`integrate_dop853` with ``terminal`` honoured as :meth:`integrate_rk45` honours it: an instance whose terminal monitor
        occurs ends at that root inside the sweep kernel (marl_sweep_dop853_stop_dev) - status 1, ``t_reached`` the root."""
        return self._integrate_rk("sweep_dop853_stop_device", y0, t_span, first_step, rtol, atol, max_attempts, t_eval, events, max_events, terminal)

    def _integrate_rk(self, sweep, y0, t_span, first_step, rtol, atol, max_attempts, t_eval, events, max_events, terminal=None):
        return _sweep_with_frames(self, sweep, np.ascontiguousarray(y0), (t_span, first_step, rtol, atol, max_attempts), terminal, events, max_events,
                                  t_eval)

    def integrate_radau(self, y0, t_span, first_step, rtol, atol, max_attempts, t_eval=None, events=False, max_events=64, terminal=None):
        """The reference's default solver over the shard: every instance its own Radau step logic, advanced together on the device
        (marl_sweep_radau_dev).  Returns (y_final (n_local, 5N), list of RK45Result); ``t_eval`` and ``events`` as for
        :meth:`integrate_rk45` (marl_sweep_radau_eval_dev: samples and roots on the accepted step's dense output, inside the sweep).
        ``terminal`` (see :func:`marlpde_amd.LHeureux_model.terminal_counts`): monitors that end an instance's run at their root -
        status 1, ``t_reached`` the root, the state the dense output there; None: none, whatever an earlier call set."""
        return _sweep_with_frames(self, "sweep_radau_device", np.ascontiguousarray(y0), (t_span, first_step, rtol, atol, max_attempts), terminal, events,
                                  max_events, t_eval)

    def integrate_bdf(self, y0, t_span, first_step, rtol, atol, max_attempts, workers=None, batched=False, t_eval=None, events=False,
                      max_events=64, terminal=None):
        """scipy BDF semantics (the other implicit method of the reference's Solver, marlpde/parameters.py:205-219) for every instance of
        the shard.  By default the instances run as concurrent SINGLE runs (marl_integrate_bdf, one context and one HIP stream per worker
        thread - ctypes releases the GIL, and a single BDF run of a small grid leaves the GPU mostly idle between its small launches),
        so each instance is bit for bit the single run.  ``batched=True`` runs the shard through the batched kernel set instead
        (marl_sweep_bdf_dev on the batched model, as :meth:`integrate_radau`: per-instance step control on the device, every launch
        over all instances that need that work; N <= 409): the same decisions up to the controller's scalar arithmetic.
        Returns (y_final (n_local, 5N), list of RK45Result).  With ``t_eval`` every result carries the samples that instance
        reached, ``t`` (n_t,) and ``y`` (5N, n_t), either way: the single runs take them from their own dense output, the batched
        sweep writes them inside the sweep (marl_sweep_bdf_eval_dev), as :meth:`integrate_radau` does.  With ``events`` every result
        carries ``t_events``, the root times of the seven monitors (at most ``max_events`` each), either way too: the batched sweep
        locates them inside the sweep (marl_sweep_bdf_events_dev), the single runs' are cut to ``max_events``.
        ``terminal`` as for :meth:`integrate_radau`, either way: the batched sweep stops an instance on the device
        (marl_sweep_bdf_terminal_dev), the single runs stop themselves (marl_integrate_bdf); None: none, whatever an earlier call set."""
        if batched:
            return _sweep_with_frames(self, "sweep_bdf_device", np.ascontiguousarray(y0, dtype=np.float64), (t_span, first_step, rtol, atol, max_attempts),
                                      terminal, events, max_events, t_eval)
        from concurrent.futures import ThreadPoolExecutor
        from .LHeureux_model import LMAHeureuxPorosityDiff
        torch = self.torch
        y0 = np.ascontiguousarray(y0, dtype=np.float64)
        n_inst = len(self.instances)
        workers = max(1, min(n_inst, workers or min(16, os.cpu_count() or 1)))
        out = [None] * n_inst
        yf = np.empty_like(y0)

        def work(w):
            stream = torch.cuda.Stream(device=self.device)
            one = None
            try:
                for b in range(w, n_inst, workers):
                    p = self.base_parms | self.instances[b]
                    if one is None:   # one context per worker; later scenarios only replace its constants (marl_ctx_set_params)
                        one = LMAHeureuxPorosityDiff.from_scenario(p, device=self.device.index)
                        one.use_stream(stream.cuda_stream)
                    else:
                        one.set_scenario(p)
                    one.set_terminal(terminal)
                    r = one.integrate_bdf(y0[b], t_span, first_step, rtol, atol, t_eval=t_eval, max_attempts=max_attempts)
                    if events:
                        r.t_events = [t[:max(int(max_events), 0)] for t in r.t_events]
                    out[b] = r
                    yf[b] = r.y_final
            finally:
                if one is not None:
                    one.close()

        with ThreadPoolExecutor(max_workers=workers) as pool:
            for f in [pool.submit(work, w) for w in range(workers)]:
                f.result()
        return yf, out

    def integrate_rk4(self, y0, dt, nsteps):
        yd = self.torch.from_numpy(np.ascontiguousarray(y0)).to(self.device)
        self.model.sweep_rk4_device(yd.data_ptr(), dt, nsteps)
        self.torch.cuda.synchronize(self.device)
        return yd.cpu().numpy()

    def integrate_rk4_watch(self, y0, dt, nsteps, t0=0.0, frame_steps=None, events=False, max_events=64, terminal=None):
        """Fixed-step RK4 with the driver inside the kernel (marl_sweep_rk4_watch_dev; N <= 1024): y0 (n_local, 5N) host array, ``dt`` a
        scalar or one per local instance.  Returns (y_final (n_local, 5N), list of RK45Result) like :meth:`integrate_rk45`: with
        ``frame_steps`` every result carries the frames that instance reached, ``t`` (n_t,) and ``y`` (5N, n_t); with ``events`` the
        root estimates ``t_events``.  ``terminal`` as for :meth:`integrate_radau`, by the fixed-step rule: the instance ends at the END
        of the step of the terminal occurrence (status 1).  Status -2: the state went non-finite, the step is too large."""
        return _sweep_with_frames(self, "sweep_rk4_watch_device", np.ascontiguousarray(y0, dtype=np.float64), (dt, nsteps), terminal, events, max_events,
                                  frame_steps, names=("frame_steps", "frames_dev_ptr"), t0=t0)

    def close(self):
        if self._model is not None:
            self._model.close()
            self._model = None


def initial_states(base_parms, instances):
    """Uniform initial state per instance (marlpde/Evolve_scenario.py:76-86), shape (n, 5N)."""
    N = int(base_parms["N"])
    out = np.empty((len(instances), 5 * N))
    for i, inst in enumerate(instances):
        p = base_parms | inst
        out[i] = np.repeat([p["CAIni"], p["CCIni"], p["cCaIni"], p["cCO3Ini"], p["PhiIni"]], N)
    return out


def run_sweep_radau(base_parms, instances, t_span, first_step, rtol, atol, max_attempts=0, y0=None, group=None,
                    device=None, engine_factory=None, gather=True, balance="cost", cost=None, t_eval=None, events=False, max_events=64,
                    terminal=None):
    """As :func:`run_sweep_rk45` with the reference's DEFAULT solver (scipy Radau semantics, marlpde/parameters.py:213): what the
    reference does one scenario per process (its tests loop over scenarios), spread over the ranks with no data-path collective.
    An implicit run's cost depends on the scenario (20x between the fastest and the slowest of a parameter grid), and the slowest
    rank sets the wall time: ``balance`` = ``"cost"`` (default: :func:`assign` by ``cost``, or by :func:`implicit_cost_proxy` when
    none is given), ``"round_robin"`` or ``"contiguous"``.  Results come back in the order of ``instances`` whatever the assignment.
    ``t_eval``, ``events``, ``max_events`` and what they add to the returned tuple: as documented for :func:`run_sweep_rk45`.
    ``terminal`` (the reference's switch, marlpde/LHeureux_model.py:113-122; see :func:`marlpde_amd.LHeureux_model.terminal_counts`):
    an instance whose terminal monitor fires ends there - ``status`` 1, ``t_reached`` the root - and stops bounding the sweep."""
    return _run_sweep("integrate_radau", base_parms, instances, t_span, first_step, rtol, atol, max_attempts, y0, group, device, engine_factory, gather,
                      balance, cost, t_eval, events, max_events, terminal=terminal)


def run_sweep_bdf(base_parms, instances, t_span, first_step, rtol, atol, max_attempts=0, y0=None, group=None,
                  device=None, engine_factory=None, gather=True, balance="cost", cost=None, batched=False, t_eval=None, events=False,
                  max_events=64, terminal=None):
    """As :func:`run_sweep_radau` with scipy's BDF semantics; on a GPU the rank's instances run as concurrent single runs, or with
    ``batched=True`` (N <= 409) through the batched BDF kernels, all instances advanced together
    (:meth:`HipSweepEngine.integrate_bdf`).  ``batched``, ``t_eval``, ``events`` and ``max_events`` reach the engine only when asked
    for; with ``t_eval`` two more elements follow, ``n_frames`` and ``y_eval``, and with ``events`` one last element, ``t_events``, as
    documented for :func:`run_sweep_rk45` (either way of running the shard).  ``terminal``: as for :func:`run_sweep_radau`, either way
    of running the shard too; it reaches the engine only when given."""
    return _run_sweep("integrate_bdf", base_parms, instances, t_span, first_step, rtol, atol, max_attempts, y0, group, device, engine_factory, gather,
                      balance, cost, t_eval, events, max_events, batched=batched, terminal=terminal)


def run_sweep_rk45(base_parms, instances, t_span, first_step, rtol, atol, max_attempts=0, y0=None, group=None,
                   device=None, engine_factory=None, gather=True, balance="contiguous", cost=None, t_eval=None, events=False, max_events=64,
                   terminal=None):
    """Integrate every instance with adaptive RK45; ranks of ``group`` each take a contiguous shard (``balance``: see :func:`assign`).

    Returns ``(y_final, status, n_accepted, n_rejected, t_reached)`` - for ALL instances, in their order, when ``gather``,
    otherwise for the rank's own instances (``assign(...)`` order).  ``engine_factory(base_parms, local_instances) -> engine`` is
    the test hook; the default is :class:`HipSweepEngine` on ``cuda:rank``.

    With ``t_eval`` (sorted sample times within ``t_span``, the same for every instance) two more elements follow: ``n_frames``, the
    number of samples each instance reached, and ``y_eval`` of shape (instances, len(t_eval), 5N), the time series
    ``solve_ivp(..., t_eval=)`` returns (Evolve_scenario.py:104-109) - NaN beyond an instance's ``n_frames``; ordered like the states.

    With ``events`` one last element follows: ``t_events``, per instance a list of 7 arrays - the root times of the reference's monitors
    (Evolve_scenario.py:118-145, 175-177), at most ``max_events`` each, located inside the sweep; ordered like the states.

    ``terminal``: as for :func:`run_sweep_radau` - set for this call only, and handed to the engine only when given."""
    return _run_sweep("integrate_rk45", base_parms, instances, t_span, first_step, rtol, atol, max_attempts, y0, group, device, engine_factory, gather,
                      balance, cost, t_eval, events, max_events, terminal=terminal)


def run_sweep_rk23(base_parms, instances, t_span, first_step, rtol, atol, max_attempts=0, y0=None, group=None,
                   device=None, engine_factory=None, gather=True, balance="contiguous", cost=None, t_eval=None, events=False, max_events=64,
                   terminal=None):
    """As :func:`run_sweep_rk45` with adaptive RK23 (scipy's Bogacki-Shampine 3(2) pair; every instance costs about the same, so
    contiguous shards): the same arguments and the same returned tuple, ``t_eval``, ``events`` and ``terminal`` included."""
    return _run_sweep("integrate_rk23", base_parms, instances, t_span, first_step, rtol, atol, max_attempts, y0, group, device, engine_factory, gather,
                      balance, cost, t_eval, events, max_events, terminal=terminal)


def run_sweep_dop853(base_parms, instances, t_span, first_step, rtol, atol, max_attempts=0, y0=None, group=None,
                     device=None, engine_factory=None, gather=True, balance="contiguous", cost=None, t_eval=None, events=False, max_events=64,
                     terminal=None):
    """As :func:`run_sweep_rk45` with adaptive DOP853 (scipy's Dormand-Prince 8(5,3); grids of up to 1024 cells): the same arguments
    and the same returned tuple, ``t_eval`` and ``events`` included.  ``terminal`` is handed on and refused by the entries, which
    cannot stop at a monitor's root."""
    return _run_sweep("integrate_dop853", base_parms, instances, t_span, first_step, rtol, atol, max_attempts, y0, group, device, engine_factory, gather,
                      balance, cost, t_eval, events, max_events, terminal=terminal)


def run_sweep_dop853_stop(base_parms, instances, t_span, first_step, rtol, atol, max_attempts=0, y0=None, group=None,
                          device=None, engine_factory=None, gather=True, balance="contiguous", cost=None, t_eval=None, events=False,
                          max_events=64, terminal=None):
    """As :func:`run_sweep_dop853` with ``terminal`` honoured, as :func:`run_sweep_rk45` honours it: an instance whose terminal
    monitor fires ends there - ``status`` 1, ``t_reached`` the root.  The same arguments and the same returned tuple."""
    return _run_sweep("integrate_dop853_stop", base_parms, instances, t_span, first_step, rtol, atol, max_attempts, y0, group, device, engine_factory,
                      gather, balance, cost, t_eval, events, max_events, terminal=terminal)


def run_sweep_rk4(base_parms, instances, dt, nsteps, t0=0.0, y0=None, group=None, device=None, engine_factory=None, gather=True,
                  balance="contiguous", cost=None, frame_steps=None, events=False, max_events=64, terminal=None):
    """As :func:`run_sweep_rk45` with fixed-step classical RK4 and the driver inside the kernel (grids of up to 1024 cells;
    :meth:`HipSweepEngine.integrate_rk4_watch`): ``nsteps`` steps of ``dt`` - a scalar or one per instance - from ``t0``; every instance
    costs the same, so contiguous shards.  The returned tuple has the layout of :func:`run_sweep_rk45`:
    ``(y_final, status, n_steps, zeros, t_reached)``; with ``frame_steps`` (strictly ascending step counts in [0, nsteps], the same for
    every instance) ``n_frames`` and ``y_frames`` of shape (instances, len(frame_steps), 5N) follow - frame j the state after
    ``frame_steps[j]`` steps, NaN beyond an instance's ``n_frames``; with ``events`` one last element, ``t_events``: the secant estimates
    of the monitors' sign changes (no dense output: O(dt^2) from the root), at most ``max_events`` each.
    ``status``: 0, 1 - a terminal monitor (``terminal``, handed to the engine only when given) ended the instance at the END of the step
    of its occurrence - or -2: the state went non-finite after ``n_steps`` steps, ``dt`` is too large for that instance."""
    dts = np.ascontiguousarray(np.broadcast_to(np.asarray(dt, dtype=np.float64), (len(instances),)))
    fs = None if frame_steps is None else np.ascontiguousarray(frame_steps, dtype=np.int64).ravel()

    def call(engine, y0_local, mine, more):
        kw = {k: v for k, v in more.items() if k != "t_eval"}
        if fs is not None:
            kw["frame_steps"] = fs
        return engine.integrate_rk4_watch(y0_local, dts[mine], int(nsteps), t0=t0, **kw)

    return _run_sweep("integrate_rk4_watch", base_parms, instances, None, None, None, None, 0, y0, group, device, engine_factory, gather,
                      balance, cost, fs, events, max_events, terminal=terminal, call=call)


def _run_sweep(method, base_parms, instances, t_span, first_step, rtol, atol, max_attempts, y0, group, device, engine_factory, gather,
               balance="contiguous", cost=None, t_eval=None, events=False, max_events=64, batched=False, terminal=None, call=None):
    import torch.distributed as dist
    on = dist.is_available() and dist.is_initialized()
    rank = dist.get_rank(group) if on else 0
    world = dist.get_world_size(group) if on else 1
    if balance == "cost" and cost is None:
        cost = implicit_cost_proxy(base_parms, instances)
    mine = assign(len(instances), rank, world, balance, cost)
    local = [instances[i] for i in mine]
    if y0 is None:
        y0 = initial_states(base_parms, instances)
    if engine_factory is None:
        dev = int(os.environ.get("LOCAL_RANK", rank)) if device is None else device   # one process per GPU
        engine_factory = lambda bp, inst: HipSweepEngine(bp, inst, dev)  # noqa: E731
    y0 = np.asarray(y0)
    sampled = t_eval is not None
    if sampled:
        t_eval = np.ascontiguousarray(t_eval, dtype=np.float64).ravel()
    if local:
        engine = engine_factory(base_parms, local)
        more = {"t_eval": t_eval} if sampled else {}
        if events:   # (passed only when asked for: engines without root location keep working)
            more |= {"events": True, "max_events": max_events}
        if batched:   # (the BDF driver; passed only when asked for, like `events`)
            more |= {"batched": True}
        if terminal is not None:   # (passed only when asked for)
            more |= {"terminal": terminal}
        if call is not None:   # (run_sweep_rk4: a fixed-step engine method takes other arguments; t_eval stands for its frame list)
            y, res = call(engine, y0[mine], mine, more)
        else:
            y, res = getattr(engine, method)(y0[mine], t_span, first_step, rtol, atol, max_attempts, **more)
        engine.close()
    else:   # (more ranks than instances)
        y, res = np.empty((0,) + y0.shape[1:]), []
    summary = np.array([[r.status, r.n_accepted, r.n_rejected, r.t_reached] for r in res], dtype=float).reshape(len(local), 4)
    frames = None
    if sampled:   # the rank's time series: column 4 of the summary counts an instance's frames, the rest of its rows stay NaN
        frames = np.full((len(local), t_eval.size) + y0.shape[1:], np.nan)
        for b, r in enumerate(res):
            frames[b, :len(r.t)] = np.asarray(r.y).T
        summary = np.concatenate([summary, np.array([len(r.t) for r in res], dtype=float).reshape(len(local), 1)], axis=1)
    roots = [[np.asarray(t) for t in (r.t_events or [np.empty(0)] * 7)] for r in res] if events else None   # (max_events = 0: none located)
    if gather and world > 1:
        parts = [None] * world
        dist.all_gather_object(parts, (mine, y, summary, frames, roots), group=group)
        y_all = np.empty((len(instances),) + y0.shape[1:])
        s_all = np.empty((len(instances), summary.shape[1]))
        f_all = np.full((len(instances), t_eval.size) + y0.shape[1:], np.nan) if sampled else None
        r_all = [None] * len(instances) if events else None
        for idx, yy, ss, ff, rr in parts:   # back into the order of `instances`
            y_all[idx] = yy
            s_all[idx] = ss
            if sampled:
                f_all[idx] = ff
            if events:
                for i, r in zip(idx, rr):
                    r_all[i] = r
        y, summary, frames, roots = y_all, s_all, f_all, r_all
    out = (y, summary[:, 0].astype(int), summary[:, 1].astype(int), summary[:, 2].astype(int), summary[:, 3])
    if sampled:
        out = out + (summary[:, 4].astype(int), frames)
    return out + (roots,) if events else out
