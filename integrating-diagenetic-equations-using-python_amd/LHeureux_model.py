"""The five-field L'Heureux (2018) model on the MI355X - host-side mirror of ``marlpde/LHeureux_model.py``.

``LMAHeureuxPorosityDiff`` keeps the reference class's constructor keywords (LHeureux_model.py:12-16),
its RHS callables ``fun`` / ``fun_numba`` with the ``(t, y, progress_proxy, progress_dt, t0)`` signature
(:162, :290) and its seven event functions (:524-593), but every one of them runs a HIP kernel through
the C ABI (include/marl_hip.h).  The py-pde grid object the reference passes as ``Depths`` is replaced
by :class:`DepthGrid` (cell-centred 1-D grid; the only things the reference reads from it are the cell
count, the spacing and the cell centres, :23-24, :322).

A model may hold a whole batch of parameter sets (a sweep): pass a list of keyword dicts to
:meth:`LMAHeureuxPorosityDiff.batch`.

There is no CPU implementation in this package; without libmarl_hip.so and a GPU construction fails.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _abi
from ._abi import LAYOUT_FIELD_MAJOR, LAYOUT_TILED, MarlParams, MarlStats, NEVENTS

FIELD_NAMES = ("CA", "CC", "cCa", "cCO3", "Phi")  # order of the state vector (Evolve_scenario.py:76-86)
LABELS = ("ARA", "CAL", "Ca", "CO3", "Po")        # labels of get_state (LHeureux_model.py:138-142)


@dataclass(frozen=True)
class DepthGrid:
    """Cell-centred grid on [0, length] with N cells (stands in for pde.CartesianGrid, Evolve_scenario.py:40)."""
    length: float
    N: int

    @property
    def shape(self):
        return (self.N,)

    @property
    def discretization(self):
        return np.array([self.length / self.N])

    @property
    def axes_coords(self):
        return ((np.arange(self.N) + 0.5) * (self.length / self.N),)

    _axes_coords = axes_coords


def _as_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class RK45Result:
    """What the reference reads off scipy's OdeResult (Evolve_scenario.py:112-178), for one instance."""

    def __init__(self, stats, t=None, y=None, t_events=None):
        self.nfev = int(stats.nfev)
        self.njev = int(stats.njev)
        self.nlu = int(stats.nlu)
        self.n_accepted = int(stats.n_accepted)
        self.n_rejected = int(stats.n_rejected)
        # library status -> scipy status: 0 finished; 1 a terminal monitor ended the run; -1 step size too small; 2 attempt budget
        # (no scipy analogue)
        self.status = int(stats.status)
        self.success = self.status == 0
        self.message = {0: "The solver successfully reached the end of the integration interval.",
                        1: "A termination event occurred.",
                        -1: "Required step size is less than spacing between numbers.",
                        2: "Attempt budget exhausted before the end of the interval.",
                        -2: "The state became non-finite: the fixed step is too large."}.get(self.status, "?")
        self.t_reached = float(stats.t)
        self.h_next = float(stats.h_next)
        self.event_values = np.array(stats.event_value[:])
        self.n_events = np.array(stats.n_events[:])
        self.t = t
        self.y = y
        self.t_events = t_events


EVENT_NAMES = ("zeros", "zeros_CA", "zeros_CC", "ones_CA_plus_CC", "ones_Phi", "zeros_U", "zeros_W")   # Evolve_scenario.py:107-109


def terminal_counts(spec):
    """The limits marl_set_terminal takes, a tuple of 7 ints, from what a user of the reference would write (its switch:
    LHeureux_model.py:113-122).  ``spec``: None (no monitor is terminal: the reference's setting), a sequence of 7 bools / ints in the
    monitors' order, or a dict keyed by the monitors' names ``zeros ... zeros_W``.  As scipy >= 1.13 reads ``event.terminal``: False
    or 0 - the monitor only records; True - the run ends at its first occurrence; an int k > 0 - at its k-th.  A pure function."""
    def one(v, what):
        if isinstance(v, (bool, np.bool_)):
            return int(v)
        if not isinstance(v, (int, np.integer)):
            raise ValueError(f"terminal: {what} must be a bool or an int, not {v!r}")
        if v < 0:
            raise ValueError(f"terminal: {what} is negative ({v}); 0 never stops, k > 0 stops at the k-th occurrence")
        return int(v)

    if spec is None:
        return (0,) * NEVENTS
    if isinstance(spec, dict):
        unknown = [k for k in spec if k not in EVENT_NAMES]
        if unknown:
            raise ValueError(f"terminal: unknown monitors {unknown}; the monitors are {list(EVENT_NAMES)}")
        return tuple(one(spec.get(name, 0), name) for name in EVENT_NAMES)
    spec = list(spec)
    if len(spec) != NEVENTS:
        raise ValueError(f"terminal: {len(spec)} entries, expected {NEVENTS} (one per monitor) or a dict keyed by monitor names")
    return tuple(one(v, name) for v, name in zip(spec, EVENT_NAMES))


# -- the one marshalling of the integrators' entries ------------------------------------------------------------------------------------
# Plain functions of a model-like object `m`: they use its _lib, _ctx, _check, n_instances and terminal only, so that tests can run
# them on stand-ins.  A new solver family chooses its entry ("The Python host layer") and calls these.
def _run_head(m, y_ptr, t_span, first_step, rtol, atol):
    """What every adaptive entry's argument list begins with."""
    return (m._ctx, y_ptr, float(t_span[0]), float(t_span[1]), float(first_step), float(rtol), float(atol))


def _groups(groups, n=None):
    """The column-grouping argument of the implicit entries: a pointer to the int32 array, which it keeps alive (None: the library's
    structured colouring).  ``n``: the number of entries to insist on."""
    if groups is None:
        return None
    grp = np.ascontiguousarray(groups, dtype=np.int32)
    if n is not None and grp.size != n:
        raise ValueError(f"groups has {grp.size} entries, expected {n}")
    return _as_ptr(grp)


def _root_buffer(shape, max_events):
    return np.full(shape + (NEVENTS, int(max_events)), np.nan)


def _root_times(tev, n_events):
    """The seven arrays of root times an entry left in its rows of ``tev``: ``min(n_events[e], max_events)`` each."""
    return [tev[e, :min(int(n_events[e]), tev.shape[1])].copy() for e in range(NEVENTS)]


def _sweep_results(stats, te=None, n_done=None, tev=None):
    """One :class:`RK45Result` per instance of a sweep: ``t`` the samples ``te[:n_done[b]]`` it reached (None without ``te``),
    ``t_events`` its root times (None without the root buffer ``tev``)."""
    return [RK45Result(s, t=None if te is None else te[:int(n_done[b])].copy(), t_events=None if tev is None else _root_times(tev[b], s.n_events))
            for b, s in enumerate(stats)]


def _sweep_call(m, family, entry, head, takes, t_eval=None, y_eval_dev_ptr=None, tev=None):
    """Call the sweep entry ``entry`` and build its results.  ``head``: the arguments up to ``max_attempts``.  ``takes`` says which
    argument groups the entry has between ``head`` and ``stats``: "samples" - (t_eval, n_eval, y_eval, n_frames), None / 0 / None
    where ``t_eval`` is None or empty; "roots" - (t_events, max_events) from the root buffer ``tev``, None / 0 without one."""
    B = m.n_instances
    stats = (MarlStats * B)()
    args, te, n_done = list(head), None, None
    if "samples" in takes:
        te = np.empty(0) if t_eval is None else np.ascontiguousarray(t_eval, dtype=np.float64).ravel()
        if te.size and not y_eval_dev_ptr:
            raise ValueError(f"sweep_{family}_device: t_eval needs y_eval_dev_ptr, device memory [instances][len(t_eval)][5N]")
        n_done = np.zeros(B, dtype=np.int64)
        args += [_as_ptr(te) if te.size else None, te.size, C.c_void_p(y_eval_dev_ptr) if te.size else None, _as_ptr(n_done)]
    if "roots" in takes:
        args += [_as_ptr(tev), tev.shape[2]] if tev is not None else [None, 0]
    m._check(getattr(m._lib, entry)(*args, stats), entry)
    return _sweep_results(stats, None if t_eval is None else te, n_done, tev)


def _sweep_choose(m, family, terminal_entry, head, t_eval, y_eval_dev_ptr, events, max_events):
    """The entry choice of the explicit families and BDF.  While a monitor is terminal: ``terminal_entry``, where the family has one
    (else the entries below, which refuse the call).  Otherwise marl_sweep_<family>_dev when there is neither ``t_eval`` nor a root to
    locate (``events`` with room for one), _events_dev when roots are to be located, _eval_dev when not."""
    locate = bool(events) and int(max_events) > 0
    if terminal_entry and any(m.terminal):
        entry, takes = terminal_entry, ("samples", "roots")
    elif t_eval is None and not locate:
        entry, takes = f"marl_sweep_{family}_dev", ()
    elif locate:
        entry, takes = f"marl_sweep_{family}_events_dev", ("samples", "roots")
    else:
        entry, takes = f"marl_sweep_{family}_eval_dev", ("samples",)
    return _sweep_call(m, family, entry, head, takes, t_eval, y_eval_dev_ptr, _root_buffer((m.n_instances,), max_events) if locate else None)


def _with_room(run, max_events):
    """``run(max_events) -> (what it made, the largest sign-change count)``, repeated with a larger root buffer until every root time
    fits: solve_ivp returns EVERY root time (a monitor sitting at exactly 0 fires on every accepted step), and the run is
    deterministic.  Returns what the last run made."""
    while True:
        made, most = run(max_events)
        if most <= max_events:
            return made
        max_events = int(most)


def _single_result(stats, y, t_events, t=None, frames=None):
    """The :class:`RK45Result` of a single run that ended in state ``y``: the samples ``t`` / ``frames`` (rows) it reached or, without
    them, the end point only."""
    res = RK45Result(stats, np.array([stats.t]), y[:, None].copy(), t_events) if t is None else RK45Result(stats, t, frames.T.copy(), t_events)
    res.y_final = y
    return res


def _single_run(m, entry, y_start, t_span, first_step, rtol, atol, t_eval, events, max_events, max_attempts, grp=()):
    """The single-run driver of every adaptive entry (``grp``: the implicit entries' groups argument, as a 1-tuple)."""
    n = y_start.size
    te = None if t_eval is None else np.ascontiguousarray(t_eval, dtype=np.float64)
    n_eval = 0 if te is None else te.size

    def run(max_events):
        y, stats, y_eval = y_start.copy(), MarlStats(), np.empty((max(n_eval, 1), n))
        tev = _root_buffer((), max_events) if events else None
        rc = getattr(m._lib, entry)(
            *_run_head(m, _as_ptr(y), t_span, first_step, rtol, atol), *grp, _as_ptr(te) if n_eval else None, n_eval,
            _as_ptr(y_eval) if n_eval else None, _as_ptr(tev) if events else None, max_events if events else 0, int(max_attempts), C.byref(stats))
        m._check(rc, entry)
        return (y, stats, y_eval, tev), max(stats.n_events[:]) if events else 0

    y, stats, y_eval, tev = _with_room(run, max_events)
    t_events = _root_times(tev, stats.n_events) if events else None
    if not n_eval:
        return _single_result(stats, y, t_events)
    k = int(np.searchsorted(te, stats.t, side="right"))
    return _single_result(stats, y, t_events, te[:k].copy(), y_eval[:k])


def pack_blocks(instances, length):
    """The marl_params blocks (include/marl_params.h) of a list of instances (constructor-keyword dicts) on a column of `length`:
    what marl_ctx_create / marl_ctx_set_params receive.  A pure function of its arguments - a rank's blocks are the corresponding
    blocks of the unsharded sweep (tests/test_multi_rank_cpu.py)."""
    blocks = (MarlParams * len(instances))()
    for blk, inst in zip(blocks, instances):
        for name in _abi.PARAM_DOUBLES[:30]:
            setattr(blk, name, float(inst[name]))
        blk.length = float(length)
        blk.shallow_limit = float(inst["ShallowLimit"]) / float(inst["Xstar"])
        blk.deep_limit = float(inst["DeepLimit"]) / float(inst["Xstar"])
        blk.FV_switch = int(inst["FV_switch"])
        blk.dPhi_variable = int(bool(inst.get("dPhi_variable", False)))
    return blocks


def instance_kwargs(pde_parms, instances):
    """Constructor keywords of every instance of a sweep: the scenario dict overridden by each instance's entries, reduced to what the
    constructor takes (what :meth:`LMAHeureuxPorosityDiff.from_scenario` passes on)."""
    import inspect
    names = {p for p in inspect.signature(LMAHeureuxPorosityDiff.__init__).parameters} - {"self", "Depths", "device"}
    sig = inspect.signature(LMAHeureuxPorosityDiff.__init__).parameters
    defaults = {k: sig[k].default for k in names if sig[k].default is not inspect.Parameter.empty and not k.startswith("_")
                and k not in ("slices_all_fields", "not_too_shallow", "not_too_deep")}
    return [defaults | {k: v for k, v in (pde_parms | inst).items() if k in names} for inst in instances]


class LMAHeureuxPorosityDiff:
    """Model object: parameters on the device + the callables scipy / the integrators need."""

    no_fields = 5

    def __init__(self, Depths, slices_all_fields=None, not_too_shallow=None, not_too_deep=None, *,
                 CA0, CC0, cCa0, cCO30, Phi0, sedimentationrate, Xstar, Tstar, k1, k2, k3, k4, m1, m2, n1, n2,
                 b, beta, rhos, rhow, rhos0, KA, KC, muA, D0Ca, PhiNR, PhiInfty, PhiIni, DCa, DCO3, FV_switch,
                 ShallowLimit=50.0, DeepLimit=150.0, dPhi_variable=False, device=0, _extra_instances=()):
        """Same keywords as the reference constructor.  ``not_too_shallow`` / ``not_too_deep`` (py-pde mask
        fields in the reference) are replaced by the two numbers that define them, ``ShallowLimit`` and
        ``DeepLimit`` in cm (Evolve_scenario.py:51-54); ``slices_all_fields`` is implied by N.
        ``dPhi_variable=True`` switches from the reference's fixed porosity diffusion coefficient (:124-133, :431) to
        the time-varying one, auxcon F Phi^3/(1-Phi), that the reference keeps commented out (:222-223, :430)."""
        if not isinstance(Depths, DepthGrid):
            raise TypeError("Depths must be a DepthGrid(length=max_depth/Xstar, N=number of cells)")
        if not_too_shallow is not None or not_too_deep is not None:
            raise TypeError("pass ShallowLimit / DeepLimit (cm) instead of mask fields")
        self.Depths = Depths
        N = Depths.N
        self.slices_all_fields = slices_all_fields or [slice(i * N, (i + 1) * N) for i in range(5)]
        (self.CA_sl, self.CC_sl, self.cCa_sl, self.cCO3_sl, self.Phi_sl) = self.slices_all_fields
        first = dict(CA0=CA0, CC0=CC0, cCa0=cCa0, cCO30=cCO30, Phi0=Phi0, sedimentationrate=sedimentationrate,
                     Xstar=Xstar, Tstar=Tstar, k1=k1, k2=k2, k3=k3, k4=k4, m1=m1, m2=m2, n1=n1, n2=n2, b=b,
                     beta=beta, rhos=rhos, rhow=rhow, rhos0=rhos0, KA=KA, KC=KC, muA=muA, D0Ca=D0Ca,
                     PhiNR=PhiNR, PhiInfty=PhiInfty, PhiIni=PhiIni, DCa=DCa, DCO3=DCO3, FV_switch=FV_switch,
                     ShallowLimit=ShallowLimit, DeepLimit=DeepLimit, dPhi_variable=bool(dPhi_variable))
        self.instances = [first, *_extra_instances]
        for k, v in first.items():   # the reference exposes its parameters as attributes
            setattr(self, k, v)
        self.last_t = 0.0            # progress-bar helper of the reference (:90)
        self.device = int(device)
        self._lib = _abi.load()
        self._ctx = C.c_void_p()
        blocks = self._pack_blocks()
        rc = self._lib.marl_ctx_create(blocks, len(self.instances), N, self.device, C.byref(self._ctx))
        if rc != 0:
            self._ctx = C.c_void_p()
            _abi.check(None, rc, "marl_ctx_create")
        for name, value in _abi.lab_options():   # (kernel-lab A/B runs only: MARL_HIP_OPTIONS="name=value,..."; bench.py records it)
            self.set_option(name, value)
        # derived constants, named as in the reference (:36-72, :130-133)
        names = ("delta_x", "nu1", "nu2", "KRat", "dCa", "dCO3", "delta", "Da", "lambda_", "auxcon", "rhorat0",
                 "rhorat", "presum", "F_fixed", "dPhi_fixed", "Peclet_min", "Peclet_max", "mask_lo", "mask_hi")
        vals = (C.c_double * 19)()
        self._check(self._lib.marl_get_constants(self._ctx, 0, vals), "marl_get_constants")
        for n_, v in zip(names, vals):
            setattr(self, n_, int(v) if n_.startswith("mask_") else float(v))
        x = Depths.axes_coords[0]
        self.not_too_shallow = np.heaviside(x - ShallowLimit / Xstar, 0)
        self.not_too_deep = np.heaviside(DeepLimit / Xstar - x, 0)

    def _pack_blocks(self):
        return pack_blocks(self.instances, self.Depths.length)

    def set_scenario(self, pde_parms):
        """The parameters of another scenario (``asdict(Map_Scenario())``-style dict, same N and max_depth / Xstar) for this
        single-instance model: what constructing the reference's model again does, with the device buffers kept (marl_ctx_set_params)."""
        import inspect
        if len(self.instances) != 1:
            raise ValueError("set_scenario: single-instance models only")
        names = {p for p in inspect.signature(type(self).__init__).parameters} - {"self", "Depths", "device", "slices_all_fields", "not_too_shallow",
                                                                                   "not_too_deep", "_extra_instances"}
        new = {k: v for k, v in pde_parms.items() if k in names}
        if int(pde_parms.get("N", self.Depths.N)) != self.Depths.N:
            raise ValueError("set_scenario: the grid size cannot change")
        # the column's length max_depth / Xstar (Evolve_scenario.py:27-31) may change with the scenario: the grid - and with it delta_x,
        # the masks and the cell centres - is rebuilt, exactly as constructing the model again would (marl_ctx_set_params re-derives
        # every constant from the new length)
        if "max_depth" in pde_parms and "Xstar" in pde_parms:
            length = float(pde_parms["max_depth"]) / float(pde_parms["Xstar"])
            if length != self.Depths.length:
                self.Depths = DepthGrid(length, self.Depths.N)
        sig = inspect.signature(type(self).__init__).parameters
        defaults = {k: sig[k].default for k in names if sig[k].default is not inspect.Parameter.empty}   # as a fresh construction would take them
        missing = [k for k in names if k not in new and k not in defaults]
        if missing:
            raise TypeError(f"set_scenario: missing parameters {sorted(missing)}")
        inst = defaults | new
        inst["dPhi_variable"] = bool(inst.get("dPhi_variable", False))
        self.instances = [inst]
        for k, v in inst.items():
            setattr(self, k, v)
        self._check(self._lib.marl_ctx_set_params(self._ctx, self._pack_blocks(), 1), "marl_ctx_set_params")
        names19 = ("delta_x", "nu1", "nu2", "KRat", "dCa", "dCO3", "delta", "Da", "lambda_", "auxcon", "rhorat0",
                   "rhorat", "presum", "F_fixed", "dPhi_fixed", "Peclet_min", "Peclet_max", "mask_lo", "mask_hi")
        vals = (C.c_double * 19)()
        self._check(self._lib.marl_get_constants(self._ctx, 0, vals), "marl_get_constants")
        for n_, v in zip(names19, vals):
            setattr(self, n_, int(v) if n_.startswith("mask_") else float(v))
        x = self.Depths.axes_coords[0]
        self.not_too_shallow = np.heaviside(x - inst["ShallowLimit"] / inst["Xstar"], 0)
        self.not_too_deep = np.heaviside(inst["DeepLimit"] / inst["Xstar"] - x, 0)

    # -- construction helpers ------------------------------------------------------------------
    @classmethod
    def batch(cls, Depths, instances, device=0):
        """A sweep: ``instances`` is a list of keyword dicts (each as for the constructor)."""
        instances = list(instances)
        return cls(Depths, **instances[0], device=device, _extra_instances=tuple(instances[1:]))

    @classmethod
    def from_scenario(cls, pde_parms, device=0, instances=None):
        """Build from ``asdict(Map_Scenario())``-style dict(s) the way Evolve_scenario.py:27-68 does."""
        import inspect
        names = {p for p in inspect.signature(cls.__init__).parameters} - {"self", "Depths", "device"}
        grid = DepthGrid(pde_parms["max_depth"] / pde_parms["Xstar"], int(pde_parms["N"]))
        pick = lambda d: {k: v for k, v in d.items() if k in names}  # noqa: E731
        if instances is None:
            return cls(grid, **pick(pde_parms), device=device)
        return cls.batch(grid, [pick(pde_parms | inst) for inst in instances], device=device)

    @property
    def n_instances(self):
        return len(self.instances)

    def _check(self, rc, what):
        return _abi.check(self._ctx, rc, what)

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.marl_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, name, value):
        self._check(self._lib.marl_set_option(self._ctx, name.encode(), int(value)), "marl_set_option")

    def set_terminal(self, spec):
        """Make monitors terminal - the reference's ``terminal`` switch (LHeureux_model.py:113-122), for every run of this model from
        now on (marl_set_terminal).  ``spec`` as for :func:`terminal_counts`; None switches it off again.  Radau and BDF single runs,
        Radau, BDF, RK45 and RK23 sweeps and :meth:`integrate_rk45_terminal` / :meth:`integrate_rk23_terminal` end at the root with
        ``status`` 1; :meth:`sweep_rk4_watch_device` / :meth:`integrate_rk4_watch` end at the END of the step of the occurrence (a fixed
        step has no dense output to interpolate with) and the plain fixed-step runs ignore the limits; the other integrators
        (:meth:`integrate_rk45` / :meth:`integrate_rk23` and the ``*_device`` single runs among them) raise while a monitor is terminal."""
        counts = terminal_counts(spec)
        self._check(self._lib.marl_set_terminal(self._ctx, (C.c_int64 * NEVENTS)(*counts)), "marl_set_terminal")
        self._terminal = counts

    @property
    def terminal(self):
        """The limits in force, a tuple of 7 ints (0: the monitor only records)."""
        return getattr(self, "_terminal", (0,) * NEVENTS)

    def use_stream(self, stream_handle):
        """Run on an existing HIP stream, e.g. ``torch.cuda.current_stream().cuda_stream``."""
        self._check(self._lib.marl_set_stream(self._ctx, C.c_void_p(stream_handle)), "marl_set_stream")

    def synchronize(self):
        self._check(self._lib.marl_synchronize(self._ctx), "marl_synchronize")

    def state_doubles(self, layout=LAYOUT_FIELD_MAJOR):
        return int(self._lib.marl_state_doubles(self._ctx, layout))

    def get_state(self, AragoniteSurface, CalciteSurface, CaSurface, CO3Surface, PorSurface):
        """Initial state (5, N) from five uniform values or arrays (reference :135-145)."""
        N = self.Depths.N
        return np.stack([np.broadcast_to(np.asarray(v, dtype=float), (N,)) for v in
                         (AragoniteSurface, CalciteSurface, CaSurface, CO3Surface, PorSurface)]).copy()

    # -- RHS: the solve_ivp callable -------------------------------------------------------------
    def _host_state(self, y):
        y = np.ascontiguousarray(y, dtype=np.float64)
        want = 5 * self.Depths.N * self.n_instances
        if y.size != want:
            raise ValueError(f"state has {y.size} entries, expected {want} (5 fields x N x instances)")
        return y

    def fun(self, t, y, progress_proxy=None, progress_dt=None, t0=None):
        """dy/dt for the field-major state ``y`` (host array); returns a new array (reference :162-288)."""
        if progress_proxy is not None and progress_dt:   # the reference's tqdm hook (:168-172)
            if self.last_t == 0.0:
                self.last_t = t0
            n = int((t - self.last_t) / progress_dt)
            progress_proxy.update(n)
            self.last_t += n * progress_dt
        y = self._host_state(y)
        out = np.empty_like(y)
        self._check(self._lib.marl_rhs(self._ctx, float(t), _as_ptr(y), _as_ptr(out)), "marl_rhs")
        return out

    fun_numba = fun  # the reference's second spelling of the same callable (:290-359)

    def rhs_device(self, y_dev_ptr, dydt_dev_ptr, layout=LAYOUT_FIELD_MAJOR, t=0.0):
        """RHS on device buffers (raw pointers, e.g. ``tensor.data_ptr()``); asynchronous."""
        self._check(self._lib.marl_rhs_dev(self._ctx, float(t), C.c_void_p(y_dev_ptr), C.c_void_p(dydt_dev_ptr), layout),
                    "marl_rhs_dev")

    # -- monitors (solve_ivp events) -----------------------------------------------------------------
    def events_all(self, y):
        """The seven monitors, shape (instances, 7), in the reference's order (Evolve_scenario.py:107-109)."""
        y = self._host_state(y)
        out = np.empty((self.n_instances, NEVENTS))
        self._check(self._lib.marl_events(self._ctx, _as_ptr(y), _as_ptr(out)), "marl_events")
        return out

    def events_device(self, y_dev_ptr, layout=LAYOUT_FIELD_MAJOR):
        out = np.empty((self.n_instances, NEVENTS))
        self._check(self._lib.marl_events_dev(self._ctx, C.c_void_p(y_dev_ptr), layout, _as_ptr(out)), "marl_events_dev")
        return out

    def _event(index):  # noqa: N805 - builds the seven scipy-style event callables
        def event(self, t, y, progress_proxy=None, progress_dt=None, t0=None):
            return float(self.events_all(y)[0, index])
        event.terminal = False   # reference :116-122: all seven only record, never stop
        return event

    zeros = _event(0)
    zeros_CA = _event(1)
    zeros_CC = _event(2)
    ones_CA_plus_CC = _event(3)
    ones_Phi = _event(4)
    zeros_U = _event(5)
    zeros_W = _event(6)
    del _event

    def convert_layout_device(self, src_ptr, dst_ptr, src_layout, dst_layout):
        self._check(self._lib.marl_convert_layout_dev(self._ctx, C.c_void_p(src_ptr), C.c_void_p(dst_ptr), src_layout,
                                                      dst_layout), "marl_convert_layout_dev")

    # -- time loops ----------------------------------------------------------------------------------
    def integrate_rk4(self, y, dt, nsteps):
        """Classical RK4, ``nsteps`` steps of ``dt``; host state in, new host state out."""
        y = self._host_state(y).copy()
        self._check(self._lib.marl_integrate_rk4(self._ctx, _as_ptr(y), float(dt), int(nsteps)), "marl_integrate_rk4")
        return y

    def integrate_rk4_device(self, y_dev_ptr, dt, nsteps, layout=LAYOUT_FIELD_MAJOR):
        self._check(self._lib.marl_integrate_rk4_dev(self._ctx, C.c_void_p(y_dev_ptr), layout, float(dt), int(nsteps)),
                    "marl_integrate_rk4_dev")

    def sweep_rk4_device(self, y_dev_ptr, dt, nsteps):
        dt = np.ascontiguousarray(np.broadcast_to(np.asarray(dt, dtype=np.float64), (self.n_instances,)))
        self._check(self._lib.marl_sweep_rk4_dev(self._ctx, C.c_void_p(y_dev_ptr), _as_ptr(dt), int(nsteps)),
                    "marl_sweep_rk4_dev")

    def sweep_rk4_watch_device(self, y_dev_ptr, dt, nsteps, t0=0.0, frame_steps=None, frames_dev_ptr=None, events=False, max_events=64):
        """:meth:`sweep_rk4_device` with the driver inside the kernel (marl_sweep_rk4_watch_dev; N <= 1024): the seven monitors after
        every step, frames, terminal monitors (:meth:`set_terminal`) and a stop when the state goes non-finite.  Device states
        [instances][5N] in place; ``dt`` a scalar or one per instance; step s goes from ``t0 + s dt`` to ``t0 + (s + 1) dt``.
        Returns one :class:`RK45Result` per instance: ``status`` 0, 1 (a terminal monitor ended the run at the END of its step - the
        state is that step's result, not interpolated) or -2 (non-finite after a step: ``dt`` too large); ``n_accepted`` the steps done,
        ``t_reached`` their end, ``event_values`` / ``n_events`` the monitors and their sign changes.

        ``frame_steps``: strictly ascending step counts in [0, nsteps], shared by all instances; frame j is the state after
        ``frame_steps[j]`` steps, written inside the kernel to ``frames_dev_ptr``, device memory [instances][len(frame_steps)][5N].
        Each result carries ``t = t0 + frame_steps[:n_frames] * dt``; frames beyond ``n_frames`` are not written.

        ``events=True``: ``t_events``, a list of 7 arrays per instance, ``min(n_events[e], max_events)`` long: the secant estimates
        ``t_s + dt go / (go - gn)`` of the sign changes - no dense output, no Brent; O(dt^2) from the root."""
        B = self.n_instances
        dts = np.ascontiguousarray(np.broadcast_to(np.asarray(dt, dtype=np.float64), (B,)))
        fs = np.empty(0, dtype=np.int64) if frame_steps is None else np.ascontiguousarray(frame_steps, dtype=np.int64).ravel()
        if fs.size and not frames_dev_ptr:
            raise ValueError("sweep_rk4_watch_device: frame_steps needs frames_dev_ptr, device memory [instances][len(frame_steps)][5N]")
        locate = bool(events) and int(max_events) > 0
        stats = (MarlStats * B)()
        n_done = np.zeros(B, dtype=np.int64)
        tev = _root_buffer((B,), max_events) if locate else None
        rc = self._lib.marl_sweep_rk4_watch_dev(self._ctx, C.c_void_p(y_dev_ptr), float(t0), _as_ptr(dts), int(nsteps),
                                                _as_ptr(fs) if fs.size else None, fs.size, C.c_void_p(frames_dev_ptr) if fs.size else None,
                                                _as_ptr(n_done), _as_ptr(tev) if locate else None, int(max_events) if locate else 0, stats)
        self._check(rc, "marl_sweep_rk4_watch_dev")
        res = _sweep_results(stats, fs if frame_steps is not None else None, n_done, tev)
        for r, h in zip(res, dts):
            if frame_steps is not None:
                r.t = float(t0) + r.t * h      # (the frames it reached, as step counts so far)
        return res

    def integrate_rk4_watch(self, y0, dt, nsteps, t0=0.0, frame_steps=None, events=True, max_events=4096):
        """:meth:`integrate_rk4` for ONE instance with the driver inside the kernel (marl_integrate_rk4_watch; N <= 1024): see
        :meth:`sweep_rk4_watch_device` for the rules.  Returns an :class:`RK45Result` whose ``t`` / ``y`` hold the frames the run
        reached (``y``: (5N, n_frames)) or, without ``frame_steps``, the end point only; ``t_events`` is a list of 7 arrays (every
        sign change: the run is repeated with a larger buffer when ``max_events`` was too small); ``y_final`` the returned state."""
        y_start = self._host_state(y0)
        n = y_start.size
        fs = np.empty(0, dtype=np.int64) if frame_steps is None else np.ascontiguousarray(frame_steps, dtype=np.int64).ravel()

        def run(max_events):
            y, stats, frames, n_done = y_start.copy(), MarlStats(), np.empty((max(fs.size, 1), n)), np.zeros(1, dtype=np.int64)
            locate = bool(events) and max_events > 0
            tev = _root_buffer((), max_events) if locate else None
            rc = self._lib.marl_integrate_rk4_watch(self._ctx, _as_ptr(y), float(t0), float(dt), int(nsteps), _as_ptr(fs) if fs.size else None, fs.size,
                                                    _as_ptr(frames) if fs.size else None, _as_ptr(n_done), _as_ptr(tev) if locate else None,
                                                    max_events if locate else 0, C.byref(stats))
            self._check(rc, "marl_integrate_rk4_watch")
            return (y, stats, frames, int(n_done[0]), tev), max(stats.n_events[:]) if locate else 0

        y, stats, frames, k, tev = _with_room(run, int(max_events))
        t_events = None
        if events:      # (without room for a root nothing is located: seven empty arrays)
            t_events = _root_times(tev, stats.n_events) if tev is not None else [np.empty(0) for _ in range(NEVENTS)]
        if frame_steps is None:
            return _single_result(stats, y, t_events)
        return _single_result(stats, y, t_events, float(t0) + fs[:k] * float(dt), frames[:k])

    def integrate_rk45(self, y0, t_span, first_step, rtol, atol, t_eval=None, events=True, max_events=4096,
                       max_attempts=0):
        """scipy ``solve_ivp(method="RK45")`` semantics for ONE instance, entirely on the device.

        Returns an :class:`RK45Result` whose ``t``/``y`` hold the ``t_eval`` samples (``y``: (5N, n_t), as
        scipy) or, without ``t_eval``, the end point only; ``t_events`` is a list of 7 arrays."""
        return self._integrate_rk("rk45", y0, t_span, first_step, rtol, atol, t_eval, events, max_events, max_attempts)

    def integrate_rk23(self, y0, t_span, first_step, rtol, atol, t_eval=None, events=True, max_events=4096,
                       max_attempts=0):
        """scipy ``solve_ivp(method="RK23")`` semantics for ONE instance, entirely on the device (marl_integrate_rk23):
        :meth:`integrate_rk45` with Bogacki-Shampine 3(2) - 3 RHS evaluations per attempt, cubic dense output.  Same result."""
        return self._integrate_rk("rk23", y0, t_span, first_step, rtol, atol, t_eval, events, max_events, max_attempts)

    def integrate_dop853(self, y0, t_span, first_step, rtol, atol, t_eval=None, events=True, max_events=4096,
                         max_attempts=0):
        """scipy ``solve_ivp(method="DOP853")`` semantics for ONE instance, entirely on the device (marl_integrate_dop853):
        :meth:`integrate_rk45` with Dormand-Prince 8(5,3) - 12 RHS evaluations per attempt, and 3 more for every accepted step with
        a monitor sign change or a ``t_eval`` sample in it (the dense output's extra stages, which scipy counts).  Same result.
        Grids of up to 1024 cells only, and no terminal monitors: both are refused with a :class:`MarlError`
        (:meth:`integrate_dop853_stop` is the run that stops at a terminal monitor's root)."""
        return self._integrate_rk("dop853", y0, t_span, first_step, rtol, atol, t_eval, events, max_events, max_attempts)

    def integrate_rk45_terminal(self, y0, t_span, first_step, rtol, atol, t_eval=None, events=True, max_events=4096,
                                max_attempts=0):
        """:meth:`integrate_rk45` honouring terminal monitors (:meth:`set_terminal`; marl_integrate_rk45_terminal): the run ends at
        the terminal monitor's root with ``status`` 1, ``t_reached`` = the root, ``y_final`` the step's dense output there (bit for
        bit a ``t_eval`` sample at that time), ``t`` / ``y`` the samples up to it and ``t_events`` the roots up to and including
        it.  The same signature and result; without a terminal monitor the same run."""
        return self._integrate_rk("rk45_terminal", y0, t_span, first_step, rtol, atol, t_eval, events, max_events, max_attempts)

    def integrate_rk23_terminal(self, y0, t_span, first_step, rtol, atol, t_eval=None, events=True, max_events=4096,
                                max_attempts=0):
        """:meth:`integrate_rk45_terminal` with RK23 (marl_integrate_rk23_terminal)."""
        return self._integrate_rk("rk23_terminal", y0, t_span, first_step, rtol, atol, t_eval, events, max_events, max_attempts)

    def integrate_dop853_stop(self, y0, t_span, first_step, rtol, atol, t_eval=None, events=True, max_events=4096,
                              max_attempts=0):
        """:meth:`integrate_dop853` honouring terminal monitors (:meth:`set_terminal`; marl_integrate_dop853_stop): the signature and
        the result of :meth:`integrate_rk45_terminal` - the run ends at the terminal monitor's root with ``status`` 1, ``t_reached``
        = the root, ``y_final`` the step's dense output there, ``t`` / ``y`` the samples up to it and ``t_events`` the roots up to
        and including it; ``events=False`` stops all the same.  Without a terminal monitor the same run as :meth:`integrate_dop853`."""
        return self._integrate_rk("dop853_stop", y0, t_span, first_step, rtol, atol, t_eval, events, max_events, max_attempts)

    def integrate_dop853_grid(self, y0, t_span, first_step, rtol, atol, t_eval=None, events=True, max_events=4096,
                              max_attempts=0):
        """:meth:`integrate_dop853` for a grid of ANY size (marl_integrate_dop853_grid): the large-grid loop - one launch per stage,
        the stage derivatives in an arena owned by the context, one status read per batch of attempts, roots by Brent's method on
        dense evaluations at a pause.  The same signature, result and ``nfev``; on grids of up to 1024 cells it agrees with
        :meth:`integrate_dop853` to rounding (the sums are ordered differently), not bit for bit.  Terminal monitors
        (:meth:`set_terminal`) are honoured as by :meth:`integrate_rk45_terminal`.  One instance, no slab contexts."""
        return self._integrate_rk("dop853_grid", y0, t_span, first_step, rtol, atol, t_eval, events, max_events, max_attempts)

    def _integrate_rk(self, method, y0, t_span, first_step, rtol, atol, t_eval, events, max_events, max_attempts):
        return _single_run(self, f"marl_integrate_{method}", self._host_state(y0), t_span, first_step, rtol, atol, t_eval, events, max_events, max_attempts)

    def integrate_radau(self, y0, t_span, first_step, rtol, atol, t_eval=None, events=True, max_events=4096, max_attempts=0,
                        groups=None):
        """scipy ``solve_ivp(method="Radau", jac_sparsity=<the reference's 27-diagonal pattern>)`` semantics for ONE instance -
        the reference's default solver (marlpde/parameters.py:213) - with the RHS, the finite-difference Jacobian, the
        block-tridiagonal factorisations and all vector work on the device (marl_integrate_radau).

        ``groups``: scipy's column grouping of the pattern (``scipy.optimize._numdiff.group_columns``), or None for a
        structured 15-colouring (same Jacobian).  Returns an :class:`RK45Result` (``nfev``/``njev``/``nlu`` as scipy counts)."""
        return self._integrate_implicit("marl_integrate_radau", y0, t_span, first_step, rtol, atol, t_eval, events, max_events, max_attempts, groups)

    def integrate_bdf(self, y0, t_span, first_step, rtol, atol, t_eval=None, events=True, max_events=4096, max_attempts=0, groups=None):
        """scipy ``solve_ivp(method="BDF", jac_sparsity=<the reference's pattern>)`` semantics for ONE instance - the other implicit
        method the reference's Solver names (marlpde/parameters.py:205-219) - on the device (marl_integrate_bdf): variable order 1..5,
        the matrix I - c J factorised by cyclic reduction.  Arguments and result as for :meth:`integrate_radau`."""
        return self._integrate_implicit("marl_integrate_bdf", y0, t_span, first_step, rtol, atol, t_eval, events, max_events, max_attempts, groups)

    def _integrate_implicit(self, entry, y0, t_span, first_step, rtol, atol, t_eval, events, max_events, max_attempts, groups):
        y_start = self._host_state(y0)
        return _single_run(self, entry, y_start, t_span, first_step, rtol, atol, t_eval, events, max_events, max_attempts,
                           grp=(_groups(groups, y_start.size),))

    # -- test hooks of the implicit path -------------------------------------------------------------------
    def debug_num_jac(self, y, threshold, groups=None, factor=None):
        """One finite-difference Jacobian as the implicit integrators evaluate it (marl_debug_num_jac).  ``factor`` None: the first
        Jacobian of a run (every factor sqrt(eps)); else the factors the previous call returned.  Returns ``(J, factor)``: J in the
        device layout (N, 3, 5, 5) - ``J[i, d, f, fp]`` = d rate(f, i) / d y(fp, i + d - 1) - and the adapted factors (5N, field-major)."""
        y = self._host_state(y)
        n, N = y.size, self.Depths.N
        grp = _groups(groups, n)
        fac = np.zeros(n) if factor is None else np.array(factor, dtype=np.float64).ravel()
        if fac.size != n:
            raise ValueError(f"factor has {fac.size} entries, expected {n}")
        J = np.empty((N, 3, 5, 5))
        self._check(self._lib.marl_debug_num_jac(self._ctx, _as_ptr(y), float(threshold), grp, _as_ptr(fac), 1 if factor is None else 0, _as_ptr(J)),
                    "marl_debug_num_jac")
        return J, fac

    def debug_block_solve(self, J, b_r, b_c=None, mu_r=1.0, mu_c=0j, jscale=1.0):
        """Factorise ``mu I - jscale J`` once and solve the right-hand sides with it (marl_debug_block_solve).  ``J``: (N, 3, 5, 5) as
        :meth:`debug_num_jac` returns it; ``b_r``: (nrhs, 5N) cell-major, real system; ``b_c``: (nrhs, 5N) complex, the complex system
        (None: the real system only, BDF's call).  Returns ``x_r`` or ``(x_r, x_c)``."""
        N = self.Depths.N
        J = np.ascontiguousarray(J, dtype=np.float64)
        if J.size != 75 * N:
            raise ValueError(f"J has {J.size} entries, expected {75 * N}")
        b_r = np.ascontiguousarray(np.atleast_2d(b_r), dtype=np.float64)
        if b_r.shape[1] != 5 * N:
            raise ValueError(f"b_r has {b_r.shape[1]} columns, expected {5 * N}")
        x_r = np.empty_like(b_r)
        x_c = None
        if b_c is not None:
            b_c = np.ascontiguousarray(np.atleast_2d(b_c), dtype=np.complex128)
            if b_c.shape != b_r.shape:
                raise ValueError("b_c must have the shape of b_r")
            x_c = np.empty_like(b_c)
        mu_c = complex(mu_c)
        self._check(self._lib.marl_debug_block_solve(self._ctx, _as_ptr(J), float(jscale), float(mu_r), mu_c.real, mu_c.imag,
                                                     1 if b_c is None else 2, b_r.shape[0], _as_ptr(b_r),
                                                     _as_ptr(b_c) if b_c is not None else None, _as_ptr(x_r),
                                                     _as_ptr(x_c) if b_c is not None else None), "marl_debug_block_solve")
        return x_r if b_c is None else (x_r, x_c)

    BDF_BATCH_OPS = {"INIT_D": 0, "CHANGE_D": 1, "ACCEPT_NORMS": 2, "SAMPLE": 3, "ROOTS": 4, "STOP": 5}   # include/marl_hip.h: MARL_BDF_*

    def debug_bdf_batch(self, op, D, y=None, f=None, d=None, ynew=None, *, instances=None, order=1, h=1.0, RU=None, rtol=1e-3, atol=1e-3,
                        want_norms=0, err_coef_m=0.0, err_coef_p=0.0, t=0.0, t_old=0.0, first=0, end=0, mask=0, slot=None, t_eval=None,
                        frames=None, t_events=None, ss=None):
        """ONE launch of one vector kernel of the BDF sweep on the sweep's arena of this model's B instances (marl_debug_bdf_batch).
        ``op``: a key of ``BDF_BATCH_OPS``.  ``D``: (B, 8, 5N), every row of every instance's differences; ``y``, ``f``, ``d``, ``ynew``:
        (B, 5N) or None (zeros).  ``instances``: the work list (instance indices in launch order) or None for all in order.  The scalars
        ``order`` .. ``mask`` are one value or one per instance, ``RU``: (B, 6, 6) or (6, 6), ``slot``: (B, 7) or (7,).  ``frames``
        (B, n_eval, 5N), ``t_events`` (B, 7, max_events) and ``ss`` (B, 2) hold what is on the device before the launch (sentinels);
        None: no frames / no root slots / zeros.  Returns a dict of copies - D, y, frames, t_events, ss - as the launch left them.
        ``"STOP"`` (the state a terminal monitor leaves) reads its ``t_stop`` from ``t_old`` and returns the seven monitors of the
        listed instances' states in ``t_events[:, :, 0]`` (it needs ``t_events`` with at least one slot)."""
        B, n = self.n_instances, 5 * self.Depths.N
        D = np.array(D, dtype=np.float64)
        if D.shape != (B, 8, n):
            raise ValueError(f"D has shape {D.shape}, expected {(B, 8, n)}")
        vec = np.zeros((B, 4, n))
        for k, v in enumerate((y, f, d, ynew)):
            if v is not None:
                vec[:, k] = np.asarray(v, dtype=np.float64).reshape(B, n)
        per = lambda v, dt: np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dt), (B,)))  # noqa: E731
        ia = np.zeros((B, 12), dtype=np.int64)
        for k, v in enumerate((order, want_norms, first, end, mask)):
            ia[:, k] = per(v, np.int64)
        ia[:, 5:] = np.broadcast_to(np.asarray(0 if slot is None else slot, dtype=np.int64), (B, 7))
        da = np.zeros((B, 43))
        for k, v in enumerate((h, rtol, atol, err_coef_m, err_coef_p, t, t_old)):
            da[:, k] = per(v, np.float64)
        da[:, 7:] = np.broadcast_to(np.asarray(0.0 if RU is None else RU, dtype=np.float64), (B, 6, 6)).reshape(B, 36)
        lst = None if instances is None else np.ascontiguousarray(instances, dtype=np.int32)
        te = np.ascontiguousarray([] if t_eval is None else t_eval, dtype=np.float64)
        fr = np.empty((B, 0, n)) if frames is None else np.array(frames, dtype=np.float64)
        if fr.shape != (B, te.size, n):
            raise ValueError(f"frames has shape {fr.shape}, expected {(B, te.size, n)}")
        tev = np.empty((B, 7, 0)) if t_events is None else np.array(t_events, dtype=np.float64)
        if tev.ndim != 3 or tev.shape[:2] != (B, 7):
            raise ValueError(f"t_events has shape {tev.shape}, expected {(B, 7)} + (max_events,)")
        ss = np.zeros((B, 2)) if ss is None else np.array(ss, dtype=np.float64)
        if ss.shape != (B, 2):
            raise ValueError(f"ss has shape {ss.shape}, expected {(B, 2)}")
        D_out, y_out = np.empty_like(D), np.empty((B, n))
        self._check(self._lib.marl_debug_bdf_batch(
            self._ctx, self.BDF_BATCH_OPS[op], _as_ptr(lst) if lst is not None else None, 0 if lst is None else lst.size, _as_ptr(ia), _as_ptr(da),
            _as_ptr(D), _as_ptr(vec), _as_ptr(te) if te.size else None, te.size, tev.shape[2], _as_ptr(D_out), _as_ptr(y_out),
            _as_ptr(fr) if fr.size else None, _as_ptr(tev) if tev.size else None, _as_ptr(ss)), "marl_debug_bdf_batch")
        return dict(D=D_out, y=y_out, frames=fr, t_events=tev, ss=ss)

    def integrate_rk45_device(self, y_dev_ptr, t_span, first_step, rtol, atol, layout=LAYOUT_FIELD_MAJOR, max_attempts=0):
        return self._integrate_rk_device("rk45", y_dev_ptr, t_span, first_step, rtol, atol, layout, max_attempts)

    def integrate_rk23_device(self, y_dev_ptr, t_span, first_step, rtol, atol, layout=LAYOUT_FIELD_MAJOR, max_attempts=0):
        """:meth:`integrate_rk45_device` with RK23 (marl_integrate_rk23_dev)."""
        return self._integrate_rk_device("rk23", y_dev_ptr, t_span, first_step, rtol, atol, layout, max_attempts)

    def integrate_dop853_grid_device(self, y_dev_ptr, t_span, first_step, rtol, atol, layout=LAYOUT_FIELD_MAJOR, max_attempts=0):
        """:meth:`integrate_rk45_device` with DOP853 on a grid of any size (marl_integrate_dop853_grid_dev); refuses terminal monitors."""
        return self._integrate_rk_device("dop853_grid", y_dev_ptr, t_span, first_step, rtol, atol, layout, max_attempts)

    def _integrate_rk_device(self, method, y_dev_ptr, t_span, first_step, rtol, atol, layout, max_attempts):
        stats = MarlStats()
        rc = getattr(self._lib, f"marl_integrate_{method}_dev")(self._ctx, C.c_void_p(y_dev_ptr), layout, float(t_span[0]), float(t_span[1]),
                                               float(first_step), float(rtol), float(atol), int(max_attempts), C.byref(stats))
        self._check(rc, f"marl_integrate_{method}_dev")
        return RK45Result(stats)

    def sweep_radau_device(self, y_dev_ptr, t_span, first_step, rtol, atol, max_attempts=0, groups=None, events=False, max_events=64,
                           t_eval=None, y_eval_dev_ptr=None):
        """Every instance of the model integrated with the reference's default solver (scipy Radau semantics), all instances
        advanced together on the device (marl_sweep_radau_dev); device states [instances][5N] in place.  Returns one
        :class:`RK45Result` per instance (statistics).  ``events=True``: the monitors' root times are located inside the sweep
        (marl_sweep_radau_events_dev) and returned as ``t_events`` - a list of 7 arrays per instance, what the reference prints and
        stores for every run (Evolve_scenario.py:118-145, 175-177); otherwise sign changes are only counted.

        With ``t_eval`` (sorted sample times within ``t_span``, shared by all instances) the sweep also writes the time series that
        ``solve_ivp(..., t_eval=)`` returns (marl_sweep_radau_eval_dev), as :meth:`sweep_rk45_device` does: ``y_eval_dev_ptr`` is device
        memory [instances][len(t_eval)][5N]; each result carries ``t = t_eval[:n_frames]``, the frames stay on the device, and frames
        beyond ``n_frames`` are not written.  Combinable with ``events``."""
        head = _run_head(self, C.c_void_p(y_dev_ptr), t_span, first_step, rtol, atol) + (_groups(groups), int(max_attempts))
        # Radau's own entry choice: its _eval_dev entry takes the root arguments too, and _events_dev is taken even without room for a root
        # (seven empty arrays); every entry honours terminal monitors
        if t_eval is not None:
            locate = bool(events) and int(max_events) > 0
            return _sweep_call(self, "radau", "marl_sweep_radau_eval_dev", head, ("samples", "roots"), t_eval, y_eval_dev_ptr,
                               _root_buffer((self.n_instances,), max_events) if locate else None)
        if not events:
            return _sweep_call(self, "radau", "marl_sweep_radau_dev", head, ())
        return _sweep_call(self, "radau", "marl_sweep_radau_events_dev", head, ("roots",), tev=_root_buffer((self.n_instances,), max_events))

    def sweep_bdf_device(self, y_dev_ptr, t_span, first_step, rtol, atol, max_attempts=0, groups=None, t_eval=None, y_eval_dev_ptr=None,
                         events=False, max_events=64):
        """Every instance of the model integrated with scipy's BDF semantics, all instances advanced together on the device
        (marl_sweep_bdf_dev: per-instance step control on the device, batched solves); device states [instances][5N] in place.
        Returns one :class:`RK45Result` per instance (statistics; the monitors' sign changes are counted in ``n_events``).  The grid
        is limited to N <= 409 (a solve must fit one workgroup).

        With ``t_eval`` (sorted sample times within ``t_span``, shared by all instances) the sweep also writes the time series that
        ``solve_ivp(..., t_eval=)`` returns (marl_sweep_bdf_eval_dev), as :meth:`sweep_radau_device` does: ``y_eval_dev_ptr`` is device
        memory [instances][len(t_eval)][5N]; each result carries ``t = t_eval[:n_frames]``, the frames stay on the device, and frames
        beyond ``n_frames`` are not written.

        ``events=True``: the monitors' root times are located inside the sweep (marl_sweep_bdf_events_dev) and returned as
        ``t_events`` - a list of 7 arrays per instance, ``min(n_events[e], max_events)`` long, what the reference prints and stores
        for every run (Evolve_scenario.py:118-145, 175-177); otherwise (or with ``max_events`` = 0) sign changes are only counted and
        ``t_events`` is None.  Combinable with ``t_eval``.

        While a monitor is terminal (:meth:`set_terminal`) the sweep runs through marl_sweep_bdf_terminal_dev: an instance whose
        terminal monitor occurs ends at that root on the device with ``status`` 1, ``t_reached`` = the root and the state there; the
        results are built as above, with or without ``t_eval`` and ``events``."""
        head = _run_head(self, C.c_void_p(y_dev_ptr), t_span, first_step, rtol, atol) + (_groups(groups), int(max_attempts))
        return _sweep_choose(self, "bdf", "marl_sweep_bdf_terminal_dev", head, t_eval, y_eval_dev_ptr, events, max_events)

    def sweep_rk45_device(self, y_dev_ptr, t_span, first_step, rtol, atol, max_attempts=0, t_eval=None, y_eval_dev_ptr=None,
                          events=False, max_events=64):
        """Every instance integrated with adaptive RK45, one workgroup each (marl_sweep_rk45_dev); device states [instances][5N]
        in place.  Returns one :class:`RK45Result` per instance.

        With ``t_eval`` (sorted sample times within ``t_span``, shared by all instances) the sweep also writes the time series
        that ``solve_ivp(..., t_eval=)`` returns (marl_sweep_rk45_eval_dev): ``y_eval_dev_ptr`` is device memory
        [instances][len(t_eval)][5N]; each result carries ``t = t_eval[:n_frames]``, the samples up to the time that instance
        reached, and the frames stay on the device - frames beyond ``n_frames`` are not written.

        ``events=True``: the monitors' root times are located inside the sweep (marl_sweep_rk45_events_dev) and returned as
        ``t_events`` - a list of 7 arrays per instance, ``min(n_events[e], max_events)`` long, what the reference prints and stores
        for every run (Evolve_scenario.py:118-145, 175-177); otherwise sign changes are only counted.  Combinable with ``t_eval``.

        While a monitor is terminal (:meth:`set_terminal`) the sweep runs through marl_sweep_rk45_terminal_dev: an instance whose
        terminal monitor occurs ends at that root inside the sweep kernel with ``status`` 1, ``t_reached`` = the root and the state
        there; the results are built as above, with or without ``t_eval`` and ``events``."""
        return self._sweep_rk_device("rk45", y_dev_ptr, t_span, first_step, rtol, atol, max_attempts, t_eval, y_eval_dev_ptr, events, max_events)

    def sweep_rk23_device(self, y_dev_ptr, t_span, first_step, rtol, atol, max_attempts=0, t_eval=None, y_eval_dev_ptr=None,
                          events=False, max_events=64):
        """:meth:`sweep_rk45_device` with RK23 (marl_sweep_rk23_dev / _eval_dev / _events_dev): the same arguments and results."""
        return self._sweep_rk_device("rk23", y_dev_ptr, t_span, first_step, rtol, atol, max_attempts, t_eval, y_eval_dev_ptr, events, max_events)

    def sweep_dop853_device(self, y_dev_ptr, t_span, first_step, rtol, atol, max_attempts=0, t_eval=None, y_eval_dev_ptr=None,
                            events=False, max_events=64):
        """:meth:`sweep_rk45_device` with DOP853 (marl_sweep_dop853_dev / _eval_dev / _events_dev): the same arguments and results;
        ``nfev`` counts 12 per attempt and 3 per accepted step with a monitor sign change or a sample in it.  These entries do not
        stop: while a monitor is terminal (:meth:`set_terminal`) they refuse the call, and so does this method
        (:meth:`sweep_dop853_stop_device` is the sweep that stops)."""
        return self._sweep_rk_device("dop853", y_dev_ptr, t_span, first_step, rtol, atol, max_attempts, t_eval, y_eval_dev_ptr, events, max_events,
                                     terminal_entry=False)

    def sweep_dop853_stop_device(self, y_dev_ptr, t_span, first_step, rtol, atol, max_attempts=0, t_eval=None, y_eval_dev_ptr=None,
                                 events=False, max_events=64):
        """:meth:`sweep_dop853_device` honouring terminal monitors: while a monitor is terminal (:meth:`set_terminal`) the sweep runs
        through marl_sweep_dop853_stop_dev - an instance whose terminal monitor occurs ends at that root inside the sweep kernel with
        ``status`` 1, ``t_reached`` = the root and the state there, as :meth:`sweep_rk45_device` describes it; the results are built
        the same way, with or without ``t_eval`` and ``events``.  While none is, it is :meth:`sweep_dop853_device`."""
        if not any(self.terminal):
            return self.sweep_dop853_device(y_dev_ptr, t_span, first_step, rtol, atol, max_attempts, t_eval, y_eval_dev_ptr, events, max_events)
        return self._sweep_rk_device("dop853", y_dev_ptr, t_span, first_step, rtol, atol, max_attempts, t_eval, y_eval_dev_ptr, events, max_events,
                                     terminal_entry="marl_sweep_dop853_stop_dev")

    def _sweep_rk_device(self, method, y_dev_ptr, t_span, first_step, rtol, atol, max_attempts, t_eval, y_eval_dev_ptr, events, max_events,
                         terminal_entry=True):
        """``terminal_entry``: the entry that honours terminal monitors, taken while one is set - True: marl_sweep_<method>_terminal_dev;
        a name: that entry; False: the method has none here, and its other entries refuse the call."""
        if terminal_entry is True:
            terminal_entry = f"marl_sweep_{method}_terminal_dev"
        head = _run_head(self, C.c_void_p(y_dev_ptr), t_span, first_step, rtol, atol) + (int(max_attempts),)
        return _sweep_choose(self, method, terminal_entry, head, t_eval, y_eval_dev_ptr, events, max_events)


__all__ = ["LMAHeureuxPorosityDiff", "DepthGrid", "RK45Result", "FIELD_NAMES", "EVENT_NAMES", "terminal_counts", "LAYOUT_FIELD_MAJOR", "LAYOUT_TILED"]
