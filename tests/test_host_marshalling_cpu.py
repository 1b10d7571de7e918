"""The Python host layer's marshalling, characterised call by call: which C entry a method reaches, the argument tuple it hands over
and what it builds from what the entry fills in.  No GPU and no libmarl_hip.so: the real methods run unbound on stand-ins whose
``_lib`` records ``(entry name, args)`` and writes - through the ctypes pointers it is handed - what the entry would write.

(a) the sweeps of the model, (b) its single runs, (c) HipSweepEngine, (d) the routes of integrate_equations.  The expected entries
and keyword arguments are spelled out here, rule by rule, not taken from the package."""
import ctypes as C
import itertools
import re
import types

import numpy as np
import pytest

from common import scenario
from marlpde_amd import _abi
from marlpde_amd.LHeureux_model import DepthGrid, LMAHeureuxPorosityDiff, RK45Result

STOP = [0, 0, 0, 0, 1, 0, 0]
T_EVALS = {"none": None, "empty": [], "two": [0.25, 0.5]}
ROOTS = {"off": (False, 64), "three": (True, 3), "zero": (True, 0)}
COUNTS = [[5, 0, 2, 0, 0, 0, 1], [0, 4, 0, 0, 3, 0, 9]]      # sign changes the fake entries report: some above max_events = 3
FRAMES_PTR = 456


def _doubles(ptr, shape):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_double)), shape)


def _longs(ptr, shape):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_int64)), shape)


def _value(p):
    return None if p is None else p.value


class Lib:
    """A library whose every entry records its call, lets ``fill`` write the outputs and returns 0."""

    def __init__(self, fill):
        self.calls, self.fill = [], fill

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            self.fill(name, args)
            return 0
        return entry


def _borrow(cls, *names):
    for name in names:
        setattr(cls, name, getattr(LMAHeureuxPorosityDiff, name))
    return cls


def _root_time(b, e, j):
    return 100.0 * b + 10.0 * e + j


# ---- (a) sweeps -------------------------------------------------------------------------------------------------------------------------
def _fill_sweep(name, args):
    """stats[b].n_events / .t, and n_done and the rows of tev where the entry has them: the layout follows from the argument count."""
    head = 9 if ("radau" in name or "bdf" in name) else 8
    stats = args[-1]
    rest = args[head:-1]
    samples = rest[:4] if len(rest) in (4, 6) else None
    roots = rest[-2:] if len(rest) in (2, 6) else None
    for b in range(2):
        stats[b].t = 0.1 * (b + 1)
        for e in range(7):
            stats[b].n_events[e] = COUNTS[b][e]
    if samples is not None:
        _longs(samples[3], (2,))[:] = [min(1, samples[1]), min(2, samples[1])]
    if roots is not None and roots[0] is not None and roots[1] > 0:
        tev = _doubles(roots[0], (2, 7, roots[1]))
        for b, e, j in itertools.product(range(2), range(7), range(roots[1])):
            if j < COUNTS[b][e]:
                tev[b, e, j] = _root_time(b, e, j)


def _sweep_model(terminal):
    class Real:
        n_instances = 2
        _ctx = "ctx"

        def __init__(self):
            self._lib, self.terminal, self.checked = Lib(_fill_sweep), list(terminal), []

        def _check(self, rc, what):
            self.checked.append(what)
            assert rc == 0
            return rc

    return _borrow(Real, "sweep_rk45_device", "sweep_rk23_device", "sweep_dop853_device", "sweep_dop853_stop_device", "sweep_bdf_device",
                   "sweep_radau_device", "_sweep_rk_device")()


SWEEPS = {   # method -> (family in the entries' names, family in the error text, the entry that honours a terminal monitor or None)
    "sweep_rk45_device": ("rk45", "rk45", "marl_sweep_rk45_terminal_dev"),
    "sweep_rk23_device": ("rk23", "rk23", "marl_sweep_rk23_terminal_dev"),
    "sweep_dop853_device": ("dop853", "dop853", None),
    "sweep_dop853_stop_device": ("dop853", "dop853", "marl_sweep_dop853_stop_dev"),
    "sweep_bdf_device": ("bdf", "bdf", "marl_sweep_bdf_terminal_dev"),
    "sweep_radau_device": ("radau", "radau", None),
}


def _expected_sweep(method, t_eval, events, max_events, terminal):
    """-> (entry, has sample arguments, has root arguments, t is None, t_events is None): today's rules."""
    family, _, stop_entry = SWEEPS[method]
    locate = events and max_events > 0
    if family == "radau":
        if t_eval is not None:
            return "marl_sweep_radau_eval_dev", True, True, False, not locate
        if not events:
            return "marl_sweep_radau_dev", False, False, True, True
        return "marl_sweep_radau_events_dev", False, True, True, False      # even with max_events == 0: seven empty arrays
    if any(terminal) and stop_entry:
        return stop_entry, True, True, t_eval is None, not locate
    if t_eval is None and not locate:
        return f"marl_sweep_{family}_dev", False, False, True, True
    if locate:
        return f"marl_sweep_{family}_events_dev", True, True, t_eval is None, False
    return f"marl_sweep_{family}_eval_dev", True, False, False, True


@pytest.mark.parametrize("terminal", [[0] * 7, STOP], ids=["free", "stop"])
@pytest.mark.parametrize("roots", list(ROOTS))
@pytest.mark.parametrize("samples", list(T_EVALS))
@pytest.mark.parametrize("method", list(SWEEPS))
def test_sweep_entry_arguments_and_results(method, samples, roots, terminal):
    t_eval, (events, max_events) = T_EVALS[samples], ROOTS[roots]
    implicit = method in ("sweep_bdf_device", "sweep_radau_device")
    m = _sweep_model(terminal)
    grp = np.arange(10, dtype=np.int32)
    more = {"groups": grp} if implicit and samples == "two" else {}
    res = getattr(m, method)(123, (0.0, 1.0), 1e-3, 1e-5, 1e-7, 9, t_eval=t_eval, y_eval_dev_ptr=FRAMES_PTR, events=events, max_events=max_events, **more)
    entry, has_samples, has_roots, t_none, roots_none = _expected_sweep(method, t_eval, events, max_events, terminal)
    assert [name for name, _ in m._lib.calls] == [entry] and m.checked == [entry]
    args = m._lib.calls[0][1]
    assert len(args) == len(_abi.PROTOTYPES[entry][1])
    assert args[0] == "ctx" and args[1].value == 123 and args[2:7] == (0.0, 1.0, 1e-3, 1e-5, 1e-7)
    head = 8
    if implicit:      # groups sits before max_attempts
        assert _value(args[7]) == (grp.ctypes.data if more else None)
        head = 9
    assert args[head - 1] == 9 and type(args[head - 1]) is int
    rest = args[head:-1]
    assert len(rest) == 4 * has_samples + 2 * has_roots
    n = 0 if t_eval is None else len(t_eval)
    if has_samples:
        if n:
            assert np.array_equal(_doubles(rest[0], (n,)), t_eval) and rest[1] == n and rest[2].value == FRAMES_PTR
        else:
            assert rest[0] is None and rest[1] == 0 and rest[2] is None
        assert rest[3] is not None
    if has_roots:
        tev_ptr, room = rest[-2:]
        if entry == "marl_sweep_radau_events_dev":
            assert tev_ptr is not None and room == max_events
        elif events and max_events > 0:
            assert tev_ptr is not None and room == max_events
        else:
            assert tev_ptr is None and room == 0
    assert len(res) == 2 and all(isinstance(r, RK45Result) for r in res)
    for b, r in enumerate(res):
        assert r.t_reached == 0.1 * (b + 1) and r.n_events.tolist() == COUNTS[b] and r.y is None
        if t_none:
            assert r.t is None
        else:
            assert np.array_equal(r.t, np.asarray(t_eval, dtype=float)[:min(b + 1, n)]) and r.t.dtype == np.float64
        if roots_none:
            assert r.t_events is None
        else:
            assert [len(t) for t in r.t_events] == [min(c, max_events) for c in COUNTS[b]]
            assert all(t[j] == _root_time(b, e, j) for e, t in enumerate(r.t_events) for j in range(len(t)))


@pytest.mark.parametrize("terminal", [[0] * 7, STOP], ids=["free", "stop"])
@pytest.mark.parametrize("method", list(SWEEPS))
def test_sweep_t_eval_without_a_frame_buffer_is_refused(method, terminal):
    for events, max_events in ROOTS.values():
        m = _sweep_model(terminal)
        with pytest.raises(ValueError) as err:
            getattr(m, method)(123, (0.0, 1.0), 1e-3, 1e-5, 1e-7, 9, t_eval=[0.25, 0.5], events=events, max_events=max_events)
        assert str(err.value).startswith(f"sweep_{SWEEPS[method][1]}_device: t_eval needs y_eval_dev_ptr") and m._lib.calls == []
        getattr(m, method)(123, (0.0, 1.0), 1e-3, 1e-5, 1e-7, 9, t_eval=[], events=events, max_events=max_events)      # nothing to write: no buffer needed
        assert len(m._lib.calls) == 1


def test_sweep_dop853_stop_without_a_limit_is_sweep_dop853_device():
    seen = []

    class M:
        terminal = [0] * 7

        def sweep_dop853_device(self, *a, **kw):
            seen.append((a, kw))
            return "free"

    assert LMAHeureuxPorosityDiff.sweep_dop853_stop_device(M(), 123, (0.0, 1.0), 1e-3, 1e-5, 1e-7, 9, [0.5], 456, True, 3) == "free"
    assert seen == [((123, (0.0, 1.0), 1e-3, 1e-5, 1e-7, 9, [0.5], 456, True, 3), {})]


def _fill_watch_sweep(name, args):
    assert name == "marl_sweep_rk4_watch_dev"
    stats, n_frames, room = args[-1], args[6], args[10]
    for b in range(2):
        stats[b].t, stats[b].n_accepted = 0.5 * (b + 1), 4
        for e in range(7):
            stats[b].n_events[e] = COUNTS[b][e]
    _longs(args[8], (2,))[:] = [min(2, n_frames), min(3, n_frames)]
    if args[9] is not None:
        tev = _doubles(args[9], (2, 7, room))
        for b, e, j in itertools.product(range(2), range(7), range(room)):
            if j < COUNTS[b][e]:
                tev[b, e, j] = _root_time(b, e, j)


@pytest.mark.parametrize("dt", [0.125, [0.125, 0.25]], ids=["one-dt", "dt-each"])
@pytest.mark.parametrize("frame_steps", [None, [0, 2, 4]], ids=["no-frames", "frames"])
@pytest.mark.parametrize("roots", list(ROOTS))
def test_sweep_rk4_watch_arguments_and_results(roots, frame_steps, dt):
    events, max_events = ROOTS[roots]

    class Real:
        n_instances = 2
        _ctx = "ctx"
        _lib = Lib(_fill_watch_sweep)

        def _check(self, rc, what):
            assert rc == 0 and what == "marl_sweep_rk4_watch_dev"

    m = _borrow(Real, "sweep_rk4_watch_device")()
    res = m.sweep_rk4_watch_device(123, dt, 4, t0=1.0, frame_steps=frame_steps, frames_dev_ptr=FRAMES_PTR if frame_steps else None,
                                   events=events, max_events=max_events)
    (name, args), = m._lib.calls
    assert name == "marl_sweep_rk4_watch_dev" and len(args) == len(_abi.PROTOTYPES[name][1])
    dts = np.broadcast_to(np.asarray(dt, dtype=float), (2,))
    assert args[0] == "ctx" and args[1].value == 123 and args[2] == 1.0 and np.array_equal(_doubles(args[3], (2,)), dts) and args[4] == 4
    if frame_steps:
        assert np.array_equal(_longs(args[5], (3,)), frame_steps) and args[6] == 3 and args[7].value == FRAMES_PTR
    else:
        assert args[5] is None and args[6] == 0 and args[7] is None
    locate = events and max_events > 0
    assert (args[9] is not None, args[10]) == ((True, max_events) if locate else (False, 0))
    for b, r in enumerate(res):
        if frame_steps is None:
            assert r.t is None
        else:
            assert np.array_equal(r.t, 1.0 + np.array(frame_steps[:b + 2]) * dts[b])
        if locate:
            assert [len(t) for t in r.t_events] == [min(c, max_events) for c in COUNTS[b]]
            assert all(t[j] == _root_time(b, e, j) for e, t in enumerate(r.t_events) for j in range(len(t)))
        else:
            assert r.t_events is None
    with pytest.raises(ValueError, match="sweep_rk4_watch_device: frame_steps needs frames_dev_ptr"):
        m.sweep_rk4_watch_device(123, dt, 4, frame_steps=[0, 2])


# ---- (b) single runs ---------------------------------------------------------------------------------------------------------------------
NCELLS = 2
Y0 = np.arange(1.0, 5 * NCELLS + 1)
SINGLE_COUNTS = [7, 0, 2, 0, 0, 0, 1]
T_STOPPED = 0.3
SINGLES = {   # method -> (entry, takes groups)
    "integrate_rk45": ("marl_integrate_rk45", False), "integrate_rk23": ("marl_integrate_rk23", False),
    "integrate_dop853": ("marl_integrate_dop853", False), "integrate_rk45_terminal": ("marl_integrate_rk45_terminal", False),
    "integrate_rk23_terminal": ("marl_integrate_rk23_terminal", False), "integrate_dop853_stop": ("marl_integrate_dop853_stop", False),
    "integrate_dop853_grid": ("marl_integrate_dop853_grid", False), "integrate_radau": ("marl_integrate_radau", True),
    "integrate_bdf": ("marl_integrate_bdf", True),
}


class SingleLib(Lib):
    """Every call notes the state it was handed, overwrites it, reports SINGLE_COUNTS sign changes and ends at T_STOPPED."""

    def __init__(self):
        super().__init__(self.fill_single)
        self.states_seen = []

    def fill_single(self, name, args):
        n = Y0.size
        y = _doubles(args[1], (n,))
        self.states_seen.append(y.copy())
        y[:] = -1.0 * len(self.calls) - np.arange(n)
        stats = args[-1]._obj
        stats.t, stats.nfev = T_STOPPED, 11
        if name == "marl_integrate_rk4_watch":
            fs, n_frames, frames, n_done, tev, room = args[5:11]
            _longs(n_done, (1,))[0] = min(2, n_frames)
        else:
            te, n_frames, frames, tev, room = args[-7:-2]
        if frames is not None:
            _doubles(frames, (n_frames, n))[:] = 1000.0 * np.arange(n_frames)[:, None] + np.arange(n)
        for e in range(7):
            stats.n_events[e] = SINGLE_COUNTS[e]
        if tev is not None and room > 0:
            rows = _doubles(tev, (7, room))
            for e, j in itertools.product(range(7), range(room)):
                if j < SINGLE_COUNTS[e]:
                    rows[e, j] = _root_time(0, e, j)


def _single_model():
    class One:
        n_instances = 1
        Depths = DepthGrid(1.0, NCELLS)
        _ctx = "ctx"
        terminal = (0,) * 7

        def __init__(self):
            self._lib, self.checked = SingleLib(), []

        def _check(self, rc, what):
            self.checked.append(what)
            assert rc == 0
            return rc

    return _borrow(One, "_host_state", "_integrate_rk", "_integrate_implicit", "integrate_rk4_watch", *SINGLES)()


def _roots_are_all_there(res):
    assert [len(t) for t in res.t_events] == SINGLE_COUNTS
    assert all(t[j] == _root_time(0, e, j) for e, t in enumerate(res.t_events) for j in range(len(t)))


@pytest.mark.parametrize("method", list(SINGLES))
def test_single_run_entry_arguments_retry_and_result(method):
    entry, implicit = SINGLES[method]
    t_eval = [0.1, 0.2, 0.3, 0.4]
    grp = np.arange(Y0.size, dtype=np.int32)
    # the retry: 7 sign changes do not fit max_events = 4, so the run is repeated once, from the same start, with room for 7
    m = _single_model()
    y0 = Y0.copy()
    res = getattr(m, method)(y0, (0.0, 1.0), 1e-3, 1e-5, 1e-7, t_eval=t_eval, events=True, max_events=4, max_attempts=9, **({"groups": grp} if implicit else {}))
    assert [name for name, _ in m._lib.calls] == [entry] * 2 and m.checked == [entry] * 2
    assert np.array_equal(y0, Y0) and all(np.array_equal(y, Y0) for y in m._lib.states_seen)      # the start state is copied per attempt
    for (_, args), room in zip(m._lib.calls, (4, 7)):
        assert len(args) == len(_abi.PROTOTYPES[entry][1])
        assert args[0] == "ctx" and args[2:7] == (0.0, 1.0, 1e-3, 1e-5, 1e-7)
        if implicit:      # groups follows atol
            assert args[7].value == grp.ctypes.data
        te, n_eval, frames, tev, max_events, max_attempts = args[-7:-1]
        assert np.array_equal(_doubles(te, (4,)), t_eval) and n_eval == 4 and frames is not None and tev is not None
        assert max_events == room and max_attempts == 9
    _roots_are_all_there(res)
    k = int(np.searchsorted(t_eval, T_STOPPED, side="right"))
    assert k == 3 and np.array_equal(res.t, t_eval[:k])
    assert res.y.shape == (Y0.size, k) and np.array_equal(res.y, (1000.0 * np.arange(k)[:, None] + np.arange(Y0.size)).T)
    assert np.array_equal(res.y_final, -2.0 - np.arange(Y0.size)) and res.nfev == 11 and res.t_reached == T_STOPPED

    # without t_eval: the end point only; room enough: one call
    m = _single_model()
    res = getattr(m, method)(Y0, (0.0, 1.0), 1e-3, 1e-5, 1e-7, events=True, max_events=8)
    (_, args), = m._lib.calls
    assert args[-7:-4] == (None, 0, None) and args[-3] == 8 and args[-2] == 0
    if implicit:
        assert args[7] is None
    _roots_are_all_there(res)
    assert np.array_equal(res.t, [T_STOPPED]) and np.array_equal(res.y, (-1.0 - np.arange(Y0.size))[:, None])
    assert np.array_equal(res.y_final, -1.0 - np.arange(Y0.size))

    # an empty t_eval is no t_eval
    m = _single_model()
    res = getattr(m, method)(Y0, (0.0, 1.0), 1e-3, 1e-5, 1e-7, t_eval=[], events=False)
    assert m._lib.calls[0][1][-7:-4] == (None, 0, None) and np.array_equal(res.t, [T_STOPPED]) and res.y.shape == (Y0.size, 1)

    # events=False: no root buffer, no retry, no t_events
    m = _single_model()
    res = getattr(m, method)(Y0, (0.0, 1.0), 1e-3, 1e-5, 1e-7, t_eval=t_eval, events=False, max_events=4)
    (_, args), = m._lib.calls
    assert args[-4] is None and args[-3] == 0 and res.t_events is None and np.array_equal(res.t, t_eval[:3])
    assert np.array_equal(res.y_final, -1.0 - np.arange(Y0.size))

    with pytest.raises(ValueError, match="state has 3 entries, expected 10"):
        getattr(m, method)(np.zeros(3), (0.0, 1.0), 1e-3, 1e-5, 1e-7)
    if implicit:
        with pytest.raises(ValueError, match="groups has 3 entries, expected 10"):
            getattr(m, method)(Y0, (0.0, 1.0), 1e-3, 1e-5, 1e-7, groups=[0, 1, 2])


def test_single_rk4_watch_arguments_retry_and_result():
    entry = "marl_integrate_rk4_watch"
    m = _single_model()
    y0 = Y0.copy()
    res = m.integrate_rk4_watch(y0, 0.125, 4, t0=1.0, frame_steps=[0, 2, 4], events=True, max_events=4)
    assert [name for name, _ in m._lib.calls] == [entry] * 2 and m.checked == [entry] * 2
    assert np.array_equal(y0, Y0) and all(np.array_equal(y, Y0) for y in m._lib.states_seen)
    for (_, args), room in zip(m._lib.calls, (4, 7)):
        assert len(args) == len(_abi.PROTOTYPES[entry][1])
        assert args[0] == "ctx" and args[2:5] == (1.0, 0.125, 4)
        assert np.array_equal(_longs(args[5], (3,)), [0, 2, 4]) and args[6] == 3 and args[7] is not None and args[8] is not None
        assert args[9] is not None and args[10] == room
    _roots_are_all_there(res)
    assert np.array_equal(res.t, 1.0 + np.array([0, 2]) * 0.125)
    assert np.array_equal(res.y, (1000.0 * np.arange(2)[:, None] + np.arange(Y0.size)).T)
    assert np.array_equal(res.y_final, -2.0 - np.arange(Y0.size))

    # no frames: the end point; events=True without room locates nothing - seven empty arrays, one call
    m = _single_model()
    res = m.integrate_rk4_watch(Y0, 0.125, 4, events=True, max_events=0)
    (_, args), = m._lib.calls
    assert args[5:8] == (None, 0, None) and args[9] is None and args[10] == 0
    assert len(res.t_events) == 7 and all(isinstance(t, np.ndarray) and t.size == 0 for t in res.t_events)
    assert np.array_equal(res.t, [T_STOPPED]) and np.array_equal(res.y, (-1.0 - np.arange(Y0.size))[:, None])
    assert np.array_equal(res.y_final, -1.0 - np.arange(Y0.size))

    m = _single_model()
    res = m.integrate_rk4_watch(Y0, 0.125, 4, frame_steps=[], events=False, max_events=4)
    (_, args), = m._lib.calls
    assert args[5:8] == (None, 0, None) and args[9] is None and args[10] == 0 and res.t_events is None
    assert res.t.size == 0 and res.y.shape == (Y0.size, 0)      # an empty frame list is still a frame list


# ---- (c) the engine -----------------------------------------------------------------------------------------------------------------------
ENGINE = {   # engine method -> (the model's sweep, y0 is made float64, keyword arguments fixed by the method)
    "integrate_rk45": ("sweep_rk45_device", False), "integrate_rk23": ("sweep_rk23_device", False),
    "integrate_dop853": ("sweep_dop853_device", False), "integrate_dop853_stop": ("sweep_dop853_stop_device", False),
    "integrate_radau": ("sweep_radau_device", False), "integrate_bdf": ("sweep_bdf_device", True),
    "integrate_rk4_watch": ("sweep_rk4_watch_device", True),
}


def _engine(state_dtype):
    import torch
    from marlpde_amd.sweep import HipSweepEngine
    order = []

    class Model:
        def set_terminal(self, spec):
            order.append(("set_terminal", spec))

        def __getattr__(self, name):
            if not name.startswith("sweep_"):
                raise AttributeError(name)

            def sweep(y_ptr, *a, **kw):
                order.append((name, a, kw))
                kind = np.ctypeslib.as_ctypes_type(state_dtype)      # the sweep advances the states in place
                np.ctypeslib.as_array(C.cast(y_ptr, C.POINTER(kind)), (2, 10))[:] += 1
                ptr = kw.get("y_eval_dev_ptr", kw.get("frames_dev_ptr"))
                samples = kw.get("t_eval", kw.get("frame_steps"))
                res = []
                for b in range(2):
                    r = types.SimpleNamespace(t=None, y=None)
                    if samples is not None:
                        n = len(samples)
                        _doubles(C.c_void_p(ptr), (2, max(n, 1), 10))[b] = 100.0 * b + 10.0 * np.arange(max(n, 1))[:, None] + np.arange(10) / 16
                        r.t = np.asarray(samples, dtype=float)[:min(b + 1, n)]
                    res.append(r)
                return res
            return sweep

    class OnDevice(torch.Tensor):      # CPU memory that is copied on the way back, as device memory is
        def cpu(self):
            return self.clone().as_subclass(torch.Tensor)

    class OnHost(torch.Tensor):      # ... and on the way there
        def to(self, device):
            assert device == "cpu"
            return self.clone().as_subclass(OnDevice)

    class Torch:
        empty = staticmethod(torch.empty)

        @staticmethod
        def from_numpy(a):
            return torch.from_numpy(a).as_subclass(OnHost)

    class Engine:
        device = "cpu"
        model = Model()
        torch = Torch

    for name in ("_integrate_rk", *ENGINE):
        setattr(Engine, name, getattr(HipSweepEngine, name))
    return Engine(), order


@pytest.mark.parametrize("events", [False, True], ids=["counts", "roots"])
@pytest.mark.parametrize("samples", list(T_EVALS))
@pytest.mark.parametrize("method", list(ENGINE))
def test_engine_sets_terminal_uploads_sweeps_once_and_attaches_the_frames(method, samples, events):
    sweep, forced = ENGINE[method]
    wanted = T_EVALS[samples] if method != "integrate_rk4_watch" else {"none": None, "empty": [], "two": [0, 2]}[samples]
    # single-precision states where no frames are written through the pointer (the fake model writes doubles), or where the method converts
    given = (np.arange(20.0) / 8).reshape(2, 10).astype(np.float32 if forced or wanted is None else np.float64)
    y0 = given.copy()
    engine, order = _engine(np.float64 if forced else y0.dtype)
    ask = {"events": True, "max_events": 5} if events else {}
    if method == "integrate_rk4_watch":
        y, res = engine.integrate_rk4_watch(y0, 0.125, 4, t0=1.0, frame_steps=wanted, terminal=STOP, **ask)
        a, kw, names = (0.125, 4), {"t0": 1.0}, ("frame_steps", "frames_dev_ptr")
    else:
        more = {"batched": True} if method == "integrate_bdf" else {}
        y, res = getattr(engine, method)(y0, (0.0, 1.0), 1e-3, 1e-5, 1e-7, 9, t_eval=wanted, terminal=STOP, **ask, **more)
        a, kw, names = ((0.0, 1.0), 1e-3, 1e-5, 1e-7, 9), {}, ("t_eval", "y_eval_dev_ptr")
    assert len(order) == 2 and order[0] == ("set_terminal", STOP) and order[1][:2] == (sweep, a)      # the limits first, then exactly one sweep
    got = dict(order[1][2])
    if wanted is not None:
        assert got.pop(names[0]) is wanted and isinstance(got.pop(names[1]), int)
    assert got == kw | ask
    assert np.array_equal(y0, given)      # uploaded, not advanced in place
    assert np.array_equal(y, given + 1)      # the uploaded states as the sweep left them: fetched after it, not before
    assert y.dtype == (np.float64 if forced else y0.dtype)      # each method keeps its own conversion of y0
    assert len(res) == 2
    for b, r in enumerate(res):
        if wanted is None:
            assert r.y is None
        else:
            n = len(r.t)
            assert n == min(b + 1, len(wanted)) and r.y.shape == (10, n) and r.y.dtype == y.dtype
            assert np.array_equal(r.y, (100.0 * b + 10.0 * np.arange(n)[:, None] + np.arange(10) / 16).T)


# ---- (d) integrate_equations ---------------------------------------------------------------------------------------------------------------
class _Model:
    """Stands where LMAHeureuxPorosityDiff stands in Evolve_scenario: notes every call and answers with the status it is told to."""
    log = []
    status = 0

    def __init__(self, N):
        self.N = N

    @classmethod
    def from_scenario(cls, pde_parms, device=0):
        return cls(int(pde_parms["N"]))

    def get_state(self, *surface):
        return np.repeat(np.asarray(surface, float), self.N).reshape(5, self.N)

    def set_terminal(self, spec):
        self.log.append(("set_terminal", tuple(spec)))

    def close(self):
        self.log.append(("close",))

    def fun(self, t, y, *args):
        return -np.asarray(y)

    def __getattr__(self, name):
        if name.startswith(("zeros", "ones")):      # the seven monitors
            return lambda t, y, *args: 1.0
        if not name.startswith("integrate_"):
            raise AttributeError(name)

        def integrate(y0, *a, **kw):
            self.log.append((name, a, kw))
            st = _abi.MarlStats()
            st.status, st.nfev, st.njev, st.nlu = self.status, 40, 5, 6
            st.t = 0.25 * (a[0][1] if name != "integrate_rk4_watch" else 1e-4)
            return RK45Result(st, np.array([st.t]), np.asarray(y0, float)[:, None].copy(), [np.empty(0)] * 7)
        return integrate


ADAPTIVE = dict(first_step=1e-6, rtol=1e-3, atol=1e-3, t_span=(0.0, 1e-4), backend="hip")
LIMITS = (0, 0, 0, 0, 1, 0, 0)
ZEROS = (0,) * 7
TERM = {"ones_Phi": True}
CAN_STOP, CANNOT_STOP, ANY = (0, 1, -1), (0, -1), None
ROUTES = [   # id, solver keys, N, terminal, the model method (None: solve_ivp), set_terminal's argument (None: not called), statuses let through, njev/nlu from the result
    ("rk4", {"method": "RK4", "dt": 2.5e-5}, 16, None, "integrate_rk4_watch", ZEROS, ANY, False),
    ("rk4-stop", {"method": "RK4", "dt": 2.5e-5}, 16, TERM, "integrate_rk4_watch", LIMITS, ANY, False),
    ("rk45", {"method": "RK45"}, 16, None, "integrate_rk45", None, CAN_STOP, False),
    ("rk45-native_terminal-no-limit", {"method": "RK45", "native_terminal": True}, 16, None, "integrate_rk45", None, CAN_STOP, False),
    ("rk45-stop", {"method": "RK45", "native_terminal": True}, 16, TERM, "integrate_rk45_terminal", LIMITS, CAN_STOP, False),
    ("rk23", {"method": "RK23"}, 16, None, "integrate_rk23", None, CAN_STOP, False),
    ("rk23-stop", {"method": "RK23", "native_terminal": True}, 16, TERM, "integrate_rk23_terminal", LIMITS, CAN_STOP, False),
    ("rk45-scipy", {"method": "RK45", "scipy_driver": True}, 16, TERM, None, None, None, None),
    ("dop853", {"method": "DOP853"}, 16, None, "integrate_dop853", None, CANNOT_STOP, False),
    ("dop853-1024-native_grid", {"method": "DOP853", "native_grid": True}, 1024, None, "integrate_dop853", None, CANNOT_STOP, False),
    ("dop853-stop", {"method": "DOP853", "native_terminal": True}, 16, TERM, "integrate_dop853_stop", LIMITS, CAN_STOP, False),
    ("dop853-stop-1024", {"method": "DOP853", "native_terminal": True}, 1024, TERM, "integrate_dop853_stop", LIMITS, CAN_STOP, False),
    ("dop853-limit-not-native", {"method": "DOP853"}, 16, TERM, None, None, None, None),
    ("dop853-stop-1025", {"method": "DOP853", "native_terminal": True}, 1025, TERM, None, None, None, None),
    ("dop853-1025", {"method": "DOP853"}, 1025, None, None, None, None, None),
    ("dop853-grid", {"method": "DOP853", "native_grid": True}, 1025, None, "integrate_dop853_grid", ZEROS, CAN_STOP, False),
    ("dop853-grid-stop", {"method": "DOP853", "native_grid": True, "native_terminal": True}, 1025, TERM, "integrate_dop853_grid", LIMITS, CAN_STOP, False),
    ("dop853-grid-limit-not-native", {"method": "DOP853", "native_grid": True}, 1025, TERM, None, None, None, None),
    ("radau", {"method": "Radau"}, 16, None, "integrate_radau", ZEROS, CAN_STOP, True),
    ("radau-stop", {"method": "Radau"}, 16, TERM, "integrate_radau", LIMITS, CAN_STOP, True),
    ("bdf", {"method": "BDF"}, 16, None, "integrate_bdf", ZEROS, CAN_STOP, True),
    ("bdf-scipy", {"method": "BDF", "scipy_driver": True}, 16, None, None, None, None, None),
    ("lsoda", {"method": "LSODA"}, 16, None, None, None, None, None),
]


@pytest.mark.parametrize("name, solver, N, terminal, method, limits, allowed, implicit", ROUTES, ids=[r[0] for r in ROUTES])
def test_integrate_equations_routes_statuses_and_covered_time(monkeypatch, capsys, name, solver, N, terminal, method, limits, allowed, implicit):
    import scipy.integrate
    from marlpde_amd import Evolve_scenario as es
    monkeypatch.setattr(es, "LMAHeureuxPorosityDiff", _Model)
    driven = []

    def solve_ivp(fun, t_span, y0, **kw):
        driven.append((kw["method"], [e.terminal for e in kw["events"]]))
        return types.SimpleNamespace(t=np.array([t_span[1]]), y=np.asarray(y0, float)[:, None], t_events=[np.empty(0)] * 7, nfev=3, njev=1, nlu=2,
                                     status=0, message="fake")

    monkeypatch.setattr(scipy.integrate, "solve_ivp", solve_ivp)
    parms = scenario("A", N)
    Tstar, t1 = parms["Tstar"], 1e-4
    tracker = {"t_eval": [0.0, 5e-5, 1e-4]}
    for status in ((0,) if method is None else (0, 1, -1, 2, -2)):
        _Model.log, _Model.status = [], status
        last, covered, depths, Xstar, folder = es.integrate_equations(ADAPTIVE | solver, tracker, parms, results_root=None, terminal=terminal)
        out = capsys.readouterr().out
        assert last.shape == (5, N) and depths.N == N and Xstar == parms["Xstar"] and folder is None
        calls = [c for c in _Model.log if c[0].startswith("integrate_")]
        if method is None:      # solve_ivp on the HIP RHS: no native run, no limits handed to the library
            assert calls == [] and len(driven) == 1 and driven[0][0] == solver["method"] and _Model.log == [("close",)]
            assert driven[0][1] == [lim if lim else False for lim in (LIMITS if terminal else ZEROS)]
            assert covered == Tstar * t1
            continue
        assert driven == [] and len(calls) == 1 and calls[0][0] == method
        assert [c for c in _Model.log if c[0] == "set_terminal"] == ([] if limits is None else [("set_terminal", limits)])
        assert _Model.log[-1] == ("close",) and _Model.log[-2] is calls[0]      # the limits, then the run, then close
        if method == "integrate_rk4_watch":
            (dt, nsteps), kw = calls[0][1], dict(calls[0][2])
            assert (dt, nsteps, kw.pop("t0")) == (2.5e-5, 4, 0.0) and np.array_equal(kw.pop("frame_steps"), [0, 2, 4]) and kw == {}
        else:
            assert calls[0][1] == ((0.0, 1e-4), 1e-6, 1e-3, 1e-3)
            assert calls[0][2] == ({"t_eval": tracker["t_eval"], "groups": None} if implicit else {"t_eval": tracker["t_eval"]})
        shown = status if allowed is None or status in allowed else -1
        njev, nlu = (5, 6) if implicit else (0, 0)
        assert re.match(rf"rhs evaluations 40, Jacobian evaluations {njev}, LU decompositions {nlu}, status {shown}\n", out), out
        assert covered == Tstar * (t1 if status == 0 else 0.25 * t1)


@pytest.mark.parametrize("method", ["RK45", "RK23"])
def test_integrate_equations_refuses_limits_in_the_explicit_loops_without_an_opt_in(monkeypatch, method):
    from marlpde_amd import Evolve_scenario as es
    monkeypatch.setattr(es, "LMAHeureuxPorosityDiff", _Model)
    _Model.log = []
    with pytest.raises(ValueError) as err:
        es.integrate_equations(ADAPTIVE | {"method": method}, {}, scenario("A", 16), results_root=None, verbose=False, terminal=TERM)
    assert str(err.value) == (f"terminal monitors in the {method} loop are opt-in: pass native_terminal=True in the solver parameters for the native loop "
                              "(marl_integrate_rk45_terminal / rk23_terminal) or scipy_driver=True for solve_ivp on the HIP RHS, or use method 'Radau' or 'BDF'")
    assert _Model.log == [("close",)]      # closed before the raise, nothing run


def test_integrate_equations_rk4_schedule_runs_before_the_model_exists(monkeypatch):
    from marlpde_amd import Evolve_scenario as es

    class Never:
        @classmethod
        def from_scenario(cls, *a, **kw):
            raise AssertionError("a model was built")

    monkeypatch.setattr(es, "LMAHeureuxPorosityDiff", Never)
    with pytest.raises(ValueError, match="method 'RK4' is a fixed-step method"):
        es.integrate_equations(ADAPTIVE | {"method": "RK4"}, {}, scenario("A", 16), results_root=None, verbose=False)
