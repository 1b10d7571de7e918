"""DOP853 sweeps and the scenario driver, the parts that need no GPU: the four C entries are declared and bound with the argument lists of
their RK45 namesakes; run_sweep_dop853 shards, gathers and orders states, counts, frames and roots like run_sweep_rk45 (what is under test
is marlpde_amd/sweep.py; the arithmetic comes from an engine double defined here: scipy's DOP853 on the oracle's RHS, tests/dop853_ref.py);
HipSweepEngine.integrate_dop853 and LMAHeureuxPorosityDiff.sweep_dop853_device hand their arguments on; integrate_equations(method="DOP853")
takes the native branch where the native loop reaches (N <= 1024, no terminal monitor, no scipy_driver) and scipy's solve_ivp elsewhere."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from common import scenario
from test_sweep_frames_cpu import _spawn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = {"marl_integrate_dop853": "marl_integrate_rk45", "marl_sweep_dop853_dev": "marl_sweep_rk45_dev",
           "marl_sweep_dop853_eval_dev": "marl_sweep_rk45_eval_dev", "marl_sweep_dop853_events_dev": "marl_sweep_rk45_events_dev"}


def _declared(header, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, f"{name} is not declared in include/marl_hip.h"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_entries_are_declared_and_bound_like_their_rk45_namesakes():
    from marlpde_amd import _abi
    header = open(os.path.join(ROOT, "include", "marl_hip.h")).read()
    lib = _abi.load()
    for new, old in ENTRIES.items():
        assert _declared(header, new) == _declared(header, old), new
        assert _abi.PROTOTYPES[new] == _abi.PROTOTYPES[old] and hasattr(lib, new), new
        args = [None if t is _abi._P or isinstance(t, type(C.POINTER(_abi.MarlStats))) else t(0) for t in _abi.PROTOTYPES[new][1]]
        assert getattr(lib, new)(*args) == -1, new     # no context: an error, not a crash
    # what is out of scope does not exist: no _dev single run, no terminal entries
    for absent in ("marl_integrate_dop853_dev", "marl_sweep_dop853_terminal_dev", "marl_integrate_dop853_terminal"):
        assert absent not in _abi.PROTOTYPES and not hasattr(lib, absent) and absent not in header


# ---- run_sweep_dop853 ---------------------------------------------------------------------------------------------------------------
N = 64
M = 60                    # t1 = M dx^2
PHI_DIPS = (0.036, 0.038, 0.04, 0.041, 0.042, 0.044)
RTOL, ATOL = 1e-5, 1e-7


class ScipyDop853Engine:
    """Test double with HipSweepEngine's interface: every instance by scipy's DOP853 on the oracle's RHS.  It notes what reached it."""
    calls = []

    def __init__(self, base_parms, instances):
        from oracle import oracle as orc
        self.orc = orc
        self.N = int(base_parms["N"])
        self.P = [orc.params_from_dict(base_parms | inst) for inst in instances]

    def integrate_dop853(self, y0, t_span, first_step, rtol, atol, max_attempts, **more):
        from marlpde_amd._abi import MarlStats
        from marlpde_amd.LHeureux_model import RK45Result
        from dop853_ref import scipy_dop853
        type(self).calls.append(dict(more))
        t_eval, events, max_events = more.get("t_eval"), more.get("events", False), more.get("max_events", 64)
        ys, res = [], []
        for P, y in zip(self.P, y0):
            r = scipy_dop853(self.orc, P, self.N, y, t_span, first_step, rtol, atol, t_eval=t_eval, max_attempts=max_attempts)
            st = MarlStats()
            st.status, st.n_accepted, st.n_rejected, st.nfev, st.t = r.status, r.n_accepted, r.n_rejected, r.nfev, r.t
            for e in range(7):
                st.n_events[e] = len(r.t_events[e])
            ys.append(r.y_final)
            res.append(RK45Result(st, r.t_eval, None if t_eval is None else r.y_eval.T.copy(),
                                  [t[:max_events] for t in r.t_events] if events else None))
        return np.array(ys).reshape(len(self.P), 5 * self.N), res

    def close(self):
        pass


def _setup():
    base = scenario("default", N)
    L = base["max_depth"] / base["Xstar"]
    x = (np.arange(N) + 0.5) * (L / N)
    insts = [{"k3": 0.02 + 0.002 * i, "k4": 0.02 + 0.002 * i} for i in range(len(PHI_DIPS))]
    y0 = np.stack([np.repeat([float(base[k]) for k in ("CAIni", "CCIni", "cCaIni", "cCO3Ini", "PhiIni")], N) for _ in PHI_DIPS])
    for b, d in enumerate(PHI_DIPS):   # the phi_dip states of the sweep tests
        y0[b, 4 * N:] = base["PhiIni"] - d * np.exp(-((x - 0.5 * L) / (0.08 * L)) ** 2)
    return base, insts, y0, (L / N) ** 2


def _worker(rank, world, t_eval, max_attempts):
    from marlpde_amd.sweep import assign, run_sweep_dop853
    base, insts, y0, dx2 = _setup()
    factory = lambda bp, inst: ScipyDop853Engine(bp, inst)  # noqa: E731
    args = (base, insts, (0.0, M * dx2), 0.5 * dx2, RTOL, ATOL)
    kw = dict(max_attempts=max_attempts, y0=y0, engine_factory=factory, balance="round_robin")   # the gathered order differs from the arrival order
    ScipyDop853Engine.calls = []
    out = {"plain": run_sweep_dop853(*args, **kw), "frames": run_sweep_dop853(*args, **kw, t_eval=t_eval),
           "events": run_sweep_dop853(*args, **kw, events=True, max_events=1),
           "both": run_sweep_dop853(*args, **kw, t_eval=t_eval, events=True, max_events=8),
           "mine": assign(len(insts), rank, world, "round_robin"), "default_mine": None, "calls": [sorted(c) for c in ScipyDop853Engine.calls]}
    ScipyDop853Engine.calls = []
    out["own"] = run_sweep_dop853(*args, max_attempts=max_attempts, y0=y0, engine_factory=factory, gather=False)   # balance: the default
    out["default_mine"] = assign(len(insts), rank, world, "contiguous")
    return out


@pytest.mark.parametrize("world", [1, 2])
def test_run_sweep_dop853_orders_and_gathers_states_counts_frames_and_roots(oracle, world):
    from dop853_ref import scipy_dop853
    base, insts, y0, dx2 = _setup()
    t1 = M * dx2
    budget = 40   # (63 attempts reach t1)
    t_eval = t1 * np.array([0.0, 0.05, 0.2, 0.9])
    ref = [scipy_dop853(oracle, oracle.params_from_dict(base | inst), N, y0[b], (0.0, t1), 0.5 * dx2, RTOL, ATOL, t_eval=t_eval, max_attempts=budget)
           for b, inst in enumerate(insts)]
    assert all(r.status == 2 and r.n_accepted + r.n_rejected == budget for r in ref), "the attempt budget stops every run"
    fired = [sum(len(t) for t in r.t_events) for r in ref]
    frames_reached = [len(r.t_eval) for r in ref]
    assert sum(fired) >= 3 and min(fired) == 0, fired                    # some instances fire, one does not
    assert all(0 < k < len(t_eval) for k in frames_reached), frames_reached    # NaN padding is exercised in every instance
    out = _spawn(_worker, world, t_eval, budget)
    if world == 2:
        assert out[0]["mine"] == [0, 2, 4] and out[1]["mine"] == [1, 3, 5] and out[0]["default_mine"] == [0, 1, 2]
    for r in range(world):
        o = out[r]
        # t_eval / events / max_events reach the engine only when asked for
        assert o["calls"] == [[], ["t_eval"], ["events", "max_events"], ["events", "max_events", "t_eval"]]
        assert [len(o[k]) for k in ("plain", "frames", "events", "both")] == [5, 7, 6, 8]
        for k in ("plain", "frames", "events", "both"):
            y, status, n_acc, n_rej, t_reached = o[k][:5]
            assert np.array_equal(y, np.stack([q.y_final for q in ref])), k
            assert status.tolist() == [2] * len(insts) and n_acc.tolist() == [q.n_accepted for q in ref], k
            assert n_rej.tolist() == [q.n_rejected for q in ref] and np.array_equal(t_reached, [q.t for q in ref]), k
        for k in ("frames", "both"):
            n_frames, y_eval = o[k][5], o[k][6]
            assert n_frames.tolist() == frames_reached and y_eval.shape == (len(insts), len(t_eval), 5 * N)
            for b, q in enumerate(ref):
                assert np.array_equal(y_eval[b, :n_frames[b]], q.y_eval) and np.all(np.isnan(y_eval[b, n_frames[b]:])), (k, b)
        for k, cap in (("events", 1), ("both", 8)):
            roots = o[k][-1]
            assert len(roots) == len(insts)
            for b, q in enumerate(ref):
                assert len(roots[b]) == 7 and all(np.array_equal(a, w[:cap]) for a, w in zip(roots[b], q.t_events)), (k, b)
        # gather=False with the default balance: the rank's own contiguous shard
        mine = o["default_mine"]
        assert np.array_equal(o["own"][0], np.stack([ref[i].y_final for i in mine])) and o["own"][2].tolist() == [ref[i].n_accepted for i in mine]


# ---- the engine and the model hand their arguments on -------------------------------------------------------------------------------
def test_engine_and_model_route_dop853_to_its_entries():
    from marlpde_amd.LHeureux_model import LMAHeureuxPorosityDiff
    from marlpde_amd.sweep import HipSweepEngine
    seen = []

    class Model:
        terminal = [0, 0, 1, 0, 0, 0, 0]   # a terminal monitor is set: DOP853 still asks its own entries, which refuse it

        def _sweep_rk_device(self, method, *a, **kw):
            seen.append((method, a, kw))
            return "results"

    out = LMAHeureuxPorosityDiff.sweep_dop853_device(Model(), 123, (0.0, 1.0), 1e-3, 1e-5, 1e-7, 9, t_eval=[0.5], y_eval_dev_ptr=456, events=True, max_events=3)
    assert out == "results" and seen == [("dop853", (123, (0.0, 1.0), 1e-3, 1e-5, 1e-7, 9, [0.5], 456, True, 3), {"terminal_entry": False})]
    asked = []

    class Engine:
        def _integrate_rk(self, *a):
            asked.append(a)
            return "y", "res"

    assert HipSweepEngine.integrate_dop853(Engine(), "y0", (0.0, 1.0), 1e-3, 1e-5, 1e-7, 0, t_eval=[0.5], events=True, max_events=5, terminal=[1] * 7) == ("y", "res")
    assert asked == [("sweep_dop853_device", "y0", (0.0, 1.0), 1e-3, 1e-5, 1e-7, 0, [0.5], True, 5, [1] * 7)]

    # the single run goes to marl_integrate_dop853 through the shared plumbing
    single = []

    class One:
        def _integrate_rk(self, *a):
            single.append(a)
            return "r"

    assert LMAHeureuxPorosityDiff.integrate_dop853(One(), "y0", (0.0, 1.0), 1e-3, 1e-5, 1e-7, t_eval=[1.0], max_attempts=4) == "r"
    assert single == [("dop853", "y0", (0.0, 1.0), 1e-3, 1e-5, 1e-7, [1.0], True, 4096, 4)]


# ---- integrate_equations(method="DOP853") -------------------------------------------------------------------------------------------
class _FakeModel:
    """Stands where LMAHeureuxPorosityDiff stands in Evolve_scenario: notes which integrator was asked for."""
    asked = []

    def __init__(self, N):
        self.N = N

    @classmethod
    def from_scenario(cls, pde_parms, device=0):
        return cls(int(pde_parms["N"]))

    def get_state(self, *surface):
        return np.repeat(np.asarray(surface, float), self.N).reshape(5, self.N)

    def integrate_dop853(self, y0, t_span, first_step, rtol, atol, t_eval=None):
        from marlpde_amd._abi import MarlStats
        from marlpde_amd.LHeureux_model import RK45Result
        type(self).asked.append("dop853")
        st = MarlStats()
        st.t, st.nfev = t_span[1], 13
        return RK45Result(st, np.array([t_span[1]]), np.asarray(y0, float)[:, None].copy(), [np.empty(0)] * 7)

    def fun(self, t, y, *args):
        return -np.asarray(y)

    def __getattr__(self, name):   # the seven monitors
        if name.startswith(("zeros", "ones")):
            return lambda t, y, *args: 1.0
        raise AttributeError(name)

    def close(self):
        pass


def test_integrate_equations_dop853_goes_native_where_the_native_loop_reaches(monkeypatch):
    import scipy.integrate
    from marlpde_amd import Evolve_scenario as es
    monkeypatch.setattr(es, "LMAHeureuxPorosityDiff", _FakeModel)
    real = scipy.integrate.solve_ivp
    seen = []

    def forbidden(*a, **kw):
        raise AssertionError("scipy.integrate.solve_ivp was called")

    def noting(*a, **kw):
        seen.append(kw.get("method"))
        return real(*a, **kw)

    solver = dict(first_step=1e-6, rtol=1e-3, atol=1e-3, t_span=(0.0, 1e-4), backend="hip", method="DOP853")
    _FakeModel.asked = []
    monkeypatch.setattr(scipy.integrate, "solve_ivp", forbidden)
    for n in (16, 1024):
        last, covered, *_ = es.integrate_equations(solver, {}, scenario("A", n), results_root=None, verbose=False)
        assert last.shape == (5, n) and covered == scenario("A", n)["Tstar"] * 1e-4
    assert _FakeModel.asked == ["dop853", "dop853"]
    # what the native loop refuses keeps today's route: scipy on the HIP RHS
    monkeypatch.setattr(scipy.integrate, "solve_ivp", noting)
    es.integrate_equations(solver | {"scipy_driver": True}, {}, scenario("A", 16), results_root=None, verbose=False)
    es.integrate_equations(solver, {}, scenario("A", 1025), results_root=None, verbose=False)
    es.integrate_equations(solver, {}, scenario("A", 16), results_root=None, verbose=False, terminal={"zeros_U": True})
    assert seen == ["DOP853"] * 3 and _FakeModel.asked == ["dop853", "dop853"]
