"""RK23 sweeps and the scenario driver, the parts that need no GPU: the five C entries are declared and bound with the argument lists of
their RK45 namesakes; run_sweep_rk23 shards, gathers and orders states, counts, frames and roots like run_sweep_rk45 (what is under test is
marlpde_amd/sweep.py; the arithmetic comes from an engine double defined here: scipy's RK23 on the oracle's RHS, tests/rk23_ref.py);
integrate_equations(method="RK23") takes the native branch and never calls scipy's solve_ivp, and scipy_driver=True still does."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from common import scenario
from test_sweep_frames_cpu import _spawn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = {"marl_integrate_rk23": "marl_integrate_rk45", "marl_integrate_rk23_dev": "marl_integrate_rk45_dev", "marl_sweep_rk23_dev": "marl_sweep_rk45_dev",
           "marl_sweep_rk23_eval_dev": "marl_sweep_rk45_eval_dev", "marl_sweep_rk23_events_dev": "marl_sweep_rk45_events_dev"}


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


# ---- run_sweep_rk23 ---------------------------------------------------------------------------------------------------------------
N = 64
M = 60                    # t1 = M dx^2
PHI_DIPS = (0.036, 0.038, 0.04, 0.041, 0.042, 0.044)
RTOL, ATOL = 1e-5, 1e-7


class ScipyRk23Engine:
    """Test double with HipSweepEngine's interface: every instance by scipy's RK23 on the oracle's RHS.  It notes what reached it."""
    calls = []

    def __init__(self, base_parms, instances):
        from oracle import oracle as orc
        self.orc = orc
        self.N = int(base_parms["N"])
        self.P = [orc.params_from_dict(base_parms | inst) for inst in instances]

    def integrate_rk23(self, y0, t_span, first_step, rtol, atol, max_attempts, **more):
        from marlpde_amd._abi import MarlStats
        from marlpde_amd.LHeureux_model import RK45Result
        from rk23_ref import scipy_rk23
        type(self).calls.append(dict(more))
        t_eval, events, max_events = more.get("t_eval"), more.get("events", False), more.get("max_events", 64)
        ys, res = [], []
        for P, y in zip(self.P, y0):
            r = scipy_rk23(self.orc, P, self.N, y, t_span, first_step, rtol, atol, t_eval=t_eval, max_attempts=max_attempts)
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
    from marlpde_amd.sweep import assign, run_sweep_rk23
    base, insts, y0, dx2 = _setup()
    factory = lambda bp, inst: ScipyRk23Engine(bp, inst)  # noqa: E731
    args = (base, insts, (0.0, M * dx2), 0.5 * dx2, RTOL, ATOL)
    kw = dict(max_attempts=max_attempts, y0=y0, engine_factory=factory, balance="round_robin")   # the gathered order differs from the arrival order
    ScipyRk23Engine.calls = []
    out = {"plain": run_sweep_rk23(*args, **kw), "frames": run_sweep_rk23(*args, **kw, t_eval=t_eval),
           "events": run_sweep_rk23(*args, **kw, events=True, max_events=1),
           "both": run_sweep_rk23(*args, **kw, t_eval=t_eval, events=True, max_events=8),
           "mine": assign(len(insts), rank, world, "round_robin"), "default_mine": None, "calls": [sorted(c) for c in ScipyRk23Engine.calls]}
    ScipyRk23Engine.calls = []
    out["own"] = run_sweep_rk23(*args, max_attempts=max_attempts, y0=y0, engine_factory=factory, gather=False)   # balance: the default
    out["default_mine"] = assign(len(insts), rank, world, "contiguous")
    return out


@pytest.mark.parametrize("world", [1, 2])
def test_run_sweep_rk23_orders_and_gathers_states_counts_frames_and_roots(oracle, world):
    from rk23_ref import scipy_rk23
    base, insts, y0, dx2 = _setup()
    t1 = M * dx2
    budget = 70
    t_eval = t1 * np.array([0.0, 0.05, 0.2, 0.9])
    ref = [scipy_rk23(oracle, oracle.params_from_dict(base | inst), N, y0[b], (0.0, t1), 0.5 * dx2, RTOL, ATOL, t_eval=t_eval, max_attempts=budget)
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


# ---- integrate_equations(method="RK23") ---------------------------------------------------------------------------------------------
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

    def _native(self, name, y0, t_span):
        from marlpde_amd._abi import MarlStats
        from marlpde_amd.LHeureux_model import RK45Result
        type(self).asked.append(name)
        st = MarlStats()
        st.t, st.nfev = t_span[1], 4
        return RK45Result(st, np.array([t_span[1]]), np.asarray(y0, float)[:, None].copy(), [np.empty(0)] * 7)

    def integrate_rk23(self, y0, t_span, first_step, rtol, atol, t_eval=None):
        return self._native("rk23", y0, t_span)

    def integrate_rk45(self, y0, t_span, first_step, rtol, atol, t_eval=None):
        return self._native("rk45", y0, t_span)

    def fun(self, t, y, *args):
        return -np.asarray(y)

    def __getattr__(self, name):   # the seven monitors
        if name.startswith(("zeros", "ones")):
            return lambda t, y, *args: 1.0
        raise AttributeError(name)

    def close(self):
        pass


def test_integrate_equations_rk23_takes_the_native_branch(monkeypatch):
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

    pde = scenario("A", 16)
    solver = dict(first_step=1e-6, rtol=1e-3, atol=1e-3, t_span=(0.0, 1e-4), backend="hip")
    _FakeModel.asked = []
    monkeypatch.setattr(scipy.integrate, "solve_ivp", forbidden)
    for method in ("RK23", "RK45"):
        last, covered, *_ = es.integrate_equations(solver | {"method": method}, {}, pde, results_root=None, verbose=False)
        assert last.shape == (5, 16) and covered == pde["Tstar"] * 1e-4
    assert _FakeModel.asked == ["rk23", "rk45"]
    monkeypatch.setattr(scipy.integrate, "solve_ivp", noting)
    es.integrate_equations(solver | {"method": "RK23", "scipy_driver": True}, {}, pde, results_root=None, verbose=False)
    assert seen == ["RK23"] and _FakeModel.asked == ["rk23", "rk45"]
