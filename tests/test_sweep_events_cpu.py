"""RK45 sweeps with events, the parts that need no GPU: the C entry is declared and bound, and run_sweep_rk45(events=True) shards,
gathers and orders the root times under gloo like the states.  The arithmetic comes from an oracle-backed engine double defined here
(the product's engine is HipSweepEngine; what is under test is marlpde_amd/sweep.py)."""
import os
import re

import numpy as np
import pytest

from common import scenario
from test_sweep_frames_cpu import _spawn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_is_declared_and_bound():
    from marlpde_amd import _abi
    header = open(os.path.join(ROOT, "include", "marl_hip.h")).read()
    m = re.search(r"\bint\s+marl_sweep_rk45_events_dev\s*\(([^)]*)\)\s*;", header)
    assert m, "marl_sweep_rk45_events_dev is not declared in include/marl_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == ["ctx", "y_dev", "t0", "t1", "first_step", "rtol", "atol", "max_attempts", "t_eval",
                                                            "n_eval", "y_eval_dev", "n_done", "t_events", "max_events", "stats"]
    restype, argtypes = _abi.PROTOTYPES["marl_sweep_rk45_events_dev"]
    # the eval entry's arguments, then (t_events, max_events) in front of the statistics
    ev_restype, ev = _abi.PROTOTYPES["marl_sweep_rk45_eval_dev"]
    assert restype is ev_restype and len(argtypes) == 15 and argtypes[:12] == ev[:12] and argtypes[14] is ev[12]
    assert argtypes[12:14] == list(_abi.PROTOTYPES["marl_sweep_radau_events_dev"][1][9:11])
    lib = _abi.load()
    assert hasattr(lib, "marl_sweep_rk45_events_dev")
    tev = np.zeros(7)
    for t_events, max_events in ((None, 0), (tev.ctypes.data, 1)):   # no context: an error, not a crash - through either path
        assert lib.marl_sweep_rk45_events_dev(None, None, 0.0, 1.0, 0.1, 1e-3, 1e-3, 0, None, 0, None, None, t_events, max_events, None) == -1


# ---- run_sweep_rk45(events=True) under gloo -------------------------------------------------------------------------------
N = 64
M = 60                    # t1 = M dx^2
MAX_ATTEMPTS = 40
PHI_DIPS = (0.036, 0.038, 0.04, 0.041, 0.042, 0.044)
RTOL, ATOL = 1e-5, 1e-7


class OracleEventsEngine:
    """Test double with HipSweepEngine's interface: every instance by the oracle, with events the t_events of a single run."""

    def __init__(self, base_parms, instances):
        from oracle import oracle as orc
        self.orc = orc
        self.N = int(base_parms["N"])
        self.P = [orc.params_from_dict(base_parms | inst) for inst in instances]

    def integrate_rk45(self, y0, t_span, first_step, rtol, atol, max_attempts, t_eval=None, events=False, max_events=64):
        from marlpde_amd.LHeureux_model import RK45Result
        ys, res = [], []
        for P, y in zip(self.P, y0):
            yf, st, _, ye, tev = self.orc.rk45(P, self.N, y, t_span[0], t_span[1], first_step, rtol, atol, t_eval=t_eval, max_attempts=max_attempts,
                                               max_steps_out=1024, max_events=max_events)
            ys.append(yf)
            k = 0 if t_eval is None else int(np.searchsorted(t_eval, st.t, side="right"))
            res.append(RK45Result(st, None if t_eval is None else np.asarray(t_eval)[:k].copy(), None if t_eval is None else ye[:k].T.copy(),
                                  tev if events else None))
        return np.array(ys).reshape(len(self.P), 5 * self.N), res

    def close(self):
        pass


def _setup():
    base = scenario("default", N)
    L = base["max_depth"] / base["Xstar"]
    x = (np.arange(N) + 0.5) * (L / N)
    insts = [{"k3": 0.02 + 0.002 * i, "k4": 0.02 + 0.002 * i} for i in range(len(PHI_DIPS))]
    y0 = np.stack([np.repeat([float(base[k]) for k in ("CAIni", "CCIni", "cCaIni", "cCO3Ini", "PhiIni")], N) for _ in PHI_DIPS])
    for b, d in enumerate(PHI_DIPS):   # the phi_dip states of tests/test_gpu_sweep_events.py
        y0[b, 4 * N:] = base["PhiIni"] - d * np.exp(-((x - 0.5 * L) / (0.08 * L)) ** 2)
    return base, insts, y0, (L / N) ** 2


def _events_worker(rank, world, t_eval):
    from marlpde_amd.sweep import assign, run_sweep_rk45
    base, insts, y0, dx2 = _setup()
    factory = lambda bp, inst: OracleEventsEngine(bp, inst)  # noqa: E731
    args = (base, insts, (0.0, M * dx2), 0.5 * dx2, RTOL, ATOL)
    kw = dict(max_attempts=MAX_ATTEMPTS, y0=y0, engine_factory=factory, balance="round_robin")   # the gathered order differs from the arrival order
    return {"events": run_sweep_rk45(*args, **kw, events=True), "plain": run_sweep_rk45(*args, **kw),
            "events_frames": run_sweep_rk45(*args, **kw, t_eval=t_eval, events=True, max_events=8), "frames": run_sweep_rk45(*args, **kw, t_eval=t_eval),
            "mine": assign(len(insts), rank, world, "round_robin")}


@pytest.mark.parametrize("world", [1, 2])
def test_run_sweep_rk45_returns_the_roots_in_the_order_of_the_instances(oracle, world):
    base, insts, y0, dx2 = _setup()
    t1 = M * dx2
    ref = [oracle.rk45(oracle.params_from_dict(base | inst), N, y0[b], 0.0, t1, 0.5 * dx2, RTOL, ATOL, max_attempts=MAX_ATTEMPTS)
           for b, inst in enumerate(insts)]
    fired = [sum(len(t) for t in r[4]) for r in ref]
    roots = [float(t) for r in ref for te in r[4] for t in te]
    assert all(r[1].status == 2 for r in ref), "the attempt budget stops every run"
    assert sum(fired) >= 3 and min(fired) == 0 and len(set(roots)) == len(roots), fired   # some instances fire, one does not, every root its own
    t_eval = t1 * np.array([0.0, 0.05, 0.2, 0.9])
    out = _spawn(_events_worker, world, t_eval)
    if world == 2:
        assert out[0]["mine"] == [0, 2, 4] and out[1]["mine"] == [1, 3, 5]
    for r in range(world):
        for with_events, without in ((out[r]["events"], out[r]["plain"]), (out[r]["events_frames"], out[r]["frames"])):
            assert len(with_events) == len(without) + 1
            for a, b in zip(with_events, without):
                assert np.array_equal(a, b, equal_nan=True)
            got = with_events[-1]
            assert len(got) == len(insts)
            for i in range(len(insts)):
                assert len(got[i]) == 7 and all(np.array_equal(a, w) for a, w in zip(got[i], ref[i][4])), i
