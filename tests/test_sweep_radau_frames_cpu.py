"""Radau sweeps with t_eval and events, the parts that need no GPU: the C entry is declared and bound, and
run_sweep_radau(t_eval=..., events=...) shards, gathers and orders the time series and the root times under gloo like the states.
The arithmetic comes from an oracle-backed engine double defined here (the product's engine is HipSweepEngine; what is under test
is marlpde_amd/sweep.py)."""
import os
import re

import numpy as np
import pytest

from test_sweep_frames_cpu import _setup, _spawn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_is_declared_and_bound():
    from marlpde_amd import _abi
    header = open(os.path.join(ROOT, "include", "marl_hip.h")).read()
    m = re.search(r"\bint\s+marl_sweep_radau_eval_dev\s*\(([^)]*)\)\s*;", header)
    assert m, "marl_sweep_radau_eval_dev is not declared in include/marl_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 16
    assert [p.split()[-1].lstrip("*") for p in params] == ["ctx", "y_dev", "t0", "t1", "first_step", "rtol", "atol", "groups", "max_attempts", "t_eval",
                                                            "n_eval", "y_eval_dev", "n_done", "t_events", "max_events", "stats"]
    restype, argtypes = _abi.PROTOTYPES["marl_sweep_radau_eval_dev"]
    # the events entry's arguments with (t_eval, n_eval, y_eval_dev, n_done) in front of (t_events, max_events, stats)
    ev_restype, ev = _abi.PROTOTYPES["marl_sweep_radau_events_dev"]
    assert restype is ev_restype and len(argtypes) == 16 and argtypes[:9] == ev[:9] and argtypes[13:] == ev[9:]
    assert argtypes[9:13] == list(_abi.PROTOTYPES["marl_sweep_rk45_eval_dev"][1][8:12])
    lib = _abi.load()
    assert hasattr(lib, "marl_sweep_radau_eval_dev")
    tev = np.zeros(7)
    for t_events, max_events in ((None, 0), (tev.ctypes.data, 1)):   # no context: an error, not a crash - through either path
        assert lib.marl_sweep_radau_eval_dev(None, None, 0.0, 1.0, 0.1, 1e-3, 1e-3, None, 0, None, 0, None, None, t_events, max_events, None) == -1


# ---- run_sweep_radau(t_eval=..., events=...) under gloo --------------------------------------------------------------------
class OracleRadauEngine:
    """Test double with HipSweepEngine's interface: every instance by the oracle's Radau, with t_eval / events the RK45Result of a
    single run."""

    def __init__(self, base_parms, instances):
        from oracle import oracle as orc
        self.orc = orc
        self.N = int(base_parms["N"])
        self.P = [orc.params_from_dict(base_parms | inst) for inst in instances]

    def integrate_radau(self, y0, t_span, first_step, rtol, atol, max_attempts, t_eval=None, events=False, max_events=64):
        from marlpde_amd.LHeureux_model import RK45Result
        ys, res = [], []
        for P, y in zip(self.P, y0):
            yf, st, _, ye, tev = self.orc.radau(P, self.N, y, t_span[0], t_span[1], first_step, rtol, atol, t_eval=t_eval, max_attempts=max_attempts,
                                                max_steps_out=1024, max_events=max_events)
            ys.append(yf)
            k = 0 if t_eval is None else int(np.searchsorted(t_eval, st.t, side="right"))
            res.append(RK45Result(st, None if t_eval is None else np.asarray(t_eval)[:k].copy(), None if t_eval is None else ye[:k].T.copy(),
                                  tev if events else None))
        return np.array(ys).reshape(len(self.P), 5 * self.N), res

    def close(self):
        pass


N = 32
H0, RTOL, ATOL = 1e-6, 1e-3, 1e-3
MAX_ATTEMPTS = 12


def _y0(p):
    return np.repeat([p["CAIni"], p["CCIni"], p["cCaIni"], p["cCO3Ini"], p["PhiIni"]], N)


def _frames_worker(rank, world, t_eval):
    from marlpde_amd.sweep import assign, run_sweep_radau
    base, insts, _ = _setup()
    factory = lambda bp, inst: OracleRadauEngine(bp, inst)  # noqa: E731
    # round robin: the gathered order differs from the order the ranks' parts arrive in
    kw = dict(max_attempts=MAX_ATTEMPTS, engine_factory=factory, balance="round_robin")
    with_frames = run_sweep_radau(base, insts, (0.0, 1.0), H0, RTOL, ATOL, t_eval=t_eval, **kw)
    plain = run_sweep_radau(base, insts, (0.0, 1.0), H0, RTOL, ATOL, **kw)
    return with_frames, plain, assign(len(insts), rank, world, "round_robin")


@pytest.mark.parametrize("world", [1, 2])
def test_run_sweep_radau_returns_the_time_series_in_the_order_of_the_instances(oracle, world):
    base, insts, _ = _setup()
    assert int(base["N"]) == N and len(insts) == 6
    ref = []
    for inst in insts:
        p = base | inst
        ref.append(oracle.radau(oracle.params_from_dict(p), N, _y0(p), 0.0, 1.0, H0, RTOL, ATOL, max_attempts=MAX_ATTEMPTS) + (_y0(p),))
    t_reached = np.array([r[1].t for r in ref])
    assert all(r[1].status == 2 and r[1].n_accepted == 12 for r in ref) and len(set(t_reached)) == len(insts)
    assert 1.0e-3 < t_reached.min() and t_reached.max() < 3.2e-3, t_reached      # (1.12e-3 .. 3.09e-3)
    # samples: t0, one inside every run, some that only the runs that got furthest reach, one that none reaches
    ts = np.sort(t_reached)
    t_eval = np.array([0.0, 0.5 * ts[0], 0.5 * (ts[1] + ts[2]), 0.5 * (ts[3] + ts[4]), ts[5], 2.0 * ts[5]])
    assert t_eval[-1] < 1.0 and np.all(np.diff(t_eval) > 0)
    want = np.searchsorted(t_eval, t_reached, side="right")
    assert want.min() == 2 and want.max() == 5 and len(set(want)) >= 3, want
    out = _spawn(_frames_worker, world, t_eval)
    if world == 2:
        assert out[0][2] == [0, 2, 4] and out[1][2] == [1, 3, 5]
    for r in range(world):
        with_frames, plain, _ = out[r]
        assert len(plain) == 5 and len(with_frames) == 7
        for a, b in zip(plain, with_frames[:5]):      # states, status, counts, times: those of the driver without t_eval
            assert np.array_equal(a, b)
        y, status, acc, rej, t, n_frames, y_eval = with_frames
        assert y_eval.shape == (len(insts), len(t_eval), 5 * N) and n_frames.dtype.kind == "i"
        assert list(n_frames) == list(want) and list(status) == [2] * len(insts) and np.array_equal(t, t_reached)
        for i, inst in enumerate(insts):
            p = base | inst
            yref, st, _, ye, _ = oracle.radau(oracle.params_from_dict(p), N, ref[i][-1], 0.0, 1.0, H0, RTOL, ATOL, t_eval=t_eval, max_attempts=MAX_ATTEMPTS)
            k = n_frames[i]
            assert np.array_equal(y[i], yref) and (acc[i], rej[i]) == (st.n_accepted, st.n_rejected)
            assert np.array_equal(y_eval[i, :k], ye[:k]) and np.array_equal(y_eval[i, 0], ref[i][-1])
            assert np.all(np.isnan(y_eval[i, k:]))


# the four instances of tests/test_gpu_radau.py::test_radau_sweep_locates_event_roots_like_the_single_run
EVENT_INSTANCES = [{"Phi0": 0.6, "PhiIni": 0.5, "PhiNR": 0.6}, {"Phi0": 0.5, "PhiIni": 0.5, "PhiNR": 0.5, "k3": 0.01, "k4": 0.01},
                   {"Phi0": 0.6, "PhiIni": 0.6, "PhiNR": 0.6}, {}]
EVENT_ROOT_COUNTS = [[2, 2, 0, 0, 0, 0, 0], [0] * 7, [2, 2, 0, 0, 0, 0, 0], [5, 3, 0, 0, 1, 0, 1]]      # the oracle's, to t = 1


def _event_base():
    from dataclasses import asdict
    from marlpde_amd.parameters import Map_Scenario
    return asdict(Map_Scenario()) | {"N": N}


def _events_worker(rank, world):
    from marlpde_amd.sweep import assign, run_sweep_radau
    factory = lambda bp, inst: OracleRadauEngine(bp, inst)  # noqa: E731
    kw = dict(engine_factory=factory, balance="round_robin")
    args = (_event_base(), EVENT_INSTANCES, (0.0, 1.0), H0, RTOL, ATOL)
    return {"events": run_sweep_radau(*args, events=True, **kw), "plain": run_sweep_radau(*args, **kw),
            "mine": assign(len(EVENT_INSTANCES), rank, world, "round_robin")}


@pytest.mark.parametrize("world", [1, 2])
def test_run_sweep_radau_returns_the_roots_in_the_order_of_the_instances(oracle, world):
    base = _event_base()
    ref = [oracle.radau(oracle.params_from_dict(base | inst), N, _y0(base | inst), 0.0, 1.0, H0, RTOL, ATOL) for inst in EVENT_INSTANCES]
    assert all(r[1].status == 0 for r in ref)
    assert [[len(t) for t in r[4]] for r in ref] == EVENT_ROOT_COUNTS
    out = _spawn(_events_worker, world)
    if world == 2:
        assert out[0]["mine"] == [0, 2] and out[1]["mine"] == [1, 3]
    for r in range(world):
        with_events, without = out[r]["events"], out[r]["plain"]
        assert len(without) == 5 and len(with_events) == 6
        for a, b in zip(with_events, without):
            assert np.array_equal(a, b)
        got = with_events[-1]
        assert len(got) == len(EVENT_INSTANCES)
        for i in range(len(EVENT_INSTANCES)):
            assert len(got[i]) == 7 and all(np.array_equal(a, w) for a, w in zip(got[i], ref[i][4])), i
