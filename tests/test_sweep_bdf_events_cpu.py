"""run_sweep_bdf(events=True), the parts that need no GPU: `events` / `max_events` reach the engine only when asked for (with and
without `batched` and `t_eval`), the root times come back as the last element of the tuple in the order of `instances` under every
`balance` mode and for world > 1 (gloo), the rest of the tuple is that of the call without events, and the C ABI carries
marl_sweep_bdf_events_dev.  The engine is a double over the CPU oracle (oracle.bdf returns the t_events of a single run), defined
here - what is under test is marlpde_amd/sweep.py."""
import os
import re
from dataclasses import asdict

import numpy as np
import pytest

from marlpde_amd.parameters import Map_Scenario
from marlpde_amd.sweep import assign, initial_states, run_sweep_bdf
from test_sweep_frames_cpu import _spawn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 24
BASE = asdict(Map_Scenario()) | {"N": N}
# oracle roots per monitor over (0, 0.2): [3,3,0,..], none, [8,8,0,..], [6,6,0,..], [3,1,0,0,1,0,1], [7,7,0,..]
INSTANCES = [{"Phi0": 0.6, "PhiIni": 0.5, "PhiNR": 0.6}, {"Phi0": 0.5, "PhiIni": 0.5, "PhiNR": 0.5, "k3": 0.01, "k4": 0.01},
             {"Phi0": 0.65, "PhiIni": 0.5, "PhiNR": 0.5, "k3": 0.05, "k4": 0.05}, {"Phi0": 0.6, "PhiIni": 0.6, "PhiNR": 0.6},
             {"Phi0": 0.8, "PhiIni": 0.8, "PhiNR": 0.8}, {"Phi0": 0.7, "PhiIni": 0.6, "PhiNR": 0.6}]
ARGS = ((0.0, 0.2), 1e-6, 1e-3, 1e-3)
T_EVAL = np.array([0.0, 0.01, 0.1, 0.2])


class OracleBdfEventsEngine:
    """integrate_bdf over oracle.bdf with HipSweepEngine's keywords; `calls` records the keywords every call received."""
    calls = []

    def __init__(self, base_parms, instances):
        from oracle import oracle as orc
        self.orc = orc
        self.N = int(base_parms["N"])
        self.P = [orc.params_from_dict(base_parms | inst) for inst in instances]

    def integrate_bdf(self, y0, t_span, first_step, rtol, atol, max_attempts, **kw):
        from marlpde_amd.LHeureux_model import RK45Result
        type(self).calls.append({k: v for k, v in kw.items() if k != "t_eval"} | ({"t_eval": True} if "t_eval" in kw else {}))
        t_eval, events, max_events = kw.get("t_eval"), kw.get("events", False), kw.get("max_events", 64)
        ys, res = [], []
        for P, y in zip(self.P, y0):
            yf, st, _, ye, tev = self.orc.bdf(P, self.N, y, t_span[0], t_span[1], first_step, rtol, atol, t_eval=t_eval, max_attempts=max_attempts)
            ys.append(yf)
            k = 0 if t_eval is None else int(np.searchsorted(t_eval, st.t, side="right"))
            res.append(RK45Result(st, None if t_eval is None else np.asarray(t_eval)[:k].copy(), None if t_eval is None else ye[:k].T.copy(),
                                  [t[:max_events] for t in tev] if events else None))
        return np.array(ys).reshape(len(self.P), 5 * self.N), res

    def close(self):
        pass


def _reference(oracle):
    y0 = initial_states(BASE, INSTANCES)
    return [oracle.bdf(oracle.params_from_dict(BASE | d), N, y, ARGS[0][0], ARGS[0][1], *ARGS[1:])[4] for d, y in zip(INSTANCES, y0)]


def _same_roots(got, want, cap=None):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert len(g) == 7
        for a, b in zip(g, w):
            assert np.array_equal(np.asarray(a), np.asarray(b)[:cap])


def test_the_instances_have_roots_to_order(oracle):
    ref = _reference(oracle)
    fired = [[len(t) for t in r] for r in ref]
    print(fired)
    assert min(sum(f) for f in fired) == 0 and sum(1 for f in fired if sum(f)) >= 4      # one instance has none
    assert len({tuple(float(x) for t in r for x in t) for r in ref}) == len(ref)          # every instance its own roots: an order shows
    assert any(f[4] or f[6] for f in fired) and any(k > 2 for f in fired for k in f)      # later monitors too; more roots than the cap below


@pytest.mark.parametrize("balance", ["cost", "round_robin", "contiguous"])
def test_roots_keep_the_order_of_instances(oracle, balance):
    E = OracleBdfEventsEngine
    E.calls = []
    plain = run_sweep_bdf(BASE, INSTANCES, *ARGS, balance=balance, engine_factory=E)
    out = run_sweep_bdf(BASE, INSTANCES, *ARGS, balance=balance, events=True, engine_factory=E)
    out_b = run_sweep_bdf(BASE, INSTANCES, *ARGS, balance=balance, events=True, max_events=2, batched=True, engine_factory=E)
    out_f = run_sweep_bdf(BASE, INSTANCES, *ARGS, balance=balance, events=True, t_eval=T_EVAL, batched=True, engine_factory=E)
    frames = run_sweep_bdf(BASE, INSTANCES, *ARGS, balance=balance, t_eval=T_EVAL, engine_factory=E)
    # the keywords reach the engine only when asked for
    assert E.calls == [{}, {"events": True, "max_events": 64}, {"events": True, "max_events": 2, "batched": True},
                       {"t_eval": True, "events": True, "max_events": 64, "batched": True}, {"t_eval": True}]
    ref = _reference(oracle)
    assert len(plain) == 5 and len(out) == len(out_b) == 6 and len(frames) == 7 and len(out_f) == 8   # t_events: the last element
    _same_roots(out[-1], ref)
    _same_roots(out_b[-1], ref, cap=2)
    _same_roots(out_f[-1], ref)
    for with_events, without in ((out, plain), (out_b, plain), (out_f, frames)):
        for a, b in zip(with_events, without):
            assert np.array_equal(a, b, equal_nan=True)


def _worker(rank, world):
    kw = dict(engine_factory=lambda bp, inst: OracleBdfEventsEngine(bp, inst), balance="round_robin")   # the gathered order differs from the arrival order
    return {"events": run_sweep_bdf(BASE, INSTANCES, *ARGS, **kw, events=True, batched=True), "plain": run_sweep_bdf(BASE, INSTANCES, *ARGS, **kw),
            "events_frames": run_sweep_bdf(BASE, INSTANCES, *ARGS, **kw, t_eval=T_EVAL, events=True, max_events=2),
            "frames": run_sweep_bdf(BASE, INSTANCES, *ARGS, **kw, t_eval=T_EVAL), "mine": assign(len(INSTANCES), rank, world, "round_robin")}


def test_roots_are_gathered_in_the_order_of_instances(oracle):
    ref = _reference(oracle)
    out = _spawn(_worker, 2)
    assert out[0]["mine"] == [0, 2, 4] and out[1]["mine"] == [1, 3, 5]
    for r in range(2):
        for with_events, without, cap in ((out[r]["events"], out[r]["plain"], None), (out[r]["events_frames"], out[r]["frames"], 2)):
            assert len(with_events) == len(without) + 1
            for a, b in zip(with_events, without):
                assert np.array_equal(a, b, equal_nan=True)
            _same_roots(with_events[-1], ref, cap=cap)


def test_entry_is_declared_and_bound():
    import ctypes as C
    from marlpde_amd import _abi
    header = open(os.path.join(ROOT, "include", "marl_hip.h")).read()
    m = re.search(r"\bint\s+marl_sweep_bdf_events_dev\s*\(([^)]*)\)\s*;", header)
    assert m, "marl_sweep_bdf_events_dev is not declared in include/marl_hip.h"
    names = [p.strip().split()[-1].lstrip("*") for p in m.group(1).split(",")]
    assert names == ["ctx", "y_dev", "t0", "t1", "first_step", "rtol", "atol", "groups", "max_attempts", "t_eval", "n_eval", "y_eval_dev",
                     "n_done", "t_events", "max_events", "stats"]
    restype, argtypes = _abi.PROTOTYPES["marl_sweep_bdf_events_dev"]
    assert restype is C.c_int and argtypes == _abi.PROTOTYPES["marl_sweep_radau_eval_dev"][1]   # the argument list of the Radau entry
    ev = _abi.PROTOTYPES["marl_sweep_bdf_eval_dev"][1]
    assert argtypes[:13] == ev[:13] and argtypes[15] is ev[13] and len(_abi.PROTOTYPES["marl_sweep_bdf_dev"][1]) == 10   # the others keep theirs
    lib = _abi.load()
    tev = np.zeros(7)
    for t_events, max_events in ((None, 0), (tev.ctypes.data, 1)):   # no context: an error, not a crash - through either path
        assert lib.marl_sweep_bdf_events_dev(None, None, 0.0, 1.0, 0.1, 1e-3, 1e-3, None, 0, None, 0, None, None, t_events, max_events, None) == -1


def test_the_words_no_longer_say_that_the_sweep_has_no_root_times():
    header = open(os.path.join(ROOT, "include", "marl_hip.h")).read()
    assert "It does NOT: locate root times" not in header
    import inspect
    from marlpde_amd import sweep
    from marlpde_amd.LHeureux_model import LMAHeureuxPorosityDiff
    for fn, names in ((sweep.run_sweep_bdf, ("events", "max_events")), (sweep.HipSweepEngine.integrate_bdf, ("events", "max_events")),
                      (LMAHeureuxPorosityDiff.sweep_bdf_device, ("events", "max_events"))):
        sig = inspect.signature(fn)
        assert sig.parameters[names[0]].default is False and sig.parameters[names[1]].default == 64
