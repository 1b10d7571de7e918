"""run_sweep_bdf(t_eval=...), the parts that need no GPU: the keyword reaches the engine only when asked for (with and without
`batched`), states and time series come back in the order of `instances` whatever the assignment, rows beyond an instance's n_frames
are NaN, and the C ABI carries marl_sweep_bdf_eval_dev.  The engine is a double over the CPU oracle (oracle.bdf(..., t_eval=)) at the
instances and arguments of tests/test_sweep_bdf_cpu.py - what is under test is marlpde_amd/sweep.py."""
import os
import re

import numpy as np

from marlpde_amd.sweep import initial_states, run_sweep_bdf
from test_sweep_bdf_cpu import ARGS, BASE, INSTANCES, N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_EVAL = np.concatenate([[0.0], np.geomspace(1e-6, 1e-3, 7), np.linspace(2e-3, ARGS[0][1], 9)])


class OracleBdfFramesEngine:
    """integrate_bdf over oracle.bdf with HipSweepEngine's keywords; `calls` records the keywords every call received."""
    calls = []

    def __init__(self, base_parms, instances):
        from oracle import oracle as orc
        self.orc = orc
        self.N = int(base_parms["N"])
        self.P = [orc.params_from_dict(base_parms | inst) for inst in instances]

    def integrate_bdf(self, y0, t_span, first_step, rtol, atol, max_attempts, **kw):
        from marlpde_amd.LHeureux_model import RK45Result
        type(self).calls.append({k: (v if k != "t_eval" else np.array(v)) for k, v in kw.items()})
        t_eval = kw.get("t_eval")
        ys, res = [], []
        for P, y in zip(self.P, y0):
            yf, st, _, ye, _ = self.orc.bdf(P, self.N, y, t_span[0], t_span[1], first_step, rtol, atol, t_eval=t_eval, max_attempts=max_attempts)
            ys.append(yf)
            if t_eval is None:
                res.append(RK45Result(st))
            else:
                k = int(np.searchsorted(t_eval, st.t, side="right"))
                res.append(RK45Result(st, np.asarray(t_eval)[:k].copy(), ye[:k].T.copy()))
        return np.array(ys).reshape(len(self.P), 5 * self.N), res

    def close(self):
        pass


def _singles(oracle, max_attempts=0):
    y0 = initial_states(BASE, INSTANCES)
    return [oracle.bdf(oracle.params_from_dict(BASE | d), N, y, ARGS[0][0], ARGS[0][1], *ARGS[1:], t_eval=T_EVAL, max_attempts=max_attempts)
            for d, y in zip(INSTANCES, y0)]


def test_t_eval_arrives_only_when_asked_for(oracle):
    E = OracleBdfFramesEngine
    E.calls = []
    plain = run_sweep_bdf(BASE, INSTANCES, *ARGS, engine_factory=E)
    plain_b = run_sweep_bdf(BASE, INSTANCES, *ARGS, batched=True, engine_factory=E)
    sampled = run_sweep_bdf(BASE, INSTANCES, *ARGS, t_eval=T_EVAL, engine_factory=E)
    sampled_b = run_sweep_bdf(BASE, INSTANCES, *ARGS, t_eval=list(T_EVAL), batched=True, engine_factory=E)
    assert [sorted(c) for c in E.calls] == [[], ["batched"], ["t_eval"], ["batched", "t_eval"]]
    assert E.calls[1] == {"batched": True} and E.calls[3]["batched"] is True
    for c in E.calls[2:]:
        assert c["t_eval"].dtype == np.float64 and np.array_equal(c["t_eval"], T_EVAL)
    assert len(plain) == len(plain_b) == 5 and len(sampled) == len(sampled_b) == 7
    for a, b in zip(plain, sampled[:5]):   # the samples change nothing else
        assert np.array_equal(a, b)
    for a, b in zip(sampled, sampled_b):
        assert np.array_equal(a, b, equal_nan=True)


def test_frames_keep_the_order_of_instances_under_cost_balance(oracle):
    y, status, acc, rej, t, n_frames, y_eval = run_sweep_bdf(BASE, INSTANCES, *ARGS, t_eval=T_EVAL, batched=True, balance="cost",
                                                             engine_factory=OracleBdfFramesEngine)
    ref = _singles(oracle)
    assert len({r[1].n_accepted for r in ref}) > 1, "the instances must differ, or their order would not show"
    assert y_eval.shape == (len(INSTANCES), T_EVAL.size, 5 * N) and n_frames.dtype.kind == "i"
    assert list(n_frames) == [T_EVAL.size] * len(INSTANCES) and np.all(t == ARGS[0][1]) and list(status) == [0] * len(INSTANCES)
    y0 = initial_states(BASE, INSTANCES)
    for b, (yf, st, _, ye, _) in enumerate(ref):
        assert np.array_equal(y[b], yf) and (acc[b], rej[b]) == (st.n_accepted, st.n_rejected)
        assert np.array_equal(y_eval[b], ye)
        np.testing.assert_allclose(y_eval[b, 0], y0[b], rtol=1e-12, atol=0)   # (the first step's dense output at t0, not a copy of y0)
    assert not any(np.array_equal(y_eval[0], y_eval[b]) for b in range(1, len(INSTANCES)))


def test_rows_beyond_n_frames_are_nan_for_a_budget_limited_instance(oracle):
    budget = 14
    y, status, acc, rej, t, n_frames, y_eval = run_sweep_bdf(BASE, INSTANCES, *ARGS, max_attempts=budget, t_eval=T_EVAL,
                                                             engine_factory=OracleBdfFramesEngine)
    ref = _singles(oracle, max_attempts=budget)
    assert list(status) == [2] * len(INSTANCES) and np.all(t < ARGS[0][1])
    want = np.searchsorted(T_EVAL, t, side="right")
    assert list(n_frames) == list(want) and 0 < want.min() and want.max() < T_EVAL.size
    for b, (yf, st, _, ye, _) in enumerate(ref):
        k = n_frames[b]
        assert t[b] == st.t and np.array_equal(y_eval[b, :k], ye[:k]) and np.all(np.isnan(y_eval[b, k:]))


def test_abi_has_the_bdf_sweep_with_frames():
    import ctypes as C
    from marlpde_amd import _abi
    res, args = _abi.PROTOTYPES["marl_sweep_bdf_eval_dev"]
    assert res is C.c_int and len(args) == 14
    assert len(_abi.PROTOTYPES["marl_sweep_bdf_dev"][1]) == 10
    # the Radau entry's arguments without the t_events / max_events pair
    radau = _abi.PROTOTYPES["marl_sweep_radau_eval_dev"][1]
    assert args == radau[:13] + radau[15:]
    header = open(os.path.join(ROOT, "include", "marl_hip.h")).read()
    m = re.search(r"\bint\s+marl_sweep_bdf_eval_dev\s*\(([^)]*)\)\s*;", header)
    assert m, "marl_sweep_bdf_eval_dev is not declared in include/marl_hip.h"
    assert [p.split()[-1].lstrip("*") for p in m.group(1).split(",")] == ["ctx", "y_dev", "t0", "t1", "first_step", "rtol", "atol", "groups", "max_attempts",
                                                                          "t_eval", "n_eval", "y_eval_dev", "n_done", "stats"]
    lib = _abi.load()
    assert lib.marl_sweep_bdf_eval_dev(None, None, 0.0, 1.0, 0.1, 1e-3, 1e-3, None, 0, None, 0, None, None, None) == -1   # an error, not a crash
