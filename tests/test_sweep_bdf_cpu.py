"""run_sweep_bdf(..., batched=): the keyword reaches the engine only when asked for, results come back in the order of `instances`
whatever the assignment, and the C ABI carries the batched entry.  The engine is a double over the CPU oracle (oracle.bdf), defined
here - no GPU."""
from dataclasses import asdict

import numpy as np

from marlpde_amd.parameters import Map_Scenario
from marlpde_amd.sweep import initial_states, run_sweep_bdf

N = 24
BASE = asdict(Map_Scenario()) | {"N": N}
# heavy end first in the cost proxy's eyes (Phi0 0.8), so that balance="cost" visits the instances in another order than given
INSTANCES = [{"Phi0": 0.6, "PhiIni": 0.5, "PhiNR": 0.6}, {"Phi0": 0.8, "PhiIni": 0.8, "PhiNR": 0.8},
             {"Phi0": 0.5, "PhiIni": 0.5, "PhiNR": 0.5, "k3": 0.01, "k4": 0.01}, {"Phi0": 0.75, "PhiIni": 0.6, "PhiNR": 0.6}]
ARGS = ((0.0, 0.01), 1e-6, 1e-3, 1e-3)


class OracleBdfEngine:
    """integrate_bdf over oracle.bdf; `calls` records the keywords every call received."""
    calls = []

    def __init__(self, base_parms, instances):
        from oracle import oracle as orc
        self.orc = orc
        self.N = int(base_parms["N"])
        self.P = [orc.params_from_dict(base_parms | inst) for inst in instances]

    def integrate_bdf(self, y0, t_span, first_step, rtol, atol, max_attempts, **kw):
        from marlpde_amd.LHeureux_model import RK45Result
        type(self).calls.append(dict(kw))
        ys, res = [], []
        for P, y in zip(self.P, y0):
            yf, st, *_ = self.orc.bdf(P, self.N, y, t_span[0], t_span[1], first_step, rtol, atol, max_attempts=max_attempts)
            ys.append(yf)
            res.append(RK45Result(st))
        return np.array(ys).reshape(len(self.P), 5 * self.N), res

    def close(self):
        pass


def _singles(oracle):
    y0 = initial_states(BASE, INSTANCES)
    out = []
    for d, y in zip(INSTANCES, y0):
        yf, st, *_ = oracle.bdf(oracle.params_from_dict(BASE | d), N, y, ARGS[0][0], ARGS[0][1], *ARGS[1:])
        out.append((yf, st.n_accepted, st.n_rejected, st.status))
    return out


def test_batched_keyword_arrives_and_results_keep_the_order_of_instances(oracle):
    OracleBdfEngine.calls = []
    y, status, acc, rej, t = run_sweep_bdf(BASE, INSTANCES, *ARGS, batched=True, balance="cost", engine_factory=OracleBdfEngine)
    assert OracleBdfEngine.calls == [{"batched": True}]
    ref = _singles(oracle)
    assert len({r[1] for r in ref}) > 1, "the instances must differ, or their order would not show"
    for b, (yf, n_acc, n_rej, st) in enumerate(ref):
        assert np.array_equal(y[b], yf) and (acc[b], rej[b], status[b]) == (n_acc, n_rej, st)
    assert np.all(t == ARGS[0][1])


def test_without_batched_the_engine_is_called_without_the_keyword(oracle):
    OracleBdfEngine.calls = []
    y, *_ = run_sweep_bdf(BASE, INSTANCES, *ARGS, engine_factory=OracleBdfEngine)
    y2, *_ = run_sweep_bdf(BASE, INSTANCES, *ARGS, batched=False, engine_factory=OracleBdfEngine)
    assert OracleBdfEngine.calls == [{}, {}]
    assert np.array_equal(y, y2)


def test_abi_has_the_batched_bdf_sweep():
    import ctypes as C
    from marlpde_amd import _abi
    res, args = _abi.PROTOTYPES["marl_sweep_bdf_dev"]
    assert res is C.c_int and len(args) == 10
    assert args == _abi.PROTOTYPES["marl_sweep_radau_dev"][1]
