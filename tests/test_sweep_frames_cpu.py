"""RK45 sweeps with t_eval, the parts that need no GPU: the C entry is declared and bound, and run_sweep_rk45(t_eval=...) shards,
gathers and orders the time series under gloo like the states.  The arithmetic comes from an oracle-backed engine double defined here
(the product's engine is HipSweepEngine; what is under test is marlpde_amd/sweep.py)."""
import os
import re
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from common import scenario

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_is_declared_and_bound():
    from marlpde_amd import _abi
    header = open(os.path.join(ROOT, "include", "marl_hip.h")).read()
    m = re.search(r"\bint\s+marl_sweep_rk45_eval_dev\s*\(([^)]*)\)\s*;", header)
    assert m, "marl_sweep_rk45_eval_dev is not declared in include/marl_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 13
    assert [p.split()[-1].lstrip("*") for p in params] == ["ctx", "y_dev", "t0", "t1", "first_step", "rtol", "atol", "max_attempts", "t_eval",
                                                            "n_eval", "y_eval_dev", "n_done", "stats"]
    restype, argtypes = _abi.PROTOTYPES["marl_sweep_rk45_eval_dev"]
    assert len(argtypes) == 13 and restype is _abi.PROTOTYPES["marl_sweep_rk45_dev"][0]
    # the plain sweep's arguments, then (t_eval, n_eval, y_eval_dev, n_done) in front of the statistics
    plain = _abi.PROTOTYPES["marl_sweep_rk45_dev"][1]
    assert argtypes[:8] == plain[:8] and argtypes[12] is plain[8]
    lib = _abi.load()
    assert hasattr(lib, "marl_sweep_rk45_eval_dev")
    assert lib.marl_sweep_rk45_eval_dev(None, None, 0.0, 1.0, 0.1, 1e-3, 1e-3, 0, None, 0, None, None, None) == -1   # no context: an error, not a crash


# ---- run_sweep_rk45(t_eval=...) under gloo --------------------------------------------------------------------------------
class OracleFramesEngine:
    """Test double with HipSweepEngine's interface: every instance by the oracle, with t_eval the RK45Result of a single run."""

    def __init__(self, base_parms, instances):
        from oracle import oracle as orc
        self.orc = orc
        self.N = int(base_parms["N"])
        self.P = [orc.params_from_dict(base_parms | inst) for inst in instances]

    def integrate_rk45(self, y0, t_span, first_step, rtol, atol, max_attempts, t_eval=None):
        from marlpde_amd.LHeureux_model import RK45Result
        ys, res = [], []
        for P, y in zip(self.P, y0):
            yf, st, _, ye, _ = self.orc.rk45(P, self.N, y, t_span[0], t_span[1], first_step, rtol, atol, t_eval=t_eval, max_attempts=max_attempts,
                                             max_steps_out=1024)
            ys.append(yf)
            if t_eval is None:
                res.append(RK45Result(st))
            else:
                k = int(np.searchsorted(t_eval, st.t, side="right"))
                res.append(RK45Result(st, np.asarray(t_eval)[:k].copy(), ye[:k].T.copy()))
        return np.array(ys).reshape(len(self.P), 5 * self.N), res

    def close(self):
        pass


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _spawn(fn, world, *args):
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_entry, args=(fn, r, world, port, q, args)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        out = [q.get(timeout=240) for _ in range(world)]      # a crashed rank must fail the test, not hang it
    finally:
        for p in procs:
            p.join(30)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    return dict(out)


def _entry(fn, rank, world, port, q, args):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        q.put((rank, fn(rank, world, *args)))
    finally:
        dist.destroy_process_group()


N = 32
MAX_ATTEMPTS = 25


def _setup():
    from marlpde_amd.sweep import product_grid
    insts = product_grid(Phi0=[0.55, 0.7, 0.8], k3=[0.02, 0.1])
    for d in insts:
        d.update(PhiIni=d["Phi0"], PhiNR=d["Phi0"], k4=d["k3"])
    base = scenario("default", N)
    dx2 = ((base["max_depth"] / base["Xstar"]) / N) ** 2
    return base, insts, dx2


def _frames_worker(rank, world, t_eval):
    from marlpde_amd.sweep import assign, run_sweep_rk45
    base, insts, dx2 = _setup()
    factory = lambda bp, inst: OracleFramesEngine(bp, inst)  # noqa: E731
    # round robin: the gathered order differs from the order the ranks' parts arrive in
    with_frames = run_sweep_rk45(base, insts, (0.0, 1.0), 0.5 * dx2, 1e-3, 1e-3, max_attempts=MAX_ATTEMPTS, engine_factory=factory, balance="round_robin",
                                 t_eval=t_eval)
    plain = run_sweep_rk45(base, insts, (0.0, 1.0), 0.5 * dx2, 1e-3, 1e-3, max_attempts=MAX_ATTEMPTS, engine_factory=factory, balance="round_robin")
    return with_frames, plain, assign(len(insts), rank, world, "round_robin")


@pytest.mark.parametrize("world", [1, 2])
def test_run_sweep_rk45_returns_the_time_series_in_the_order_of_the_instances(oracle, world):
    base, insts, dx2 = _setup()
    ref = []
    for inst in insts:
        p = base | inst
        y0 = np.repeat([p["CAIni"], p["CCIni"], p["cCaIni"], p["cCO3Ini"], p["PhiIni"]], N)
        ref.append(oracle.rk45(oracle.params_from_dict(p), N, y0, 0.0, 1.0, 0.5 * dx2, 1e-3, 1e-3, max_attempts=MAX_ATTEMPTS) + (y0,))
    t_reached = np.array([r[1].t for r in ref])
    assert all(r[1].status == 2 for r in ref) and len(set(t_reached)) == len(insts)
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
        for a, b in zip(plain, with_frames[:5]):
            assert np.array_equal(a, b)
        y, status, acc, rej, t, n_frames, y_eval = with_frames
        assert y_eval.shape == (len(insts), len(t_eval), 5 * N) and n_frames.dtype.kind == "i"
        assert list(n_frames) == list(want) and list(status) == [2] * len(insts) and np.array_equal(t, t_reached)
        for i, inst in enumerate(insts):
            p = base | inst
            yref, st, _, ye, _ = oracle.rk45(oracle.params_from_dict(p), N, ref[i][-1], 0.0, 1.0, 0.5 * dx2, 1e-3, 1e-3, t_eval=t_eval,
                                             max_attempts=MAX_ATTEMPTS)
            k = n_frames[i]
            assert np.array_equal(y[i], yref) and (acc[i], rej[i]) == (st.n_accepted, st.n_rejected)
            assert np.array_equal(y_eval[i, :k], ye[:k]) and np.array_equal(y_eval[i, 0], ref[i][-1])
            assert np.all(np.isnan(y_eval[i, k:]))
