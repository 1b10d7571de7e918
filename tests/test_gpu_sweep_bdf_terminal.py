"""BDF sweeps that honour terminal monitors (marl_sweep_bdf_terminal_dev): the reference's `terminal` switch
(marlpde/LHeureux_model.py:113-122) ends an instance of the batched BDF sweep at a monitor's root on the device, as solve_ivp does
(ivp.py:79-130, 681-723) - BdfTerm / A_TERM_ROOTS / A_STOP in csrc/marl_bdf_ctl.h, roots_batch_kernel<true> and
stop_state_batch_kernel in csrc/marl_bdf_batch.h.  The yardstick is the same sweep without limits (marl_sweep_bdf_events_dev): up to
the step that ends it a limited run IS that run, so roots, frames and counts are compared bit for bit, and the expectations of the
rule are derived from the unlimited sweep's own root lists (keep r < t_stop; equal roots up to the terminal monitor's index).  Only
the comparison with the single run carries a tolerance, the project's 5e-4 between controllers (tests/test_gpu_terminal.py).
N = 64, the five instances of tests/test_gpu_sweep_radau_frames.py (the last is the default scenario), t_span (0, 0.3), first step
1e-6, rtol = atol = 1e-3, max_events 64.
The last test launches stop_state_batch_kernel once through marl_debug_bdf_batch (op STOP), as tests/test_gpu_bdf_batch_parts.py
launches the other vector kernels."""
import ctypes as C
import json

import numpy as np
import pytest

import bdf_batch_ref as R
from common import BDF_BATCH_ROOTS
from test_gpu_sweep_radau_frames import ATOL, H0, INSTANCES, RTOL, _base, _key, _model, _same_roots, _y0
from test_gpu_terminal import MESSAGE, NAMES, ONES_PHI, SENTINEL, ZEROS_W, _expected_roots

pytestmark = pytest.mark.gpu

N, T1, MAX_EVENTS = 64, 0.3, 64
T_EVAL = np.linspace(0.0, T1, 11)
RULE = ((0, 3), (1, 3), (ZEROS_W, 6), (ZEROS_W, 2))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def setup():
    base = _base(N)
    return base, _y0(base, INSTANCES)


def _run(torch, setup, terminal=None, t_eval=None, fill=np.nan, events=True, max_events=MAX_EVENTS, max_attempts=0):
    """One batched BDF sweep of the five instances through the model's entry -> (states, results, frames or None)."""
    base, y0 = setup
    eq = _model(torch, base, INSTANCES)
    try:
        eq.set_terminal(terminal)
        yd = torch.from_numpy(y0).cuda()
        more = {"events": True, "max_events": max_events} if events else {}
        if t_eval is None:
            res = eq.sweep_bdf_device(yd.data_ptr(), (0.0, T1), H0, RTOL, ATOL, max_attempts, **more)
            return yd.cpu().numpy(), res, None
        frames = torch.full((y0.shape[0], len(t_eval), y0.shape[1]), fill, dtype=yd.dtype, device=yd.device)
        res = eq.sweep_bdf_device(yd.data_ptr(), (0.0, T1), H0, RTOL, ATOL, max_attempts, t_eval=t_eval, y_eval_dev_ptr=frames.data_ptr(), **more)
        return yd.cpu().numpy(), res, frames.cpu().numpy()
    finally:
        eq.close()


@pytest.fixture(scope="module")
def unlimited(torch_cuda, setup):
    """The yardstick: the sweep without limits, roots located and the frames at T_EVAL - computed once."""
    return _run(torch_cuda, setup, t_eval=T_EVAL)


# 1 ---------------------------------------------------------------------------------------------------------------------------------
def test_stops_the_one_instance_only(torch_cuda, setup, unlimited):
    yu, ru, fu = unlimited
    print("roots of the unlimited sweep per instance:", [[len(t) for t in r.t_events] for r in ru])
    assert ru[4].status == 0 and len(ru[4].t_events[ONES_PHI]) >= 1 and not any(ru[1].n_events)
    yl, rl, fl = _run(torch_cuda, setup, {"ones_Phi": 1}, t_eval=T_EVAL)
    t_stop = ru[4].t_events[ONES_PHI][0]
    print("t_stop", t_stop, "status", [r.status for r in rl], "roots of instance 4", [len(t) for t in rl[4].t_events])
    assert rl[4].status == 1 and rl[4].t_reached == t_stop
    assert [len(t) for t in rl[4].t_events] == [0, 0, 0, 0, 1, 0, 0] and rl[4].t_events[ONES_PHI][0] == t_stop
    assert list(rl[4].n_events) == [0, 0, 0, 0, 1, 0, 0]
    for b in range(4):      # the other instances: bit for bit the sweep without the limit
        assert np.array_equal(yl[b], yu[b]) and _key(rl[b]) == _key(ru[b]) and _same_roots(rl[b], ru[b]), b
        assert np.array_equal(rl[b].event_values, ru[b].event_values) and rl[b].h_next == ru[b].h_next
        assert np.array_equal(rl[b].t, ru[b].t) and np.array_equal(fl[b], fu[b]), b


# 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rule_runs(torch_cuda, setup):
    return {(e, k): _run(torch_cuda, setup, {NAMES[e]: k})[1] for e, k in RULE}


@pytest.mark.parametrize("e, k", RULE)
def test_the_rule_on_the_device(unlimited, rule_runs, e, k):
    ru, rl = unlimited[1][4], rule_runs[(e, k)][4]
    assert len(ru.t_events[e]) >= k
    t_stop, want = _expected_roots(ru.t_events, e, k)
    got = [len(t) for t in rl.t_events]
    print(NAMES[e], k, "t_stop", t_stop, "roots of monitors 0 / 1 / 6:", got[0], got[1], got[6])
    if (e, k) == (ZEROS_W, 6):   # did the third roots of zeros and zeros_CA and the sixth of zeros_W share a step?  Then the three limits end in the same attempt
        att = [rule_runs[key][4] for key in RULE[:3]]
        print("the three roots shared a step on the device:", len({r.n_accepted + r.n_rejected for r in att}) == 1)
    assert rl.status == 1 and rl.t_reached == t_stop
    for m in range(7):
        assert np.array_equal(rl.t_events[m], want[m]), (e, k, m, rl.t_events[m], want[m])
        assert rl.n_events[m] == len(rl.t_events[m])


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_frames_and_final_state(torch_cuda, setup, unlimited):
    r = unlimited[1][4].t_events[ONES_PHI][0]
    t_eval = np.array([0.0, 0.5 * r, r, np.nextafter(r, np.inf), T1])
    _, _, fu = _run(torch_cuda, setup, t_eval=t_eval)
    yl, rl, fl = _run(torch_cuda, setup, {"ones_Phi": 1}, t_eval=t_eval, fill=SENTINEL)
    assert rl[4].status == 1 and len(rl[4].t) == 3                      # n_done == 3
    assert np.array_equal(fl[4, :3], fu[4, :3]) and np.all(fl[4, :3] != SENTINEL)
    assert np.all(fl[4, 3:] == SENTINEL)
    assert np.array_equal(yl[4], fl[4, 2])                              # the state returned is the frame at t_stop, bit for bit
    print("ones_Phi of the state returned", rl[4].event_values[ONES_PHI])
    assert abs(rl[4].event_values[ONES_PHI]) <= 1e-9                    # the bound of tests/test_gpu_terminal.py
    for b in range(4):
        assert len(rl[b].t) == 5 and np.array_equal(fl[b], fu[b])


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_counts_are_those_after_the_accepted_step(torch_cuda, setup):
    rl = _run(torch_cuda, setup, {"ones_Phi": 1})[1][4]
    A = rl.n_accepted + rl.n_rejected
    same = _run(torch_cuda, setup, max_attempts=A)[1][4]
    short = _run(torch_cuda, setup, max_attempts=A - 1)[1][4]
    print("attempts", A, "t_stop", rl.t_reached, "the sweep without limits after A / A - 1 attempts:", same.t_reached, short.t_reached)
    assert (same.nfev, same.njev, same.nlu, same.n_accepted, same.n_rejected) == (rl.nfev, rl.njev, rl.nlu, rl.n_accepted, rl.n_rejected)
    assert same.t_reached >= rl.t_reached > short.t_reached


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_no_slot_and_no_buffer(torch_cuda, setup, rule_runs):
    full = rule_runs[(ZEROS_W, 2)][4]
    one = _run(torch_cuda, setup, {"zeros_W": 2}, max_events=1)[1][4]
    assert one.status == 1 and one.t_reached == full.t_reached and len(one.t_events[ZEROS_W]) == 1 and one.n_events[ZEROS_W] == 2
    assert one.t_events[ZEROS_W][0] == full.t_events[ZEROS_W][0] and list(one.n_events) == list(full.n_events)
    plain = _run(torch_cuda, setup, {"zeros_W": 2}, events=False)[1][4]      # no t_events at all
    assert plain.status == 1 and plain.t_reached == full.t_reached and plain.t_events is None and list(plain.n_events) == list(full.n_events)


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_sweeps_instance_against_the_single_run(torch_cuda, setup, oracle):
    from marlpde_amd.LHeureux_model import LMAHeureuxPorosityDiff
    base, y0 = setup
    rl = _run(torch_cuda, setup, {"ones_Phi": 1})[1][4]
    eq = LMAHeureuxPorosityDiff.from_scenario(base | INSTANCES[4], device=0)
    try:
        eq.set_terminal({"ones_Phi": 1})
        one = eq.integrate_bdf(y0[4], (0.0, T1), H0, RTOL, ATOL, groups=oracle.scipy_groups(N))
    finally:
        eq.close()
    print("sweep", rl.t_reached, "single run", one.t_reached, "difference", abs(rl.t_reached - one.t_reached))
    assert rl.status == one.status == 1 and abs(rl.t_reached - one.t_reached) <= 5e-4
    assert [len(t) for t in rl.t_events] == [len(t) for t in one.t_events]


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def _raw(torch, eq, name, y0, t_eval=None, max_events=0, budget=0):
    """entry `name` called as the C ABI has it -> (rc, states, stats, n_done, frames, t_events)"""
    from marlpde_amd._abi import MarlStats
    B = y0.shape[0]
    yd = torch.from_numpy(y0).cuda()
    stats = (MarlStats * B)()
    args = [eq._ctx, C.c_void_p(yd.data_ptr()), 0.0, T1, H0, RTOL, ATOL, None, budget]
    n_done, frames, tev = np.zeros(B, dtype=np.int64), None, None
    if name != "marl_sweep_bdf_dev":
        te = np.ascontiguousarray([] if t_eval is None else t_eval, dtype=np.float64)
        frames = torch.full((B, max(te.size, 1), y0.shape[1]), SENTINEL, dtype=yd.dtype, device=yd.device)
        args += [te.ctypes.data_as(C.c_void_p) if te.size else None, te.size, C.c_void_p(frames.data_ptr()) if te.size else None, n_done.ctypes.data_as(C.c_void_p)]
        if name != "marl_sweep_bdf_eval_dev":
            tev = np.full((B, 7, max(max_events, 1)), np.nan)
            args += [tev.ctypes.data_as(C.c_void_p) if max_events > 0 else None, max_events]
    rc = getattr(eq._lib, name)(*args, stats)
    return rc, yd.cpu().numpy(), stats, n_done, None if frames is None else frames.cpu().numpy(), tev


def test_without_limits_the_new_entry_is_the_events_entry(torch_cuda, setup):
    base, y0 = setup
    eq = _model(torch_cuda, base, INSTANCES)
    try:
        for kw in (dict(t_eval=T_EVAL, max_events=MAX_EVENTS), dict(max_events=MAX_EVENTS), dict(t_eval=T_EVAL), dict()):
            a = _raw(torch_cuda, eq, "marl_sweep_bdf_events_dev", y0, **kw)
            b = _raw(torch_cuda, eq, "marl_sweep_bdf_terminal_dev", y0, **kw)
            assert a[0] == b[0] == 0
            assert np.array_equal(a[1], b[1]) and bytes(a[2]) == bytes(b[2]) and np.array_equal(a[3], b[3])
            assert np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5], equal_nan=True)
    finally:
        eq.close()


def test_the_old_entries_still_refuse_a_limit(torch_cuda, setup):
    base, y0 = setup
    eq = _model(torch_cuda, base, INSTANCES)
    try:
        eq.set_terminal({"ones_Phi": 1})
        for name in ("marl_sweep_bdf_dev", "marl_sweep_bdf_eval_dev", "marl_sweep_bdf_events_dev"):
            rc, y, *_ = _raw(torch_cuda, eq, name, y0, t_eval=T_EVAL, max_events=MAX_EVENTS, budget=30)
            assert rc < 0 and MESSAGE in eq._lib.marl_last_error(eq._ctx)
            assert np.array_equal(y, y0)                                         # the state is untouched
        rc, y, stats, *_ = _raw(torch_cuda, eq, "marl_sweep_bdf_terminal_dev", y0, t_eval=T_EVAL, max_events=MAX_EVENTS)
        assert rc == 0 and [s.status for s in stats] == [0, 0, 0, 0, 1]
    finally:
        eq.close()


# 8 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batched", (True, False))
def test_drivers(setup, unlimited, batched):
    from marlpde_amd.sweep import run_sweep_bdf
    base, y0 = setup
    more = dict(y0=y0, device=0, batched=batched)
    y, status, acc, rej, t = run_sweep_bdf(base, INSTANCES, (0.0, T1), H0, RTOL, ATOL, terminal={"ones_Phi": True}, **more)
    free = run_sweep_bdf(base, INSTANCES, (0.0, T1), H0, RTOL, ATOL, events=True, **more)    # a limit does not outlive the call that set it
    t_stop = free[-1][4][ONES_PHI][0]
    print("batched", batched, "status", list(status), "t", list(t), "the unlimited run's first ones_Phi root", t_stop)
    assert list(status) == [0, 0, 0, 0, 1] and t[4] == t_stop and list(t[:4]) == [T1] * 4
    assert list(free[1]) == [0] * 5 and list(free[4]) == [T1] * 5
    assert np.array_equal(y[:4], free[0][:4]) and not np.array_equal(y[4], free[0][4])
    if batched:
        assert np.array_equal(free[0], unlimited[0]) and t_stop == unlimited[1][4].t_events[ONES_PHI][0]


# 9 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N_", (33, 64))
def test_one_launch_of_the_stop_kernel(oracle, N_):
    """stop_state_batch_kernel alone (marl_debug_bdf_batch, op STOP) on the steps of the one-launch ROOTS test (bdf_batch_ref.make_root_D,
    ROOT_STEPS; t_stop at 0.4 of the step), lists None / (1,) / (2, 0), orders 1 .. 5: y of a listed instance is the dense state at t_stop within SAMPLE's bound, (order + 2) eps sum |terms| against the sum in
    extended precision; its monitors are the oracle's of that very state within BDF_BATCH_ROOTS["bound"] relative to max(1, |monitor|)
    (the one-launch ROOTS test's tolerance: the kernel's table-driven exp in F(Phi) is a few ulp off libm); D, the state of every
    instance not listed, the other monitors' slots and every other buffer come back with the bits they went in with."""
    from marlpde_amd.LHeureux_model import LMAHeureuxPorosityDiff
    n = 5 * N_
    t_old, t = [s[0] for s in R.ROOT_STEPS], [s[1] for s in R.ROOT_STEPS]
    h = [b_ - a_ for a_, b_ in R.ROOT_STEPS]
    t_stop = [a_ + 0.4 * (b_ - a_) for a_, b_ in R.ROOT_STEPS]
    assert all(a_ < s_ < b_ for a_, s_, b_ in zip(t_old, t_stop, t))
    eq = LMAHeureuxPorosityDiff.from_scenario(R.base_params(N_), device=0, instances=R.INSTANCES)
    worst_y, worst_g = 0.0, 0.0
    try:
        for lst in R.LISTS:
            for orders in R.ORDER_SETS:
                D = R.make_root_D(N_, orders)
                for b in range(R.B):
                    D[b, orders[b] + 1:] = R.sentinel((R.ROWS - orders[b] - 1, n), 2 + b)
                y0 = R.sentinel((R.B, n), 7)
                tev0, ss0, fr0 = R.sentinel((R.B, 7, R.MAX_EVENTS), 12), R.sentinel((R.B, 2), 13), R.sentinel((R.B, 2, n), 11)
                got = eq.debug_bdf_batch("STOP", D, y=y0, instances=lst, order=orders, t=t, h=h, t_old=t_stop, t_events=tev0, ss=ss0,
                                         t_eval=[0.1, 0.2], frames=fr0)
                assert R.same_bits(got["D"], D) and R.same_bits(got["ss"], ss0) and R.same_bits(got["frames"], fr0)
                want_y, want_tev = y0.copy(), tev0.copy()
                for b in (range(R.B) if lst is None else lst):
                    ref, bound = R.sample_ref(D[b], orders[b], t[b], h[b], t_stop[b])
                    worst_y = max(worst_y, R.worst_ratio(got["y"][b], ref, bound))
                    want_y[b] = got["y"][b]
                    P = oracle.params_from_dict(R.base_params(N_) | R.INSTANCES[b])
                    g_ref = np.asarray(oracle.events(P, N_, got["y"][b]))
                    g = got["t_events"][b, :, 0]
                    worst_g = max(worst_g, float(np.max(np.abs(g - g_ref) / np.maximum(1.0, np.abs(g_ref)))))
                    want_tev[b, :, 0] = g
                assert R.same_bits(got["y"], want_y), "the state of an instance that was not listed was written"
                assert R.same_bits(got["t_events"], want_tev)
    finally:
        eq.close()
    print("BDF_BATCH_STOP", json.dumps({"N": N_, "y_worst_over_bound": worst_y, "monitors_worst": worst_g, "monitors_bound": BDF_BATCH_ROOTS["bound"]}))
    assert worst_y <= 1 and worst_g <= BDF_BATCH_ROOTS["bound"]


def test_the_hook_refuses_a_stop_without_a_slot():
    from marlpde_amd._abi import MarlError
    from marlpde_amd.LHeureux_model import LMAHeureuxPorosityDiff
    eq = LMAHeureuxPorosityDiff.from_scenario(R.base_params(33), device=0, instances=R.INSTANCES)
    try:
        D = R.make_D(33, 0)
        tev = R.sentinel((R.B, 7, R.MAX_EVENTS), 12)
        for kw, word in ((dict(order=2), "max_events"), (dict(order=(1, 6, 3), t_events=tev), "order"), (dict(order=2, instances=[3], t_events=tev), "list entry")):
            with pytest.raises(MarlError, match=word):
                eq.debug_bdf_batch("STOP", D, t=0.75, h=0.25, t_old=0.7, **kw)
    finally:
        eq.close()
