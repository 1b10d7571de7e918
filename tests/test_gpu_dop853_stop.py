"""Terminal monitors in the native DOP853 loop (marl_set_terminal): sweeps that end an instance at a monitor's root inside the sweep
kernel (dop853_sweep_stop_kernel behind marl_sweep_dop853_stop_dev) and the single run that is that sweep for one instance
(marl_integrate_dop853_stop), as solve_ivp does (ivp.py:79-130, 681-723).  The file mirrors tests/test_gpu_rk_terminal.py.

The yardstick is the same path's run without limits, through sweep_dop853_device with events=True: up to the step that ends it a limited
run IS that run, so roots, frames, counts and states are compared bit for bit; only the comparison with scipy carries a tolerance, the
project's root bound.  N = 64, the five instances of tests/test_gpu_sweep_radau_frames.py (the last is the default scenario), t_span
(0, 0.03), first step 1e-6, rtol 1e-5, atol 1e-7 (at 1e-3 scipy's DOP853 ends a quarter of the attempts of instances 0 and 3 in a NaN
norm), max_events 64.  scipy's DOP853 on the oracle with these inputs: instances 0 - 3 without a sign change, instance 4 with one ones_Phi
root at 0.013516647... and seven zeros_W roots (0.01390... to 0.02856...), each in a step of its own, 981 accepted and 22 rejected
attempts, no error norm within 1.2e-3 of 1; with ones_Phi: 1 it stops with nfev 4711."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_sweep_radau_frames import H0, INSTANCES, _base, _key, _model, _same_roots, _y0
from test_gpu_terminal import _expected_roots

pytestmark = pytest.mark.gpu

N, T1, MAX_EVENTS = 64, 0.03, 64
RTOL, ATOL = 1e-5, 1e-7
T_EVAL = np.linspace(0.0, T1, 11)
ONES_PHI, ZEROS_W = 4, 6
SENTINEL = -7.25
NAMES = ("zeros", "zeros_CA", "zeros_CC", "ones_CA_plus_CC", "ones_Phi", "zeros_U", "zeros_W")
ROOT_RTOL, ROOT_ATOL_T1 = 1e-9, 1e-12      # root times against scipy, decision for decision (tests/test_gpu_sweep_events.py)
NFEV_ATTEMPT, NFEV_DENSE = 12, 3


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def setup():
    base = _base(N)
    return base, _y0(base, INSTANCES)


def _sweep(torch, eq, y0, t_eval=None, fill=np.nan, stop=True, **kw):
    """stop: through sweep_dop853_stop_device (the stop entry while a limit is set), else through sweep_dop853_device"""
    yd = torch.from_numpy(y0).cuda()
    sweep = eq.sweep_dop853_stop_device if stop else eq.sweep_dop853_device
    if t_eval is None:
        res = sweep(yd.data_ptr(), (0.0, T1), H0, RTOL, ATOL, **kw)
        return yd.cpu().numpy(), res, None
    frames = torch.full((y0.shape[0], len(t_eval), y0.shape[1]), fill, dtype=yd.dtype, device=yd.device)
    res = sweep(yd.data_ptr(), (0.0, T1), H0, RTOL, ATOL, t_eval=t_eval, y_eval_dev_ptr=frames.data_ptr(), **kw)
    return yd.cpu().numpy(), res, frames.cpu().numpy()


def _run(torch, setup, terminal=None, t_eval=None, fill=np.nan, events=True, max_events=MAX_EVENTS, max_attempts=0, variant=None, base_more=None):
    """One sweep of the five instances -> (states, results, frames); variant: the sweep_variant option (0 / 2: 256 / 1024 threads).
    Without `terminal` the sweep goes through sweep_dop853_device: the three older entries."""
    base, y0 = setup
    eq = _model(torch, base | (base_more or {}), INSTANCES)
    try:
        if variant is not None:
            eq.set_option("sweep_variant", variant)
        eq.set_terminal(terminal)
        return _sweep(torch, eq, y0, t_eval, fill=fill, stop=terminal is not None, events=events, max_events=max_events, max_attempts=max_attempts)
    finally:
        eq.close()


@pytest.fixture(scope="module")
def unlimited(torch_cuda, setup):
    """The yardstick: {variant: (y, res, frames)} without limits through sweep_dop853_device, roots located, frames at T_EVAL - each
    computed once, and held to what the tests below rely on (the counts scipy gives on the oracle)."""
    cache = {}

    def get(variant=None):
        if variant not in cache:
            y, res, frames = _run(torch_cuda, setup, t_eval=T_EVAL, variant=variant)
            counts = [[len(t) for t in r.t_events] for r in res]
            print(variant, "roots per monitor", counts, "steps of instance 4", res[4].n_accepted, res[4].n_rejected, "ones_Phi root", res[4].t_events[ONES_PHI])
            assert all(r.status == 0 for r in res) and counts[:4] == [[0] * 7] * 4 and counts[4] == [0, 0, 0, 0, 1, 0, 7], counts
            assert np.all(res[4].t_events[ZEROS_W] < T1) and res[4].t_events[ONES_PHI][0] < res[4].t_events[ZEROS_W][0]
            cache[variant] = (y, res, frames)
        return cache[variant]
    return get


def _same_instance(a, b, ya, yb, fa=None, fb=None):
    ok = np.array_equal(ya, yb) and _key(a) == _key(b) and _same_roots(a, b) and np.array_equal(a.event_values, b.event_values)
    ok = ok and a.h_next == b.h_next and (a.t is None) == (b.t is None) and (a.t is None or np.array_equal(a.t, b.t))
    return ok and (fa is None or np.array_equal(fa, fb, equal_nan=True))


def _check_stopped(rl, yl, fl, ru, fu, b, t_eval):
    """instance b of a sweep limited by ones_Phi: 1 against its own free run"""
    t_stop = ru[b].t_events[ONES_PHI][0]
    assert rl[b].status == 1 and rl[b].t_reached == t_stop and rl[b].message == "A termination event occurred."
    for m in range(7):      # the roots up to the stop: a prefix of the free run's, bit for bit
        k = len(rl[b].t_events[m])
        assert k == rl[b].n_events[m] and np.array_equal(rl[b].t_events[m], ru[b].t_events[m][:k]) and np.all(ru[b].t_events[m][k:] >= t_stop)
    assert len(rl[b].t_events[ONES_PHI]) == 1
    k = int(np.searchsorted(t_eval, t_stop, side="right"))
    assert len(rl[b].t) == k and np.array_equal(fl[b, :k], fu[b, :k]) and np.all(np.isnan(fl[b, k:]))
    assert abs(rl[b].event_values[ONES_PHI]) <= 1e-9


# 4 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", (0, 2))
def test_stops_the_one_instance_only(torch_cuda, setup, unlimited, variant):
    yu, ru, fu = unlimited(variant)
    yl, rl, fl = _run(torch_cuda, setup, {"ones_Phi": 1}, t_eval=T_EVAL, variant=variant)
    t_stop = ru[4].t_events[ONES_PHI][0]
    print(variant, "t_stop", t_stop, "status", [r.status for r in rl], "roots of instance 4", [len(t) for t in rl[4].t_events], "nfev", rl[4].nfev)
    assert rl[4].status == 1 and rl[4].t_reached == t_stop and rl[4].message == "A termination event occurred."
    assert [len(t) for t in rl[4].t_events] == [0, 0, 0, 0, 1, 0, 0] and rl[4].t_events[ONES_PHI][0] == t_stop
    assert list(rl[4].n_events) == [0, 0, 0, 0, 1, 0, 0]
    k = int(np.searchsorted(T_EVAL, t_stop, side="right"))
    assert len(rl[4].t) == k and np.array_equal(fl[4, :k], fu[4, :k]) and np.all(np.isnan(fl[4, k:]))
    for b in range(4):      # the other instances: bit for bit the run without the limit
        assert _same_instance(rl[b], ru[b], yl[b], yu[b], fl[b], fu[b]), (variant, b)


# 5 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rule_runs(torch_cuda, setup):
    cache = {}

    def get(e, k):
        if (e, k) not in cache:
            y, res, _ = _run(torch_cuda, setup, {NAMES[e]: k})
            cache[(e, k)] = (y[4], res[4])      # instance 4: the state and the result
        return cache[(e, k)]
    return get


@pytest.mark.parametrize("e, k", [(ZEROS_W, 2), (ZEROS_W, 7), (ONES_PHI, 1)])
def test_the_rule_on_the_device(unlimited, rule_runs, e, k):
    ru, rl = unlimited()[1][4], rule_runs(e, k)[1]
    t_stop, want = _expected_roots(ru.t_events, e, k)
    print(NAMES[e], k, "t_stop", t_stop, "roots", [len(t) for t in rl.t_events], "nfev", rl.nfev)
    assert rl.status == 1 and rl.t_reached == t_stop
    for m in range(7):
        assert np.array_equal(rl.t_events[m], want[m]), (e, k, m, rl.t_events[m], want[m])
        assert rl.n_events[m] == len(rl.t_events[m])


@pytest.mark.parametrize("limit", [{"zeros_CC": 1}, {"zeros_W": 8}])
def test_a_limit_that_is_never_met_changes_nothing(torch_cuda, setup, unlimited, limit):
    """The whole sweep through dop853_sweep_stop_kernel: bit for bit the sweep of marl_sweep_dop853_events_dev."""
    yu, ru, fu = unlimited()
    yl, rl, fl = _run(torch_cuda, setup, limit, t_eval=T_EVAL)
    for b in range(5):
        assert rl[b].status == 0 and _same_instance(rl[b], ru[b], yl[b], yu[b], fl[b], fu[b]), (limit, b)


# 6 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", (None, 2))
def test_frames_and_final_state(torch_cuda, setup, unlimited, variant):
    r = unlimited(variant)[1][4].t_events[ONES_PHI][0]
    t_eval = np.array([0.0, 0.5 * r, r, np.nextafter(r, np.inf), T1])
    _, _, fu = _run(torch_cuda, setup, t_eval=t_eval, variant=variant)
    yl, rl, fl = _run(torch_cuda, setup, {"ones_Phi": 1}, t_eval=t_eval, fill=SENTINEL, variant=variant)
    assert rl[4].status == 1 and len(rl[4].t) == 3                      # n_done == 3
    assert np.array_equal(fl[4, :3], fu[4, :3]) and np.all(fl[4, :3] != SENTINEL)
    assert np.all(fl[4, 3:] == SENTINEL)
    assert np.array_equal(yl[4], fl[4, 2])                              # the state returned is the frame at t_stop, bit for bit
    print(variant, "ones_Phi of the state returned", rl[4].event_values[ONES_PHI])
    assert abs(rl[4].event_values[ONES_PHI]) <= 1e-9                    # Brent's 4 eps times a slope of O(10): tests/test_gpu_terminal.py
    for b in range(4):
        assert len(rl[b].t) == 5 and np.array_equal(fl[b], fu[b])


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_counts_are_those_after_the_accepted_step(torch_cuda, setup, rule_runs):
    rl = rule_runs(ONES_PHI, 1)[1]
    A = rl.n_accepted + rl.n_rejected
    same = _run(torch_cuda, setup, max_attempts=A)[1][4]
    short = _run(torch_cuda, setup, max_attempts=A - 1)[1][4]
    print("attempts", A, "nfev", rl.nfev, "t_stop", rl.t_reached, "the run without limits after A / A - 1 attempts:", same.t_reached, short.t_reached)
    assert (same.nfev, same.n_accepted, same.n_rejected) == (rl.nfev, rl.n_accepted, rl.n_rejected)
    assert rl.nfev == 1 + NFEV_ATTEMPT * A + NFEV_DENSE                 # the terminal step's dense output, counted once; the stop counts nothing
    assert same.t_reached >= rl.t_reached > short.t_reached


# 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_no_slot_and_no_buffer(torch_cuda, setup, rule_runs):
    y_full, full = rule_runs(ZEROS_W, 2)
    t_stop = full.t_reached
    y1, res1, _ = _run(torch_cuda, setup, {"zeros_W": 2}, max_events=1)
    one = res1[4]
    assert one.status == 1 and one.t_reached == t_stop and len(one.t_events[ZEROS_W]) == 1 and one.n_events[ZEROS_W] == 2
    assert one.t_events[ZEROS_W][0] == full.t_events[ZEROS_W][0] and list(one.n_events) == list(full.n_events)
    assert np.array_equal(y1[4], y_full) and (one.nfev, one.n_accepted, one.n_rejected) == (full.nfev, full.n_accepted, full.n_rejected)
    for t_eval in (None, T_EVAL):      # no t_events at all, with frames and without
        y, res, _ = _run(torch_cuda, setup, {"zeros_W": 2}, events=False, t_eval=t_eval)
        plain = res[4]
        assert plain.status == 1 and plain.t_reached == t_stop and plain.t_events is None and list(plain.n_events) == list(full.n_events)
        assert np.array_equal(y[4], y_full)
        assert (plain.n_accepted, plain.n_rejected) == (full.n_accepted, full.n_rejected)


# 9 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def single(torch_cuda, setup):
    """Instance 4 alone through marl_integrate_dop853_stop: (without limits, with ones_Phi: 1, the free run's frame at t_stop, with
    ones_Phi: 1 and events=False)."""
    from marlpde_amd.LHeureux_model import LMAHeureuxPorosityDiff
    base, y0 = setup
    eq = LMAHeureuxPorosityDiff.from_scenario(base | INSTANCES[4], device=0)
    try:
        eq.set_terminal(None)
        free = eq.integrate_dop853_stop(y0[4], (0.0, T1), H0, RTOL, ATOL)
        eq.set_terminal({"ones_Phi": 1})
        stop = eq.integrate_dop853_stop(y0[4], (0.0, T1), H0, RTOL, ATOL)
        quiet = eq.integrate_dop853_stop(y0[4], (0.0, T1), H0, RTOL, ATOL, events=False)
        eq.set_terminal(None)
        frame = eq.integrate_dop853_stop(y0[4], (0.0, T1), H0, RTOL, ATOL, t_eval=np.array([stop.t_reached]))
    finally:
        eq.close()
    return free, stop, frame, quiet


def test_single_runs_against_their_own_run_without_limits(single):
    free, stop, frame, quiet = single
    assert free.status == 0 and stop.status == 1 and stop.message == "A termination event occurred."
    assert [len(t) for t in free.t_events] == [0, 0, 0, 0, 1, 0, 7]
    assert stop.t_reached == free.t_events[ONES_PHI][0] and list(stop.t) == [stop.t_reached]
    for m in range(7):      # the roots up to the stop: a prefix of the free run's, bit for bit
        k = len(stop.t_events[m])
        assert k == stop.n_events[m] and np.array_equal(stop.t_events[m], free.t_events[m][:k])
        assert np.all(free.t_events[m][k:] > stop.t_reached)
    assert frame.status == 0 and np.array_equal(stop.y_final, frame.y[:, 0])
    assert abs(stop.event_values[ONES_PHI]) <= 1e-9
    # without t_events the run stops all the same
    assert quiet.status == 1 and quiet.t_reached == stop.t_reached and np.array_equal(quiet.y_final, stop.y_final) and quiet.t_events is None
    assert list(quiet.n_events) == list(stop.n_events) and (quiet.nfev, quiet.n_accepted, quiet.n_rejected) == (stop.nfev, stop.n_accepted, stop.n_rejected)


def test_single_runs_against_solve_ivp(single, setup, oracle):
    """solve_ivp(method="DOP853") on the oracle's RHS and monitors with the same `terminal` flags: equal nfev, equal accepted count, equal
    root counts, and t_stop within the bound the project puts on root times against scipy."""
    from scipy.integrate import solve_ivp
    base, y0 = setup
    P = oracle.params_from_dict(base | INSTANCES[4])

    def event(e):
        f = lambda t, y: oracle.events(P, N, y)[e]  # noqa: E731
        f.terminal = e == ONES_PHI
        return f
    sol = solve_ivp(lambda t, y: oracle.rhs(P, N, y), (0.0, T1), y0[4], method="DOP853", first_step=H0, rtol=RTOL, atol=ATOL,
                    events=[event(e) for e in range(7)])
    stop = single[1]
    t_scipy = sol.t_events[ONES_PHI][0]
    print("t_stop", stop.t_reached, "scipy", t_scipy, "difference", abs(stop.t_reached - t_scipy), "nfev", stop.nfev, sol.nfev,
          "accepted + rejected", stop.n_accepted, stop.n_rejected, "scipy's accepted", len(sol.t) - 1)
    assert sol.status == 1 and sol.t[-1] == t_scipy
    assert [len(t) for t in stop.t_events] == [len(t) for t in sol.t_events] == [0, 0, 0, 0, 1, 0, 0]
    assert stop.nfev == sol.nfev and stop.n_accepted == len(sol.t) - 1     # decision for decision
    assert abs(stop.t_reached - t_scipy) <= ROOT_RTOL * abs(t_scipy) + ROOT_ATOL_T1 * T1


def test_the_sweeps_instance_against_the_single_run(single, rule_runs):
    """Both are dop853_sweep_stop_kernel at the same window: bit for bit."""
    (yl, rl), one = rule_runs(ONES_PHI, 1), single[1]
    assert rl.status == one.status == 1 and rl.t_reached == one.t_reached and np.array_equal(yl, one.y_final)
    assert _key(rl) == _key(one) and _same_roots(rl, one) and np.array_equal(rl.event_values, one.event_values)


# 11 --------------------------------------------------------------------------------------------------------------------------------
def _stop_entry(torch, eq, y0, t_eval, events, max_events=MAX_EVENTS, bad=None):
    """marl_sweep_dop853_stop_dev called directly -> (rc, states, stats, n_done, frames, t_events); bad: arguments to replace."""
    from marlpde_amd._abi import MarlStats
    B = y0.shape[0]
    yd = torch.from_numpy(y0).cuda()
    te = np.empty(0) if t_eval is None else np.ascontiguousarray(t_eval, dtype=np.float64)
    frames = torch.full((B, max(te.size, 1), y0.shape[1]), np.nan, dtype=yd.dtype, device=yd.device)
    n_done = np.full(B, -1, dtype=np.int64)
    tev = np.full((B, 7, max_events), np.nan)
    stats = (MarlStats * B)()
    a = dict(y=C.c_void_p(yd.data_ptr()), h0=H0, t_eval=te.ctypes.data_as(C.c_void_p) if te.size else None, n_eval=te.size) | (bad or {})
    rc = eq._lib.marl_sweep_dop853_stop_dev(
        eq._ctx, a["y"], 0.0, T1, a["h0"], RTOL, ATOL, 0, a["t_eval"], a["n_eval"], C.c_void_p(frames.data_ptr()) if te.size else None,
        n_done.ctypes.data_as(C.c_void_p), tev.ctypes.data_as(C.c_void_p) if events else None, max_events if events else 0, stats)
    return rc, yd.cpu().numpy(), stats, n_done, frames.cpu().numpy(), tev


def test_entries_without_a_limit_and_with_invalid_arguments(torch_cuda, setup, unlimited, single):
    from marlpde_amd._abi import MarlError
    from marlpde_amd.LHeureux_model import LMAHeureuxPorosityDiff, RK45Result
    torch = torch_cuda
    base, y0 = setup
    eq = _model(torch, base, INSTANCES)
    try:
        for t_eval, events in ((None, False), (T_EVAL, False), (T_EVAL, True), (None, True)):      # the three older entries, and roots without frames
            yo, ro, fo = _sweep(torch, eq, y0, t_eval, stop=False, events=events, max_events=MAX_EVENTS)
            rc, yn, stats, n_done, fn, tev = _stop_entry(torch, eq, y0, t_eval, events)
            assert rc == 0 and np.array_equal(yn, yo), events
            for b in range(5):
                rn = RK45Result(stats[b])
                assert _key(rn) == _key(ro[b]) and np.array_equal(rn.event_values, ro[b].event_values) and rn.h_next == ro[b].h_next
                assert n_done[b] == (0 if t_eval is None else len(ro[b].t))
                if events:
                    assert all(np.array_equal(tev[b, e, :len(ro[b].t_events[e])], ro[b].t_events[e]) for e in range(7))
                    assert all(np.all(np.isnan(tev[b, e, len(ro[b].t_events[e]):])) for e in range(7))
            if t_eval is not None:
                assert np.array_equal(fn, fo, equal_nan=True)
        # invalid arguments: -1, a message, and the context stays usable - with a limit set too
        eq.set_terminal({"ones_Phi": 1})
        for bad in (dict(y=None), dict(n_eval=3, t_eval=None), dict(n_eval=-1), dict(h0=0.0), dict(h0=1.0),
                    dict(t_eval=np.array([0.02, 0.01]).ctypes.data_as(C.c_void_p), n_eval=2)):
            rc, yn, *_ = _stop_entry(torch, eq, y0, T_EVAL, True, bad=bad)
            assert rc == -1 and eq._lib.marl_last_error(eq._ctx) and np.array_equal(yn, y0), bad
        yl, rl, _ = _sweep(torch, eq, y0, events=True, max_events=MAX_EVENTS)
        assert [r.status for r in rl] == [0, 0, 0, 0, 1] and rl[4].t_reached == unlimited()[1][4].t_events[ONES_PHI][0]
    finally:
        eq.close()
    one = LMAHeureuxPorosityDiff.from_scenario(base | INSTANCES[4], device=0)
    try:      # the single-run entry without a limit is marl_integrate_dop853
        older, free = one.integrate_dop853(y0[4], (0.0, T1), H0, RTOL, ATOL), single[0]
        assert np.array_equal(older.y_final, free.y_final) and _key(older) == _key(free) and _same_roots(older, free)
        with pytest.raises(MarlError):
            one.integrate_dop853_stop(y0[4], (0.0, T1), 0.0, RTOL, ATOL)
        again = one.integrate_dop853_stop(y0[4], (0.0, T1), H0, RTOL, ATOL)
        assert np.array_equal(again.y_final, free.y_final)
    finally:
        one.close()
    # a grid above one workgroup is refused first, with a limit set too
    big = LMAHeureuxPorosityDiff.from_scenario(_base(1025), device=0)
    try:
        big.set_terminal({"ones_Phi": 1})
        yb = _y0(_base(1025), [{}])[0]
        with pytest.raises(MarlError, match=r"rc=-1.*dop853: N = 1025: .*N <= 1024 cells"):
            big.integrate_dop853_stop(yb, (0.0, T1), H0, RTOL, ATOL)
        yd = torch.from_numpy(yb[None].copy()).cuda()
        with pytest.raises(MarlError, match=r"rc=-1.*dop853: N = 1025: .*N <= 1024 cells"):
            big.sweep_dop853_stop_device(yd.data_ptr(), (0.0, T1), H0, RTOL, ATOL)
        assert np.array_equal(yd.cpu().numpy()[0], yb)
    finally:
        big.close()


def test_drivers(torch_cuda, setup, unlimited, single):
    from dataclasses import asdict

    from marlpde_amd.Evolve_scenario import integrate_equations
    from marlpde_amd.parameters import Solver
    from marlpde_amd.sweep import HipSweepEngine, run_sweep_dop853_stop
    base, y0 = setup
    yu, ru, fu = unlimited()
    t_stop = ru[4].t_events[ONES_PHI][0]
    y, status, acc, rej, t = run_sweep_dop853_stop(base, INSTANCES, (0.0, T1), H0, RTOL, ATOL, device=0, terminal={"ones_Phi": True})
    assert list(status) == [0, 0, 0, 0, 1] and t[4] == t_stop and list(t[:4]) == [T1] * 4
    assert np.array_equal(y[:4], yu[:4]) and np.array_equal(y[4], single[1].y_final)
    free = run_sweep_dop853_stop(base, INSTANCES, (0.0, T1), H0, RTOL, ATOL, device=0)      # a limit does not outlive the call that set it
    assert list(free[1]) == [0] * 5 and np.array_equal(free[0], yu)
    eng = HipSweepEngine(base, INSTANCES, 0)
    try:
        ye, re = eng.integrate_dop853_stop(y0, (0.0, T1), H0, RTOL, ATOL, 0, t_eval=T_EVAL, events=True, terminal={"ones_Phi": 1})
    finally:
        eng.close()
    assert np.array_equal(ye, y) and [r.status for r in re] == [0, 0, 0, 0, 1] and re[4].t_reached == t_stop
    assert np.array_equal(re[4].y, fu[4, :len(re[4].t)].T) and [len(x) for x in re[4].t_events] == [0, 0, 0, 0, 1, 0, 0]

    pde = base | INSTANCES[4]
    solver = asdict(Solver(method="DOP853")) | {"t_span": (0.0, T1), "first_step": H0, "rtol": RTOL, "atol": ATOL}
    one = single[1]
    last, covered, *_ = integrate_equations(solver | {"native_terminal": True}, {}, pde, results_root=None, verbose=False, terminal={"ones_Phi": True})
    assert covered == pde["Tstar"] * one.t_reached and np.array_equal(last.ravel(), one.y_final)
    _, covered_free, *_ = integrate_equations(solver | {"native_terminal": True}, {}, pde, results_root=None, verbose=False)
    assert covered_free == pde["Tstar"] * T1


# one dPhi_variable case (the VD instantiations) ------------------------------------------------------------------------------------
def test_dphi_variable(torch_cuda, setup):
    vd = {"dPhi_variable": True}
    yu, ru, fu = _run(torch_cuda, setup, t_eval=T_EVAL, base_more=vd)
    yl, rl, fl = _run(torch_cuda, setup, {"ones_Phi": 1}, t_eval=T_EVAL, base_more=vd)
    stopping = [b for b in range(5) if len(ru[b].t_events[ONES_PHI]) > 0]
    print("dPhi_variable: status of the free run", [r.status for r in ru], "ones_Phi roots", [list(r.t_events[ONES_PHI]) for r in ru],
          "instances that stop", stopping, "status of the limited run", [r.status for r in rl])
    for b in range(5):
        if b in stopping:      # checked against its own free run
            _check_stopped(rl, yl, fl, ru, fu, b, T_EVAL)
        else:                  # no ones_Phi root: the limited sweep is the free sweep, bit for bit
            assert _same_instance(rl[b], ru[b], yl[b], yu[b], fl[b], fu[b]), b
