"""Terminal monitors in the explicit integrators (marl_set_terminal): RK45 and RK23 sweeps that end an instance at a monitor's root inside
the sweep kernel (rk45_sweep_term_kernel / rk23_sweep_term_kernel behind marl_sweep_rk45_terminal_dev / rk23_terminal_dev), and the single
runs that do it at a pause of their host loop (marl_integrate_rk45_terminal / rk23_terminal), as solve_ivp does (ivp.py:79-130, 681-723).
The yardstick is the same path's run without limits: up to the step that ends it a limited run IS that run, so roots, frames and counts
are compared bit for bit; only the comparisons with scipy and between loops carry a tolerance, those the project already has.
N = 64, the five instances of tests/test_gpu_sweep_radau_frames.py (the last is the default scenario: one ones_Phi root near 0.0136 and
seven zeros_W roots inside (0, 0.03)), t_span (0, 0.03), first step 1e-6, rtol = atol = 1e-3, max_events 64."""
import ctypes as C
import os

import numpy as np
import pytest

from common import GOLDEN, scenario
from test_gpu_sweep_radau_frames import ATOL, H0, INSTANCES, RTOL, _base, _key, _model, _same_roots, _y0
from test_gpu_terminal import _expected_roots

pytestmark = pytest.mark.gpu

N, T1, MAX_EVENTS = 64, 0.03, 64
T_EVAL = np.linspace(0.0, T1, 11)
METHODS = ("rk45", "rk23")
ONES_PHI, ZEROS_U, ZEROS_W = 4, 5, 6
SENTINEL = -7.25
NAMES = ("zeros", "zeros_CA", "zeros_CC", "ones_CA_plus_CC", "ones_Phi", "zeros_U", "zeros_W")
ROOT_RTOL, ROOT_ATOL_T1 = 1e-9, 1e-12      # root times against scipy, decision for decision (tests/test_gpu_sweep_events.py)
BETWEEN_CONTROLLERS = 5e-4                 # t_stop between two loops that round their steps differently (tests/test_gpu_terminal.py)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def setup():
    base = _base(N)
    return base, _y0(base, INSTANCES)


def _sweep(torch, eq, method, y0, t_eval=None, fill=np.nan, **kw):
    yd = torch.from_numpy(y0).cuda()
    sweep = getattr(eq, f"sweep_{method}_device")
    if t_eval is None:
        res = sweep(yd.data_ptr(), (0.0, T1), H0, RTOL, ATOL, **kw)
        return yd.cpu().numpy(), res, None
    frames = torch.full((y0.shape[0], len(t_eval), y0.shape[1]), fill, dtype=yd.dtype, device=yd.device)
    res = sweep(yd.data_ptr(), (0.0, T1), H0, RTOL, ATOL, t_eval=t_eval, y_eval_dev_ptr=frames.data_ptr(), **kw)
    return yd.cpu().numpy(), res, frames.cpu().numpy()


def _run(torch, setup, method, terminal=None, t_eval=None, fill=np.nan, events=True, max_events=MAX_EVENTS, max_attempts=0, variant=None):
    """One sweep of the five instances -> (states, results, frames); variant: the sweep_variant option (0 / 2: 256 / 1024 threads)."""
    base, y0 = setup
    eq = _model(torch, base, INSTANCES)
    try:
        if variant is not None:
            eq.set_option("sweep_variant", variant)
        eq.set_terminal(terminal)
        return _sweep(torch, eq, method, y0, t_eval, fill=fill, events=events, max_events=max_events, max_attempts=max_attempts)
    finally:
        eq.close()


@pytest.fixture(scope="module")
def unlimited(torch_cuda, setup):
    """The yardstick: {(method, variant): (y, res, frames)} without limits, roots located, frames at T_EVAL - each computed once, and
    held to what the tests below rely on: instances 0 - 3 without a sign change, instance 4 with one ones_Phi and seven zeros_W roots."""
    cache = {}

    def get(method, variant=None):
        if (method, variant) not in cache:
            y, res, frames = _run(torch_cuda, setup, method, t_eval=T_EVAL, variant=variant)
            counts = [[len(t) for t in r.t_events] for r in res]
            print(method, variant, "roots per monitor", counts, "steps of instance 4", res[4].n_accepted, res[4].n_rejected)
            assert all(r.status == 0 for r in res) and counts[:4] == [[0] * 7] * 4 and counts[4] == [0, 0, 0, 0, 1, 0, 7], counts
            assert np.all(res[4].t_events[ZEROS_W] < T1) and res[4].t_events[ONES_PHI][0] < res[4].t_events[ZEROS_W][0]
            cache[(method, variant)] = (y, res, frames)
        return cache[(method, variant)]
    return get


def _same_instance(a, b, ya, yb, fa=None, fb=None):
    ok = np.array_equal(ya, yb) and _key(a) == _key(b) and _same_roots(a, b) and np.array_equal(a.event_values, b.event_values)
    ok = ok and a.h_next == b.h_next and (a.t is None) == (b.t is None) and (a.t is None or np.array_equal(a.t, b.t))
    return ok and (fa is None or np.array_equal(fa, fb, equal_nan=True))


# 4 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", (0, 2))
@pytest.mark.parametrize("method", METHODS)
def test_stops_the_one_instance_only(torch_cuda, setup, unlimited, method, variant):
    yu, ru, fu = unlimited(method, variant)
    yl, rl, fl = _run(torch_cuda, setup, method, {"ones_Phi": 1}, t_eval=T_EVAL, variant=variant)
    t_stop = ru[4].t_events[ONES_PHI][0]
    print(method, variant, "t_stop", t_stop, "status", [r.status for r in rl], "roots of instance 4", [len(t) for t in rl[4].t_events])
    assert rl[4].status == 1 and rl[4].t_reached == t_stop and rl[4].message == "A termination event occurred."
    assert [len(t) for t in rl[4].t_events] == [0, 0, 0, 0, 1, 0, 0] and rl[4].t_events[ONES_PHI][0] == t_stop
    assert list(rl[4].n_events) == [0, 0, 0, 0, 1, 0, 0]
    k = int(np.searchsorted(T_EVAL, t_stop, side="right"))
    assert len(rl[4].t) == k and np.array_equal(fl[4, :k], fu[4, :k]) and np.all(np.isnan(fl[4, k:]))
    for b in range(4):      # the other instances: bit for bit the run without the limit
        assert _same_instance(rl[b], ru[b], yl[b], yu[b], fl[b], fu[b]), (method, variant, b)


# 5 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rule_runs(torch_cuda, setup):
    cache = {}

    def get(method, e, k):
        if (method, e, k) not in cache:
            y, res, _ = _run(torch_cuda, setup, method, {NAMES[e]: k})
            cache[(method, e, k)] = (y[4], res[4])      # instance 4: the state and the result
        return cache[(method, e, k)]
    return get


@pytest.mark.parametrize("e, k", [(ZEROS_W, 2), (ZEROS_W, 7), (ONES_PHI, 1)])
@pytest.mark.parametrize("method", METHODS)
def test_the_rule_on_the_device(unlimited, rule_runs, method, e, k):
    ru, rl = unlimited(method)[1][4], rule_runs(method, e, k)[1]
    t_stop, want = _expected_roots(ru.t_events, e, k)
    print(method, NAMES[e], k, "t_stop", t_stop, "roots", [len(t) for t in rl.t_events])
    assert rl.status == 1 and rl.t_reached == t_stop
    for m in range(7):
        assert np.array_equal(rl.t_events[m], want[m]), (method, e, k, m, rl.t_events[m], want[m])
        assert rl.n_events[m] == len(rl.t_events[m])


@pytest.mark.parametrize("limit", [{"zeros_CC": 1}, {"zeros_W": 8}])
@pytest.mark.parametrize("method", METHODS)
def test_a_limit_that_is_never_met_changes_nothing(torch_cuda, setup, unlimited, method, limit):
    """The whole sweep through the *_term_kernel: bit for bit the sweep of marl_sweep_*_events_dev."""
    yu, ru, fu = unlimited(method)
    yl, rl, fl = _run(torch_cuda, setup, method, limit, t_eval=T_EVAL)
    for b in range(5):
        assert rl[b].status == 0 and _same_instance(rl[b], ru[b], yl[b], yu[b], fl[b], fu[b]), (method, limit, b)


# 6 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", (None, 2))
@pytest.mark.parametrize("method", METHODS)
def test_frames_and_final_state(torch_cuda, setup, unlimited, method, variant):
    r = unlimited(method, variant)[1][4].t_events[ONES_PHI][0]
    t_eval = np.array([0.0, 0.5 * r, r, np.nextafter(r, np.inf), T1])
    _, _, fu = _run(torch_cuda, setup, method, t_eval=t_eval, variant=variant)
    yl, rl, fl = _run(torch_cuda, setup, method, {"ones_Phi": 1}, t_eval=t_eval, fill=SENTINEL, variant=variant)
    assert rl[4].status == 1 and len(rl[4].t) == 3                      # n_done == 3
    assert np.array_equal(fl[4, :3], fu[4, :3]) and np.all(fl[4, :3] != SENTINEL)
    assert np.all(fl[4, 3:] == SENTINEL)
    assert np.array_equal(yl[4], fl[4, 2])                              # the state returned is the frame at t_stop, bit for bit
    print(method, variant, "ones_Phi of the state returned", rl[4].event_values[ONES_PHI])
    assert abs(rl[4].event_values[ONES_PHI]) <= 1e-9                    # Brent's 4 eps times a slope of O(10): tests/test_gpu_terminal.py
    for b in range(4):
        assert len(rl[b].t) == 5 and np.array_equal(fl[b], fu[b])


# 7 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_counts_are_those_after_the_accepted_step(torch_cuda, setup, rule_runs, method):
    rl = rule_runs(method, ONES_PHI, 1)[1]
    A = rl.n_accepted + rl.n_rejected
    same = _run(torch_cuda, setup, method, max_attempts=A)[1][4]
    short = _run(torch_cuda, setup, method, max_attempts=A - 1)[1][4]
    print(method, "attempts", A, "t_stop", rl.t_reached, "the run without limits after A / A - 1 attempts:", same.t_reached, short.t_reached)
    assert (same.nfev, same.n_accepted, same.n_rejected) == (rl.nfev, rl.n_accepted, rl.n_rejected)
    assert same.t_reached >= rl.t_reached > short.t_reached


# 8 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_no_slot_and_no_buffer(torch_cuda, setup, rule_runs, method):
    y_full, full = rule_runs(method, ZEROS_W, 2)
    t_stop = full.t_reached
    one = _run(torch_cuda, setup, method, {"zeros_W": 2}, max_events=1)[1][4]
    assert one.status == 1 and one.t_reached == t_stop and len(one.t_events[ZEROS_W]) == 1 and one.n_events[ZEROS_W] == 2
    assert one.t_events[ZEROS_W][0] == full.t_events[ZEROS_W][0] and list(one.n_events) == list(full.n_events)
    for t_eval in (None, T_EVAL):      # no t_events at all, with frames and without
        y, res, _ = _run(torch_cuda, setup, method, {"zeros_W": 2}, events=False, t_eval=t_eval)
        plain = res[4]
        assert plain.status == 1 and plain.t_reached == t_stop and plain.t_events is None and list(plain.n_events) == list(full.n_events)
        assert np.array_equal(y[4], y_full)


# 9 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def single(torch_cuda, setup):
    """Instance 4 alone: {method: (without limits, with ones_Phi: 1 through the terminal entry, the free run's frame at t_stop)}."""
    from marlpde_amd.LHeureux_model import LMAHeureuxPorosityDiff
    base, y0 = setup
    eq = LMAHeureuxPorosityDiff.from_scenario(base | INSTANCES[4], device=0)
    out = {}
    try:
        for method in METHODS:
            eq.set_terminal(None)
            free = getattr(eq, "integrate_" + method)(y0[4], (0.0, T1), H0, RTOL, ATOL)
            eq.set_terminal({"ones_Phi": 1})
            stop = getattr(eq, f"integrate_{method}_terminal")(y0[4], (0.0, T1), H0, RTOL, ATOL)
            quiet = getattr(eq, f"integrate_{method}_terminal")(y0[4], (0.0, T1), H0, RTOL, ATOL, events=False)
            eq.set_terminal(None)
            frame = getattr(eq, "integrate_" + method)(y0[4], (0.0, T1), H0, RTOL, ATOL, t_eval=np.array([stop.t_reached]))
            out[method] = (free, stop, frame, quiet)
    finally:
        eq.close()
    return out


@pytest.mark.parametrize("method", METHODS)
def test_single_runs_against_their_own_run_without_limits(single, method):
    free, stop, frame, quiet = single[method]
    assert free.status == 0 and stop.status == 1 and stop.message == "A termination event occurred."
    assert [len(t) for t in free.t_events] == [0, 0, 0, 0, 1, 0, 7]
    assert stop.t_reached == free.t_events[ONES_PHI][0] and list(stop.t) == [stop.t_reached]
    for m in range(7):      # the roots up to the stop: a prefix of the free run's, bit for bit
        k = len(stop.t_events[m])
        assert k == stop.n_events[m] and np.array_equal(stop.t_events[m], free.t_events[m][:k])
        assert np.all(free.t_events[m][k:] > stop.t_reached)
    assert frame.status == 0 and np.array_equal(stop.y_final, frame.y[:, 0])
    assert abs(stop.event_values[ONES_PHI]) <= 1e-9
    # without t_events the loop pauses and stops all the same
    assert quiet.status == 1 and quiet.t_reached == stop.t_reached and np.array_equal(quiet.y_final, stop.y_final) and quiet.t_events is None
    assert list(quiet.n_events) == list(stop.n_events) and (quiet.nfev, quiet.n_accepted, quiet.n_rejected) == (stop.nfev, stop.n_accepted, stop.n_rejected)


@pytest.mark.parametrize("method", METHODS)
def test_single_runs_against_solve_ivp(single, setup, oracle, method):
    """solve_ivp on the oracle's RHS and monitors with the same `terminal` flags.  The run is decision for decision scipy's (equal accepted
    and rejected counts, printed), so t_stop is held to the bound the project puts on RK45 / RK23 root times against scipy.
    Measured on an MI355X: RK45 754 accepted + 169 rejected, nfev 5 539 on both sides, |t_stop - scipy| 3.8e-17; RK23 977 + 3, nfev 2 941,
    1.4e-16."""
    from scipy.integrate import solve_ivp
    base, y0 = setup
    P = oracle.params_from_dict(base | INSTANCES[4])

    def event(e):
        f = lambda t, y: oracle.events(P, N, y)[e]  # noqa: E731
        f.terminal = e == ONES_PHI
        return f
    sol = solve_ivp(lambda t, y: oracle.rhs(P, N, y), (0.0, T1), y0[4], method=method.upper(), first_step=H0, rtol=RTOL, atol=ATOL,
                    events=[event(e) for e in range(7)])
    stop = single[method][1]
    t_scipy = sol.t_events[ONES_PHI][0]
    print(method, "t_stop", stop.t_reached, "scipy", t_scipy, "difference", abs(stop.t_reached - t_scipy), "nfev", stop.nfev, sol.nfev,
          "accepted + rejected", stop.n_accepted, stop.n_rejected, "scipy's accepted", len(sol.t) - 1)
    assert sol.status == 1 and sol.t[-1] == t_scipy
    assert [len(t) for t in stop.t_events] == [len(t) for t in sol.t_events]
    assert stop.nfev == sol.nfev and stop.n_accepted == len(sol.t) - 1     # decision for decision
    assert abs(stop.t_reached - t_scipy) <= ROOT_RTOL * abs(t_scipy) + ROOT_ATOL_T1 * T1


@pytest.mark.parametrize("method", METHODS)
def test_the_sweeps_instance_against_the_single_run(single, rule_runs, method):
    rl, one = rule_runs(method, ONES_PHI, 1)[1], single[method][1]
    print(method, "sweep", rl.t_reached, "single run", one.t_reached, "difference", abs(rl.t_reached - one.t_reached))
    assert rl.status == one.status == 1 and abs(rl.t_reached - one.t_reached) <= BETWEEN_CONTROLLERS
    assert [len(t) for t in rl.t_events] == [len(t) for t in one.t_events]


# 10 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_single_runs_above_one_workgroup(method):
    """N = 1500, the inputs of tests/golden/rk23_event_default_N1500.npz (a zeros_U root near 1.2223e-4): RK23 runs one launch per
    attempt, RK45 the streamed loop; both pause on the sign change and end there."""
    from test_gpu_rk23 import roots_close
    g = np.load(os.path.join(GOLDEN, "rk23_event_default_N1500.npz"))
    t1, args = float(g["t_span"][1]), (float(g["first_step"]), float(g["rtol"]), float(g["atol"]))
    from marlpde_amd.LHeureux_model import LMAHeureuxPorosityDiff
    eq = LMAHeureuxPorosityDiff.from_scenario(scenario("default", 1500), device=0)
    try:
        free = getattr(eq, "integrate_" + method)(g["y0"], (0.0, t1), *args)
        eq.set_terminal({"zeros_U": 1})
        stop = getattr(eq, f"integrate_{method}_terminal")(g["y0"], (0.0, t1), *args)
        eq.set_terminal(None)
        frame = getattr(eq, "integrate_" + method)(g["y0"], (0.0, t1), *args, t_eval=np.array([stop.t_reached]))
    finally:
        eq.close()
    print(method, "free run's roots", [len(t) for t in free.t_events], "t_stop", stop.t_reached, "attempts", stop.n_accepted + stop.n_rejected)
    assert free.status == 0 and len(free.t_events[ZEROS_U]) >= 1
    assert stop.status == 1 and stop.t_reached == free.t_events[ZEROS_U][0]
    assert [len(t) for t in stop.t_events] == [0, 0, 0, 0, 0, 1, 0] and stop.t_events[ZEROS_U][0] == stop.t_reached
    assert np.array_equal(stop.y_final, frame.y[:, 0])
    if method == "rk23":
        roots_close(stop.t_events, [g["t_events"][:1] if e == ZEROS_U else np.empty(0) for e in range(7)], t1)


# 11 --------------------------------------------------------------------------------------------------------------------------------
def _terminal_entry(torch, eq, method, y0, t_eval, events, max_events=MAX_EVENTS, bad=None):
    """marl_sweep_<method>_terminal_dev called directly -> (rc, states, stats, n_done, frames, t_events); bad: arguments to replace."""
    from marlpde_amd._abi import MarlStats
    B = y0.shape[0]
    yd = torch.from_numpy(y0).cuda()
    te = np.empty(0) if t_eval is None else np.ascontiguousarray(t_eval, dtype=np.float64)
    frames = torch.full((B, max(te.size, 1), y0.shape[1]), np.nan, dtype=yd.dtype, device=yd.device)
    n_done = np.full(B, -1, dtype=np.int64)
    tev = np.full((B, 7, max_events), np.nan)
    stats = (MarlStats * B)()
    a = dict(y=C.c_void_p(yd.data_ptr()), h0=H0, t_eval=te.ctypes.data_as(C.c_void_p) if te.size else None, n_eval=te.size) | (bad or {})
    rc = getattr(eq._lib, f"marl_sweep_{method}_terminal_dev")(
        eq._ctx, a["y"], 0.0, T1, a["h0"], RTOL, ATOL, 0, a["t_eval"], a["n_eval"], C.c_void_p(frames.data_ptr()) if te.size else None,
        n_done.ctypes.data_as(C.c_void_p), tev.ctypes.data_as(C.c_void_p) if events else None, max_events if events else 0, stats)
    return rc, yd.cpu().numpy(), stats, n_done, frames.cpu().numpy(), tev


@pytest.mark.parametrize("method", METHODS)
def test_entries_without_a_limit_and_with_invalid_arguments(torch_cuda, setup, unlimited, single, method):
    from marlpde_amd.LHeureux_model import LMAHeureuxPorosityDiff, RK45Result
    torch = torch_cuda
    base, y0 = setup
    eq = _model(torch, base, INSTANCES)
    try:
        for t_eval, events in ((None, False), (T_EVAL, False), (T_EVAL, True), (None, True)):      # the three older entries, and roots without frames
            yo, ro, fo = _sweep(torch, eq, method, y0, t_eval, events=events, max_events=MAX_EVENTS)
            rc, yn, stats, n_done, fn, tev = _terminal_entry(torch, eq, method, y0, t_eval, events)
            assert rc == 0 and np.array_equal(yn, yo), (method, events)
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
            rc, yn, *_ = _terminal_entry(torch, eq, method, y0, T_EVAL, True, bad=bad)
            assert rc == -1 and eq._lib.marl_last_error(eq._ctx) and np.array_equal(yn, y0), bad
        yl, rl, _ = _sweep(torch, eq, method, y0, events=True, max_events=MAX_EVENTS)
        assert [r.status for r in rl] == [0, 0, 0, 0, 1] and rl[4].t_reached == unlimited(method)[1][4].t_events[ONES_PHI][0]
    finally:
        eq.close()
    one = LMAHeureuxPorosityDiff.from_scenario(base | INSTANCES[4], device=0)
    try:      # the single-run entry without a limit is marl_integrate_<method>
        free, again = single[method][0], getattr(one, f"integrate_{method}_terminal")(y0[4], (0.0, T1), H0, RTOL, ATOL)
        assert np.array_equal(again.y_final, free.y_final) and _key(again) == _key(free) and _same_roots(again, free)
        from marlpde_amd._abi import MarlError
        with pytest.raises(MarlError):
            getattr(one, f"integrate_{method}_terminal")(y0[4], (0.0, T1), 0.0, RTOL, ATOL)
        again = getattr(one, f"integrate_{method}_terminal")(y0[4], (0.0, T1), H0, RTOL, ATOL)
        assert np.array_equal(again.y_final, free.y_final)
    finally:
        one.close()


@pytest.mark.parametrize("method", METHODS)
def test_drivers(torch_cuda, setup, unlimited, single, method):
    from dataclasses import asdict

    from marlpde_amd import sweep
    from marlpde_amd.Evolve_scenario import integrate_equations
    from marlpde_amd.parameters import Solver
    base, y0 = setup
    run = getattr(sweep, "run_sweep_" + method)
    yu, ru, _ = unlimited(method)
    t_stop = ru[4].t_events[ONES_PHI][0]
    y, status, acc, rej, t = run(base, INSTANCES, (0.0, T1), H0, RTOL, ATOL, device=0, terminal={"ones_Phi": True})
    assert list(status) == [0, 0, 0, 0, 1] and t[4] == t_stop and list(t[:4]) == [T1] * 4
    assert np.array_equal(y[:4], yu[:4])
    free = run(base, INSTANCES, (0.0, T1), H0, RTOL, ATOL, device=0)      # a limit does not outlive the call that set it
    assert list(free[1]) == [0] * 5 and np.array_equal(free[0], yu)

    pde = base | INSTANCES[4]
    solver = asdict(Solver(method=method.upper())) | {"t_span": (0.0, T1), "first_step": H0, "rtol": RTOL, "atol": ATOL}
    one = single[method][1]
    last, covered, *_ = integrate_equations(solver | {"native_terminal": True}, {}, pde, results_root=None, verbose=False, terminal={"ones_Phi": 1})
    assert covered == pde["Tstar"] * one.t_reached and np.array_equal(last.ravel(), one.y_final)
    _, covered_free, *_ = integrate_equations(solver | {"native_terminal": True}, {}, pde, results_root=None, verbose=False)
    assert covered_free == pde["Tstar"] * T1
    with pytest.raises(ValueError, match="scipy_driver=True") as err:
        integrate_equations(solver, {}, pde, results_root=None, verbose=False, terminal={"ones_Phi": 1})
    assert "native_terminal=True" in str(err.value)
