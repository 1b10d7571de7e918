"""The native DOP853 loop of ONE grid of any size on the GPU (marl_integrate_dop853_grid / _dev; kernels: csrc/marl_dop853_grid.h): one
launch per stage, the stage derivatives in an arena, the records reduced in a fixed order.

References: solve_ivp(method="DOP853", events=[7 monitors], t_eval=...) on the CPU oracle's RHS and monitors, computed here
(tests/dop853_ref.py) - every run takes about a second of scipy at most - and one golden file of tools/make_dop853_goldens.py.  States, time
spans and helpers are those of tests/test_gpu_rk23.py (synthetic_state, bump_state, make_model, counts, roots_close).

Bounds - those of tests/test_gpu_dop853.py:
    counts      (status, n_accepted, n_rejected, nfev) equal, nfev = 1 + 12 attempts + 3 (accepted steps with a dense output: a monitor sign
                change or a t_eval sample in them).  What makes equality a fair demand is asserted where the references are made: no
                attempt of a reference run has an error norm within 1e-4 of 1 (`margin`); the attempt and rejection counts of every
                reference are pinned too, so that a changed oracle is noticed.
    states      final states and frames: rel_to_max <= 1e-9 - but the FRAMES of the t_eval run at N = 1025: <= 2.21e-7.  There the frames at
                0.5 t1 and 0.77 t1 differ from scipy's by up to 5.6e-9 (every count equal, the final state within 1.3e-11).  scipy itself
                moves further: with its RHS multiplied elementwise by 1 + 2.5e-16 N(0, 1) - the median elementwise distance of the HIP
                RHS from the oracle's on this run's states, measured here (99th percentile 1.2e-15) - the same frames of the same run
                spread by 2.21e-8 with no decision changed (1.51e-8 at 1.2e-15; tools/dop853_noise.py grid1025, 8 seeds): the step
                controller saw-tooths at the stability limit and the frames catch it mid-tooth, as at N513 in tests/test_gpu_dop853.py.
                The bound is 10 x that spread; the final state of that run and everything else keep 1e-9.
    roots      |t - t_ref| <= 1e-9 |t_ref| + 1e-12 t1
    bit for bit the device entry against the host entry, a second identical call against the first (the reductions have a fixed order and
                there is no atomic), a run that locates roots against one that does not, a limit that is never met against no limit, the
                state of a stopped run against a frame asked for at t_stop.
The large-grid path and the one-workgroup path (marl_integrate_dop853) need NOT agree bit for bit: the one-workgroup body reduces its
error sums over one window of up to 1024 threads, this one over windows of 254 cells and then over the windows, so the sums are ordered
differently and the step sizes differ in their last bits.  Where both can run they are held to the same reference, and to equal counts.
The worst values are printed per test (pytest -rA: lines starting with DOP853 grid) and recorded in MEASURED below."""
import os

import numpy as np
import pytest

from common import GOLDEN, rel_to_max, scenario, synthetic_state
from dop853_ref import scipy_dop853
from test_gpu_rk23 import bump_state, counts, make_model, roots_close

pytestmark = pytest.mark.gpu

STATE_TOL = 1e-9
ROOT_RTOL, ROOT_ATOL_T1 = 1e-9, 1e-12
MARGIN = 1e-4
RTOL, ATOL = 1e-5, 1e-7
FRAME_TOL_1025 = 10 * 2.21e-8   # the frames of the t_eval run at N = 1025 (see above); everything else: STATE_TOL

# measured on an MI355X (pytest -rA): worst rel_to_max of final states and frames, worst root |dt| / t1, per group of tests
MEASURED = {
    # group                                             final states     frames           roots
    "shapes 255 .. 2540, both layouts, both entries": dict(state=1.27e-11, frame=None, root=None),          # N = 1025; the others <= 7.7e-13
    "N = 5003 default":                               dict(state=3.10e-11, frame=None, root=None),
    "t_eval at N = 1025":                             dict(state=1.27e-11, frame=5.60e-09, root=None),      # the frames at 0.5 t1 / 0.77 t1: see above
    "root and samples, N = 1100":                     dict(state=5.34e-13, frame=1.46e-10, root=1.26e-13),
    "stop, N = 1100":                                 dict(state=None, frame=3.86e-11, root=1.26e-13),      # |t_stop - scipy's| / t1
    "golden N = 200":                                 dict(state=1.62e-13, frame=2.86e-11, root=None),
    "N = 513 against the one-workgroup path":         dict(state=0.0, frame=None, root=4.30e-16),           # equal counts; here also equal states
}

# (scenario, N, span in dx^2, dPhi_variable, amplitude): (why this grid, attempts, rejections of scipy DOP853 on the oracle)
SHAPES = {
    ("A", 255, 40, False, 0.05): ("the second window holds one cell", 29, 4),
    ("A", 508, 40, False, 0.05): ("exactly two windows of 254", 27, 3),
    ("A", 1025, 40, False, 0.05): ("the first grid the one-workgroup entries refuse; last window 9 cells", 26, 3),
    ("A", 1271, 40, False, 0.05): ("one cell past 5 x 254", 29, 6),
    ("A", 2540, 40, False, 0.05): ("exact multiple of the window's 254 written cells", 27, 4),
    ("A", 2540, 40, True, 0.05): ("the dPhi_variable instantiation", 27, 4),
    ("default", 5003, 60, False, 0.01): ("twenty windows, the default scenario", 57, 3),
}
_REF = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _freeze(r):
    for a in (r.y_final, r.y_eval, *r.t_events):
        if a is not None:
            a.setflags(write=False)
    return r


def _reference(oracle, name, N, m, vd, amplitude):
    """scipy DOP853 on the oracle, made once per session and never changed -> (scenario, y0, dx^2, reference)"""
    key = (name, N, m, vd, amplitude)
    if key not in _REF:
        p = scenario(name, N) | ({"dPhi_variable": True} if vd else {})
        y = synthetic_state(p, N, amplitude=amplitude)
        dx2 = ((p["max_depth"] / p["Xstar"]) / N) ** 2
        ref = _freeze(scipy_dop853(oracle, oracle.params_from_dict(p), N, y, (0.0, m * dx2), 0.5 * dx2, RTOL, ATOL))
        print(f"DOP853 grid {name} N={N} vd={vd}: scipy attempts {ref.n_accepted + ref.n_rejected} rejected {ref.n_rejected} nfev {ref.nfev} "
              f"closest norm {ref.margin:.1e}")
        assert ref.status == 0 and ref.margin > MARGIN
        assert (ref.n_accepted + ref.n_rejected, ref.n_rejected) == SHAPES[key][1:], SHAPES[key][0]
        _REF[key] = (p, y, dx2, ref)
    return _REF[key]


def _run_device(torch, eq, y, t_span, h0, layout, max_attempts=0):
    yd = torch.from_numpy(y).cuda()
    if layout == 0:
        res = eq.integrate_dop853_grid_device(yd.data_ptr(), t_span, h0, RTOL, ATOL, layout, max_attempts)
        got = yd
    else:
        yt = torch.zeros(eq.state_doubles(layout), dtype=torch.float64, device="cuda")
        eq.convert_layout_device(yd.data_ptr(), yt.data_ptr(), 0, layout)
        res = eq.integrate_dop853_grid_device(yt.data_ptr(), t_span, h0, RTOL, ATOL, layout, max_attempts)
        got = torch.empty_like(yd)
        eq.convert_layout_device(yt.data_ptr(), got.data_ptr(), layout, 0)
    torch.cuda.synchronize()
    return res, got.cpu().numpy()


def _key(r):
    return (r.status, r.n_accepted, r.n_rejected, r.nfev, r.t_reached, r.h_next, tuple(r.n_events), tuple(r.event_values))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. shapes against scipy, both layouts, both entries
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("N,vd", [(255, False), (508, False), (1025, False), (1271, False), (2540, False), (2540, True)])
def test_shapes_against_scipy_both_layouts_both_entries(torch_cuda, oracle, N, vd, layout):
    p, y, dx2, ref = _reference(oracle, "A", N, 40, vd, 0.05)
    t1, h0 = 40 * dx2, 0.5 * dx2
    eq = make_model(p)
    try:
        eq.use_stream(torch_cuda.cuda.current_stream().cuda_stream)
        eq.set_option("host_layout", layout)
        res, got = _run_device(torch_cuda, eq, y, (0.0, t1), h0, layout)
        again, got2 = _run_device(torch_cuda, eq, y, (0.0, t1), h0, layout)
        host = eq.integrate_dop853_grid(y, (0.0, t1), h0, RTOL, ATOL, events=False)
    finally:
        eq.close()
    want = (ref.status, ref.n_accepted, ref.n_rejected, ref.nfev)
    assert counts(res) == want and counts(host) == want and res.t_reached == t1 and host.t_reached == t1
    e_dev, e_host = rel_to_max(got, ref.y_final), rel_to_max(host.y_final, ref.y_final)
    print(f"DOP853 grid N={N} vd={vd} layout={layout}: device entry {e_dev:.2e} host entry {e_host:.2e}")
    assert e_dev <= STATE_TOL and e_host <= STATE_TOL
    assert np.array_equal(got, host.y_final) and _key(res) == _key(host)
    assert np.array_equal(got2, got) and _key(again) == _key(res)      # fixed reduction order: a run is reproducible bit for bit


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. N = 5003, and t_eval / the attempt budget at N = 1025
# ---------------------------------------------------------------------------------------------------------------------------------
def test_default_scenario_n5003_and_t_eval_and_budget_at_n1025(torch_cuda, oracle):
    p, y, dx2, ref = _reference(oracle, "default", 5003, 60, False, 0.01)
    eq = make_model(p)
    try:
        res, got = _run_device(torch_cuda, eq, y, (0.0, 60 * dx2), 0.5 * dx2, 0)
    finally:
        eq.close()
    assert counts(res) == (0, ref.n_accepted, ref.n_rejected, ref.nfev) and res.t_reached == 60 * dx2
    e5003 = rel_to_max(got, ref.y_final)
    # five samples, both ends included, at the first grid past the one-workgroup window
    p, y, dx2, plain = _reference(oracle, "A", 1025, 40, False, 0.05)
    t1, h0 = 40 * dx2, 0.5 * dx2
    te = t1 * np.array([0.0, 0.13, 0.5, 0.77, 1.0])
    ref = scipy_dop853(oracle, oracle.params_from_dict(p), 1025, y, (0.0, t1), h0, RTOL, ATOL, t_eval=te)
    assert ref.margin > MARGIN and (ref.n_accepted + ref.n_rejected, len(ref.dense_steps), ref.nfev) == (26, 5, 328)
    eq = make_model(p)
    try:
        res = eq.integrate_dop853_grid(y, (0.0, t1), h0, RTOL, ATOL, t_eval=te)
        cut = eq.integrate_dop853_grid(y, (0.0, t1), h0, RTOL, ATOL, max_attempts=9, events=False)
        cut_dev, _ = _run_device(torch_cuda, eq, y, (0.0, t1), h0, 0, max_attempts=9)
    finally:
        eq.close()
    assert counts(res) == (0, ref.n_accepted, ref.n_rejected, 328) and np.array_equal(res.t, te) and np.array_equal(res.y[:, 0], y)
    worst = max(rel_to_max(res.y[:, j], ref.y_eval[j]) for j in range(len(te)))
    final = rel_to_max(res.y_final, ref.y_final)
    assert [len(e) for e in res.t_events] == [len(e) for e in ref.t_events]
    for c in (cut, cut_dev):
        assert c.status == 2 and c.n_accepted + c.n_rejected == 9 and c.nfev == 1 + 12 * 9
    print(f"DOP853 grid N=5003 final {e5003:.2e}; N=1025 frames {worst:.2e} final {final:.2e}")
    assert e5003 <= STATE_TOL and worst <= FRAME_TOL_1025 and final <= STATE_TOL


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. / 4. a root, samples and a stop at N = 1100: the porosity-dip state, zeros_U changes sign at 0.1839 t1
# ---------------------------------------------------------------------------------------------------------------------------------
N_EV, M_EV, ZEROS_U = 1100, 300, 5


@pytest.fixture(scope="module")
def event_case(oracle):
    p = scenario("default", N_EV)
    y = bump_state(p, N_EV, phi_dip=0.037)
    dx2 = ((p["max_depth"] / p["Xstar"]) / N_EV) ** 2
    t1, h0 = M_EV * dx2, 0.5 * dx2
    te = t1 * np.array([0.0, 0.25, 0.5, 1.0])
    ref = _freeze(scipy_dop853(oracle, oracle.params_from_dict(p), N_EV, y, (0.0, t1), h0, RTOL, ATOL, t_eval=te))
    print(f"DOP853 grid event N={N_EV}: scipy attempts {ref.n_accepted + ref.n_rejected} rejected {ref.n_rejected} nfev {ref.nfev} "
          f"closest norm {ref.margin:.1e} root / t1 {[list(t / t1) for t in ref.t_events]}")
    assert ref.status == 0 and ref.margin > MARGIN
    assert (ref.n_accepted + ref.n_rejected, ref.n_rejected, len(ref.dense_steps), ref.nfev) == (276, 4, 5, 3328)
    assert [len(t) for t in ref.t_events] == [0, 0, 0, 0, 0, 1, 0] and abs(ref.t_events[ZEROS_U][0] / t1 - 0.1839) < 1e-3
    return p, y, t1, h0, te, ref


def test_root_and_samples_at_n1100(event_case):
    p, y, t1, h0, te, ref = event_case
    eq = make_model(p)
    try:
        res = eq.integrate_dop853_grid(y, (0.0, t1), h0, RTOL, ATOL, t_eval=te)
        quiet = eq.integrate_dop853_grid(y, (0.0, t1), h0, RTOL, ATOL, t_eval=te, events=False)
        bare = eq.integrate_dop853_grid(y, (0.0, t1), h0, RTOL, ATOL, events=False)
    finally:
        eq.close()
    assert counts(res) == (0, ref.n_accepted, ref.n_rejected, 3328) and res.t_reached == t1
    assert list(res.n_events) == [0, 0, 0, 0, 0, 1, 0]
    worst_root = roots_close(res.t_events, ref.t_events, t1)
    assert np.array_equal(res.t, te) and np.array_equal(res.y[:, 0], y)
    worst = max(rel_to_max(res.y[:, j], ref.y_eval[j]) for j in range(len(te)))
    final = rel_to_max(res.y_final, ref.y_final)
    print(f"DOP853 grid event N={N_EV}: final {final:.2e} frames {worst:.2e} root |dt|/t1 {worst_root:.2e}")
    assert worst <= STATE_TOL and final <= STATE_TOL
    # locating the root leaves the integration alone: without t_events the same state and frames bit for bit, the same counts
    assert quiet.t_events is None and np.array_equal(quiet.y_final, res.y_final) and np.array_equal(quiet.y, res.y) and _key(quiet) == _key(res)
    # neither samples nor roots: the monitors are still watched, the sign change counts its step's dense output
    assert counts(bare) == (0, ref.n_accepted, ref.n_rejected, 1 + 12 * 276 + 3) and np.array_equal(bare.y_final, res.y_final)
    assert list(bare.n_events) == [0, 0, 0, 0, 0, 1, 0]


def test_stop_at_n1100(torch_cuda, event_case, oracle):
    """solve_ivp(method="DOP853") on the oracle with zeros_U terminal: status 1, two frames, the root at 0.18392 t1, nfev 658 (54 attempts,
    3 steps with a dense output: the two samples' and the root's)."""
    from scipy.integrate import solve_ivp

    from marlpde_amd._abi import MarlError
    p, y, t1, h0, _, free_ref = event_case
    te = t1 * np.array([0.0, 0.1, 0.5, 1.0])
    P = oracle.params_from_dict(p)

    def event(e):
        f = lambda t, s: oracle.events(P, N_EV, s)[e]  # noqa: E731
        f.terminal = e == ZEROS_U
        return f
    sol = solve_ivp(lambda t, s: oracle.rhs(P, N_EV, s), (0.0, t1), y, method="DOP853", first_step=h0, rtol=RTOL, atol=ATOL, t_eval=te,
                    events=[event(e) for e in range(7)])
    t_scipy = sol.t_events[ZEROS_U][0]
    assert sol.status == 1 and sol.nfev == 658 and len(sol.t) == 2 and abs(t_scipy / t1 - 0.18392) < 1e-4
    assert [len(t) for t in sol.t_events] == [0, 0, 0, 0, 0, 1, 0]
    eq = make_model(p)
    try:
        free = eq.integrate_dop853_grid(y, (0.0, t1), h0, RTOL, ATOL, t_eval=te)
        eq.set_terminal({"zeros_CC": 1})                       # a limit that is never met: the run without limits, bit for bit
        unmet = eq.integrate_dop853_grid(y, (0.0, t1), h0, RTOL, ATOL, t_eval=te)
        eq.set_terminal({"zeros_U": True})
        stop = eq.integrate_dop853_grid(y, (0.0, t1), h0, RTOL, ATOL, t_eval=te)
        quiet = eq.integrate_dop853_grid(y, (0.0, t1), h0, RTOL, ATOL, t_eval=te, events=False)
        at_stop = np.array([0.0, 0.1 * t1, stop.t_reached])
        frame = eq.integrate_dop853_grid(y, (0.0, t1), h0, RTOL, ATOL, t_eval=at_stop)
        yd = torch_cuda.from_numpy(y).cuda()
        with pytest.raises(MarlError, match=r"rc=-1.*marl_integrate_dop853_grid_dev: terminal monitors are not supported by this entry \(marl_set_terminal\)"):
            eq.integrate_dop853_grid_device(yd.data_ptr(), (0.0, t1), h0, RTOL, ATOL, 0)
        torch_cuda.cuda.synchronize()
        assert np.array_equal(yd.cpu().numpy(), y)
    finally:
        eq.close()
    assert free.status == 0 and np.array_equal(unmet.y_final, free.y_final) and np.array_equal(unmet.y, free.y) and _key(unmet) == _key(free)
    assert all(np.array_equal(a, b) for a, b in zip(unmet.t_events, free.t_events))
    # the stop: scipy's status, counts, frames reached and root; t_reached is the root; the state is the step's dense output there
    assert stop.status == 1 and stop.nfev == sol.nfev and stop.n_accepted == len(free_ref.step_times[free_ref.step_times <= t_scipy])
    assert stop.n_accepted + stop.n_rejected == 54
    assert [len(t) for t in stop.t_events] == [0, 0, 0, 0, 0, 1, 0] and list(stop.n_events) == [0, 0, 0, 0, 0, 1, 0]
    assert stop.t_reached == stop.t_events[ZEROS_U][0]
    assert abs(stop.t_reached - t_scipy) <= ROOT_RTOL * abs(t_scipy) + ROOT_ATOL_T1 * t1
    assert np.array_equal(stop.t, te[:2]) and len(sol.t) == 2                                    # n_done; the later frames are not returned
    assert np.array_equal(stop.y, free.y[:, :2])                                                 # the steps before the stop are the free run's
    worst = max(rel_to_max(stop.y[:, j], sol.y[:, j]) for j in range(2))
    assert np.array_equal(frame.t, at_stop) and np.array_equal(frame.y[:, 2], stop.y_final) and np.array_equal(frame.y_final, stop.y_final)
    assert abs(stop.event_values[ZEROS_U]) <= 1e-9
    assert quiet.status == 1 and quiet.t_reached == stop.t_reached and np.array_equal(quiet.y_final, stop.y_final) and quiet.t_events is None
    assert (quiet.nfev, quiet.n_accepted, quiet.n_rejected, list(quiet.n_events)) == (stop.nfev, stop.n_accepted, stop.n_rejected, list(stop.n_events))
    print(f"DOP853 grid stop N={N_EV}: t_stop / t1 {stop.t_reached / t1:.6f} scipy {t_scipy / t1:.6f} |dt|/t1 {abs(stop.t_reached - t_scipy) / t1:.2e} "
          f"frames {worst:.2e} nfev {stop.nfev}")
    assert worst <= STATE_TOL


def test_later_frames_of_a_stopped_run_are_untouched(torch_cuda, event_case):
    """The C entry itself: frames beyond the stop keep what the caller put there."""
    import ctypes as C

    from marlpde_amd._abi import MarlStats
    p, y, t1, h0, _, _ = event_case
    te = t1 * np.array([0.0, 0.1, 0.5, 1.0])
    frames = np.full((4, y.size), -7.0)
    state = y.copy()
    stats = MarlStats()
    eq = make_model(p)
    try:
        eq.set_terminal({"zeros_U": 1})
        rc = eq._lib.marl_integrate_dop853_grid(eq._ctx, state.ctypes.data_as(C.c_void_p), 0.0, t1, h0, RTOL, ATOL, te.ctypes.data_as(C.c_void_p), 4,
                                                frames.ctypes.data_as(C.c_void_p), None, 0, 0, C.byref(stats))
    finally:
        eq.close()
    assert rc == 0 and stats.status == 1 and np.array_equal(frames[0], y) and not np.any(frames[1] == -7.0) and np.all(frames[2:] == -7.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. against the one-workgroup path
# ---------------------------------------------------------------------------------------------------------------------------------
def test_golden_n200_and_the_one_workgroup_path_at_n513(oracle):
    g = np.load(os.path.join(GOLDEN, "dop853_traj_default_N200.npz"))
    N, t1 = g["y0"].size // 5, float(g["t_span"][1])
    assert float(g["err_margin"]) > MARGIN
    eq = make_model(scenario("default", N))
    try:
        res = eq.integrate_dop853_grid(g["y0"], tuple(g["t_span"]), float(g["first_step"]), float(g["rtol"]), float(g["atol"]), t_eval=g["t_eval"])
    finally:
        eq.close()
    assert counts(res) == (0, int(g["n_accepted"]), int(g["n_rejected"]), int(g["nfev"])) and res.t_reached == t1
    assert np.array_equal(res.t, g["t_eval"]) and np.array_equal(res.y[:, 0], g["y0"])
    assert [len(e) for e in res.t_events] == list(g["n_events"])
    err = rel_to_max(res.y_final, g["y_final"])
    worst_frame = max(rel_to_max(res.y[:, j], g["y_eval"][:, j]) for j in range(len(g["t_eval"])))
    # N = 513, the porosity-dip instance of the sweep tests alone: three windows here, one window of 1024 threads there
    from test_gpu_dop853 import DopCase
    c = DopCase("N513")
    p = c.base | c.inst[1]
    eq = make_model(p)
    try:
        one = eq.integrate_dop853(c.y0[1], (0.0, c.t1), c.h0, RTOL, ATOL)
        grid = eq.integrate_dop853_grid(c.y0[1], (0.0, c.t1), c.h0, RTOL, ATOL)
    finally:
        eq.close()
    assert counts(grid) == counts(one) and list(grid.n_events) == list(one.n_events) == [0, 0, 0, 0, 0, 1, 0]
    droot = abs(grid.t_events[5][0] - one.t_events[5][0]) / c.t1
    between = rel_to_max(grid.y_final, one.y_final)
    print(f"DOP853 grid golden N=200: final {err:.2e} frames {worst_frame:.2e}; N=513 against the one-workgroup path: final {between:.2e} "
          f"root |dt|/t1 {droot:.2e} attempts {one.n_accepted + one.n_rejected}")
    assert err <= STATE_TOL and worst_frame <= STATE_TOL


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. edges
# ---------------------------------------------------------------------------------------------------------------------------------
def test_edges_of_the_entries(torch_cuda, oracle):
    import ctypes as C

    from marlpde_amd._abi import MarlError, MarlStats
    from marlpde_amd.domain import HipSlabEngine
    p, y, dx2, _ = _reference(oracle, "A", 1025, 40, False, 0.05)
    t1, h0 = 40 * dx2, 0.5 * dx2
    eq = make_model(p)
    try:
        # t0 == t1: no step, one evaluation counted, the sample at t0 is y0
        res = eq.integrate_dop853_grid(y, (0.5, 0.5), h0, RTOL, ATOL, t_eval=np.array([0.5]))
        assert counts(res) == (0, 0, 0, 1) and np.array_equal(res.y[:, 0], y) and np.array_equal(res.y_final, y)
        dev, got = _run_device(torch_cuda, eq, y, (0.5, 0.5), h0, 0)
        assert counts(dev) == (0, 0, 0, 1) and np.array_equal(got, y)
        with pytest.raises(MarlError, match=r"dop853: `first_step` exceeds bounds"):
            eq.integrate_dop853_grid(y, (0.0, t1), 2 * t1, RTOL, ATOL)
        with pytest.raises(MarlError, match=r"dop853: need first_step > 0"):
            eq.integrate_dop853_grid(y, (0.0, t1), 0.0, RTOL, ATOL)
        with pytest.raises(MarlError, match=r"dop853: `t_eval` must be sorted"):
            eq.integrate_dop853_grid(y, (0.0, t1), h0, RTOL, ATOL, t_eval=np.array([0.5 * t1, 0.25 * t1]))
        with pytest.raises(MarlError, match=r"dop853: tolerances must be positive"):
            eq.integrate_dop853_grid(y, (0.0, t1), h0, 0.0, ATOL)
        yd = torch_cuda.from_numpy(y).cuda()
        with pytest.raises(MarlError, match=r"dop853: `first_step` exceeds bounds"):
            eq.integrate_dop853_grid_device(yd.data_ptr(), (0.0, t1), 2 * t1, RTOL, ATOL, 0)
        torch_cuda.cuda.synchronize()
        assert np.array_equal(yd.cpu().numpy(), y)
    finally:
        eq.close()
    # more than one instance: refused before the state is touched
    two = make_model(p, [{}, {}])
    try:
        yd = torch_cuda.from_numpy(np.stack([y, y])).cuda()
        with pytest.raises(MarlError, match=r"rc=-1.*marl_integrate_dop853_grid_dev: single-instance context required"):
            two.integrate_dop853_grid_device(yd.data_ptr(), (0.0, t1), h0, RTOL, ATOL, 0)
        with pytest.raises(MarlError, match=r"rc=-1.*marl_integrate_dop853_grid: single-instance context required"):
            two.integrate_dop853_grid(np.stack([y, y]), (0.0, t1), h0, RTOL, ATOL)
        torch_cuda.cuda.synchronize()
        assert np.array_equal(yd.cpu().numpy(), np.stack([y, y]))
    finally:
        two.close()
    # a slab context (domain decomposition)
    slab = HipSlabEngine(p, 1025, 0, 600, 0)
    ys = torch_cuda.full((5 * 1025,), 0.25, dtype=torch_cuda.float64, device="cuda")
    host = np.full(5 * 1025, 0.25)
    stats = MarlStats()
    rc_dev = slab.lib.marl_integrate_dop853_grid_dev(slab.ctx, C.c_void_p(ys.data_ptr()), 0, 0.0, t1, h0, RTOL, ATOL, 0, C.byref(stats))
    msg_dev = slab.lib.marl_last_error(slab.ctx).decode()
    rc_host = slab.lib.marl_integrate_dop853_grid(slab.ctx, host.ctypes.data_as(C.c_void_p), 0.0, t1, h0, RTOL, ATOL, None, 0, None, None, 0, 0,
                                                  C.byref(stats))
    msg_host = slab.lib.marl_last_error(slab.ctx).decode()
    torch_cuda.cuda.synchronize()
    slab.close()
    assert rc_dev == rc_host == -1 and np.all(host == 0.25) and bool((ys == 0.25).all().item())
    assert "dop853: slab contexts (domain decomposition) are not supported" in msg_dev and msg_dev == msg_host


def test_integrate_equations_with_native_grid(oracle, monkeypatch):
    from dataclasses import asdict

    import scipy.integrate

    from marlpde_amd.Evolve_scenario import integrate_equations
    from marlpde_amd.parameters import Solver
    p, _, dx2, _ = _reference(oracle, "A", 1025, 40, False, 0.05)
    t1, h0 = 40 * dx2, 0.5 * dx2

    def no_scipy(*a, **kw):
        raise AssertionError("solve_ivp was called")
    monkeypatch.setattr(scipy.integrate, "solve_ivp", no_scipy)
    solver = asdict(Solver(method="DOP853")) | {"t_span": (0.0, t1), "first_step": h0, "rtol": RTOL, "atol": ATOL, "native_grid": True}
    last, covered, *_ = integrate_equations(solver, {}, p, results_root=None, verbose=False)
    eq = make_model(p)
    try:
        y0 = eq.get_state(p["CAIni"], p["CCIni"], p["cCaIni"], p["cCO3Ini"], p["PhiIni"]).ravel()
        res = eq.integrate_dop853_grid(y0, (0.0, t1), h0, RTOL, ATOL)
    finally:
        eq.close()
    assert res.status == 0 and covered == p["Tstar"] * t1 and np.array_equal(last.ravel(), res.y_final)
