"""Radau sweeps with t_eval (marl_sweep_radau_eval_dev): the time series that solve_ivp(..., t_eval=) fills with the reference's default
solver (marlpde/Evolve_scenario.py:104-109), written inside the sweep by the accepted step's dense output - one A_FRAME action per
sample, after the step's roots (PC_FRAMES in radau_control_step), through frame_eval_batch_kernel on the launch path and through the
A_FRAME block of radau_wg_kernel on the workgroup paths.  Samples never change the steps (ivp.py:706-723): every test here compares a
run with frames against the same run without."""
import ctypes as C
from dataclasses import asdict

import numpy as np
import pytest

from common import GOLDEN

pytestmark = pytest.mark.gpu

H0, RTOL, ATOL = 1e-6, 1e-3, 1e-3
SCENARIO_A = {"Phi0": 0.6, "PhiIni": 0.5, "PhiNR": 0.6}
MATLAB = {"Phi0": 0.5, "PhiIni": 0.5, "PhiNR": 0.5, "k3": 0.01, "k4": 0.01}
# the four instances of test_gpu_radau.py::test_radau_sweep_workgroup_paths_against_the_launch_path, then the high-porosity default
# scenario (123 accepted and 63 rejected steps to t = 0.3 at N = 64, roots of four monitors)
INSTANCES = [SCENARIO_A, MATLAB, {"Phi0": 0.6, "PhiIni": 0.6, "PhiNR": 0.6}, {"Phi0": 0.65, "PhiIni": 0.5, "PhiNR": 0.5, "k3": 0.05, "k4": 0.05}, {}]
N_SMALL, T1_SMALL = 64, 0.3
T_EVAL_SMALL = np.linspace(0.0, T1_SMALL, 11)
MODES = (0, 1, 2, 3)


@pytest.fixture(scope="module")
def torch_cuda_radau():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _base(N):
    from marlpde_amd.parameters import Map_Scenario
    return asdict(Map_Scenario()) | {"N": N}


def _y0(base, inst):
    N = int(base["N"])
    return np.stack([np.concatenate([np.full(N, (base | d)[k]) for k in ("CAIni", "CCIni", "cCaIni", "cCO3Ini", "PhiIni")]) for d in inst])


def _model(torch, base, inst, wg=None):
    from marlpde_amd.LHeureux_model import LMAHeureuxPorosityDiff
    eq = LMAHeureuxPorosityDiff.from_scenario(base, device=0, instances=inst)
    eq.use_stream(torch.cuda.current_stream().cuda_stream)
    if wg is not None:
        eq.set_option("radau_sweep_wg", wg)
    return eq


def _sweep(torch, eq, y0, t_span, t_eval=None, fill=np.nan, **kw):
    """One sweep through the model's entry -> (final states, results, frames [B][n_eval][5N] or None); frames start as `fill`."""
    yd = torch.from_numpy(y0).cuda()
    if t_eval is None:
        res = eq.sweep_radau_device(yd.data_ptr(), t_span, H0, RTOL, ATOL, **kw)
        return yd.cpu().numpy(), res, None
    frames = torch.full((y0.shape[0], len(t_eval), y0.shape[1]), fill, dtype=yd.dtype, device=yd.device)
    res = eq.sweep_radau_device(yd.data_ptr(), t_span, H0, RTOL, ATOL, t_eval=t_eval, y_eval_dev_ptr=frames.data_ptr(), **kw)
    return yd.cpu().numpy(), res, frames.cpu().numpy()


def _key(r):
    return (r.status, r.nfev, r.njev, r.nlu, r.n_accepted, r.n_rejected, list(r.n_events), r.t_reached)


def _same_roots(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a.t_events, b.t_events))


@pytest.fixture(scope="module")
def small(torch_cuda_radau):
    """N = 64 to t = 0.3 in every path, with frames and without (events located in both): {mode: {with_frames: (y, res, frames)}}."""
    torch = torch_cuda_radau
    base = _base(N_SMALL)
    y0 = _y0(base, INSTANCES)
    out = {}
    for wg in MODES:
        eq = _model(torch, base, INSTANCES, wg)
        out[wg] = {te is not None: _sweep(torch, eq, y0, (0.0, T1_SMALL), te, events=True, max_events=64) for te in (None, T_EVAL_SMALL)}
        eq.close()
    return y0, out


@pytest.mark.parametrize("wg", MODES)
def test_frames_do_not_disturb_the_sweep(small, wg):
    y0, out = small
    (yp, rp, _), (yf, rf, frames) = out[wg][False], out[wg][True]
    assert np.array_equal(yp, yf)
    for b in range(len(INSTANCES)):
        print(wg, b, _key(rf[b]), [len(t) for t in rf[b].t_events], float(np.max(np.abs(frames[b, -1] - yf[b]))))
        assert _key(rp[b]) == _key(rf[b]), (wg, b)
        assert _same_roots(rp[b], rf[b]), (wg, b)
        assert rf[b].status == 0 and len(rf[b].t) == 11 and np.array_equal(rf[b].t, T_EVAL_SMALL)      # n_done == 11
        assert np.array_equal(frames[b, 0], y0[b])                      # the dense output at x = 0 is y_old exactly
        # Q (1, 1, 1) = Z_3 up to the rounding of three-term sums with |P| <= 26 on O(1) data (~1e-14)
        assert np.max(np.abs(frames[b, -1] - yf[b])) <= 1e-12, (wg, b)
    assert sum(len(t) > 0 for t in rf[4].t_events) >= 4                 # the high-porosity scenario: roots of four monitors, frames after them


def test_frames_of_the_paths_against_each_other(small):
    _, out = small
    f = {wg: out[wg][True][2][:4] for wg in MODES}
    print("launch path against hybrid", float(np.max(np.abs(f[0] - f[1]))))
    assert np.array_equal(f[3], f[1])                  # the Jacobian in the workgroup too: bit-identical
    assert np.max(np.abs(f[0] - f[1])) <= 1e-12        # the bound test_radau_sweep_workgroup_paths_against_the_launch_path puts on these paths' states
    assert np.array_equal(f[2], f[1])                  # with frames the all-in-workgroup mode takes the hybrid path


def test_launch_path_above_the_one_workgroup_limit(torch_cuda_radau):
    """N = 450 (5 N > PCR_FUSED_MAX): frame_eval_batch_kernel over L_FRAME whatever radau_sweep_wg says; twelve attempts."""
    torch = torch_cuda_radau
    base, inst = _base(450), [SCENARIO_A, MATLAB]
    y0 = _y0(base, inst)
    eq = _model(torch, base, inst)
    yp, rp, _ = _sweep(torch, eq, y0, (0.0, 1.0), max_attempts=12)
    t_a = min(r.t_reached for r in rp)
    t_eval = np.array([0.0, 0.5 * t_a, t_a, 0.5])
    assert 0 < t_a < 0.5
    SENTINEL = -7.25
    yf, rf, frames = _sweep(torch, eq, y0, (0.0, 1.0), t_eval, fill=SENTINEL, max_attempts=12)
    eq.close()
    assert np.array_equal(yp, yf)
    for b in range(2):
        assert rf[b].status == 2 and _key(rp[b]) == _key(rf[b])
        k = len(rf[b].t)
        assert (k == 3) if rp[b].t_reached == t_a else (k >= 3), (b, k)
        assert np.array_equal(frames[b, 0], y0[b]) and np.all(frames[b, :k] != SENTINEL) and np.all(frames[b, k:] == SENTINEL)
        if rp[b].t_reached == t_a:
            assert np.max(np.abs(frames[b, 2] - yf[b])) <= 1e-12


def test_frames_against_the_single_run_and_the_reference(torch_cuda_radau):
    torch = torch_cuda_radau
    from marlpde_amd.LHeureux_model import LMAHeureuxPorosityDiff
    N = 200
    base, inst = _base(N), [SCENARIO_A, MATLAB]
    y0 = _y0(base, inst)
    t_eval = np.array([0.0, 0.1, 0.25, 0.5, 1.0])
    eq = _model(torch, base, inst)
    _, res, frames = _sweep(torch, eq, y0, (0.0, 1.0), t_eval)
    eq.close()
    for b, d in enumerate(inst):
        one = LMAHeureuxPorosityDiff.from_scenario(base | d, device=0)
        ref = one.integrate_radau(y0[b], (0.0, 1.0), H0, RTOL, ATOL, t_eval=t_eval)
        one.close()
        assert res[b].status == 0 == ref.status and len(res[b].t) == 5
        assert (res[b].nfev, res[b].njev, res[b].nlu, res[b].n_accepted) == (ref.nfev, ref.njev, ref.nlu, ref.n_accepted)
        err = float(np.max(np.abs(frames[b] - ref.y.T)))
        print(b, "sweep frames against the single run's", err)
        # the bound test_radau_sweep_equals_instance_by_instance puts on the final states of these two controllers (observed 1.9e-5)
        assert err <= 1e-4
    gold = np.load(f"{GOLDEN}/ref_frames_scenarioA_t0.1_0.25_0.5.npy")   # (3, 5, 200): the reference's stored frames
    for i in range(3):
        np.testing.assert_allclose(frames[0, 1 + i].reshape(5, N), gold[i], rtol=0.1, atol=0.01)


def test_engine_and_driver_return_the_time_series_and_the_roots(torch_cuda_radau, small):
    from marlpde_amd.sweep import HipSweepEngine, run_sweep_radau
    y0, out = small
    _, r3, f3 = out[3][True]                  # the default path's direct call
    base, inst, pick = _base(N_SMALL), INSTANCES[:3], [0, 2, 5, 8, 10]
    t_eval = T_EVAL_SMALL[pick]
    got = run_sweep_radau(base, inst, (0.0, T1_SMALL), H0, RTOL, ATOL, device=0, t_eval=t_eval, events=True)
    assert len(got) == 8
    y, status, acc, rej, t, n_frames, y_eval, roots = got
    assert list(status) == [0] * 3 and list(n_frames) == [5] * 3 and y_eval.shape == (3, 5, 5 * N_SMALL)
    assert np.array_equal(y, out[3][True][0][:3]) and list(acc) == [r.n_accepted for r in r3[:3]]
    assert np.array_equal(y_eval, f3[:3][:, pick])
    for b in range(3):
        assert len(roots[b]) == 7 and all(np.array_equal(a, w) for a, w in zip(roots[b], r3[b].t_events))
    eng = HipSweepEngine(base, inst, 0)
    try:
        ye, res = eng.integrate_radau(y0[:3], (0.0, T1_SMALL), H0, RTOL, ATOL, 0, t_eval=t_eval, events=True)
        y00, res00 = eng.integrate_radau(y0[:3], (0.0, 0.0), H0, RTOL, ATOL, 0, t_eval=np.array([0.0]), events=True)
    finally:
        eng.close()
    assert np.array_equal(ye, y)
    for b in range(3):
        assert res[b].y.shape == (5 * N_SMALL, 5) and np.array_equal(res[b].y.T, y_eval[b])
        # t1 == t0: no step; the sample at t0 is y0, and there are no roots
        assert res00[b].status == 0 and res00[b].n_accepted == 0 and list(res00[b].t) == [0.0]
        assert np.array_equal(res00[b].y[:, 0], y0[b]) and all(len(t) == 0 for t in res00[b].t_events)
    assert np.array_equal(y00, y0[:3])


def test_argument_errors_leave_the_context_usable(torch_cuda_radau):
    from marlpde_amd._abi import MarlError, MarlStats
    torch = torch_cuda_radau
    base, inst = _base(N_SMALL), INSTANCES[:2]
    y0 = _y0(base, inst)
    eq = _model(torch, base, inst)
    t1 = 0.01
    for bad in ([0.5 * t1, 0.25 * t1], [0.5 * t1, 0.5 * t1], [-1e-9, 0.5 * t1], [0.5 * t1, 1.0000001 * t1], [float("nan")]):
        with pytest.raises(MarlError, match="`t_eval` must be sorted and within t_span"):      # scipy's message (ivp.py:603-609)
            _sweep(torch, eq, y0, (0.0, t1), np.array(bad))
    # samples without a place for the frames
    yd = torch.from_numpy(y0).cuda()
    te = np.array([0.0, t1])
    n_done = np.zeros(2, dtype=np.int64)
    stats = (MarlStats * 2)()
    rc = eq._lib.marl_sweep_radau_eval_dev(eq._ctx, C.c_void_p(yd.data_ptr()), 0.0, t1, H0, RTOL, ATOL, None, 0, te.ctypes.data_as(C.c_void_p), 2, None,
                                           n_done.ctypes.data_as(C.c_void_p), None, 0, stats)
    assert rc < 0 and b"invalid argument" in eq._lib.marl_last_error(eq._ctx)
    assert np.array_equal(yd.cpu().numpy(), y0)
    # the context still works: the same numbers as a fresh one
    y, res, frames = _sweep(torch, eq, y0, (0.0, t1), te)
    eq.close()
    eq = _model(torch, base, inst)
    y2, res2, frames2 = _sweep(torch, eq, y0, (0.0, t1), te)
    eq.close()
    assert all(r.status == 0 and len(r.t) == 2 for r in res) and [_key(r) for r in res] == [_key(r) for r in res2]
    assert np.array_equal(y, y2) and np.array_equal(frames, frames2) and np.array_equal(frames[:, 0], y0)
