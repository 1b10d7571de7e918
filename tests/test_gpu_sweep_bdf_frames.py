"""BDF sweeps with t_eval (marl_sweep_bdf_eval_dev): the time series that solve_ivp(method="BDF", t_eval=) fills, written inside the
batched sweep by the accepted step's dense output (A_SAMPLE in csrc/marl_bdf_ctl.h, sample_batch_kernel in csrc/marl_bdf_batch.h) -
against the same sweep without samples, against single integrate_bdf(..., t_eval=) runs, and against itself.  Scenarios, first step and
tolerances are those of tests/test_gpu_sweep_bdf.py; so is the acceptance rule against single runs (at most ONE instance per test may
leave the single run's decisions and is then held to rtol = 0.1, atol = 0.01 only).

t_eval = {0} u geomspace(1e-6, 1e-2, 9) u linspace(0.02, t1, 25): early steps without a sample, late steps with several, a sample at
t0, one at t1 and one at the nominal end of the first step.  Frame buffers start as a sentinel.  The measured deviations from the
single runs are in test_frames_against_single_runs' docstring."""
import numpy as np
import pytest

from test_gpu_sweep_bdf import ATOL, FIRST, RTOL, S, base_of, counts, rule_R, single, stats_of

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
TRIO = [S[0], S[6], S[1]]
_SINGLES, _SWEEPS = {}, {}


def t_eval_of(t1):
    return np.concatenate([[0.0], np.geomspace(1e-6, 1e-2, 9), np.linspace(0.02, t1, 25)])


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected without a HIP device")
    return torch


def single_frames(N, d, t1, t_eval, max_attempts=0):
    """The single integrate_bdf(..., t_eval=) run of scenario d (computed once per configuration, never modified)."""
    from marlpde_amd.LHeureux_model import LMAHeureuxPorosityDiff
    from marlpde_amd.sweep import initial_states
    key = (N, tuple(sorted(d.items())), t1, t_eval.tobytes(), max_attempts)
    if key not in _SINGLES:
        base = base_of(N)
        one = LMAHeureuxPorosityDiff.from_scenario(base | d, device=0)
        _SINGLES[key] = one.integrate_bdf(initial_states(base, [d])[0], (0.0, t1), FIRST, RTOL, ATOL, t_eval=t_eval, max_attempts=max_attempts)
        one.close()
    return _SINGLES[key]


def sweep(torch, N, inst, t_span, t_eval=None, max_attempts=0, eq=None):
    """(final states, results, frames [B][n_eval][5N] or None) of one sweep over `inst`; the frames start as SENTINEL."""
    from marlpde_amd.LHeureux_model import LMAHeureuxPorosityDiff
    from marlpde_amd.sweep import initial_states
    base = base_of(N)
    own = eq is None
    if own:
        eq = LMAHeureuxPorosityDiff.from_scenario(base, device=0, instances=inst)
        eq.use_stream(torch.cuda.current_stream().cuda_stream)
    yd = torch.from_numpy(initial_states(base, inst)).cuda()
    try:
        if t_eval is None:
            res = eq.sweep_bdf_device(yd.data_ptr(), t_span, FIRST, RTOL, ATOL, max_attempts)
            return yd.cpu().numpy(), res, None
        frames = torch.full((len(inst), len(t_eval), 5 * N), SENTINEL, dtype=yd.dtype, device=yd.device)
        res = eq.sweep_bdf_device(yd.data_ptr(), t_span, FIRST, RTOL, ATOL, max_attempts, t_eval=t_eval, y_eval_dev_ptr=frames.data_ptr())
        return yd.cpu().numpy(), res, frames.cpu().numpy()
    finally:
        if own:
            eq.close()


def trio_sweep(torch, t1=0.5, sampled=True):
    """The N = 64 sweep of TRIO to t1 with t_eval_of(t1) or without samples (computed once, never modified)."""
    key = (t1, sampled)
    if key not in _SWEEPS:
        _SWEEPS[key] = sweep(torch, 64, TRIO, (0.0, t1), t_eval_of(t1) if sampled else None)
    return _SWEEPS[key]


def test_frames_do_not_disturb_the_sweep(torch_cuda):
    te = t_eval_of(0.5)
    yp, rp, _ = trio_sweep(torch_cuda, sampled=False)
    yf, rf, frames = trio_sweep(torch_cuda)
    assert np.array_equal(yp, yf)
    for b in range(3):
        err = float(np.max(np.abs(frames[b, -1] - yf[b])))
        print(f"frames[{b}]: {stats_of(rf[b])[:7]}  max |frame(t1) - y_final| = {err:.3e}")
        assert stats_of(rp[b]) == stats_of(rf[b]), b
        assert rf[b].status == 0 and len(rf[b].t) == len(te) and np.array_equal(rf[b].t, te)
        assert not np.any(frames[b] == SENTINEL)
        # D[0] of the last step and y_new are the same sum of at most 7 terms of O(1) data in another order
        assert err <= 1e-12, b
    rule_R("N64 frames", yf, rf, [single(64, d, 0.5) for d in TRIO])   # (the states of tests that hold the cap of one loose instance)


@pytest.mark.parametrize("N,which,t1", [(200, [0, 1, 2, 3, 4, 5], 0.5), (33, [0, 4], 0.5), (409, [0, 2, 4], 0.1)])
def test_frames_against_single_runs(torch_cuda, N, which, t1):
    """Strict instances (the single run's nfev, njev, nlu and accepted steps): n_frames equal, frames within 1e-4, rule_R's bound on the
    same pairs of states.  Measured on an MI355X, largest |sweep - single| over the 35 frames of each instance (all strict):
    N = 200: 1.9e-07, 1.2e-08, 9.9e-06, 1.2e-08, 3.8e-06, 7.9e-09;  N = 33: 7.3e-09, 9.3e-08;  N = 409: 5.4e-08, 3.1e-07, 5.4e-07
    - the size of the differences between the final states of the same pairs (tests/test_gpu_sweep_bdf.py), and not below 1e-8 on
    every strict instance, so the bound stays at 1e-4."""
    inst = [S[k] for k in which]
    te = t_eval_of(t1)
    got, res, frames = sweep(torch_cuda, N, inst, (0.0, t1), te)
    loose = 0
    for b, (d, r) in enumerate(zip(inst, res)):
        ref = single_frames(N, d, t1, te)
        k = min(len(r.t), len(ref.t))
        dev = float(np.max(np.abs(frames[b, :k] - ref.y.T[:k])))
        strict = counts(r) == counts(ref)
        print(f"N{N}[{b}]: sweep {counts(r)} single {counts(ref)} frames {len(r.t)} / {len(ref.t)}  max |sweep - single| over frames = {dev:.3e}"
              f"  ({'strict' if strict else 'loose'})")
        assert r.status == ref.status == 0 and len(ref.t) == len(te)
        if strict:
            assert len(r.t) == len(ref.t) and np.array_equal(r.t, ref.t)
            assert dev <= 1e-4
        else:
            loose += 1
            np.testing.assert_allclose(frames[b, :k], ref.y.T[:k], rtol=0.1, atol=0.01)
        assert not np.any(frames[b, :len(r.t)] == SENTINEL)
    assert loose <= 1, f"N{N}: {loose} instances left the single runs' decisions"


def test_sample_indexing(torch_cuda):
    te = t_eval_of(0.5)
    extra = np.array([3e-7, 2e-6, 5e-5, 7e-4, 0.015, 0.033, 0.101, 0.2501, 0.377, 0.4999])
    more = np.sort(np.concatenate([te, extra]))
    assert more.size == te.size + 10 and np.all(np.diff(more) > 0)
    y, res, frames = trio_sweep(torch_cuda)
    y2, res2, frames2 = sweep(torch_cuda, 64, TRIO, (0.0, 0.5), more)
    common = np.searchsorted(more, te)
    assert np.array_equal(more[common], te)
    assert np.array_equal(y, y2) and [stats_of(r) for r in res] == [stats_of(r) for r in res2]
    assert all(len(r.t) == more.size for r in res2) and not np.any(frames2 == SENTINEL)
    assert np.array_equal(frames2[:, common], frames)


def test_instances_do_not_see_each_other(torch_cuda):
    te = t_eval_of(0.5)
    y, res, frames = sweep(torch_cuda, 64, TRIO * 4, (0.0, 0.5), te)
    for k in range(3):
        for rep in range(1, 4):
            assert np.array_equal(frames[k], frames[k + 3 * rep]) and np.array_equal(y[k], y[k + 3 * rep]), (k, rep)
    alone_y, alone_res, alone_frames = sweep(torch_cuda, 64, [S[6]], (0.0, 0.5), te)
    assert np.array_equal(alone_frames[0], frames[1]) and stats_of(alone_res[0]) == stats_of(res[1])
    _, _, trio_frames = trio_sweep(torch_cuda)
    assert np.array_equal(trio_frames, frames[:3])
    assert not np.array_equal(frames[0], frames[1])


def test_how_a_run_ends(torch_cuda):
    from marlpde_amd._abi import MarlError
    from marlpde_amd.LHeureux_model import LMAHeureuxPorosityDiff
    from marlpde_amd.sweep import initial_states
    te = t_eval_of(0.5)
    got, res, frames = sweep(torch_cuda, 64, TRIO, (0.0, 0.5), te, max_attempts=25)
    plain, resp, _ = sweep(torch_cuda, 64, TRIO, (0.0, 0.5), max_attempts=25)
    assert np.array_equal(got, plain)
    for b, r in enumerate(res):
        k = int(np.searchsorted(te, r.t_reached, side="right"))
        print(f"budget[{b}]: {stats_of(r)[:7]} frames {len(r.t)}")
        assert r.status == 2 and r.t_reached < 0.5 and stats_of(r) == stats_of(resp[b])
        assert len(r.t) == k and 0 < k < len(te)
        assert not np.any(frames[b, :k] == SENTINEL) and np.all(frames[b, k:] == SENTINEL)
    # t0 == t1: no step, no frame (as integrate_bdf writes none)
    base = base_of(64)
    y0 = initial_states(base, TRIO)
    got0, res0, frames0 = sweep(torch_cuda, 64, TRIO, (0.0, 0.0), np.array([0.0]))
    assert np.array_equal(got0, y0) and all(len(r.t) == 0 and r.status == 0 and r.n_accepted == 0 for r in res0)
    assert np.all(frames0 == SENTINEL)
    # t_eval unsorted or outside t_span: an error before anything runs
    eq = LMAHeureuxPorosityDiff.from_scenario(base, device=0, instances=TRIO)
    eq.use_stream(torch_cuda.cuda.current_stream().cuda_stream)
    try:
        yd = torch_cuda.from_numpy(y0).cuda()
        fr = torch_cuda.full((3, 3, 5 * 64), SENTINEL, dtype=yd.dtype, device=yd.device)
        for bad in ([0.0, 0.3, 0.2], [0.0, 0.2, 0.2], [0.1, 0.2, 0.6], [-0.1, 0.2, 0.3]):
            with pytest.raises(MarlError, match="t_eval"):
                eq.sweep_bdf_device(yd.data_ptr(), (0.0, 0.5), FIRST, RTOL, ATOL, t_eval=bad, y_eval_dev_ptr=fr.data_ptr())
            assert np.array_equal(yd.cpu().numpy(), y0) and np.all(fr.cpu().numpy() == SENTINEL)
        with pytest.raises(ValueError, match="y_eval_dev_ptr"):
            eq.sweep_bdf_device(yd.data_ptr(), (0.0, 0.5), FIRST, RTOL, ATOL, t_eval=[0.0, 0.1])
        again = sweep(torch_cuda, 64, TRIO, (0.0, 0.5), te, eq=eq)   # the context stays usable
    finally:
        eq.close()
    want = trio_sweep(torch_cuda)
    assert np.array_equal(again[0], want[0]) and np.array_equal(again[2], want[2])


def test_list_lengths_by_copy_or_by_polled_host_memory(torch_cuda):
    from marlpde_amd.LHeureux_model import LMAHeureuxPorosityDiff
    te = t_eval_of(0.3)
    out = {}
    for zc in (0, 1):
        eq = LMAHeureuxPorosityDiff.from_scenario(base_of(64), device=0, instances=TRIO)
        eq.use_stream(torch_cuda.cuda.current_stream().cuda_stream)
        eq.set_option("implicit_zero_copy", zc)
        try:
            out[zc] = sweep(torch_cuda, 64, TRIO, (0.0, 0.3), te, eq=eq)
        finally:
            eq.close()
    assert all(r.status == 0 and len(r.t) == len(te) for r in out[1][1])
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][2], out[1][2])
    assert [stats_of(r) for r in out[0][1]] == [stats_of(r) for r in out[1][1]]
    assert not np.any(out[1][2] == SENTINEL)


def test_drivers(torch_cuda):
    from marlpde_amd.sweep import HipSweepEngine, initial_states, run_sweep_bdf
    N, inst, t1 = 64, [S[0], S[1], S[3], S[5]], 0.5
    base, te = base_of(N), t_eval_of(0.5)
    y0 = initial_states(base, inst)
    y, status, acc, rej, t, n_frames, y_eval = run_sweep_bdf(base, inst, (0.0, t1), FIRST, RTOL, ATOL, batched=True, t_eval=te, device=0)
    eng = HipSweepEngine(base, inst, 0)
    yb, resb = eng.integrate_bdf(y0, (0.0, t1), FIRST, RTOL, ATOL, 0, batched=True, t_eval=te)
    eng.close()
    assert np.array_equal(y, yb) and list(n_frames) == [len(r.t) for r in resb] == [len(te)] * len(inst)
    assert y_eval.shape == (len(inst), len(te), 5 * N)
    for b, r in enumerate(resb):
        assert np.array_equal(r.t, te) and r.y.shape == (5 * N, len(te)) and np.array_equal(y_eval[b], r.y.T)
        assert (status[b], acc[b], rej[b], t[b]) == (r.status, r.n_accepted, r.n_rejected, r.t_reached)
    # unbatched: every instance IS the single run, its frames included
    yu, _, _, _, _, nu, fu = run_sweep_bdf(base, inst, (0.0, t1), FIRST, RTOL, ATOL, t_eval=te, device=0)
    for b, d in enumerate(inst):
        ref = single_frames(N, d, t1, te)
        assert nu[b] == len(ref.t) == len(te) and np.array_equal(fu[b], ref.y.T) and np.array_equal(yu[b], ref.y_final)
        print(f"driver[{b}]: max |batched - unbatched| over frames = {float(np.max(np.abs(y_eval[b] - fu[b]))):.3e}")
