"""BDF sweeps with events (marl_sweep_bdf_events_dev): the root times of the reference's seven monitors, located inside the batched
sweep on the accepted step's dense output (A_ROOTS in csrc/marl_bdf_ctl.h; roots_batch_kernel in csrc/marl_bdf_batch.h runs the whole
Brent search of a step's monitors in one launch) - against the same sweep without roots, against single integrate_bdf runs (whose
`events` default is on), against the monitors of the sweep's own dense output around every root, and against itself.  Scenarios,
first step and tolerances are those of tests/test_gpu_sweep_bdf.py; so is the cap of at most ONE loose instance per test against
single runs.  The measured deviations from the single runs are in test_roots_against_single_runs' docstring."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_sweep_bdf import ATOL, FIRST, RTOL, S, base_of, counts, single, stats_of
from test_gpu_sweep_bdf_frames import SENTINEL, t_eval_of

pytestmark = pytest.mark.gpu

TRIO = [S[0], S[6], S[1]]       # S1 has no sign change
_SWEEPS = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected without a HIP device")
    return torch


def model(torch, N, inst):
    from marlpde_amd.LHeureux_model import LMAHeureuxPorosityDiff
    eq = LMAHeureuxPorosityDiff.from_scenario(base_of(N), device=0, instances=inst)
    eq.use_stream(torch.cuda.current_stream().cuda_stream)
    return eq


def sweep(torch, N, inst, t_span, t_eval=None, max_attempts=0, eq=None, **more):
    """(final states, results, frames [B][n_eval][5N] or None) of one sweep over `inst`; more: events / max_events, passed only when given."""
    from marlpde_amd.sweep import initial_states
    own = eq is None
    if own:
        eq = model(torch, N, inst)
    yd = torch.from_numpy(initial_states(base_of(N), inst)).cuda()
    try:
        if t_eval is None:
            res = eq.sweep_bdf_device(yd.data_ptr(), t_span, FIRST, RTOL, ATOL, max_attempts, **more)
            return yd.cpu().numpy(), res, None
        frames = torch.full((len(inst), len(t_eval), 5 * N), SENTINEL, dtype=yd.dtype, device=yd.device)
        res = eq.sweep_bdf_device(yd.data_ptr(), t_span, FIRST, RTOL, ATOL, max_attempts, t_eval=t_eval, y_eval_dev_ptr=frames.data_ptr(), **more)
        return yd.cpu().numpy(), res, frames.cpu().numpy()
    finally:
        if own:
            eq.close()


def cached(torch, N, which, t1, events=True):
    """The sweep of the scenarios `which` (indices into S) on N cells to t1, with or without roots (computed once, never modified)."""
    key = (N, tuple(which), t1, events)
    if key not in _SWEEPS:
        _SWEEPS[key] = sweep(torch, N, [S[i] for i in which], (0.0, t1), **({"events": True} if events else {}))
    return _SWEEPS[key]


def consistent(r, t1, max_events=64):
    """what every located set of roots satisfies on its own: as many as sign changes, finite, non-decreasing, inside (0, t1]"""
    assert len(r.t_events) == 7
    for e in range(7):
        t = r.t_events[e]
        assert len(t) == min(int(r.n_events[e]), max_events), (e, len(t), r.n_events[e])
        assert np.all(np.isfinite(t)) and np.all(np.diff(t) >= 0) and np.all(t > 0) and np.all(t <= t1), (e, t)


def same_roots(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a.t_events, b.t_events))


def test_locating_roots_leaves_the_integration_alone(torch_cuda):
    which, t1 = [0, 6, 1], 0.5
    yp, rp, _ = cached(torch_cuda, 64, which, t1, events=False)
    ye, re_, _ = cached(torch_cuda, 64, which, t1)
    assert np.array_equal(yp, ye)
    for b in range(3):
        print(f"roots[{b}]: {stats_of(re_[b])[:7]} n_events {list(re_[b].n_events)} first roots {[list(t[:2]) for t in re_[b].t_events[:2]]}")
        assert stats_of(rp[b]) == stats_of(re_[b]), b
        assert rp[b].t_events is None
        consistent(re_[b], t1)
    assert sum(re_[0].n_events) > 0 and sum(re_[1].n_events) > sum(re_[0].n_events)
    assert not any(re_[2].n_events) and all(len(t) == 0 for t in re_[2].t_events)   # the instance without sign changes has none
    te = t_eval_of(t1)
    yf, rf, ff = sweep(torch_cuda, 64, TRIO, (0.0, t1), te)
    yb, rb, fb = sweep(torch_cuda, 64, TRIO, (0.0, t1), te, events=True)
    assert np.array_equal(yf, yb) and np.array_equal(yb, ye) and np.array_equal(ff, fb) and not np.any(fb == SENTINEL)
    for b in range(3):
        assert stats_of(rf[b]) == stats_of(rb[b]) == stats_of(re_[b]) and np.array_equal(rb[b].t, te) and rf[b].t_events is None
        assert same_roots(rb[b], re_[b])   # the samples do not move the roots


@pytest.mark.parametrize("N,which,t1", [(200, [0, 1, 2, 3, 4, 5], 0.5), (33, [0, 4], 0.5), (409, [0, 2, 4], 0.1)])
def test_roots_against_single_runs(torch_cuda, N, which, t1):
    """Strict instances (the single run's nfev, njev, nlu and accepted steps): as many roots per monitor and |root - single's| <= 5e-4,
    the project's tolerance for these ill-conditioned roots (tests/test_gpu_radau.py).  At most one loose instance per test, held to
    the self-consistency of test_locating_roots_leaves_the_integration_alone only.
    Measured (MI355X), the largest |root - single run's| per instance (roots per monitor) - N = 200: S0 9.1e-9 ([5,5,0,0,0,0,0]),
    S1 none, S2 1.9e-4 ([3,3,6,0,0,1,0]), S3 6.7e-9 ([1,1,..]), S4 2.8e-4 ([15,15,0,0,0,2,0]), S5 9.4e-11 ([1,1,..]);
    N = 33: S0 1.9e-7 ([9,9,..]), S4 2.0e-6 ([10,10,..]); N = 409: S0 4.3e-8 ([1,3,2,..]), S2 1.3e-7 ([1,1,3,..]), S4 7.1e-8 ([5,5,..]).
    Every instance was strict, and the counts are the CPU oracle's."""
    _, res, _ = cached(torch_cuda, N, which, t1)
    loose = 0
    for b, i in enumerate(which):
        ref = single(N, S[i], t1)
        consistent(res[b], t1)
        if counts(res[b]) != counts(ref):
            loose += 1
            print(f"N{N} S{i}: loose - sweep {counts(res[b])}, single {counts(ref)}")
            continue
        assert [len(t) for t in res[b].t_events] == [len(t) for t in ref.t_events], (i, res[b].n_events)
        worst = max([float(np.max(np.abs(a - w))) for a, w in zip(res[b].t_events, ref.t_events) if len(w)], default=0.0)
        print(f"N{N} S{i}: roots per monitor {[len(t) for t in ref.t_events]}, max |root - single run's| = {worst:.3e}")
        assert worst <= 5e-4, i
    assert loose <= 1, f"N{N}: {loose} instances left the single runs' decisions"


@pytest.mark.parametrize("N,which,t1", [(64, [0, 2, 5], 0.5), (409, [0, 2], 0.1)])
def test_a_root_is_a_root(torch_cuda, N, which, t1):
    """A second sweep samples the dense output 1e-9 on either side of every located root: the monitor changes sign in between."""
    inst = [S[i] for i in which]
    _, res, _ = cached(torch_cuda, N, which, t1)
    roots = np.unique(np.concatenate([t for r in res for t in r.t_events]))
    assert roots.size >= 6
    te = np.unique(np.concatenate([roots - 1e-9, roots + 1e-9]))
    assert te[0] > 0 and te[-1] <= t1 and np.all(np.diff(te) > 0)
    eq = model(torch_cuda, N, inst)
    try:
        _, res2, frames = sweep(torch_cuda, N, inst, (0.0, t1), te, eq=eq, events=True)
        g = np.stack([eq.events_all(frames[:, k]) for k in range(len(te))], axis=1)   # [instance][sample][monitor]
    finally:
        eq.close()
    checked = 0
    for b, r in enumerate(res):
        assert same_roots(r, res2[b]) and len(res2[b].t) == len(te)
        for e in range(7):
            for root in r.t_events[e]:
                lo, hi = np.searchsorted(te, root - 1e-9), np.searchsorted(te, root + 1e-9)
                assert te[lo] == root - 1e-9 and te[hi] == root + 1e-9
                assert g[b, lo, e] * g[b, hi, e] <= 0, (which[b], e, root, g[b, lo, e], g[b, hi, e])
                checked += 1
    print(f"N{N}: {checked} roots checked at {len(te)} samples")
    assert checked >= roots.size


def test_caps_and_fallbacks(torch_cuda):
    from marlpde_amd._abi import MarlStats
    from marlpde_amd.sweep import initial_states
    N, which, t1 = 64, [0, 2, 5], 0.5
    inst = [S[i] for i in which]
    yfull, full, _ = cached(torch_cuda, N, which, t1)
    yplain, plain, _ = cached(torch_cuda, N, which, t1, events=False)
    assert all(max(r.n_events) >= 3 for r in full)
    y1, r1, _ = sweep(torch_cuda, N, inst, (0.0, t1), events=True, max_events=1)
    assert np.array_equal(y1, yfull)
    for b in range(3):
        assert stats_of(r1[b]) == stats_of(full[b])   # counts go on
        consistent(r1[b], t1, max_events=1)
        for e in range(7):
            assert np.array_equal(r1[b].t_events[e], full[b].t_events[e][:1])   # the first roots only
    te = t_eval_of(t1)
    for more in ({"events": True, "max_events": 0}, {"events": False}, {}):
        y0_, r0, _ = sweep(torch_cuda, N, inst, (0.0, t1), **more)
        _, rf, _ = sweep(torch_cuda, N, inst, (0.0, t1), te, **more)
        assert np.array_equal(y0_, yplain)
        for b in range(3):
            assert r0[b].t_events is None and rf[b].t_events is None
            assert stats_of(r0[b]) == stats_of(plain[b]) == stats_of(rf[b]) and np.array_equal(rf[b].t, te)
    # the raw C entry: the buffer is NaN beyond the first root of every monitor; t_events = NULL and max_events <= 0 locate nothing
    eq = model(torch_cuda, N, inst)
    try:
        def raw(tev, max_events):
            yd = torch_cuda.from_numpy(initial_states(base_of(N), inst)).cuda()
            stats = (MarlStats * 3)()
            rc = eq._lib.marl_sweep_bdf_events_dev(eq._ctx, C.c_void_p(yd.data_ptr()), 0.0, t1, FIRST, RTOL, ATOL, None, 0, None, 0, None, None,
                                                   None if tev is None else tev.ctypes.data_as(C.c_void_p), max_events, stats)
            assert rc == 0
            return yd.cpu().numpy(), stats
        buf = np.full((3, 7, 1), -1.0)
        yr, st = raw(buf, 1)
        assert np.array_equal(yr, yfull)
        for b in range(3):
            for e in range(7):
                assert list(st[b].n_events) == list(full[b].n_events)
                if st[b].n_events[e]:
                    assert buf[b, e, 0] == full[b].t_events[e][0]
                else:
                    assert np.isnan(buf[b, e, 0])
        wide = np.full((3, 7, 64), -1.0)
        raw(wide, 64)
        for b in range(3):
            for e in range(7):
                k = len(full[b].t_events[e])
                assert np.array_equal(wide[b, e, :k], full[b].t_events[e]) and np.isnan(wide[b, e, k:]).all()
        untouched = np.full((3, 7, 4), -1.0)
        for t_events, max_events in ((None, 0), (None, 8), (untouched, 0), (untouched, -1)):
            yr, st = raw(t_events, max_events)
            assert np.array_equal(yr, yplain) and [list(s.n_events) for s in st] == [list(r.n_events) for r in plain]
        assert np.all(untouched == -1.0)
    finally:
        eq.close()


def test_instances_do_not_see_each_other(torch_cuda):
    N, which, t1 = 64, [0, 2, 5], 0.5
    _, one, _ = cached(torch_cuda, N, which, t1)
    y12, r12, _ = sweep(torch_cuda, N, [S[i] for i in which] * 4, (0.0, t1), events=True)
    for k in range(3):
        for rep in range(4):
            assert same_roots(r12[k + 3 * rep], one[k]) and stats_of(r12[k + 3 * rep]) == stats_of(one[k]), (k, rep)
    _, rev, _ = sweep(torch_cuda, N, [S[i] for i in reversed(which)], (0.0, t1), events=True)
    for k in range(3):
        assert same_roots(rev[2 - k], one[k]), k
    for k in (1,):
        _, alone, _ = sweep(torch_cuda, N, [S[which[k]]], (0.0, t1), events=True)
        assert same_roots(alone[0], one[k])


def test_how_a_run_ends(torch_cuda):
    from marlpde_amd._abi import MarlError
    N, which, t1 = 64, [5, 6, 2], 0.5
    inst = [S[i] for i in which]
    _, full, _ = cached(torch_cuda, N, which, t1)
    eq = model(torch_cuda, N, inst)
    try:
        _, res, _ = sweep(torch_cuda, N, inst, (0.0, t1), max_attempts=60, eq=eq, events=True)
        for b, r in enumerate(res):
            got, want = sum(len(t) for t in r.t_events), sum(len(t) for t in full[b].t_events)
            print(f"budget S{which[b]}: status {r.status} t {r.t_reached:.4f}, {got} of {want} roots {[len(t) for t in r.t_events]}")
            assert r.status == 2 and r.t_reached < t1 and 0 < got < want
            consistent(r, r.t_reached)
            for e in range(7):   # the leading roots of the full run
                assert np.array_equal(r.t_events[e], full[b].t_events[e][:len(r.t_events[e])]), (b, e)
        _, res0, _ = sweep(torch_cuda, N, inst, (0.0, 0.0), eq=eq, events=True)
        for r in res0:
            assert (r.status, r.n_accepted) == (0, 0) and all(len(t) == 0 for t in r.t_events)
        with pytest.raises(MarlError):
            sweep(torch_cuda, N, inst, (0.0, t1), np.array([0.3, 0.2]), eq=eq, events=True)   # t_eval must increase
        _, again, _ = sweep(torch_cuda, N, inst, (0.0, t1), eq=eq, events=True)   # the context stays usable
        for b in range(3):
            assert same_roots(again[b], full[b]) and stats_of(again[b]) == stats_of(full[b])
    finally:
        eq.close()


def test_list_lengths_by_copy_or_by_polled_host_memory(torch_cuda):
    N, out = 64, {}
    for zc in (0, 1):
        eq = model(torch_cuda, N, TRIO)
        eq.set_option("implicit_zero_copy", zc)
        try:
            out[zc] = sweep(torch_cuda, N, TRIO, (0.0, 0.3), eq=eq, events=True)
        finally:
            eq.close()
    assert np.array_equal(out[0][0], out[1][0])
    for a, b in zip(out[0][1], out[1][1]):
        assert stats_of(a) == stats_of(b) and same_roots(a, b)
        consistent(a, 0.3)
    assert sum(out[0][1][1].n_events) > 0


def test_drivers(torch_cuda):
    from marlpde_amd.sweep import HipSweepEngine, initial_states, run_sweep_bdf
    N, which, t1 = 64, [0, 2, 5], 0.5
    inst = [S[i] for i in which]
    base = base_of(N)
    y0 = initial_states(base, inst)
    yfull, full, _ = cached(torch_cuda, N, which, t1)
    out = run_sweep_bdf(base, inst, (0.0, t1), FIRST, RTOL, ATOL, batched=True, events=True, device=0)
    assert len(out) == 6 and np.array_equal(out[0], yfull)
    te = t_eval_of(t1)
    out_f = run_sweep_bdf(base, inst, (0.0, t1), FIRST, RTOL, ATOL, batched=True, events=True, max_events=2, t_eval=te, device=0)
    assert len(out_f) == 8 and np.array_equal(out_f[0], yfull) and list(out_f[5]) == [len(te)] * 3
    eng = HipSweepEngine(base, inst, 0)
    try:
        yb, rb = eng.integrate_bdf(y0, (0.0, t1), FIRST, RTOL, ATOL, 0, batched=True, events=True)
        yu, ru = eng.integrate_bdf(y0, (0.0, t1), FIRST, RTOL, ATOL, 0, events=True, max_events=2)
        _, rn = eng.integrate_bdf(y0, (0.0, t1), FIRST, RTOL, ATOL, 0, batched=True)
    finally:
        eng.close()
    assert np.array_equal(yb, yfull) and all(r.t_events is None for r in rn)
    for b in range(3):
        assert same_roots(rb[b], full[b])
        for e in range(7):
            assert np.array_equal(out[-1][b][e], full[b].t_events[e])
            assert np.array_equal(out_f[-1][b][e], full[b].t_events[e][:2])
        ref = single(N, inst[b], t1)   # unbatched: each single run's roots, cut to max_events
        assert np.array_equal(yu[b], ref.y_final)
        for e in range(7):
            assert np.array_equal(ru[b].t_events[e], ref.t_events[e][:2])
    unb = run_sweep_bdf(base, inst, (0.0, t1), FIRST, RTOL, ATOL, events=True, device=0)
    for b in range(3):
        assert all(np.array_equal(unb[-1][b][e], single(N, inst[b], t1).t_events[e][:64]) for e in range(7))
