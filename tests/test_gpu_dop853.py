"""The native DOP853 loops on the GPU (marl_integrate_dop853, marl_sweep_dop853_dev / _eval_dev / _events_dev; kernels: csrc/marl_dop853.h).

References: the golden files of tools/make_dop853_goldens.py (scipy DOP853 on the REFERENCE's RHS) where one holds the case, otherwise
solve_ivp(method="DOP853", events=[7 monitors], t_eval=...) on the CPU oracle's RHS and monitors, computed here (tests/dop853_ref.py).
Shapes and states are those of tests/test_gpu_rk23.py.

Bounds - those of the RK45 and RK23 tests of the same kind:
    counts      (status, n_accepted, n_rejected, nfev) equal, nfev = 1 + 12 attempts + 3 (accepted steps with a dense output: a monitor sign
                change or a t_eval sample in them).  What makes equality a fair demand is asserted where the references are made: no
                attempt of a reference run has an error norm within 1e-4 of 1 (`margin`).
    states      final states and frames: rel_to_max <= 1e-9 - but the FRAMES of N513: <= 3.12e-8.  There the sweep's frames at 0.1 t1 and
                0.5 t1 differ from scipy's by up to 2.2e-9 (dissolved carbonate near cell 52; every count equal, the final states within
                1e-11).  scipy itself moves that far: with its RHS multiplied elementwise by 1 + 8e-15 N(0, 1) - the median elementwise
                distance of the HIP RHS from the oracle's on this run's states, measured here - the same frames of the same runs spread
                by 3.12e-9 with no decision changed (1.66e-9 at 1e-15; tools/dop853_noise.py, 4 seeds x 3 instances), the step
                controller saw-tooths at the stability limit and the frames catch it mid-tooth.  The bound is 10 x that spread; the final
                states of N513 and everything of the other shapes keep 1e-9.
    roots       |t - t_ref| <= 1e-9 |t_ref| + 1e-12 t1
The plain and the eval kernel against the roots kernel: the same final states and frames bit for bit, the same counts, times, step sizes
and monitor values; nfev equal where the same steps build a dense output (eval: the same samples, and the monitors are always watched) and
smaller by 3 per step that only holds samples where there are none (plain).
The worst values are printed per test (pytest -rA: lines starting with DOP853) and recorded in MEASURED below."""
import os

import numpy as np
import pytest

from common import GOLDEN, rel_to_max, scenario
from dop853_ref import scipy_dop853
from test_gpu_rk23 import Case, bump_state, counts, make_model, roots_close

pytestmark = pytest.mark.gpu

STATE_TOL = 1e-9
FRAME_TOL = {"N513": 10 * 3.12e-9}   # (see above; every other shape: STATE_TOL)
MARGIN = 1e-4
RTOL, ATOL = 1e-5, 1e-7

# measured on an MI355X (pytest -rA): worst rel_to_max of final states and frames, worst root |dt| / t1, per group of tests
MEASURED = {
    # group                                        final states     frames           roots
    "goldens (3, integrate_dop853)":          dict(state=1.11e-12, frame=2.86e-11, root=1.23e-14),
    "single run, dPhi_variable, N = 64":      dict(state=3.54e-13, frame=3.54e-13, root=None),       # no monitor fires
    "sweeps N200 / N200-vd":                  dict(state=7.97e-12, frame=1.18e-10, root=2.81e-13),
    "sweep N513":                             dict(state=9.49e-12, frame=2.22e-09, root=1.71e-14),   # the frames at 0.1 t1 and 0.5 t1: see above
    "sweep N1024":                            dict(state=9.97e-12, frame=2.75e-10, root=7.15e-14),
    "sweep N200, budget / close samples":     dict(state=7.97e-12, frame=1.65e-10, root=2.81e-13),
}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. single runs
# ---------------------------------------------------------------------------------------------------------------------------------
GOLDENS = ["dop853_traj_A_N64", "dop853_traj_default_N200", "dop853_event_default_N400"]


@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_through_integrate_dop853(name):
    """The attempt counts of scipy's DOP853 on the reference's RHS, its nfev with the dense outputs it built, its final state, its t_eval
    frames and its root time."""
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    N = g["y0"].size // 5
    assert float(g["err_margin"]) > MARGIN
    assert int(g["nfev"]) == 1 + 12 * g["accepted"].size + 3 * g["dense_steps"].size
    eq = make_model(scenario("A" if "_A_" in name else "default", N))
    try:
        te = g["t_eval"] if "t_eval" in g.files and g["t_eval"].size else None
        t1 = float(g["t_span"][1])
        res = eq.integrate_dop853(g["y0"], tuple(g["t_span"]), float(g["first_step"]), float(g["rtol"]), float(g["atol"]), t_eval=te)
    finally:
        eq.close()
    assert counts(res) == (0, int(g["n_accepted"]), int(g["n_rejected"]), int(g["nfev"])) and res.t_reached == t1
    err = rel_to_max(res.y_final, g["y_final"])
    worst_frame = 0.0
    if te is not None:
        assert g["dense_steps"].size >= 2
        assert np.array_equal(res.t, g["t_eval"]) and np.array_equal(res.y[:, 0], g["y0"])
        worst_frame = max(rel_to_max(res.y[:, j], g["y_eval"][:, j]) for j in range(len(te)))
    assert [len(e) for e in res.t_events] == list(g["n_events"])
    worst_root = 0.0
    if "t_events" in g.files:
        assert list(g["n_events"]) == [0, 0, 0, 0, 0, 1, 0] and g["dense_steps"].size == 1
        ref = [g["t_events"][:1] if e == 5 else np.empty(0) for e in range(7)]
        worst_root = roots_close(res.t_events, ref, t1)
    print(f"DOP853 golden {name}: final {err:.2e} frames {worst_frame:.2e} root |dt|/t1 {worst_root:.2e}")
    assert err <= STATE_TOL and worst_frame <= STATE_TOL


def test_single_run_with_time_varying_porosity_diffusion_and_edges_of_the_entry(oracle):
    """A, N = 64 with dPhi_variable (the VD instantiations) against scipy on the oracle; t_eval holding t0 and t1; t0 == t1; an attempt
    budget (status 2 and the attempts made); a first step beyond the span and unsorted samples are refused as scipy refuses them."""
    from marlpde_amd._abi import MarlError
    N = 64
    p = scenario("A", N) | {"dPhi_variable": True}
    eq = make_model(p)
    try:
        P = oracle.params_from_model(eq)
        y0 = np.repeat([float(p[k]) for k in ("CAIni", "CCIni", "cCaIni", "cCO3Ini", "PhiIni")], N)
        t1, h0 = 2e-3, 1e-6
        te = np.array([0.0, 0.3 * t1, 0.30001 * t1, t1])
        ref = scipy_dop853(oracle, P, N, y0, (0.0, t1), h0, RTOL, ATOL, t_eval=te)
        assert ref.margin > MARGIN and ref.n_rejected >= 1 and len(ref.dense_steps) == 3
        res = eq.integrate_dop853(y0, (0.0, t1), h0, RTOL, ATOL, t_eval=te)
        assert counts(res) == (ref.status, ref.n_accepted, ref.n_rejected, ref.nfev)
        assert np.array_equal(res.t, te) and np.array_equal(res.y[:, 0], y0)
        worst = max([rel_to_max(res.y[:, j], ref.y_eval[j]) for j in range(len(te))] + [rel_to_max(res.y_final, ref.y_final)])
        roots_close(res.t_events, ref.t_events, t1)
        print(f"DOP853 single vd: worst state / frame {worst:.2e}")
        assert worst <= STATE_TOL
        # without t_eval and without located roots: the plain kernel, no dense output (no monitor fires), the same state bit for bit
        bare = eq.integrate_dop853(y0, (0.0, t1), h0, RTOL, ATOL, events=False)
        assert counts(bare) == (0, ref.n_accepted, ref.n_rejected, 1 + 12 * len(ref.accepted)) and np.array_equal(bare.y_final, res.y_final)
        # t0 == t1: no step, one evaluation counted, the sample at t0 is y0
        res = eq.integrate_dop853(y0, (0.5, 0.5), h0, RTOL, ATOL, t_eval=np.array([0.5]))
        assert counts(res) == (0, 0, 0, 1) and np.array_equal(res.y[:, 0], y0) and np.array_equal(res.y_final, y0)
        # attempt budget
        cut = scipy_dop853(oracle, P, N, y0, (0.0, t1), h0, RTOL, ATOL, max_attempts=30)
        res = eq.integrate_dop853(y0, (0.0, t1), h0, RTOL, ATOL, max_attempts=30)
        assert counts(res) == (2, cut.n_accepted, cut.n_rejected, 1 + 12 * 30) and res.n_accepted + res.n_rejected == 30
        assert res.t_reached == pytest.approx(cut.t, rel=1e-12) and rel_to_max(res.y_final, cut.y_final) <= STATE_TOL
        with pytest.raises(MarlError, match=r"dop853: `first_step` exceeds bounds"):
            eq.integrate_dop853(y0, (0.0, t1), 2 * t1, RTOL, ATOL)
        with pytest.raises(MarlError, match=r"dop853: `t_eval` must be sorted"):
            eq.integrate_dop853(y0, (0.0, t1), h0, RTOL, ATOL, t_eval=np.array([0.5 * t1, 0.25 * t1]))
        with pytest.raises(MarlError, match=r"dop853: tolerances must be positive"):
            eq.integrate_dop853(y0, (0.0, t1), h0, 0.0, ATOL)
    finally:
        eq.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. sweeps: the states and instance lists of tests/test_gpu_rk23.py
# ---------------------------------------------------------------------------------------------------------------------------------
# name -> what scipy DOP853 does on the oracle there: attempts per instance (lo, hi), rejections (lo, hi); the roots are those of the RK23
# table (the same states: test_gpu_rk23.SHAPES), asserted against it to 1e-3 of t1
FACTS = {"N200": ((234, 235), (2, 2)), "N200-vd": ((234, 234), (2, 2)), "N513": ((1397, 1399), (6, 6)), "N1024": ((1102, 1102), (2, 2))}


class DopCase(Case):
    def run(self, torch, events=True, max_events=64, t_eval="case", max_attempts=0, t_span=None):
        """Through LMAHeureuxPorosityDiff.sweep_dop853_device: (results, final states, frames [instance][sample][5N] or None)."""
        eq = make_model(self.base, self.inst)
        eq.use_stream(torch.cuda.current_stream().cuda_stream)
        te = self.t_eval if isinstance(t_eval, str) else t_eval
        yd = torch.from_numpy(np.ascontiguousarray(self.y0)).cuda()
        frames, more = None, {}
        try:
            if te is not None:
                frames = torch.full((len(self.inst), max(len(te), 1), 5 * self.N), float("nan"), dtype=torch.float64, device="cuda")
                more = dict(t_eval=te, y_eval_dev_ptr=frames.data_ptr())
            if events is not None:
                more |= dict(events=events, max_events=max_events)
            res = eq.sweep_dop853_device(yd.data_ptr(), t_span or (0.0, self.t1), self.h0, RTOL, ATOL, max_attempts, **more)
            torch.cuda.synchronize()
        finally:
            eq.close()
        return res, yd.cpu().numpy(), None if frames is None else frames.cpu().numpy()


_REF, _GOT = {}, {}


def _reference(oracle, name, max_attempts=0, t_eval=None):
    """scipy DOP853 on the oracle for every instance of a shape, made once per session and never changed; what the shapes were chosen for
    is asserted on the full runs."""
    key = (name, max_attempts, None if t_eval is None else tuple(t_eval))
    if key not in _REF:
        c = DopCase(name)
        te = c.t_eval if t_eval is None else t_eval
        out = [scipy_dop853(oracle, oracle.params_from_dict(c.base | inst), c.N, c.y0[b], (0.0, c.t1), c.h0, RTOL, ATOL, t_eval=te,
                            max_attempts=max_attempts) for b, inst in enumerate(c.inst)]
        for r in out:
            for a in (r.y_final, r.y_eval, *r.t_events):
                a.setflags(write=False)
            assert r.margin > MARGIN, (name, r.margin)
        if max_attempts == 0:
            print(f"DOP853 {name}: scipy attempts {[r.n_accepted + r.n_rejected for r in out]} rejected {[r.n_rejected for r in out]} "
                  f"nfev {[r.nfev for r in out]} closest norm {min(r.margin for r in out):.1e}")
            assert all(r.status == 0 and r.t == c.t1 for r in out)
            assert sum(len(t) for r in out for t in r.t_events) >= 1
            attempts, rejections = FACTS[name]
            assert all(attempts[0] <= r.n_accepted + r.n_rejected <= attempts[1] for r in out)
            assert all(rejections[0] <= r.n_rejected <= rejections[1] for r in out)
            if c.facts is not None:
                for b, r in enumerate(out):
                    found = [(e, float(t) / c.t1) for e in range(7) for t in r.t_events[e]]
                    assert [e for e, _ in found] == [e for e, _ in c.facts[b]], (name, b, found)
                    assert all(abs(f - w) < 1e-3 for (_, f), (_, w) in zip(found, c.facts[b])), (name, b, found)
            if name == "N200":   # monitors 0 and 1 of instances 1 and 6 change sign in the same step: ONE dense output, +3 once
                for b in (1, 6):
                    t0_, t1_ = out[b].t_events[0][0], out[b].t_events[1][0]
                    assert np.searchsorted(out[b].step_times, t0_) == np.searchsorted(out[b].step_times, t1_)
                if t_eval is None:   # four sample steps; one more step where the two monitors fire together
                    assert out[0].nfev == 1 + 12 * 234 + 3 * 4 and out[1].nfev == out[0].nfev + 3
        _REF[key] = (c, out)
    return _REF[key]


def _event_steps(r):
    """the accepted steps of a reference run in which a monitor changes sign"""
    return {int(np.searchsorted(r.step_times, t)) for e in range(7) for t in r.t_events[e]}


def _stats_key(r, nfev=True):
    return (r.status, r.n_accepted, r.n_rejected, r.nfev if nfev else None, r.t_reached, r.h_next, tuple(r.n_events), tuple(r.event_values))


def _check(c, ref, res, yfin, frames, label, t_eval=None):
    te = c.t_eval if t_eval is None else t_eval
    worst, worst_frame, worst_root = 0.0, 0.0, 0.0
    for b, r in enumerate(ref):
        assert counts(res[b]) == (r.status, r.n_accepted, r.n_rejected, r.nfev), (label, b)
        assert list(res[b].n_events) == [len(t) for t in r.t_events], (label, b)
        if res[b].t_events is not None:
            worst_root = max(worst_root, roots_close(res[b].t_events, r.t_events, c.t1))
        if frames is not None:
            k = len(res[b].t)
            assert k == len(r.t_eval) and np.array_equal(res[b].t, te[:k]), (label, b)
            for i in range(k):
                worst_frame = max(worst_frame, rel_to_max(frames[b, i], r.y_eval[i]))
            assert np.all(np.isnan(frames[b, k:])), (label, b)
        worst = max(worst, rel_to_max(yfin[b], r.y_final))
    print(f"DOP853 sweep {label}: worst final state {worst:.2e}, worst frame {worst_frame:.2e}, worst root |dt|/t1 {worst_root:.2e}")
    assert worst <= STATE_TOL and worst_frame <= FRAME_TOL.get(c.name, STATE_TOL)


def _with_events(torch, oracle, name):
    c, ref = _reference(oracle, name)
    if name not in _GOT:
        _GOT[name] = c.run(torch)
    return (c, ref) + _GOT[name]


@pytest.mark.parametrize("name", ["N200", "N200-vd", "N513", "N1024"])
def test_sweep_kernels_against_scipy_and_bit_for_bit_against_each_other(torch_cuda, oracle, name):
    """dop853_sweep_roots_kernel (roots + frames) against scipy; dop853_sweep_eval_kernel (frames) and dop853_sweep_kernel (plain): the
    same final states, bit for bit, and the same statistics - locating roots and writing samples leave the integration alone.  nfev of the
    plain sweep: no sample, so only the steps with a sign change count a dense output."""
    c, ref, res, yfin, frames = _with_events(torch_cuda, oracle, name)
    _check(c, ref, res, yfin, frames, name)
    assert np.array_equal(frames[:, 0], c.y0)
    fr, yfr, ffr = c.run(torch_cuda, events=False)
    pl, ypl, none = c.run(torch_cuda, events=None, t_eval=None)
    assert none is None and np.array_equal(yfr, yfin) and np.array_equal(ypl, yfin) and np.array_equal(ffr, frames, equal_nan=True)
    for b, r in enumerate(ref):
        assert _stats_key(fr[b]) == _stats_key(res[b]), b
        assert _stats_key(pl[b], nfev=False) == _stats_key(res[b], nfev=False), b
        assert pl[b].nfev == 1 + 12 * (r.n_accepted + r.n_rejected) + 3 * len(_event_steps(r)), b
        assert fr[b].t_events is None and pl[b].t_events is None and pl[b].t is None and np.array_equal(fr[b].t, res[b].t)


def test_sweep_budget_caps_close_samples_idle_instances_and_refusals(torch_cuda, oracle):
    from marlpde_amd._abi import MarlError
    torch = torch_cuda
    c, ref, res, yfin, frames = _with_events(torch, oracle, "N200")
    # max_attempts = 100: every instance stops with status 2; the frames reached are scipy's, the memory above them still holds its NaN
    _, cut = _reference(oracle, "N200", max_attempts=100)
    assert all(r.status == 2 and 0 < len(r.t_eval) < len(c.t_eval) for r in cut)
    got, y, f = c.run(torch, max_attempts=100)
    _check(c, cut, got, y, f, "N200 budget")
    assert all(r.n_accepted + r.n_rejected == 100 for r in got)
    # max_events = 1: every count unchanged, one root per fired monitor; max_events = 0: the frames-only entry
    one, y1, f1 = c.run(torch, max_events=1)
    assert np.array_equal(y1, yfin) and np.array_equal(f1, frames, equal_nan=True)
    for b in range(len(c.inst)):
        assert _stats_key(one[b]) == _stats_key(res[b]), b
        assert all(np.array_equal(a, w[:1]) for a, w in zip(one[b].t_events, res[b].t_events)), b
    zero, y0_, f0 = c.run(torch, max_events=0)
    assert np.array_equal(y0_, yfin) and np.array_equal(f0, frames, equal_nan=True)
    assert all(_stats_key(zero[b]) == _stats_key(res[b]) and zero[b].t_events is None for b in range(len(c.inst)))
    # three samples inside one step (a step is ~ t1 / 230): more than one replay before the commit, ONE dense output counted
    te = c.t1 * np.array([0.5, 0.5005, 0.501, 0.9])
    _, close = _reference(oracle, "N200", t_eval=te)
    per_step = np.bincount(np.searchsorted(close[0].step_times, te[:3], side="left"))
    assert per_step.max() >= 2
    got, y, f = c.run(torch, t_eval=te)
    _check(c, close, got, y, f, "N200 close samples", t_eval=te)
    assert np.array_equal(y, yfin)
    # t0 == t1: no instance runs - no step, no root, the state untouched; a sample at t0 is y0
    idle, yi, fi = c.run(torch, t_eval=np.array([0.0]), t_span=(0.0, 0.0))
    assert all(counts(r) == (0, 0, 0, 1) and list(r.t) == [0.0] and sum(len(t) for t in r.t_events) == 0 for r in idle)
    assert np.array_equal(yi, c.y0) and np.array_equal(fi[:, 0], c.y0)
    # a grid that does not fit one workgroup: every entry refuses it, and the state is untouched
    big = DopCase("N200")
    big.N, big.base = 1025, scenario("default", 1025)
    big.inst, big.y0 = [{}, {}], np.stack([bump_state(big.base, 1025)] * 2)
    for kw in (dict(events=None, t_eval=None), dict(events=False), dict()):
        with pytest.raises(MarlError, match=r"rc=-1.*dop853: N = 1025: .*N <= 1024 cells"):
            big.run(torch, **kw)
    eq = make_model(scenario("default", 1025))
    try:
        with pytest.raises(MarlError, match=r"rc=-1.*dop853: N = 1025: .*N <= 1024 cells"):
            eq.integrate_dop853(big.y0[0], (0.0, c.t1), c.h0, RTOL, ATOL)
    finally:
        eq.close()


def test_terminal_monitors_are_refused_by_every_entry(torch_cuda):
    """No DOP853 entry stops at a monitor's root: while a limit is set each returns -1 with the standard message and leaves the state alone."""
    from marlpde_amd._abi import MarlError
    from marlpde_amd.sweep import run_sweep_dop853
    torch = torch_cuda
    c = DopCase("N200")
    msg = r"rc=-1.*marl_{}: terminal monitors are not supported by this entry \(marl_set_terminal\)"
    eq = make_model(c.base, c.inst)
    try:
        eq.set_terminal({"zeros_U": True})
        yd = torch.from_numpy(np.ascontiguousarray(c.y0)).cuda()
        frames = torch.full((len(c.inst), len(c.t_eval), 5 * c.N), float("nan"), dtype=torch.float64, device="cuda")
        with pytest.raises(MarlError, match=msg.format("sweep_dop853_dev")):
            eq.sweep_dop853_device(yd.data_ptr(), (0.0, c.t1), c.h0, RTOL, ATOL)
        with pytest.raises(MarlError, match=msg.format("sweep_dop853_eval_dev")):
            eq.sweep_dop853_device(yd.data_ptr(), (0.0, c.t1), c.h0, RTOL, ATOL, t_eval=c.t_eval, y_eval_dev_ptr=frames.data_ptr())
        with pytest.raises(MarlError, match=msg.format("sweep_dop853_events_dev")):
            eq.sweep_dop853_device(yd.data_ptr(), (0.0, c.t1), c.h0, RTOL, ATOL, t_eval=c.t_eval, y_eval_dev_ptr=frames.data_ptr(), events=True)
        torch.cuda.synchronize()
        assert np.array_equal(yd.cpu().numpy(), c.y0) and bool(torch.isnan(frames).all())
    finally:
        eq.close()
    one = make_model(c.base | c.inst[3])
    try:
        one.set_terminal({"zeros_U": True})
        with pytest.raises(MarlError, match=msg.format("integrate_dop853")):
            one.integrate_dop853(c.y0[3], (0.0, c.t1), c.h0, RTOL, ATOL)
    finally:
        one.close()
    with pytest.raises(MarlError, match=msg.format("sweep_dop853_dev")):
        run_sweep_dop853(c.base, c.inst, (0.0, c.t1), c.h0, RTOL, ATOL, y0=c.y0, device=0, terminal={"zeros_U": True})


def test_engine_driver_and_integrate_equations_return_what_the_entries_return(torch_cuda, oracle):
    from marlpde_amd.Evolve_scenario import integrate_equations
    from marlpde_amd.sweep import HipSweepEngine, run_sweep_dop853
    c, ref, res, yfin, frames = _with_events(torch_cuda, oracle, "N200")
    eng = HipSweepEngine(c.base, c.inst, 0)
    try:
        y, got = eng.integrate_dop853(c.y0, (0.0, c.t1), c.h0, RTOL, ATOL, 0, t_eval=c.t_eval, events=True)
    finally:
        eng.close()
    assert np.array_equal(y, yfin)
    for b in range(len(c.inst)):
        assert all(np.array_equal(a, w) for a, w in zip(got[b].t_events, res[b].t_events)) and np.array_equal(got[b].y, frames[b].T), b
    out = run_sweep_dop853(c.base, c.inst, (0.0, c.t1), c.h0, RTOL, ATOL, y0=c.y0, device=0, t_eval=c.t_eval, events=True)
    plain = run_sweep_dop853(c.base, c.inst, (0.0, c.t1), c.h0, RTOL, ATOL, y0=c.y0, device=0)
    assert len(out) == 8 and len(plain) == 5
    for a, w in zip(out[:5], plain):
        assert np.array_equal(a, w)
    assert np.array_equal(out[0], yfin) and out[1].tolist() == [0] * len(c.inst) and out[2].tolist() == [r.n_accepted for r in ref]
    assert out[3].tolist() == [r.n_rejected for r in ref] and out[5].tolist() == [len(c.t_eval)] * len(c.inst)
    assert np.array_equal(out[6], frames)
    for b in range(len(c.inst)):
        assert len(out[7][b]) == 7 and all(np.array_equal(a, w) for a, w in zip(out[7][b], res[b].t_events)), b
    # integrate_equations(method="DOP853"): the native single run of the uniform initial state, bit for bit
    p = scenario("A", 64)
    t1 = 2e-3
    solver = dict(method="DOP853", backend="hip", first_step=1e-6, rtol=RTOL, atol=ATOL, t_span=(0.0, t1))
    last, covered, depths, Xstar, folder = integrate_equations(solver, {"t_eval": np.array([0.0, t1])}, p, results_root=None, verbose=False)
    eq = make_model(p)
    try:
        y0 = np.repeat([float(p[k]) for k in ("CAIni", "CCIni", "cCaIni", "cCO3Ini", "PhiIni")], 64)
        direct = eq.integrate_dop853(y0, (0.0, t1), 1e-6, RTOL, ATOL, t_eval=np.array([0.0, t1]))
    finally:
        eq.close()
    assert direct.status == 0 and covered == p["Tstar"] * t1 and np.array_equal(last, direct.y[:, -1].reshape(5, 64))
