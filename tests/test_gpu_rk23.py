"""The native RK23 loops on the GPU (marl_integrate_rk23 / _dev, marl_sweep_rk23_dev / _eval_dev / _events_dev; kernels: csrc/marl_rk23.h).

References: the golden files of tools/make_rk23_goldens.py (scipy RK23 on the REFERENCE's RHS) where one holds the case, otherwise
solve_ivp(method="RK23", events=[7 monitors], t_eval=...) on the CPU oracle's RHS and monitors, computed here (tests/rk23_ref.py).

Bounds - those of the RK45 tests of the same kind:
    counts      (status, n_accepted, n_rejected, nfev) equal.  What makes equality a fair demand is asserted where the references are
                made: no attempt of a reference run has an error norm within 1e-4 of 1 (`margin`).
    states      final states and frames: rel_to_max <= 1e-9
    roots       |t - t_ref| <= 1e-9 |t_ref| + 1e-12 t1
The worst values are printed per test (pytest -rA: lines starting with RK23) and recorded in MEASURED below."""
import os

import numpy as np
import pytest

from common import GOLDEN, rel_to_max, scenario, synthetic_state
from rk23_ref import scipy_rk23

pytestmark = pytest.mark.gpu

STATE_TOL = 1e-9
ROOT_RTOL, ROOT_ATOL_T1 = 1e-9, 1e-12
MARGIN = 1e-4
RTOL, ATOL = 1e-5, 1e-7
T_FRAC = np.array([0.0, 0.1, 0.5, 1.0])

# measured on an MI355X (pytest -rA): worst rel_to_max of final states and frames, worst root |dt| / t1, per group of tests
MEASURED = {
    # group                                        states / frames     roots
    "goldens (5, integrate_rk23)":            dict(state=1.03e-12, root=4.75e-15),   # the tight-tolerance run; the others <= 2.7e-14
    "single run, dPhi_variable, N = 64":      dict(state=2.55e-15, root=None),       # no monitor fires
    "sweeps N200 / N200-vd":                  dict(state=4.92e-11, root=1.42e-12),   # monitor 3 (max CA + CC - 1): the shallow crossing
    "sweeps N513 / N1024":                    dict(state=1.30e-14, root=1.01e-14),
    "sweep N200, budget / close samples":     dict(state=8.21e-11, root=1.42e-12),
    "large grids 1025 .. 5003, both layouts": dict(state=4.41e-15, root=None),
    "large event, N = 1500":                  dict(state=3.62e-15, root=1.05e-13),
}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def make_model(p, instances=None):
    from marlpde_amd.LHeureux_model import LMAHeureuxPorosityDiff
    return LMAHeureuxPorosityDiff.from_scenario(p, device=0, instances=instances)


def counts(r):
    return (r.status, r.n_accepted, r.n_rejected, r.nfev)


def roots_close(got, ref, t1):
    worst = 0.0
    for e in range(7):
        assert len(got[e]) == len(ref[e]), (e, got[e], ref[e])
        for a, b in zip(got[e], ref[e]):
            assert abs(a - b) <= ROOT_RTOL * abs(b) + ROOT_ATOL_T1 * t1, (e, a, b)
            worst = max(worst, abs(a - b) / t1)
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. single small runs
# ---------------------------------------------------------------------------------------------------------------------------------
GOLDENS = ["rk23_traj_A_N64", "rk23_traj_A_N200", "rk23_traj_default_N200", "rk23_traj_A_N64_tight", "rk23_event_default_N400"]


@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_through_integrate_rk23(name):
    """The attempt counts of scipy's RK23 on the reference's RHS, its final state, its t_eval frames and its root times."""
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    N = g["y0"].size // 5
    assert float(g["err_margin"]) > MARGIN
    eq = make_model(scenario("A" if "_A_" in name else "default", N))
    try:
        te = g["t_eval"] if "t_eval" in g.files and g["t_eval"].size else None
        t1 = float(g["t_span"][1])
        res = eq.integrate_rk23(g["y0"], tuple(g["t_span"]), float(g["first_step"]), float(g["rtol"]), float(g["atol"]), t_eval=te)
    finally:
        eq.close()
    assert counts(res) == (0, int(g["n_accepted"]), int(g["n_rejected"]), int(g["nfev"])) and res.t_reached == t1
    err = rel_to_max(res.y_final, g["y_final"])
    worst_frame = 0.0
    if te is not None:
        assert np.array_equal(res.t, g["t_eval"]) and np.array_equal(res.y[:, 0], g["y0"])
        worst_frame = max(rel_to_max(res.y[:, j], g["y_eval"][:, j]) for j in range(len(te)))
    assert [len(e) for e in res.t_events] == list(g["n_events"])
    worst_root = 0.0
    if "t_events" in g.files:
        assert list(g["n_events"]) == [0, 0, 0, 0, 0, 1, 0]
        ref = [g["t_events"][:1] if e == 5 else np.empty(0) for e in range(7)]
        worst_root = roots_close(res.t_events, ref, t1)
    print(f"RK23 golden {name}: final {err:.2e} frames {worst_frame:.2e} root |dt|/t1 {worst_root:.2e}")
    assert err <= STATE_TOL and worst_frame <= STATE_TOL


def test_single_small_run_with_time_varying_porosity_diffusion_and_edges_of_the_entry(oracle):
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
        ref = scipy_rk23(oracle, P, N, y0, (0.0, t1), h0, 1e-3, 1e-3, t_eval=te)
        assert ref.margin > MARGIN and ref.n_rejected >= 1
        res = eq.integrate_rk23(y0, (0.0, t1), h0, 1e-3, 1e-3, t_eval=te)
        assert counts(res) == (ref.status, ref.n_accepted, ref.n_rejected, ref.nfev)
        assert np.array_equal(res.t, te) and np.array_equal(res.y[:, 0], y0)
        worst = max([rel_to_max(res.y[:, j], ref.y_eval[j]) for j in range(len(te))] + [rel_to_max(res.y_final, ref.y_final)])
        roots_close(res.t_events, ref.t_events, t1)
        print(f"RK23 single vd: worst state / frame {worst:.2e}")
        assert worst <= STATE_TOL
        # t0 == t1: no step, one evaluation counted, the sample at t0 is y0
        res = eq.integrate_rk23(y0, (0.5, 0.5), h0, 1e-3, 1e-3, t_eval=np.array([0.5]))
        assert counts(res) == (0, 0, 0, 1) and np.array_equal(res.y[:, 0], y0) and np.array_equal(res.y_final, y0)
        # attempt budget
        cut = scipy_rk23(oracle, P, N, y0, (0.0, t1), h0, 1e-3, 1e-3, max_attempts=40)
        res = eq.integrate_rk23(y0, (0.0, t1), h0, 1e-3, 1e-3, max_attempts=40)
        assert counts(res) == (2, cut.n_accepted, cut.n_rejected, 1 + 3 * 40) and res.n_accepted + res.n_rejected == 40
        assert res.t_reached == pytest.approx(cut.t, rel=1e-12) and rel_to_max(res.y_final, cut.y_final) <= STATE_TOL
        with pytest.raises(MarlError, match=r"rk23: `first_step` exceeds bounds"):
            eq.integrate_rk23(y0, (0.0, t1), 2 * t1, 1e-3, 1e-3)
        with pytest.raises(MarlError, match=r"rk23: `t_eval` must be sorted"):
            eq.integrate_rk23(y0, (0.0, t1), h0, 1e-3, 1e-3, t_eval=np.array([0.5 * t1, 0.25 * t1]))
    finally:
        eq.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. sweeps: the states and instance lists of tests/test_gpu_sweep_events.py
# ---------------------------------------------------------------------------------------------------------------------------------
_N200 = [({}, {}), (dict(ca_low=-1e-3), {}), (dict(phi_dip=0.038, sum_top=1.0005), {}), (dict(phi_dip=0.04), {}), (dict(phi_dip=0.042), {}),
         (dict(phi_dip=0.04), dict(k3=0.05, k4=0.05)), (dict(ca_low=-1e-3), dict(Phi0=0.7))]
# name -> (N, m, [(state, parameter overrides)], scenario extras,
#          what scipy RK23 does on the oracle there: attempts per instance (lo, hi), rejections (lo, hi),
#          per instance [(monitor, root / t1)]; None: not tabulated, only that a monitor fires)
SHAPES = {
    "N200": (200, 250, _N200, {}, (592, 594), (3, 6),
             [[], [(0, 0.8148), (1, 0.8148)], [(3, 0.9235), (5, 0.0378)], [(5, 0.1349)], [(5, 0.336)], [(5, 0.2601)], [(0, 0.2709), (1, 0.2709)]]),
    "N200-vd": (200, 250, _N200[:5], {"dPhi_variable": True}, None, None, None),
    "N513": (513, 1500, [(dict(ca_low=-3e-4), {}), (dict(phi_dip=0.04), {}), ({}, {})], {}, (3543, 3549), (5, 7),
             [[(0, 0.7072), (1, 0.7072)], [(5, 0.1491)], []]),
    "N1024": (1024, 1200, [(dict(phi_dip=0.04), {}), ({}, {})], {}, (2803, 2803), (4, 4), [[(5, 0.7429)], []]),
}


def bump_state(p, N, phi_dip=None, ca_low=None, sum_top=None):
    L = p["max_depth"] / p["Xstar"]
    x = (np.arange(N) + 0.5) * (L / N)
    b = lambda c, w: np.exp(-((x - c * L) / (w * L)) ** 2)  # noqa: E731
    y = np.stack([np.full(N, float(p[k])) for k in ("CAIni", "CCIni", "cCaIni", "cCO3Ini", "PhiIni")])
    if phi_dip is not None:
        y[4] = p["PhiIni"] - phi_dip * b(0.5, 0.08)
    if ca_low is not None:
        y[0] = p["CAIni"] - (p["CAIni"] - ca_low) * b(0.2, 0.08)
    if sum_top is not None:
        y[0] = p["CAIni"] + (sum_top - p["CAIni"] - p["CCIni"]) * b(0.7, 0.05)
    return y.ravel()


class Case:
    def __init__(self, name):
        self.name = name
        self.N, m, pairs, extra, self.attempts, self.rejections, self.facts = SHAPES[name]
        self.base = scenario("default", self.N) | extra
        self.inst = [dict(ov) for _, ov in pairs]
        self.dx2 = ((self.base["max_depth"] / self.base["Xstar"]) / self.N) ** 2
        self.t1 = m * self.dx2
        self.h0 = 0.5 * self.dx2
        self.t_eval = self.t1 * T_FRAC
        self.y0 = np.stack([bump_state(self.base | ov, self.N, **st) for st, ov in pairs])

    def run(self, torch, events=True, max_events=64, t_eval="case", max_attempts=0, t_span=None):
        """Through LMAHeureuxPorosityDiff.sweep_rk23_device: (results, final states, frames [instance][sample][5N] or None)."""
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
            res = eq.sweep_rk23_device(yd.data_ptr(), t_span or (0.0, self.t1), self.h0, RTOL, ATOL, max_attempts, **more)
            torch.cuda.synchronize()
        finally:
            eq.close()
        return res, yd.cpu().numpy(), None if frames is None else frames.cpu().numpy()


_REF, _GOT = {}, {}


def _reference(oracle, name, max_attempts=0, t_eval=None):
    """scipy RK23 on the oracle for every instance of a shape, made once per session and never changed; what the shapes were chosen for
    is asserted on the full runs."""
    key = (name, max_attempts, None if t_eval is None else tuple(t_eval))
    if key not in _REF:
        c = Case(name)
        te = c.t_eval if t_eval is None else t_eval
        out = [scipy_rk23(oracle, oracle.params_from_dict(c.base | inst), c.N, c.y0[b], (0.0, c.t1), c.h0, RTOL, ATOL, t_eval=te,
                          max_attempts=max_attempts) for b, inst in enumerate(c.inst)]
        for r in out:
            for a in (r.y_final, r.y_eval, *r.t_events):
                a.setflags(write=False)
            assert r.margin > MARGIN, (name, r.margin)
        if max_attempts == 0:
            print(f"RK23 {name}: scipy attempts {[r.n_accepted + r.n_rejected for r in out]} rejected {[r.n_rejected for r in out]} "
                  f"closest norm {min(r.margin for r in out):.1e}")
            assert all(r.status == 0 and r.t == c.t1 for r in out)
            assert sum(len(t) for r in out for t in r.t_events) >= 1
            if c.attempts is not None:
                assert all(c.attempts[0] <= r.n_accepted + r.n_rejected <= c.attempts[1] for r in out)
                assert all(c.rejections[0] <= r.n_rejected <= c.rejections[1] for r in out)
                for b, r in enumerate(out):
                    found = [(e, float(t) / c.t1) for e in range(7) for t in r.t_events[e]]
                    assert [e for e, _ in found] == [e for e, _ in c.facts[b]], (name, b, found)
                    assert all(abs(f - w) < 1e-3 for (_, f), (_, w) in zip(found, c.facts[b])), (name, b, found)
            if name == "N200":   # monitors 0 and 1 of instance 1 change sign in the same step
                t0_, t1_ = out[1].t_events[0][0], out[1].t_events[1][0]
                assert np.searchsorted(out[1].step_times, t0_) == np.searchsorted(out[1].step_times, t1_)
        _REF[key] = (c, out)
    return _REF[key]


def _stats_key(r):
    return (r.status, r.n_accepted, r.n_rejected, r.nfev, r.t_reached, r.h_next, tuple(r.n_events), tuple(r.event_values))


def _check(c, ref, res, yfin, frames, label, t_eval=None):
    te = c.t_eval if t_eval is None else t_eval
    worst, worst_root = 0.0, 0.0
    for b, r in enumerate(ref):
        assert counts(res[b]) == (r.status, r.n_accepted, r.n_rejected, r.nfev), (label, b)
        assert list(res[b].n_events) == [len(t) for t in r.t_events], (label, b)
        if res[b].t_events is not None:
            worst_root = max(worst_root, roots_close(res[b].t_events, r.t_events, c.t1))
        if frames is not None:
            k = len(res[b].t)
            assert k == len(r.t_eval) and np.array_equal(res[b].t, te[:k]), (label, b)
            for i in range(k):
                worst = max(worst, rel_to_max(frames[b, i], r.y_eval[i]))
            assert np.all(np.isnan(frames[b, k:])), (label, b)
        worst = max(worst, rel_to_max(yfin[b], r.y_final))
    print(f"RK23 sweep {label}: worst state / frame {worst:.2e}, worst root |dt|/t1 {worst_root:.2e}")
    assert worst <= STATE_TOL


def _with_events(torch, oracle, name):
    c, ref = _reference(oracle, name)
    if name not in _GOT:
        _GOT[name] = c.run(torch)
    return (c, ref) + _GOT[name]


@pytest.mark.parametrize("name", ["N200", "N200-vd", "N513", "N1024"])
def test_sweep_kernels_against_scipy_and_bit_for_bit_against_each_other(torch_cuda, oracle, name):
    """rk23_sweep_roots_kernel (roots + frames) against scipy; rk23_sweep_eval_kernel (frames) and rk23_sweep_kernel (plain): the same
    final states, bit for bit, and the same counts - locating roots and writing samples leave the integration alone."""
    c, ref, res, yfin, frames = _with_events(torch_cuda, oracle, name)
    _check(c, ref, res, yfin, frames, name)
    assert np.array_equal(frames[:, 0], c.y0)
    fr, yfr, ffr = c.run(torch_cuda, events=False)
    pl, ypl, none = c.run(torch_cuda, events=None, t_eval=None)
    assert none is None and np.array_equal(yfr, yfin) and np.array_equal(ypl, yfin) and np.array_equal(ffr, frames, equal_nan=True)
    for b in range(len(c.inst)):
        assert _stats_key(fr[b]) == _stats_key(res[b]) == _stats_key(pl[b]), b
        assert fr[b].t_events is None and pl[b].t_events is None and pl[b].t is None and np.array_equal(fr[b].t, res[b].t)


def test_sweep_budget_caps_close_samples_idle_instances_and_the_window_limit(torch_cuda, oracle):
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
    # three samples inside one step (a step is ~ t1 / 590): more than one replay before the commit
    te = c.t1 * np.array([0.5, 0.5002, 0.5004, 0.9])
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
    # a grid that does not fit one workgroup
    big = Case("N200")
    big.N, big.base = 1025, scenario("default", 1025)
    big.inst, big.y0 = [{}, {}], np.stack([bump_state(big.base, 1025)] * 2)
    for kw in (dict(events=None, t_eval=None), dict(events=False), dict()):
        with pytest.raises(MarlError, match=r"rc=-1.*marl_sweep_rk23_dev: N = 1025 exceeds the largest one-workgroup window \(1024 cells\)"):
            big.run(torch, **kw)


def test_engine_and_driver_return_what_the_sweep_returns(torch_cuda, oracle):
    from marlpde_amd.sweep import HipSweepEngine, run_sweep_rk23
    c, ref, res, yfin, frames = _with_events(torch_cuda, oracle, "N200")
    eng = HipSweepEngine(c.base, c.inst, 0)
    try:
        y, got = eng.integrate_rk23(c.y0, (0.0, c.t1), c.h0, RTOL, ATOL, 0, t_eval=c.t_eval, events=True)
    finally:
        eng.close()
    assert np.array_equal(y, yfin)
    for b in range(len(c.inst)):
        assert all(np.array_equal(a, w) for a, w in zip(got[b].t_events, res[b].t_events)) and np.array_equal(got[b].y, frames[b].T), b
    out = run_sweep_rk23(c.base, c.inst, (0.0, c.t1), c.h0, RTOL, ATOL, y0=c.y0, device=0, t_eval=c.t_eval, events=True)
    plain = run_sweep_rk23(c.base, c.inst, (0.0, c.t1), c.h0, RTOL, ATOL, y0=c.y0, device=0)
    assert len(out) == 8 and len(plain) == 5
    for a, w in zip(out[:5], plain):
        assert np.array_equal(a, w)
    assert np.array_equal(out[0], yfin) and out[1].tolist() == [0] * len(c.inst) and out[2].tolist() == [r.n_accepted for r in ref]
    assert out[3].tolist() == [r.n_rejected for r in ref] and out[5].tolist() == [len(c.t_eval)] * len(c.inst)
    assert np.array_equal(out[6], frames)
    for b in range(len(c.inst)):
        assert len(out[7][b]) == 7 and all(np.array_equal(a, w) for a, w in zip(out[7][b], res[b].t_events)), b


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. large grids: one launch per attempt (rk23_attempt_kernel: 250 cells written per 256-thread window)
# ---------------------------------------------------------------------------------------------------------------------------------
# N: (why this grid, attempts, rejections of scipy RK23 on the oracle)
LARGE = {1025: ("first grid past the one-workgroup window, last tile nearly empty", 62, 5),
         1251: ("one cell past a multiple of 250", 65, 8),
         2500: ("exact multiple of the tile's 250 written cells", 62, 6)}
_LARGE_REF = {}


def _large_reference(oracle, name, N, m, vd, amplitude):
    key = (name, N, m, vd)
    if key not in _LARGE_REF:
        p = scenario(name, N) | ({"dPhi_variable": True} if vd else {})
        y = synthetic_state(p, N, amplitude=amplitude)
        dx2 = ((p["max_depth"] / p["Xstar"]) / N) ** 2
        ref = scipy_rk23(oracle, oracle.params_from_dict(p), N, y, (0.0, m * dx2), 0.5 * dx2, RTOL, ATOL)
        assert ref.status == 0 and ref.margin > MARGIN
        print(f"RK23 large {name} N={N} vd={vd}: scipy attempts {ref.n_accepted + ref.n_rejected} rejected {ref.n_rejected} closest norm {ref.margin:.1e}")
        _LARGE_REF[key] = (p, y, dx2, ref)
    return _LARGE_REF[key]


def _run_device(torch, eq, y, t_span, h0, layout):
    yd = torch.from_numpy(y).cuda()
    if layout == 0:
        res = eq.integrate_rk23_device(yd.data_ptr(), t_span, h0, RTOL, ATOL, layout)
        got = yd
    else:
        yt = torch.zeros(eq.state_doubles(layout), dtype=torch.float64, device="cuda")
        eq.convert_layout_device(yd.data_ptr(), yt.data_ptr(), 0, layout)
        res = eq.integrate_rk23_device(yt.data_ptr(), t_span, h0, RTOL, ATOL, layout)
        got = torch.empty_like(yd)
        eq.convert_layout_device(yt.data_ptr(), got.data_ptr(), layout, 0)
    torch.cuda.synchronize()
    return res, got.cpu().numpy()


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("N,vd", [(1025, False), (1251, False), (2500, False), (2500, True)])
def test_large_grid_against_scipy_both_layouts_both_entries(torch_cuda, oracle, N, vd, layout):
    p, y, dx2, ref = _large_reference(oracle, "A", N, 40, vd, 0.05)
    if not vd:
        assert (ref.n_accepted + ref.n_rejected, ref.n_rejected) == LARGE[N][1:], LARGE[N][0]
    eq = make_model(p)
    try:
        eq.use_stream(torch_cuda.cuda.current_stream().cuda_stream)
        eq.set_option("host_layout", layout)
        res, got = _run_device(torch_cuda, eq, y, (0.0, 40 * dx2), 0.5 * dx2, layout)
        host = eq.integrate_rk23(y, (0.0, 40 * dx2), 0.5 * dx2, RTOL, ATOL, events=False)
    finally:
        eq.close()
    want = (ref.status, ref.n_accepted, ref.n_rejected, ref.nfev)
    assert counts(res) == want and counts(host) == want and res.t_reached == 40 * dx2
    e_dev, e_host = rel_to_max(got, ref.y_final), rel_to_max(host.y_final, ref.y_final)
    print(f"RK23 large N={N} vd={vd} layout={layout}: device entry {e_dev:.2e} host entry {e_host:.2e}")
    assert e_dev <= STATE_TOL and e_host <= STATE_TOL
    assert np.array_equal(got, host.y_final)


def test_large_grid_default_scenario_n5003_and_t_eval_at_n1025(torch_cuda, oracle):
    p, y, dx2, ref = _large_reference(oracle, "default", 5003, 60, False, 0.01)
    assert (ref.n_accepted + ref.n_rejected, ref.n_rejected) == (139, 3)
    eq = make_model(p)
    try:
        res, got = _run_device(torch_cuda, eq, y, (0.0, 60 * dx2), 0.5 * dx2, 0)
    finally:
        eq.close()
    assert counts(res) == (0, ref.n_accepted, ref.n_rejected, ref.nfev)
    e5003 = rel_to_max(got, ref.y_final)
    # five samples, both ends included, at the first grid past the one-workgroup window
    p, y, dx2, _ = _large_reference(oracle, "A", 1025, 40, False, 0.05)
    t1 = 40 * dx2
    te = t1 * np.array([0.0, 0.13, 0.5, 0.77, 1.0])
    ref = scipy_rk23(oracle, oracle.params_from_dict(p), 1025, y, (0.0, t1), 0.5 * dx2, RTOL, ATOL, t_eval=te)
    eq = make_model(p)
    try:
        res = eq.integrate_rk23(y, (0.0, t1), 0.5 * dx2, RTOL, ATOL, t_eval=te)
        cut = eq.integrate_rk23(y, (0.0, t1), 0.5 * dx2, RTOL, ATOL, max_attempts=9, events=False)
    finally:
        eq.close()
    assert counts(res) == (0, ref.n_accepted, ref.n_rejected, ref.nfev) and np.array_equal(res.t, te) and np.array_equal(res.y[:, 0], y)
    worst = max(rel_to_max(res.y[:, j], ref.y_eval[j]) for j in range(len(te)))
    assert [len(e) for e in res.t_events] == [len(e) for e in ref.t_events]
    assert cut.status == 2 and cut.n_accepted + cut.n_rejected == 9 and cut.nfev == 1 + 3 * 9
    print(f"RK23 large N=5003 final {e5003:.2e}; N=1025 frames {worst:.2e}")
    assert e5003 <= STATE_TOL and worst <= STATE_TOL


def test_large_grid_event_root_against_the_golden_trajectory():
    """The porosity-dip state of test_rk45_event_root_on_a_large_grid_every_schedule at N = 1500 to 2200 dx^2: the loop pauses on the sign
    change of zeros_U, the host locates the root by RK23 dense output + Brent (about 1 914 dx^2).  The reference is the golden made by
    tools/make_rk23_goldens.py --large (scipy RK23 on the reference's RHS: 5 133 attempts, 3 rejected, closest norm 1.6e-4 from 1); the
    same call on the oracle takes several seconds, too long for this suite."""
    g = np.load(os.path.join(GOLDEN, "rk23_event_default_N1500.npz"))
    N, t1 = 1500, float(g["t_span"][1])
    assert float(g["err_margin"]) > MARGIN and list(g["n_events"]) == [0, 0, 0, 0, 0, 1, 0]
    assert (int(g["n_accepted"]) + int(g["n_rejected"]), int(g["n_rejected"])) == (5133, 3)
    dx2 = t1 / 2200
    assert 1900 < float(g["t_events"][0]) / dx2 < 1930
    eq = make_model(scenario("default", N))
    try:
        res = eq.integrate_rk23(g["y0"], (0.0, t1), float(g["first_step"]), float(g["rtol"]), float(g["atol"]))
    finally:
        eq.close()
    assert counts(res) == (0, int(g["n_accepted"]), int(g["n_rejected"]), int(g["nfev"]))
    worst_root = roots_close(res.t_events, [g["t_events"][:1] if e == 5 else np.empty(0) for e in range(7)], t1)
    err = rel_to_max(res.y_final, g["y_final"])
    print(f"RK23 large event N=1500: final {err:.2e} root |dt|/t1 {worst_root:.2e}")
    assert err <= STATE_TOL
