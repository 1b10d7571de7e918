"""RK45 sweeps with events (marl_sweep_rk45_events_dev, rk45_sweep_roots_kernel): the root times of the reference's seven monitors
(marlpde/Evolve_scenario.py:118-145, 175-177; solve_ivp(..., events=[7])) located inside the sweep kernel by Brent's method on dense-output
replays of the accepted step, against the CPU oracle's t_events (oracle/marl_oracle.c:486-497, orc_brent :357-393).

States: the scenario's uniform initial values with Gaussian bumps b(c, w) = exp(-((x - cL) / (wL))^2), x = (i + 1/2) L / N:
    phi_dip=d   Phi = PhiIni - d b(0.5, 0.08)                       zeros_U (monitor 5) crosses zero once
    ca_low=v    CA = CAIni - (CAIni - v) b(0.2, 0.08)               min(y) and min CA (monitors 0, 1) cross zero in the SAME step
    sum_top=s   CA = CAIni + (s - CAIni - CCIni) b(0.7, 0.05)       max(CA + CC) - 1 (monitor 3) crosses zero
Every run: rtol 1e-5, atol 1e-7, first_step = 0.5 dx^2, t1 = m dx^2.  What the oracle does on these inputs (which monitors fire, in which
step, where) is asserted where the references are made (`_reference`), so that a changed input cannot silently test nothing.

Root-time bound, per monitor: |t - t_oracle| <= rtol |t_oracle| + atol, atol = 1e-12 t1 - the bound of the single-run tests
(tests/test_gpu_parity.py::test_rk45_event_root_matches_oracle).  `measured` is the worst |t - t_oracle| / t1 over all shapes and instances
of this file on an MI355X (printed per root, pytest -rA).  No bound may exceed 1e-6 t1."""
import ctypes as C

import numpy as np
import pytest

from common import rel_to_max, scenario

pytestmark = pytest.mark.gpu

ROOT_TOL = {
    # monitor                                bound                     measured on MI355X: worst |dt| / t1 (n: roots compared)
    0: dict(rtol=1e-9, atol_t1=1e-12, measured=3.4e-15),   # no_negatives (min y), n = 4; crosses with min CA, in the same step
    1: dict(rtol=1e-9, atol_t1=1e-12, measured=3.4e-15),   # zeros_CA (min CA), n = 4: the shallow slope needs no wider bound
    2: dict(rtol=1e-9, atol_t1=1e-12, measured=None),      # zeros_CC: never fires here
    3: dict(rtol=1e-9, atol_t1=1e-12, measured=2.1e-12),   # ones_CA_plus_CC, n = 2 (bound there: 9.2e-10 t1)
    4: dict(rtol=1e-9, atol_t1=1e-12, measured=None),      # ones_Phi: never fires here
    5: dict(rtol=1e-9, atol_t1=1e-12, measured=9.3e-14),   # zeros_U, n = 10
    6: dict(rtol=1e-9, atol_t1=1e-12, measured=None),      # zeros_W: never fires here
}
ROOT_CAP = 1e-6            # of t1: a cap on any bound above, not a measurement
FRAME_TOL = 1e-9           # rel_to_max of frames and final states (tests/test_gpu_sweep_frames.py)
T_FRAC = np.array([0.0, 0.1, 0.5, 1.0])
RTOL, ATOL = 1e-5, 1e-7

_N200 = [({}, {}), (dict(ca_low=-1e-3), {}), (dict(phi_dip=0.038, sum_top=1.0005), {}), (dict(phi_dip=0.04), {}), (dict(phi_dip=0.042), {}),
         (dict(phi_dip=0.04), dict(k3=0.05, k4=0.05)), (dict(ca_low=-1e-3), dict(Phi0=0.7))]
# name -> (N, m, [(state, parameter overrides)], scenario extras,
#          oracle facts per instance: [(monitor, root / t1, index of the accepted step that holds it)], accepted steps of instance 0)
SHAPES = {
    "N200": (200, 250, _N200, {},
             [[], [(0, 0.815, 364), (1, 0.815, 364)], [(3, 0.923, 413), (5, 0.038, 18)], [(5, 0.135, 61)], [(5, 0.336, 150)], [(5, 0.260, 116)],
              [(0, 0.271, 121), (1, 0.271, 121)]], 448),
    "N200-vd": (200, 250, _N200[:5], {"dPhi_variable": True},
                [[], [(0, 0.8147, 364), (1, 0.8147, 364)], [(3, 0.9235, 413), (5, 0.0379, 18)], [(5, 0.135, 61)], [(5, 0.339, 151)]], 448),
    "N513": (513, 1500, [(dict(ca_low=-3e-4), {}), (dict(phi_dip=0.04), {}), ({}, {})], {},
             [[(0, 0.707, 1893), (1, 0.707, 1893)], [(5, 0.149, 394)], []], 2689),
    "N1024": (1024, 1200, [(dict(phi_dip=0.04), {}), ({}, {})], {}, [[(5, 0.743, 1573)], []], 2124),
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
        self.N, m, pairs, extra, self.facts, self.accepted0 = SHAPES[name]
        self.base = scenario("default", self.N) | extra
        self.inst = [dict(ov) for _, ov in pairs]
        self.dx2 = ((self.base["max_depth"] / self.base["Xstar"]) / self.N) ** 2
        self.t1 = m * self.dx2
        self.h0 = 0.5 * self.dx2
        self.t_eval = self.t1 * T_FRAC
        self.y0 = np.stack([bump_state(self.base | ov, self.N, **st) for st, ov in pairs])

    def run(self, torch, events=True, max_events=64, t_eval="case", max_attempts=0, order=None):
        """The sweep through LMAHeureuxPorosityDiff.sweep_rk45_device: (results, final states, frames [instance][sample][5N] or None)."""
        from marlpde_amd.LHeureux_model import LMAHeureuxPorosityDiff
        order = list(range(len(self.inst))) if order is None else order
        eq = LMAHeureuxPorosityDiff.from_scenario(self.base, device=0, instances=[self.inst[i] for i in order])
        eq.use_stream(torch.cuda.current_stream().cuda_stream)
        te = self.t_eval if isinstance(t_eval, str) else t_eval
        yd = torch.from_numpy(np.ascontiguousarray(self.y0[order])).cuda()
        frames, more = None, {}
        try:
            if te is not None:
                frames = torch.full((len(order), len(te), 5 * self.N), float("nan"), dtype=torch.float64, device="cuda")
                more = dict(t_eval=te, y_eval_dev_ptr=frames.data_ptr())
            if events is not None:
                more |= dict(events=events, max_events=max_events)
            res = eq.sweep_rk45_device(yd.data_ptr(), (0.0, self.t1), self.h0, RTOL, ATOL, max_attempts, **more)
            torch.cuda.synchronize()
        finally:
            eq.close()
        return res, yd.cpu().numpy(), None if frames is None else frames.cpu().numpy()

    def run_raw(self, torch, max_events):
        """The C entry itself: (statistics, the whole t_events buffer [instance][7][max_events])."""
        from marlpde_amd._abi import MarlStats
        from marlpde_amd.LHeureux_model import LMAHeureuxPorosityDiff
        eq = LMAHeureuxPorosityDiff.from_scenario(self.base, device=0, instances=self.inst)
        eq.use_stream(torch.cuda.current_stream().cuda_stream)
        yd = torch.from_numpy(np.ascontiguousarray(self.y0)).cuda()
        frames = torch.empty((len(self.inst), len(self.t_eval), 5 * self.N), dtype=torch.float64, device="cuda")
        stats = (MarlStats * len(self.inst))()
        n_done = np.zeros(len(self.inst), dtype=np.int64)
        tev = np.full((len(self.inst), 7, max_events), 123.0)     # the entry fills it with NaN itself
        try:
            rc = eq._lib.marl_sweep_rk45_events_dev(eq._ctx, C.c_void_p(yd.data_ptr()), 0.0, self.t1, self.h0, RTOL, ATOL, 0,
                                                    self.t_eval.ctypes.data_as(C.c_void_p), len(self.t_eval), C.c_void_p(frames.data_ptr()),
                                                    n_done.ctypes.data_as(C.c_void_p), tev.ctypes.data_as(C.c_void_p), max_events, stats)
            assert rc == 0
        finally:
            eq.close()
        return stats, tev


_REF, _GOT = {}, {}


def _reference(oracle, name, max_attempts=0):
    """The oracle's run of every instance of a shape, made once per session and never changed: list of (y_final, stats, step_times, y_eval,
    t_events).  The facts listed in SHAPES are asserted on the full runs."""
    key = (name, max_attempts)
    if key not in _REF:
        c = Case(name)
        out = []
        for b, inst in enumerate(c.inst):
            P = oracle.params_from_dict(c.base | inst)
            yf, st, steps, ye, tev = oracle.rk45(P, c.N, c.y0[b], 0.0, c.t1, c.h0, RTOL, ATOL, t_eval=c.t_eval, max_attempts=max_attempts,
                                                 max_steps_out=4096, max_events=64)
            for a in (yf, steps, ye, *tev):
                a.setflags(write=False)
            out.append((yf, st, steps, ye, tev))
        if max_attempts == 0:
            assert out[0][1].n_accepted == c.accepted0
            for b, (yf, st, steps, ye, tev) in enumerate(out):
                assert st.status == 0 and steps[-1] == c.t1, b
                found = [(e, float(t)) for e in range(7) for t in tev[e]]
                assert [e for e, _ in found] == [e for e, _, _ in c.facts[b]], (b, found)
                assert list(st.n_events) == [sum(1 for e, _, _ in c.facts[b] if e == k) for k in range(7)], b
                for (e, t), (_, frac, step) in zip(found, c.facts[b]):
                    assert abs(t / c.t1 - frac) < 1e-3 and int(np.searchsorted(steps, t, side="left")) == step, (b, e, t / c.t1)
        _REF[key] = (c, out)
    return _REF[key]


def _root_ok(e, got, ref, t1):
    tol = ROOT_TOL[e]
    bound = tol["rtol"] * abs(ref) + tol["atol_t1"] * t1
    assert bound <= ROOT_CAP * t1
    return abs(got - ref) <= bound


def _stats_key(r):
    return (r.status, r.n_accepted, r.n_rejected, r.nfev, r.t_reached, r.h_next, tuple(r.n_events), tuple(r.event_values))


def _check_against(c, ref, res, yfin, frames, label):
    """Decisions, counts, roots, frames and final state of a sweep with events against the oracle's runs."""
    bad = []
    for b, (yf, st, steps, ye, tev) in enumerate(ref):
        assert (res[b].status, res[b].n_accepted, res[b].n_rejected, res[b].nfev) == (st.status, st.n_accepted, st.n_rejected, st.nfev), b
        assert list(res[b].n_events) == list(st.n_events), b
        assert [len(t) for t in res[b].t_events] == [len(t) for t in tev], b
        for e in range(7):
            for got, want in zip(res[b].t_events[e], tev[e]):
                print(f"ROOT {label} instance {b} monitor {e}: t/t1 {want / c.t1:.6f} |dt|/t1 {abs(got - want) / c.t1:.2e}")
                if not _root_ok(e, got, want, c.t1):
                    bad.append((b, e, got, want))
        if frames is not None:
            k = len(res[b].t)
            assert k == int(np.searchsorted(c.t_eval, st.t, side="right")), b
            for i in range(k):
                assert rel_to_max(frames[b, i], ye[i]) <= FRAME_TOL, (b, i)
            assert np.all(np.isnan(frames[b, k:])), b
        assert rel_to_max(yfin[b], yf) <= FRAME_TOL, b
    assert not bad, bad


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _with_events(torch, oracle, name):
    """The sweep of a shape with events and the shape's t_eval, made once per session: (case, oracle runs, results, final states, frames)."""
    c, ref = _reference(oracle, name)
    if name not in _GOT:
        _GOT[name] = c.run(torch)
    return (c, ref) + _GOT[name]


@pytest.mark.parametrize("name", ["N200", "N200-vd", "N513", "N1024"])
def test_roots_against_the_oracle_and_locating_them_leaves_the_integration_alone(torch_cuda, oracle, name):
    """(1) statistics, counts, root times, frames and final state against the oracle; the raw buffer is NaN beyond the counts.
    (2) the same sweep without events (rk45_sweep_eval_kernel): bit-identical final states and frames, every statistic equal."""
    c, ref, res, yfin, frames = _with_events(torch_cuda, oracle, name)
    _check_against(c, ref, res, yfin, frames, name)
    stats, raw = c.run_raw(torch_cuda, 5)
    for b, r in enumerate(res):
        assert list(stats[b].n_events) == list(r.n_events), b
        for e in range(7):
            k = min(int(r.n_events[e]), 5)
            assert np.array_equal(raw[b, e, :k], r.t_events[e][:k]) and np.all(np.isnan(raw[b, e, k:])), (b, e)
    plain, yplain, fplain = c.run(torch_cuda, events=False)
    assert np.array_equal(yplain, yfin) and np.array_equal(fplain, frames, equal_nan=True)
    for b in range(len(c.inst)):
        assert _stats_key(plain[b]) == _stats_key(res[b]), b
        assert plain[b].t_events is None and np.array_equal(plain[b].t, res[b].t)


def test_max_events_cap_and_the_entries_it_falls_back_to(torch_cuda, oracle):
    c, ref, res, yfin, frames = _with_events(torch_cuda, oracle, "N200")
    # one slot per monitor: every count unchanged, one root per fired monitor (no monitor fires twice here, so every root is stored)
    one, y1, f1 = c.run(torch_cuda, max_events=1)
    assert np.array_equal(y1, yfin) and np.array_equal(f1, frames, equal_nan=True)
    for b in range(len(c.inst)):
        assert _stats_key(one[b]) == _stats_key(res[b]), b
        assert [len(t) for t in one[b].t_events] == [min(int(n), 1) for n in res[b].n_events], b
        assert all(np.array_equal(a, w[:1]) for a, w in zip(one[b].t_events, res[b].t_events)), b
    # max_events = 0 / events = False / no keyword: what the eval entry returns
    plain, yp, fp = c.run(torch_cuda, events=None)
    for kw in (dict(max_events=0), dict(events=False)):
        got, y, f = c.run(torch_cuda, **kw)
        assert np.array_equal(y, yp) and np.array_equal(f, fp, equal_nan=True)
        for b in range(len(c.inst)):
            assert _stats_key(got[b]) == _stats_key(plain[b]) and got[b].t_events is None and np.array_equal(got[b].t, plain[b].t), b
    # no samples, roots asked for: the roots of the run with samples
    bare, yb, none = c.run(torch_cuda, t_eval=None)
    assert none is None and np.array_equal(yb, yfin)
    for b in range(len(c.inst)):
        assert _stats_key(bare[b]) == _stats_key(res[b]) and bare[b].t is None, b
        assert all(np.array_equal(a, w) for a, w in zip(bare[b].t_events, res[b].t_events)), b


def test_roots_do_not_depend_on_the_position_in_the_batch(torch_cuda, oracle):
    c, ref, res, yfin, frames = _with_events(torch_cuda, oracle, "N200")
    order = list(range(len(c.inst)))[::-1]
    rev, yrev, frev = c.run(torch_cuda, order=order)
    for pos, b in enumerate(order):
        assert np.array_equal(yrev[pos], yfin[b]) and np.array_equal(frev[pos], frames[b], equal_nan=True), b
        assert _stats_key(rev[pos]) == _stats_key(res[b]), b
        assert all(np.array_equal(a, w) for a, w in zip(rev[pos].t_events, res[b].t_events)), b
    assert sum(len(t) for r in res for t in r.t_events) == 9


def test_attempt_budget_keeps_the_roots_reached(torch_cuda, oracle):
    """max_attempts = 100: every instance stops with status 2 after the zeros_U root of instance 3 (0.135 t1) and before that of
    instance 5 (0.260 t1) - asserted on the oracle; the roots reached are there, the others are not."""
    c, ref = _reference(oracle, "N200", max_attempts=100)
    assert all(st.status == 2 for _, st, _, _, _ in ref)
    assert [len(t) for t in ref[3][4]] == [0, 0, 0, 0, 0, 1, 0] and 0.13 < ref[3][4][5][0] / c.t1 < 0.14 and ref[3][1].t > ref[3][4][5][0]
    assert [len(t) for t in ref[5][4]] == [0] * 7 and ref[5][1].t < 0.26 * c.t1
    res, yfin, frames = c.run(torch_cuda, max_attempts=100)
    _check_against(c, ref, res, yfin, frames, "N200 budget")
    assert [sum(len(t) for t in r.t_events) for r in res] == [sum(len(t) for t in tev) for _, _, _, _, tev in ref]


def test_engine_and_driver_return_the_roots(torch_cuda, oracle):
    from marlpde_amd.sweep import HipSweepEngine, run_sweep_rk45
    c, ref, res, yfin, frames = _with_events(torch_cuda, oracle, "N200")
    eng = HipSweepEngine(c.base, c.inst, 0)
    try:
        y, got = eng.integrate_rk45(c.y0, (0.0, c.t1), c.h0, RTOL, ATOL, 0, t_eval=c.t_eval, events=True)
        y2, got2 = eng.integrate_rk45(c.y0, (0.0, c.t1), c.h0, RTOL, ATOL, 0, events=True, max_events=3)
    finally:
        eng.close()
    assert np.array_equal(y, yfin) and np.array_equal(y2, yfin)
    for b in range(len(c.inst)):
        assert all(np.array_equal(a, w) for a, w in zip(got[b].t_events, res[b].t_events)), b
        assert all(np.array_equal(a, w) for a, w in zip(got2[b].t_events, res[b].t_events)), b
        assert np.array_equal(got[b].y, frames[b].T) and got2[b].t is None
    out = run_sweep_rk45(c.base, c.inst, (0.0, c.t1), c.h0, RTOL, ATOL, y0=c.y0, device=0, t_eval=c.t_eval, events=True)
    plain = run_sweep_rk45(c.base, c.inst, (0.0, c.t1), c.h0, RTOL, ATOL, y0=c.y0, device=0, t_eval=c.t_eval)
    assert len(out) == 8 and len(plain) == 7
    for a, w in zip(out[:7], plain):
        assert np.array_equal(a, w, equal_nan=True)
    assert np.array_equal(out[0], yfin) and len(out[7]) == len(c.inst)
    for b in range(len(c.inst)):
        assert len(out[7][b]) == 7 and all(np.array_equal(a, w) for a, w in zip(out[7][b], res[b].t_events)), b
