"""RK45 sweeps with t_eval (marl_sweep_rk45_eval_dev, rk45_sweep_eval_kernel): the frames that solve_ivp(..., t_eval=) fills
(marlpde/Evolve_scenario.py:104-109) written by dense output inside the sweep kernel, against the CPU oracle's run with the same t_eval.

The shapes are the smallest that reach every window of the sweep (256 / 1024 with idle lanes / 1024 full, the last with fields of y parked
in LDS); the sample times put three samples into one step, two into the first (one of them t0) and one on t1.  That the oracle's runs
really have these properties is asserted on its step times where the references are made (`_reference`)."""
import numpy as np
import pytest

from common import rel_to_max, scenario, synthetic_state

pytestmark = pytest.mark.gpu

T_FRAC = np.array([0.0, 0.004, 0.31, 0.5, 0.50001, 0.50002, 0.83, 1.0])
FRAME_TOL = 1e-9        # the bound of the existing sweep tests against the oracle (tests/test_gpu_parity.py)


def _instances_a(n):
    return [{"Phi0": 0.55 + 0.04 * i, "PhiIni": 0.5 + 0.03 * i, "PhiNR": 0.5 + 0.03 * i} for i in range(n)]


def _instances_default(n):
    rng = np.random.default_rng(3)
    return [{"Phi0": float(a), "PhiIni": float(b), "PhiNR": float(b), "k3": float(k), "k4": float(k)}
            for a, b, k in zip(rng.uniform(0.5, 0.8, n), rng.uniform(0.5, 0.8, n), 10 ** rng.uniform(-2, -1, n))]


def _shape(name):
    """(base scenario, instances, first_step / dx^2, rtol, atol, amplitude)"""
    if name == "A-200":
        return scenario("A", 200), _instances_a(5), 0.3, 1e-4, 1e-6, 0.03
    if name == "A-513":
        return scenario("A", 513), _instances_a(2), 0.3, 1e-4, 1e-6, 0.03
    if name == "A-200-vd":
        return scenario("A", 200) | {"dPhi_variable": True}, _instances_a(3), 0.3, 1e-4, 1e-6, 0.03
    if name == "default-1024":
        return scenario("default", 1024), _instances_default(6), 0.5, 1e-3, 1e-3, 0.02
    raise KeyError(name)


class Case:
    def __init__(self, name):
        self.name = name
        self.base, self.inst, hf, self.rtol, self.atol, amp = _shape(name)
        self.N = int(self.base["N"])
        self.dx2 = ((self.base["max_depth"] / self.base["Xstar"]) / self.N) ** 2
        self.t1 = 60 * self.dx2
        self.h0 = hf * self.dx2
        self.t_eval = self.t1 * T_FRAC
        self.y0 = np.stack([synthetic_state(self.base | i, self.N, amplitude=amp) for i in self.inst])

    def model(self, torch, inst=None):
        from marlpde_amd.LHeureux_model import LMAHeureuxPorosityDiff
        eq = LMAHeureuxPorosityDiff.from_scenario(self.base, device=0, instances=self.inst if inst is None else inst)
        eq.use_stream(torch.cuda.current_stream().cuda_stream)
        return eq

    def run(self, torch, t_eval="case", max_attempts=0, inst=None, y0=None, fill=None, t_span=None):
        """The sweep through the Python surface: (results, final states, frames [instance][sample][5N] or None)."""
        eq = self.model(torch, inst)
        y0 = self.y0 if y0 is None else y0
        te = self.t_eval if isinstance(t_eval, str) else t_eval
        yd = torch.from_numpy(np.ascontiguousarray(y0)).cuda()
        frames = None
        try:
            if te is None:
                res = eq.sweep_rk45_device(yd.data_ptr(), t_span or (0.0, self.t1), self.h0, self.rtol, self.atol, max_attempts)
            else:
                frames = torch.full((len(y0), max(len(te), 1), 5 * self.N), float("nan") if fill is None else fill, dtype=torch.float64, device="cuda")
                res = eq.sweep_rk45_device(yd.data_ptr(), t_span or (0.0, self.t1), self.h0, self.rtol, self.atol, max_attempts, t_eval=te,
                                           y_eval_dev_ptr=frames.data_ptr())
            torch.cuda.synchronize()
        finally:
            eq.close()
        return res, yd.cpu().numpy(), None if frames is None else frames.cpu().numpy()


_REF = {}


def _reference(oracle, name, max_attempts=0):
    """The oracle's run of every instance of a shape with the shape's t_eval, made once per session and never changed:
    list of (y_final, stats, step_times, y_eval)."""
    key = (name, max_attempts)
    if key not in _REF:
        c = Case(name)
        out = []
        for b, inst in enumerate(c.inst):
            P = oracle.params_from_dict(c.base | inst)
            yf, st, steps, ye, _ = oracle.rk45(P, c.N, c.y0[b], 0.0, c.t1, c.h0, c.rtol, c.atol, t_eval=c.t_eval, max_attempts=max_attempts,
                                               max_steps_out=4096)
            for a in (yf, steps, ye):
                a.setflags(write=False)
            out.append((yf, st, steps, ye))
        _REF[key] = (c, out)
    return _REF[key]


def _samples_per_step(t_eval, steps):
    """How many samples each accepted step holds: those in (t_old, t], and t0 itself in the first (ivp.py:706-723)."""
    edges = np.concatenate([[-np.inf], steps])
    return np.array([np.count_nonzero((t_eval > lo) & (t_eval <= hi)) for lo, hi in zip(edges[:-1], edges[1:])])


def check_full_run_preconditions(c, ref):
    """What the shapes and sample times were chosen for, asserted on the oracle's own step times."""
    sequences = set()
    for yf, st, steps, ye in ref:
        assert st.status == 0 and steps[-1] == c.t1
        assert 66 <= st.n_accepted <= 92 and len(steps) == st.n_accepted
        per = _samples_per_step(c.t_eval, steps)
        assert per.sum() == len(c.t_eval)
        assert per.max() == 3, "some step holds three samples"
        assert per[0] == 2 and c.t_eval[0] == 0.0, "the first step holds two samples, one of them t0"
        sequences.add((st.n_accepted, st.n_rejected, tuple(steps)))
    assert len(sequences) == len(ref), "every instance takes its own accept / reject sequence"


def check_budget_preconditions(c, ref):
    reached = []
    for yf, st, steps, ye in ref:
        assert st.status == 2
        reached.append(int(np.searchsorted(c.t_eval, st.t, side="right")))
    assert set(reached) == {2, 3}, reached
    return reached


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _against_oracle(torch, oracle, name):
    c, ref = _reference(oracle, name)
    check_full_run_preconditions(c, ref)
    res, yfin, frames = c.run(torch)
    for b, (yf, st, steps, ye) in enumerate(ref):
        assert (res[b].status, res[b].n_accepted, res[b].n_rejected) == (st.status, st.n_accepted, st.n_rejected), b
        assert len(res[b].t) == len(c.t_eval) and np.array_equal(res[b].t, c.t_eval), b
        assert np.array_equal(frames[b, 0], c.y0[b]), b
        errs = [rel_to_max(frames[b, i], ye[i]) for i in range(len(c.t_eval))] + [rel_to_max(yfin[b], yf)]
        print(f"FRAMES {name} instance {b}: accepted {st.n_accepted} rejected {st.n_rejected} rel_to_max per frame "
              + " ".join(f"{e:.1e}" for e in errs[:-1]) + f" final {errs[-1]:.1e}")
        assert max(errs) <= FRAME_TOL, (b, errs)
    return c, res, yfin, frames


@pytest.mark.parametrize("name", ["A-200", "A-513", "default-1024"])
def test_frames_against_the_oracle_and_sampling_leaves_the_integration_alone(torch_cuda, oracle, name):
    """(1) decisions, frames and final state against the oracle's run with the same t_eval; frame 0 is y0 bit for bit.
    (2) the same call without t_eval (rk45_sweep_kernel): bit-identical final states, every statistic equal - nfev included,
    scipy's dense output costs no evaluation."""
    c, res, yfin, frames = _against_oracle(torch_cuda, oracle, name)
    plain, yplain, none = c.run(torch_cuda, t_eval=None)
    assert none is None and np.array_equal(yplain, yfin)
    key = lambda r: (r.status, r.n_accepted, r.n_rejected, r.nfev, r.t_reached, r.h_next, tuple(r.n_events), tuple(r.event_values))  # noqa: E731
    for b in range(len(c.inst)):
        assert key(plain[b]) == key(res[b]), b
        assert plain[b].t is None


@pytest.mark.parametrize("name", ["A-200", "default-1024"])
def test_attempt_budget_writes_the_frames_reached_and_touches_no_other(torch_cuda, oracle, name):
    """max_attempts = 25: every instance stops with status 2 after 2 or 3 of the 8 samples; n_done says which, the frames below it are
    the oracle's and the memory above it still holds the NaN it was filled with."""
    c, ref = _reference(oracle, name, max_attempts=25)
    reached = check_budget_preconditions(c, ref)
    res, yfin, frames = c.run(torch_cuda, max_attempts=25)
    for b, (yf, st, steps, ye) in enumerate(ref):
        assert (res[b].status, res[b].n_accepted, res[b].n_rejected) == (2, st.n_accepted, st.n_rejected), b
        k = int(np.searchsorted(c.t_eval, res[b].t_reached, side="right"))
        assert len(res[b].t) == k == reached[b] and np.array_equal(res[b].t, c.t_eval[:k]), b
        assert np.all(np.isnan(frames[b, k:])), b
        assert np.array_equal(frames[b, 0], c.y0[b]), b
        for i in range(k):
            assert rel_to_max(frames[b, i], ye[i]) <= FRAME_TOL, (b, i)
        assert rel_to_max(yfin[b], yf) <= FRAME_TOL, b


def test_frames_do_not_depend_on_the_position_in_the_batch(torch_cuda):
    """One parameter block first, in the middle and last, among different neighbours: its frames are bit-identical."""
    c = Case("A-200")
    me = 2
    got = []
    for pos, order in ((0, [me, 0, 1, 3, 4]), (2, [3, 4, me, 1, 0]), (4, [1, 3, 0, 4, me])):
        res, yfin, frames = c.run(torch_cuda, inst=[c.inst[i] for i in order], y0=c.y0[order])
        assert order[pos] == me and len(res[pos].t) == len(c.t_eval)
        got.append((frames[pos], yfin[pos], res[pos].n_accepted, res[pos].n_rejected))
    for other in got[1:]:
        assert np.array_equal(other[0], got[0][0]) and np.array_equal(other[1], got[0][1]) and other[2:] == got[0][2:]
    assert not np.isnan(got[0][0]).any()


def test_frames_with_the_time_varying_porosity_diffusion(torch_cuda, oracle):
    """dPhi_variable = 1 (rk45_sweep_eval_kernel<256, true>) against the oracle."""
    _against_oracle(torch_cuda, oracle, "A-200-vd")


def test_edges_of_the_entry(torch_cuda):
    from marlpde_amd._abi import MarlError
    torch = torch_cuda
    c = Case("A-200")
    plain, yplain, _ = c.run(torch, t_eval=None)
    key = lambda r: (r.status, r.n_accepted, r.n_rejected, r.nfev, r.t_reached, r.h_next)  # noqa: E731
    # no samples: the plain sweep (n_eval = 0 launches rk45_sweep_kernel itself)
    res, y, frames = c.run(torch, t_eval=np.empty(0))
    assert np.array_equal(y, yplain) and [key(r) for r in res] == [key(r) for r in plain]
    assert all(r.t is not None and len(r.t) == 0 for r in res) and np.all(np.isnan(frames))
    # t_span = (0, 0): no step; the sample at t0 is y0
    res, y, frames = c.run(torch, t_eval=np.array([0.0]), t_span=(0.0, 0.0))
    assert all(r.status == 0 and r.n_accepted == 0 and list(r.t) == [0.0] for r in res)
    assert np.array_equal(frames[:, 0], c.y0) and np.array_equal(y, c.y0)
    # unsorted, repeated or out-of-span samples
    for bad in ([0.5 * c.t1, 0.25 * c.t1], [0.5 * c.t1, 0.5 * c.t1], [-1e-9, 0.5 * c.t1], [0.5 * c.t1, 1.0000001 * c.t1], [float("nan")]):
        with pytest.raises(MarlError, match="t_eval"):
            c.run(torch, t_eval=np.array(bad))
    # a grid that does not fit one workgroup: the plain sweep's refusal
    big = Case("A-200")
    big.base = scenario("A", 1025)
    big.N, big.inst = 1025, _instances_a(2)
    big.y0 = np.stack([synthetic_state(big.base | i, 1025, amplitude=0.03) for i in big.inst])
    errors = []
    for te in (None, big.t_eval):
        with pytest.raises(MarlError, match="exceeds the largest one-workgroup window") as e:
            big.run(torch, t_eval=te)
        errors.append(str(e.value).split(":", 1)[-1])
    assert errors[0] == errors[1]


def test_engine_returns_the_time_series_like_a_single_run(torch_cuda, oracle):
    """HipSweepEngine.integrate_rk45(t_eval=...): .t (n_t,) and .y (5N, n_t) per instance, as a single run's RK45Result."""
    from marlpde_amd.sweep import HipSweepEngine
    c, ref = _reference(oracle, "A-200")
    eng = HipSweepEngine(c.base, c.inst, 0)
    try:
        y, res = eng.integrate_rk45(c.y0, (0.0, c.t1), c.h0, c.rtol, c.atol, 0, t_eval=c.t_eval)
        y25, res25 = eng.integrate_rk45(c.y0, (0.0, c.t1), c.h0, c.rtol, c.atol, 25, t_eval=c.t_eval)
    finally:
        eng.close()
    assert y.shape == (len(c.inst), 5 * c.N)
    for b, (yf, st, steps, ye) in enumerate(ref):
        assert res[b].t.shape == (8,) and res[b].y.shape == (5 * c.N, 8)
        assert rel_to_max(y[b], yf) <= FRAME_TOL
        for i in range(8):
            assert rel_to_max(res[b].y[:, i], ye[i]) <= FRAME_TOL
        k = len(res25[b].t)
        assert 0 < k < 8 and res25[b].y.shape == (5 * c.N, k) and np.array_equal(res25[b].y, res[b].y[:, :k])
