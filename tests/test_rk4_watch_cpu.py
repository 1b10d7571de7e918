"""Monitored fixed-step RK4, the drivers that need no GPU: the two C entries are declared, bound and exported; run_sweep_rk4 shards,
gathers and orders states, counts, frames and roots in the tuple layout of run_sweep_rk45 (what is under test is marlpde_amd/sweep.py;
the arithmetic comes from an engine double defined here: the CPU oracle's RK4 stepped under the rules of csrc/marl_rk4_watch_ctl.h,
tests/rk4_watch_ref.py); integrate_equations(method="RK4") raises every complaint about its schedule before a model exists and hands
an on-grid schedule to the model."""
import ctypes as C
import os

import numpy as np
import pytest

import rk4_watch_ref as ref
from common import scenario
from test_gpu_sweep_radau_frames import INSTANCES, _base, _y0
from test_sweep_frames_cpu import _spawn
from test_sweep_rk23_cpu import _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entries_are_declared_bound_and_exported():
    from marlpde_amd import _abi
    header = open(os.path.join(ROOT, "include", "marl_hip.h")).read()
    lib = _abi.load()
    tail = ["int64_t nsteps", "const int64_t* frame_steps", "int64_t n_frames"]
    assert _declared(header, "marl_sweep_rk4_watch_dev") == ["marl_ctx* ctx", "double* y_dev", "double t0", "const double* dt", *tail, "double* frames_dev",
                                                             "int64_t* n_done", "double* t_events", "int64_t max_events", "marl_stats* stats"]
    assert _declared(header, "marl_integrate_rk4_watch") == ["marl_ctx* ctx", "double* y", "double t0", "double dt", *tail, "double* y_frames",
                                                             "int64_t* n_done", "double* t_events", "int64_t max_events", "marl_stats* stats"]
    P, D, L, S = _abi._P, _abi._D, _abi._L, C.POINTER(_abi.MarlStats)
    assert _abi.PROTOTYPES["marl_sweep_rk4_watch_dev"] == (_abi._I, [P, P, D, P, L, P, L, P, P, P, L, S])
    assert _abi.PROTOTYPES["marl_integrate_rk4_watch"] == (_abi._I, [P, P, D, D, L, P, L, P, P, P, L, S])
    for name in ("marl_sweep_rk4_watch_dev", "marl_integrate_rk4_watch"):
        entry = getattr(lib, name)
        assert entry(*[a() for a in entry.argtypes]) == -1, name      # zeros and null pointers, no context: -1, nothing touched
    # the plain entries stand where they stood, in front of the new ones
    assert header.index("int marl_sweep_rk4_dev(") < header.index("int marl_sweep_rk4_watch_dev(") < header.index("int marl_integrate_rk4_watch(")
    from marlpde_amd._abi import MarlStats
    from marlpde_amd.LHeureux_model import RK45Result
    st = MarlStats()
    st.status = -2
    assert "non-finite" in RK45Result(st).message and RK45Result(MarlStats()).message.startswith("The solver successfully")


# ---- run_sweep_rk4 ------------------------------------------------------------------------------------------------------------------
N = 64
NSTEPS = 2800
DTS = np.array([1e-5, 5e-6, 5e-6, 5e-6, 5e-6])      # instance 0 goes non-finite after two steps; instance 4 has a root of ones_Phi and of zeros_W
FRAME_STEPS = (0, 1, 2000, 2750, 2800)


class OracleRk4Engine:
    """Test double with HipSweepEngine's interface: every instance by the oracle's RK4 under the watch rules.  It notes what reached it."""
    calls = []

    def __init__(self, base_parms, instances):
        from oracle import oracle as orc
        self.N = int(base_parms["N"])
        self.P = [orc.params_from_dict(base_parms | inst) for inst in instances]

    def integrate_rk4_watch(self, y0, dt, nsteps, t0=0.0, **more):
        from marlpde_amd._abi import MarlStats
        from marlpde_amd.LHeureux_model import RK45Result, terminal_counts
        type(self).calls.append(sorted(more))
        fs, events, max_events = more.get("frame_steps"), more.get("events", False), more.get("max_events", 64)
        lim = terminal_counts(more["terminal"]) if "terminal" in more else None
        assert len(dt) == len(self.P) == len(y0)
        ys, res = [], []
        for P, y, h in zip(self.P, y0, dt):
            w, yf, frames = ref.oracle_run(P, self.N, y, h, nsteps, t0, () if fs is None else list(fs), lim, max_events if events else None)
            st = MarlStats()
            st.status, st.n_accepted, st.nfev, st.t = w.status, w.steps, 4 * w.steps, w.t
            for e in range(7):
                st.n_events[e] = w.n_events[e]
            ys.append(yf)
            k = w.next_frame
            res.append(RK45Result(st, None if fs is None else t0 + np.asarray(fs[:k]) * h,
                                  None if fs is None else np.stack([frames[j] for j in range(k)], axis=1).reshape(5 * self.N, k),
                                  [np.array(t) for t in w.t_events] if events else None))
        return np.array(ys).reshape(len(self.P), 5 * self.N), res

    def close(self):
        pass


def _worker(rank, world):
    from marlpde_amd.sweep import assign, run_sweep_rk4
    base = _base(N)
    y0 = _y0(base, INSTANCES)
    factory = lambda bp, inst: OracleRk4Engine(bp, inst)  # noqa: E731
    kw = dict(y0=y0, engine_factory=factory, balance="round_robin")    # the gathered order differs from the arrival order
    OracleRk4Engine.calls = []
    out = {"plain": run_sweep_rk4(base, INSTANCES, DTS, NSTEPS, **kw),
           "frames": run_sweep_rk4(base, INSTANCES, DTS, NSTEPS, **kw, frame_steps=FRAME_STEPS),
           "events": run_sweep_rk4(base, INSTANCES, DTS, NSTEPS, **kw, events=True, max_events=1),
           "stop": run_sweep_rk4(base, INSTANCES, DTS, NSTEPS, **kw, frame_steps=FRAME_STEPS, events=True, max_events=8, terminal={"ones_Phi": 1}),
           "mine": assign(len(INSTANCES), rank, world, "round_robin"), "calls": list(OracleRk4Engine.calls)}
    out["own"] = run_sweep_rk4(base, INSTANCES, DTS, NSTEPS, y0=y0, engine_factory=factory, gather=False)      # balance: the default
    out["default_mine"] = assign(len(INSTANCES), rank, world, "contiguous")
    return out


@pytest.fixture(scope="module")
def reference(oracle):
    base = _base(N)
    y0 = _y0(base, INSTANCES)
    P = [oracle.params_from_dict(base | inst) for inst in INSTANCES]
    free = [ref.oracle_run(P[b], N, y0[b], DTS[b], NSTEPS, 0.0, list(FRAME_STEPS), None, 8) for b in range(len(INSTANCES))]
    stop = [ref.oracle_run(P[b], N, y0[b], DTS[b], NSTEPS, 0.0, list(FRAME_STEPS), (0, 0, 0, 0, 1, 0, 0), 8) for b in range(len(INSTANCES))]
    return free, stop


def test_the_reference_runs_cover_every_status(reference):
    free, stop = reference
    assert [w.status for w, _, _ in free] == [ref.NONFINITE, 0, 0, 0, 0] and [w.status for w, _, _ in stop] == [ref.NONFINITE, 0, 0, 0, ref.TERMINAL]
    assert free[0][0].steps == 2 and not np.all(np.isfinite(free[0][1])) and free[0][0].next_frame == 2      # frames 0 and 1, none at the bad step
    assert free[4][0].n_events == [0, 0, 0, 0, 1, 0, 1] and stop[4][0].n_events == [0, 0, 0, 0, 1, 0, 0]
    assert stop[4][0].steps == 2704 and stop[4][0].next_frame == 3 and free[4][0].next_frame == 5
    assert 2703 * 5e-6 < free[4][0].t_events[4][0] < 2704 * 5e-6 and 2780 * 5e-6 <= free[4][0].t_events[6][0] <= 2781 * 5e-6


@pytest.mark.parametrize("world", [1, 2])
def test_run_sweep_rk4_orders_and_gathers_states_counts_frames_and_roots(reference, world):
    free, stop = reference
    B = len(INSTANCES)
    out = _spawn(_worker, world)
    if world == 2:
        assert out[0]["mine"] == [0, 2, 4] and out[1]["mine"] == [1, 3] and out[0]["default_mine"] == [0, 1]
    for r in range(world):
        o = out[r]
        # frame_steps / events / max_events / terminal reach the engine only when asked for
        assert o["calls"] == [[], ["frame_steps"], ["events", "max_events"], ["events", "frame_steps", "max_events", "terminal"]]
        assert [len(o[k]) for k in ("plain", "frames", "events", "stop")] == [5, 7, 6, 8]
        for k, want in (("plain", free), ("frames", free), ("events", free), ("stop", stop)):
            y, status, steps, zeros, t_reached = o[k][:5]
            assert np.array_equal(y, np.stack([q[1] for q in want]), equal_nan=True), k
            assert status.tolist() == [q[0].status for q in want] and steps.tolist() == [q[0].steps for q in want], k
            assert zeros.tolist() == [0] * B and np.array_equal(t_reached, [q[0].t for q in want]), k
        for k, want in (("frames", free), ("stop", stop)):
            n_frames, y_frames = o[k][5], o[k][6]
            assert n_frames.tolist() == [q[0].next_frame for q in want] and y_frames.shape == (B, len(FRAME_STEPS), 5 * N), k
            for b, (w, _, frames) in enumerate(want):
                assert all(np.array_equal(y_frames[b, j], frames[j]) for j in range(w.next_frame)), (k, b)
                assert np.all(np.isnan(y_frames[b, w.next_frame:])), (k, b)
        for k, want, cap in (("events", free, 1), ("stop", stop, 8)):
            roots = o[k][-1]
            assert len(roots) == B
            for b, (w, _, _) in enumerate(want):
                assert len(roots[b]) == 7 and all(np.array_equal(a, t[:cap]) for a, t in zip(roots[b], w.t_events)), (k, b)
        mine = o["default_mine"]
        assert np.array_equal(o["own"][0], np.stack([free[i][1] for i in mine]), equal_nan=True) and o["own"][2].tolist() == [free[i][0].steps for i in mine]


# ---- integrate_equations(method="RK4") ----------------------------------------------------------------------------------------------
class _NoModel:
    @classmethod
    def from_scenario(cls, *a, **kw):
        raise AssertionError("a model was created before the schedule was checked")


@pytest.mark.parametrize("solver, tracker, n, needle", [
    (dict(t_span=(0.0, 0.03)), {}, 64, "need 'dt'"),
    (dict(dt=-1e-6, t_span=(0.0, 0.03)), {}, 64, "positive"),
    (dict(dt=7e-6, t_span=(0.0, 0.03)), {}, 64, "t_span[1] = 0.03"),
    (dict(dt=5e-6, t_span=(0.0, 0.03)), {"t_eval": [0.0, 0.003, 0.0030021]}, 64, "t_eval[2] = 0.0030021"),
    (dict(dt=5e-6, t_span=(0.0, 0.03)), {"t_eval": [0.0, 0.006, 0.003]}, 64, "t_eval[2] = 0.003 does not follow"),
    (dict(dt=5e-6, t_span=(0.0, 0.03)), {"t_eval": [0.0, 0.03, 0.033]}, 64, "t_eval[2] = 0.033 lies outside"),
    (dict(dt=5e-6, t_span=(0.0, 0.03)), {}, 1025, "N = 1025 exceeds 1024"),
])
def test_rk4_schedule_errors_are_raised_before_a_model_exists(monkeypatch, solver, tracker, n, needle):
    from marlpde_amd import Evolve_scenario as es
    monkeypatch.setattr(es, "LMAHeureuxPorosityDiff", _NoModel)
    with pytest.raises(ValueError) as err:
        es.integrate_equations(solver | {"method": "RK4", "backend": "hip"}, tracker, scenario("default", n), results_root=None, verbose=False)
    assert needle in str(err.value) and "RK4" in str(err.value), str(err.value)


def test_rk4_schedule_is_a_pure_function():
    from marlpde_amd.Evolve_scenario import rk4_schedule
    dt, nsteps, frames = rk4_schedule({"dt": 5e-6}, (0.0, 0.03), np.linspace(0.0, 0.03, 11), 64)
    assert (dt, nsteps) == (5e-6, 6000) and frames.tolist() == [600 * j for j in range(11)] and frames.dtype == np.int64
    assert rk4_schedule({"dt": 0.25}, (1.0, 3.0), None, 1024) == (0.25, 8, None)
    assert rk4_schedule({"dt": 0.25}, (1.0, 3.0), [1.0 + 0.25 * (1 + 9e-7)], 5)[2].tolist() == [1]        # within 1e-6 of a step
    with pytest.raises(ValueError):
        rk4_schedule({"dt": 0.25}, (1.0, 3.0), [1.0 + 0.25 * (1 + 2e-6)], 5)


def test_integrate_equations_rk4_hands_the_schedule_and_the_limits_to_the_model(monkeypatch, tmp_path):
    from marlpde_amd import Evolve_scenario as es
    from marlpde_amd._abi import MarlStats
    from marlpde_amd.LHeureux_model import RK45Result
    from test_sweep_rk23_cpu import _FakeModel
    seen = []

    class Model(_FakeModel):
        def set_terminal(self, limits):
            seen.append(("terminal", list(limits)))

        def integrate_rk4_watch(self, y0, dt, nsteps, t0=0.0, frame_steps=None):
            seen.append((dt, nsteps, t0, None if frame_steps is None else list(frame_steps)))
            st = MarlStats()
            st.status, st.t, st.nfev = 1, t0 + 7 * dt, 28
            k = 2
            return RK45Result(st, t0 + np.asarray(frame_steps[:k]) * dt, np.stack([np.asarray(y0, float)] * k, axis=1),
                              [np.empty(0)] * 4 + [np.array([6.5 * dt])] + [np.empty(0)] * 2)

    monkeypatch.setattr(es, "LMAHeureuxPorosityDiff", Model)
    pde = scenario("default", 16)
    last, covered, _, _, folder = es.integrate_equations(dict(method="RK4", dt=1e-5, t_span=(0.0, 1e-4), backend="hip"), {"t_eval": [0.0, 5e-5, 1e-4]}, pde,
                                                         results_root=str(tmp_path) + "/", verbose=False, terminal={"ones_Phi": 1})
    assert seen == [("terminal", [0, 0, 0, 0, 1, 0, 0]), (1e-5, 10, 0.0, [0, 5, 10])]
    assert last.shape == (5, 16) and covered == pde["Tstar"] * (0.0 + 7 * 1e-5)      # status 1: the time the run reached
    stored = np.load(folder + "LMAHeureuxPorosityDiff.npz")
    assert stored["solutions"].shape == (5, 16, 2) and stored["times"].tolist() == [0.0, 5e-5] and stored["event_4"].tolist() == [6.5 * 1e-5]
    assert str(stored["attr_method"]) == "RK4" and float(stored["attr_dt"]) == 1e-5
