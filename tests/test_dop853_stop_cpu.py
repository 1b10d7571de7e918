"""DOP853 runs and sweeps that stop at a terminal monitor's root, the parts that need no GPU.

* the two C entries are declared and bound with the argument lists of marl_sweep_rk45_terminal_dev / marl_integrate_rk45_terminal,
  exported, and return -1 without a context;
* csrc/marl_dop853_stop.h - the scalar walk of an accepted step that ends the run: which monitors need a root, what rk_terminal_step
  says, and which trip comes next (probes, the samples <= t_stop, the stop) - built alone by a host C++ compiler and run on synthetic
  accepted steps against scipy's own handle_events (as tests/test_terminal_select_cpu.py runs it) plus the count / slot rule.  Two
  monitors changing sign in one step happen here only: no such step was found in a cheap run of these equations;
* routing with doubles: HipSweepEngine.integrate_dop853_stop sets `terminal` and then asks sweep_dop853_stop_device, which takes the
  stop entry only while a limit is set; run_sweep_dop853_stop shards, gathers and orders status 1 and t_reached like the other
  drivers; integrate_equations(method="DOP853", terminal=...) takes integrate_dop853_stop only with native_terminal=True and
  N <= 1024, and solve_ivp otherwise."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from common import scenario
from test_sweep_dop853_cpu import _FakeModel, _declared
from test_sweep_frames_cpu import _spawn
from test_terminal_select_cpu import T_NEW, T_OLD, _scipys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "integrating-diagenetic-equations-using-python_amd", "csrc")

ENTRIES = {"marl_sweep_dop853_stop_dev": "marl_sweep_rk45_terminal_dev", "marl_integrate_dop853_stop": "marl_integrate_rk45_terminal"}


def test_entries_are_declared_bound_and_exported_like_the_rk45_terminal_entries():
    from marlpde_amd import _abi
    header = open(os.path.join(ROOT, "include", "marl_hip.h")).read()
    lib = _abi.load()
    for new, old in ENTRIES.items():
        assert _declared(header, new) == _declared(header, old), new
        assert _abi.PROTOTYPES[new] == _abi.PROTOTYPES[old] and hasattr(lib, new), new
        entry = getattr(lib, new)
        assert entry(*[a() for a in entry.argtypes]) == -1, new      # zeros and null pointers, no context: -1, nothing touched


# ---- the walk of a step that ends the run (csrc/marl_dop853_stop.h) ---------------------------------------------------------------
PROBE, SAMPLE, STOP = 100, 200, 300      # a trip of the walk as the shim notes it: PROBE + monitor, SAMPLE + frame, STOP
SHIM = r"""
#include "marl_dop853_stop.h"
using namespace marl;
static_assert(DOP853_NEXT_SAMPLE == 1 && DOP853_NEXT_PROBE == 2 && DOP853_NEXT_STOP == 3, "the loop's trip kinds");
// One accepted step as thread 0 of the stop kernel walks it: begin; while the walk asks for a probe, the lowest monitor still to be
// located gets its root (Brent's method is not under test: the root is given); behind the last one the rule; then samples and the stop.
// Returns -1 when the step meets no limit (and checks that the record was left alone), else the number of trips noted.
extern "C" int walk_shim(unsigned changed, const double* roots, const long long* n_events, const long long* limits, long long max_events,
                         const double* t_eval, long long n_eval, long long ie, unsigned* locate, unsigned* kept, double* t_stop,
                         long long* n_out, long long* slot, long long* ie_out, int* trips, int max_trips)
{
    int64_t c[7], l[7], o[7], sl[7];
    for (int e = 0; e < 7; e++) { c[e] = n_events[e]; l[e] = limits[e]; o[e] = -7; sl[e] = -7; }
    Dop853Stop s;
    dop853_stop_init(s, l);
    if (!dop853_stop_begin(s, changed, c)) return (s.stage == DOP853_STOP_IDLE && s.locate == 0 && s.active == 0) ? -1 : -2;
    if (s.stage != DOP853_STOP_ROOTS) return -3;
    *locate = s.locate;
    int n = 0;
    while (n < max_trips) {
        const int next = dop853_stop_next(s, ie, n_eval, t_eval);
        if (next == DOP853_NEXT_PROBE) {
            const int e = __builtin_ctz(s.locate);
            trips[n++] = 100 + e;
            if (dop853_stop_root(s, e, roots[e]) == 0) dop853_stop_rule(s, c, max_events, o, sl);
        } else if (next == DOP853_NEXT_SAMPLE) {
            if (s.stage != DOP853_STOP_SAMPLES) return -4;
            trips[n++] = 200 + (int)ie;
            ie++;
        } else {
            if (s.stage != DOP853_STOP_SAMPLES) return -5;
            trips[n++] = 300;
            break;
        }
    }
    for (int e = 0; e < 7; e++) { n_out[e] = o[e]; slot[e] = sl[e]; }
    *kept = s.kept;
    *t_stop = s.t_stop;
    *ie_out = ie;
    return n;
}
"""
LL7 = C.c_longlong * 7


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("dop853stop")
    src, so = d / "dop853_stop_shim.cpp", d / "libdop853_stop_shim.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.walk_shim.restype = C.c_int
    return lib


def _walk(shim, active, roots, n_events, limits, max_events, t_eval=(), ie=0):
    """-> None (the step meets no limit), or (monitors to locate, kept, t_stop, counts, slots, next sample, trips)"""
    mask = sum(1 << e for e in active)
    r = (C.c_double * 7)(*[roots.get(e, float("nan")) for e in range(7)])      # entries of monitors that did not change sign must not be read
    te = (C.c_double * max(len(t_eval), 1))(*t_eval)
    locate, kept, t_stop, n_out, slot, ie_out, trips = C.c_uint(0), C.c_uint(0), C.c_double(-1.0), LL7(), LL7(), C.c_longlong(-1), (C.c_int * 64)()
    n = shim.walk_shim(C.c_uint(mask), r, LL7(*n_events), LL7(*limits), C.c_longlong(max_events), te, C.c_longlong(len(t_eval)), C.c_longlong(ie),
                       C.byref(locate), C.byref(kept), C.byref(t_stop), n_out, slot, C.byref(ie_out), trips, 64)
    assert n >= -1, f"the walk left its stages ({n})"
    if n == -1:
        return None
    bits = lambda m: [e for e in range(7) if (m >> e) & 1]  # noqa: E731
    return bits(locate.value), bits(kept.value), t_stop.value, list(n_out), list(slot), ie_out.value, list(trips[:n])


def _expected(active, targets, n_events, limits, max_events, t_eval=(), ie=0):
    """scipy's handle_events for the step (counts with this occurrence included, ivp.py:680), then the count / slot rule of
    marl_rk_terminal.h and the order of trips: one probe per monitor that changed sign (ascending), the samples <= t_stop, the stop.
    Also returns the roots scipy located, which the walk is given."""
    counts = {e: n_events[e] + 1 for e in active}
    terminate, kept, roots, located = _scipys(active, targets, counts, limits)
    if not terminate:
        return None, located
    kept, t_stop = sorted(kept), roots[-1]
    n_out = [n_events[e] + (1 if e in kept else 0) for e in range(7)]
    slot = [n_events[e] if (e in kept and n_events[e] < max_events) else -1 for e in range(7)]
    trips = [PROBE + e for e in sorted(active)]
    k = ie
    while k < len(t_eval) and t_eval[k] <= t_stop:
        trips.append(SAMPLE + k)
        k += 1
    return (sorted(active), kept, t_stop, n_out, slot, k, trips + [STOP]), located


A, B, C_ = (T_OLD + (T_NEW - T_OLD) * f for f in (0.2, 0.5, 0.75))      # three root times inside the step
COUNTS = [0, 2, 1, 0, 0, 3, 6]
CASES = [
    # active, targets, limits, what the case is about
    ([4], {4: B}, {4: 1}, "one monitor, limit 1"),
    ([6], {6: B}, {6: 7}, "one monitor, limit k > 1 met by this occurrence"),
    ([6], {6: B}, {6: 8}, "one monitor, the limit one occurrence away: not met"),
    ([6], {6: B}, {4: 1}, "the limit belongs to a monitor that did not change sign: not met"),
    ([1, 6], {1: A, 6: C_}, {1: 3}, "two monitors, distinct roots, the earlier one ends the run: the later never happened"),
    ([1, 6], {1: A, 6: C_}, {6: 7}, "two monitors, the terminal one is not the earliest: both kept"),
    ([1, 6], {1: B, 6: B}, {6: 7}, "two monitors, equal roots, the higher one terminal: both kept"),
    ([1, 6], {1: B, 6: B}, {1: 1}, "two monitors, equal roots, the lower one terminal (limit passed long ago): the higher never happened"),
    ([1, 6], {1: A, 6: C_}, {1: 4, 6: 8}, "two monitors, neither limit met"),
    ([0, 4, 6], {0: C_, 4: A, 6: B}, {6: 7}, "three monitors, the terminal one in the middle of the order"),
    ([0, 4, 6], {0: C_, 4: A, 6: B}, {0: 1}, "three monitors, the terminal one last: all kept"),
    ([0, 4, 6], {0: B, 4: B, 6: B}, {4: 1}, "three monitors, all roots equal: monitor order decides"),
    ([0, 4, 6], {0: A, 4: A, 6: C_}, {0: 1, 6: 7}, "three monitors, two limits met: the first in the order of roots ends the run"),
    ([0, 4, 6], {0: A, 4: B, 6: C_}, {0: 2, 4: 2, 6: 9}, "three monitors, no limit met"),
]
T_EVAL = [T_OLD - 1e-3, T_OLD + 1e-9, A, 0.5 * (A + B), B, C_, T_NEW, T_NEW + 1e-3]


@pytest.mark.parametrize("max_events", [0, 1, 64])
@pytest.mark.parametrize("active, targets, limits, what", CASES, ids=[c[3] for c in CASES])
def test_walk_against_scipys_handle_events(shim, active, targets, limits, what, max_events):
    lim = [limits.get(e, 0) for e in range(7)]
    for t_eval, ie in (((), 0), (T_EVAL, 1), (T_EVAL, 4), (T_EVAL, len(T_EVAL))):      # no samples; from the step's first; from a later one; none left
        want, located = _expected(active, targets, COUNTS, lim, max_events, t_eval, ie)
        got = _walk(shim, active, located, COUNTS, lim, max_events, t_eval, ie)
        print(f"{what}, max_events {max_events}, ie {ie}/{len(t_eval)}: {got}")
        assert got == want, (what, max_events, ie, got, want)
        assert ("not met" in what or "no limit" in what or "neither" in what) == (want is None), what
        if want is not None:
            # probes -> samples <= t_stop -> stop, and a root is stored only where it is kept and a slot is free
            kinds = [t // 100 for t in got[6]]
            assert kinds == sorted(kinds) and kinds[-1] == 3 and kinds.count(3) == 1 and kinds.count(1) == len(active)
            assert all(t_eval[t - SAMPLE] <= got[2] for t in got[6] if t // 100 == 2)
            assert got[5] == len(t_eval) or t_eval[got[5]] > got[2]
            assert all((s >= 0) == (e in got[1] and COUNTS[e] < max_events) for e, s in enumerate(got[4]))


def test_walk_on_random_steps_against_scipys_handle_events(shim):
    rng = np.random.default_rng(20261021)
    pool = T_OLD + (T_NEW - T_OLD) * np.array([0.05, 0.2, 0.2000001, 0.5, 0.75, 0.99])    # few values: ties are common
    n_stop = n_dropped = n_tie = 0
    for _ in range(300):
        active = sorted(rng.choice(7, size=rng.integers(1, 4), replace=False).tolist())
        targets = {e: float(rng.choice(pool)) for e in active}
        n_events = [int(k) for k in rng.integers(0, 4, size=7)]
        limits = [int(k) for k in rng.integers(0, 5, size=7)]
        max_events = int(rng.choice([0, 1, 2, 64]))
        t_eval = sorted(float(x) for x in rng.uniform(T_OLD, T_NEW, size=rng.integers(0, 5)))
        want, located = _expected(active, targets, n_events, limits, max_events, t_eval, 0)
        got = _walk(shim, active, located, n_events, limits, max_events, t_eval, 0)
        assert got == want, (active, targets, n_events, limits, max_events, t_eval, got, want)
        if want is not None:
            n_stop += 1
            n_dropped += want[1] != active
            n_tie += sum(located[e] == want[2] for e in active) > 1
    print(f"{n_stop} of 300 steps stop: {n_dropped} drop a sign change, {n_tie} with another root equal to t_stop")
    assert n_stop >= 100 and n_dropped >= 20 and n_tie >= 5


# ---- routing ------------------------------------------------------------------------------------------------------------------------
def test_engine_and_model_route_the_stop_to_its_entries():
    from marlpde_amd.LHeureux_model import LMAHeureuxPorosityDiff
    from marlpde_amd.sweep import HipSweepEngine
    order = []

    class Model:
        terminal = [0] * 7

        def set_terminal(self, spec):
            order.append(("set_terminal", spec))
            self.terminal = [0] * 7 if spec is None else list(spec)

        def sweep_dop853_stop_device(self, *a, **kw):
            order.append(("sweep_dop853_stop_device", list(self.terminal), a[1:], kw))
            return ["res"]

    class Engine:
        torch = __import__("torch")
        device = "cpu"
        model = Model()
        _integrate_rk = HipSweepEngine._integrate_rk

    y0 = np.arange(10.0).reshape(2, 5)
    y, res = HipSweepEngine.integrate_dop853_stop(Engine(), y0, (0.0, 1.0), 1e-3, 1e-5, 1e-7, 9, events=True, max_events=5, terminal=[0, 0, 0, 0, 1, 0, 0])
    assert np.array_equal(y, y0) and res == ["res"]
    assert order == [("set_terminal", [0, 0, 0, 0, 1, 0, 0]),      # the limits first, then the sweep that honours them
                     ("sweep_dop853_stop_device", [0, 0, 0, 0, 1, 0, 0], ((0.0, 1.0), 1e-3, 1e-5, 1e-7, 9), {"events": True, "max_events": 5})]

    # the model: the stop entry while a limit is set - through the shared marshalling, the entry named - and sweep_dop853_device while none is
    seen = []

    class M:
        def __init__(self, terminal):
            self.terminal = terminal

        def _sweep_rk_device(self, method, *a, **kw):
            seen.append(("shared", method, a, kw))
            return "stopped"

        def sweep_dop853_device(self, *a, **kw):
            seen.append(("plain", a, kw))
            return "free"

    args = (123, (0.0, 1.0), 1e-3, 1e-5, 1e-7, 9)
    assert LMAHeureuxPorosityDiff.sweep_dop853_stop_device(M([0, 0, 0, 0, 2, 0, 0]), *args, t_eval=[0.5], y_eval_dev_ptr=456, events=True, max_events=3) == "stopped"
    assert LMAHeureuxPorosityDiff.sweep_dop853_stop_device(M([0] * 7), *args, t_eval=[0.5], y_eval_dev_ptr=456, events=True, max_events=3) == "free"
    assert seen == [("shared", "dop853", args + ([0.5], 456, True, 3), {"terminal_entry": "marl_sweep_dop853_stop_dev"}),
                    ("plain", args + ([0.5], 456, True, 3), {})]

    # the shared marshalling calls the entry it is given, with the argument list of the terminal entries
    called = []

    class Lib:
        def marl_sweep_dop853_stop_dev(self, *a):
            called.append(a)
            return 0

    class Real:
        n_instances = 2
        terminal = [0, 0, 0, 0, 1, 0, 0]
        _lib, _ctx = Lib(), "ctx"

        def _check(self, rc, what):
            assert rc == 0 and what == "marl_sweep_dop853_stop_dev"

    out = LMAHeureuxPorosityDiff._sweep_rk_device(Real(), "dop853", 123, (0.0, 1.0), 1e-3, 1e-5, 1e-7, 9, None, None, False, 64,
                                                  terminal_entry="marl_sweep_dop853_stop_dev")
    assert len(out) == 2 and len(called) == 1 and len(called[0]) == len(__import__("marlpde_amd")._abi.PROTOTYPES["marl_sweep_dop853_stop_dev"][1])
    assert called[0][8] is None and called[0][9] == 0 and called[0][12] is None and called[0][13] == 0      # no t_eval, no roots asked for

    # the single run goes to marl_integrate_dop853_stop through the shared plumbing
    single = []

    class One:
        def _integrate_rk(self, *a):
            single.append(a)
            return "r"

    assert LMAHeureuxPorosityDiff.integrate_dop853_stop(One(), "y0", (0.0, 1.0), 1e-3, 1e-5, 1e-7, t_eval=[1.0], events=False, max_attempts=4) == "r"
    assert single == [("dop853_stop", "y0", (0.0, 1.0), 1e-3, 1e-5, 1e-7, [1.0], False, 4096, 4)]


N = 16
STOPS = {1: 0.25, 4: 0.75}      # instance -> the fraction of t1 at which its terminal monitor ends it


class StoppingEngine:
    """Test double with HipSweepEngine's interface: instances named in STOPS end early with status 1 when `terminal` reaches it."""
    calls = []

    def __init__(self, base_parms, instances):
        self.ids = [int(i["id"]) for i in instances]

    def integrate_dop853_stop(self, y0, t_span, first_step, rtol, atol, max_attempts, **more):
        from marlpde_amd._abi import MarlStats
        from marlpde_amd.LHeureux_model import RK45Result
        type(self).calls.append(sorted(more))
        res = []
        for i in self.ids:
            st = MarlStats()
            stopped = more.get("terminal") is not None and i in STOPS
            st.status, st.t, st.n_accepted, st.n_rejected = (1, STOPS[i] * t_span[1], 10 + i, i) if stopped else (0, t_span[1], 40 + i, 2 * i)
            st.n_events[4] = 1 if stopped else 0
            res.append(RK45Result(st, t_events=[np.array([st.t])[:st.n_events[e]] for e in range(7)] if more.get("events") else None))
        return np.array(y0) + np.array(self.ids)[:, None], res

    def close(self):
        pass


def _stop_worker(rank, world):
    from marlpde_amd.sweep import run_sweep_dop853_stop
    base = scenario("default", N)
    insts = [{"id": float(i)} for i in range(6)]
    y0 = np.zeros((6, 5 * N))
    kw = dict(y0=y0, engine_factory=lambda bp, inst: StoppingEngine(bp, inst), balance="round_robin")
    StoppingEngine.calls = []
    return {"stop": run_sweep_dop853_stop(base, insts, (0.0, 2.0), 1e-3, 1e-5, 1e-7, **kw, events=True, max_events=4, terminal={"ones_Phi": True}),
            "free": run_sweep_dop853_stop(base, insts, (0.0, 2.0), 1e-3, 1e-5, 1e-7, **kw),
            "calls": StoppingEngine.calls}


@pytest.mark.parametrize("world", [1, 2])
def test_run_sweep_dop853_stop_shards_gathers_and_orders_the_stops(world):
    out = _spawn(_stop_worker, world)
    for r in range(world):
        o = out[r]
        assert o["calls"] == [["events", "max_events", "terminal"], []]      # `terminal` reaches the engine only when given
        y, status, n_acc, n_rej, t_reached, roots = o["stop"]
        assert status.tolist() == [0, 1, 0, 0, 1, 0] and np.array_equal(t_reached, [2.0, 0.5, 2.0, 2.0, 1.5, 2.0])
        assert n_acc.tolist() == [40, 11, 42, 43, 14, 45] and n_rej.tolist() == [0, 1, 4, 6, 4, 10]
        assert np.array_equal(y[:, 0], np.arange(6.0))                       # back in the order of `instances`
        assert [len(rt[4]) for rt in roots] == [0, 1, 0, 0, 1, 0] and roots[4][4][0] == 1.5
        y, status, n_acc, n_rej, t_reached = o["free"]
        assert status.tolist() == [0] * 6 and np.array_equal(t_reached, [2.0] * 6) and np.array_equal(y[:, 0], np.arange(6.0))


class _StopModel(_FakeModel):
    limits = None

    def set_terminal(self, spec):
        type(self).limits = list(spec)

    def integrate_dop853_stop(self, y0, t_span, first_step, rtol, atol, t_eval=None):
        from marlpde_amd._abi import MarlStats
        from marlpde_amd.LHeureux_model import RK45Result
        type(self).asked.append(("dop853_stop", list(type(self).limits)))
        st = MarlStats()
        st.status, st.t, st.nfev = 1, 0.25 * t_span[1], 16
        return RK45Result(st, np.array([st.t]), np.asarray(y0, float)[:, None].copy(), [np.empty(0)] * 4 + [np.array([st.t])] + [np.empty(0)] * 2)


def test_integrate_equations_takes_the_native_stop_only_on_request(monkeypatch):
    import scipy.integrate
    from marlpde_amd import Evolve_scenario as es
    monkeypatch.setattr(es, "LMAHeureuxPorosityDiff", _StopModel)
    real = scipy.integrate.solve_ivp
    seen = []

    def noting(*a, **kw):
        seen.append(kw.get("method"))
        return real(*a, **kw)

    monkeypatch.setattr(scipy.integrate, "solve_ivp", noting)
    solver = dict(first_step=1e-6, rtol=1e-3, atol=1e-3, t_span=(0.0, 1e-4), backend="hip", method="DOP853")
    term = {"ones_Phi": True}
    _FakeModel.asked = []
    for n in (16, 1024):
        last, covered, *_ = es.integrate_equations(solver | {"native_terminal": True}, {}, scenario("A", n), results_root=None, verbose=False, terminal=term)
        assert last.shape == (5, n) and covered == scenario("A", n)["Tstar"] * 0.25e-4      # Tstar * t_reached
    assert _FakeModel.asked == [("dop853_stop", [0, 0, 0, 0, 1, 0, 0])] * 2 and seen == []
    # without the request, above one workgroup, or with scipy_driver: today's route, solve_ivp on the HIP RHS
    es.integrate_equations(solver, {}, scenario("A", 16), results_root=None, verbose=False, terminal=term)
    es.integrate_equations(solver | {"native_terminal": True}, {}, scenario("A", 1025), results_root=None, verbose=False, terminal=term)
    es.integrate_equations(solver | {"native_terminal": True, "scipy_driver": True}, {}, scenario("A", 16), results_root=None, verbose=False, terminal=term)
    assert seen == ["DOP853"] * 3 and len(_FakeModel.asked) == 2
    # native_terminal without a limit: the run without limits, as before
    es.integrate_equations(solver | {"native_terminal": True}, {}, scenario("A", 16), results_root=None, verbose=False)
    assert _FakeModel.asked[2:] == ["dop853"] and seen == ["DOP853"] * 3
