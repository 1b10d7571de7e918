"""The root-location form of csrc/marl_bdf_ctl.h (struct BdfRoots, A_ROOTS, bdf_locate_roots): the monitors' root times of the BDF
sweep, driven on the CPU in lockstep with scipy.  The header is built alone by a host C++ compiler, as
tests/test_bdf_frames_control_cpu.py builds it, with a shim of its own; the data-parallel work of every action bit is done with scipy's
pieces in the order the header documents: A_ACCEPT, A_CHANGE_D, A_ROOTS, A_SAMPLE, A_JAC, A_LU, A_SOLVE.  A_ROOTS is served by the
header's own bdf_locate_roots through the shim, with a callback that forms the dense state from the driver's own D as the sweep's
kernel forms it (D[0] + sum_j D[j + 1] p[j], p from the header's bdf_dense_weights) and returns seven event functions of that state.

The three problems of test_bdf_control_cpu.py, each with seven event functions of the state (EVENTS) chosen so that some monitors have
several roots (robertson's y1 - 2e-5 rises and falls through it; van der Pol's y0 + 1.5 is passed by the jump and by the slow branch
after it), two monitors change sign in the same step (robertson's step 47, van der Pol's 78, the blow-up's 6) and some have none.  Held to solve_ivp(method="BDF", events=...):
  * the number of roots of every monitor: exact, and equal to the controller's n_events;
  * the root times.  Measured with the finished code (scipy 1.15.3), the largest |root - scipy's| / scipy's over a run: robertson
    2.1e-15, van_der_pol 0, blow_up 0 (in these runs the controller's step times are scipy's to the last bits; the sum of the dense
    state is formed term by term, scipy's by a dot product).  ROOT_BOUND = 2.1e-14 is 10 times the largest.  Each of the three
    injected driver defects exceeds it (asserted for every defect; printed per problem; measured, the worst of the three problems, in
    units of the bound: before_change_D 4.8e13, after_next_rescaling 3.3e11, solved_h 1.4e13):
        searching before the selection's change_D;  searching after the next step's clip / min_step rescaling;
        the solved step's h_abs in place of the post-selection one;
  * max_events = 1: n_events goes on counting, only slot 0 of every monitor is written;
  * a max_attempts-limited run keeps the roots it reached (the leading ones of the full run); t1 == t0 has none;
  * without roots (no BdfRoots, or max_events = 0) the action words, the cycle count and the bytes of BdfCtl are those of the
    three-argument call; with roots the work bits come in the same order, and the extra cycles are <= the A_ROOTS words <= the steps
    with sign changes; with roots and samples together the extra cycles are no more than the steps that have either."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from scipy.integrate import solve_ivp
from scipy.integrate._ivp import bdf as scipy_bdf
from scipy.linalg import lu_factor, lu_solve

from test_bdf_control_cpu import A_ACCEPT, A_CHANGE_D, A_JAC, A_LU, A_SOLVE, CASES, CSRC, PC_DONE, BdfCtl
from test_bdf_frames_control_cpu import A_SAMPLE, BdfSample

A_ROOTS = 64
ROOT_BOUND = 2.1e-14   # relative to the root time: 10 times the largest measured deviation (docstring)
BIG = 64               # max_events that holds every root of these runs

# Seven event functions of the state per problem.  The thresholds are placed by scipy's own runs (scipy 1.15.3; the step numbers are
# asserted by test_the_event_functions_cover_the_cases): roots in steps that end with an order / step-size selection (the defect
# "before_change_D" shows only there), in the step before the last, whose successor is clipped at t_bound (the defect
# "after_next_rescaling" shows only there), two monitors inside one step, monitors with two roots, monitors with none.
EVENTS = {
    # y0 falls, y2 rises, y1 rises to 3.6e-5 and falls.  Steps 47, 52, 57 select; 73 is the step before the last.
    "robertson": [lambda y: y[1] - 2e-5, lambda y: y[0] - 0.87, lambda y: y[0] - 0.73, lambda y: y[2] - 0.094, lambda y: y[2] - 0.0576,
                  lambda y: y[0] - 0.9425, lambda y: y[0] - 5.0],
    # y0 creeps down from 2, jumps to -2 at t = 81, creeps up.  Steps 37 and 78 select; 156 is the step before the last.
    "van_der_pol": [lambda y: y[0] + 1.5, lambda y: y[0] + 0.3, lambda y: y[0] + 0.4, lambda y: y[0] - 1.43, lambda y: y[0] + 1.44,
                    lambda y: y[1] + 0.01, lambda y: y[0] - 5.0],
    # y = 1 / (1 - t).  Steps 1, 3, 6 select.
    "blow_up": [lambda y: y[0] - 1.0015, lambda y: y[0] - 1.017, lambda y: y[0] - 1.15, lambda y: y[0] - 1.18, lambda y: y[0] - 10.0,
                lambda y: y[0] + 1.0, lambda y: y[0] - 1e4],
}
# (problem, monitor) -> the accepted step of scipy's run (counted from 0) that holds its (last) root
PLACED = {("robertson", 1): 57, ("robertson", 2): 73, ("robertson", 3): 52, ("robertson", 4): 47, ("robertson", 5): 47,
          ("van_der_pol", 1): 78, ("van_der_pol", 2): 78, ("van_der_pol", 3): 37, ("van_der_pol", 4): 156,
          ("blow_up", 0): 1, ("blow_up", 1): 3, ("blow_up", 2): 6, ("blow_up", 3): 6}

SHIM = r"""
#include "marl_bdf_ctl.h"
using namespace marl::bdfctl;
typedef void (*eval_fn)(double tq, double* g);   // the seven monitors of the dense state at tq
extern "C" {
int bdf_ctl_sizeof() { return (int)sizeof(BdfCtl); }
int bdf_smp_sizeof() { return (int)sizeof(BdfSample); }
int bdf_roots_sizeof() { return (int)sizeof(BdfRoots); }
int bdf_ctl_a_roots() { return A_ROOTS; }
void bdf_ctl_init(BdfCtl* c, double t0, double t1, double first_step, double rtol, double atol, long long max_attempts)
{
    bdf_control_init(*c, t0, t1, first_step, rtol, atol, max_attempts);
}
void bdf_smp_init(BdfSample* s, long long n_eval) { bdf_sample_init(*s, n_eval); }
void bdf_rts_init(BdfRoots* r, long long max_events) { bdf_roots_init(*r, max_events); }
void bdf_ctl_step3(BdfCtl* c, long long n, const double* g0) { bdf_control_step(*c, n, g0); }
void bdf_ctl_step6(BdfCtl* c, long long n, const double* g0, BdfSample* s, const double* t_eval, BdfRoots* r) { bdf_control_step(*c, n, g0, s, t_eval, r); }
void bdf_rts_locate(const BdfRoots* r, eval_fn f, double* t_events)
{
    bdf_locate_roots(*r, [f](double tq, int e) { double g[7]; f(tq, g); return g[e]; }, t_events);
}
void bdf_weights(double t, double h, int order, double tq, double* p)
{
    double w[MAX_ORDER + 1];
    bdf_dense_weights(t, h, order, tq, w);
    for (int j = 0; j <= MAX_ORDER; j++) p[j] = w[j];
}
double bdf_ctl_gamma(int k) { return gamma_of(k); }
}
"""

EVAL_FN = C.CFUNCTYPE(None, C.c_double, C.POINTER(C.c_double))


class BdfRoots(C.Structure):
    _fields_ = [("max_events", C.c_int64), ("t_old", C.c_double), ("t", C.c_double), ("h", C.c_double), ("order", C.c_int32),
                ("pending", C.c_int32), ("mask", C.c_int32), ("pad", C.c_int32), ("slot", C.c_int64 * 7)]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("bdfroots")
    src, so = d / "bdf_roots_shim.cpp", d / "libbdf_roots_shim.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.bdf_ctl_init.argtypes = [C.POINTER(BdfCtl)] + [C.c_double] * 5 + [C.c_longlong]
    lib.bdf_ctl_init.restype = None
    lib.bdf_smp_init.argtypes = [C.POINTER(BdfSample), C.c_longlong]
    lib.bdf_smp_init.restype = None
    lib.bdf_rts_init.argtypes = [C.POINTER(BdfRoots), C.c_longlong]
    lib.bdf_rts_init.restype = None
    lib.bdf_ctl_step3.argtypes = [C.POINTER(BdfCtl), C.c_longlong, C.POINTER(C.c_double)]
    lib.bdf_ctl_step3.restype = None
    lib.bdf_ctl_step6.argtypes = [C.POINTER(BdfCtl), C.c_longlong, C.POINTER(C.c_double), C.POINTER(BdfSample), C.POINTER(C.c_double), C.POINTER(BdfRoots)]
    lib.bdf_ctl_step6.restype = None
    lib.bdf_rts_locate.argtypes = [C.POINTER(BdfRoots), EVAL_FN, C.POINTER(C.c_double)]
    lib.bdf_rts_locate.restype = None
    lib.bdf_weights.argtypes = [C.c_double, C.c_double, C.c_int, C.c_double, C.POINTER(C.c_double)]
    lib.bdf_weights.restype = None
    lib.bdf_ctl_gamma.argtypes = [C.c_int]
    lib.bdf_ctl_gamma.restype = C.c_double
    assert lib.bdf_ctl_sizeof() == C.sizeof(BdfCtl), "BdfCtl must keep its size (tests/test_bdf_control_cpu.py mirrors it)"
    assert lib.bdf_smp_sizeof() == C.sizeof(BdfSample), "BdfSample must keep its size (tests/test_bdf_frames_control_cpu.py mirrors it)"
    assert lib.bdf_roots_sizeof() == C.sizeof(BdfRoots), "the ctypes mirror of BdfRoots is out of date"
    assert lib.bdf_ctl_a_roots() == A_ROOTS
    return lib


def drive(lib, name, t_span=None, max_events=BIG, roots=True, t_eval=None, max_attempts=0, three_args=False, defect=None, guard=0):
    """The cycle of the sweep's host driver for one instance of problem `name`, scipy's pieces as the kernels.  roots False: the
    controller gets no BdfRoots (three_args: through the three-argument call).  t_eval: sample times (the samples themselves are not
    formed here).  defect: None, or one of the three injected driver mistakes: "before_change_D" (the search runs before the cycle's
    rescaling), "after_next_rescaling" (it runs in the NEXT cycle, after its rescaling), "solved_h" (the weights use the solved
    step's h_abs).  guard: NaN doubles behind the [7][max_events] root times, returned with them.
    Returns (controller, root times (7 * max_events + guard,), action words, steps with a sign change, steps with a sign change or a sample)."""
    (fun, jac, y0, span, first_step, rtol, atol), _ = CASES[name]
    ev = EVENTS[name]
    t0, t1 = span if t_span is None else t_span
    y0 = np.asarray(y0, float)
    n = y0.size
    gamma = np.array([lib.bdf_ctl_gamma(k) for k in range(6)])
    c, s, r = BdfCtl(), BdfSample(), BdfRoots()
    lib.bdf_ctl_init(C.byref(c), t0, t1, first_step, rtol, atol, max_attempts)
    te = np.ascontiguousarray([] if t_eval is None else t_eval, dtype=np.float64)
    lib.bdf_smp_init(C.byref(s), te.size)
    lib.bdf_rts_init(C.byref(r), max_events)
    te_p = te.ctypes.data_as(C.POINTER(C.c_double))
    tev = np.full(7 * max(max_events, 0) + guard, np.nan)
    tev_p = tev.ctypes.data_as(C.POINTER(C.c_double))
    D = np.zeros((8, n))
    D[0] = y0
    D[1] = fun(t0, y0) * first_step
    J = jac(t0, y0)
    LU = y_predict = psi = scale = y_new = d = None
    g_prev = [f(y0) for f in ev]
    g0 = (C.c_double * 7)(*g_prev)
    eye = np.identity(n)
    words, solved_order, solved_h, pending, n_changed, n_either = [], 1, first_step, None, 0, 0
    p = (C.c_double * 6)()

    def locate(snap, h):
        """bdf_locate_roots on the snapshot `snap` (a copy of the instance's BdfRoots) with the dense output of the driver's D now"""
        def monitors(tq, g):
            lib.bdf_weights(snap.t, h, snap.order, tq, p)
            a = np.zeros(n)
            for j in range(snap.order):
                a = a + D[j + 1] * p[j]
            y = a + D[0]
            for e in range(7):
                g[e] = ev[e](y)
        lib.bdf_rts_locate(C.byref(snap), EVAL_FN(monitors), tev_p)

    def copy_of(x):
        out = BdfRoots()
        C.memmove(C.byref(out), C.byref(x), C.sizeof(BdfRoots))
        return out

    while True:
        next0 = s.next
        if three_args:
            lib.bdf_ctl_step3(C.byref(c), n, g0)
        else:
            lib.bdf_ctl_step6(C.byref(c), n, g0, C.byref(s) if t_eval is not None else None, te_p if t_eval is not None else None,
                              C.byref(r) if roots else None)
        words.append(c.action)
        assert len(words) < 100000
        a = c.action
        snap = copy_of(r) if a & A_ROOTS else None
        if a & A_ACCEPT:
            order = solved_order
            D[order + 2] = d - D[order + 1]
            D[order + 1] = d
            for i in reversed(range(order + 1)):
                D[i] += D[i + 1]
            sc = atol + rtol * np.abs(y_new)
            if c.want_norms & 1:
                c.ss_m = float(np.sum((c.err_coef_m * D[order] / sc) ** 2))
            if c.want_norms & 2:
                c.ss_p = float(np.sum((c.err_coef_p * D[order + 2] / sc) ** 2))
            g_now = [c.g[e] for e in range(7)]   # (the controller has taken g_new over)
            changed = any((a_ <= 0 and b_ >= 0) or (a_ >= 0 and b_ <= 0) for a_, b_ in zip(g_prev, g_now))
            covered = t_eval is not None and next0 < te.size and te[next0] <= c.t
            n_changed += changed
            n_either += changed or covered
            g_prev = g_now
        if snap and defect == "before_change_D":
            locate(snap, snap.h)
        if a & A_CHANGE_D:
            o = c.ru_order
            RU = np.array([[c.RU[i][j] for j in range(o + 1)] for i in range(o + 1)])
            D[:o + 1] = RU.T @ D[:o + 1].copy()
        if pending is not None:   # (defect "after_next_rescaling": the previous cycle's search, after this cycle's rescaling)
            locate(pending, pending.h)
            pending = None
        if snap and defect is None:
            locate(snap, snap.h)
        if snap and defect == "solved_h":
            locate(snap, solved_h)
        if snap and defect == "after_next_rescaling":
            if c.pc == PC_DONE:
                locate(snap, snap.h)
            else:
                pending = snap
        if a & A_JAC:
            J = jac(c.t_new, y_predict)
        if a & A_LU:
            LU = lu_factor(eye - c.c * J)
        if a & A_SOLVE:
            order = c.order
            if c.mode == 0:
                y_predict = np.sum(D[:order + 1], axis=0)
                scale = atol + rtol * np.abs(y_predict)
                psi = np.dot(D[1:order + 1].T, gamma[1:order + 1]) / c.alpha_order
            converged, n_iter, y_new, d = scipy_bdf.solve_bdf_system(fun, c.t_new, y_predict, c.c, psi, LU, lambda lu, b: lu_solve(lu, b),
                                                                     scale, c.newton_tol)
            c.iters, c.converged = n_iter, int(converged)
            if converged:
                c.err_ss = float(np.sum((c.err_coef * d / (atol + rtol * np.abs(y_new))) ** 2))
                for e in range(7):
                    c.g_new[e] = ev[e](y_new)
            solved_order, solved_h = order, c.h_abs
        if c.pc == PC_DONE:
            break
    return c, tev, words, n_changed, n_either


def state_bytes(c):
    """the controller without its last action word (a run whose last step has roots ends with A_ROOTS in it)"""
    out = BdfCtl()
    C.memmove(C.byref(out), C.byref(c), C.sizeof(BdfCtl))
    out.action = 0
    return bytes(out)


def roots_of(c, tev, max_events=BIG):
    """per monitor the root times written, by the rule of the C ABI: entry k is valid for k < min(n_events, max_events)"""
    return [tev[e * max_events:e * max_events + min(int(c.n_events[e]), max_events)].copy() for e in range(7)]


_REF = {}


def reference(name):
    """solve_ivp(method="BDF", events=<the seven>) of problem `name` - computed once"""
    if name not in _REF:
        (fun, jac, y0, t_span, first_step, rtol, atol), _ = CASES[name]
        ev = [(lambda t, y, f=f: f(y)) for f in EVENTS[name]]
        _REF[name] = solve_ivp(fun, t_span, y0, method="BDF", jac=jac, rtol=rtol, atol=atol, first_step=first_step, events=ev)
    return _REF[name]


def deviation(got, sol):
    """largest |root - scipy's| / scipy's over the monitors (equal counts asserted)"""
    worst = 0.0
    for e in range(7):
        want = np.asarray(sol.t_events[e])
        assert len(got[e]) == len(want), (e, len(got[e]), len(want))
        assert not np.isnan(got[e]).any()
        if len(want):
            worst = max(worst, float(np.max(np.abs(got[e] - want) / np.abs(want))))
    return worst


def test_the_event_functions_cover_the_cases():
    counts = {name: [len(t) for t in reference(name).t_events] for name in CASES}
    print(counts)
    assert any(k >= 2 for v in counts.values() for k in v)    # a monitor with several roots
    assert any(k == 0 for v in counts.values() for k in v)    # a monitor with none
    assert all(sum(v) > 0 for v in counts.values())
    for name in CASES:
        sol = reference(name)
        assert all(np.all(np.asarray(t) > 0) for t in sol.t_events)
        for (nm, e), step in PLACED.items():
            if nm == name:
                assert sol.t[step] < sol.t_events[e][-1] <= sol.t[step + 1], (nm, e)
    assert len(reference("robertson").t) - 1 == 75 and len(reference("van_der_pol").t) - 1 == 158   # (73 and 156: the steps before the last)


@pytest.mark.parametrize("name", list(CASES))
def test_roots_are_scipys(shim, name):
    sol = reference(name)
    c, tev, words, n_changed, _ = drive(shim, name)
    assert c.status == sol.status
    got = roots_of(c, tev)
    assert [len(g) for g in got] == [int(c.n_events[e]) for e in range(7)] == [len(t) for t in sol.t_events]   # exact
    assert np.isnan(tev).sum() == tev.size - sum(len(g) for g in got)   # nothing else is written
    dev = deviation(got, sol)
    n_roots_words = sum(1 for w in words if w & A_ROOTS)   # (two monitors in one search: fewer searched steps than roots)
    print(f"{name}: roots per monitor {[len(g) for g in got]}, {n_roots_words} searched steps of {c.n_acc}, "
          f"max |root - scipy's| / scipy's = {dev:.3e}")
    assert dev <= ROOT_BOUND
    assert all(np.all(np.diff(g) >= 0) for g in got)
    assert n_roots_words < sum(len(g) for g in got)


@pytest.mark.parametrize("defect", ["before_change_D", "after_next_rescaling", "solved_h"])
def test_the_bound_sees_each_driver_defect(shim, defect):
    worst = 0.0
    for name in CASES:
        sol = reference(name)
        c, tev, _, _, _ = drive(shim, name, defect=defect)
        dev = deviation(roots_of(c, tev), sol)
        print(f"{defect} / {name}: {dev:.3e} = {dev / ROOT_BOUND:.3e} bounds")
        worst = max(worst, dev)
    assert worst > ROOT_BOUND


@pytest.mark.parametrize("name", list(CASES))
def test_max_events_one_counts_on_and_writes_slot_zero(shim, name):
    sol = reference(name)
    full, tev_full, _, _, _ = drive(shim, name)
    c, tev, _, _, _ = drive(shim, name, max_events=1, guard=16)
    assert [int(c.n_events[e]) for e in range(7)] == [len(t) for t in sol.t_events]
    assert state_bytes(c) == state_bytes(full)   # the integration does not see the cap
    assert np.isnan(tev[7:]).all()
    for e in range(7):
        if c.n_events[e]:
            assert tev[e] == tev_full[e * BIG]   # the first root, bit for bit the uncapped run's
        else:
            assert np.isnan(tev[e])


def test_attempt_budget_keeps_the_roots_it_reached(shim):
    full, tev_full, _, _, _ = drive(shim, "robertson")
    c, tev, _, _, _ = drive(shim, "robertson", max_attempts=40)
    assert c.status == 2 and c.t < CASES["robertson"][0][3][1]
    got, want = roots_of(c, tev), roots_of(full, tev_full)
    assert 0 < sum(len(g) for g in got) < sum(len(w) for w in want)
    for e in range(7):
        assert np.array_equal(got[e], want[e][:len(got[e])])   # the leading roots of the full run
        assert np.all(got[e] <= c.t) and np.all(want[e][len(got[e]):] > c.t)


def test_no_step_no_root_when_t1_equals_t0(shim):
    c, tev, words, _, _ = drive(shim, "robertson", t_span=(3.0, 3.0))
    assert (c.status, c.n_acc) == (0, 0) and words == [0] and np.isnan(tev).all() and not any(c.n_events[e] for e in range(7))


@pytest.mark.parametrize("name", list(CASES))
def test_without_roots_the_cycles_are_the_three_argument_calls(shim, name):
    c3, _, w3, _, _ = drive(shim, name, three_args=True)
    cn, tn, wn, _, _ = drive(shim, name, roots=False)
    c0, t0_, w0, _, _ = drive(shim, name, max_events=0, guard=4)
    for cc, ww in ((cn, wn), (c0, w0)):
        assert ww == w3 and bytes(cc) == bytes(c3)
    assert not any(w & A_ROOTS for w in w3) and np.isnan(tn).all() and np.isnan(t0_).all()
    c, _, w, n_changed, _ = drive(shim, name)
    work = lambda ws: [b for x in ws for b in (A_ACCEPT, A_CHANGE_D, A_JAC, A_LU, A_SOLVE) if x & b]  # noqa: E731
    assert work(w) == work(w3)   # the same work in the same order: a searched step only ends its cycle early
    n_words = sum(1 for x in w if x & A_ROOTS)
    assert 0 < len(w) - len(w3) <= n_words <= n_changed
    assert state_bytes(c) == state_bytes(c3)   # locating roots leaves the integration alone


@pytest.mark.parametrize("name", list(CASES))
def test_roots_and_samples_share_a_cycle(shim, name):
    (_, _, _, t_span, first_step, _, _), _ = CASES[name]
    sol = reference(name)
    te = np.unique(np.concatenate([np.linspace(t_span[0], sol.t[-1], 41)[1:], np.concatenate([np.asarray(t) for t in sol.t_events])]))
    c3, _, w3, _, _ = drive(shim, name, three_args=True)
    cr, tev_r, _, _, _ = drive(shim, name)
    c, tev, w, n_changed, n_either = drive(shim, name, t_eval=te)
    assert np.array_equal(tev, tev_r, equal_nan=True)   # the samples do not move the roots
    both = sum(1 for x in w if (x & A_ROOTS) and (x & A_SAMPLE))
    print(f"{name}: {len(w) - len(w3)} extra cycles, {n_either} steps with roots or samples, {both} with both")
    assert len(w) - len(w3) <= sum(1 for x in w if x & (A_ROOTS | A_SAMPLE)) <= n_either
    assert all((w_ & (A_ROOTS | A_SAMPLE)) == 0 or not (w_ & (A_JAC | A_LU | A_SOLVE)) for w_ in w)   # such a cycle ends there
