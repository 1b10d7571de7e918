"""The terminal form of csrc/marl_bdf_ctl.h (struct BdfTerm, A_TERM_ROOTS, A_STOP, PC_TERM): a BDF sweep's instance that a terminal
monitor ends at its root, driven on the CPU in lockstep with scipy.  The header is built alone by a host C++ compiler with a shim of
its own, as tests/test_bdf_roots_control_cpu.py builds it (its CASES / EVENTS / PLACED are imported, not repeated); the data-parallel
work of every action bit is done with scipy's pieces in the order the header documents:
    A_ACCEPT, A_CHANGE_D, A_ROOTS / A_TERM_ROOTS, A_SAMPLE, A_STOP, A_JAC, A_LU, A_SOLVE.
A_TERM_ROOTS is served by the header's own bdf_locate_term_roots through the shim; A_SAMPLE and A_STOP form the dense state from the
driver's own D as the sweep's kernels form it (D[0] + sum_j D[j + 1] p[j], p from the header's bdf_dense_weights).

Held to solve_ivp(method="BDF", events=...) with event.terminal = k (an int: scipy >= 1.13), for every problem the limits
    later    the later of the two monitors whose roots share a step (robertson 47, van der Pol 78, blow-up 6): the earlier is kept;
    earlier  the earlier of the two: the later never happened;
    second   k = 2 on a monitor with two roots (robertson, van der Pol; the blow-up has none);
    never    a limit that is never met (one more than the monitor's roots): status 0, the action words and bytes of the run without a BdfTerm.
Checked: status 1; the number of roots of every monitor equals scipy's and the controller's n_events; t_stop and every root within
ROOT_BOUND (2.1e-14 relative, the bound of tests/test_bdf_roots_control_cpu.py) of scipy's; the samples t_eval <= t_stop and no others
(scipy's sol.t with the same t_eval), each equal to the state the driver forms; max_events = 1 and no BdfRoots at all stop at the
same t_stop, bit for bit, with the same counts.

The stop state against scipy's sol.y[:, -1].  Measured with the finished code (scipy 1.15.3), the largest |y - scipy's| / |scipy's|
over the components, over all cases: 7.2e-16 (robertson 7.2e-16, van_der_pol 1.9e-16, blow_up 0; the sum is formed term by
term, scipy's by a dot product).  STATE_BOUND = 7.2e-15 is 10 times the largest.  Both injected driver defects exceed it (asserted
for each; measured, the worst case, in units of the bound: before_change_D 8.7e12, solved_h 7.9e12; a terminal step without an
order / step-size selection shows neither):
    the stop state taken before the selection's change_D;  the solved step's h_abs in place of the post-selection one.

Without a BdfTerm (m == nullptr) the eight-argument call gives the action words and the bytes of BdfCtl / BdfSample / BdfRoots of the
six-argument call, whose sizes are those the existing tests mirror."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from scipy.integrate import solve_ivp
from scipy.integrate._ivp import bdf as scipy_bdf
from scipy.linalg import lu_factor, lu_solve

from test_bdf_control_cpu import A_ACCEPT, A_CHANGE_D, A_JAC, A_LU, A_SOLVE, CASES, CSRC, PC_DONE, BdfCtl
from test_bdf_frames_control_cpu import A_SAMPLE, BdfSample
from test_bdf_roots_control_cpu import A_ROOTS, BIG, EVAL_FN, EVENTS, PLACED, ROOT_BOUND, BdfRoots

A_TERM_ROOTS, A_STOP = 128, 256
STATE_BOUND = 7.2e-15   # relative, per component: 10 times the largest measured deviation (docstring)

SHIM = r"""
#include "marl_bdf_ctl.h"
using namespace marl::bdfctl;
typedef void (*eval_fn)(double tq, double* g);   // the seven monitors of the dense state at tq
extern "C" {
int bdf_ctl_sizeof() { return (int)sizeof(BdfCtl); }
int bdf_smp_sizeof() { return (int)sizeof(BdfSample); }
int bdf_roots_sizeof() { return (int)sizeof(BdfRoots); }
int bdf_term_sizeof() { return (int)sizeof(BdfTerm); }
int bdf_ctl_a_term_roots() { return A_TERM_ROOTS; }
int bdf_ctl_a_stop() { return A_STOP; }
void bdf_ctl_init(BdfCtl* c, double t0, double t1, double first_step, double rtol, double atol, long long max_attempts)
{
    bdf_control_init(*c, t0, t1, first_step, rtol, atol, max_attempts);
}
void bdf_smp_init(BdfSample* s, long long n_eval) { bdf_sample_init(*s, n_eval); }
void bdf_rts_init(BdfRoots* r, long long max_events) { bdf_roots_init(*r, max_events); }
void bdf_trm_init(BdfTerm* m, const long long* terminal)
{
    int64_t k[7];
    for (int e = 0; e < 7; e++) k[e] = terminal[e];
    bdf_term_init(*m, k);
}
void bdf_ctl_step6(BdfCtl* c, long long n, const double* g0, BdfSample* s, const double* t_eval, BdfRoots* r) { bdf_control_step(*c, n, g0, s, t_eval, r); }
void bdf_ctl_step8(BdfCtl* c, long long n, const double* g0, BdfSample* s, const double* t_eval, BdfRoots* r, BdfTerm* m, double* t_events)
{
    bdf_control_step(*c, n, g0, s, t_eval, r, m, t_events);
}
void bdf_rts_locate(const BdfRoots* r, eval_fn f, double* t_events)
{
    bdf_locate_roots(*r, [f](double tq, int e) { double g[7]; f(tq, g); return g[e]; }, t_events);
}
void bdf_trm_locate(BdfTerm* m, eval_fn f)
{
    bdf_locate_term_roots(*m, [f](double tq, int e) { double g[7]; f(tq, g); return g[e]; });
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


class BdfTerm(C.Structure):
    _fields_ = [("terminal", C.c_int64 * 7), ("root", C.c_double * 7), ("t_old", C.c_double), ("t", C.c_double), ("h", C.c_double),
                ("t_stop", C.c_double), ("order", C.c_int32), ("active", C.c_int32), ("stopped", C.c_int32), ("pad", C.c_int32)]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("bdfterm")
    src, so = d / "bdf_term_shim.cpp", d / "libbdf_term_shim.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    P, D, L = C.POINTER, C.c_double, C.c_longlong
    lib.bdf_ctl_init.argtypes = [P(BdfCtl)] + [D] * 5 + [L]
    lib.bdf_smp_init.argtypes = [P(BdfSample), L]
    lib.bdf_rts_init.argtypes = [P(BdfRoots), L]
    lib.bdf_trm_init.argtypes = [P(BdfTerm), P(L)]
    lib.bdf_ctl_step6.argtypes = [P(BdfCtl), L, P(D), P(BdfSample), P(D), P(BdfRoots)]
    lib.bdf_ctl_step8.argtypes = [P(BdfCtl), L, P(D), P(BdfSample), P(D), P(BdfRoots), P(BdfTerm), P(D)]
    lib.bdf_rts_locate.argtypes = [P(BdfRoots), EVAL_FN, P(D)]
    lib.bdf_trm_locate.argtypes = [P(BdfTerm), EVAL_FN]
    lib.bdf_weights.argtypes = [D, D, C.c_int, D, P(D)]
    for f in (lib.bdf_ctl_init, lib.bdf_smp_init, lib.bdf_rts_init, lib.bdf_trm_init, lib.bdf_ctl_step6, lib.bdf_ctl_step8, lib.bdf_rts_locate,
              lib.bdf_trm_locate, lib.bdf_weights):
        f.restype = None
    lib.bdf_ctl_gamma.argtypes = [C.c_int]
    lib.bdf_ctl_gamma.restype = D
    assert lib.bdf_ctl_sizeof() == C.sizeof(BdfCtl), "BdfCtl must keep its size (tests/test_bdf_control_cpu.py mirrors it)"
    assert lib.bdf_smp_sizeof() == C.sizeof(BdfSample), "BdfSample must keep its size (tests/test_bdf_frames_control_cpu.py mirrors it)"
    assert lib.bdf_roots_sizeof() == C.sizeof(BdfRoots), "BdfRoots must keep its size (tests/test_bdf_roots_control_cpu.py mirrors it)"
    assert lib.bdf_term_sizeof() == C.sizeof(BdfTerm), "the ctypes mirror of BdfTerm is out of date"
    assert (lib.bdf_ctl_a_term_roots(), lib.bdf_ctl_a_stop()) == (A_TERM_ROOTS, A_STOP)
    return lib


class Run:
    """what drive() returns"""


def drive(lib, name, terminal=None, max_events=BIG, roots=True, t_eval=None, six_args=False, defect=None):
    """The cycle of the sweep's host driver for one instance of problem `name`, scipy's pieces as the kernels.  terminal: the seven
    limits, or None - the controller gets no BdfTerm (six_args: through the six-argument call).  roots False: no BdfRoots and no
    t_events.  defect: None, or an injected driver mistake in A_STOP: "before_change_D" (the stop state is formed from D as it was
    before the terminal step's rescaling), "solved_h" (its weights use the solved step's h_abs)."""
    (fun, jac, y0, (t0, t1), first_step, rtol, atol), _ = CASES[name]
    ev = EVENTS[name]
    y0 = np.asarray(y0, float)
    n = y0.size
    gamma = np.array([lib.bdf_ctl_gamma(k) for k in range(6)])
    c, s, r, m = BdfCtl(), BdfSample(), BdfRoots(), BdfTerm()
    lib.bdf_ctl_init(C.byref(c), t0, t1, first_step, rtol, atol, 0)
    te = np.ascontiguousarray([] if t_eval is None else t_eval, dtype=np.float64)
    lib.bdf_smp_init(C.byref(s), te.size)
    lib.bdf_rts_init(C.byref(r), max_events)
    lib.bdf_trm_init(C.byref(m), (C.c_longlong * 7)(*(terminal or [0] * 7)))
    te_p = te.ctypes.data_as(C.POINTER(C.c_double))
    tev = np.full(7 * max(max_events, 0), np.nan)
    tev_p = tev.ctypes.data_as(C.POINTER(C.c_double))
    D = np.zeros((8, n))
    D[0] = y0
    D[1] = fun(t0, y0) * first_step
    J = jac(t0, y0)
    LU = y_predict = psi = scale = y_new = d = D_before = None
    g0 = (C.c_double * 7)(*[f(y0) for f in ev])
    eye = np.identity(n)
    out = Run()
    out.words, out.frames, out.y = [], {}, None
    solved_order, solved_h = 1, first_step
    p = (C.c_double * 6)()

    def dense(Dm, t, h, order, tq):
        lib.bdf_weights(t, h, order, tq, p)
        a = np.zeros(n)
        for j in range(order):
            a = a + Dm[j + 1] * p[j]
        return a + Dm[0]

    def monitors_on(snap):
        def monitors(tq, g):
            y = dense(D, snap.t, snap.h, snap.order, tq)
            for e in range(7):
                g[e] = ev[e](y)
        return EVAL_FN(monitors)

    while True:
        smp = C.byref(s) if t_eval is not None else None
        if six_args:
            lib.bdf_ctl_step6(C.byref(c), n, g0, smp, te_p if t_eval is not None else None, C.byref(r) if roots else None)
        else:
            lib.bdf_ctl_step8(C.byref(c), n, g0, smp, te_p if t_eval is not None else None, C.byref(r) if roots else None,
                              C.byref(m) if terminal is not None else None, tev_p if roots else None)
        out.words.append(c.action)
        assert len(out.words) < 100000
        a = c.action
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
            out.y = y_new.copy()
        if a & A_TERM_ROOTS:
            D_before = D.copy()
        if a & A_CHANGE_D:
            o = c.ru_order
            RU = np.array([[c.RU[i][j] for j in range(o + 1)] for i in range(o + 1)])
            D[:o + 1] = RU.T @ D[:o + 1].copy()
        if a & A_ROOTS:
            lib.bdf_rts_locate(C.byref(r), monitors_on(r), tev_p)
        if a & A_TERM_ROOTS:
            lib.bdf_trm_locate(C.byref(m), monitors_on(m))
        if a & A_SAMPLE:
            for k in range(s.first, s.end):
                assert k not in out.frames
                out.frames[k] = dense(D, s.t, s.h, s.order, te[k])
        if a & A_STOP:
            out.y = dense(D_before if defect == "before_change_D" else D, m.t, solved_h if defect == "solved_h" else m.h, m.order, m.t_stop)
            for e in range(7):
                c.g[e] = ev[e](out.y)
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
    out.c, out.s, out.r, out.m, out.tev = c, s, r, m, tev
    out.roots = [tev[e * max_events:e * max_events + min(int(c.n_events[e]), max_events)].copy() for e in range(7)] if max_events > 0 else [np.empty(0)] * 7
    return out


_REF = {}


def reference(name, terminal=None, t_eval=None):
    """solve_ivp(method="BDF", events=<the seven>, event.terminal = the limits) of problem `name` - each computed once"""
    key = (name, tuple(terminal or ()), None if t_eval is None else tuple(t_eval))
    if key not in _REF:
        (fun, jac, y0, t_span, first_step, rtol, atol), _ = CASES[name]
        ev = []
        for e, f in enumerate(EVENTS[name]):
            g = lambda t, y, f=f: f(y)  # noqa: E731
            g.terminal = int(terminal[e]) if terminal else False
            ev.append(g)
        _REF[key] = solve_ivp(fun, t_span, y0, method="BDF", jac=jac, rtol=rtol, atol=atol, first_step=first_step, events=ev, t_eval=t_eval)
    return _REF[key]


def shared_pair(name):
    """the two monitors whose (last) roots lie in one accepted step of scipy's run, (earlier, later) by root time"""
    by_step = {}
    for (nm, e), step in PLACED.items():
        if nm == name:
            by_step.setdefault(step, []).append(e)
    pair = next(v for v in by_step.values() if len(v) == 2)
    sol = reference(name)
    assert all(len(sol.t_events[e]) == 1 for e in pair)
    return tuple(sorted(pair, key=lambda e: sol.t_events[e][0]))


def limits(name, kind):
    """the seven limits of case `kind` (docstring), or None where the problem has no such case"""
    sol = reference(name)
    k = [0] * 7
    if kind in ("later", "earlier"):
        k[shared_pair(name)[kind == "later"]] = 1
    elif kind == "second":
        two = [e for e in range(7) if len(sol.t_events[e]) == 2]
        if not two:
            return None
        k[two[0]] = 2
    else:
        for e in range(7):
            k[e] = len(sol.t_events[e]) + 1
    return k


STOPPING = [(name, kind) for name in CASES for kind in ("later", "earlier", "second") if not (name == "blow_up" and kind == "second")]


def test_the_cases_exist():
    assert all(limits(name, kind) is not None for name, kind in STOPPING) and limits("blow_up", "second") is None
    for name in CASES:
        early, late = shared_pair(name)
        sol = reference(name)
        assert sol.t_events[early][0] < sol.t_events[late][0]
        n_late = reference(name, limits(name, "later")).t_events
        n_early = reference(name, limits(name, "earlier")).t_events
        assert len(n_late[early]) == 1 and len(n_late[late]) == 1       # the earlier is kept
        assert len(n_early[early]) == 1 and len(n_early[late]) == 0     # the later never happened


def relative(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(np.asarray(b))))


@pytest.mark.parametrize("name, kind", STOPPING)
def test_a_terminal_monitor_stops_the_run_where_scipy_stops(shim, name, kind):
    k = limits(name, kind)
    sol = reference(name, k)
    assert sol.status == 1
    run = drive(shim, name, k)
    c, m = run.c, run.m
    assert c.status == 1 and c.pc == PC_DONE and m.stopped == 1 and c.t == m.t_stop
    counts = [len(t) for t in sol.t_events]
    assert [len(g) for g in run.roots] == [int(c.n_events[e]) for e in range(7)] == counts   # exact
    assert np.isnan(run.tev).sum() == run.tev.size - sum(counts)                             # nothing else is written
    dev_stop = abs(m.t_stop - sol.t[-1]) / abs(sol.t[-1])
    dev_roots = max([relative(run.roots[e], sol.t_events[e]) for e in range(7) if counts[e]], default=0.0)
    dev_y = relative(run.y, sol.y[:, -1])
    print(f"{name} / {kind}: limits {k}, roots {counts}, t_stop {m.t_stop!r} (scipy {sol.t[-1]!r}: {dev_stop:.2e}), roots {dev_roots:.2e}, "
          f"stop state {dev_y:.3e} = {dev_y / STATE_BOUND:.2f} bounds")
    assert dev_stop <= ROOT_BOUND and dev_roots <= ROOT_BOUND
    assert dev_y <= STATE_BOUND
    assert [c.g[e] for e in range(7)] == [f(run.y) for f in EVENTS[name]]                    # the monitors are the stop state's own
    assert run.words[-2] & A_TERM_ROOTS and not (run.words[-2] & (A_ROOTS | A_SAMPLE | A_JAC | A_LU | A_SOLVE))
    assert run.words[-1] == A_STOP and sum(1 for w in run.words if w & (A_TERM_ROOTS | A_STOP)) == 2
    free = drive(shim, name)                                                                 # up to the terminal step it IS the run without limits
    i = len(run.words) - 2
    assert run.words[:i] == free.words[:i] and run.words[i] == free.words[i] - A_ROOTS + A_TERM_ROOTS
    for e in range(7):
        assert np.array_equal(run.roots[e], free.roots[e][:counts[e]])                       # bit for bit


@pytest.mark.parametrize("name, kind", STOPPING)
def test_the_samples_up_to_t_stop_and_no_others(shim, name, kind):
    k = limits(name, kind)
    t_stop = reference(name, k).t[-1]
    (_, _, _, (t0, t1), _, _, _), _ = CASES[name]
    plain = drive(shim, name, k)
    te = np.unique(np.concatenate([np.linspace(t0, t1, 23), t0 + (plain.m.t_stop - t0) * np.array([0.5, 0.9, 0.999]),
                                   [plain.m.t_stop, np.nextafter(plain.m.t_stop, np.inf)]]))
    knife = np.isin(te, [plain.m.t_stop, np.nextafter(plain.m.t_stop, np.inf)])   # (scipy's t_stop is a few ulp from the controller's)
    sol = reference(name, k, te[~knife])
    run = drive(shim, name, k, t_eval=te)
    assert run.m.t_stop == plain.m.t_stop and np.array_equal(run.y, plain.y) and np.array_equal(run.tev, plain.tev, equal_nan=True)
    n_done = int(np.searchsorted(te, run.m.t_stop, side="right"))
    assert run.s.next == n_done == len(sol.t) + 1 and sorted(run.frames) == list(range(n_done))
    assert te[n_done - 1] == run.m.t_stop and np.array_equal(run.frames[n_done - 1], run.y)   # the state returned is the frame at t_stop
    assert abs(t_stop - run.m.t_stop) <= ROOT_BOUND * t_stop
    assert run.s.t == run.m.t and run.s.t >= run.m.t_stop                                     # BdfSample.t stays the step's end
    got = np.array([run.frames[i] for i in range(n_done - 1)]).T
    (_, _, _, _, _, rtol, atol), _ = CASES[name]
    dev = float(np.max(np.abs(got - sol.y) / (atol + rtol * np.abs(sol.y))))
    print(f"{name} / {kind}: {n_done} of {te.size} samples, largest |frame - sol.y| / (atol + rtol |sol.y|) = {dev:.2e}")
    assert dev <= 9.6e-11                                                                     # FRAME_BOUND of tests/test_bdf_frames_control_cpu.py


@pytest.mark.parametrize("name, kind", STOPPING)
def test_no_slot_and_no_roots_stop_at_the_same_time(shim, name, kind):
    k = limits(name, kind)
    full = drive(shim, name, k)
    one = drive(shim, name, k, max_events=1)
    none = drive(shim, name, k, roots=False)
    for run in (one, none):
        assert run.c.status == 1 and run.m.t_stop == full.m.t_stop and np.array_equal(run.y, full.y)
        assert [int(run.c.n_events[e]) for e in range(7)] == [int(full.c.n_events[e]) for e in range(7)]
    for e in range(7):
        if full.c.n_events[e]:
            assert one.tev[e] == full.roots[e][0]
        else:
            assert np.isnan(one.tev[e])
    assert np.isnan(none.tev).all() and not any(w & A_ROOTS for w in none.words) and none.words[-1] == A_STOP


@pytest.mark.parametrize("defect", ["before_change_D", "solved_h"])
def test_the_bound_sees_each_driver_defect(shim, defect):
    worst = 0.0
    for name, kind in STOPPING:
        k = limits(name, kind)
        dev = relative(drive(shim, name, k, defect=defect).y, reference(name, k).y[:, -1])
        print(f"{defect} / {name} / {kind}: {dev:.3e} = {dev / STATE_BOUND:.3e} bounds")
        worst = max(worst, dev)
    assert worst > STATE_BOUND


@pytest.mark.parametrize("name", list(CASES))
def test_a_limit_never_met_changes_nothing(shim, name):
    k = limits(name, "never")
    te = np.linspace(*CASES[name][0][3], 17)
    for t_eval in (None, te):
        free = drive(shim, name, None, t_eval=t_eval)
        run = drive(shim, name, k, t_eval=t_eval)
        assert run.c.status == reference(name).status and run.m.stopped == 0 and run.m.active == 0
        assert run.words == free.words and bytes(run.c) == bytes(free.c) and bytes(run.s) == bytes(free.s) and bytes(run.r) == bytes(free.r)
        assert np.array_equal(run.tev, free.tev, equal_nan=True)


@pytest.mark.parametrize("name", list(CASES))
def test_without_a_bdfterm_the_existing_call_forms_are_unchanged(shim, name):
    te = np.linspace(*CASES[name][0][3], 17)
    for kw in ({}, {"roots": False}, {"t_eval": te}, {"t_eval": te, "roots": False}, {"max_events": 0}):
        old = drive(shim, name, None, six_args=True, **kw)
        new = drive(shim, name, None, **kw)
        assert new.words == old.words and not any(w & (A_TERM_ROOTS | A_STOP) for w in new.words)
        assert bytes(new.c) == bytes(old.c) and bytes(new.s) == bytes(old.s) and bytes(new.r) == bytes(old.r)
        assert np.array_equal(new.tev, old.tev, equal_nan=True)
