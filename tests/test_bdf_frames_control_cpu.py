"""The sampling form of csrc/marl_bdf_ctl.h (struct BdfSample, A_SAMPLE, bdf_dense_weights): the t_eval samples of the BDF sweep,
driven on the CPU in lockstep with scipy.  The header is built alone by a host C++ compiler, as tests/test_bdf_control_cpu.py builds
it, with a shim of its own; the data-parallel work of every action bit is done with scipy's pieces in the order the header documents:
A_ACCEPT, A_CHANGE_D, A_SAMPLE, A_JAC, A_LU, A_SOLVE.  A sample is formed from the driver's own D as the sweep's kernel forms it:
D[0] + sum_j D[j + 1] p[j] with p from the header's bdf_dense_weights.

Held to scipy (the three problems of test_bdf_control_cpu.py; t_eval = t0, 80 log-spaced early times, 118 uniform late ones, t1, and
one accepted step time of scipy's own run, so that `t_eval[i] <= t` is exercised at equality):
  * at every step with samples the published snapshot is scipy.integrate.BDF's dense output of that step: order and sample index range
    exact, t and h to 1e-9 relative (the bound test_bdf_control_cpu.py puts on step times);
  * the frames agree with solve_ivp(method="BDF", t_eval=...).y.  Measured with the finished code (scipy 1.15.3), largest
    |frame - sol.y| / (atol + rtol |sol.y|) over a run: robertson 9.6e-12, van_der_pol 0, blow_up 1.8e-13 (the controller's error
    norm is a few ulp from scipy's, see test_bdf_control_cpu.py; the sum of a frame is formed term by term, scipy's by a dot product).
    FRAME_BOUND = 9.6e-11 is 10 times the largest.  Each of the three injected driver defects exceeds it by at least 1e3 (asserted;
    measured, the worst of the three problems: 1.6e3, 2.9e1 and 7.1e3 of those units):
        sampling before the selection's change_D;  sampling after the next step's clip / min_step rescaling;
        the solved step's h_abs in place of the post-selection one;
  * n_done of a max_attempts-limited run is searchsorted(t_eval, t_reached, "right");
  * driven through the three-argument call, the action words and the cycle count of a run are those of the sampling form with n_eval = 0."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from scipy.integrate import solve_ivp
from scipy.integrate._ivp import bdf as scipy_bdf
from scipy.linalg import lu_factor, lu_solve

from test_bdf_control_cpu import A_ACCEPT, A_CHANGE_D, A_JAC, A_LU, A_SOLVE, CASES, CSRC, PC_DONE, BdfCtl

A_SAMPLE = 32
FRAME_BOUND = 9.6e-11   # in units of atol + rtol |sol.y|: 10 times the largest measured deviation (docstring)

SHIM = r"""
#include "marl_bdf_ctl.h"
using namespace marl::bdfctl;
extern "C" {
int bdf_ctl_sizeof() { return (int)sizeof(BdfCtl); }
int bdf_smp_sizeof() { return (int)sizeof(BdfSample); }
int bdf_ctl_a_sample() { return A_SAMPLE; }
void bdf_ctl_init(BdfCtl* c, double t0, double t1, double first_step, double rtol, double atol, long long max_attempts)
{
    bdf_control_init(*c, t0, t1, first_step, rtol, atol, max_attempts);
}
void bdf_smp_init(BdfSample* s, long long n_eval) { bdf_sample_init(*s, n_eval); }
void bdf_ctl_step3(BdfCtl* c, long long n, const double* g0) { bdf_control_step(*c, n, g0); }
void bdf_ctl_step5(BdfCtl* c, long long n, const double* g0, BdfSample* s, const double* t_eval) { bdf_control_step(*c, n, g0, s, t_eval); }
void bdf_weights(double t, double h, int order, double tq, double* p)
{
    double w[MAX_ORDER + 1];
    bdf_dense_weights(t, h, order, tq, w);
    for (int j = 0; j <= MAX_ORDER; j++) p[j] = w[j];
}
double bdf_ctl_gamma(int k) { return gamma_of(k); }
}
"""


class BdfSample(C.Structure):
    _fields_ = [("n_eval", C.c_int64), ("next", C.c_int64), ("t", C.c_double), ("h", C.c_double), ("first", C.c_int64), ("end", C.c_int64),
                ("order", C.c_int32), ("pad", C.c_int32)]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("bdfframes")
    src, so = d / "bdf_frames_shim.cpp", d / "libbdf_frames_shim.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.bdf_ctl_init.argtypes = [C.POINTER(BdfCtl)] + [C.c_double] * 5 + [C.c_longlong]
    lib.bdf_ctl_init.restype = None
    lib.bdf_smp_init.argtypes = [C.POINTER(BdfSample), C.c_longlong]
    lib.bdf_smp_init.restype = None
    lib.bdf_ctl_step3.argtypes = [C.POINTER(BdfCtl), C.c_longlong, C.POINTER(C.c_double)]
    lib.bdf_ctl_step3.restype = None
    lib.bdf_ctl_step5.argtypes = [C.POINTER(BdfCtl), C.c_longlong, C.POINTER(C.c_double), C.POINTER(BdfSample), C.POINTER(C.c_double)]
    lib.bdf_ctl_step5.restype = None
    lib.bdf_weights.argtypes = [C.c_double, C.c_double, C.c_int, C.c_double, C.POINTER(C.c_double)]
    lib.bdf_weights.restype = None
    lib.bdf_ctl_gamma.argtypes = [C.c_int]
    lib.bdf_ctl_gamma.restype = C.c_double
    assert lib.bdf_ctl_sizeof() == C.sizeof(BdfCtl), "BdfCtl must keep its size (tests/test_bdf_control_cpu.py mirrors it)"
    assert lib.bdf_smp_sizeof() == C.sizeof(BdfSample), "the ctypes mirror of BdfSample is out of date"
    assert lib.bdf_ctl_a_sample() == A_SAMPLE
    return lib


def drive(lib, fun, jac, y0, t_span, first_step, rtol, atol, t_eval=None, max_attempts=0, three_args=False, defect=None):
    """The cycle of the sweep's host driver for one instance, scipy's pieces as the kernels.  t_eval None: the controller gets no
    BdfSample (three_args: through the three-argument call).  defect: None, or one of the three injected driver mistakes:
    "before_change_D" (the samples are taken before the cycle's rescaling), "after_next_rescaling" (they are taken in the NEXT cycle,
    after its rescaling), "solved_h" (the weights use the solved step's h_abs).
    Returns (controller, sample state, frames (n_eval, n), snapshots [(t, h, order, first, end)], action words)."""
    t0, t1 = t_span
    y0 = np.asarray(y0, float)
    n = y0.size
    gamma = np.array([lib.bdf_ctl_gamma(k) for k in range(6)])
    c, s = BdfCtl(), BdfSample()
    lib.bdf_ctl_init(C.byref(c), t0, t1, first_step, rtol, atol, max_attempts)
    te = np.ascontiguousarray([] if t_eval is None else t_eval, dtype=np.float64)
    lib.bdf_smp_init(C.byref(s), te.size)
    te_p = te.ctypes.data_as(C.POINTER(C.c_double))
    frames = np.full((te.size, n), np.nan)
    D = np.zeros((8, n))
    D[0] = y0
    D[1] = fun(t0, y0) * first_step
    J = jac(t0, y0)
    LU = y_predict = psi = scale = y_new = d = None
    g0 = (C.c_double * 7)(*([1.0] * 7))
    eye = np.identity(n)
    snaps, words, solved_order, solved_h, pending = [], [], 1, first_step, None
    p = (C.c_double * 6)()

    def sample(snap, h):
        t, _, order, first, end = snap
        for k in range(first, end):
            lib.bdf_weights(t, h, order, te[k], p)
            a = np.zeros(n)
            for j in range(order):
                a = a + D[j + 1] * p[j]
            frames[k] = a + D[0]

    while True:
        if three_args:
            lib.bdf_ctl_step3(C.byref(c), n, g0)
        else:
            lib.bdf_ctl_step5(C.byref(c), n, g0, C.byref(s) if t_eval is not None else None, te_p if t_eval is not None else None)
        words.append(c.action)
        assert len(words) < 100000
        a = c.action
        snap = (s.t, s.h, s.order, s.first, s.end) if a & A_SAMPLE else None
        if snap:
            snaps.append(snap)
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
        if snap and defect == "before_change_D":
            sample(snap, snap[1])
        if a & A_CHANGE_D:
            o = c.ru_order
            RU = np.array([[c.RU[i][j] for j in range(o + 1)] for i in range(o + 1)])
            D[:o + 1] = RU.T @ D[:o + 1].copy()
        if pending is not None:   # (defect "after_next_rescaling": the previous cycle's samples, after this cycle's rescaling)
            sample(pending, pending[1])
            pending = None
        if snap and defect is None:
            sample(snap, snap[1])
        if snap and defect == "solved_h":
            sample(snap, solved_h)
        if snap and defect == "after_next_rescaling":
            if c.pc == PC_DONE:
                sample(snap, snap[1])
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
            solved_order, solved_h = order, c.h_abs
        if c.pc == PC_DONE:
            break
    return c, s, frames, snaps, words


_REF = {}


def reference(name):
    """(t_eval, solve_ivp's result with it, scipy's dense output per step with samples [(t, h, order, first, end)]) - computed once."""
    if name not in _REF:
        (fun, jac, y0, t_span, first_step, rtol, atol), _ = CASES[name]
        kw = dict(method="BDF", jac=jac, rtol=rtol, atol=atol, first_step=first_step)
        plain = solve_ivp(fun, t_span, y0, **kw)
        t0, t1 = t_span
        t_end = plain.t[-1]   # (blow_up ends early: the samples cover what the run reaches, and t1 beyond it)
        mid = t0 + 0.05 * (t_end - t0)
        te = np.unique(np.concatenate([[t0], np.geomspace(t0 + 1e-3 * first_step + first_step, mid, 80), np.linspace(mid, t_end, 119)[1:],
                                       [plain.t[len(plain.t) // 2], t1]]))
        assert plain.t[len(plain.t) // 2] in te and te[0] == t0 and te[-1] == t1 and te.size >= 195
        sol = solve_ivp(fun, t_span, y0, t_eval=te, **kw)
        s = scipy_bdf.BDF(fun, t0, np.asarray(y0, float), t1, first_step=first_step, rtol=rtol, atol=atol, jac=jac)
        dense, i = [], 0
        while s.status == "running":
            s.step()
            if s.status == "failed":
                break
            e = int(np.searchsorted(te, s.t, side="right"))
            if e > i:   # BdfDenseOutput(t_old, t, h_abs * direction, order, D[:order + 1]) of the solver after the step (bdf.py:452-454)
                o = s.dense_output()
                assert o.t == s.t and o.order == s.order and np.array_equal(o.t_shift, s.t - s.h_abs * np.arange(s.order))
                dense.append((s.t, s.h_abs, s.order, i, e))
                i = e
        _REF[name] = (te, sol, dense)
    return _REF[name]


def deviation(frames, sol, rtol, atol):
    k = sol.y.shape[1]
    assert not np.isnan(frames[:k]).any()
    return float(np.max(np.abs(frames[:k].T - sol.y) / (atol + rtol * np.abs(sol.y))))


@pytest.mark.parametrize("name", list(CASES))
def test_snapshots_and_frames_are_scipys(shim, name):
    (fun, jac, y0, t_span, first_step, rtol, atol), _ = CASES[name]
    te, sol, dense = reference(name)
    c, s, frames, snaps, words = drive(shim, fun, jac, y0, t_span, first_step, rtol, atol, t_eval=te)
    assert c.status == sol.status and s.n_eval == te.size
    assert s.next == sol.t.size == int(np.searchsorted(te, c.t, side="right"))
    assert np.array_equal(te[:s.next], sol.t)
    assert np.isnan(frames[s.next:]).all()   # later frames are not written
    assert len(snaps) == len(dense)
    assert [x[2:] for x in snaps] == [x[2:] for x in dense]   # order, first, end: exact
    np.testing.assert_allclose([x[0] for x in snaps], [x[0] for x in dense], rtol=1e-9, atol=0)
    np.testing.assert_allclose([x[1] for x in snaps], [x[1] for x in dense], rtol=1e-9, atol=0)
    assert any(x[4] - x[3] > 1 for x in snaps) and len(snaps) < c.n_acc   # steps with several samples, steps with none
    assert any(x[0] == te[x[4] - 1] for x in dense)   # a sample exactly at a step's end (scipy's own step time)
    dev = deviation(frames, sol, rtol, atol)
    print(f"{name}: {len(snaps)} sampled steps of {c.n_acc}, {s.next} of {te.size} frames, max |frame - sol.y| / (atol + rtol |sol.y|) = {dev:.3e}")
    assert dev <= FRAME_BOUND
    assert sum(1 for w in words if w & A_SAMPLE) == len(snaps) <= te.size


@pytest.mark.parametrize("defect", ["before_change_D", "after_next_rescaling", "solved_h"])
def test_the_bound_sees_each_driver_defect(shim, defect):
    worst = 0.0
    for name in CASES:
        (fun, jac, y0, t_span, first_step, rtol, atol), _ = CASES[name]
        te, sol, _ = reference(name)
        _, s, frames, _, _ = drive(shim, fun, jac, y0, t_span, first_step, rtol, atol, t_eval=te, defect=defect)
        assert s.next == sol.t.size
        dev = deviation(frames, sol, rtol, atol)
        print(f"{defect} / {name}: {dev:.3e}")
        worst = max(worst, dev)
    assert worst >= 1e3 * FRAME_BOUND


def test_attempt_budget_keeps_the_frames_it_reached(shim):
    (fun, jac, y0, t_span, first_step, rtol, atol), _ = CASES["robertson"]
    te, sol, _ = reference("robertson")
    c, s, frames, snaps, _ = drive(shim, fun, jac, y0, t_span, first_step, rtol, atol, t_eval=te, max_attempts=25)
    assert c.status == 2 and c.t < t_span[1]
    k = int(np.searchsorted(te, c.t, side="right"))
    assert s.next == k and 0 < k < te.size
    assert not np.isnan(frames[:k]).any() and np.isnan(frames[k:]).all()
    assert np.max(np.abs(frames[:k].T - sol.y[:, :k]) / (atol + rtol * np.abs(sol.y[:, :k]))) <= FRAME_BOUND


def test_no_step_no_frame_when_t1_equals_t0(shim):
    (fun, jac, y0, _, first_step, rtol, atol), _ = CASES["robertson"]
    c, s, frames, snaps, words = drive(shim, fun, jac, y0, (3.0, 3.0), first_step, rtol, atol, t_eval=[3.0])
    assert (c.status, c.n_acc, s.next) == (0, 0, 0) and words == [0] and snaps == [] and np.isnan(frames).all()


@pytest.mark.parametrize("name", list(CASES))
def test_without_samples_the_cycles_are_the_three_argument_calls(shim, name):
    (fun, jac, y0, t_span, first_step, rtol, atol), _ = CASES[name]
    c3, _, _, _, w3 = drive(shim, fun, jac, y0, t_span, first_step, rtol, atol, three_args=True)
    c0, s0, _, snaps, w0 = drive(shim, fun, jac, y0, t_span, first_step, rtol, atol, t_eval=[])
    assert w3 == w0 and len(w3) == len(w0) and snaps == [] and s0.next == 0
    assert bytes(c3) == bytes(c0)
    assert not any(w & A_SAMPLE for w in w3)
    te, _, dense = reference(name)
    _, _, _, snaps, w = drive(shim, fun, jac, y0, t_span, first_step, rtol, atol, t_eval=te)
    work = lambda ws: [b for x in ws for b in (A_ACCEPT, A_CHANGE_D, A_JAC, A_LU, A_SOLVE) if x & b]  # noqa: E731
    assert work(w) == work(w3)   # the same work in the same order: a sampled step only ends its cycle early
    assert len(w) - len(w3) <= len(snaps) <= te.size   # at most one more cycle per step with samples
