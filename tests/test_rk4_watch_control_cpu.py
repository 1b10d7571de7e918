"""csrc/marl_rk4_watch_ctl.h - the record, the step epilogue and the frame-list check of the monitored fixed-step RK4 loop - built alone
by a host C++ compiler and driven with made-up monitor sequences against the Python restatement (tests/rk4_watch_ref.py).  Every
comparison is exact: header and restatement form the same floating-point expressions (times by multiplication, the secant estimate
t_s + dt (go / (go - gn)), nothing contracted)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rk4_watch_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "integrating-diagenetic-equations-using-python_amd", "csrc")

SHIM = r"""
#include "marl_rk4_watch_ctl.h"
using namespace marl;
static_assert(sizeof(Rk4WatchRec) == 160, "the record crosses to the device as 20 doubles");
static_assert(RK4W_DONE == 0 && RK4W_TERMINAL == 1 && RK4W_NONFINITE == -2 && RK4W_FRAME == 1 && RK4W_STOP == 2, "the codes");
extern "C" {
int rec_sizeof() { return (int)sizeof(Rk4WatchRec); }
double monitor_shim(const double* rec, int e) { return rk4_watch_monitor(rec, e); }
double time_shim(double t0, double dt, long long s) { return rk4_watch_time(t0, dt, s); }
int begin_shim(Rk4WatchRec* r, const double* rec, const long long* fs, long long n) { return rk4_watch_begin(*r, rec, (const int64_t*)fs, n); }
int step_shim(Rk4WatchRec* r, const double* rec, const long long* fs, long long n, const long long* lim, double* tev, long long max_events)
{
    return rk4_watch_step(*r, rec, (const int64_t*)fs, n, (const int64_t*)lim, tev, max_events);
}
long long check_shim(const long long* fs, long long n, long long nsteps) { return rk4_watch_check_frames((const int64_t*)fs, n, nsteps); }
}
"""


class Rec(C.Structure):
    _fields_ = [("t0", C.c_double), ("dt", C.c_double), ("t", C.c_double), ("g", C.c_double * 7), ("n_events", C.c_int64 * 7),
                ("steps", C.c_int64), ("next_frame", C.c_int64), ("status", C.c_int32), ("pad", C.c_int32)]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("rk4watch")
    src, so = d / "rk4_watch_shim.cpp", d / "librk4_watch_shim.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.monitor_shim.restype = lib.time_shim.restype = C.c_double
    lib.monitor_shim.argtypes = [C.c_void_p, C.c_int]
    lib.time_shim.argtypes = [C.c_double, C.c_double, C.c_longlong]
    lib.begin_shim.argtypes = [C.POINTER(Rec), C.c_void_p, C.c_void_p, C.c_longlong]
    lib.step_shim.argtypes = [C.POINTER(Rec), C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_longlong]
    lib.check_shim.restype = C.c_longlong
    lib.check_shim.argtypes = [C.c_void_p, C.c_longlong, C.c_longlong]
    assert lib.rec_sizeof() == C.sizeof(Rec) == 160
    return lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def drive(shim, t0, dt, seq, frame_steps=(), lim=None, max_events=None, bad=None):
    """Run the header and the restatement over the monitor sequence `seq` (seq[0]: the initial state's monitors; bad[i]: slot 0 of
    record i), compare after every step, and return (restatement, decisions)."""
    bad = bad or [0.0] * len(seq)
    fs = np.asarray(frame_steps, dtype=np.int64)
    lm = None if lim is None else np.asarray(lim, dtype=np.int64)
    tev = None if max_events is None else np.full((7, max(max_events, 1)), np.nan)
    rec0 = ref.record_of_events(seq[0], bad[0])
    r = Rec(t0=t0, dt=dt)
    w = ref.Watch(t0, dt, rec0, frame_steps, lim, max_events)
    assert shim.begin_shim(C.byref(r), _ptr(rec0), _ptr(fs) if fs.size else None, fs.size) == w.begin
    decisions = []
    for i in range(1, len(seq)):
        rec = ref.record_of_events(seq[i], bad[i])
        got = shim.step_shim(C.byref(r), _ptr(rec), _ptr(fs) if fs.size else None, fs.size, _ptr(lm) if lm is not None else None,
                             _ptr(tev) if tev is not None else None, max_events or 0)
        want = w.step(rec)
        assert got == want, i
        assert (r.steps, r.next_frame, r.status, r.t) == (w.steps, w.next_frame, w.status, w.t), i
        assert list(r.n_events) == w.n_events and list(r.g) == [float(x) for x in w.g], i
        decisions.append(got)
        if got & ref.STOP:
            break
    if tev is not None:
        for e in range(7):
            k = len(w.t_events[e])
            assert k == min(w.n_events[e], max_events)
            assert list(tev[e, :k]) == w.t_events[e] and np.all(np.isnan(tev[e, k:])), e
    return w, decisions


def g7(**kw):
    """seven monitors, all at -1 (no sign change ever) but the named ones"""
    names = ("zeros", "zeros_CA", "zeros_CC", "ones_CA_plus_CC", "ones_Phi", "zeros_U", "zeros_W")
    return [kw.get(n, -1.0) for n in names]


def test_slot_map_and_times(shim):
    rec = np.arange(8, dtype=float) * 1.5 + 0.25
    for e in range(7):
        assert shim.monitor_shim(_ptr(rec), e) == ref.monitor(rec, e)
    assert [ref.SLOT[e] for e in range(7)] == [1, 2, 3, 5, 6, 4, 7]
    for t0, dt, s in ((0.0, 5e-6, 2704), (0.1, 1e-5 / 3, 12345), (-2.0, 0.3, 7)):
        assert shim.time_shim(t0, dt, s) == t0 + np.float64(s) * dt      # formed by multiplication, never accumulated


def test_both_directions_and_the_secant_time(shim):
    w, _ = drive(shim, 0.0, 5e-6, [g7(ones_Phi=-0.3), g7(ones_Phi=-0.1), g7(ones_Phi=0.2), g7(ones_Phi=0.4), g7(ones_Phi=-0.6)], max_events=8)
    assert w.n_events == [0, 0, 0, 0, 2, 0, 0]
    up, down = w.t_events[4]
    assert up == 1 * 5e-6 + 5e-6 * (-0.1 / (-0.1 - 0.2)) and down == np.float64(3) * 5e-6 + 5e-6 * (0.4 / (0.4 + 0.6))
    assert w.status == ref.DONE and w.steps == 4


def test_touching_zero_and_staying_there(shim):
    """go < 0 -> gn == 0 fires (at the step's end: go / (go - 0) = 1), 0 -> 0 fires with go == gn at t_(s+1), 0 -> > 0 fires at the step's start"""
    w, _ = drive(shim, 1.0, 0.25, [g7(zeros_W=-2.0), g7(zeros_W=0.0), g7(zeros_W=0.0), g7(zeros_W=3.0), g7(zeros_W=4.0)], max_events=8)
    assert w.n_events[6] == 3 and w.t_events[6] == [1.25, 1.5, 1.5]


def test_two_monitors_in_one_step(shim):
    w, _ = drive(shim, 0.0, 1e-3, [g7(zeros_U=1.0, zeros_W=-1.0), g7(zeros_U=-1.0, zeros_W=3.0), g7(zeros_U=-2.0, zeros_W=4.0)], max_events=2)
    assert w.n_events == [0, 0, 0, 0, 0, 1, 1] and w.t_events[5] == [0.5e-3] and w.t_events[6] == [0.25e-3]


def test_max_events_caps_the_stored_times_not_the_count(shim):
    seq = [g7(zeros_W=(-1.0) ** i) for i in range(9)]
    w, _ = drive(shim, 0.0, 1.0, seq, max_events=3)
    assert w.n_events[6] == 8 and w.t_events[6] == [0.5, 1.5, 2.5]
    w, _ = drive(shim, 0.0, 1.0, seq)                      # no buffer: counted only
    assert w.n_events[6] == 8 and w.t_events[6] == []


def test_terminal_limits(shim):
    seq = [g7(zeros_W=(-1.0) ** i, ones_Phi=-1.0 if i < 4 else 1.0) for i in range(9)]
    for k, steps in ((1, 1), (2, 2)):
        w, dec = drive(shim, 0.0, 1.0, seq, lim=[0, 0, 0, 0, 0, 0, k], max_events=8, frame_steps=(steps, 5))
        assert w.status == ref.TERMINAL and w.steps == steps and w.t == float(steps) and w.n_events[6] == k
        assert dec[-1] == ref.STOP | ref.FRAME and w.next_frame == 1           # the frame due at the terminal step is written
    # all sign changes of the terminal step are counted and stored: step 4 (3 -> 4) has zeros_W and ones_Phi
    w, _ = drive(shim, 0.0, 1.0, seq, lim=[0, 0, 0, 0, 1, 0, 0], max_events=8)
    assert w.status == ref.TERMINAL and w.steps == 4 and w.n_events == [0, 0, 0, 0, 1, 0, 4] and len(w.t_events[6]) == 4
    # a limit never met changes nothing
    free, dfree = drive(shim, 0.0, 1.0, seq, max_events=8, frame_steps=(0, 8))
    w, dec = drive(shim, 0.0, 1.0, seq, lim=[3, 0, 0, 0, 2, 0, 9], max_events=8, frame_steps=(0, 8))
    assert (w.status, w.steps, w.n_events, w.t_events, dec) == (ref.DONE, 8, free.n_events, free.t_events, dfree)


def test_non_finite_is_processed_before_events_and_frames(shim):
    seq = [g7(zeros_W=-1.0), g7(zeros_W=-0.5), g7(zeros_W=2.0), g7(zeros_W=3.0)]
    for flag in (1.0, 7.0, float("nan")):
        w, dec = drive(shim, 0.0, 1.0, seq, bad=[0.0, 0.0, flag, 0.0], lim=[0, 0, 0, 0, 0, 0, 1], max_events=4, frame_steps=(1, 2, 3))
        assert w.status == ref.NONFINITE and w.steps == 2 and w.t == 2.0 and dec == [ref.FRAME, ref.STOP]
        assert w.n_events == [0] * 7 and w.g[6] == -0.5 and w.next_frame == 1      # neither the sign change nor the frame of that step


def test_frames_at_step_zero_in_the_middle_and_at_the_end(shim):
    seq = [g7()] * 7
    w, dec = drive(shim, 0.0, 1.0, seq, frame_steps=(0, 3, 6))
    assert w.begin == ref.FRAME and dec == [0, 0, ref.FRAME, 0, 0, ref.FRAME] and w.next_frame == 3
    w, dec = drive(shim, 0.0, 1.0, seq, frame_steps=(2,))
    assert w.begin == 0 and dec == [0, ref.FRAME, 0, 0, 0, 0] and w.next_frame == 1
    w, dec = drive(shim, 0.0, 1.0, seq)
    assert w.begin == 0 and dec == [0] * 6 and w.next_frame == 0


def test_rejected_frame_lists(shim):
    def check(fs, nsteps):
        a = np.asarray(fs, dtype=np.int64)
        got = shim.check_shim(_ptr(a) if a.size else None, a.size, nsteps)
        assert got == ref.check_frames(list(fs), nsteps)
        return got
    assert check((), 10) == -1 and check((0, 1, 7, 10), 10) == -1 and check((10,), 10) == -1 and check((0,), 0) == -1
    assert check((0, 7, 3), 10) == 2           # descending
    assert check((0, 3, 3, 4), 10) == 2        # duplicate
    assert check((-1, 3), 10) == 0             # negative
    assert check((0, 3, 11), 10) == 2          # beyond nsteps
