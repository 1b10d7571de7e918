"""Terminal monitors in the explicit loops on the CPU: csrc/marl_rk_terminal.h - what one accepted step of an RK45 / RK23 run does with
the rule of marl_terminal.h (which sign changes happened, how the counts move, where a kept root is stored) - built alone by a host C++
compiler and held to a Python restatement of scipy's handle_events (ivp.py:79-130) plus the count / slot rule; and run_sweep_rk45 /
run_sweep_rk23(..., terminal=), which hand the spec to the engine only when it is given."""
import ctypes as C
import itertools
import os
import subprocess
from dataclasses import asdict

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "integrating-diagenetic-equations-using-python_amd", "csrc")

SHIM = r"""
#include "marl_rk_terminal.h"
extern "C" int any_met_shim(unsigned active, const long long* n_events, const long long* terminal)
{
    int64_t c[7], l[7];
    for (int e = 0; e < 7; e++) { c[e] = n_events[e]; l[e] = terminal[e]; }
    return marl::rk_terminal_any_met(active, c, l) ? 1 : 0;
}
extern "C" int step_shim(unsigned active, const double* roots, const long long* n_events, const long long* terminal, long long max_events,
                         unsigned* keep, double* t_stop, long long* n_out, long long* slot)
{
    int64_t c[7], l[7], o[7], s[7];
    for (int e = 0; e < 7; e++) { c[e] = n_events[e]; l[e] = terminal[e]; }
    uint32_t k = 0;
    const int rc = marl::rk_terminal_step(active, roots, c, l, max_events, &k, t_stop, o, s);
    for (int e = 0; e < 7; e++) { n_out[e] = o[e]; slot[e] = s[e]; }
    *keep = k;
    return rc;
}
extern "C" int step_in_place_shim(unsigned active, const double* roots, long long* n_events, const long long* terminal, long long max_events)
{
    int64_t c[7], l[7], s[7];
    for (int e = 0; e < 7; e++) { c[e] = n_events[e]; l[e] = terminal[e]; }
    uint32_t k = 0;
    double t = 0.0;
    const int rc = marl::rk_terminal_step(active, roots, c, l, max_events, &k, &t, c, s);   // the counts updated in place, as the callers do
    for (int e = 0; e < 7; e++) n_events[e] = c[e];
    return rc;
}
"""
LL7 = C.c_longlong * 7
UNTOUCHED = -1.0


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("rk_terminal")
    src, so = d / "rk_terminal_shim.cpp", d / "librk_terminal_shim.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.any_met_shim.restype = lib.step_shim.restype = lib.step_in_place_shim.restype = C.c_int
    return lib


def _ours(shim, mask, roots, n_events, limits, max_events):
    r = (C.c_double * 7)(*[roots[e] if (mask >> e) & 1 else float("nan") for e in range(7)])   # entries of inactive monitors must not be read
    keep, t_stop, n_out, slot = C.c_uint(0), C.c_double(UNTOUCHED), LL7(), LL7()
    rc = shim.step_shim(C.c_uint(mask), r, LL7(*n_events), LL7(*limits), C.c_longlong(max_events), C.byref(keep), C.byref(t_stop), n_out, slot)
    met = shim.any_met_shim(C.c_uint(mask), LL7(*n_events), LL7(*limits))
    in_place = LL7(*n_events)
    assert shim.step_in_place_shim(C.c_uint(mask), r, in_place, LL7(*limits), C.c_longlong(max_events)) == rc and list(in_place) == list(n_out)
    return rc, keep.value, t_stop.value, list(n_out), list(slot), met


def _restated(mask, roots, n_events, limits, max_events):
    """scipy's handle_events (ivp.py:79-130) for a forward step - the active monitors by root time, equal roots in monitor order, cut
    after the first whose count (this occurrence included, ivp.py:680) has reached its limit - then the counts and the slots."""
    active = [e for e in range(7) if (mask >> e) & 1]
    count = {e: n_events[e] + 1 for e in active}
    met = any(limits[e] > 0 and count[e] >= limits[e] for e in active)
    kept, t_stop = active, UNTOUCHED
    if met:
        order = sorted(active, key=lambda e: roots[e])         # (sorted is stable: equal roots keep the monitors' order)
        cut = next(i for i, e in enumerate(order) if limits[e] > 0 and count[e] >= limits[e])
        kept, t_stop = order[:cut + 1], roots[order[cut]]
    n_out = [n_events[e] + (1 if e in kept else 0) for e in range(7)]
    slot = [n_events[e] if (e in kept and n_events[e] < max_events) else -1 for e in range(7)]
    return int(met), sum(1 << e for e in kept), t_stop, n_out, slot, int(met)


def test_every_mask_against_the_restated_rule(shim):
    rng = np.random.default_rng(20261020)
    pool = [0.0125, 0.013, 0.013, 0.0135, 0.0142, 0.0149]      # few values: tied roots are common, and monitor order decides them
    limit_sets = [[0] * 7, [1] * 7, [3] * 7, [0, 1, 0, 3, 1, 0, 2], [2, 0, 5, 0, 0, 1, 3]]
    n_stop = n_tie = n_dropped = n_noslot = 0
    for mask in range(128):
        for limits, max_events in itertools.product(limit_sets, (0, 1, 4)):
            for _ in range(3):
                roots = [float(rng.choice(pool)) for _ in range(7)]
                # counts before the step: just below the limit (this occurrence meets it), at it, above it, and far below
                n_events = [max(0, limits[e] - 1 + int(rng.integers(-2, 3))) if limits[e] else int(rng.integers(0, 6)) for e in range(7)]
                got, want = _ours(shim, mask, roots, n_events, limits, max_events), _restated(mask, roots, n_events, limits, max_events)
                assert got == want, (mask, limits, max_events, roots, n_events, got, want)
                if want[0]:
                    kept = [e for e in range(7) if (want[1] >> e) & 1]
                    n_stop += 1
                    n_tie += sum(roots[e] == want[2] for e in range(7) if (mask >> e) & 1) > 1
                    n_dropped += want[1] != mask
                    n_noslot += any(want[4][e] < 0 for e in kept)
    print(f"{n_stop} cases stop: {n_tie} with another root equal to t_stop, {n_dropped} drop a sign change, {n_noslot} keep a root without a slot")
    assert n_stop >= 500 and n_tie >= 50 and n_dropped >= 100 and n_noslot >= 100


def test_named_cases(shim):
    r = [0.013514078, 0.013514078, 0.0, 0.0, 0.0, 0.0, 0.0142]
    mask = 0b1000011                                             # zeros and zeros_CA with the same root, zeros_W later in the step
    # zeros_CA's second occurrence ends the run: `zeros` (equal root, lower index) is kept in front of it, zeros_W never happened
    assert _ours(shim, mask, r, [1, 1, 0, 0, 0, 0, 5], [0, 2, 0, 0, 0, 0, 0], 4) == (1, 0b11, r[1], [2, 2, 0, 0, 0, 0, 5], [1, 1, -1, -1, -1, -1, -1], 1)
    # `zeros` ends it in front of zeros_CA
    assert _ours(shim, mask, r, [1, 1, 0, 0, 0, 0, 5], [2, 0, 0, 0, 0, 0, 0], 4) == (1, 0b1, r[0], [2, 1, 0, 0, 0, 0, 5], [1, -1, -1, -1, -1, -1, -1], 1)
    # the limit is one occurrence away: nothing stops, every sign change is kept, zeros_W has no slot left
    assert _ours(shim, mask, r, [1, 1, 0, 0, 0, 0, 5], [0, 0, 0, 0, 0, 0, 7], 4) == (0, mask, UNTOUCHED, [2, 2, 0, 0, 0, 0, 6], [1, 1, -1, -1, -1, -1, -1], 0)
    # a limit passed long ago still stops (count >= limit); no buffer at all: counted, not stored
    assert _ours(shim, mask, r, [1, 1, 0, 0, 0, 0, 5], [0, 0, 0, 0, 0, 0, 2], 0) == (1, mask, r[6], [2, 2, 0, 0, 0, 0, 6], [-1] * 7, 1)
    # limits of monitors that did not change sign do not matter
    assert _ours(shim, mask, r, [0] * 7, [0, 0, 1, 1, 1, 1, 0], 4)[0] == 0


# ---- run_sweep_rk45 / run_sweep_rk23(..., terminal=) ------------------------------------------------------------------------------
class RecordingEngine:
    """Stands in for HipSweepEngine: returns the initial states and records the keywords of every call."""
    calls = []

    def __init__(self, base_parms, instances):
        self.n = len(instances)

    def _run(self, name, y0, t_span, first_step, rtol, atol, max_attempts, **kw):
        from marlpde_amd._abi import MarlStats
        from marlpde_amd.LHeureux_model import RK45Result
        type(self).calls.append((name, dict(kw)))
        res = []
        for b in range(self.n):
            st = MarlStats()
            st.status, st.t = (1, 0.5 * t_span[1]) if kw.get("terminal") and b == self.n - 1 else (0, t_span[1])
            res.append(RK45Result(st))
        return np.array(y0), res

    def integrate_rk45(self, *a, **kw):
        return self._run("rk45", *a, **kw)

    def integrate_rk23(self, *a, **kw):
        return self._run("rk23", *a, **kw)

    def close(self):
        pass


@pytest.mark.parametrize("method", ("rk45", "rk23"))
def test_run_sweep_hands_the_spec_to_the_engine_only_when_given(method):
    from marlpde_amd import sweep
    from marlpde_amd.parameters import Map_Scenario
    run = getattr(sweep, "run_sweep_" + method)
    base = asdict(Map_Scenario()) | {"N": 16}
    instances = [{"Phi0": 0.6, "PhiIni": 0.5}, {"Phi0": 0.8, "PhiIni": 0.8}, {}]
    RecordingEngine.calls = []
    y, status, acc, rej, t = run(base, instances, (0.0, 0.02), 1e-6, 1e-3, 1e-3, engine_factory=RecordingEngine, terminal={"ones_Phi": True})
    assert RecordingEngine.calls == [(method, {"terminal": {"ones_Phi": True}})]
    assert list(status) == [0, 0, 1] and list(t) == [0.02, 0.02, 0.01]
    run(base, instances, (0.0, 0.02), 1e-6, 1e-3, 1e-3, engine_factory=RecordingEngine)
    run(base, instances, (0.0, 0.02), 1e-6, 1e-3, 1e-3, engine_factory=RecordingEngine, events=True, max_events=8, terminal=[0, 0, 0, 0, 0, 0, 2])
    assert RecordingEngine.calls[1:] == [(method, {}), (method, {"events": True, "max_events": 8, "terminal": [0, 0, 0, 0, 0, 0, 2]})]


def test_the_abi_carries_the_four_entries():
    from marlpde_amd import _abi
    lib = _abi.load()
    for name in ("marl_sweep_rk45_terminal_dev", "marl_sweep_rk23_terminal_dev", "marl_integrate_rk45_terminal", "marl_integrate_rk23_terminal"):
        entry = getattr(lib, name)
        assert entry(*[a() for a in entry.argtypes]) == -1, name      # zeros and null pointers, no context: -1, nothing touched
