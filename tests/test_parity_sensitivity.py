"""Can the GPU parity bounds catch a wrong kernel?  (CPU only: the oracle stands in for a kernel with a known error.)

At the fixed-step configurations of tests/test_gpu_parity.py with N >= 65 536 (common.RK4_FINE_CONFIGS), the oracle with ONE model constant
scaled by (1 + delta) is compared with the unperturbed oracle, through the GPU tests' own increment bound (common.INCR_TOL).  The increment
check must flag every perturbed run and pass the unperturbed one.  Each delta sits well below what the state measure alone
(rel_to_max <= RUN_TOL) notices: the error of a run is linear in delta, so the smallest delta each measure catches follows from one run, and
their ratio - the gain of the increment measure - is asserted (>= 100 at N = 2^20) and printed (pytest -rA).
"""
import numpy as np
import pytest

from common import INCR_TOL, RK4_FINE_CONFIGS, increment_ok, rel_to_max, saturating_state, scenario, synthetic_state

RUN_TOL = 1e-10          # tests/test_gpu_parity.py
MIN_GAIN = {"rk4_full_size": 100.0, "rk4_config2": 1.0}

# one constant of each part of the model: reaction rate, dissolution exponent, porosity diffusion (two), a solute's diffusivity
DELTAS = {
    "rk4_full_size": {"k2": 2e-5, "m2": 5e-5, "b": 1e-4, "beta": 1e-4, "DCa": 2e-6},
    "rk4_config2": {"k2": 1e-7, "m2": 2e-7, "b": 1e-6, "beta": 1e-6, "DCa": 1e-8},
}


@pytest.fixture(scope="module")
def runs(oracle):
    cache = {}

    def run(key, name=None, delta=0.0):
        if (key, name) not in cache:
            cfg = RK4_FINE_CONFIGS[key]
            p = scenario(cfg["scenario"], cfg["N"])
            P = oracle.params_from_dict(p)
            if name is not None:
                setattr(P, name, getattr(P, name) * (1.0 + delta))
            y0 = synthetic_state(p, cfg["N"], amplitude=cfg["amplitude"])
            dt = cfg["dtf"] * (P.length / cfg["N"]) ** 2
            cache[(key, name)] = (y0, oracle.rk4(P, cfg["N"], y0, dt, cfg["nsteps"], omp=True))
        return cache[(key, name)]
    return run


@pytest.mark.parametrize("key", list(RK4_FINE_CONFIGS))
def test_increment_bound_passes_the_unperturbed_oracle(runs, key):
    y0, ref = runs(key)
    ok, ratio, msg = increment_ok(ref.copy(), ref, y0, key, RK4_FINE_CONFIGS[key]["nsteps"])
    assert ok and np.all(ratio == 0), msg
    assert np.all(np.max(np.abs((ref - y0).reshape(5, -1)), axis=1) > 0)


@pytest.mark.parametrize("name", ["k2", "m2", "b", "beta", "DCa"])
@pytest.mark.parametrize("key", list(RK4_FINE_CONFIGS))
def test_increment_bound_flags_a_perturbed_constant(runs, key, name):
    cfg, tol = RK4_FINE_CONFIGS[key], INCR_TOL[key]
    delta = DELTAS[key][name]
    y0, ref = runs(key)
    _, got = runs(key, name, delta)
    ok, ratio, msg = increment_ok(got, ref, y0, key, cfg["nsteps"])
    state_err = rel_to_max(got, ref)
    # smallest delta each measure would notice (the error is linear in delta at these sizes)
    err = np.max(np.abs((got - ref).reshape(5, -1)), axis=1)
    inc = np.max(np.abs((ref - y0).reshape(5, -1)), axis=1)
    floor = tol["ulps"] * cfg["nsteps"] * np.finfo(np.float64).eps * np.max(np.abs(y0.reshape(5, -1)), axis=1)
    delta_incr = delta * np.min((np.asarray(tol["rel"]) * inc + floor) / err)
    delta_state = delta * RUN_TOL / state_err
    print(f"SENSITIVITY {key} N={cfg['N']} {name}: delta {delta:.0e}; smallest delta caught: state measure {delta_state:.1e}, "
          f"increment measure {delta_incr:.1e} (gain {delta_state / delta_incr:.0f}x); {msg}")
    assert state_err <= RUN_TOL, "delta too large to show the gap: the state measure alone already notices it"
    assert not ok, msg
    assert delta_state / delta >= MIN_GAIN[key], (delta_state, delta)


def test_saturating_state_reaches_the_branches(oracle):
    """The state tests/test_gpu_increment.py feeds in: equal to the Dirichlet values at x = 0, O2 crosses 1 many times, O3 > 1 somewhere."""
    for N in (1024, 5003, 65536, 1 << 20):
        p = scenario("default", N)
        KRat = oracle.derive(oracle.params_from_dict(p), N)["KRat"]
        y = saturating_state(p, N).reshape(5, N)
        O2 = y[2] * y[3]
        assert np.all(np.abs(y[:, 0] - np.array([p["CA0"], p["CC0"], p["cCa0"], p["cCO30"], p["Phi0"]])) <= 0.01 * np.abs(y[:, 0]))
        assert 0.3 < np.mean(O2 > 1) < 0.7 and np.mean(KRat * O2 > 1) > 0.03
        assert np.count_nonzero(np.diff(np.sign(O2 - 1))) >= 10
