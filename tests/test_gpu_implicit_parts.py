"""The implicit path's parts on the device, one call at a time (marl_debug_num_jac, marl_debug_block_solve: the functions radau_run /
bdf_run call), against the references of tests/implicit_ref.py (checked on the CPU in tests/test_implicit_reference_cpu.py).

The whole-integration tests (tests/test_gpu_radau.py, test_gpu_bdf.py) pin scipy's decision counts on three runs from the flat state and
the bit-identity of alternative launch paths; a wrong Jacobian entry or elimination step elsewhere costs Newton an iteration and passes.
Here:
  * the finite-difference Jacobian ALGORITHM: device J and step factors against scipy's num_jac driven by the device's own RHS (same RHS
    values, same algorithm: equal to the last bit), over three chained calls, on inputs that reach num_jac's adaptation branches;
  * the Jacobian VALUES: the same J against scipy's num_jac on the oracle RHS, per entry within K rounding errors of the rates;
  * the block SOLVES: every factorisation / solve path against a high-precision solution, in the solver's scaled norm E.
Measured figures are printed as JSON lines (pytest -rA) and recorded in IMPLICIT_JAC_K / IMPLICIT_SOLVE_E of tests/common.py.
"""
import json

import numpy as np
import pytest
from scipy.sparse import csc_matrix

import implicit_ref as R
from common import IMPLICIT_JAC_K, IMPLICIT_SOLVE_E

pytestmark = pytest.mark.gpu


def _model(scn, N):
    from marlpde_amd.LHeureux_model import LMAHeureuxPorosityDiff
    return LMAHeureuxPorosityDiff.from_scenario(R.params(scn, N), device=0)


# ---- Jacobian ----------------------------------------------------------------------------------------------------------------------
# (scenario, N, state, threshold, chained calls, groups): the grid N x state x grouping on Scenario A, the named inputs of
# implicit_ref.JAC_INPUTS (branch coverage asserted on the CPU), and FV_switch = 0 / dPhi_variable = 1 at one N each (their
# counterparts with FV_switch = 1 / dPhi_variable = 0 are in the grid)
_STATE_THRESHOLD = (("flat", 1e-3), ("depleted", 1e-3), ("zeros", 1e-30), ("tiny", 1e-30))
JAC_CASES = ([("A", N, st, thr, 3, g) for N in (5, 33, 67, 200) for st, thr in _STATE_THRESHOLD for g in ("scipy", None)]
             + [v + (g,) for v in R.JAC_INPUTS.values() for g in ("scipy", None)]
             + [("A_fv0", 67, "tiny", 1e-30, 3, "scipy"), ("A_fv0", 67, "depleted", 1e-3, 3, None), ("matlab_fv0", 33, "zeros", 1e-30, 3, "scipy"),
                ("A_dphi", 33, "tiny", 1e-30, 3, None)])
_JAC_IDS = ["%s-N%d-%s-thr%g-x%d-%s" % (c[:5] + ("scipy" if c[5] else "colouring",)) for c in JAC_CASES]
_jac_runs = {}


def _jac_run(oracle, case):
    """One case on the device and by scipy, once per session: per chained call the device's (J, factor), scipy's num_jac on the DEVICE RHS
    (J as blocks, factor), and the trace (steps h) of the same algorithm on the device RHS."""
    if case not in _jac_runs:
        scn, N, state, thr, calls, grouping = case
        y = R.STATES[state](R.params(scn, N), N)
        g = oracle.scipy_groups(N) if grouping == "scipy" else None
        gs = g if g is not None else R.structured_groups(N)
        eq = _model(scn, N)
        fun = R.columnwise(lambda v: eq.fun(0.0, v))
        dev, ref, steps = [], [], []
        fac_d = fac_s = None
        with np.errstate(all="ignore"):
            for _ in range(calls):
                J, fac_d = eq.debug_num_jac(y, thr, groups=g, factor=fac_d)
                dev.append((J, fac_d.copy()))
                steps.append(R.traced_num_jac(fun, y, thr, fac_s, N, gs)[2]["h"])
                Js, fac_s, _ = R.scipy_num_jac(fun, y, thr, fac_s, N, gs)
                ref.append((R.to_blocks(Js, N), fac_s.copy()))
        eq.close()
        _jac_runs[case] = (y, dev, ref, steps)
    return _jac_runs[case]


def _ulps(a, b):
    with np.errstate(all="ignore"):
        return np.where(a == b, 0.0, np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b))))


@pytest.mark.parametrize("case", JAC_CASES, ids=_JAC_IDS)
def test_num_jac_is_scipys_algorithm_on_the_device_rhs(oracle, case):
    """fd_prepare / fd_columns / fd_finish against scipy's num_jac fed the device's own RHS column by column: the same values through
    the same algorithm - J equal to the last bit, factors equal, on each of the chained calls (first = 1, then the factors carried over).
    Entries outside the pattern (CA / CC rows x Phi columns) and outside the grid are exactly 0."""
    N = case[1]
    _, dev, ref, _ = _jac_run(oracle, case)
    outside = ~R.blocks_mask(N)
    report = []
    for (Jd, fd), (Js, fs) in zip(dev, ref):
        u = _ulps(Jd, Js)
        report.append(dict(factor_mismatches=int(np.sum(fd != fs)), J_mismatches=int(np.sum(~(Jd == Js))), J_max_ulps=float(np.nanmax(u))))
    print("NUM_JAC_ALGORITHM", json.dumps({"case": _JAC_IDS[JAC_CASES.index(case)], "calls": report}))
    for (Jd, fd), (Js, fs) in zip(dev, ref):
        assert np.all(np.isfinite(Jd)) and np.all(Jd[outside] == 0)
        assert np.array_equal(fd, fs)
        assert np.array_equal(Jd, Js)


@pytest.mark.parametrize("case", JAC_CASES, ids=_JAC_IDS)
def test_jacobian_values_against_the_oracle(oracle, case):
    """The same device J against scipy's num_jac on the ORACLE RHS (each side chains its own factors).  Where both sides took the same
    step h_c for column c, entry (r, c) may differ by the rounding of the two rates it is the difference of:
        |J_dev - J_oracle| <= K eps max(|f0_r|, |f_r(y + h_c e_c)|) / |h_c|,
    K = IMPLICIT_JAC_K[state] (10 x the largest ratio measured on an MI355X over the cases of that state: the margin INCR_TOL uses for the
    case-to-case spread of last-bit RHS differences).  K is a row per state because the unit of the bound, eps |f_r|, is the rounding of
    the RESULT of a rate: on the flat state that is what the two implementations differ by (ratio 3); where a rate is the small
    remainder of large terms that cancel, the rounding of the terms is 1e4 .. 1e8 times that of the result.  The largest ratio, 2.8e8, is
    d rate(CC) / d CA inside the depleted region (CC = 1 - 1e-9, CA = 0, h = 1.5e-13): the oracle forms CC coA + (1 - CC) lambda coC as
    written (rate 2.2e-7, resolved to 1e-23), the kernel as DC + CC (DA - DC) (marl_math.h, point_local: terms of ~200, resolved to
    1e-14) - the device's difference is exactly 0 where the oracle's is 1.4e-14.  An absolute error of 1e-14 in a rate, harmless to an
    integration at any tolerance the drivers take, but the reason this row's K is what it is.  A column whose step differs took another branch of the adaptation on a knife edge (the device RHS differs from the
    oracle's in the last bits): it is compared in the algorithm test above, not here; such columns must stay the exception (<= 5 % of
    the columns of a call)."""
    scn, N, state, thr, calls, grouping = case
    y, dev, _, steps = _jac_run(oracle, case)
    fun = R.oracle_fun(oracle, scn, N)
    gs = oracle.scipy_groups(N) if grouping == "scipy" else R.structured_groups(N)
    S = R.structure(N).toarray() != 0
    fac, worst, other, at = None, 0.0, [], None
    with np.errstate(all="ignore"):
        for (Jd, _), h_dev in zip(dev, steps):
            Jt, fac, tr = R.traced_num_jac(fun, y, thr, fac, N, gs)
            same = tr["h"] == h_dev
            other.append(int(np.sum(~same)))
            unit = R.EPS * np.maximum(np.abs(tr["f0"])[:, None], np.abs(tr["fnew"])) / np.abs(tr["h"])[None, :]
            keep = S & same[None, :]
            Jo, Un, Kp = (R.to_blocks(csc_matrix(np.where(keep, a, 0.0)), N) for a in (Jt, unit, keep.astype(float)))
            diff = np.abs(Jd - Jo)[Kp > 0]
            un = Un[Kp > 0]
            ratio = np.where(diff == 0, 0.0, diff / np.where(un > 0, un, np.nan))
            ratio = np.where(np.isnan(ratio), np.inf, ratio)      # a difference where both rates are exactly 0
            if ratio.size and float(ratio.max()) > worst:
                worst = float(ratio.max())
                i, d, f, fp = (int(v[np.argmax(ratio)]) for v in np.nonzero(Kp > 0))
                at = dict(cell=i, slot=d, row_field=f, column_field=fp, J_device=float(Jd[i, d, f, fp]), J_oracle=float(Jo[i, d, f, fp]),
                          f0_row=float(tr["f0"][f * N + i]), h=float(tr["h"][fp * N + i + d - 1]))
    print("NUM_JAC_VALUES", json.dumps({"case": _JAC_IDS[JAC_CASES.index(case)], "max_ratio": worst, "at": at, "columns_with_another_step": other}))
    assert max(other) <= 0.05 * 5 * N, other
    assert worst <= IMPLICIT_JAC_K[state]["K"], (worst, IMPLICIT_JAC_K[state])


# ---- solves ------------------------------------------------------------------------------------------------------------------------
_DEFAULTS = dict(radau_cr=-1, radau_cr_small=3, radau_cr_small_min_n=205, radau_fused_solve=3, radau_cr_tail=1)


def _variants(N, want):
    """name -> options of the paths that solve a case; all variants of one case are documented as bit-identical (marl_radau.h:
    pcr_solve_all, crpcr_solve_all; marl_radau_cr.h: the tail kernels)"""
    if want == 0:      # parallel cyclic reduction alone: one launch per level / all levels in one launch
        base = _DEFAULTS | dict(radau_cr=0, radau_cr_small=0)
        return {"pcr_per_level": base | dict(radau_fused_solve=0), "pcr_fused": base | dict(radau_fused_solve=1)}
    if want < 0:       # large grids: automatic levels, launch path
        return {"cr_level_by_level": _DEFAULTS | dict(radau_cr_tail=0), "cr_tail": _DEFAULTS}
    out = {"crpcr_one_launch": _DEFAULTS | dict(radau_cr_small=want, radau_cr_small_min_n=32)}
    if N in (37, 409):  # the launch-path kernels on a small grid: levels forced, one-launch solves off
        base = _DEFAULTS | dict(radau_cr=want, radau_cr_small=0, radau_fused_solve=0)
        out |= {"cr_level_by_level": base | dict(radau_cr_tail=0), "cr_tail": base}
    return out


@pytest.mark.parametrize("N,want", R.SOLVE_CASES, ids=["N%d-levels%d" % c for c in R.SOLVE_CASES])
def test_block_solves_against_the_high_precision_solution(oracle, N, want):
    """marl_debug_block_solve (pcr_factor_launch + radau_solve) on every path of the case: J from scipy's num_jac on the oracle at four
    states; mu I - J for the Radau pair MU_REAL / h, MU_COMPLEX / h (h = 1e-6 .. 1) together, and BDF's I - c J (c = 1e-6, 0.02) alone;
    two right-hand sides per system solved with ONE factorisation.  Each solution's E against x_ref must stay within
    100 x the E of the numpy restatement with the same level count on the same system (FMA contraction, the summation order of the 25-lane
    block products), at least 1e-12; tests/test_implicit_reference_cpu.py shows that these bounds still catch each injected defect by a
    factor of 100.  The paths of one case are bit-identical to each other.

    Measured on an MI355X (IMPLICIT_SOLVE_E): the 22 cases stay at 0.011 .. 0.13 of their bounds (the largest: N = 409, PCR alone) and
    every pair of paths is bit-identical.  The restatement inverts its blocks as pcr_factor_group does (Gauss-Jordan with partial
    pivoting): the factor of 100 is for FMA contraction and summation order, not for another inversion algorithm - with LAPACK's inverse
    in its place the restatement makes E = 2.6e-11 where the device and the Gauss-Jordan restatement make 6.1e-9 and 7.4e-9 (N = 409, PCR
    alone, saturating state, h = 1, complex system), a bound the device's own algorithm cannot meet
    (tests/test_implicit_reference_cpu.py::test_restatement_inverts_as_the_device_does_and_what_another_inverse_costs)."""
    k = len(R.cr_sizes(N, want)) - 1
    rows = R.case_systems(oracle, N)
    eq = _model(R.SOLVE_SCENARIO[N], N)
    got = {}
    for name, opts in _variants(N, want).items():
        for o, v in opts.items():
            eq.set_option(o, v)
        for idx, (_, sd) in enumerate(rows):
            if sd["b_c"] is None:
                got[name, idx] = (eq.debug_block_solve(sd["J"], sd["b_r"], None, mu_r=sd["mu_r"], jscale=sd["jscale"]), None)
            else:
                got[name, idx] = eq.debug_block_solve(sd["J"], sd["b_r"], sd["b_c"], mu_r=sd["mu_r"], mu_c=sd["mu_c"], jscale=sd["jscale"])
    eq.close()
    names = list(_variants(N, want))
    worst_e, worst_q, misses, differ = 0.0, 0.0, [], []
    for idx, (st, sd) in enumerate(rows):
        er, ec = R.restated_errors(sd, k)
        for name in names:
            xr, xc = got[name, idx]
            for part, x, x_ref, e0 in (("real", xr, sd["x_r"], er), ("complex", xc, sd["x_c"], ec)):
                if x is None:
                    continue
                e, bound = R.worst_error(x, x_ref, sd["s"]), R.solve_bound(e0)
                worst_e, worst_q = max(worst_e, e if bound < 1 else 0.0), max(worst_q, e / bound)
                if not e <= bound:
                    misses.append((name, st, sd["tag"], part, e, bound))
            if name != names[0]:
                x0r, x0c = got[names[0], idx]
                if not (np.array_equal(xr, x0r) and (xc is None or np.array_equal(xc, x0c))):
                    differ.append((names[0], name, st, sd["tag"]))
    key = "N%d|levels%d" % (N, want)
    print("BLOCK_SOLVE", json.dumps({"case": key, "paths": names, "worst_E_where_bound_below_1": worst_e, "worst_E_over_bound": worst_q,
                                     "misses": misses, "not_bit_identical": differ}))
    assert not differ, differ[:6]
    assert not misses, misses[:6]
    assert key in IMPLICIT_SOLVE_E
