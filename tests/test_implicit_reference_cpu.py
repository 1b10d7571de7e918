"""The references of the implicit path's parts (tests/implicit_ref.py), checked on the CPU so that they are trusted before the device is
held against them in tests/test_gpu_implicit_parts.py:

  * x_ref (banded LU + refinement in extended precision) against an 80-digit block Thomas solve on the worst-behaved system of the list;
  * the numpy restatement of block cyclic reduction + parallel cyclic reduction: its error E in the solver's scaled norm, and - the point
    of this file - that E tells each of four injected defects from rounding at the bounds the device test uses;
  * the traced restatement of num_jac equals scipy's num_jac bit for bit, and the Jacobian inputs reach the branches they are there for.

Why E and nothing else: the matrices mu I - J of this model are badly row-scaled and, for step sizes from ~0.05 on, have solutions that
grow geometrically along the column (the porosity rows are not diagonally dominant: |x| up to 1e78 for right-hand sides of size 1).
Their 2-norm condition numbers are 1e10 .. 1e20 and the row-wise backward error of a CORRECT float64 block PCR reaches 2.5e-6 at N = 409 -
neither separates a right solve from a wrong one.  E(x) = rms((x - x_ref) / s) / rms(x_ref / s), s = atol + rtol |y| cell-major, is the
norm in which Newton's convergence tests see a solve error.
"""
import json

import numpy as np
import pytest

import implicit_ref as R


def _branches(orc, name):
    """per chained call: the trace of num_jac on the oracle RHS, and whether the traced restatement equalled scipy's num_jac"""
    scn, N, y, thr, calls = R.jac_input(name)
    fun, g = R.oracle_fun(orc, scn, N), orc.scipy_groups(N)
    fac, out = None, []
    with np.errstate(all="ignore"):
        for _ in range(calls):
            Js, fs, _ = R.scipy_num_jac(fun, y, thr, fac, N, g)
            Jt, ft, tr = R.traced_num_jac(fun, y, thr, fac, N, g)
            out.append((np.array_equal(Js.toarray(), Jt) and np.array_equal(fs, ft), tr))
            fac = fs
    return out


@pytest.fixture(scope="module")
def branches(oracle):
    return {name: _branches(oracle, name) for name in R.JAC_INPUTS}


def test_traced_num_jac_is_scipys_num_jac(branches):
    """The trace that the branch assertions below (and the device test's value bound) read is scipy's: J and factor equal to the last bit
    on every input and every chained call."""
    for name, calls in branches.items():
        assert all(same for same, _ in calls), name


def test_jacobian_inputs_reach_the_branches_of_num_jac(branches):
    """Which branches of scipy's num_jac (common.py:268-451) the inputs of the device test drive - on the flat and the smooth states of the
    pinned integrations no factor ever changes.  Counted per call over the 5 N columns:
      FACTOR_DECREASE (difference too big): the depleted state, 24 of 320 columns on every call (11 of 165 at N = 33 with dPhi_variable);
      MIN_FACTOR: the same columns on the fifth chained call (1.5e-8 -> ... -> 1.5e-13 -> clamped to 1000 eps);
      retry with a ten times larger step, NOT adopted, then FACTOR_INCREASE: exact zeros / 1e-200 entries with threshold 1e-30
        (steps of 1e-38: the differences are exactly 0 both times) - 32 and 35 columns on every call; with threshold 1e-3, 1 column once;
      retry ADOPTED (md sc_new < md_new sc): the zeros state with threshold 1e-9 - steps of 1e-17 .. 1e-15 next to the resolution of the
        rates; both outcomes occur in one call;
      h == 0: the zeros state with a subnormal threshold, 1e-320: factor x threshold underflows, five rounds of factor *= 10 on the 32 zero
        entries.  (With a normal threshold the loop cannot run: |y_scale| >= |y| and factor >= 1000 eps keep y + h apart from y.)"""
    count = lambda name, key: [int(np.sum(tr[key])) for _, tr in branches[name]]  # noqa: E731
    assert count("depleted", "dec") == [24] * 5 and count("depleted", "inc") == [0] * 5
    assert count("depleted", "clamped") == [0, 0, 0, 0, 24]
    assert count("depleted_dphi", "dec") == [11] * 3
    for name, cols in (("zeros", 32), ("tiny", 35)):
        assert count(name, "small") == [cols] * 3 and count(name, "adopted") == [0] * 3 and count(name, "inc") == [cols] * 3
        assert count(name, "dec") == [0] * 3
    assert count("tiny_atol", "inc") == [1, 0, 0] and count("tiny_atol", "small") == [0, 0, 0]
    small, adopted = count("zeros_retry", "small"), count("zeros_retry", "adopted")
    assert all(a > 0 for a in adopted) and any(a < s for a, s in zip(adopted, small)), (small, adopted)
    h0 = [tr["h0"] for _, tr in branches["zeros_denormal"]]
    assert int(np.sum(h0[0] > 0)) == 32 and int(h0[0].max()) == 5 and not h0[1].any() and not h0[2].any()
    print("NUM_JAC_BRANCHES", json.dumps({name: {k: count(name, k) for k in ("small", "adopted", "inc", "dec", "clamped")} for name in R.JAC_INPUTS}))


def test_block_layout_of_the_jacobian(oracle):
    """to_blocks: slot d of cell i holds d rate(f, i) / d y(fp, i + d - 1); nothing lies outside the pattern and the grid."""
    N = 7
    J, _, _ = R.scipy_num_jac(R.oracle_fun(oracle, "A", N), R.STATES["saturating"](R.params("A", N), N), R.ATOL, None, N, oracle.scipy_groups(N))
    B, Jd = R.to_blocks(J, N), J.toarray()
    for i in range(N):
        for d in range(3):
            for f in range(5):
                for fp in range(5):
                    inside = 0 <= i + d - 1 < N
                    assert B[i, d, f, fp] == (Jd[f * N + i, fp * N + i + d - 1] if inside else 0.0)
    assert np.all(B[~R.blocks_mask(N)] == 0) and np.count_nonzero(B) == np.count_nonzero(Jd) > 0


def _mp_block_thomas(J, mu, jscale, b, digits=80):
    """sequential block Thomas in `digits`-digit arithmetic (mpmath): shares nothing with the references but the matrix"""
    import mpmath as mp
    with mp.workdps(digits):
        N = J.shape[0]
        blk = lambda a: mp.matrix(a.tolist())  # noqa: E731
        D = [mp.mpf(mu) * mp.eye(5) - mp.mpf(jscale) * blk(J[i, 1]) for i in range(N)]
        L = [-mp.mpf(jscale) * blk(J[i, 0]) for i in range(N)]
        U = [-mp.mpf(jscale) * blk(J[i, 2]) for i in range(N)]
        B = [mp.matrix(b[5 * i:5 * i + 5].tolist()) for i in range(N)]
        for i in range(1, N):
            m = L[i] * mp.inverse(D[i - 1])
            D[i] = D[i] - m * U[i - 1]
            B[i] = B[i] - m * B[i - 1]
        X = [None] * N
        X[N - 1] = mp.lu_solve(D[N - 1], B[N - 1])
        for i in range(N - 2, -1, -1):
            X[i] = mp.lu_solve(D[i], B[i] - U[i] * X[i + 1])
        return np.array([[float(X[i][r]) for r in range(5)] for i in range(N)]).ravel()


def test_reference_solution_against_80_digit_block_thomas(oracle):
    """x_ref on the system where float64 solvers do worst (Scenario A, N = 200, flat state, h = 1: |x| ~ 1e71, plain PCR's E ~ 1e-8,
    LAPACK's dense LU 1.2e-9): E(x_ref) against 80-digit block Thomas must lie below SOLVE_FLOOR, the smallest bound x_ref is used with
    (measured 5.4e-14; on the BDF system c = 0.02 it is the rounding of the output alone)."""
    mpmath = pytest.importorskip("mpmath")
    assert mpmath
    sysd = {sd["tag"]: sd for sd in R.solve_systems(oracle, "A", 200, "flat")}
    for tag in ("h=1", "c=0.02"):
        sd = sysd[tag]
        e = R.scaled_error(sd["x_r"][1], _mp_block_thomas(sd["J"], sd["mu_r"], sd["jscale"], sd["b_r"][1]), sd["s"])
        print("X_REF", json.dumps({"system": f"A|N200|flat|{tag}", "E_vs_80_digits": e}))
        assert e < R.SOLVE_FLOOR


def _levels(N, want):
    return len(R.cr_sizes(N, want)) - 1


def test_level_plan_matches_the_cases():
    """cr_sizes restates radau_alloc's plan: the odd row counts the cases are there for"""
    assert R.cr_sizes(37, 3) == [37, 18, 9, 4] and R.cr_sizes(33, 3) == [33, 16, 8, 4] and R.cr_sizes(409, 3) == [409, 204, 102, 51]
    assert R.cr_sizes(2049, -1) == [2049, 1024, 512, 256, 128] and R.cr_sizes(5003, -1) == [5003, 2501, 1250, 625, 312, 156]
    assert R.cr_sizes(200, 0) == [200] and R.cr_sizes(5, 3) == [5, 2]


@pytest.fixture(scope="module")
def restated(oracle):
    """(N, want) -> [(state, system, E real, E complex or None)] of the restatement with the case's level count"""
    return {(N, want): [(st, sd) + R.restated_errors(sd, _levels(N, want)) for st, sd in R.case_systems(oracle, N)] for N, want in R.SOLVE_CASES}


def test_restatement_error_in_the_scaled_norm(restated):
    """The restatement's E over every system of the device test (four states, h = 1e-6 .. 1, BDF's c = 1e-6 and 0.02, real and complex,
    N = 5 .. 5003, 0 .. 5 reduction levels) - the numbers the device bounds are 100 times of.  Asserted: E is finite everywhere, and where
    mu I dominates the rows (h = 1e-6: mu = 3.6e6 against off-diagonal row sums of at most 1.5e6) the solve is good to rounding,
    E <= 100 eps.  Recorded (pytest -rA), not asserted, because it is what float64 cyclic reduction does on these matrices and nothing a
    bound could be derived for: the worst E per case.  It grows with the step size and the grid, since from h ~ 0.05 on the solutions grow
    geometrically along the column: <= 2e-12 up to N = 64, 3e-9 at N = 200, 1e-4 at N = 409 (PCR alone or with one or two levels),
    and at N = 2049 / 5003 the systems with h >= 0.05 or c = 0.02 are solved to NO digit by any float64 method (E = 0.1 .. 300) - there
    the device bound is vacuous and the cases rest on their h <= 1e-3 and c = 1e-6 systems."""
    worst = {}
    for case, rows in restated.items():
        es = [e for _, _, er, ec in rows for e in (er, ec) if e is not None]
        worst["N%d|levels%d" % case] = max(es)
        assert np.all(np.isfinite(es)), case
        dominant = [e for _, sd, er, ec in rows if sd["tag"] == "h=1e-06" for e in (er, ec)]
        assert len(dominant) == 8 and max(dominant) <= 100 * R.EPS, (case, max(dominant))
    print("RESTATED_E", json.dumps(worst))


def test_restatement_inverts_as_the_device_does_and_what_another_inverse_costs(oracle):
    """The restatement follows pcr_factor_group down to the inverse of a block: Gauss-Jordan elimination with partial pivoting
    (gj_inverse_elem, restated as implicit_ref.gauss_jordan_inv - an inverse to rounding, checked here against LAPACK's).  The factor
    of 100 in the device bounds is there for FMA contraction and the summation order of the block products, NOT for another inversion
    algorithm: the same restatement with LAPACK's LU inverse (np.linalg.inv), measured against the bounds the device test uses, is
    printed per case.  Up to N = 200 it stays below 0.1 of the bound; at N = 409 with PCR alone the two correct inverses lie a factor of
    ~300 apart on one system (saturating state, h = 1, complex: E 7.4e-9 with Gauss-Jordan, 2.6e-11 with LAPACK) - a restatement with
    another inverse than the device's would set a bound there that the device's own algorithm cannot meet.  Recorded, not asserted."""
    rng = np.random.default_rng(0)
    D = rng.standard_normal((50, 5, 5)) + 1j * rng.standard_normal((50, 5, 5))
    for A in (D, D.real):
        inv = R.gauss_jordan_inv(A)
        assert inv.dtype == A.dtype and np.max(np.abs(inv @ A - np.eye(5))) < 1e-11 and np.max(np.abs(inv - np.linalg.inv(A))) < 1e-10
    spread = {}
    for N, k in ((64, 0), (200, 0), (200, 3), (409, 3), (409, 0)):
        over, apart = 0.0, 1.0
        for _, sd in R.case_systems(oracle, N):
            base, other = R.restated_errors(sd, k), R.restated_errors(sd, k, inv=np.linalg.inv)
            for b, o in zip(base, other):
                if b is not None:
                    over, apart = max(over, o / R.solve_bound(b)), max(apart, o / b, b / o)
        spread[f"N{N}|levels{k}"] = dict(lapack_E_over_bound=over, largest_factor_between_the_two=apart)
    print("LAPACK_INVERSE_RESTATEMENT", json.dumps(spread))


def test_bounds_separate_injected_defects_from_rounding(restated):
    """THE POINT OF THIS FILE.  The restatement with one defect at a time -
        odd_last_unreduced: the unpaired last row of a level with an odd row count is not folded into its neighbour;
        swap_alpha_gamma:   alpha and gamma exchanged in the right-hand side update of ONE interior row of the first level;
        guard_off_by_one:   PCR's `i + s < N` taken as `i + s < N - 1`;
        jscale_diag_only:   BDF's c applied to the diagonal block only
    - must miss the device test's bound by a factor of 100 or more: E(defect) >= 100 x bound = 100 x max(100 E(restatement), 1e-12) on
    the same system.  A device case asserts every one of its systems, so a defect is caught by a case when ONE of its systems shows it;
    that is what is required here, per case and defect - not every system can show every defect (at h = 1e-6 the coupling between rows
    eight cells apart is 1e-16 of the solution: there a dropped neighbour of the compact system changes no bit)."""
    report = {}
    for (N, want), rows in restated.items():
        k = _levels(N, want)
        sizes = R.cr_sizes(N, want)
        for defect in R.DEFECTS:
            if defect == "odd_last_unreduced" and not any(n % 2 for n in sizes[:-1]):
                continue          # no level with an odd row count in this case
            best = 0.0
            for _, sd, er, ec in rows:
                if defect == "jscale_diag_only" and sd["jscale"] == 1.0:
                    continue
                dr, dc = R.restated_errors(sd, k, defect)
                best = max(best, dr / R.solve_bound(er), 0.0 if dc is None else dc / R.solve_bound(ec))
            report[f"N{N}|levels{want}|{defect}"] = best
            assert best >= 100, (N, want, defect, best)
    assert any(key.endswith("odd_last_unreduced") for key in report)
    print("DEFECT_OVER_BOUND", json.dumps({k: (v if np.isfinite(v) else "inf") for k, v in report.items()}))
