"""References of the implicit path's parts (test infrastructure; tests/test_implicit_reference_cpu.py checks them on the CPU before
tests/test_gpu_implicit_parts.py holds the device against them).

Layouts.  A state is field-major, y[f * N + i].  The device stores the Jacobian as blocks (N, 3, 5, 5): J[i, d, f, fp] =
d rate(f, i) / d y(fp, i + d - 1); the linear systems  mu I - jscale J  are cell-major (unknown 5 i + f), block-tridiagonal with 5 x 5
blocks.  Everything here is plain numpy / scipy in float64 (x_ref: residuals in np.longdouble).
"""
import functools

import numpy as np
from scipy.integrate._ivp import common as ivp_common
from scipy.integrate._ivp.radau import MU_COMPLEX, MU_REAL  # noqa: F401  (the tests' systems are MU / h I - J)
from scipy.sparse import coo_matrix, csc_matrix

from common import noisy_state, saturating_state, scenario, synthetic_state

EPS = ivp_common.EPS
RTOL = ATOL = 1e-3      # the tolerances of the reference's runs: the scale of the error measure


# ---- states ----------------------------------------------------------------------------------------------------------------------
def flat_state(p, N):
    return np.concatenate([np.full(N, p[k]) for k in ("CAIni", "CCIni", "cCaIni", "cCO3Ini", "PhiIni")])


def depleted_state(p, N):
    """saturating_state with the aragonite gone and the calcite a hair under one on the middle third: large differences, factors decrease"""
    y = saturating_state(p, N).reshape(5, N).copy()
    y[0, N // 3:2 * N // 3] = 0.0
    y[1, N // 3:2 * N // 3] = 1.0 - 1e-9
    return y.ravel()


def zeros_state(p, N):
    """saturating_state with exact zeros in the solids (with a tiny threshold: steps of 1e-38, differences that drown - factors increase)"""
    y = saturating_state(p, N).reshape(5, N).copy()
    y[0, ::4] = 0.0
    y[1, 1::4] = 0.0
    return y.ravel()


def tiny_state(p, N):
    y = saturating_state(p, N).reshape(5, N).copy()
    y[0, ::3] = 1e-200
    y[2, 1::5] = 1e-150
    return y.ravel()


STATES = {
    "flat": flat_state,
    "synthetic": lambda p, N: synthetic_state(p, N, amplitude=0.05),
    "saturating": saturating_state,
    "noisy": noisy_state,
    "depleted": depleted_state,
    "zeros": zeros_state,
    "tiny": tiny_state,
}

SCENARIO_ARGS = {   # name -> (scenario of tests/common.py, FV_switch, extra parameters)
    "A": ("A", 1, {}),
    "default": ("default", 1, {}),
    "matlab_fv0": ("matlab", 0, {}),
    "A_dphi": ("A", 1, {"dPhi_variable": 1}),
    "A_fv0": ("A", 0, {}),
}


def params(scn, N):
    name, fv, extra = SCENARIO_ARGS[scn]
    return scenario(name, N, fv, **extra)


# ---- the Jacobian: scipy's num_jac with the reference's pattern ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def structure(N):
    """The reference's jac_sparsity (marlpde/parameters.py:150-199) as csc: rows (f, i) x columns (f', i - 1 .. i + 1) minus the CA / CC
    rows x Phi columns."""
    n = 5 * N
    f, fp, i, d = np.meshgrid(np.arange(5), np.arange(5), np.arange(N), np.arange(-1, 2), indexing="ij")
    keep = (i + d >= 0) & (i + d < N) & ~((f < 2) & (fp == 4))
    r, c = (f * N + i)[keep], (fp * N + i + d)[keep]
    return csc_matrix((np.ones(r.size), (r, c)), shape=(n, n))


def structured_groups(N):
    """the library's own 15-colouring (groups = NULL)"""
    j = np.arange(5 * N)
    return (3 * (j // N) + (j % N) % 3).astype(np.int32)


def columnwise(rhs):
    """solve_ivp-style fun(t, Y) for a 2-D Y (num_jac passes one perturbed state per column) from a function of one state"""
    def fun(t, Y):
        Y = np.asarray(Y)
        if Y.ndim == 1:
            return rhs(Y)
        return np.stack([rhs(np.ascontiguousarray(Y[:, k])) for k in range(Y.shape[1])], axis=1)
    return fun


def scipy_num_jac(fun, y, threshold, factor, N, groups):
    """scipy's own num_jac; f0 = fun(y).  Returns (J as csc, adapted factor, f0)."""
    y = np.asarray(y, dtype=np.float64)
    f0 = fun(0.0, y)
    J, factor = ivp_common.num_jac(fun, 0.0, y, f0, threshold, factor, (structure(N), np.asarray(groups)))
    return csc_matrix(J), factor, f0


def to_blocks(J, N):
    """sparse (5N, 5N) field-major Jacobian -> the device layout (N, 3, 5, 5)"""
    J = coo_matrix(J)
    f, i, fp, ip = J.row // N, J.row % N, J.col // N, J.col % N
    d = ip - i + 1
    assert np.all((d >= 0) & (d <= 2)), "entries outside the three block diagonals"
    B = np.zeros((N, 3, 5, 5))
    np.add.at(B, (i, d, f, fp), J.data)
    return B


def blocks_mask(N):
    """True where an entry of the device layout is inside the pattern and the grid"""
    m = np.ones((N, 3, 5, 5), dtype=bool)
    m[:, :, :2, 4] = False
    m[0, 0] = False
    m[N - 1, 2] = False
    return m


def traced_num_jac(fun, y, threshold, factor, N, groups):
    """num_jac restated with dense arrays, returning which branch every column took.  The CPU tests require it to equal scipy's num_jac
    bit for bit, so the trace is scipy's.  Returns (J dense, factor, trace); trace: h0 (times the h == 0 loop multiplied the factor),
    small (step retried), adopted (retried step taken), inc / dec (factor x 10 / x 0.1), clamped (MIN_FACTOR), h (steps used), f0,
    fnew (n, n): column c = f at the perturbed state column c was differenced with."""
    y = np.asarray(y, dtype=np.float64)
    n = y.size
    S = structure(N).toarray() != 0
    groups = np.asarray(groups)
    f = fun(0.0, y)
    factor = np.full(n, EPS ** 0.5) if factor is None else np.array(factor, dtype=np.float64)
    y_scale = (2 * (f >= 0).astype(float) - 1) * np.maximum(threshold, np.abs(y))
    h = (y + factor * y_scale) - y
    h0 = np.zeros(n, dtype=int)
    for i in np.nonzero(h == 0)[0]:
        while h[i] == 0:
            factor[i] *= 10
            h[i] = (y[i] + factor[i] * y_scale[i]) - y[i]
            h0[i] += 1
    ng = int(groups.max()) + 1
    H = np.where(groups[None, :] == np.arange(ng)[:, None], h, 0.0).T
    fnew = fun(0.0, y[:, None] + H)[:, groups]
    diff = np.where(S, fnew - f[:, None], 0.0)
    r = np.arange(n)
    max_ind = np.argmax(np.abs(diff), axis=0)
    max_diff = np.abs(diff[max_ind, r])
    scale = np.maximum(np.abs(f[max_ind]), np.abs(fnew[max_ind, r]))
    small = max_diff < ivp_common.NUM_JAC_DIFF_REJECT * scale
    adopted = np.zeros(n, dtype=bool)
    if small.any():
        ind = np.nonzero(small)[0]
        new_factor = ivp_common.NUM_JAC_FACTOR_INCREASE * factor[ind]
        h_new = (y[ind] + new_factor * y_scale[ind]) - y[ind]
        h_all = np.zeros(n)
        h_all[ind] = h_new
        gu = np.unique(groups[ind])
        gmap = np.empty(ng, dtype=int)
        gmap[gu] = np.arange(gu.size)
        H2 = np.where(groups[None, :] == gu[:, None], h_all, 0.0).T
        fnew2 = fun(0.0, y[:, None] + H2)[:, gmap[groups[ind]]]
        diff_new = np.where(S[:, ind], fnew2 - f[:, None], 0.0)
        rr = np.arange(ind.size)
        mi = np.argmax(np.abs(diff_new), axis=0)
        md_new = np.abs(diff_new[mi, rr])
        sc_new = np.maximum(np.abs(f[mi]), np.abs(fnew2[mi, rr]))
        upd = max_diff[ind] * sc_new < md_new * scale[ind]
        ui = ind[upd]
        factor[ui] = new_factor[upd]
        h[ui] = h_new[upd]
        diff[:, ui] = diff_new[:, upd]
        fnew[:, ui] = fnew2[:, upd]
        scale[ui] = sc_new[upd]
        max_diff[ui] = md_new[upd]
        adopted[ui] = True
    J = diff / h
    inc = max_diff < ivp_common.NUM_JAC_DIFF_SMALL * scale
    dec = max_diff > ivp_common.NUM_JAC_DIFF_BIG * scale
    factor[inc] *= ivp_common.NUM_JAC_FACTOR_INCREASE
    factor[dec] *= ivp_common.NUM_JAC_FACTOR_DECREASE
    clamped = factor < ivp_common.NUM_JAC_MIN_FACTOR
    factor = np.maximum(factor, ivp_common.NUM_JAC_MIN_FACTOR)
    return J, factor, dict(h0=h0, small=small, adopted=adopted, inc=inc, dec=dec, clamped=clamped, h=h, f0=f, fnew=fnew)


# Inputs that drive num_jac through its branches: name -> (scenario, N, state, threshold, chained calls).  What each reaches is asserted in
# tests/test_implicit_reference_cpu.py (on the oracle RHS); tests/test_gpu_implicit_parts.py runs the device on the same list.
JAC_INPUTS = {
    "depleted":       ("A", 64, "depleted", 1e-3, 5),        # FACTOR_DECREASE on 24 columns per call; the fifth call meets MIN_FACTOR
    "depleted_dphi":  ("A_dphi", 33, "depleted", 1e-3, 3),   # the same with the variable porosity diffusion: 11 columns
    "zeros":          ("A", 64, "zeros", 1e-30, 3),          # differences that drown: retried, not adopted, FACTOR_INCREASE (32 columns)
    "tiny":           ("A", 64, "tiny", 1e-30, 3),           # 35 columns
    "tiny_atol":      ("A", 64, "tiny", 1e-3, 3),            # the integrators' threshold: one increase on the first call
    "zeros_retry":    ("A", 64, "zeros", 1e-9, 3),           # steps at the edge of resolution: the ten times larger step is adopted
    "zeros_denormal": ("A", 64, "zeros", 1e-320, 3),         # factor x threshold underflows: the h == 0 loop (five rounds on 32 columns)
}


def jac_input(name):
    scn, N, state, thr, calls = JAC_INPUTS[name]
    return scn, N, STATES[state](params(scn, N), N), thr, calls


def oracle_fun(orc, scn, N):
    P = orc.params_from_dict(params(scn, N))
    return columnwise(lambda y: orc.rhs(P, N, y))


_JAC_CACHE = {}


def oracle_jacobian(orc, scn, N, state):
    """(J blocks (N, 3, 5, 5), y) of scipy's num_jac on the oracle RHS at a named state, first call (factor None), threshold 1e-3.
    Computed once per (scenario, N, state) and shared; callers must not change it."""
    key = (scn, N, state)
    if key not in _JAC_CACHE:
        y = STATES[state](params(scn, N), N)
        J, _, _ = scipy_num_jac(oracle_fun(orc, scn, N), y, ATOL, None, N, structured_groups(N))
        B = to_blocks(J, N)
        B.setflags(write=False)
        y.setflags(write=False)
        _JAC_CACHE[key] = (B, y)
    return _JAC_CACHE[key]


# ---- the solves: block cyclic reduction + parallel cyclic reduction, restated ---------------------------------------------------------
DEFECTS = ("odd_last_unreduced", "swap_alpha_gamma", "guard_off_by_one", "jscale_diag_only")
PCR_FUSED_THREADS = 1024    # marl_radau.h
CR_WG_MAX_LEVELS = 3


def cr_sizes(N, want):
    """Row counts [n_0 = N, n_1, ..., n_k] of the cyclic-reduction levels radau_alloc plans: `want` > 0 levels (as many as leave two rows),
    want < 0: automatic - until the compact system fits one workgroup (5 n_k <= 1024); want == 0: none."""
    n = [N]
    while n[-1] // 2 >= 2 and (len(n) - 1 < want if want > 0 else (want < 0 and 5 * n[-1] > PCR_FUSED_THREADS)):
        n.append(n[-1] // 2)
    return n


def _where(mask, a):
    return np.where(mask[:, None, None], a, 0.0)


def crpcr_solve(J, mu, jscale, b, k, defect=None, inv=None):
    """x of (mu I - jscale J) x = b by k levels of block cyclic reduction and block PCR on the rows that are left - the recurrences of
    marl_radau_cr.h (cr_init / cr_reduce / cr_rhs / cr_back) and pcr_factor_group / pcr_solve_row, vectorised over rows with stacked
    5 x 5 matmul; float64, or complex128 with a complex mu.  J: (N, 3, 5, 5); b: (5N,) or (5N, nrhs) cell-major.  `defect`: one of DEFECTS -
    the restatement with that one mistake (tests/test_implicit_reference_cpu.py: the bounds must tell these from rounding).  `inv`: the
    stacked 5 x 5 inverse; None: gauss_jordan_inv below, pcr_factor_group's own algorithm (np.linalg.inv, LAPACK's LU, is another correct
    inverse: tests/test_implicit_reference_cpu.py records how far the two lie apart)."""
    assert defect is None or defect in DEFECTS
    inv = gauss_jordan_inv if inv is None else inv
    N = J.shape[0]
    dt = np.complex128 if np.iscomplexobj(mu) or np.iscomplexobj(b) else np.float64
    off = 1.0 if defect == "jscale_diag_only" else jscale
    D = (mu * np.eye(5) - jscale * J[:, 1]).astype(dt)
    L = (-(off * J[:, 0])).astype(dt)
    U = (-(off * J[:, 2])).astype(dt)
    L[0] = 0
    U[N - 1] = 0
    B = np.asarray(b, dtype=dt).reshape(N, 5, -1)
    first = True    # the swap defect hits one interior row of the first level of whatever kind
    levels = []
    for _ in range(k):
        n = D.shape[0]
        nn = n // 2
        p = 2 * np.arange(nn) + 1
        pp = np.minimum(p + 1, n - 1)
        Dinv = inv(D)
        hi = p + 1 < n
        if defect == "odd_last_unreduced" and n % 2 == 1:
            hi = p + 1 < n - 1
        al = -L[p] @ Dinv[p - 1]
        ga = _where(hi, -U[p] @ Dinv[pp])
        Dn = D[p] + al @ U[p - 1] + ga @ L[pp]
        Ln, Un = al @ L[p - 1], ga @ U[pp]
        alb, gab = al, ga
        if defect == "swap_alpha_gamma" and first:
            m = nn // 2
            alb, gab = al.copy(), ga.copy()
            alb[m], gab[m] = ga[m], al[m]
        Bn = B[p] + alb @ B[p - 1] + gab @ B[pp]
        e = 2 * np.arange((n + 1) // 2)
        levels.append((n, Dinv[e], -Dinv[e] @ L[e], -Dinv[e] @ U[e], B))
        L, D, U, B = Ln, Dn, Un, Bn
        first = False
    M = D.shape[0]
    i = np.arange(M)
    s = 1
    while s < M:
        Dinv = inv(D)
        lo = i - s >= 0
        hi = i + s < (M - 1 if defect == "guard_off_by_one" else M)
        im, ip = np.maximum(i - s, 0), np.minimum(i + s, M - 1)
        al = _where(lo, -L @ Dinv[im])
        ga = _where(hi, -U @ Dinv[ip])
        Dn = D + al @ U[im] + ga @ L[ip]
        Ln, Un = al @ L[im], ga @ U[ip]
        alb, gab = al, ga
        if defect == "swap_alpha_gamma" and first:
            m = M // 2
            alb, gab = al.copy(), ga.copy()
            alb[m], gab[m] = ga[m], al[m]
        B = B + alb @ B[im] + gab @ B[ip]
        L, D, U = Ln, Dn, Un
        first = False
        s *= 2
    X = inv(D) @ B
    for n, Dinv_e, P, Q, Bl in reversed(levels):
        nn = n // 2
        e = 2 * np.arange((n + 1) // 2)
        q = e // 2
        v = Dinv_e @ Bl[e] + _where(q >= 1, P @ X[np.maximum(q - 1, 0)]) + _where(q < nn, Q @ X[np.minimum(q, nn - 1)])
        Xl = np.empty((n,) + X.shape[1:], dtype=dt)
        Xl[1:2 * nn:2] = X
        Xl[e] = v
        X = Xl
    return X.reshape(np.shape(b))


def gauss_jordan_inv(D):
    """stacked inverse by Gauss-Jordan elimination with partial pivoting - gj_inverse_elem of marl_radau.h: pivot size |re| + |im|, first
    largest; the pivot row scaled by the reciprocal of the pivot (complex: conj / |.|^2), then taken out of every other row"""
    A = np.array(D)
    V = np.broadcast_to(np.eye(5, dtype=A.dtype), A.shape).copy()
    rows = np.arange(A.shape[0])
    for k in range(5):
        size = np.abs(A[:, k:, k].real) + np.abs(A[:, k:, k].imag)
        p = k + np.argmax(size, axis=1)
        for M in (A, V):
            M[rows, k], M[rows, p] = M[rows, p].copy(), M[rows, k].copy()
        pv = A[:, k, k]
        pv = np.conj(pv) * (1.0 / (pv.real * pv.real + pv.imag * pv.imag)) if np.iscomplexobj(A) else 1.0 / pv
        dk, vk = A[:, k] * pv[:, None], V[:, k] * pv[:, None]
        m = A[:, :, k].copy()
        m[:, k] = 0
        A -= m[:, :, None] * dk[:, None, :]
        V -= m[:, :, None] * vk[:, None, :]
        A[:, k], V[:, k] = dk, vk
    return V


def _matvec_ld(Jl, mu, jscale, x):
    """(mu I - jscale J) x in extended precision; Jl: (N, 3, 5, 5) np.longdouble, x: (N, 5, nrhs) (c)longdouble"""
    N = Jl.shape[0]
    y = mu * x - jscale * (Jl[:, 1] @ x)
    y[1:] -= jscale * (Jl[1:, 0] @ x[:-1])
    y[:-1] -= jscale * (Jl[:-1, 2] @ x[1:])
    assert y.shape[0] == N
    return y


def reference_solve(J, mu, jscale, b):
    """High-precision x_ref: LAPACK's banded LU (gbtrf / gbtrs - what scipy.linalg.solve_banded calls - factorised once) refined with
    residuals accumulated in np.longdouble until the correction stops shrinking.  Returns x_ref (float64 / complex128, the rounded refined solution), shape of b."""
    from scipy.linalg import get_lapack_funcs
    N = J.shape[0]
    n = 5 * N
    cx = np.iscomplexobj(mu) or np.iscomplexobj(b)
    dt, ldt = (np.complex128, np.clongdouble) if cx else (np.float64, np.longdouble)
    i, d, f, fp = np.meshgrid(np.arange(N), np.arange(3), np.arange(5), np.arange(5), indexing="ij")
    keep = (i + d - 1 >= 0) & (i + d - 1 < N)
    r, c = (5 * i + f)[keep], (5 * (i + d - 1) + fp)[keep]
    ab = np.zeros((28, n), dtype=dt)          # gbtrf's layout: kl = ku = 9, kl spare rows on top for the pivoting
    ab[18 + r - c, c] = -jscale * J[keep]
    ab[18, :] += mu
    gbtrf, gbtrs = get_lapack_funcs(("gbtrf", "gbtrs"), (ab,))
    lu, piv, info = gbtrf(ab, 9, 9)
    assert info == 0, "banded LU: singular matrix"
    Jl = J.astype(np.longdouble)
    bl = np.asarray(b).reshape(N, 5, -1).astype(ldt)
    mul = ldt(mu)
    jl = np.longdouble(jscale)
    x = np.zeros_like(bl)
    last = np.inf
    for _ in range(12):
        res = bl - _matvec_ld(Jl, mul, jl, x)
        dx = gbtrs(lu, 9, 9, res.reshape(n, -1).astype(dt), piv)[0].reshape(bl.shape)
        size = float(np.max(np.abs(dx)))
        if not size < last:    # the correction no longer shrinks: x is as good as this factorisation gets it
            break
        x = x + dx.astype(ldt)
        last = size
        if size == 0:
            break
    return x.astype(dt).reshape(np.shape(b))


def scale_cell_major(y, N):
    """s = atol + rtol |y| in the systems' cell-major order"""
    return (ATOL + RTOL * np.abs(np.asarray(y).reshape(5, N))).T.ravel()


def scaled_error(x, x_ref, s):
    """E(x) = rms((x - x_ref) / s) / rms(x_ref / s): the norm in which Newton's convergence tests see a solve error"""
    s = s.reshape((-1,) + (1,) * (np.ndim(x) - 1))
    return float(np.sqrt(np.mean(np.abs((x - x_ref) / s) ** 2)) / np.sqrt(np.mean(np.abs(x_ref / s) ** 2)))


H_LIST = (1e-6, 1e-3, 0.05, 1.0)       # Radau: mu = MU_REAL / h and MU_COMPLEX / h, jscale = 1
C_LIST = (1e-6, 0.02)                  # BDF: mu = 1, jscale = c


def right_hand_sides(f0, seed):
    """(2, 5N) cell-major: f0 (1 + 0.1 noise) - what a Newton iteration solves for - and a random one"""
    N = f0.size // 5
    rng = np.random.default_rng(seed)
    fc = f0.reshape(5, N).T.ravel()
    return np.stack([fc * (1 + 0.1 * rng.standard_normal(5 * N)), rng.standard_normal(5 * N)])


_SYS_CACHE = {}


def solve_systems(orc, scn, N, state):
    """The systems of the solve tests at one (scenario, N, state), with their references, computed once and shared (read-only):
    a list of dicts  kind ('radau' | 'bdf'), tag, J, s, mu_r, mu_c, jscale, b_r (2, 5N), b_c (2, 5N) or None, x_r, x_c (references)."""
    key = (scn, N, state)
    if key in _SYS_CACHE:
        return _SYS_CACHE[key]
    J, y = oracle_jacobian(orc, scn, N, state)
    f0 = oracle_fun(orc, scn, N)(0.0, np.asarray(y))
    s = scale_cell_major(y, N)
    b = right_hand_sides(f0, seed=N)
    bc = b + 1j * right_hand_sides(f0, seed=N + 1)
    out = []
    for h in H_LIST:
        mu_r, mu_c = MU_REAL / h, MU_COMPLEX / h
        out.append(dict(kind="radau", tag=f"h={h:g}", J=J, s=s, mu_r=mu_r, mu_c=mu_c, jscale=1.0, b_r=b, b_c=bc,
                        x_r=reference_solve(J, mu_r, 1.0, b.T).T, x_c=reference_solve(J, mu_c, 1.0, bc.T).T))
    for c in C_LIST:
        out.append(dict(kind="bdf", tag=f"c={c:g}", J=J, s=s, mu_r=1.0, mu_c=0j, jscale=c, b_r=b, b_c=None,
                        x_r=reference_solve(J, 1.0, c, b.T).T, x_c=None))
    _SYS_CACHE[key] = out
    return out


def worst_error(x, x_ref, s):
    """the larger E of the right-hand sides; x, x_ref: (nrhs, 5N).  Not finite (a solve that blew up) counts as inf."""
    with np.errstate(all="ignore"):
        e = max(scaled_error(a, b, s) for a, b in zip(x, x_ref))
    return e if np.isfinite(e) else np.inf


def restated_errors(sysd, k, defect=None, inv=None):
    """E of the numpy restatement with k reduction levels on one system: (E real, E complex or None)"""
    def run(mu, b, x_ref):
        try:
            with np.errstate(all="ignore"):
                x = crpcr_solve(sysd["J"], mu, sysd["jscale"], b.T, k, defect, inv).T
        except np.linalg.LinAlgError:     # (an injected defect may leave a singular block)
            assert defect is not None
            return np.inf
        return worst_error(x, x_ref, sysd["s"])
    er = run(sysd["mu_r"], sysd["b_r"], sysd["x_r"])
    ec = None if sysd["b_c"] is None else run(sysd["mu_c"], sysd["b_c"], sysd["x_c"])
    return er, ec


# the solve tests' grids: N -> scenario (the four of SCENARIO_ARGS the measure was tried on), and (N, levels) cases: levels 0 = PCR alone,
# 1 .. 3 = that many reduction levels in front, -1 = radau_alloc's automatic choice for large grids
SOLVE_SCENARIO = {5: "A", 33: "default", 37: "A", 64: "matlab_fv0", 200: "A", 409: "A_dphi", 2049: "A", 5003: "A"}
SOLVE_STATES = ("flat", "synthetic", "saturating", "noisy")
SOLVE_CASES = ([(N, 0) for N in (5, 33, 64, 200, 409)] + [(N, k) for N in (33, 37, 64, 200, 409) for k in (1, 2, 3)]
               + [(2049, -1), (5003, -1)])


def case_systems(orc, N):
    """[(state, system)] of one grid: every state x (four Radau step sizes, two BDF coefficients)"""
    return [(st, sd) for st in SOLVE_STATES for sd in solve_systems(orc, SOLVE_SCENARIO[N], N, st)]


SOLVE_FACTOR, SOLVE_FLOOR = 100.0, 1e-12   # bound of the device's E: SOLVE_FACTOR x the restatement's E on the same system, at least SOLVE_FLOOR


def solve_bound(e_restated):
    return max(SOLVE_FACTOR * e_restated, SOLVE_FLOOR)
