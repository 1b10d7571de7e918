"""References of the BDF sweep's five vector kernels (csrc/marl_bdf_batch.h: init_D / change_D / accept_norms / sample / roots_batch_kernel),
the bounds a device result is held to, and the inputs of the tests (test infrastructure: tests/test_bdf_batch_reference_cpu.py checks all
of this on the CPU before tests/test_gpu_bdf_batch_parts.py holds the device against it).

Everything is plain numpy.  Sums whose rounding a bound speaks about are formed in extended precision - np.longdouble where it has at
least 64 significant bits (x86), otherwise mpmath at 80 bits - and rounded to float64 once.  The float64 restatements (`*_f64`) spell
the kernels' own loops; they take a `defect` so that the CPU test can show that the bounds flag each of them.

Layouts: a state is field-major, y[f * N + i], n = 5 N.  D: (8, n), the rows of scipy's BDF.D (MAX_ORDER + 3 = 8).
"""
import math

import numpy as np

from common import scenario, synthetic_state

EPS = float(np.finfo(np.float64).eps)
MAX_ORDER = 5
ROWS = MAX_ORDER + 3

if np.finfo(np.longdouble).nmant >= 63:
    def ext(a):
        return np.asarray(a, dtype=np.longdouble)
else:   # (np.longdouble is float64 here)
    import mpmath
    mpmath.mp.prec = 80

    def ext(a):
        return np.vectorize(mpmath.mpf, otypes=[object])(np.asarray(a, dtype=np.float64))


def f64(a):
    return np.asarray(a).astype(np.float64)


# ---- scipy's constants (bdf.py:189-193) ------------------------------------------------------------------------------------------
KAPPA = np.array([0, -0.1850, -1 / 9, -0.0823, -0.0415, 0])
GAMMA = np.hstack((0, np.cumsum(1 / np.arange(1, MAX_ORDER + 1))))
ERROR_CONST = KAPPA * GAMMA + 1 / np.arange(1, MAX_ORDER + 2)
FACTORS = (0.2, 0.9, 10.0)   # MIN_FACTOR, a typical one, MAX_FACTOR


def scipy_RU(order, factor):
    """R U of change_D (bdf.py:28-33), padded to the controller's 6 x 6."""
    from scipy.integrate._ivp.bdf import compute_R
    RU = np.zeros((MAX_ORDER + 1, MAX_ORDER + 1))
    RU[:order + 1, :order + 1] = compute_R(order, factor).dot(compute_R(order, 1))
    return RU


# ---- INIT_D ----------------------------------------------------------------------------------------------------------------------
def init_D_ref(y, f, h):
    """rows 0 and 1: D[0] = y, D[1] = f h (float64: one multiplication, equal to the last bit)"""
    return np.stack([np.asarray(y, dtype=np.float64), np.asarray(f, dtype=np.float64) * h])


# ---- CHANGE_D --------------------------------------------------------------------------------------------------------------------
def change_D_ref(D, order, RU):
    """(rows 0 .. order of RU^T D[:order + 1], their bounds): row k = sum_j RU[j][k] D[j] in extended precision; bound
    (order + 2) eps sum_j |RU[j][k]| |D[j]| - a chain of order + 1 products and sums, with or without fused multiply-add."""
    Dx, R = ext(D[:order + 1]), ext(RU[:order + 1, :order + 1])
    out = [sum(R[j, k] * Dx[j] for j in range(order + 1)) for k in range(order + 1)]
    A = np.abs(RU[:order + 1, :order + 1]).T @ np.abs(D[:order + 1])
    return f64(np.stack(out)), (order + 2) * EPS * A


def change_D_f64(D, order, RU, defect=None):
    """the kernel's loop in float64.  defect "transposed": RU[k][j] for RU[j][k]"""
    out = np.empty((order + 1, D.shape[1]))
    for k in range(order + 1):
        a = np.zeros(D.shape[1])
        for j in range(order + 1):
            a = a + (RU[k][j] if defect == "transposed" else RU[j][k]) * D[j]
        out[k] = a
    return out


# ---- ACCEPT_NORMS ----------------------------------------------------------------------------------------------------------------
def accept_ref(D, d, order):
    """scipy's statements bdf.py:414-418 in float64, in their order (additions only: equal to the last bit).  Returns all rows; rows above
    order + 2 are the input's."""
    D = np.array(D, dtype=np.float64)
    D[order + 2] = d - D[order + 1]
    D[order + 1] = d
    for i in reversed(range(order + 1)):
        D[i] += D[i + 1]
    return D


def norm_terms(v, y, coef, rtol, atol):
    return coef * v / (atol + rtol * np.abs(y))


def norms_ref(D_after, y_after, order, rtol, atol, defect=None):
    """(ss_m, ss_p) = sum (error_const[order -+ 1] D[order], D[order + 2] / (atol + rtol |y|))^2 in extended precision, on the rows AFTER the
    update and y = y_new.  ss_m is meaningless at order 1, ss_p at order 5 (the controller does not ask for them); both are returned
    with the constants the controller would pass where they exist, else 1.  defect "ss_p_row": ss_p from row order + 1."""
    cm = ERROR_CONST[order - 1] if order > 1 else 1.0
    cp = ERROR_CONST[order + 1] if order < MAX_ORDER else 1.0
    sc = ext(atol) + ext(rtol) * np.abs(ext(y_after))
    rows = (order, order + 1 if defect == "ss_p_row" else order + 2)
    out = []
    for coef, row in zip((cm, cp), rows):
        e = ext(coef) * ext(D_after[row]) / sc
        out.append(float(np.sum(e * e)))
    return out[0], out[1], cm, cp


def norms_f64(D_after, y_after, order, rtol, atol, defect=None):
    """the same sums in float64 (numpy's pairwise sum)"""
    cm = ERROR_CONST[order - 1] if order > 1 else 1.0
    cp = ERROR_CONST[order + 1] if order < MAX_ORDER else 1.0
    rows = (order, order + 1 if defect == "ss_p_row" else order + 2)
    return tuple(float(np.sum(norm_terms(D_after[row], y_after, coef, rtol, atol) ** 2)) for coef, row in zip((cm, cp), rows))


def norm_bound(n):
    """relative: 5 roundings per term (product, product, sum, quotient, square - a fused multiply-add only removes one), the per-thread
    chain of ceil(n / 1024) additions, ten tree levels, and a factor 2.  Every term is non-negative, so the bound is relative."""
    return 2 * (5 + math.ceil(n / 1024) + 10) * EPS


# ---- SAMPLE ----------------------------------------------------------------------------------------------------------------------
def dense_weights(t, h, order, tq):
    """bdf_dense_weights (marl_bdf_ctl.h) in float64, every operation rounded on its own: p[j] = prod_{i <= j} (tq - (t - h i)) / (h (1 + i))"""
    p, acc = np.zeros(MAX_ORDER + 1), 1.0
    for j in range(order):
        acc *= (tq - (t - h * j)) / (h * (1 + j))
        p[j] = acc
    return p


def sample_ref(D, order, t, h, tq):
    """(D[0] + sum_j D[j + 1] p[j] summed in extended precision, bound (order + 2) eps (|D[0]| + sum |D[j + 1] p[j]|))"""
    p = dense_weights(t, h, order, tq)
    Dx = ext(D[:order + 1])
    val = Dx[0] + sum(Dx[j + 1] * ext(p[j]) for j in range(order))
    A = np.abs(D[0]) + sum(np.abs(D[j + 1] * p[j]) for j in range(order))
    return f64(val), (order + 2) * EPS * A


def sample_f64(D, order, t, h, tq, defect=None):
    """the kernel's loop in float64.  defect "short": the sum stops one term early at the highest order"""
    p = dense_weights(t, h, order, tq)
    a = np.zeros(D.shape[1])
    for j in range(order - 1 if defect == "short" else order):
        a = a + D[j + 1] * p[j]
    return a + D[0]


# ---- ROOTS -----------------------------------------------------------------------------------------------------------------------
def monitor_on_dense(orc, P, N, D, order, t, h, e):
    """tq -> monitor e (oracle.events) of the step's dense state"""
    return lambda tq: float(orc.events(P, N, sample_ref(D, order, t, h, tq)[0])[e])


def root_ref(orc, P, N, D, order, t_old, t, e):
    """scipy.optimize.brentq with solve_ivp's tolerances (ivp.py:51-76) on monitor e of the dense state over [t_old, t]; h = t - t_old"""
    from scipy.optimize import brentq
    return brentq(monitor_on_dense(orc, P, N, D, order, t, t - t_old, e), t_old, t, xtol=4 * EPS, rtol=4 * EPS)


# ---- comparison ------------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the elements; equal bits count 0, a non-finite difference or a difference at bound 0 counts inf"""
    got, ref, bound = np.broadcast_arrays(np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.asarray(bound, dtype=np.float64))
    with np.errstate(all="ignore"):
        diff = np.abs(got - ref)
        q = np.where(bits(got).reshape(got.shape) == bits(ref).reshape(ref.shape), 0.0, diff / bound)
    q = np.where(np.isnan(q), np.inf, q)
    return float(q.max()) if q.size else 0.0


def sentinel(shape, tag):
    """quiet NaNs with a payload no arithmetic produces; `tag` (< 2^16) and the element's index in the low bits"""
    idx = np.arange(int(np.prod(shape)), dtype=np.uint64).reshape(shape)
    return (np.uint64(0x7FF8_5EED_0000_0000) | (np.uint64(tag) << np.uint64(20)) | (idx & np.uint64(0xFFFFF))).view(np.float64)


# ---- inputs of the tests ---------------------------------------------------------------------------------------------------------
GRIDS = (5, 33, 64, 409)          # n = 25 (below one block), 165 (no multiple of 256), 320, 2045 (above 1024, no multiple; the largest grid)
ROOT_GRIDS = (33, 409)            # both below roots_batch_kernel's 1024 threads: its `mine` mask is live
B = 3
LISTS = (None, (1,), (2, 0))      # every instance in order; one; two out of order (a list position never equals its instance)
ORDER_SETS = ((1, 2, 3), (4, 5, 1), (5, 3, 2))   # per launch: the instances' orders (orders 1 .. 5 all occur; the orders of one launch differ)
TOLS = ((1e-3, 1e-3), (1e-5, 1e-7), (1e-6, 1e-9))   # (rtol, atol) of instance 0, 1, 2
STEPS = (3.0e-3, 1.7e-5, 0.4)     # h of instance 0, 1, 2 (INIT_D)
INSTANCES = [{}, dict(k3=0.05, k4=0.05), dict(Phi0=0.7)]   # parameter overrides: three models in one context


def base_params(N):
    return scenario("default", N)


def state_of(N, b):
    """instance b's state: the scenarios' magnitudes (synthetic_state), another wave number and amplitude per instance"""
    return synthetic_state(base_params(N) | INSTANCES[b], N, amplitude=0.05 + 0.02 * b, waves=3 + 2 * b)


def make_D(N, seed, mixed=False):
    """(B, 8, n): row 0 the instance's state, row j about 10^-j of it (a decade per row), smooth sign pattern; mixed: random signs per
    element in every row (the sums cancel: the bounds' sum |...| is then far above the result)."""
    rng = np.random.default_rng(seed)
    n = 5 * N
    D = np.empty((B, ROWS, n))
    for b in range(B):
        y = state_of(N, b)
        for j in range(ROWS):
            D[b, j] = y * 10.0 ** -j * (0.5 + rng.random(n))
            if mixed:
                D[b, j] *= rng.choice([-1.0, 1.0], n)
            elif j:
                D[b, j] *= np.sign(np.sin(0.37 * (j + 1) * np.arange(n) + b) + 0.2)
    return D


def make_vectors(N, seed, orders):
    """(y, f, d, ynew), each (B, n): f a rate of the states' size, d of the size of row order + 1, ynew near the state"""
    rng = np.random.default_rng(seed + 1000)
    n = 5 * N
    y = np.stack([state_of(N, b) for b in range(B)])
    f = y * (rng.random((B, n)) - 0.5) * 40
    d = np.stack([y[b] * 10.0 ** -(orders[b] + 1) * (rng.random(n) - 0.3) for b in range(B)])
    ynew = y * (1 + 1e-3 * (rng.random((B, n)) - 0.5))
    return y, f, d, ynew


# SAMPLE: the shared sample times (dyadic: t - h is exact) and per instance (t, h, first, end) - three launch plans.
#   plan 0  instance 0: samples 1 .. 5 = t - h, three inside the step, t;  instance 1: t - h, t and an end beyond n_eval (clipped);
#           instance 2: an empty range
#   plan 1  the ranges rotated: the empty one on instance 0, the clipped one on instance 2
#   plan 2  every instance extrapolates over all eight samples (weights up to |p| >> 1)
T_EVAL = np.array([0.25, 0.5, 0.5625, 0.625, 0.6875, 0.75, 0.875, 1.0])
SAMPLE_PLANS = (
    ((0.75, 0.25, 1, 6), (1.0, 0.125, 6, 11), (0.625, 0.0625, 3, 3)),
    ((0.625, 0.0625, 5, 5), (0.75, 0.25, 1, 6), (1.0, 0.125, 6, 9)),
    ((0.8125, 0.3, 0, 8), (1.0, 0.77, 0, 8), (0.7, 0.21, 0, 8)),
)


# ROOTS: the dense output of one accepted step from y_old (at t_old) to y_new (at t), D[0] = y_new, D[1] = y_new - y_old, small higher
# differences (at t_old every weight from p[1] on is 0, so the dense state there is D[0] - D[1] whatever they are).
#   instance 0  ca_low +1e-3 -> -1e-3: monitors 0 (the smallest value of all fields) and 1 (the smallest CA) cross in the same step
#   instance 1  a porosity dip 0.035 -> 0.04 across the zeros_U threshold: monitor 5
#   instance 2  ca_low +2e-3 -> -2e-3 with Phi0 = 0.7: monitors 0 and 1 again, other scalars
ROOT_STATES = ((dict(ca_low=1e-3), dict(ca_low=-1e-3)), (dict(phi_dip=0.035), dict(phi_dip=0.04)), (dict(ca_low=2e-3), dict(ca_low=-2e-3)))
ROOT_MASKS = (0b11, 1 << 5, 0b11)
ROOT_STEPS = ((0.37, 0.381), (2.0e-3, 2.3e-3), (11.0, 11.5))   # (t_old, t) of instance 0, 1, 2
ROOT_SLOTS = ((0, 1, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 1, 0), (1, 0, 0, 0, 0, 0, 0))   # max_events = 2: slot 1 for one monitor per instance
MAX_EVENTS = 2


def make_root_D(N, orders):
    """(B, 8, n) for ROOTS with the instances' orders; rows above an instance's order are left 0 (the test overwrites them)"""
    from test_gpu_rk23 import bump_state   # (the states of the event sweeps: the initial values with a Gaussian dip in Phi or CA)
    n = 5 * N
    D = np.zeros((B, ROWS, n))
    x = np.arange(n)
    for b in range(B):
        p = base_params(N) | INSTANCES[b]
        y_old, y_new = (bump_state(p, N, **kw) for kw in ROOT_STATES[b])
        D[b, 0], D[b, 1] = y_new, y_new - y_old
        for j in range(2, orders[b] + 1):
            D[b, j] = 0.3 ** (j - 1) * D[b, 1] * np.cos(0.05 * j * x)
    return D


# ---- one launch: what it must leave (expected), a float64 emulation of it (emulate), and the comparison both tests use ------------
# A launch is a dict: op, N, lst (None or instance indices), D (B, 8, n) and, as the op needs them: y, f, d, ynew (B, n); h, orders,
# RU (B, 6, 6), tols, want (per instance); plan ((t, h, first, end) per instance), t_eval, frames (B, n_eval, n); ss (B, 2).
def listed(launch):
    return list(range(B)) if launch["lst"] is None else list(launch["lst"])


def expected(launch):
    """name -> (ref, bound) for D, y, frames, ss: ref holds the input's bits wherever the launch must write nothing, bound 0 demands
    equal bits"""
    op, D0 = launch["op"], launch["D"]
    n = D0.shape[2]
    out = {"D": [D0.copy(), np.zeros_like(D0)], "y": [launch["y"].copy(), np.zeros_like(launch["y"])]}
    if "frames" in launch:
        out["frames"] = [launch["frames"].copy(), np.zeros_like(launch["frames"])]
    if "ss" in launch:
        out["ss"] = [launch["ss"].copy(), np.zeros_like(launch["ss"])]
    for b in listed(launch):
        if op == "INIT_D":
            out["D"][0][b, :2] = init_D_ref(launch["y"][b], launch["f"][b], launch["h"][b])
        elif op == "CHANGE_D":
            k = launch["orders"][b]
            out["D"][0][b, :k + 1], out["D"][1][b, :k + 1] = change_D_ref(D0[b], k, launch["RU"][b])
        elif op == "ACCEPT_NORMS":
            k, (rtol, atol) = launch["orders"][b], launch["tols"][b]
            out["D"][0][b] = accept_ref(D0[b], launch["d"][b], k)
            out["y"][0][b] = launch["ynew"][b]
            sm, sp, _, _ = norms_ref(out["D"][0][b], launch["ynew"][b], k, rtol, atol)
            for bit, v in ((0, sm), (1, sp)):
                if (launch["want"][b] >> bit) & 1:
                    out["ss"][0][b, bit], out["ss"][1][b, bit] = v, norm_bound(n) * v
        elif op == "SAMPLE":
            t, h, first, end = launch["plan"][b]
            for k in range(first, min(end, len(launch["t_eval"]))):
                out["frames"][0][b, k], out["frames"][1][b, k] = sample_ref(D0[b], launch["orders"][b], t, h, launch["t_eval"][k])
    return {k: tuple(v) for k, v in out.items()}


def emulate(launch, defect=None):
    """the launch by the float64 restatements, in place on copies of the inputs, with the kernels' list semantics.  Defects:
    "transposed" (CHANGE_D), "short" (SAMPLE: order 5 only, the highest), "ss_p_row" (ACCEPT_NORMS), "list_position" (SAMPLE: the frame
    goes to the list position's slot), "unwritten_last" (every op: element n - 1 of what the launch writes stays as it was)."""
    op = launch["op"]
    got = {k: launch[k].copy() for k in ("D", "y", "frames", "ss") if k in launch}
    keep = slice(None, -1) if defect == "unwritten_last" else slice(None)
    for pos, b in enumerate(listed(launch)):
        D0 = launch["D"][b]
        if op == "INIT_D":
            got["D"][b, :2, keep] = init_D_ref(launch["y"][b], launch["f"][b], launch["h"][b])[:, keep]
        elif op == "CHANGE_D":
            k = launch["orders"][b]
            got["D"][b, :k + 1, keep] = change_D_f64(D0, k, launch["RU"][b], defect)[:, keep]
        elif op == "ACCEPT_NORMS":
            k, (rtol, atol) = launch["orders"][b], launch["tols"][b]
            after = accept_ref(D0, launch["d"][b], k)
            got["D"][b, :, keep] = after[:, keep]
            got["y"][b, keep] = launch["ynew"][b][keep]
            ss = norms_f64(got["D"][b], got["y"][b], k, rtol, atol, defect)
            for bit in (0, 1):
                if (launch["want"][b] >> bit) & 1:
                    got["ss"][b, bit] = ss[bit]
        elif op == "SAMPLE":
            t, h, first, end = launch["plan"][b]
            k_ord = launch["orders"][b]
            for k in range(first, min(end, len(launch["t_eval"]))):
                fr = sample_f64(D0, k_ord, t, h, launch["t_eval"][k], defect if k_ord == MAX_ORDER else None)
                got["frames"][pos if defect == "list_position" else b, k, keep] = fr[keep]
    return got


def compare(launch, got):
    """name -> worst |got - ref| / bound over the array (0: all within, bit-equal where demanded; inf: a value where none may be, or a
    sentinel where a value belongs)"""
    return {k: worst_ratio(got[k], ref, bound) for k, (ref, bound) in expected(launch).items()}


def launches(op, N, seed=0):
    """the launches of one op on one grid: every list x every order set (x what the op adds), inputs with sentinels in every place
    the launch does not own"""
    n = 5 * N
    for li, lst in enumerate(LISTS):
        for oi, orders in enumerate(ORDER_SETS):
            mixed = (li + oi) % 3 == 2
            D = make_D(N, seed + 10 * li + oi, mixed)
            y, f, d, ynew = make_vectors(N, seed + 10 * li + oi, orders)
            base = dict(op=op, N=N, lst=lst, orders=orders, mixed=mixed)
            if op == "INIT_D":
                if oi:
                    continue      # (no order)
                yield base | dict(D=sentinel((B, ROWS, n), 1), y=y, f=f, h=STEPS)
            elif op == "CHANGE_D":
                for b in range(B):
                    D[b, orders[b] + 1:] = sentinel((ROWS - orders[b] - 1, n), 2 + b)
                for fi in range(len(FACTORS)):
                    RU = np.stack([scipy_RU(orders[b], FACTORS[(fi + b) % len(FACTORS)]) for b in range(B)])
                    yield base | dict(D=D, y=sentinel((B, n), 7), RU=RU, factors=[FACTORS[(fi + b) % len(FACTORS)] for b in range(B)])
            elif op == "ACCEPT_NORMS":
                for b in range(B):
                    D[b, orders[b] + 2:] = sentinel((ROWS - orders[b] - 2, n), 2 + b)
                for w0 in range(4):
                    yield base | dict(D=D, y=sentinel((B, n), 7), d=d, ynew=ynew, tols=TOLS, want=[(w0 + b) % 4 for b in range(B)], ss=sentinel((B, 2), 8))
            elif op == "SAMPLE":
                for b in range(B):
                    D[b, orders[b] + 1:] = sentinel((ROWS - orders[b] - 1, n), 2 + b)
                yield base | dict(D=D, y=sentinel((B, n), 7), plan=SAMPLE_PLANS[(li + oi) % len(SAMPLE_PLANS)], t_eval=T_EVAL,
                                  frames=sentinel((B, len(T_EVAL), n), 9))
