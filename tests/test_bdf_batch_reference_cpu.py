"""The references, bounds and inputs of tests/test_gpu_bdf_batch_parts.py (tests/bdf_batch_ref.py), checked without a GPU:
  * the references are scipy's: CHANGE_D against scipy's change_D, SAMPLE against BdfDenseOutput, within twice the bound;
  * the comparison the GPU test applies to the device passes the plain float64 restatement of every launch and flags each injected
    defect by at least 100 x its bound (a value where none may be written, or a sentinel left where a value belongs, counts as inf);
  * the ROOTS inputs do what they were chosen for.
"""
import numpy as np
import pytest
from scipy.integrate._ivp import bdf as scipy_bdf

import bdf_batch_ref as R

OPS = ("INIT_D", "CHANGE_D", "ACCEPT_NORMS", "SAMPLE")


def test_extended_precision_has_64_bits():
    one = R.ext(1.0)
    assert (one + R.ext(2.0 ** -63)) - one != 0


@pytest.mark.parametrize("N", R.GRIDS)
def test_change_D_reference_is_scipys(N):
    worst = 0.0
    for L in R.launches("CHANGE_D", N):
        for b in range(R.B):
            k = L["orders"][b]
            D = L["D"][b].copy()
            scipy_bdf.change_D(D, k, L["factors"][b])
            ref, bound = R.change_D_ref(L["D"][b], k, L["RU"][b])
            worst = max(worst, R.worst_ratio(D[:k + 1], ref, 2 * bound))
            assert R.same_bits(D[k + 1:], L["D"][b][k + 1:])
    print("CHANGE_D reference against scipy.change_D, worst |diff| / (2 bound):", worst)
    assert worst <= 1


@pytest.mark.parametrize("N", R.GRIDS)
def test_sample_reference_is_scipys_dense_output(N):
    worst = 0.0
    for L in R.launches("SAMPLE", N):
        for b in range(R.B):
            k, (t, h, _, _) = L["orders"][b], L["plan"][b]
            sol = scipy_bdf.BdfDenseOutput(t - h, t, h, k, L["D"][b][:k + 1])
            for tq in L["t_eval"]:
                ref, bound = R.sample_ref(L["D"][b], k, t, h, tq)
                worst = max(worst, R.worst_ratio(sol(tq), ref, 2 * bound))
                if tq == t:   # every weight is 0: the state itself
                    assert R.same_bits(ref, L["D"][b][0]) and R.same_bits(R.sample_f64(L["D"][b], k, t, h, tq), L["D"][b][0])
    print("SAMPLE reference against BdfDenseOutput, worst |diff| / (2 bound):", worst)
    assert worst <= 1


def test_accept_reference_is_scipys_statements():
    """bdf.py:414-418 on a copy, spelled as scipy spells them"""
    L = next(R.launches("ACCEPT_NORMS", 33))
    for b in range(R.B):
        order, d = L["orders"][b], L["d"][b]
        D = L["D"][b].copy()
        D[order + 2] = d - D[order + 1]
        D[order + 1] = d
        for i in reversed(range(order + 1)):
            D[i] += D[i + 1]
        assert R.same_bits(D, R.accept_ref(L["D"][b], d, order))
        # scipy's scaled norms of the order selection from the same rows (bdf.py:427-437), as sums of squares
        rtol, atol = L["tols"][b]
        scale = atol + rtol * np.abs(L["ynew"][b])
        sm, sp, cm, cp = R.norms_ref(D, L["ynew"][b], order, rtol, atol)
        n = D.shape[1]
        for ss, coef, row in ((sm, cm, order), (sp, cp, order + 2)):
            assert ss == pytest.approx(n * scipy_bdf.norm(coef * D[row] / scale) ** 2, rel=1e-13)


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("N", R.GRIDS)
def test_float64_restatement_passes_every_launch(op, N):
    worst = {}
    for L in R.launches(op, N):
        for k, v in R.compare(L, R.emulate(L)).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(op, N, "float64 restatement, worst |diff| / bound:", worst)
    assert worst and max(worst.values()) <= 1


def _applies(defect, L):
    """does the defect change anything this launch writes?"""
    on = R.listed(L)
    if defect == "transposed":
        return L["op"] == "CHANGE_D"
    if defect == "ss_p_row":
        return L["op"] == "ACCEPT_NORMS" and any(L["want"][b] & 2 for b in on)
    samples = L["op"] == "SAMPLE" and [b for b in on if min(L["plan"][b][3], len(R.T_EVAL)) > L["plan"][b][2]]
    if defect == "short":     # (a sample at tq == t has every weight 0: a range with another sample)
        return bool(samples) and any(L["orders"][b] == R.MAX_ORDER and any(tq != L["plan"][b][0] for tq in R.T_EVAL[L["plan"][b][2]:L["plan"][b][3]])
                                     for b in samples)
    if defect == "list_position":
        return bool(samples) and any(pos != b for pos, b in enumerate(on) if b in samples)
    if defect == "unwritten_last":
        return L["op"] != "SAMPLE" or bool(samples)
    raise KeyError(defect)


@pytest.mark.parametrize("defect,ops", [("transposed", ("CHANGE_D",)), ("short", ("SAMPLE",)), ("unwritten_last", OPS), ("ss_p_row", ("ACCEPT_NORMS",)),
                                        ("list_position", ("SAMPLE",))])
def test_bounds_flag_each_injected_defect(defect, ops):
    """every launch the defect can show in exceeds a bound by at least 100 x - on every grid"""
    for op in ops:
        for N in R.GRIDS:
            hit, least = 0, np.inf
            for L in R.launches(op, N):
                if _applies(defect, L):
                    hit += 1
                    least = min(least, max(R.compare(L, R.emulate(L, defect)).values()))
            print(defect, op, N, "launches:", hit, "smallest worst ratio:", least)
            assert hit > 0 and least >= 100, (defect, op, N, hit, least)


def test_launches_cover_what_they_were_chosen_for():
    orders, wants5, factors = set(), set(), set()
    for op in OPS:
        for L in R.launches(op, 33):
            assert len(set(L["orders"])) == R.B           # the instances of one launch hold different orders
            orders |= {L["orders"][b] for b in R.listed(L)}
            if op == "ACCEPT_NORMS":
                wants5 |= {L["want"][b] for b in R.listed(L) if L["orders"][b] == R.MAX_ORDER}   # want & 2 at order 5 reads row 7
                assert len(set(L["want"])) == R.B
            if op == "CHANGE_D":
                factors |= set(L["factors"])
    assert orders == {1, 2, 3, 4, 5} and {2, 3} <= wants5 and factors == set(R.FACTORS)
    assert any(L["mixed"] for L in R.launches("SAMPLE", 33)) and any(not L["mixed"] for L in R.launches("SAMPLE", 33))
    plans = [p for plan in R.SAMPLE_PLANS for p in plan]
    assert any(f == e for _, _, f, e in plans) and any(e > len(R.T_EVAL) for _, _, f, e in plans)
    t, h, f, e = R.SAMPLE_PLANS[0][0]
    inside = [tq for tq in R.T_EVAL[f:e] if t - h < tq < t]
    assert t in R.T_EVAL[f:e] and t - h in R.T_EVAL[f:e] and len(inside) == 3


@pytest.mark.parametrize("N", R.ROOT_GRIDS)
@pytest.mark.parametrize("orders", R.ORDER_SETS)
def test_root_inputs_do_what_they_were_chosen_for(oracle, N, orders):
    """exactly the masked monitors change sign over [t_old, t]; monitors 0 and 1 do so in the same step of instance 0; every root lies
    strictly inside its step"""
    D = R.make_root_D(N, orders)
    for b in range(R.B):
        P = oracle.params_from_dict(R.base_params(N) | R.INSTANCES[b])
        t_old, t = R.ROOT_STEPS[b]
        changed = 0
        for e in range(7):
            g = R.monitor_on_dense(oracle, P, N, D[b], orders[b], t, t - t_old, e)
            ga, gb = g(t_old), g(t)
            assert ga != 0 and gb != 0
            if ga * gb < 0:
                changed |= 1 << e
                root = R.root_ref(oracle, P, N, D[b], orders[b], t_old, t, e)
                assert t_old < root < t
        assert changed == R.ROOT_MASKS[b], (b, bin(changed))
    assert R.ROOT_MASKS[0] == 0b11
    assert all(sum(s) == 1 and max(s) == 1 and max(s) < R.MAX_EVENTS for s in R.ROOT_SLOTS)
