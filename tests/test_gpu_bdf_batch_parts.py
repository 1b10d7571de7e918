"""The BDF sweep's five vector kernels on the device, ONE launch at a time (marl_debug_bdf_batch: the sweep's arena and stride, the
launchers sweep_bdf calls, its work-list semantics), against the references and bounds of tests/bdf_batch_ref.py (checked on the CPU in
tests/test_bdf_batch_reference_cpu.py, where the same comparison flags five injected defects by 100 x).

The whole-sweep tests (tests/test_gpu_sweep_bdf*.py) compare sweeps with single runs within 1e-4 .. 1e-6: an error of a vector kernel
below that is absorbed by the step control.  Here every launch is held per element:
  INIT_D, the differences and y of ACCEPT_NORMS     equal to the last bit
  CHANGE_D, SAMPLE                                  (order + 2) eps sum |terms|
  ss_m, ss_p of ACCEPT_NORMS                        relative 2 (5 + ceil(n / 1024) + 10) eps
  ROOTS                                             |t - t_ref| / h against brentq on the oracle's monitors, BDF_BATCH_ROOTS (tests/common.py)
and everything a launch does not own - instances not listed, rows of D above the op's, frames outside [first, end), root slots of
monitors not searched, sums not asked for, and the buffers of the other ops - must come back with the bits it went in with (NaNs with a
payload).  B = 3 instances with different parameters, orders and scalars in every launch; lists None, [1] and [2, 0].
The worst ratio of every bound is printed as a JSON line (pytest -rA)."""
import functools
import json

import numpy as np
import pytest

import bdf_batch_ref as R
from common import BDF_BATCH_ROOTS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def models():
    from marlpde_amd.LHeureux_model import LMAHeureuxPorosityDiff
    made = {}

    def get(N):
        if N not in made:
            made[N] = LMAHeureuxPorosityDiff.from_scenario(R.base_params(N), device=0, instances=R.INSTANCES)
        return made[N]
    yield get
    for eq in made.values():
        eq.close()


def run(eq, L):
    """the launch on the device; the buffers the op has nothing to do with go in as sentinels and must come back as they went"""
    n = 5 * L["N"]
    others = {k: R.sentinel(shape, tag) for k, shape, tag in (("frames", (R.B, 2, n), 11), ("t_events", (R.B, 7, R.MAX_EVENTS), 12), ("ss", (R.B, 2), 13))
              if k not in L}
    kw = dict(instances=L["lst"], order=L["orders"], **others)
    if "frames" in others:
        kw["t_eval"] = [0.1, 0.2]
    op = L["op"]
    if op == "INIT_D":
        kw |= dict(y=L["y"], f=L["f"], h=L["h"])
    elif op == "CHANGE_D":
        kw |= dict(y=L["y"], RU=L["RU"])
    elif op == "ACCEPT_NORMS":
        coef = [R.norms_ref(L["D"][b], L["ynew"][b], L["orders"][b], 1.0, 1.0)[2:] for b in range(R.B)]
        kw |= dict(y=L["y"], d=L["d"], ynew=L["ynew"], rtol=[t[0] for t in L["tols"]], atol=[t[1] for t in L["tols"]], want_norms=L["want"],
                   err_coef_m=[c[0] for c in coef], err_coef_p=[c[1] for c in coef], ss=L["ss"])
    elif op == "SAMPLE":
        kw |= dict(y=L["y"], t=[p[0] for p in L["plan"]], h=[p[1] for p in L["plan"]], first=[p[2] for p in L["plan"]], end=[p[3] for p in L["plan"]],
                   t_eval=L["t_eval"], frames=L["frames"])
    got = eq.debug_bdf_batch(op, L["D"], **kw)
    for k, v in others.items():
        assert R.same_bits(got[k], v), (op, k, "written by a launch that does not own it")
    return got


@pytest.mark.parametrize("N", R.GRIDS)
@pytest.mark.parametrize("op", ("INIT_D", "CHANGE_D", "ACCEPT_NORMS", "SAMPLE"))
def test_one_launch_against_its_reference(models, op, N):
    """Every launch of bdf_batch_ref.launches(op, N) - lists x order sets x (factors 0.2 / 0.9 / 10 | want_norms 0 .. 3 | sample plans: an
    empty range, an end beyond n_eval, samples at t - h, inside and at t) - within its bounds, sentinels intact.  A SAMPLE at tq == t is
    D[0] to the last bit (every weight is 0)."""
    eq = models(N)
    worst, count = {}, 0
    for L in R.launches(op, N):
        got = run(eq, L)
        count += 1
        for k, v in R.compare(L, got).items():
            worst[k] = max(worst.get(k, 0.0), v)
        if op == "SAMPLE":
            for b in R.listed(L):
                t, _, first, end = L["plan"][b]
                for k in range(first, min(end, len(L["t_eval"]))):
                    if L["t_eval"][k] == t:
                        assert R.same_bits(got["frames"][b, k], L["D"][b, 0]), (b, k)
    print("BDF_BATCH_PARTS", json.dumps({"op": op, "N": N, "launches": count, "worst_over_bound": worst}))
    assert count and max(worst.values()) <= 1, worst


@functools.lru_cache(maxsize=None)
def _root_refs(N, b, order):
    """brentq's roots of instance b's masked monitors on its dense output, once per session"""
    from oracle import oracle as orc
    orc.build()
    P = orc.params_from_dict(R.base_params(N) | R.INSTANCES[b])
    D = R.make_root_D(N, tuple(order if i == b else 1 for i in range(R.B)))[b]
    t_old, t = R.ROOT_STEPS[b]
    return {e: R.root_ref(orc, P, N, D, order, t_old, t, e) for e in range(7) if (R.ROOT_MASKS[b] >> e) & 1}


@pytest.mark.parametrize("N", R.ROOT_GRIDS)
def test_roots_against_brentq_on_the_oracle(models, N):
    """roots_batch_kernel on the dense output of one step (bdf_batch_ref.make_root_D), lists x order sets: the roots of the masked monitors
    of the listed instances in their slots (max_events = 2, slot 1 for one monitor per instance), every other slot untouched, D and y
    untouched; |t - t_ref| / h within BDF_BATCH_ROOTS["bound"] = 10 x the largest value measured on an MI355X (the margin of INCR_TOL /
    IMPLICIT_JAC_K: brentq and the kernel's Brent stop within 4 eps (1 + |t|) of the root of THEIR function, and the kernel's monitors
    differ from the oracle's by the roundings of F(Phi)'s table-driven exp).  Measured: 1.3e-14 at N = 33 (monitor 5, order 5), 7.2e-15 at
    N = 409 - far below the 1e-9 above which the figure would be a finding, not a number to record."""
    eq = models(N)
    n = 5 * N
    worst, at = 0.0, None
    for lst in R.LISTS:
        for orders in R.ORDER_SETS:
            D = R.make_root_D(N, orders)
            for b in range(R.B):
                D[b, orders[b] + 1:] = R.sentinel((R.ROWS - orders[b] - 1, n), 2 + b)
            y0, tev0, ss0 = R.sentinel((R.B, n), 7), R.sentinel((R.B, 7, R.MAX_EVENTS), 12), R.sentinel((R.B, 2), 13)
            got = eq.debug_bdf_batch("ROOTS", D, y=y0, instances=lst, order=orders, t_old=[s[0] for s in R.ROOT_STEPS], t=[s[1] for s in R.ROOT_STEPS],
                                     h=[s[1] - s[0] for s in R.ROOT_STEPS], mask=R.ROOT_MASKS, slot=R.ROOT_SLOTS, t_events=tev0, ss=ss0)
            assert R.same_bits(got["D"], D) and R.same_bits(got["y"], y0) and R.same_bits(got["ss"], ss0)
            want = tev0.copy()
            on = range(R.B) if lst is None else lst
            for b in on:
                t_old, t = R.ROOT_STEPS[b]
                for e, t_ref in _root_refs(N, b, orders[b]).items():
                    root = got["t_events"][b, e, R.ROOT_SLOTS[b][e]]
                    assert t_old < root < t, (b, e, root)
                    q = abs(root - t_ref) / (t - t_old)
                    if q > worst:
                        worst, at = q, dict(instance=b, monitor=e, order=orders[b], root=root, brentq=t_ref, list=lst)
                    want[b, e, R.ROOT_SLOTS[b][e]] = root
            assert R.same_bits(got["t_events"], want), "a root slot that is not the launch's was written"
            if lst is None:   # monitors 0 and 1 of instance 0 cross at the same root (the smallest value of all fields is the smallest CA)
                assert got["t_events"][0, 0, R.ROOT_SLOTS[0][0]] == got["t_events"][0, 1, R.ROOT_SLOTS[0][1]]
    print("BDF_BATCH_ROOTS", json.dumps({"N": N, "worst_dt_over_h": worst, "bound": BDF_BATCH_ROOTS["bound"], "at": at}))
    assert worst <= BDF_BATCH_ROOTS["bound"], (worst, at)


def test_hook_refuses_what_would_index_out_of_range(models):
    """every bad argument is a MarlError before anything is launched, and the context goes on working"""
    from marlpde_amd._abi import MarlError
    from marlpde_amd.LHeureux_model import LMAHeureuxPorosityDiff
    N = 33
    eq = models(N)
    n = 5 * N
    D = R.make_D(N, 0)
    ok = dict(order=(1, 2, 3), RU=np.stack([R.scipy_RU(k, 0.9) for k in (1, 2, 3)]))
    tev = R.sentinel((R.B, 7, R.MAX_EVENTS), 12)
    bad = [("CHANGE_D", ok | dict(order=(1, 0, 3)), "order"), ("CHANGE_D", ok | dict(order=(1, 2, 6)), "order"),
           ("ACCEPT_NORMS", dict(order=(1, 2, 6)), "order"), ("SAMPLE", dict(order=(1, 7, 3)), "order"), ("ROOTS", dict(order=(-1, 2, 3), t_events=tev), "order"),
           ("CHANGE_D", ok | dict(instances=[3]), "list entry"), ("CHANGE_D", ok | dict(instances=[0, -1]), "list entry"),
           ("CHANGE_D", ok | dict(instances=[0, 1, 2, 0]), "list"),
           ("SAMPLE", dict(order=2, first=3, end=2, t_eval=R.T_EVAL, frames=R.sentinel((R.B, len(R.T_EVAL), n), 9)), "first"),
           ("SAMPLE", dict(order=2, first=-1, end=2, t_eval=R.T_EVAL, frames=R.sentinel((R.B, len(R.T_EVAL), n), 9)), "first"),
           ("ACCEPT_NORMS", dict(order=2, want_norms=4), "want_norms"),
           ("ROOTS", dict(order=2, mask=1, t_old=0.0, t=1.0), "max_events"),
           ("ROOTS", dict(order=2, mask=1, slot=(R.MAX_EVENTS, 0, 0, 0, 0, 0, 0), t_events=tev), "slot"),
           ("ROOTS", dict(order=2, mask=128, t_events=tev), "mask")]
    for op, kw, word in bad:
        with pytest.raises(MarlError, match=word):
            eq.debug_bdf_batch(op, D, **kw)
    big = LMAHeureuxPorosityDiff.from_scenario(R.base_params(410), device=0, instances=R.INSTANCES)   # 5 N = 2050 > 2048
    try:
        with pytest.raises(MarlError, match="N <= 409"):
            big.debug_bdf_batch("INIT_D", np.zeros((R.B, R.ROWS, 5 * 410)))
    finally:
        big.close()
    L = next(R.launches("CHANGE_D", N))
    assert max(R.compare(L, run(eq, L)).values()) <= 1
