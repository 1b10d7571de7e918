#!/usr/bin/env python3
"""What the native DOP853 loop buys and what its storage of the stage derivatives costs.  A measurement, not a test: no threshold.

    python tools/dop853_timing.py [--rounds 5] [--out profiles/dop853_timing.log]

  single  integrate_equations(method="DOP853") on the reference's default scenario at N = 200 with the Solver's defaults (first_step 1e-6,
          rtol = atol = 1e-3) over t_span (0, 2e-4), the span of test_every_other_method_..._runs_through_scipy_on_the_hip_rhs: the native
          route (marl_integrate_dop853) against scipy's solve_ivp driving the HIP RHS and monitors (scipy_driver=True - the route of this
          method before the native loop existed, the same code).  Wall times of the whole call, medians over the rounds, alternating; the
          evaluations either route reports; the ratio.
  sweep   512 instances of a 16 x 32 Phi0 x PhiIni grid (0.5 .. 0.8 each; PhiNR = PhiIni) at N = 200, uniform initial state, rtol 1e-5,
          atol 1e-7, first_step 1e-6, to t1 = 0.002, through marl_sweep_rk45_dev and marl_sweep_dop853_dev, alternating: wall time,
          attempts, RHS evaluations (sums of the statistics) and evaluations per second - RK45 keeps its stage derivatives in registers,
          DOP853 in a global arena, so the two rates side by side say what that storage costs per evaluation.

One JSON line, printed and appended to --out."""
import argparse
import json
import os
import sys
import time
from dataclasses import asdict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def single(rounds):
    from marlpde_amd.Evolve_scenario import integrate_equations
    from marlpde_amd.LHeureux_model import LMAHeureuxPorosityDiff
    from marlpde_amd.parameters import Map_Scenario, Solver, Tracker
    from dataclasses import replace
    N, t1 = 200, 2e-4
    p = asdict(Map_Scenario()) | {"N": N}
    solver = asdict(replace(Solver(), method="DOP853", t_span=(0.0, t1)))
    tracker = asdict(Tracker()) | {"t_eval": np.linspace(0.0, t1, 2)}
    routes = {"native": solver, "scipy_driver": solver | {"scipy_driver": True}}
    last, times = {}, {k: [] for k in routes}
    for k, s in routes.items():   # warm-up
        last[k] = integrate_equations(s, tracker, p, results_root=None, verbose=False)[0]
    for _ in range(rounds):
        for k, s in routes.items():
            t = time.perf_counter()
            integrate_equations(s, tracker, p, results_root=None, verbose=False)
            times[k].append(time.perf_counter() - t)
    eq = LMAHeureuxPorosityDiff.from_scenario(p, device=0)
    y0 = eq.get_state(p["CAIni"], p["CCIni"], p["cCaIni"], p["cCO3Ini"], p["PhiIni"]).ravel()
    r = eq.integrate_dop853(y0, (0.0, t1), solver["first_step"], solver["rtol"], solver["atol"], t_eval=tracker["t_eval"])
    eq.close()
    out = {"N": N, "t1": t1, "rtol": solver["rtol"], "atol": solver["atol"], "first_step": solver["first_step"],
           "native_nfev": int(r.nfev), "native_attempts": int(r.n_accepted + r.n_rejected), "native_status": int(r.status),
           "max_abs_difference_of_the_last_profiles": float(np.max(np.abs(last["native"] - last["scipy_driver"])))}
    for k, ts in times.items():
        out[k + "_median_ms"] = 1e3 * float(np.median(ts))
        out[k + "_min_ms"] = 1e3 * min(ts)
    out["scipy_driver_over_native_time"] = out["scipy_driver_median_ms"] / out["native_median_ms"]
    return out


def sweep(rounds):
    import torch
    from marlpde_amd.LHeureux_model import LMAHeureuxPorosityDiff
    from marlpde_amd.parameters import Map_Scenario
    from marlpde_amd.sweep import initial_states, product_grid
    N, t1, rtol, atol, h0 = 200, 2e-3, 1e-5, 1e-7, 1e-6
    p = asdict(Map_Scenario()) | {"N": N}
    inst = product_grid(Phi0=np.linspace(0.5, 0.8, 16), PhiIni=np.linspace(0.5, 0.8, 32))
    for d in inst:
        d["PhiNR"] = d["PhiIni"]
    eq = LMAHeureuxPorosityDiff.from_scenario(p, device=0, instances=inst)
    eq.use_stream(torch.cuda.current_stream().cuda_stream)
    y0 = torch.from_numpy(initial_states(p, inst)).cuda()
    entries = {"rk45": eq.sweep_rk45_device, "dop853": eq.sweep_dop853_device}

    def call(name):
        buf = y0.clone()
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = entries[name](buf.data_ptr(), (0.0, t1), h0, rtol, atol, max_attempts=0)
        torch.cuda.synchronize()
        return time.perf_counter() - t, res

    out = {"instances": len(inst), "N": N, "t1": t1, "rtol": rtol, "atol": atol, "first_step": h0}
    times = {name: [] for name in entries}
    for name in entries:   # warm-up, and the counts (the runs are deterministic)
        _, res = call(name)
        out[name] = {"attempts": int(sum(r.n_accepted + r.n_rejected for r in res)), "rejected": int(sum(r.n_rejected for r in res)),
                     "nfev": int(sum(r.nfev for r in res)), "reached_t1": int(sum(r.status == 0 for r in res))}
    for _ in range(rounds):
        for name in entries:
            times[name].append(call(name)[0])
    eq.close()
    for name, ts in times.items():
        med = float(np.median(ts))
        out[name] |= {"median_ms": 1e3 * med, "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts),
                      "evaluations_per_second": out[name]["nfev"] / med, "cell_evaluations_per_second": out[name]["nfev"] * N / med}
    out["rk45_over_dop853_evaluations_per_second"] = out["rk45"]["evaluations_per_second"] / out["dop853"]["evaluations_per_second"]
    out["dop853_over_rk45_time"] = out["dop853"]["median_ms"] / out["rk45"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dop853_timing.log"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU path to time"
    out = {"tool": "tools/dop853_timing.py", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "single": single(args.rounds), "sweep": sweep(args.rounds)}
    line = json.dumps(out)
    print(line)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
