#!/usr/bin/env python3
"""What the large-grid DOP853 loop (marl_integrate_dop853_grid) buys over the scipy route, and what an attempt costs.  A measurement,
not a test: no threshold.

    python tools/dop853_grid_timing.py [--rounds 5] [--out profiles/dop853_grid_timing.log]

Every GPU step runs in a child process of its own under `timeout`; the steps are chained, and the first one that fails ends the run.

  single    integrate_equations(method="DOP853") on the reference's default scenario at N = 4096 with the Solver's tolerances (first_step
            1e-6, rtol = atol = 1e-3) over t_span (0, 1e-5): the native route (native_grid=True: marl_integrate_dop853_grid) against
            scipy's solve_ivp driving the HIP RHS and monitors (scipy_driver=True - the route of this grid before the native loop
            existed, the same code).  Wall times of the whole call, medians over the rounds, alternating; the evaluations of either
            route; the ratio.
  attempts  N = 2^20 and 2^22, default scenario, the synthetic state of the tests, first_step 0.5 dx^2, rtol 1e-5, atol 1e-7, a fixed
            budget of attempts through marl_integrate_dop853_grid_dev and marl_integrate_rk45_dev, alternating: time per attempt and per
            evaluation (12 and 6 per attempt), and the bytes per second the DOP853 attempt reaches under an ESTIMATE from the tableau, not
            a measurement: an attempt moves about 90 state-sized arrays (58 K reads over rows 1-12, 12 y reads, 13 writes, 8 K reads
            for the error sums: 3.6 KB per cell).

One JSON line, printed and appended to --out."""
import argparse
import json
import os
import subprocess
import sys
import time
from dataclasses import asdict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BYTES_PER_CELL_ESTIMATE = 90 * 5 * 8


def single(rounds):
    from dataclasses import replace

    from marlpde_amd.Evolve_scenario import integrate_equations
    from marlpde_amd.LHeureux_model import EVENT_NAMES, LMAHeureuxPorosityDiff
    from marlpde_amd.parameters import Map_Scenario, Solver, Tracker
    N, t1 = 4096, 1e-5
    p = asdict(Map_Scenario()) | {"N": N}
    solver = asdict(replace(Solver(), method="DOP853", t_span=(0.0, t1)))
    tracker = asdict(Tracker()) | {"t_eval": np.linspace(0.0, t1, 2)}
    routes = {"native_grid": solver | {"native_grid": True}, "scipy_driver": solver | {"scipy_driver": True}}
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
    r = eq.integrate_dop853_grid(y0, (0.0, t1), solver["first_step"], solver["rtol"], solver["atol"], t_eval=tracker["t_eval"])
    from scipy.integrate import solve_ivp
    sol = solve_ivp(eq.fun, (0.0, t1), y0, method="DOP853", t_eval=tracker["t_eval"], events=[getattr(eq, n) for n in EVENT_NAMES],
                    first_step=solver["first_step"], rtol=solver["rtol"], atol=solver["atol"])   # (the counts of the scipy route)
    eq.close()
    out = {"N": N, "t1": t1, "rtol": solver["rtol"], "atol": solver["atol"], "first_step": solver["first_step"],
           "native_nfev": int(r.nfev), "native_attempts": int(r.n_accepted + r.n_rejected), "native_rejected": int(r.n_rejected),
           "native_status": int(r.status), "scipy_nfev": int(sol.nfev), "scipy_status": int(sol.status),
           "max_abs_difference_of_the_last_profiles": float(np.max(np.abs(last["native_grid"] - last["scipy_driver"])))}
    for k, ts in times.items():
        out[k + "_median_ms"] = 1e3 * float(np.median(ts))
        out[k + "_min_ms"] = 1e3 * min(ts)
    out["scipy_driver_over_native_time"] = out["scipy_driver_median_ms"] / out["native_grid_median_ms"]
    return out


def attempts(rounds, N, budget):
    import torch
    from common import synthetic_state
    from marlpde_amd.LHeureux_model import LMAHeureuxPorosityDiff
    from marlpde_amd.parameters import Map_Scenario
    p = asdict(Map_Scenario()) | {"N": N}
    dx2 = ((p["max_depth"] / p["Xstar"]) / N) ** 2
    h0, t1, rtol, atol = 0.5 * dx2, 1e6 * dx2, 1e-5, 1e-7
    eq = LMAHeureuxPorosityDiff.from_scenario(p, device=0)
    eq.use_stream(torch.cuda.current_stream().cuda_stream)
    y0 = torch.from_numpy(synthetic_state(p, N, amplitude=0.01)).cuda()
    entries = {"rk45": (eq.integrate_rk45_device, 6), "dop853_grid": (eq.integrate_dop853_grid_device, 12)}

    def call(name, n):
        buf = y0.clone()
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = entries[name][0](buf.data_ptr(), (0.0, t1), h0, rtol, atol, 0, n)
        torch.cuda.synchronize()
        return time.perf_counter() - t, res

    out = {"N": N, "budget": budget, "rtol": rtol, "atol": atol, "first_step_in_dx2": 0.5}
    times = {name: [] for name in entries}
    for name in entries:   # warm-up (buffers, the arena), and the counts of a budgeted run
        call(name, 3)
        _, res = call(name, budget)
        out[name] = {"status": int(res.status), "attempts": int(res.n_accepted + res.n_rejected), "rejected": int(res.n_rejected), "nfev": int(res.nfev)}
    for _ in range(rounds):
        for name in entries:
            times[name].append(call(name, budget)[0])
    eq.close()
    for name, ts in times.items():
        med, n = float(np.median(ts)), out[name]["attempts"]
        out[name] |= {"median_ms": 1e3 * med, "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts), "ms_per_attempt": 1e3 * med / n,
                      "us_per_evaluation": 1e6 * med / (n * entries[name][1])}
    d = out["dop853_grid"]
    d["estimated_bytes_per_attempt"] = BYTES_PER_CELL_ESTIMATE * N
    d["estimated_TB_per_s"] = BYTES_PER_CELL_ESTIMATE * N / (1e-3 * d["ms_per_attempt"]) / 1e12
    d["arena_GB"] = 16 * 5 * N * 8 / 1e9
    out["dop853_over_rk45_time_per_evaluation"] = d["us_per_evaluation"] / out["rk45"]["us_per_evaluation"]
    return out


def step(args):
    import torch
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU path to time"
    if args.step == "single":
        out = single(args.rounds)
    else:
        out = attempts(args.rounds, args.N, args.budget)
    print("STEP " + json.dumps(out | {"device": torch.cuda.get_device_name(0)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dop853_grid_timing.log"))
    ap.add_argument("--step", choices=("single", "attempts"))
    ap.add_argument("--N", type=int, default=1 << 20)
    ap.add_argument("--budget", type=int, default=64)
    args = ap.parse_args()
    if args.step:
        return step(args)
    me = [sys.executable, os.path.abspath(__file__), "--rounds", str(args.rounds)]
    steps = [("single", 300, ["--step", "single"]), ("attempts_2^20", 180, ["--step", "attempts", "--N", str(1 << 20)]),
             ("attempts_2^22", 240, ["--step", "attempts", "--N", str(1 << 22)])]
    out = {"tool": "tools/dop853_grid_timing.py", "rounds": args.rounds}
    for name, limit, more in steps:   # chained: a step that fails, faults or runs into its limit ends the run
        r = subprocess.run(["timeout", "-k", "10", str(limit)] + me + more, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("STEP ")]
        if r.returncode != 0 or not lines:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"step {name} ended with status {r.returncode}: nothing further is run")
        out[name] = json.loads(lines[-1][5:])
    line = json.dumps(out)
    print(line)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
