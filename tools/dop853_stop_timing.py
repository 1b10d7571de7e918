#!/usr/bin/env python3
"""What the DOP853 kernel that stops at a terminal monitor's root costs an ordinary step, and what a stop saves.  A measurement, not a
test: no threshold.

    python tools/dop853_stop_timing.py [--rounds 5] [--out profiles/dop853_stop_timing.log]

  never   the 512-instance sweep of tools/dop853_timing.py (16 x 32 Phi0 x PhiIni grid, N = 200, rtol 1e-5, atol 1e-7, first_step 1e-6, to
          t1 = 0.002) with the monitors' roots located (max_events 64): through marl_sweep_dop853_events_dev, and through
          marl_sweep_dop853_stop_dev with a limit that is never met (zeros_CC: 1) - dop853_sweep_stop_kernel for every step.  Alternating,
          medians over the rounds; the ratio is what the TERM branches cost a step that meets no limit.  The two runs are compared bit
          for bit first.
  stops   the same sweep with ones_Phi: 1 through the stop entry: the time, and how many instances stop.
  single  integrate_equations(method="DOP853", terminal={"ones_Phi": True}) on the default scenario at N = 200, rtol 1e-5, atol 1e-7,
          first_step 1e-6, t_span (0, 0.03): native_terminal=True (marl_integrate_dop853_stop) against the scipy route (solve_ivp on the
          HIP RHS and monitors).  Wall times of the whole call, alternating; the time both routes stop at.

One JSON line, printed and appended to --out."""
import argparse
import json
import os
import sys
import time
from dataclasses import asdict, replace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sweeps(rounds):
    import torch
    from marlpde_amd.LHeureux_model import LMAHeureuxPorosityDiff
    from marlpde_amd.parameters import Map_Scenario
    from marlpde_amd.sweep import initial_states, product_grid
    N, t1, rtol, atol, h0, max_events = 200, 2e-3, 1e-5, 1e-7, 1e-6, 64
    p = asdict(Map_Scenario()) | {"N": N}
    inst = product_grid(Phi0=np.linspace(0.5, 0.8, 16), PhiIni=np.linspace(0.5, 0.8, 32))
    for d in inst:
        d["PhiNR"] = d["PhiIni"]
    eq = LMAHeureuxPorosityDiff.from_scenario(p, device=0, instances=inst)
    eq.use_stream(torch.cuda.current_stream().cuda_stream)
    y0 = torch.from_numpy(initial_states(p, inst)).cuda()
    routes = {"events_entry": (None, eq.sweep_dop853_device), "stop_entry_never_met": ({"zeros_CC": 1}, eq.sweep_dop853_stop_device),
              "stop_entry_ones_Phi": ({"ones_Phi": 1}, eq.sweep_dop853_stop_device)}

    def call(name):
        terminal, entry = routes[name]
        eq.set_terminal(terminal)
        buf = y0.clone()
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = entry(buf.data_ptr(), (0.0, t1), h0, rtol, atol, max_attempts=0, events=True, max_events=max_events)
        torch.cuda.synchronize()
        return time.perf_counter() - t, res, buf.cpu().numpy()

    out = {"instances": len(inst), "N": N, "t1": t1, "rtol": rtol, "atol": atol, "first_step": h0, "max_events": max_events}
    times, first = {name: [] for name in routes}, {}
    for name in routes:   # warm-up, and the counts (the runs are deterministic)
        _, res, y = call(name)
        first[name] = (res, y)
        out[name] = {"attempts": int(sum(r.n_accepted + r.n_rejected for r in res)), "nfev": int(sum(r.nfev for r in res)),
                     "roots": int(sum(len(t) for r in res for t in r.t_events)), "reached_t1": int(sum(r.status == 0 for r in res)),
                     "stopped": int(sum(r.status == 1 for r in res))}
    (ra, ya), (rb, yb) = first["events_entry"], first["stop_entry_never_met"]
    out["never_met_equals_the_events_entry_bit_for_bit"] = bool(
        np.array_equal(ya, yb) and all(a.nfev == b.nfev and a.t_reached == b.t_reached and all(np.array_equal(u, v) for u, v in zip(a.t_events, b.t_events))
                                       for a, b in zip(ra, rb)))
    for _ in range(rounds):
        for name in routes:
            times[name].append(call(name)[0])
    eq.close()
    for name, ts in times.items():
        out[name] |= {"median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts)}
    out["never_met_over_events_entry_time"] = out["stop_entry_never_met"]["median_ms"] / out["events_entry"]["median_ms"]
    out["ones_Phi_over_events_entry_time"] = out["stop_entry_ones_Phi"]["median_ms"] / out["events_entry"]["median_ms"]
    return out


def single(rounds):
    from marlpde_amd.Evolve_scenario import integrate_equations
    from marlpde_amd.parameters import Map_Scenario, Solver, Tracker
    N, t1 = 200, 0.03
    p = asdict(Map_Scenario()) | {"N": N}
    solver = asdict(replace(Solver(), method="DOP853", t_span=(0.0, t1), rtol=1e-5, atol=1e-7, first_step=1e-6))
    tracker = asdict(Tracker()) | {"t_eval": None}
    routes = {"native_terminal": solver | {"native_terminal": True}, "scipy_route": solver}
    covered, last, times = {}, {}, {k: [] for k in routes}
    for k, s in routes.items():   # warm-up
        last[k], covered[k], *_ = integrate_equations(s, tracker, p, results_root=None, verbose=False, terminal={"ones_Phi": True})
    for _ in range(rounds):
        for k, s in routes.items():
            t = time.perf_counter()
            integrate_equations(s, tracker, p, results_root=None, verbose=False, terminal={"ones_Phi": True})
            times[k].append(time.perf_counter() - t)
    out = {"N": N, "t1": t1, "rtol": solver["rtol"], "atol": solver["atol"], "first_step": solver["first_step"],
           "t_stop": {k: v / p["Tstar"] for k, v in covered.items()},
           "max_abs_difference_of_the_last_profiles": float(np.max(np.abs(last["native_terminal"] - last["scipy_route"])))}
    for k, ts in times.items():
        out[k + "_median_ms"] = 1e3 * float(np.median(ts))
        out[k + "_min_ms"] = 1e3 * min(ts)
    out["scipy_route_over_native_time"] = out["scipy_route_median_ms"] / out["native_terminal_median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dop853_stop_timing.log"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU path to time"
    out = {"tool": "tools/dop853_stop_timing.py", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "sweeps": sweeps(args.rounds), "single": single(args.rounds)}
    line = json.dumps(out)
    print(line)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
