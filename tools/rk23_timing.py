#!/usr/bin/env python3
"""The same sweeps through the RK45 and the RK23 entries (marl_sweep_rk45_dev, marl_sweep_rk23_dev), same build, same process, the two
entries alternating in every round; medians over the rounds.  A measurement, not a test: there is no threshold.

    python tools/rk23_timing.py [--rounds 7] [--skip-bench-shape]

  to_t1   512 instances of a 16 x 32 Phi0 x PhiIni grid (0.5 .. 0.8 each; PhiNR = PhiIni) at N = 200, uniform initial state, rtol = atol =
          1e-3, first_step 1e-6, to t1 = 0.01: what an explicit user waits for - the same time reached by either method.  Per entry: wall
          time, attempts, rejections and RHS evaluations (sums over the instances, from the statistics), instances that reached t1.
  budget  the bench's sweep shape (bench.py --workload sweep_rk45: 4096 instances x 1024 cells, the 16 x 16 x 16 parameter grid, the synthetic
          state, rtol = atol = 1e-3, first_step 0.5 dx^2) for 60 attempts: the cost of an attempt (3 against 6 evaluations after K1).

Each call is timed with a host clock around the (synchronising) entry, the state copy excluded.  One JSON line in all.
Where a run on an MI355X is recorded: profiles/rk23_timing.log, with the figures in DESIGN.md."""
import argparse
import json
import os
import sys
import time
from dataclasses import asdict

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def measure(torch, eq, y0, t_span, first_step, rtol, atol, max_attempts, rounds):
    entries = {"rk45": eq.sweep_rk45_device, "rk23": eq.sweep_rk23_device}

    def call(name):
        buf = y0.clone()
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = entries[name](buf.data_ptr(), t_span, first_step, rtol, atol, max_attempts=max_attempts)
        torch.cuda.synchronize()
        return time.perf_counter() - t, res

    out, times = {}, {name: [] for name in entries}
    for name in entries:                                      # warm-up, and the counts (the runs are deterministic)
        _, res = call(name)
        out[name] = {"attempts": int(sum(r.n_accepted + r.n_rejected for r in res)), "rejected": int(sum(r.n_rejected for r in res)),
                     "nfev": int(sum(r.nfev for r in res)), "reached_t1": int(sum(r.status == 0 for r in res)),
                     "status_counts": {str(s): int(sum(r.status == s for r in res)) for s in sorted({r.status for r in res})}}
    for _ in range(rounds):
        for name in entries:
            times[name].append(call(name)[0])
    for name, ts in times.items():
        out[name] |= {"median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts)}
        out[name]["us_per_attempt_per_instance"] = 1e6 * float(np.median(ts)) / max(out[name]["attempts"], 1)
    out["rk45_over_rk23_time"] = out["rk45"]["median_ms"] / out["rk23"]["median_ms"]
    out["rk45_over_rk23_nfev"] = out["rk45"]["nfev"] / out["rk23"]["nfev"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--skip-bench-shape", action="store_true")
    args = ap.parse_args()
    import torch
    from bench import synthetic
    from marlpde_amd.LHeureux_model import LMAHeureuxPorosityDiff
    from marlpde_amd.parameters import Map_Scenario
    from marlpde_amd.sweep import initial_states, product_grid
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU path to time"
    out = {"rounds": args.rounds}

    N = 200
    p = asdict(Map_Scenario()) | {"N": N}
    inst = product_grid(Phi0=np.linspace(0.5, 0.8, 16), PhiIni=np.linspace(0.5, 0.8, 32))
    for d in inst:
        d["PhiNR"] = d["PhiIni"]
    eq = LMAHeureuxPorosityDiff.from_scenario(p, device=0, instances=inst)
    eq.use_stream(torch.cuda.current_stream().cuda_stream)
    y0 = torch.from_numpy(initial_states(p, inst)).cuda()
    out["to_t1"] = {"instances": len(inst), "N": N, "t1": 0.01, "rtol": 1e-3, "atol": 1e-3, "first_step": 1e-6}
    out["to_t1"] |= measure(torch, eq, y0, (0.0, 0.01), 1e-6, 1e-3, 1e-3, 0, args.rounds)
    eq.close()

    if not args.skip_bench_shape:
        B, N, attempts = 4096, 1024, 60
        k = max(1, round(B ** (1 / 3)))
        inst = [{"Phi0": float(0.5 + 0.3 * ((i % k) / max(k - 1, 1))), "PhiIni": float(0.5 + 0.3 * (((i // k) % k) / max(k - 1, 1))),
                 "k3": float(10 ** (-2 + ((i // (k * k)) % k) / max(k - 1, 1)))} for i in range(B)]
        for d in inst:
            d["PhiNR"], d["k4"] = d["PhiIni"], d["k3"]
        p = asdict(Map_Scenario()) | {"N": N}
        eq = LMAHeureuxPorosityDiff.from_scenario(p, device=0, instances=inst)
        eq.use_stream(torch.cuda.current_stream().cuda_stream)
        y0 = torch.from_numpy(np.stack([synthetic(p | d, N) for d in inst])).cuda()
        dx2 = (eq.Depths.length / N) ** 2
        out["budget"] = {"instances": B, "N": N, "max_attempts": attempts, "rtol": 1e-3, "atol": 1e-3, "first_step_over_dx2": 0.5}
        out["budget"] |= measure(torch, eq, y0, (0.0, 1.0e9), 0.5 * dx2, 1e-3, 1e-3, attempts, args.rounds)
        eq.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
