"""BDF sweeps, thread pool of single runs against the batched kernels (needs a GPU):  python3 tools/bdf_sweep_ab.py [--sizes 64 512] [--reps 5]

run_sweep_bdf on one GPU over product_grid(Phi0, k3 = k4) at N = 200, t_span (0, 1), first step 1e-6, rtol = atol = 1e-3: once with
the thread pool (concurrent marl_integrate_bdf runs, at its own limit of 16 workers) and once with batched=True (marl_sweep_bdf_dev).
One warm-up each, then alternating repetitions in one process; medians and spread per size, and how far the two agree."""
import argparse
import json
import os
import sys
import time
from dataclasses import asdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402

from marlpde_amd.parameters import Map_Scenario  # noqa: E402
from marlpde_amd.sweep import initial_states, product_grid, run_sweep_bdf  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", type=int, nargs="+", default=[64, 512])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--N", type=int, default=200)
args = ap.parse_args()

base = asdict(Map_Scenario()) | {"N": args.N}
ARGS = ((0.0, 1.0), 1e-6, 1e-3, 1e-3)
for B in args.sizes:
    nk = 8 if B <= 64 else 16
    insts = product_grid(Phi0=np.linspace(0.5, 0.7, B // nk), k3=np.logspace(-2, -1, nk))
    for d in insts:
        d.update(PhiIni=d["Phi0"], PhiNR=d["Phi0"], k4=d["k3"])
    y0 = initial_states(base, insts)
    times = {False: [], True: []}
    out = {}
    for rep in range(-1, args.reps):   # -1: warm-up (module load, allocations)
        for batched in (False, True):
            t0 = time.perf_counter()
            out[batched] = run_sweep_bdf(base, insts, *ARGS, y0=y0, device=0, batched=batched)
            if rep >= 0:
                times[batched].append(time.perf_counter() - t0)
    (yp, sp, ap_, rp, tp), (yb, sb, ab, rb, tb) = out[False], out[True]
    same = int(np.sum((ap_ == ab) & (rp == rb)))
    rec = {"instances": len(insts), "N": args.N, "reps": args.reps,
           "thread_pool_s": {"median": float(np.median(times[False])), "min": min(times[False]), "max": max(times[False])},
           "batched_s": {"median": float(np.median(times[True])), "min": min(times[True]), "max": max(times[True])},
           "ratio_of_medians": float(np.median(times[False]) / np.median(times[True])),
           "status_0": [int(np.sum(sp == 0)), int(np.sum(sb == 0))],
           "accepted_steps_median_max": [float(np.median(ab)), int(np.max(ab))],
           "instances_with_equal_accepted_and_rejected_counts": same,
           "max_abs_state_difference": float(np.max(np.abs(yp - yb)))}
    print(json.dumps(rec), flush=True)
