"""BDF sweeps, thread pool of single runs against the batched kernels (needs a GPU):
    python3 tools/bdf_sweep_ab.py [--sizes 64 512] [--reps 5] [--t-eval K] [--events] [--only batched|pool]

run_sweep_bdf on one GPU over product_grid(Phi0, k3 = k4) at N = 200, t_span (0, 1), first step 1e-6, rtol = atol = 1e-3: once with
the thread pool (concurrent marl_integrate_bdf runs, at its own limit of 16 workers) and once with batched=True (marl_sweep_bdf_dev).
One warm-up each, then alternating repetitions in one process; medians and spread per size, and how far the two agree.
--t-eval K: both paths also return the time series at K uniform samples over t_span (marl_sweep_bdf_eval_dev against the single runs'
t_eval); the record then carries the frames' agreement too.  --events: both paths also return the monitors' root times (at most 64
each; marl_sweep_bdf_events_dev against the single runs' t_events); the record then carries the roots located per instance by the
batched path - every searched step locates at least one root and costs its instance one more cycle, so this bounds the added cycles
per instance from above - and, with both paths, how far the roots agree.  --only: time one of the two paths alone (no comparison)."""
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
ap.add_argument("--t-eval", type=int, default=0, dest="t_eval", help="K uniform samples over t_span (0: none)")
ap.add_argument("--events", action="store_true", help="locate the monitors' root times too")
ap.add_argument("--only", choices=["batched", "pool"], default=None)
args = ap.parse_args()

base = asdict(Map_Scenario()) | {"N": args.N}
ARGS = ((0.0, 1.0), 1e-6, 1e-3, 1e-3)
more = {"t_eval": np.linspace(ARGS[0][0], ARGS[0][1], args.t_eval)} if args.t_eval > 0 else {}
if args.events:
    more |= {"events": True}
paths = {None: (False, True), "batched": (True,), "pool": (False,)}[args.only]
for B in args.sizes:
    nk = 8 if B <= 64 else 16
    insts = product_grid(Phi0=np.linspace(0.5, 0.7, B // nk), k3=np.logspace(-2, -1, nk))
    for d in insts:
        d.update(PhiIni=d["Phi0"], PhiNR=d["Phi0"], k4=d["k3"])
    y0 = initial_states(base, insts)
    times = {False: [], True: []}
    out = {}
    for rep in range(-1, args.reps):   # -1: warm-up (module load, allocations)
        for batched in paths:
            t0 = time.perf_counter()
            out[batched] = run_sweep_bdf(base, insts, *ARGS, y0=y0, device=0, batched=batched, **more)
            if rep >= 0:
                times[batched].append(time.perf_counter() - t0)
    rec = {"instances": len(insts), "N": args.N, "reps": args.reps, "t_eval": args.t_eval, "events": args.events}
    roots = {k: v[-1] for k, v in out.items()} if args.events else {}
    if args.events:
        out = {k: v[:-1] for k, v in out.items()}
        if True in roots:
            per = [sum(len(t) for t in r) for r in roots[True]]
            rec["roots_per_instance_median_max_total"] = [float(np.median(per)), int(np.max(per)), int(np.sum(per))]
    for batched, name in ((False, "thread_pool_s"), (True, "batched_s")):
        if batched in paths:
            rec[name] = {"median": float(np.median(times[batched])), "min": min(times[batched]), "max": max(times[batched])}
            rec["status_0_" + name[:-2]] = int(np.sum(out[batched][1] == 0))
    if args.only is None:
        (yp, sp, ap_, rp, tp, *fp), (yb, sb, ab, rb, tb, *fb) = out[False], out[True]
        rec |= {"ratio_of_medians": float(np.median(times[False]) / np.median(times[True])),
                "accepted_steps_median_max": [float(np.median(ab)), int(np.max(ab))],
                "instances_with_equal_accepted_and_rejected_counts": int(np.sum((ap_ == ab) & (rp == rb))),
                "max_abs_state_difference": float(np.max(np.abs(yp - yb)))}
        if args.events:
            same = [all(len(a) == len(b) for a, b in zip(p_, b_)) for p_, b_ in zip(roots[False], roots[True])]
            rec |= {"instances_with_equal_root_counts": int(np.sum(same)),
                    "max_abs_root_difference": max([float(np.max(np.abs(a - b))) for p_, b_, ok in zip(roots[False], roots[True], same) if ok
                                                    for a, b in zip(p_, b_) if len(a)], default=0.0)}
        if args.t_eval > 0:
            rec |= {"instances_with_equal_frame_counts": int(np.sum(fp[0] == fb[0])),
                    "max_abs_frame_difference": float(np.nanmax(np.abs(fp[1] - fb[1])))}
    print(json.dumps(rec), flush=True)
