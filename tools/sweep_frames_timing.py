#!/usr/bin/env python3
"""What t_eval frames cost inside the RK45 sweep: the bench's sweep shape (bench.py --workload sweep_rk45: 4096 instances x 1024 cells,
60 attempts each, the 16 x 16 x 16 parameter grid, the synthetic state) through marl_sweep_rk45_dev and through
marl_sweep_rk45_eval_dev, same build, same process, the variants alternating in every round.

    python tools/sweep_frames_timing.py [--batch 4096] [--n 1024] [--attempts 60] [--rounds 7] [--frames 4 16]

Variants: `plain` (rk45_sweep_kernel); `eval_0` (rk45_sweep_eval_kernel with one sample that no instance reaches: what the sampling
loop costs the ordinary path); `eval_K` (K samples spread evenly over [0, t_min], t_min = the earliest time any instance's budget
reaches, so every instance writes all K).  Each call is timed with a host clock around the (synchronising) entry; per variant the
median and the min..max over the rounds are printed, one JSON line in all.  Expectation to judge against: a frame is one more attempt's
worth of evaluations, time ~ plain x (1 + K / attempts) + the frame writes (K x 40 KB per instance).
Where a run on an MI355X is recorded: profiles/r07_sweep_frames_timing.log, with the figures in DESIGN.md 5.5."""
import argparse
import json
import os
import sys
import time
from dataclasses import asdict

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--attempts", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, nargs="*", default=[4, 16])
    args = ap.parse_args()
    import torch
    from bench import synthetic
    from marlpde_amd.LHeureux_model import LMAHeureuxPorosityDiff
    from marlpde_amd.parameters import Map_Scenario
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU path to time"
    B, N = args.batch, args.n
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
    frames = torch.empty((B, max(args.frames + [1]), 5 * N), dtype=torch.float64, device="cuda")

    def call(t_eval):
        buf = y0.clone()
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = eq.sweep_rk45_device(buf.data_ptr(), (0.0, 1.0e9), 0.5 * dx2, 1e-3, 1e-3, max_attempts=args.attempts, t_eval=t_eval,
                                   y_eval_dev_ptr=None if t_eval is None else frames.data_ptr())
        torch.cuda.synchronize()
        return time.perf_counter() - t, res, buf

    _, res, ref = call(None)                                  # (also the warm-up of the plain kernel)
    t_min = min(r.t_reached for r in res)
    variants = {"plain": None, "eval_0": np.array([2.0 * max(r.t_reached for r in res)])}
    for K in args.frames:
        variants[f"eval_{K}"] = np.linspace(0.0, t_min, K)
    emitted = {}
    for name, te in variants.items():                         # warm-up of every shape, and: sampling changes neither state nor statistics
        _, r, buf = call(te)
        assert torch.equal(buf, ref), name
        assert [(a.n_accepted, a.n_rejected, a.nfev) for a in r] == [(a.n_accepted, a.n_rejected, a.nfev) for a in res], name
        emitted[name] = 0.0 if te is None else float(np.mean([len(a.t) for a in r]))
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, te in variants.items():
            times[name].append(call(te)[0])
    eq.close()
    plain = float(np.median(times["plain"]))
    out = {"batch": B, "N": N, "attempts": args.attempts, "rounds": args.rounds, "t_min_over_dx2": t_min / dx2, "variants": {}}
    for name, ts in times.items():
        med = float(np.median(ts))
        out["variants"][name] = {"median_ms": 1e3 * med, "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts), "frames_per_instance": emitted[name],
                                 "over_plain": med / plain,
                                 "expected_over_plain": 1.0 + emitted[name] / args.attempts,
                                 "cost_per_frame_in_attempts": (med / plain - 1.0) * args.attempts / emitted[name] if emitted[name] else None}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
