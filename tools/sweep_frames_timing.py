#!/usr/bin/env python3
"""What t_eval frames cost inside the RK45 sweep: the bench's sweep shape (bench.py --workload sweep_rk45: 4096 instances x 1024 cells,
60 attempts each, the 16 x 16 x 16 parameter grid, the synthetic state) through marl_sweep_rk45_dev and through
marl_sweep_rk45_eval_dev, same build, same process, the variants alternating in every round.

    python tools/sweep_frames_timing.py [--batch 4096] [--n 1024] [--attempts 60] [--rounds 7] [--frames 4 16] [--roots]

Variants: `plain` (rk45_sweep_kernel); `eval_0` (rk45_sweep_eval_kernel with one sample that no instance reaches: what the sampling
loop costs the ordinary path); `eval_K` (K samples spread evenly over [0, t_min], t_min = the earliest time any instance's budget
reaches, so every instance writes all K).  Each call is timed with a host clock around the (synchronising) entry; per variant the
median and the min..max over the rounds are printed, one JSON line in all.  Expectation to judge against: a frame is one more attempt's
worth of evaluations, time ~ plain x (1 + K / attempts) + the frame writes (K x 40 KB per instance).
`--roots` adds `roots_0`: eval_0 through marl_sweep_rk45_events_dev (rk45_sweep_roots_kernel) - one more barrier per accepted step, and one
replay per Brent function evaluation where a monitor changes sign; `roots_located` says how many roots the batch located (0: the barrier alone).
The mirror builds seven arrays per instance around that call, so `--roots` also times the two C entries themselves (`eval_0_c`, `roots_0_c`:
ctypes calls with preallocated arguments) - the pair to compare the kernels by.
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
    ap.add_argument("--roots", action="store_true")
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

    def call(t_eval, roots=False):
        buf = y0.clone()
        torch.cuda.synchronize()
        t = time.perf_counter()
        more = {"events": True, "max_events": 1} if roots else {}   # (one slot per monitor: the root buffer's copy to the host stays small)
        res = eq.sweep_rk45_device(buf.data_ptr(), (0.0, 1.0e9), 0.5 * dx2, 1e-3, 1e-3, max_attempts=args.attempts, t_eval=t_eval,
                                   y_eval_dev_ptr=None if t_eval is None else frames.data_ptr(), **more)
        torch.cuda.synchronize()
        return time.perf_counter() - t, res, buf

    def call_c(roots):                                        # the C entry alone: no result objects
        import ctypes as C
        from marlpde_amd._abi import MarlStats
        buf = y0.clone()
        te = variants["eval_0"]
        stats, n_done, tev = (MarlStats * B)(), np.zeros(B, dtype=np.int64), np.empty((B, 7, 1))
        args = (eq._ctx, C.c_void_p(buf.data_ptr()), 0.0, 1.0e9, 0.5 * dx2, 1e-3, 1e-3, args_attempts, te.ctypes.data_as(C.c_void_p), te.size,
                C.c_void_p(frames.data_ptr()), n_done.ctypes.data_as(C.c_void_p))
        torch.cuda.synchronize()
        t = time.perf_counter()
        if roots:
            rc = eq._lib.marl_sweep_rk45_events_dev(*args, tev.ctypes.data_as(C.c_void_p), 1, stats)
        else:
            rc = eq._lib.marl_sweep_rk45_eval_dev(*args, stats)
        torch.cuda.synchronize()
        assert rc == 0
        return time.perf_counter() - t, [], buf

    args_attempts = args.attempts
    _, res, ref = call(None)                                  # (also the warm-up of the plain kernel)
    t_min = min(r.t_reached for r in res)
    variants = {"plain": None, "eval_0": np.array([2.0 * max(r.t_reached for r in res)])}
    for K in args.frames:
        variants[f"eval_{K}"] = np.linspace(0.0, t_min, K)
    if args.roots:
        variants["roots_0"] = variants["eval_0"]
        variants["eval_0_c"] = variants["roots_0_c"] = variants["eval_0"]

    def run(name, te):
        return call_c(name == "roots_0_c") if name.endswith("_c") else call(te, name == "roots_0")

    emitted, located = {}, None
    for name, te in variants.items():                         # warm-up of every shape, and: sampling changes neither state nor statistics
        _, r, buf = run(name, te)
        if name == "roots_0":
            located = int(sum(len(t) for a in r for t in a.t_events))
        assert torch.equal(buf, ref), name
        if not name.endswith("_c"):
            assert [(a.n_accepted, a.n_rejected, a.nfev) for a in r] == [(a.n_accepted, a.n_rejected, a.nfev) for a in res], name
        emitted[name] = 0.0 if te is None or name.endswith("_c") else float(np.mean([len(a.t) for a in r]))
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, te in variants.items():
            times[name].append(run(name, te)[0])
    eq.close()
    plain = float(np.median(times["plain"]))
    out = {"batch": B, "N": N, "attempts": args.attempts, "rounds": args.rounds, "t_min_over_dx2": t_min / dx2, "roots_located": located,
           "variants": {}}
    for name, ts in times.items():
        med = float(np.median(ts))
        out["variants"][name] = {"median_ms": 1e3 * med, "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts), "frames_per_instance": emitted[name],
                                 "over_plain": med / plain,
                                 "expected_over_plain": 1.0 + emitted[name] / args.attempts,
                                 "cost_per_frame_in_attempts": (med / plain - 1.0) * args.attempts / emitted[name] if emitted[name] else None}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
