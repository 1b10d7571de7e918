#!/usr/bin/env python3
"""What the monitored fixed-step RK4 loop (rk4_watch_kernel, marl_sweep_rk4_watch_dev) costs a step beside the plain sweep
(rk4_sweep_kernel, marl_sweep_rk4_dev): per step the watch kernel adds the monitor partials of the new state, one 8-slot workgroup
reduction and one more barrier to the four evaluations.  A measurement, not a test: no threshold.

    python tools/rk4_watch_timing.py [--rounds 5] [--steps 2000] [--warmup 20] [--out profiles/rk4_watch_timing.log]

  N = 1024 x 4096 instances   the sweep of the benchmark's sweep configuration (bench.py --workload sweep_rk4: the 16 x 16 x 16 grid over Phi0,
                              PhiIni and k3 = k4, the synthetic state, dt = 0.25 dx^2) with the same steps, through the plain entry and
                              through the watch entry three ways: no frames, 10 frames, a terminal limit that is never met (zeros_CC: 1).
  N = 64, N = 200 x 512       the same four routes on the small grids of the tests and of the reference, with dt = 2.5e-6 (there the
                              reactions limit the explicit step: 0.25 dx^2 goes non-finite).
Each route is warmed up, then the routes alternate for --rounds rounds; a call is timed by the host clock around work that ends in a
device synchronise (the watch entry synchronises itself).  Reported: median / min / max ms per call, us per step, and the ratio of
every watch route to the plain one.  The final states of all routes are compared bit for bit first, and the watch results must all have
status 0 after all steps.  One JSON line, printed and appended to --out."""
import argparse
import json
import os
import sys
import time
from dataclasses import asdict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


SMALL_GRID_DT = 2.5e-6   # on coarse grids the reactions limit the explicit step, not diffusion: 0.25 dx^2 goes non-finite there


def bench_instances(B):
    """bench.py's sweep instances (run_sweep, rank 0)"""
    k = max(1, round(B ** (1 / 3)))
    inst = [{"Phi0": float(0.5 + 0.3 * ((i % k) / max(k - 1, 1))), "PhiIni": float(0.5 + 0.3 * (((i // k) % k) / max(k - 1, 1))),
             "k3": float(10 ** (-2 + ((i // (k * k)) % k) / max(k - 1, 1)))} for i in range(B)]
    for d in inst:
        d["PhiNR"] = d["PhiIni"]
        d["k4"] = d["k3"]
    return inst


def synthetic(p, N):
    """bench.py's synthetic input: initial values x (1 + 0.01 sin(2 pi 8 x / L))"""
    L = p["max_depth"] / p["Xstar"]
    x = (np.arange(N) + 0.5) * (L / N)
    y = np.stack([np.full(N, p[k]) for k in ("CAIni", "CCIni", "cCaIni", "cCO3Ini", "PhiIni")])
    return (y * (1.0 + 0.01 * np.sin(2 * np.pi * 8 * x / L))).ravel()


def measure(N, B, steps, warmup, rounds):
    import torch
    from marlpde_amd.LHeureux_model import LMAHeureuxPorosityDiff
    from marlpde_amd.parameters import Map_Scenario
    p = asdict(Map_Scenario()) | {"N": N}
    inst = bench_instances(B)
    eq = LMAHeureuxPorosityDiff.from_scenario(p, device=0, instances=inst)
    eq.use_stream(torch.cuda.current_stream().cuda_stream)
    y0 = torch.from_numpy(np.stack([synthetic(p | d, N) for d in inst])).cuda()
    dt = min(0.25 * (eq.Depths.length / N) ** 2, SMALL_GRID_DT)
    frames = torch.empty((B, 10, 5 * N), dtype=y0.dtype, device=y0.device)
    routes = {"plain": (None, False), "watch": (None, False), "watch_10_frames": (None, True), "watch_limit_never_met": ({"zeros_CC": 1}, False)}

    def call(name, n):
        terminal, with_frames = routes[name]
        eq.set_terminal(terminal)
        buf = y0.clone()
        torch.cuda.synchronize()
        t = time.perf_counter()
        if name == "plain":
            res = None
            eq.sweep_rk4_device(buf.data_ptr(), dt, n)
        elif not with_frames:
            res = eq.sweep_rk4_watch_device(buf.data_ptr(), dt, n)
        else:   # ten frames, the first the initial state, the last the final one
            res = eq.sweep_rk4_watch_device(buf.data_ptr(), dt, n, frame_steps=np.unique(np.linspace(0, n, 10).astype(np.int64)), frames_dev_ptr=frames.data_ptr())
        torch.cuda.synchronize()
        return time.perf_counter() - t, res, buf

    out = {"N": N, "instances": B, "steps": steps, "warmup": warmup, "dt": dt}
    finals = {}
    for name in routes:   # warm-up at the timed shape's kernels, then one full call for the comparison of results
        call(name, warmup)
        _, res, buf = call(name, steps)
        finals[name] = buf.cpu().numpy()
        out[name] = {} if res is None else {"status_0": int(sum(r.status == 0 for r in res)), "steps_done_min": int(min(r.n_accepted for r in res)),
                                            "sign_changes": int(sum(int(np.sum(r.n_events)) for r in res))}
    out["finite"] = bool(np.all(np.isfinite(finals["plain"])))
    out["all_routes_equal_the_plain_sweep_bit_for_bit"] = bool(all(np.array_equal(finals["plain"], v) for v in finals.values()))
    times = {name: [] for name in routes}
    for _ in range(rounds):
        for name in routes:
            times[name].append(call(name, steps)[0])
    eq.set_terminal(None)
    eq.close()
    for name, ts in times.items():
        out[name] |= {"median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts), "us_per_step": 1e6 * float(np.median(ts)) / steps}
    for name in routes:
        if name != "plain":
            out[name]["over_plain"] = out[name]["median_ms"] / out["plain"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rk4_watch_timing.log"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU path to time"
    out = {"tool": "tools/rk4_watch_timing.py", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "runs": [measure(N, B, args.steps, args.warmup, args.rounds) for N, B in ((1024, 4096), (64, 512), (200, 512))]}
    line = json.dumps(out)
    print(line)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
