#!/usr/bin/env python3
"""What a terminal monitor saves in a Radau sweep, or with --method bdf in a batched BDF sweep (marl_set_terminal): the 512-instance Phi0 x PhiIni sweep of tools/rk23_timing.py and
DESIGN.md section 8 (16 x 32 values in 0.5 .. 0.8, PhiNR = PhiIni) at N = 200, uniform initial state, rtol = atol = 1e-3, first_step
1e-6, to t1 = 1 through marl_sweep_radau_dev (bdf: marl_sweep_bdf_dev / marl_sweep_bdf_terminal_dev) - once without limits and once with `ones_Phi: 1`, the reference's own example of "stop
here" (marlpde/LHeureux_model.py:113-122), same build, same process, the two alternating in every round; medians over the rounds.
--method rk45 / rk23: the explicit sweeps with the roots located (sweep_rk45_device(events=True, max_events=64): marl_sweep_rk45_events_dev
without limits, marl_sweep_rk45_terminal_dev with), and a third setting, `zeros_CC: 1`, a limit that is never met: the whole sweep through
the *_term_kernel on the steps of the sweep without limits - what the flag costs.
A measurement, not a test: there is no threshold.

    python tools/terminal_timing.py [--method radau|bdf|rk45|rk23] [--rounds 7] [--t1 1.0]

Per setting: wall time (a host clock around the synchronising entry, the state copy excluded), RHS evaluations summed over the
instances, instances per status.  One JSON line.  Where a run on an MI355X is recorded: profiles/terminal_timing.log (Radau) and
profiles/bdf_terminal_timing.log (BDF), with the figures in DESIGN.md section 8; profiles/rk_terminal_timing.log (RK45, RK23), section 4."""
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
    ap.add_argument("--method", choices=("radau", "bdf", "rk45", "rk23"), default="radau")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--t1", type=float, default=1.0)
    args = ap.parse_args()
    import torch
    from marlpde_amd.LHeureux_model import LMAHeureuxPorosityDiff
    from marlpde_amd.parameters import Map_Scenario
    from marlpde_amd.sweep import initial_states, product_grid
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU path to time"
    N = 200
    p = asdict(Map_Scenario()) | {"N": N}
    inst = product_grid(Phi0=np.linspace(0.5, 0.8, 16), PhiIni=np.linspace(0.5, 0.8, 32))
    for d in inst:
        d["PhiNR"] = d["PhiIni"]
    eq = LMAHeureuxPorosityDiff.from_scenario(p, device=0, instances=inst)
    eq.use_stream(torch.cuda.current_stream().cuda_stream)
    y0 = torch.from_numpy(initial_states(p, inst)).cuda()
    settings = {"no_limits": None, "ones_Phi_1": {"ones_Phi": 1}}
    explicit = args.method in ("rk45", "rk23")
    more = {"events": True, "max_events": 64} if explicit else {}
    if explicit:
        settings["never_met"] = {"zeros_CC": 1}

    def call(name):
        eq.set_terminal(settings[name])
        buf = y0.clone()
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = getattr(eq, f"sweep_{args.method}_device")(buf.data_ptr(), (0.0, args.t1), 1e-6, 1e-3, 1e-3, **more)
        torch.cuda.synchronize()
        return time.perf_counter() - t, res

    out = {"method": args.method, "instances": len(inst), "N": N, "t1": args.t1, "rtol": 1e-3, "atol": 1e-3, "first_step": 1e-6, "rounds": args.rounds}
    times = {name: [] for name in settings}
    for name in settings:                                      # warm-up, and the counts (the runs are deterministic)
        _, res = call(name)
        out[name] = {"nfev": int(sum(r.nfev for r in res)), "nfev_max": int(max(r.nfev for r in res)),
                     "attempts": int(sum(r.n_accepted + r.n_rejected for r in res)),
                     "status_counts": {str(s): int(sum(r.status == s for r in res)) for s in sorted({r.status for r in res})}}
    for _ in range(args.rounds):
        for name in settings:
            times[name].append(call(name)[0])
    for name, ts in times.items():
        out[name] |= {"median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts)}
    out["time_ratio"] = out["no_limits"]["median_ms"] / out["ones_Phi_1"]["median_ms"]
    out["nfev_ratio"] = out["no_limits"]["nfev"] / out["ones_Phi_1"]["nfev"]
    if explicit:
        out["never_met_over_no_limits"] = out["never_met"]["median_ms"] / out["no_limits"]["median_ms"]
    eq.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
