#!/usr/bin/env python3
"""How far scipy's own DOP853 moves when its right-hand side is perturbed at rounding level - the yardstick for the state bounds of
tests/test_gpu_dop853.py.  CPU only: scipy on the oracle (tests/dop853_ref.py), the sweep shapes of the GPU tests.

    python tools/dop853_noise.py SHAPE SIGMA [SIGMA ...]        e.g.  N513 1e-15 8e-15 3e-13
    python tools/dop853_noise.py grid1025 2.5e-16 1.2e-15        the large-grid t_eval run of tests/test_gpu_dop853_grid.py (class Grid1025)

Every evaluation f(y) is multiplied elementwise by 1 + SIGMA * N(0, 1); four seeds per instance.  Printed per SIGMA: the worst rel_to_max
difference of the t_eval frames and the final state from the unperturbed run, the worst root shift / t1, and how many runs took another
accept / reject sequence (those are left out of the spreads).

Recorded with scipy 1.15.3 (N513; the HIP RHS differs from the oracle's by 3e-15 .. 8e-15 elementwise in the median on this run's states,
3e-13 at the 99th percentile):
    sigma 1e-15:  frames / states 1.66e-09   roots 3.1e-14   no decision changed
    sigma 8e-15:  frames / states 3.12e-09   roots 5.3e-14   no decision changed
    sigma 3e-13:  frames / states 7.64e-08   roots 6.9e-14   no decision changed
The spread sits in the frames at 0.1 t1 and 0.5 t1 (dissolved carbonate near cell 52, where the step controller saw-tooths at the
stability limit); the final states of the same runs agree to 4e-11."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from common import rel_to_max  # noqa: E402
from dop853_ref import scipy_dop853  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from test_gpu_rk23 import Case  # noqa: E402

RTOL, ATOL = 1e-5, 1e-7


class Noisy:
    def __init__(self, sigma, seed):
        self.sigma, self.rng = sigma, np.random.default_rng(seed)

    def rhs(self, P, N, y):
        r = orc.rhs(P, N, y)
        return r * (1.0 + self.sigma * self.rng.standard_normal(r.shape))

    def events(self, P, N, y):
        return orc.events(P, N, y)


class Grid1025:
    """The t_eval run of tests/test_gpu_dop853_grid.py at N = 1025: scenario A, the synthetic state, 40 dx^2, five samples; 8 seeds.

    Recorded with scipy 1.15.3 (the HIP RHS differs from the oracle's on this run's states by 2.3e-16 .. 2.7e-16 elementwise in the
    median, 1.2e-15 at the 99th percentile):
        sigma 2.5e-16:  frames 2.21e-08   final state 5.1e-11   no decision changed
        sigma 1.2e-15:  frames 1.51e-08   final state 3.6e-11   no decision changed
    The spread sits in the frames at 0.5 t1 and 0.77 t1 and does not shrink with sigma: any rounding-level change is amplified alike."""
    seeds = 8

    def __init__(self):
        from common import scenario, synthetic_state
        self.N = 1025
        self.base, self.inst = scenario("A", self.N), [{}]
        dx2 = ((self.base["max_depth"] / self.base["Xstar"]) / self.N) ** 2
        self.t1, self.h0 = 40 * dx2, 0.5 * dx2
        self.t_eval = self.t1 * np.array([0.0, 0.13, 0.5, 0.77, 1.0])
        self.y0 = synthetic_state(self.base, self.N, amplitude=0.05)[None]


def main(name, sigmas):
    c = Grid1025() if name == "grid1025" else Case(name)
    run = lambda o, b: scipy_dop853(o, orc.params_from_dict(c.base | c.inst[b]), c.N, c.y0[b], (0.0, c.t1), c.h0, RTOL, ATOL, t_eval=c.t_eval)  # noqa: E731
    base = [run(orc, b) for b in range(len(c.inst))]
    for sigma in sigmas:
        frames = final = roots = 0.0
        changed = 0
        for seed in range(getattr(c, "seeds", 4)):
            for b, ref in enumerate(base):
                r = run(Noisy(sigma, seed), b)
                if not np.array_equal(r.accepted, ref.accepted):
                    changed += 1
                    continue
                frames = max([frames] + [rel_to_max(r.y_eval[i], ref.y_eval[i]) for i in range(len(c.t_eval))])
                final = max(final, rel_to_max(r.y_final, ref.y_final))
                roots = max([roots] + [abs(a - w) / c.t1 for e in range(7) for a, w in zip(r.t_events[e], ref.t_events[e])])
        print(f"{name} sigma {sigma:.1e}: frames {frames:.2e} final states {final:.2e} roots / t1 {roots:.2e}; runs with other decisions: {changed}", flush=True)


if __name__ == "__main__":
    main(sys.argv[1], [float(s) for s in sys.argv[2:]])
