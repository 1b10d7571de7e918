// Brent's method, the only one in the project: scipy.optimize.brentq as solve_event_equation calls it (scipy/integrate/_ivp/ivp.py:51-76:
// xtol = rtol = 4 eps, at most 100 iterations).  brent_advance is one pass of the loop, for callers that cannot call a function in the
// middle of it - the device-side controllers of the sweeps (marl_radau_batch.h, rk45_sweep_roots_kernel in marl_kernels.h); brent_root
// is the loop around it for the host drivers of the single runs (marl_api.hip).  Nothing but <math.h>: a host C++ compiler builds this
// header alone (tests/test_brent_cpu.py pins it to scipy's roots and call counts that way); under hipcc it follows <hip/hip_runtime.h>,
// which defines __forceinline__.
#pragma once
#include <math.h>

#ifdef __HIPCC__
#define MARL_BRENT_FN __host__ __device__ __forceinline__
#else
#define MARL_BRENT_FN inline
#endif

namespace marl {

// One pass of Brent's method from the top of its loop to the next function evaluation.  Returns true when the root is final (c.xcur);
// false: evaluate at c.xcur.  BS: any structure with the fields below - the Radau sweeps' controller (RadauCtl), BrentState.
struct BrentState { double xpre, xcur, xblk, fpre, fcur, fblk, spre, scur; };
template <class BS>
MARL_BRENT_FN bool brent_advance(BS& c)
{
    const double xtol = 4 * 2.220446049250313e-16, rtol = xtol;
    if (c.fpre != 0 && c.fcur != 0 && ((c.fpre < 0) != (c.fcur < 0))) { c.xblk = c.xpre; c.fblk = c.fpre; c.spre = c.scur = c.xcur - c.xpre; }
    if (fabs(c.fblk) < fabs(c.fcur)) { c.xpre = c.xcur; c.xcur = c.xblk; c.xblk = c.xpre; c.fpre = c.fcur; c.fcur = c.fblk; c.fblk = c.fpre; }
    const double delta = (xtol + rtol * fabs(c.xcur)) / 2, sbis = (c.xblk - c.xcur) / 2;
    if (c.fcur == 0 || fabs(sbis) < delta) return true;
    if (fabs(c.spre) > delta && fabs(c.fcur) < fabs(c.fpre)) {
        double stry;
        if (c.xpre == c.xblk) stry = -c.fcur * (c.xcur - c.xpre) / (c.fcur - c.fpre);
        else {
            const double dpre = (c.fpre - c.fcur) / (c.xpre - c.xcur), dblk = (c.fblk - c.fcur) / (c.xblk - c.xcur);
            stry = -c.fcur * (c.fblk * dblk - c.fpre * dpre) / (dblk * dpre * (c.fblk - c.fpre));
        }
        const double lim = fmin(fabs(c.spre), 3 * fabs(sbis) - delta);
        if (2 * fabs(stry) < lim) { c.spre = c.scur; c.scur = stry; }
        else { c.spre = sbis; c.scur = sbis; }
    } else { c.spre = sbis; c.scur = sbis; }
    c.xpre = c.xcur; c.fpre = c.fcur;
    if (fabs(c.scur) > delta) c.xcur += c.scur; else c.xcur += (sbis > 0 ? delta : -delta);
    return false;
}

// The root of f in [a, b] given fa = f(a), fb = f(b) of opposite signs (host).  f(x, &fx) returns non-zero on failure, which is
// returned as it is; otherwise 0 and *root - an end point whose value is zero, else the last iterate.
template <class F>
int brent_root(F&& f, double a, double fa, double b, double fb, double* root)
{
    if (fa == 0) { *root = a; return 0; }
    if (fb == 0) { *root = b; return 0; }
    BrentState s = {a, b, 0, fa, fb, 0, 0, 0};
    for (int it = 0; it < 100; it++) {
        if (brent_advance(s)) break;
        if (int rc = f(s.xcur, &s.fcur)) return rc;
    }
    *root = s.xcur;
    return 0;
}

}  // namespace marl
