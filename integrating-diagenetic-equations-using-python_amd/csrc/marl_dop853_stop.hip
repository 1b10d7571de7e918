// marl_dop853_stop.hip - the DOP853 sweep that stops at a terminal monitor's root (dop853_sweep_stop_kernel, marl_dop853.h) as a
// translation unit of its own: the code object of marl_dop853.hip keeps the three kernels it had, instruction for instruction, and the
// build runs in parallel.  Same flags as marl_api.hip.
//
// Every symbol of the shared headers lands in its own namespace (marl_dop853_stop), as in marl_dop853.hip: device code of the units is
// linked separately (no relocatable device code), and the host-side kernel stubs must not collide.  The host driver (marl_api.hip)
// reaches the kernel through the launcher below; structures cross as opaque device pointers (Rk45Ctrl, DevConsts), the limits as seven
// host integers.  It returns the hipGetLastError() of its launch.
#define marl marl_dop853_stop
#include "marl_dop853.h"
#undef marl

using namespace marl_dop853_stop;

#define DOP853_STOP_VIS extern "C" __attribute__((visibility("hidden")))

// blk: 256, 512 or 1024 (anything else: hipErrorInvalidValue, nothing launched); karena: marl_dop853_arena_doubles(grid, blk) doubles;
// terminal: marl_set_terminal's seven limits (host).  t_events may be NULL with max_events = 0, t_eval / Yeval with n_eval = 0.
DOP853_STOP_VIS int marl_dop853_stop_launch(int blk, int vd, unsigned grid, hipStream_t stream, double* Y, const void* consts, void* ctrls, int64_t N,
                                            double* karena, const double* t_eval, int64_t n_eval, double* Yeval, int64_t* n_done,
                                            double* t_events, int64_t max_events, const int64_t* terminal)
{
    if (!terminal || !karena || !n_done || N < 1 || N > blk || n_eval < 0 || max_events < 0 || (n_eval > 0 && (!t_eval || !Yeval)) ||
        (max_events > 0 && !t_events))
        return (int)hipErrorInvalidValue;
    const DevConsts* c = static_cast<const DevConsts*>(consts);
    Rk45Ctrl* k = static_cast<Rk45Ctrl*>(ctrls);
    TermLimits lim = {};
    for (int e = 0; e < 7; e++) lim.k[e] = terminal[e];
    const dim3 g(grid);
#define DOP853_STOP_SWEEP(B)                                                                                                           \
    if (vd) hipLaunchKernelGGL((dop853_sweep_stop_kernel<B, true>), g, dim3(B), 0, stream, Y, c, k, N, karena, t_eval, n_eval, Yeval,  \
                               n_done, t_events, max_events, lim);                                                                     \
    else hipLaunchKernelGGL((dop853_sweep_stop_kernel<B, false>), g, dim3(B), 0, stream, Y, c, k, N, karena, t_eval, n_eval, Yeval,    \
                            n_done, t_events, max_events, lim)
    switch (blk) {
        case 256: DOP853_STOP_SWEEP(256); break;
        case 512: DOP853_STOP_SWEEP(512); break;
        case 1024: DOP853_STOP_SWEEP(1024); break;
        default: return (int)hipErrorInvalidValue;
    }
#undef DOP853_STOP_SWEEP
    return (int)hipGetLastError();
}
