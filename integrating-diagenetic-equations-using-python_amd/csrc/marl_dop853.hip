// marl_dop853.hip - the DOP853 kernels (marl_dop853.h) as a translation unit of their own: the library's other units keep the code
// generation they had before DOP853 existed, and the build runs in parallel.  Same flags as marl_api.hip.
//
// Every symbol of the shared headers lands in its own namespace (marl_dop853): device code of the units is linked separately (no
// relocatable device code), and the host-side kernel stubs must not collide.  The host driver (marl_api.hip) reaches the kernels
// through the launcher below; structures cross as opaque device pointers (Rk45Ctrl, DevConsts).  It returns the hipGetLastError() of
// its launch.
#define marl marl_dop853
#include "marl_dop853.h"
#undef marl

using namespace marl_dop853;

#define DOP853_VIS extern "C" __attribute__((visibility("hidden")))

namespace {
// the kernel of the sweep family's `kind` (the numbers of marl_rk23_launch_sweep): 0 plain, 2 eval, 3 roots
template <int BLK, bool VD>
void launch_sweep_t(int kind, unsigned grid, hipStream_t stream, double* Y, const DevConsts* consts, Rk45Ctrl* ctrls, int64_t N, double* karena,
                    const double* t_eval, int64_t n_eval, double* Yeval, int64_t* n_done, double* t_events, int64_t max_events)
{
    const dim3 g(grid), b(BLK);
    switch (kind) {
        case 0: hipLaunchKernelGGL((dop853_sweep_kernel<BLK, VD>), g, b, 0, stream, Y, consts, ctrls, N, karena); break;
        case 2: hipLaunchKernelGGL((dop853_sweep_eval_kernel<BLK, VD>), g, b, 0, stream, Y, consts, ctrls, N, karena, t_eval, n_eval, Yeval, n_done); break;
        default: hipLaunchKernelGGL((dop853_sweep_roots_kernel<BLK, VD>), g, b, 0, stream, Y, consts, ctrls, N, karena, t_eval, n_eval, Yeval, n_done,
                                    t_events, max_events); break;
    }
}
}  // namespace

// doubles of the stage-derivative arena `karena` for `grid` instances at window `blk`
DOP853_VIS int64_t marl_dop853_arena_doubles(int64_t grid, int blk) { return dop853_arena_doubles(grid, blk); }

// blk: 256, 512 or 1024; kind: 0, 2 or 3 (anything else: hipErrorInvalidValue, nothing launched).  There is no pausing kernel (kind 1)
// and kind 4 is refused here: single runs go through kind 3 with one instance, and the kernel that stops at a terminal monitor's root
// lives in marl_dop853_stop.hip behind a launcher of its own.
DOP853_VIS int marl_dop853_launch_sweep(int kind, int blk, int vd, unsigned grid, hipStream_t stream, double* Y, const void* consts, void* ctrls,
                                        int64_t N, double* karena, const double* t_eval, int64_t n_eval, double* Yeval, int64_t* n_done,
                                        double* t_events, int64_t max_events)
{
    if ((kind != 0 && kind != 2 && kind != 3) || !karena || N < 1 || N > blk) return (int)hipErrorInvalidValue;
    const DevConsts* c = static_cast<const DevConsts*>(consts);
    Rk45Ctrl* k = static_cast<Rk45Ctrl*>(ctrls);
#define DOP853_SWEEP(B)                                                                                                                \
    if (vd) launch_sweep_t<B, true>(kind, grid, stream, Y, c, k, N, karena, t_eval, n_eval, Yeval, n_done, t_events, max_events);       \
    else launch_sweep_t<B, false>(kind, grid, stream, Y, c, k, N, karena, t_eval, n_eval, Yeval, n_done, t_events, max_events)
    switch (blk) {
        case 256: DOP853_SWEEP(256); break;
        case 512: DOP853_SWEEP(512); break;
        case 1024: DOP853_SWEEP(1024); break;
        default: return (int)hipErrorInvalidValue;
    }
#undef DOP853_SWEEP
    return (int)hipGetLastError();
}
