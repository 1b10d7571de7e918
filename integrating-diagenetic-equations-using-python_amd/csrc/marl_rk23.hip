// marl_rk23.hip - the RK23 kernels (marl_rk23.h) as a translation unit of their own: the library's other units keep the code
// generation they had before RK23 existed, and the build runs in parallel.  Same flags as marl_api.hip.
//
// Every symbol of the shared headers lands in its own namespace (marl_rk23): device code of the units is linked separately (no
// relocatable device code), and the host-side kernel stubs must not collide.  The host drivers (marl_api.hip) reach the kernels
// through the launchers below; structures cross as what they are in memory (Slab: five int64, DenseWeights: seven doubles,
// Rk45Ctrl / DevConsts: opaque device pointers).  Every launcher returns the hipGetLastError() of its launch.
#define marl marl_rk23
#include "marl_rk23.h"
#undef marl

using namespace marl_rk23;

#define RK23_VIS extern "C" __attribute__((visibility("hidden")))

namespace {
// the kernel of the rk45_sweep_* family's `kind`: 0 plain, 1 events (pausing loop), 2 eval, 3 roots, 4 roots with terminal monitors (`lim`)
template <int BLK, bool VD>
void launch_sweep_t(int kind, unsigned grid, hipStream_t stream, double* Y, const DevConsts* consts, Rk45Ctrl* ctrls, int64_t N, double* Yold,
                    double* Fold, const double* t_eval, int64_t n_eval, double* Yeval, int64_t* n_done, double* t_events, int64_t max_events,
                    const TermLimits& lim)
{
    const dim3 g(grid), b(BLK);
    switch (kind) {
        case 0: hipLaunchKernelGGL((rk23_sweep_kernel<BLK, VD>), g, b, 0, stream, Y, consts, ctrls, N, Yold, Fold); break;
        case 1: hipLaunchKernelGGL((rk23_sweep_events_kernel<BLK, VD>), g, b, 0, stream, Y, consts, ctrls, N, Yold, Fold); break;
        case 2: hipLaunchKernelGGL((rk23_sweep_eval_kernel<BLK, VD>), g, b, 0, stream, Y, consts, ctrls, N, t_eval, n_eval, Yeval, n_done); break;
        case 3: hipLaunchKernelGGL((rk23_sweep_roots_kernel<BLK, VD>), g, b, 0, stream, Y, consts, ctrls, N, t_eval, n_eval, Yeval, n_done,
                                   t_events, max_events); break;
        default: hipLaunchKernelGGL((rk23_sweep_term_kernel<BLK, VD>), g, b, 0, stream, Y, consts, ctrls, N, t_eval, n_eval, Yeval, n_done,
                                    t_events, max_events, lim); break;
    }
}
}  // namespace

// blk: 256, 512 or 1024 (anything else: hipErrorInvalidValue, nothing launched); terminal: the seven limits of kind 4 (host; else NULL)
RK23_VIS int marl_rk23_launch_sweep(int kind, int blk, int vd, unsigned grid, hipStream_t stream, double* Y, const void* consts, void* ctrls,
                                    int64_t N, double* Yold, double* Fold, const double* t_eval, int64_t n_eval, double* Yeval, int64_t* n_done,
                                    double* t_events, int64_t max_events, const int64_t* terminal)
{
    if ((kind == 4) != (terminal != nullptr) || kind < 0 || kind > 4) return (int)hipErrorInvalidValue;
    TermLimits lim = {};
    for (int e = 0; terminal && e < 7; e++) lim.k[e] = terminal[e];
    const DevConsts* c = static_cast<const DevConsts*>(consts);
    Rk45Ctrl* k = static_cast<Rk45Ctrl*>(ctrls);
#define RK23_SWEEP(B)                                                                                                                   \
    if (vd) launch_sweep_t<B, true>(kind, grid, stream, Y, c, k, N, Yold, Fold, t_eval, n_eval, Yeval, n_done, t_events, max_events, lim);  \
    else launch_sweep_t<B, false>(kind, grid, stream, Y, c, k, N, Yold, Fold, t_eval, n_eval, Yeval, n_done, t_events, max_events, lim)
    switch (blk) {
        case 256: RK23_SWEEP(256); break;
        case 512: RK23_SWEEP(512); break;
        case 1024: RK23_SWEEP(1024); break;
        default: return (int)hipErrorInvalidValue;
    }
#undef RK23_SWEEP
    return (int)hipGetLastError();
}

RK23_VIS int marl_rk23_launch_attempt(int tiled, int vd, unsigned nb, hipStream_t stream, double* Y0, double* Y1, double* F0, double* F1,
                                      const void* consts, const int64_t slab5[5], const void* ctrl, double* part)
{
    const Slab S{slab5[0], slab5[1], slab5[2], slab5[3], slab5[4]};
    const DevConsts* c = static_cast<const DevConsts*>(consts);
    const Rk45Ctrl* k = static_cast<const Rk45Ctrl*>(ctrl);
    const dim3 g(nb), b(256);
    if (tiled) {
        if (vd) hipLaunchKernelGGL((rk23_attempt_kernel<256, LAYOUT_TILED, true>), g, b, 0, stream, Y0, Y1, F0, F1, c, S, k, part);
        else hipLaunchKernelGGL((rk23_attempt_kernel<256, LAYOUT_TILED, false>), g, b, 0, stream, Y0, Y1, F0, F1, c, S, k, part);
    } else {
        if (vd) hipLaunchKernelGGL((rk23_attempt_kernel<256, LAYOUT_FIELD_MAJOR, true>), g, b, 0, stream, Y0, Y1, F0, F1, c, S, k, part);
        else hipLaunchKernelGGL((rk23_attempt_kernel<256, LAYOUT_FIELD_MAJOR, false>), g, b, 0, stream, Y0, Y1, F0, F1, c, S, k, part);
    }
    return (int)hipGetLastError();
}

RK23_VIS int marl_rk23_launch_control(hipStream_t stream, const double* recs, int64_t nrec, void* ctrl)
{
    hipLaunchKernelGGL(rk23_control_kernel, dim3(1), dim3(CONTROL_THREADS), 0, stream, recs, nrec, static_cast<Rk45Ctrl*>(ctrl));
    return (int)hipGetLastError();
}

RK23_VIS int marl_rk23_launch_dense(int tiled, int vd, unsigned nb, hipStream_t stream, const double* yold, const double* fold, const void* consts,
                                    const int64_t slab5[5], double h, const double w[7], double* yout, double* part)
{
    const Slab S{slab5[0], slab5[1], slab5[2], slab5[3], slab5[4]};
    const DevConsts* c = static_cast<const DevConsts*>(consts);
    DenseWeights dw;
    for (int j = 0; j < 7; j++) dw.w[j] = w[j];
    const dim3 g(nb), b(256);
    if (tiled) {
        if (vd) hipLaunchKernelGGL((rk23_dense_kernel<256, LAYOUT_TILED, true>), g, b, 0, stream, yold, fold, c, S, h, dw, yout, part);
        else hipLaunchKernelGGL((rk23_dense_kernel<256, LAYOUT_TILED, false>), g, b, 0, stream, yold, fold, c, S, h, dw, yout, part);
    } else {
        if (vd) hipLaunchKernelGGL((rk23_dense_kernel<256, LAYOUT_FIELD_MAJOR, true>), g, b, 0, stream, yold, fold, c, S, h, dw, yout, part);
        else hipLaunchKernelGGL((rk23_dense_kernel<256, LAYOUT_FIELD_MAJOR, false>), g, b, 0, stream, yold, fold, c, S, h, dw, yout, part);
    }
    return (int)hipGetLastError();
}
