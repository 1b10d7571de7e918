// marl_rk4_watch.hip - the monitored fixed-step RK4 kernel (marl_rk4_watch.h) as a translation unit of its own: the library's other
// units keep the code generation they had before it existed, and the build runs in parallel.  Same flags as marl_api.hip.
//
// Every symbol of the shared headers lands in its own namespace (marl_rk4w): device code of the units is linked separately (no
// relocatable device code), and the host-side kernel stubs must not collide.  The host driver (marl_api.hip) reaches the kernel
// through the launcher below; structures cross as what they are in memory (Rk4WatchRec: plain data, marl_rk4_watch_ctl.h;
// DevConsts: an opaque device pointer).  The launcher returns the hipGetLastError() of its launch.
#define marl marl_rk4w
#include "marl_rk4_watch.h"
#undef marl

using namespace marl_rk4w;

// blk: 256, 512 or 1024 (anything else: hipErrorInvalidValue, nothing launched); terminal: the seven limits (device) or NULL for none
extern "C" __attribute__((visibility("hidden"))) int marl_rk4_watch_launch(int blk, int vd, unsigned grid, hipStream_t stream, double* Y, const void* consts,
                                                                           void* recs, int64_t N, int64_t nsteps, const int64_t* frame_steps,
                                                                           int64_t n_frames, double* frames, double* t_events, int64_t max_events,
                                                                           const int64_t* terminal)
{
    const DevConsts* c = static_cast<const DevConsts*>(consts);
    Rk4WatchRec* r = static_cast<Rk4WatchRec*>(recs);
#define RK4W_LAUNCH(B)                                                                                                                      \
    if (vd) hipLaunchKernelGGL((rk4_watch_kernel<B, true>), dim3(grid), dim3(B), 0, stream, Y, c, r, N, nsteps, frame_steps, n_frames, frames,  \
                               t_events, max_events, terminal);                                                                                 \
    else hipLaunchKernelGGL((rk4_watch_kernel<B, false>), dim3(grid), dim3(B), 0, stream, Y, c, r, N, nsteps, frame_steps, n_frames, frames,    \
                            t_events, max_events, terminal)
    switch (blk) {
        case 256: RK4W_LAUNCH(256); break;
        case 512: RK4W_LAUNCH(512); break;
        case 1024: RK4W_LAUNCH(1024); break;
        default: return (int)hipErrorInvalidValue;
    }
#undef RK4W_LAUNCH
    return (int)hipGetLastError();
}
