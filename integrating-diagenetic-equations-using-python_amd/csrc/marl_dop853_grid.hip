// marl_dop853_grid.hip - the large-grid DOP853 kernels (marl_dop853_grid.h) as a translation unit of their own: the library's other
// units, marl_dop853.hip and marl_dop853_stop.hip among them, keep the code objects they had, and the build runs in parallel.  Same
// flags as marl_api.hip.
//
// Every symbol of the shared headers lands in its own namespace (marl_dop853_grid): device code of the units is linked separately (no
// relocatable device code), and the host-side kernel stubs must not collide.  The host driver (marl_api.hip) reaches the kernels
// through the launchers below; structures cross as what they are in memory (Slab: five int64; Rk45Ctrl / DevConsts: opaque device
// pointers), the dense output's abscissa as a double - its 16 weights and the layout of the record buffer are made here, so the
// driver's unit includes nothing of DOP853.  Every launcher returns the hipGetLastError() of its launch.
#define marl marl_dop853_grid
#include "marl_dop853_grid.h"
#undef marl

using namespace marl_dop853_grid;

#define DOP853_GRID_VIS extern "C" __attribute__((visibility("hidden")))

// doubles of the record buffer `part` of a grid of nb windows (dop853_grid_parts)
DOP853_GRID_VIS int64_t marl_dop853_grid_part_doubles(int64_t nb) { return dop853_grid_parts(nb).total; }

// One stage of an attempt (s = 1..12), K_1 of the first step (s = 0), or an extra stage of the step just accepted (s = 13..15, with
// replay).  nb: windows of 254 written cells.  part: the record buffer (row 12 writes its records and second sums there).
DOP853_GRID_VIS int marl_dop853_grid_launch_stage(int tiled, int vd, unsigned nb, hipStream_t stream, double* Y0, double* Y1, double* karena,
                                                  int64_t kstride, const void* consts, const int64_t slab5[5], const void* ctrl, int s, int replay,
                                                  double* part)
{
    if (s < 0 || s >= DOP853_GRID_SLOTS || (s > dop853::N_STAGES && !replay) || !karena || !part || nb == 0) return (int)hipErrorInvalidValue;
    const Dop853GridParts pp = dop853_grid_parts(nb);
    double* part3 = part + pp.sum3;
    part += pp.rec;
    const Slab S{slab5[0], slab5[1], slab5[2], slab5[3], slab5[4]};
    const DevConsts* c = static_cast<const DevConsts*>(consts);
    const Rk45Ctrl* k = static_cast<const Rk45Ctrl*>(ctrl);
    const dim3 g(nb), b(DOP853_GRID_BLK);
    if (tiled) {
        if (vd) hipLaunchKernelGGL((dop853_grid_stage_kernel<LAYOUT_TILED, true>), g, b, 0, stream, Y0, Y1, karena, kstride, c, S, k, s, replay, part, part3);
        else hipLaunchKernelGGL((dop853_grid_stage_kernel<LAYOUT_TILED, false>), g, b, 0, stream, Y0, Y1, karena, kstride, c, S, k, s, replay, part, part3);
    } else {
        if (vd) hipLaunchKernelGGL((dop853_grid_stage_kernel<LAYOUT_FIELD_MAJOR, true>), g, b, 0, stream, Y0, Y1, karena, kstride, c, S, k, s, replay, part, part3);
        else hipLaunchKernelGGL((dop853_grid_stage_kernel<LAYOUT_FIELD_MAJOR, false>), g, b, 0, stream, Y0, Y1, karena, kstride, c, S, k, s, replay, part, part3);
    }
    return (int)hipGetLastError();
}

// The reduction of an attempt's `nb` records (buffer layout: dop853_grid_parts) and its decision.
DOP853_GRID_VIS int marl_dop853_grid_launch_control(hipStream_t stream, double* part, int64_t nb, void* ctrl)
{
    if (!part || nb < 1) return (int)hipErrorInvalidValue;
    const Dop853GridParts p = dop853_grid_parts(nb);
    const double* recs = part + p.rec;
    const double* sums3 = part + p.sum3;
    int64_t chunk = 1, nrec = nb;
    if (dop853_grid_first_level(nb, &chunk, &nrec)) {
        hipLaunchKernelGGL(dop853_grid_reduce_kernel, dim3((unsigned)nrec), dim3(256), 0, stream, recs, sums3, nb, chunk, part + p.rec1, part + p.sum3_1);
        if (const hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
        recs = part + p.rec1;
        sums3 = part + p.sum3_1;
    }
    hipLaunchKernelGGL(dop853_grid_control_kernel, dim3(1), dim3(CONTROL_THREADS), 0, stream, recs, sums3, nrec, static_cast<Rk45Ctrl*>(ctrl));
    return (int)hipGetLastError();
}

// Dense output of the accepted step [t_old, t_old + h] that starts at `yold` (slots of `frame`), at t_old + x h (at_start: x = 0, the
// result is y_old).  nb: workgroups of 256 cells.  yout, part: may be NULL.
DOP853_GRID_VIS int marl_dop853_grid_launch_dense(int tiled, unsigned nb, hipStream_t stream, const double* yold, const double* karena, int64_t kstride,
                                                  int frame, const void* consts, const int64_t slab5[5], double h, double x, int at_start,
                                                  double* yout, double* part)
{
    if (!karena || !yold || nb == 0 || (frame != 0 && frame != 1)) return (int)hipErrorInvalidValue;
    const Slab S{slab5[0], slab5[1], slab5[2], slab5[3], slab5[4]};
    const DevConsts* c = static_cast<const DevConsts*>(consts);
    Dop853GridWeights dw;
    dop853_dense_weights(x, dw.w);
    const dim3 g(nb), b(DOP853_GRID_BLK);
    if (tiled) hipLaunchKernelGGL((dop853_grid_dense_kernel<LAYOUT_TILED>), g, b, 0, stream, yold, karena, kstride, frame, c, S, h, dw, at_start, yout, part);
    else hipLaunchKernelGGL((dop853_grid_dense_kernel<LAYOUT_FIELD_MAJOR>), g, b, 0, stream, yold, karena, kstride, frame, c, S, h, dw, at_start, yout, part);
    return (int)hipGetLastError();
}
