// marl_rk4_watch.h - fixed-step classical RK4 of one-workgroup grids (N <= 1024) with the reference's driver inside the kernel: the
// seven monitors after every step with their sign changes and root estimates, frames at given step counts, the `terminal` switch,
// and a stop when the state goes non-finite - word that the step was too large, which only a fixed-step method needs.  The monitored
// sibling of rk4_sweep_kernel (marl_kernels.h), which stays what it is; rules and record: marl_rk4_watch_ctl.h.
//
// Roots: the secant estimate  t_s + dt go / (go - gn)  between the monitor values at the two ends of a step.  NO dense output and NO
// Brent: a fixed step takes no partial steps, and the estimate is O(dt^2) away from the root of the solution's monitor.  A terminal
// monitor ends the run at the END of its step with that step's result - not interpolated to the root, unlike marl_terminal.h's rule.
//
// One step:  rk4_sweep_kernel's, expression for expression (TR_FILL, then three TR_REUSE, the same order of sums), then the epilogue:
//   per-thread monitor partials of the new state (monitors_kernel's U and W from Phi - uw_point -, monitors_accumulate; slot 0, the sum
//   slot, counts the thread's cell when one of its fields is non-finite) into LDS columns of their own  ->  barrier  ->  waves 0..7
//   reduce one quantity each, in block_reduce's order and with its combine, into the record in LDS  ->  barrier  ->  thread 0 runs
//   rk4_watch_step on it and publishes its decision  ->  barrier  ->  every thread reads the decision, stores its cell of a frame that
//   is due, and leaves the loop on a stop.
// Three barriers per step beside the evaluations' four.  The columns are not the edge-exchange buffers (block_reduce through those
// costs two more barriers, one on either side: measured 1.475 x the plain sweep per step at 4096 x N = 1024 against 1.438 x;
// profiles/rk4_watch_timing.log):
// columns, record and decision word are rewritten only after the next step's barriers, so nothing else orders them.  Everything the
// loop branches on (the decision, the step count) is the same in every thread: each barrier is reached by all waves or by none.
#pragma once
#include "marl_kernels.h"
#include "marl_rk4_watch_ctl.h"

namespace marl {

// Y: [instance][5][N] in place; recs: [instance], t0 and dt filled by the host, the rest written here; frame_steps: n_frames step counts
// (device; checked by the host); frames: [instance][n_frames][5][N], a frame the instance does not reach is not touched; t_events:
// [instance][7][max_events] or NULL, filled by the caller (NaN); lim: marl_set_terminal's seven limits (device; read by thread 0 at a
// sign change only - by value they cost the loop 14 scalar registers) or NULL for none.
template <int BLK, bool VD = false>
__global__ void __launch_bounds__(BLK) rk4_watch_kernel(double* __restrict__ Y, const DevConsts* __restrict__ consts, Rk4WatchRec* __restrict__ recs,
                                                        int64_t N, int64_t nsteps, const int64_t* __restrict__ frame_steps, int64_t n_frames,
                                                        double* __restrict__ frames, double* __restrict__ t_events, int64_t max_events,
                                                        const int64_t* __restrict__ lim)
{
    using SB = StencilBlock<BLK, false, VD>;
    constexpr int NW = BLK / 64;
    __shared__ double lds[SB::LDS_DOUBLES + NQ * BLK + NQ];   // the evaluations' part, the monitor columns [slot][thread], the reduced record
    __shared__ Rk4WatchRec sr;
    __shared__ int s_dec;
    __shared__ int64_t s_frame;
    const DevConsts& C = consts[blockIdx.x];
    double* yg = Y + (int64_t)blockIdx.x * NF * N;
    double* fg = frames + (int64_t)blockIdx.x * n_frames * NF * N;
    double* tev = t_events ? t_events + (int64_t)blockIdx.x * 7 * max_events : nullptr;
    Slab S = {N, 0, N, 0, N};
    const int64_t l0 = threadIdx.x;
    SB sb(lds, l0, consts + blockIdx.x);
    const double dt = recs[blockIdx.x].dt;
    const double h2 = 0.5 * dt, h6 = dt / 6.0;
    double y[NF], ys[NF], k[NF], acc[NF];
    PointAux aux;
    load_cells<LAYOUT_FIELD_MAJOR>(yg, l0, S, C, y);

    double* mon = lds + SB::LDS_DOUBLES;
    double* rec = mon + NQ * BLK;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // the reduction record of the state in y into rec, visible to every thread on return
    auto record_of_state = [&]() {
        double q[NQ];
        monitors_init(q);
        MARL_ONCE if (l0 < N) {
            double U, W;
            uw_point(y[4], C, sb.T, U, W);
            monitors_accumulate(q, y, U, W);
            bool finite = true;
            MARL_FIELDS finite = finite && (fabs(y[f]) < __builtin_inf());
            q[0] = finite ? 0.0 : 1.0;
        }
#pragma unroll
        for (int j = 0; j < NQ; j++) mon[j * BLK + threadIdx.x] = q[j];
        __syncthreads();
#pragma unroll
        for (int jj = 0; jj < (NQ + NW - 1) / NW; jj++) {   // (block_reduce's second half: slot 0 summed, 1..NQMIN minima, the rest maxima)
            const int j = wave + jj * NW;                   // wave-uniform
            if (j < NQ) {
                auto combine = [j](double a, double o) { return (j == 0) ? a + o : (j <= NQMIN ? mon_min(a, o) : mon_max(a, o)); };
                double a = mon[j * BLK + lane];
#pragma unroll
                for (int i = 1; i < NW; i++) a = combine(a, mon[j * BLK + lane + 64 * i]);
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) a = combine(a, __shfl_xor(a, off, 64));
                if (lane == 0) rec[j] = a;
            }
        }
        __syncthreads();
    };
    auto store_frame = [&](int64_t j) {
        MARL_ONCE if (l0 < N) {
#pragma unroll
            for (int f = 0; f < NF; f++) fg[j * NF * N + at<LAYOUT_FIELD_MAJOR>(f, l0, N)] = y[f];
        }
    };

    {
        record_of_state();
        if (threadIdx.x == 0) {
            sr = recs[blockIdx.x];
            s_dec = rk4_watch_begin(sr, rec, frame_steps, n_frames);
        }
        __syncthreads();
        if (s_dec & RK4W_FRAME) store_frame(0);
    }
#pragma unroll 1
    for (int64_t s = 0; s < nsteps; s++) {
        sb.template eval<TR_FILL>(y, k, aux);
        MARL_FIELDS { acc[f] = k[f]; ys[f] = y[f] + h2 * k[f]; }
        sb.template eval<TR_REUSE>(ys, k, aux);
        MARL_FIELDS { acc[f] = acc[f] + 2.0 * k[f]; ys[f] = y[f] + h2 * k[f]; }
        sb.template eval<TR_REUSE>(ys, k, aux);
        MARL_FIELDS { acc[f] = acc[f] + 2.0 * k[f]; ys[f] = y[f] + dt * k[f]; }
        sb.template eval<TR_REUSE>(ys, k, aux);
        MARL_FIELDS y[f] = y[f] + h6 * (acc[f] + k[f]);

        record_of_state();
        if (threadIdx.x == 0) {
            const int dec = rk4_watch_step(sr, rec, frame_steps, n_frames, lim, tev, max_events);
            s_frame = sr.next_frame - 1;
            s_dec = dec;
        }
        __syncthreads();
        const int dec = s_dec;
        if (dec & RK4W_FRAME) store_frame(s_frame);
        if (dec & RK4W_STOP) break;
    }
    MARL_ONCE if (l0 < N) {
#pragma unroll
        for (int f = 0; f < NF; f++) yg[at<LAYOUT_FIELD_MAJOR>(f, l0, N)] = y[f];
    }
    if (threadIdx.x == 0) recs[blockIdx.x] = sr;
}

}  // namespace marl
