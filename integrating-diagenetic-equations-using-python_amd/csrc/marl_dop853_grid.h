// marl_dop853_grid.h - the native DOP853 loop of ONE grid of any size (gfx950): scipy's DOP853 (marl_dop853_ctl.h) as one launch per
// STAGE, the large-grid counterpart of the one-workgroup body of marl_dop853.h.
//
// On a grid of many workgroups a stage state  y + h sum_j a_sj K_j  needs its neighbours' values, which other workgroups own: the
// stage loop that dop853_sweep_body runs around one inlined evaluation is here a loop of LAUNCHES on the host - the launch-per-attempt
// shape of rk23_attempt_kernel, cut at every evaluation.  What the kernels share with the other explicit loops: StencilBlock and
// everything under it, load_cells, the monitors and their record, block_reduce, the controller record Rk45Ctrl with rk45_init_kernel /
// rk45_resume_kernel (they hold no method constant) and the event bookkeeping rk45_events.
//
//   * dop853_grid_stage_kernel: 256 threads, one cell each, windows of 254 written cells and one halo cell per side.  EVERY thread
//     of the window, halo included, forms its own stage state from the arena, so no launch depends on another workgroup of the same
//     launch; the row index s is an argument, a zero coefficient of the row skips its load and its add (the row is wave-uniform: a
//     scalar branch), the others are summed left to right in the order of j.  The step size and the status come from the device
//     controller: a launch whose controller is not ST_RUNNING returns at once, so the host enqueues batches of attempts blindly.
//     Row 12 forms y_new, writes it into the other state buffer, evaluates K_13 = f(y_new), forms both error sums over K_1..K_12 and
//     the seven monitors of y_new and leaves one record per workgroup: {sum (err5 / scale)^2, monitors} and, in an array of its own,
//     sum (err3 / scale)^2.  Rows 13..15 (the dense output's extra stages) are run once per step that needs them, with `replay`: the
//     step just ACCEPTED (state buffer cur ^ 1, size h_prev), whatever the status.  Row 0 is K_1 = f(y) of the first step.
//   * The arena: 16 state-shaped buffers in the layout of the state, `kstride` doubles apart.  Slots 0 and 12 alternate as K_1 and
//     K_13 (dop853_grid_slot, marl_dop853_grid_ctl.h): acceptance flips Rk45Ctrl.cur, which swaps the state buffers AND these two
//     slots; nothing is copied.
//   * dop853_grid_reduce_kernel / dop853_grid_control_kernel: records and second sums are combined in a fixed order (strided partial
//     sums per thread, a butterfly per wave, the waves in order) - no float atomics, a run is reproducible bit for bit.  One lane then
//     decides (dop853_decide), books the monitors (rk45_events), counts the dense output of a step that has one, and pauses as
//     rk45_control_kernel does: ST_PAUSED when the accepted step holds a sample or, with pause_on_event, a sign change.
//   * dop853_grid_dense_kernel:  y_old + h sum_j w_j K_j  over the 16 slots (weights by value: dop853_dense_weights), into `yout`
//     when given, and its monitors as one record per workgroup.  No evaluation, so no halo: 256 cells per workgroup.
//
// Every kernel runs to completion: no device-wide barrier, no persistent loop, no wait on memory.
//
// Compiled as its own translation unit (marl_dop853_grid.hip); it includes nothing of marl_dop853.h and instantiates none of its kernels.
#pragma once
#include "marl_kernels.h"
#include "marl_dop853_ctl.h"
#include "marl_dop853_grid_ctl.h"

namespace marl {

constexpr int DOP853_GRID_BATCH = 4;   // stage derivatives loaded together in a stage sum
static_assert(DOP853_GRID_SLOTS == dop853::N_STAGES_EXTENDED, "one slot per stage derivative of the extended tableau");
static_assert(dop853::N_STAGES % DOP853_GRID_BATCH == 0, "the error sums walk K_1..K_12 in whole batches");

struct Dop853GridWeights { double w[DOP853_GRID_SLOTS]; };

// s = 0: K_1 = f(y).  s = 1..11: K_(s+1).  s = 12: y_new, K_13 and the attempt's records.  s = 13..15 (replay only): K_14..K_16.
//   Y0, Y1: the two state buffers; karena + slot * kstride: the slots; part [gridDim.x][NQ], part3 [gridDim.x] (row 12 only).
template <int LAYOUT, bool VD = false>
__global__ void __launch_bounds__(DOP853_GRID_BLK)
dop853_grid_stage_kernel(double* __restrict__ Y0, double* __restrict__ Y1, double* __restrict__ karena, int64_t kstride,
                         const DevConsts* __restrict__ consts, Slab S, const Rk45Ctrl* __restrict__ ctrl, int s, int replay,
                         double* __restrict__ part, double* __restrict__ part3)
{
    constexpr int BLK = DOP853_GRID_BLK, H = DOP853_GRID_HALO, V = DOP853_GRID_WRITTEN;
    using SB = StencilBlock<BLK, false, VD>;
    static_assert(SB::EDGE_DOUBLES >= NQ * BLK, "block_reduce transposes the record through the edge buffers");
    __shared__ double lds[SB::LDS_DOUBLES];
    __shared__ double wsum3[BLK / 64];             // per-wave sums of (err3 / scale)^2
    if (!replay && ctrl->status != ST_RUNNING) return;
    const DevConsts& C = consts[0];
    const int frame = replay ? (ctrl->cur ^ 1) : ctrl->cur;
    const double h = replay ? ctrl->h_prev : ctrl->h_try;
    const double* yin = frame ? Y1 : Y0;
    double* yout = frame ? Y0 : Y1;

    const int64_t w0 = S.out_lo + (int64_t)blockIdx.x * V - H;
    const int64_t l = w0 + (int64_t)threadIdx.x;
    const bool in = l >= 0 && l < S.n_buf;

    double y[NF], ys[NF], k[NF];
    PointAux aux;
    load_cells<LAYOUT>(yin, l, S, C, y);              // in flight while the tables are staged
    SB sb(lds, l + S.goff, consts);                   // (table copy + barrier inside)

    double acc[NF] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (s > 0) {
        const double* row = dop853_row(s);
        // four K_j in flight at a time; a zero coefficient (the same in every lane) skips the load and the add
#pragma nounroll
        for (int j0 = 0; j0 < s; j0 += DOP853_GRID_BATCH) {
            double kk[DOP853_GRID_BATCH][NF];
#pragma unroll
            for (int u = 0; u < DOP853_GRID_BATCH; u++) {
                if (j0 + u < s && row[j0 + u] != 0.0) {
                    const double* kj = karena + (int64_t)dop853_grid_slot(j0 + u, frame) * kstride;
                    MARL_FIELDS kk[u][f] = in ? kj[at<LAYOUT>(f, l, S.ld)] : 0.0;
                }
            }
#pragma unroll
            for (int u = 0; u < DOP853_GRID_BATCH; u++) {
                if (j0 + u < s) {
                    const double a = row[j0 + u];
                    if (a != 0.0) {
                        MARL_FIELDS acc[f] += a * kk[u][f];
                    }
                }
            }
        }
    }
    MARL_FIELDS ys[f] = y[f] + acc[f] * h;
    sb.eval(ys, k, aux);

    const int wi = threadIdx.x;
    const bool owned = wi >= H && wi < BLK - H && l >= S.out_lo && l < S.out_hi;
    double* kout = karena + (int64_t)dop853_grid_slot(s, frame) * kstride;
    MARL_ONCE if (owned) {
        MARL_FIELDS kout[at<LAYOUT>(f, l, S.ld)] = k[f];
    }
    if (s != dop853::N_STAGES) return;                // (the row is a kernel argument: every wave leaves, or none)

    // row 12: ys is y_new
    double q[NQ], q3 = 0.0;
    monitors_init(q);
    MARL_ONCE if (owned) {
        double e5[NF] = {0.0, 0.0, 0.0, 0.0, 0.0}, e3[NF] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma nounroll
        for (int j0 = 0; j0 < dop853::N_STAGES; j0 += DOP853_GRID_BATCH) {   // (E5[12] = E3[12] = 0: f(y_new) has weight 0 in both estimates)
            double kk[DOP853_GRID_BATCH][NF];
#pragma unroll
            for (int u = 0; u < DOP853_GRID_BATCH; u++) {
                if (dop853::E5[j0 + u] != 0.0 || dop853::E3[j0 + u] != 0.0) {
                    const double* kj = karena + (int64_t)dop853_grid_slot(j0 + u, frame) * kstride;
                    MARL_FIELDS kk[u][f] = kj[at<LAYOUT>(f, l, S.ld)];
                }
            }
#pragma unroll
            for (int u = 0; u < DOP853_GRID_BATCH; u++) {
                const double a5 = dop853::E5[j0 + u], a3 = dop853::E3[j0 + u];
                if (a5 != 0.0 || a3 != 0.0) {
                    MARL_FIELDS {
                        e5[f] += a5 * kk[u][f];
                        e3[f] += a3 * kk[u][f];
                    }
                }
            }
        }
        const double rtol = ctrl->rtol, atol = ctrl->atol;
        MARL_FIELDS {
            yout[at<LAYOUT>(f, l, S.ld)] = ys[f];
            const double scale = atol + fmax(fabs(y[f]), fabs(ys[f])) * rtol;
            const double r5 = e5[f] / scale, r3 = e3[f] / scale;
            q[0] += r5 * r5;
            q3 += r3 * r3;
        }
        monitors_accumulate(q, ys, aux.U, aux.W);   // (aux: of this evaluation, f(y_new))
    }
    // the second sum rides on the record reduction's barriers: every wave butterflies its own, lane 0 leaves it in wsum3, and thread 0
    // adds the waves' sums in wave order behind block_reduce
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) q3 += __shfl_xor(q3, off, 64);
    if ((threadIdx.x & 63) == 0) wsum3[threadIdx.x >> 6] = q3;
    block_reduce<BLK, NQ, NQMIN>(q, lds);   // (a barrier first: the edge-exchange buffers are free behind it)
    if (threadIdx.x == 0) {
        double s3 = 0.0;
#pragma unroll
        for (int w = 0; w < BLK / 64; w++) s3 += wsum3[w];
#pragma unroll
        for (int j = 0; j < NQ; j++) part[(int64_t)blockIdx.x * NQ + j] = q[j];
        part3[blockIdx.x] = s3;
    }
}

// `n` records and second sums of this thread's share, combined in index order into (q, s3)
__device__ __forceinline__ void dop853_grid_gather(const double* __restrict__ recs, const double* __restrict__ sums3, int64_t lo, int64_t hi,
                                                   int stride, double (&q)[NQ], double& s3)
{
    for (int64_t b = lo + threadIdx.x; b < hi; b += stride) {
        double o[NQ];
#pragma unroll
        for (int j = 0; j < NQ; j++) o[j] = recs[b * NQ + j];
        const double o3 = sums3[b];
#pragma unroll
        for (int j = 0; j < NQ; j++) q[j] = (j == 0) ? q[j] + o[j] : (j <= NQMIN ? nanmin(q[j], o[j]) : nanmax(q[j], o[j]));
        s3 += o3;
    }
}

// (q, s3) of every thread -> thread 0: block_reduce for the record; the second sum by a butterfly per wave and the waves in order
template <int THREADS>
__device__ __forceinline__ void dop853_grid_block_reduce(double (&q)[NQ], double& s3, double* scratch, double* wsum3)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s3 += __shfl_xor(s3, off, 64);
    if ((threadIdx.x & 63) == 0) wsum3[threadIdx.x >> 6] = s3;
    block_reduce<THREADS, NQ, NQMIN>(q, scratch);   // (barriers inside: wsum3 is complete behind them)
    if (threadIdx.x == 0) {
        double a = 0.0;
#pragma unroll
        for (int w = 0; w < THREADS / 64; w++) a += wsum3[w];
        s3 = a;
    }
}

// First level for many workgroups (dop853_grid_first_level): workgroup g reduces records and second sums [g chunk, (g + 1) chunk).
__global__ void __launch_bounds__(256) dop853_grid_reduce_kernel(const double* __restrict__ recs, const double* __restrict__ sums3, int64_t nrec,
                                                                 int64_t chunk, double* __restrict__ out, double* __restrict__ out3)
{
    __shared__ double scratch[NQ * 256];
    __shared__ double wsum3[256 / 64];
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = (lo + chunk < nrec) ? lo + chunk : nrec;
    double q[NQ], s3 = 0.0;
    monitors_init(q);
    dop853_grid_gather(recs, sums3, lo, hi, 256, q, s3);
    dop853_grid_block_reduce<256>(q, s3, scratch, wsum3);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < NQ; j++) out[(int64_t)blockIdx.x * NQ + j] = q[j];
        out3[blockIdx.x] = s3;
    }
}

// The attempt's decision on the reduced record: q = {sum (err5 / scale)^2, monitors of y_new}, s3 = sum (err3 / scale)^2.
__device__ __forceinline__ void dop853_grid_finish_attempt(Rk45Ctrl& c, const double (&q)[NQ], double s3)
{
    if (dop853_decide(c, q[0], s3)) {
        const int fired = rk45_events(c, q);
        if (dop853_grid_step_is_dense(fired, c.t, c.pause_t)) dop853_count_dense_output(c);
        dop853_status_after_accept(c);            // end of the interval, or the pause for a sample
        if (c.status == ST_RUNNING && fired && c.pause_on_event) c.status = ST_PAUSED;
        if (c.status == ST_PAUSED) c.event_fired = fired;
    }
    if (c.status == ST_RUNNING) dop853_prepare_attempt(c);
}

// rk45_control_kernel with the DOP853 decision and its two sums: combine `nrec` records in index order and finish the attempt.
__global__ void __launch_bounds__(CONTROL_THREADS) dop853_grid_control_kernel(const double* __restrict__ recs, const double* __restrict__ sums3,
                                                                              int64_t nrec, Rk45Ctrl* ctrl)
{
    __shared__ double scratch[NQ * CONTROL_THREADS];
    __shared__ double wsum3[CONTROL_THREADS / 64];
    const int32_t status = ctrl->status;
    double q[NQ], s3 = 0.0;
    monitors_init(q);
    dop853_grid_gather(recs, sums3, 0, nrec, CONTROL_THREADS, q, s3);
    if (status != ST_RUNNING) return;   // (read first, tested last: the record loads do not wait for it)
    dop853_grid_block_reduce<CONTROL_THREADS>(q, s3, scratch, wsum3);
    if (threadIdx.x == 0) {
        Rk45Ctrl c = *ctrl;
        dop853_grid_finish_attempt(c, q, s3);
        *ctrl = c;
    }
}

// Dense output of the accepted step whose first state is `yold` and whose stage derivatives lie in the slots of `frame`:
//   d = y_old + h sum_j w_j K_j  (at_start: y_old itself, whatever 0 * K_j gives)  -> yout (may be NULL), monitors of d -> part
//   (may be NULL), one record per workgroup.  256 cells per workgroup.
template <int LAYOUT>
__global__ void __launch_bounds__(DOP853_GRID_BLK)
dop853_grid_dense_kernel(const double* __restrict__ yold, const double* __restrict__ karena, int64_t kstride, int frame,
                         const DevConsts* __restrict__ consts, Slab S, double h, Dop853GridWeights dw, int at_start,
                         double* __restrict__ yout, double* __restrict__ part)
{
    constexpr int BLK = DOP853_GRID_BLK;
    __shared__ double scratch[NQ * BLK];
    __shared__ double tabs[TABLE_DOUBLES];
    const Tables T = load_tables(tabs, BLK);
    const DevConsts& C = consts[0];
    const int64_t l = S.out_lo + (int64_t)blockIdx.x * BLK + threadIdx.x;
    double q[NQ];
    monitors_init(q);
    MARL_ONCE if (l < S.out_hi) {
        double y[NF], d[NF] = {0.0, 0.0, 0.0, 0.0, 0.0};
        MARL_FIELDS y[f] = yold[at<LAYOUT>(f, l, S.ld)];
#pragma nounroll
        for (int j0 = 0; j0 < DOP853_GRID_SLOTS; j0 += DOP853_GRID_BATCH) {
            double kk[DOP853_GRID_BATCH][NF];
#pragma unroll
            for (int u = 0; u < DOP853_GRID_BATCH; u++) {
                const double* kj = karena + (int64_t)dop853_grid_slot(j0 + u, frame) * kstride;
                MARL_FIELDS kk[u][f] = kj[at<LAYOUT>(f, l, S.ld)];
            }
#pragma unroll
            for (int u = 0; u < DOP853_GRID_BATCH; u++) {
                const double wj = dw.w[j0 + u];
                MARL_FIELDS d[f] += wj * kk[u][f];
            }
        }
        MARL_FIELDS d[f] = at_start ? y[f] : h * d[f] + y[f];
        if (yout) {
            MARL_FIELDS yout[at<LAYOUT>(f, l, S.ld)] = d[f];
        }
        if (part) {
            double U, W;
            uw_point(d[4], C, T, U, W);
            monitors_accumulate(q, d, U, W);
        }
    }
    if (!part) return;                 // (an argument: every wave leaves, or none)
    block_reduce<BLK, NQ, NQMIN>(q, scratch);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < NQ; j++) part[(int64_t)blockIdx.x * NQ + j] = q[j];
    }
}

}  // namespace marl
