// marl_rk23.h - the native RK23 loops (gfx950): scipy's RK23 (scipy/integrate/_ivp/rk.py, class RK23: Bogacki-Shampine 3(2)) on the
// stencil engine, the monitors, the reductions and the step controller record of the RK45 kernels (marl_kernels.h).
//
// Shared with RK45: StencilBlock and everything under it, Rk45Ctrl, rk45_init_kernel / rk45_resume_kernel (they hold no method
// constant), the event bookkeeping (rk45_event_one, rk45_events, rk45_advance_status), the error scale (dp45_err2), the record
// reductions, and the whole loop of the one-workgroup sweeps: rk45_sweep_body is instantiated with Bs23Method below in place of
// Dp45Method - loop shapes, barrier counts, uniformity rules and argument lists are those of the rk45_sweep_* kernels by construction.
// Not shared: the attempt (three evaluations after K1 instead of six, a halo of 3 cells per side instead of 6), the decision
// (marl_rk23_ctl.h: exponent -1/3, 3 evaluations per attempt) and the dense-output weights (four, cubic).
//
// Compiled as its own translation unit (marl_rk23.hip), which leaves the code generation of the other units alone.
#pragma once
#include "marl_kernels.h"
#include "marl_rk23_ctl.h"

namespace marl {

// x^e for the step factor: exp(e log x) through the LDS tables where the caller has them (~3 ulp, a fifth of OCML pow's
// instructions - as the RK45 decision), OCML pow outside (1e-300, 1e300) and without tables.
struct Rk23Power {
    const Tables* T;
    __device__ __forceinline__ double operator()(double x, double e) const
    {
        if (T && x > 1e-300 && x < 1e300) return fast_exp(e * fast_log(x, *T), *T);
        return pow(x, e);
    }
};

// One Bogacki-Shampine attempt on the per-thread cells, the counterpart of dp45_attempt: K1 given; returns y_new in `yn`,
// K4 = f(y_new) in `k4` (FSAL: the next step's K1) and the error-estimate numerator  sum_j E_j K_j  in `esum` (rk_step, rk.py:61-69;
// _estimate_error :103-104).  With DENSE, or with EITHER when `dense_now` (workgroup-uniform), `esum` instead receives
// sum_j w_j K_j  for the dense-output weights dw.w[0..3] (RkDenseOutput, rk.py:560-574).  Every sum runs in the left-to-right order of
// np.dot(K[:s].T, a[:s]); the zero A31 is skipped as the zero coefficients of Dormand-Prince are.
// PARK and the two separate blocks of EITHER: see dp45_attempt - the constant block is the statement of the plain attempt, so that it
// is compiled as there, and the run-time block hands its sums through an empty asm.
template <int BLK, bool DENSE = false, class SB = StencilBlock<BLK>, int PARK = 0, bool EITHER = false>
__device__ __forceinline__ void bs23_attempt(SB& sb, double h, const double (&y)[NF], const double (&k1)[NF],
                                             double (&yn)[NF], double (&k4)[NF], double (&esum)[NF],
                                             PointAux& aux, const DenseWeights& dw = DenseWeights{}, const double* pk = nullptr,
                                             bool dense_now = false)
{
    static_assert(!(EITHER && DENSE), "EITHER chooses at run time");
#define MARL_SEPARATE_BLOCKS() MARL_FIELDS asm volatile("" : "+v"(esum[f]))
#define MARL_Y(f) ((f) < PARK ? pk[(f) * BLK] : y[f])
    const double e1 = DENSE ? dw.w[0] : bs23::E1, e2 = DENSE ? dw.w[1] : bs23::E2, e3 = DENSE ? dw.w[2] : bs23::E3;
    const double e4 = DENSE ? dw.w[3] : bs23::E4;
    double ys[NF], k2[NF], k3[NF];
    MARL_FIELDS ys[f] = MARL_Y(f) + (k1[f] * bs23::A21) * h;
    sb.template eval<TR_FILL>(ys, k2, aux);
    MARL_FIELDS ys[f] = MARL_Y(f) + (k2[f] * bs23::A32) * h;
    sb.template eval<TR_REUSE>(ys, k3, aux);
    MARL_FIELDS {
        yn[f] = MARL_Y(f) + h * (k1[f] * bs23::B1 + k2[f] * bs23::B2 + k3[f] * bs23::B3);
        if constexpr (!EITHER) esum[f] = k1[f] * e1 + k2[f] * e2 + k3[f] * e3;
    }
    if constexpr (EITHER) {
        if (dense_now) {
            MARL_FIELDS esum[f] = k1[f] * dw.w[0] + k2[f] * dw.w[1] + k3[f] * dw.w[2];
            MARL_SEPARATE_BLOCKS();
        } else {
            MARL_FIELDS esum[f] = k1[f] * bs23::E1 + k2[f] * bs23::E2 + k3[f] * bs23::E3;
        }
    }
    sb.template eval<TR_REUSE>(yn, k4, aux);
    if constexpr (EITHER) {
        if (dense_now) {
            MARL_FIELDS esum[f] = esum[f] + k4[f] * dw.w[3];
            MARL_SEPARATE_BLOCKS();
        } else {
            MARL_FIELDS esum[f] = esum[f] + k4[f] * bs23::E4;
        }
    } else {
        MARL_FIELDS esum[f] = esum[f] + k4[f] * e4;
    }
#undef MARL_SEPARATE_BLOCKS
#undef MARL_Y
}

__device__ __forceinline__ DenseWeights bs23_dense_weights(double x)
{
    DenseWeights dw = {};
    double w[4];
    rk23_dense_weights(x, w);
#pragma unroll
    for (int j = 0; j < 4; j++) dw.w[j] = w[j];
    return dw;
}

// rec = {sum (err/scale)^2, monitors of y_new}: rk45_finish_attempt with the RK23 decision.
__device__ __forceinline__ void rk23_finish_attempt(Rk45Ctrl& c, const double (&rec)[NQ], const Tables* T = nullptr)
{
    const bool accepted = rk23_decide(c, rec[0], Rk23Power{T});
    const int fired = accepted ? rk45_events(c, rec) : 0;
    rk45_advance_status(c, accepted, fired);
}

// the method description rk45_sweep_body asks for (Dp45Method, marl_kernels.h)
struct Bs23Method {
    static constexpr int N_WEIGHTS = bs23::N_WEIGHTS;
    template <int BLK, class SB, int PARK, bool EITHER>
    static __device__ __forceinline__ void attempt(SB& sb, double h, const double (&y)[NF], const double (&k1)[NF], double (&yn)[NF],
                                                   double (&kn)[NF], double (&esum)[NF], PointAux& aux, const DenseWeights& dw,
                                                   const double* pk, bool dense_now)
    {
        bs23_attempt<BLK, false, SB, PARK, EITHER>(sb, h, y, k1, yn, kn, esum, aux, dw, pk, dense_now);
    }
    static __device__ __forceinline__ void finish_attempt(Rk45Ctrl& c, const double (&rec)[NQ], const Tables* T) { rk23_finish_attempt(c, rec, T); }
    static __device__ __forceinline__ bool decide_lean(Rk45Ctrl& c, double sumsq, double inv_n, const Tables& T)
    {
        return rk23_decide_lean(c, sumsq, inv_n, Rk23Power{&T});
    }
    static __device__ __forceinline__ void prepare_attempt_lean(Rk45Ctrl& c) { rk23_prepare_attempt_lean(c); }
    static __device__ __forceinline__ DenseWeights weights(double x) { return bs23_dense_weights(x); }
};

// ---- one workgroup per instance (N <= BLK cells): the loops of the rk45_sweep_* kernels of the same names ----------------------
template <int BLK, bool VD = false>
__global__ void __launch_bounds__(BLK) rk23_sweep_kernel(double* __restrict__ Y, const DevConsts* __restrict__ consts,
                                                         Rk45Ctrl* __restrict__ ctrls, int64_t N,
                                                         double* __restrict__ Yold, double* __restrict__ Fold)
{
    rk45_sweep_body<BLK, VD, true, false, false, Bs23Method>(Y, consts, ctrls, N, Yold, Fold);
}

// single small runs with event root finding (Rk45Ctrl.pause_on_event): the loop that decides with this step's events
template <int BLK, bool VD = false>
__global__ void __launch_bounds__(BLK) rk23_sweep_events_kernel(double* __restrict__ Y, const DevConsts* __restrict__ consts,
                                                                Rk45Ctrl* __restrict__ ctrls, int64_t N,
                                                                double* __restrict__ Yold, double* __restrict__ Fold)
{
    rk45_sweep_body<BLK, VD, false, false, false, Bs23Method>(Y, consts, ctrls, N, Yold, Fold);
}

// sweeps with t_eval: frames by dense-output replays before the commit (arguments: rk45_sweep_eval_kernel)
template <int BLK, bool VD = false>
__global__ void __launch_bounds__(BLK) rk23_sweep_eval_kernel(double* __restrict__ Y, const DevConsts* __restrict__ consts,
                                                              Rk45Ctrl* __restrict__ ctrls, int64_t N,
                                                              const double* __restrict__ t_eval, int64_t n_eval,
                                                              double* __restrict__ Yeval, int64_t* __restrict__ n_done)
{
    rk45_sweep_body<BLK, VD, true, true, false, Bs23Method>(Y, consts, ctrls, N, nullptr, nullptr, t_eval, n_eval, Yeval, n_done);
}

// sweeps that also locate the monitors' roots by Brent's method on probe trips (arguments: rk45_sweep_roots_kernel)
template <int BLK, bool VD = false>
__global__ void __launch_bounds__(BLK) rk23_sweep_roots_kernel(double* __restrict__ Y, const DevConsts* __restrict__ consts,
                                                               Rk45Ctrl* __restrict__ ctrls, int64_t N,
                                                               const double* __restrict__ t_eval, int64_t n_eval,
                                                               double* __restrict__ Yeval, int64_t* __restrict__ n_done,
                                                               double* __restrict__ t_events, int64_t max_events)
{
    rk45_sweep_body<BLK, VD, true, true, true, Bs23Method>(Y, consts, ctrls, N, nullptr, nullptr, t_eval, n_eval, Yeval, n_done, t_events,
                                                           max_events);
}

// rk23_sweep_roots_kernel honouring terminal monitors (arguments: rk45_sweep_term_kernel)
template <int BLK, bool VD = false>
__global__ void __launch_bounds__(BLK) rk23_sweep_term_kernel(double* __restrict__ Y, const DevConsts* __restrict__ consts,
                                                              Rk45Ctrl* __restrict__ ctrls, int64_t N,
                                                              const double* __restrict__ t_eval, int64_t n_eval,
                                                              double* __restrict__ Yeval, int64_t* __restrict__ n_done,
                                                              double* __restrict__ t_events, int64_t max_events, TermLimits lim)
{
    rk45_sweep_body<BLK, VD, true, true, true, Bs23Method, true>(Y, consts, ctrls, N, nullptr, nullptr, t_eval, n_eval, Yeval, n_done, t_events,
                                                                 max_events, lim);
}

// ---- one large grid, one launch per attempt ---------------------------------------------------------------------------------------
// The counterpart of rk45_attempt_kernel: reads (y, f) from buffer `cur`, writes (y_new, f_new) into the other buffer and one
// reduction record per block; rk23_control_kernel then accepts (flips `cur`) or rejects.  Three evaluations after K1: a halo of
// H = 3 cells per side, 250 cells written per 256-thread window.  The same Slab, buffer pairs and record layout; the same
// four-waves-per-SIMD shape with RK23_ATTEMPT_PARK fields of y parked in LDS (their columns double as reduction columns).
constexpr int RK23_HALO = 3;
constexpr int RK23_ATTEMPT_PARK = 3;

template <int BLK, int LAYOUT, bool VD = false>
__global__ void __launch_bounds__(BLK) __attribute__((amdgpu_waves_per_eu(4, 8)))
rk23_attempt_kernel(double* __restrict__ Y0, double* __restrict__ Y1, double* __restrict__ F0, double* __restrict__ F1,
                    const DevConsts* __restrict__ consts, Slab S, const Rk45Ctrl* __restrict__ ctrl, double* __restrict__ part)
{
    constexpr int H = RK23_HALO;
    constexpr int V = BLK - 2 * H;
    constexpr int PARK = RK23_ATTEMPT_PARK;
    using SB = StencilBlock<BLK, true, VD>;
    static_assert(BLK == 256 && SB::CACHE && PC_LDS_SLOTS >= 4, "the one-barrier record reduction (tile_reduce_halfwaves)");
    __shared__ double lds[SB::LDS_DOUBLES + PARK * BLK];
    if (ctrl->status != ST_RUNNING) return;
    const DevConsts& C = consts[0];
    const int cur = ctrl->cur;
    const double h = ctrl->h_try, rtol = ctrl->rtol, atol = ctrl->atol;
    const double* yin = cur ? Y1 : Y0;
    const double* fin = cur ? F1 : F0;
    double* yout = cur ? Y0 : Y1;
    double* fout = cur ? F0 : F1;

    const int64_t w0 = S.out_lo + (int64_t)blockIdx.x * V - H;
    const int64_t l = w0 + (int64_t)threadIdx.x;

    double y[NF], k1[NF], yn[NF], k4[NF], esum[NF];
    PointAux aux;
    load_cells<LAYOUT>(yin, l, S, C, y);              // in flight while the tables are staged
    MARL_ONCE {
        const bool in = l >= 0 && l < S.n_buf;
#pragma unroll
        for (int f = 0; f < NF; f++) k1[f] = in ? fin[at<LAYOUT>(f, l, S.ld)] : 0.0;
    }
    SB sb(lds, l + S.goff, consts);   // (table copy + barrier inside)
    double* pk = lds + SB::LDS_DOUBLES + threadIdx.x;
#pragma unroll
    for (int f = 0; f < PARK; f++) pk[f * BLK] = y[f];
    bs23_attempt<BLK, false, SB, PARK>(sb, h, y, k1, yn, k4, esum, aux, DenseWeights{}, pk);

    double q[NQ];
    monitors_init(q);
    const int wi = threadIdx.x;
    MARL_ONCE if (wi >= H && wi < BLK - H && l >= S.out_lo && l < S.out_hi) {
#pragma unroll
        for (int f = 0; f < NF; f++) {
            yout[at<LAYOUT>(f, l, S.ld)] = yn[f];
            fout[at<LAYOUT>(f, l, S.ld)] = k4[f];
            q[0] += dp45_err2(esum[f], h, f < PARK ? pk[f * BLK] : y[f], yn[f], rtol, atol);
        }
        monitors_accumulate<true>(q, yn, aux.U, aux.W);   // (the controller reads the extrema of ACCEPTED attempts only: all finite)
    }
    // Column 7 of the reduction is field 0 of the parity-0 edge buffer, which the THIRD (last) evaluation of this launch reads after its
    // exchange barrier: unlike the six-evaluation attempt, a wave may still be reading it when another arrives here.  One barrier first.
    __syncthreads();
    const double r = tile_reduce_halfwaves<BLK, SB>(q, lds, threadIdx.x);
    if ((threadIdx.x & 31) == 0) {
        const int j = threadIdx.x >> 5;
        part[(int64_t)blockIdx.x * NQ + j] = (j > NQMIN) ? -r : r;
    }
}

// rk45_control_kernel with the RK23 decision: combine `nrec` reduction records in index order and finish the attempt.
__global__ void __launch_bounds__(CONTROL_THREADS) rk23_control_kernel(const double* __restrict__ recs, int64_t nrec, Rk45Ctrl* ctrl)
{
    __shared__ double scratch[NQ * CONTROL_THREADS];
    const int32_t status = ctrl->status;
    double q[NQ];
    monitors_init(q);
    for (int64_t b = threadIdx.x; b < nrec; b += CONTROL_THREADS) {
        double o[NQ];
#pragma unroll
        for (int j = 0; j < NQ; j++) o[j] = recs[b * NQ + j];
#pragma unroll
        for (int j = 0; j < NQ; j++) q[j] = (j == 0) ? q[j] + o[j] : (j <= NQMIN ? nanmin(q[j], o[j]) : nanmax(q[j], o[j]));
    }
    if (status != ST_RUNNING) return;   // (read first, tested last: the record loads do not wait for it)
    block_reduce<CONTROL_THREADS, NQ, NQMIN>(q, scratch);
    if (threadIdx.x == 0) {
        Rk45Ctrl c = *ctrl;
        rk23_finish_attempt(c, q);
        *ctrl = c;
    }
}

// Dense output of the step that starts at (yold, fold) with size h: replays the step's stages and writes
// y(t_old + x h) = y_old + h sum_j w_j(x) K_j  (t_eval samples) and the monitors record of that state (event root finding), as
// rk45_dense_kernel does.  yout may be NULL.
template <int BLK, int LAYOUT, bool VD = false>
__global__ void __launch_bounds__(BLK) rk23_dense_kernel(const double* __restrict__ yold, const double* __restrict__ fold,
                                                         const DevConsts* __restrict__ consts, Slab S, double h,
                                                         DenseWeights dw, double* __restrict__ yout, double* __restrict__ part)
{
    constexpr int H = RK23_HALO;
    constexpr int V = BLK - 2 * H;
    using SB = StencilBlock<BLK, true, VD>;
    __shared__ double lds[SB::LDS_DOUBLES];
    const DevConsts& C = consts[0];
    const int64_t w0 = S.out_lo + (int64_t)blockIdx.x * V - H;
    const int64_t l = w0 + (int64_t)threadIdx.x;
    SB sb(lds, l + S.goff, consts);
    double y[NF], k1[NF], yn[NF], k4[NF], dsum[NF];
    PointAux aux;
    load_cells<LAYOUT>(yold, l, S, C, y);
    MARL_ONCE {
        const bool in = l >= 0 && l < S.n_buf;
#pragma unroll
        for (int f = 0; f < NF; f++) k1[f] = in ? fold[at<LAYOUT>(f, l, S.ld)] : 0.0;
    }
    bs23_attempt<BLK, true, SB>(sb, h, y, k1, yn, k4, dsum, aux, dw);
    double q[NQ];
    monitors_init(q);
    const int wi = threadIdx.x;
    MARL_ONCE if (wi >= H && wi < BLK - H && l >= S.out_lo && l < S.out_hi) {
        double d[NF];
#pragma unroll
        for (int f = 0; f < NF; f++) {
            d[f] = h * dsum[f] + y[f];
            if (yout) yout[at<LAYOUT>(f, l, S.ld)] = d[f];
        }
        double U, W;
        uw_point(d[4], C, sb.T, U, W);
        monitors_accumulate(q, d, U, W);
    }
    block_reduce<BLK, NQ, NQMIN>(q, lds);   // (a barrier first: the edge-exchange buffers are free behind it)
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < NQ; j++) part[(int64_t)blockIdx.x * NQ + j] = q[j];
    }
}

}  // namespace marl
