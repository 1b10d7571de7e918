// marl_bdf_batch.h - a SWEEP of implicit BDF integrations: the kernels of marl_sweep_bdf_dev (marl_api.hip, sweep_bdf).  The shape is
// the Radau sweep's launch-per-action cycle (marl_radau_batch.h, radau_sweep_wg = 0): every instance runs scipy's BDF step logic as a
// resumable state machine (marl_bdf_ctl.h; bdf_control_kernel, one lane per instance) that publishes its next piece of data-parallel
// work as an action word; the host repeats one fixed cycle of launches, each over the work list of the instances that asked for it.
// Every kernel runs to completion; nothing here waits for another workgroup.
//
// Arena of an instance (radau_alloc; bdf_run's layout): D = [Z | W | F] (8 n of 9 n), f(t_new, y) of the Newton iteration = Z0,
// y_predict / psi / d = Q, f(t0, y0) = f, f(t_new, y_predict) of a Jacobian refresh = fnew.
// The vector kernels keep the thread mapping and the reduction order of their single-run kernels (marl_bdf.h), the solve IS the
// single run's (solve_wg_body, marl_bdf_wg.h), the Jacobian is the Radau path's fd_* sequence over a list and the factorisation calls
// the same group functions (pcr_factor_group, cr_init_group, cr_reduce_group) with (mu, jscale) = (1, c) of the instance - so a sweep
// and a single run differ by the controller's scalar arithmetic (device libm; R U with numpy's roundings) and nothing else.
#pragma once
#include "marl_bdf_ctl.h"
#include "marl_bdf_wg.h"
#include "marl_radau_cr.h"

namespace marl {
namespace bdf {

using bdfctl::BdfCtl;
using bdfctl::BdfRoots;
using bdfctl::BdfSample;
using bdfctl::BdfTerm;

// work lists of a cycle; the count words are published by radau::publish_counts_kernel (L_COUNT words, then the sequence word)
// (BL_ROOTS holds the instances of A_ROOTS and of A_TERM_ROOTS - a step is one or the other - so that the words still fit L_COUNT)
enum : int { BL_ACCEPT = 0, BL_CHANGE_D, BL_JAC, BL_LU, BL_SOLVE, BL_SAMPLE, BL_ROOTS, BL_RUNNING, BL_PROGRESS, BL_STOP, BL_COUNT };
static_assert(BL_COUNT <= radau::L_COUNT, "publish_counts_kernel copies L_COUNT words");

// blockIdx.z -> instance (list == NULL: every instance, in order), its arena and its controller
struct BdfBatch {
    int64_t zstride;
    BdfCtl* ctls;
    const int32_t* list;
};
__device__ __forceinline__ ZBatch z_of(const BdfBatch& B) { return ZBatch{B.zstride, nullptr, 0, 0, B.list}; }

// One lane per instance: resume the step logic, run it to the next action word, append the instance to the list of every bit.
// rec: [B][8] monitors records of the instances' initial states (read at the first cycle).
// SAMPLES: the sweep has t_eval samples - samples, t_eval: the instances' t_eval states and the shared sample times.  Without them
// the step logic is compiled as the three-argument call: a sweep without samples runs the code it ran before there were any.
// ROOTS: the sweep locates the monitors' root times - roots: the instances' root-location states (A_ROOTS -> BL_ROOTS); without
// them the step logic is compiled as the call without a BdfRoots.
// TERM: the context has terminal monitors - terms: the instances' terminal-monitor states, t_events: the [B][7][max_events] root
// times the controller stores a terminal step's kept roots into (ROOTS only).  A_TERM_ROOTS -> BL_ROOTS, A_STOP -> BL_STOP.  A sweep
// without limits launches the instantiations without TERM: the code it ran before there were any.
template <bool SAMPLES, bool ROOTS, bool TERM = false>
__global__ void __launch_bounds__(64) bdf_control_kernel(BdfCtl* __restrict__ ctls, const double* __restrict__ rec, int64_t B, int64_t n,
                                                         int32_t* __restrict__ counts, int32_t* __restrict__ lists,
                                                         BdfSample* __restrict__ samples, const double* __restrict__ t_eval,
                                                         BdfRoots* __restrict__ roots, BdfTerm* __restrict__ terms = nullptr,
                                                         double* __restrict__ t_events = nullptr)
{
    const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    BdfCtl c = ctls[b];
    if (c.pc == bdfctl::PC_DONE) return;
    const double* r = rec + b * 8;
    const double g0[7] = {r[1], r[2], r[3], r[5] - 1.0, r[6] - 1.0, r[4], r[7]};   // record_to_events (marl_api.hip)
    const int32_t pc0 = c.pc, status0 = c.status;
    const int64_t attempts0 = c.attempts;
    if constexpr (TERM)
        bdfctl::bdf_control_step(c, n, g0, SAMPLES ? samples + b : nullptr, SAMPLES ? t_eval : nullptr, ROOTS ? roots + b : nullptr, terms + b,
                                 ROOTS ? t_events + b * 7 * roots[ROOTS ? b : 0].max_events : nullptr);
    else if constexpr (ROOTS) bdfctl::bdf_control_step(c, n, g0, SAMPLES ? samples + b : nullptr, SAMPLES ? t_eval : nullptr, roots + b);
    else if constexpr (SAMPLES) bdfctl::bdf_control_step(c, n, g0, samples + b, t_eval);
    else bdfctl::bdf_control_step(c, n, g0);
    ctls[b] = c;
    if (c.pc != bdfctl::PC_DONE) atomicAdd(&counts[BL_RUNNING], 1);
    if (c.pc != pc0 || c.status != status0 || c.attempts != attempts0) atomicAdd(&counts[BL_PROGRESS], 1);
    auto push = [&](int which) { lists[(int64_t)which * B + atomicAdd(&counts[which], 1)] = (int32_t)b; };
    if (c.action & bdfctl::A_ACCEPT) push(BL_ACCEPT);
    if (c.action & bdfctl::A_CHANGE_D) push(BL_CHANGE_D);
    if (c.action & bdfctl::A_JAC) push(BL_JAC);
    if (c.action & bdfctl::A_LU) push(BL_LU);
    if (c.action & bdfctl::A_SOLVE) push(BL_SOLVE);
    if constexpr (SAMPLES)
        if (c.action & bdfctl::A_SAMPLE) push(BL_SAMPLE);
    if constexpr (ROOTS)
        if (c.action & bdfctl::A_ROOTS) push(BL_ROOTS);
    if constexpr (TERM) {
        if (c.action & bdfctl::A_TERM_ROOTS) push(BL_ROOTS);
        if (c.action & bdfctl::A_STOP) push(BL_STOP);
    }
}

// D[0] = y0, D[1] = f h  (init_D_kernel; h = the controller's first step)
__global__ void __launch_bounds__(256) init_D_batch_kernel(const double* __restrict__ y, const double* __restrict__ f, int64_t n, double* __restrict__ D, BdfBatch B)
{
    const ZBatch zb = z_of(B);
    const double h = B.ctls[z_inst(zb)].S_h_abs;
    y = z_shift(y, zb); f = z_shift(f, zb); D = z_shift(D, zb);
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    D[i] = y[i];
    D[n + i] = f[i] * h;
}

// A_CHANGE_D: D[:order + 1] = RU^T D[:order + 1] with the controller's RU and ru_order (change_D_kernel)
__global__ void __launch_bounds__(256) change_D_batch_kernel(double* __restrict__ D, int64_t n, BdfBatch B)
{
    const ZBatch zb = z_of(B);
    const BdfCtl* c = B.ctls + z_inst(zb);
    D = z_shift(D, zb);
    const int order = c->ru_order;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double d[MAX_ORDER + 1];
#pragma unroll
    for (int j = 0; j <= MAX_ORDER; j++) d[j] = j <= order ? D[(int64_t)j * n + i] : 0.0;
#pragma unroll
    for (int k = 0; k <= MAX_ORDER; k++) {
        if (k > order) break;
        double a = 0;
#pragma unroll
        for (int j = 0; j <= MAX_ORDER; j++)
            if (j <= order) a += c->RU[j][k] * d[j];
        D[(int64_t)k * n + i] = a;
    }
}

// A_SAMPLE: the t_eval samples [first, end) of the step the instance just accepted, by the step's dense output (dense_kernel's sum
// with the weights of bdf_dense, here per sample on the device) -> frames y_eval[(instance n_eval + k) n + i], contiguous
// [B][n_eval][n] (not the arena's stride).  One element per thread: its D[0 .. order] are read once, every sample is one store.
__global__ void __launch_bounds__(256) sample_batch_kernel(const double* __restrict__ D, int64_t n, const double* __restrict__ t_eval, int64_t n_eval,
                                                           const BdfSample* __restrict__ samples, double* __restrict__ y_eval, BdfBatch B)
{
    const ZBatch zb = z_of(B);
    const int64_t inst = z_inst(zb);
    const BdfSample* s = samples + inst;
    D = z_shift(D, zb);
    const int order = s->order;
    const double t = s->t, h = s->h;
    const int64_t first = s->first, end = s->end < n_eval ? s->end : n_eval;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double d[MAX_ORDER + 1];
#pragma unroll
    for (int j = 0; j <= MAX_ORDER; j++) d[j] = j <= order ? D[(int64_t)j * n + i] : 0.0;
    double* out = y_eval + (inst * n_eval) * n + i;
    for (int64_t k = first; k < end; k++) {
        double p[MAX_ORDER + 1];
        bdfctl::bdf_dense_weights(t, h, order, t_eval[k], p);
        // the sum as dense_kernel (marl_bdf.h) writes it; that kernel keeps its own copy: called through a shared function its
        // machine code changed (another order of its argument loads)
        double a = 0;
#pragma unroll
        for (int j = 0; j < MAX_ORDER; j++)
            if (j < order) a += d[j + 1] * p[j];
        out[k * n] = a + d[0];
    }
}

// A_ROOTS, one workgroup per listed instance: the root times of every monitor that changed sign over the step the instance just accepted,
// the WHOLE search of all of them in this one launch (a root costs about ten evaluations of the step's dense output: one host cycle
// per evaluation would multiply the cycles of a run).  N <= WG_THREADS (the sweep takes 5 N <= PCR_FUSED_MAX): thread l owns cell l,
// loads its D[0 .. order] of the five fields once (at most 30 doubles, kept in registers) and an evaluation at tq is
//     scalar weights (bdf_dense_weights)  ->  the cell's dense state, sample_batch_kernel's sum  ->  the cell's monitor terms
//     (wg_monitors / monitors_kernel)  ->  block_reduce in LDS  ->  the seven monitors, read back from LDS by every thread
// with no global memory touched.  Control flow is uniform: every thread runs the scalar search (bdfctl::bdf_find_roots) redundantly
// on the reduced monitors all threads read after the barrier, so every thread reaches every barrier; the loops are bounded
// (<= 7 monitors x (2 + <= 100) evaluations).
// The body, shared by the two searches: src = the instance's BdfRoots (A_ROOTS) or BdfTerm (A_TERM_ROOTS) - the step (order, t, h,
// t_old) and the monitors to search - read where it is (a private copy would sit in scratch memory); put(e, root): once per monitor
// searched, in every thread.  red / tabs / g_sh: the kernel's LDS.
template <class Src, class Put>
__device__ __forceinline__ void roots_wg_body(const double* __restrict__ D, int64_t N, const Src& r, const DevConsts& C, double* red, double* tabs, double* g_sh,
                                              Put&& put)
{
    using namespace radau;
    const Tables T = load_tables(tabs, WG_THREADS);
    const int64_t n = NF * N, l = threadIdx.x;
    const bool mine = l < N;
    const int order = r.order;
    const double t = r.t, h = r.h;
    double d[NF][MAX_ORDER + 1];
#pragma unroll
    for (int f = 0; f < NF; f++)
#pragma unroll
        for (int j = 0; j <= MAX_ORDER; j++) d[f][j] = (mine && j <= order) ? D[(int64_t)j * n + f * N + l] : 0.0;
    const double rhorat = C.hot.rhorat, presum = C.hot.presum;
    auto eval = [&](double tq, int e) -> double {
        double p[MAX_ORDER + 1];
        bdfctl::bdf_dense_weights(t, h, order, tq, p);
        double q[NQ];
        monitors_init(q);
        if (mine) {
            double u[NF];
#pragma unroll
            for (int f = 0; f < NF; f++) {
                double a = 0;
#pragma unroll
                for (int j = 0; j < MAX_ORDER; j++)
                    if (j < order) a += d[f][j + 1] * p[j];
                u[f] = a + d[f][0];
            }
            const double Phi = u[4];
            const double F = 1.0 - fast_exp(10.0 - 10.0 * rcp_nr(Phi), T);
            const double rF = rhorat * F;
            monitors_accumulate(q, u, presum + rF * (Phi * Phi * Phi) * rcp_nr(1.0 - Phi), presum - rF * Phi * Phi);
        }
        block_reduce<WG_THREADS, NQ, NQMIN>(q, red);   // (begins and ends with a barrier; the result is thread 0's)
        if (threadIdx.x == 0) {
            const double gq[7] = {q[1], q[2], q[3], q[5] - 1.0, q[6] - 1.0, q[4], q[7]};   // record_to_events (marl_api.hip)
            for (int e = 0; e < 7; e++) g_sh[e] = gq[e];
        }
        __syncthreads();
        const double ge = g_sh[e];
        __syncthreads();   // (g_sh is free for the next evaluation)
        return ge;
    };
    bdfctl::bdf_find_roots(r, eval, put);
}

// Thread 0 stores the roots: t_events [instances][7][max_events] (device).
// TERM (a sweep with terminal monitors): a listed instance whose action word has A_TERM_ROOTS is searched on its BdfTerm (t_old, t, h,
// order, active) and leaves the roots in BdfTerm::root[] - the same body; its BdfRoots is not read (there is none in a sweep without
// root slots).  Which of the two an instance is is uniform over its workgroup.  Without TERM the kernel is the body on BdfRoots alone.
template <bool TERM>
__global__ void __launch_bounds__(radau::WG_THREADS) roots_batch_kernel(const double* __restrict__ D, int64_t N, const BdfRoots* __restrict__ roots,
                                                                         double* __restrict__ t_events, const DevConsts* __restrict__ consts, BdfBatch B,
                                                                         BdfTerm* __restrict__ terms)
{
    using namespace radau;
    __shared__ double red[NQ * WG_THREADS];
    __shared__ double tabs[TABLE_DOUBLES];
    __shared__ double g_sh[7];
    const ZBatch zb = z_of(B);
    const int64_t inst = z_inst(zb);
    D = z_shift(D, zb);
    if constexpr (TERM)
        if (B.ctls[inst].action & bdfctl::A_TERM_ROOTS) {   // (uniform)
            BdfTerm& m = terms[inst];
            roots_wg_body(D, N, m, consts[inst], red, tabs, g_sh, [&](int e, double root) {
                if (threadIdx.x == 0) m.root[e] = root;
            });
            return;
        }
    const BdfRoots& r = roots[inst];
    double* out = t_events + inst * 7 * r.max_events;
    roots_wg_body(D, N, r, consts[inst], red, tabs, g_sh, [&](int e, double root) {
        if (threadIdx.x == 0) out[e * r.max_events + r.slot[e]] = root;
    });
}

// A_STOP, one workgroup per listed instance: the run ended at t_stop inside the step just accepted (a terminal monitor's root) - the
// state there, y = the step's dense output at t_stop (field-major in the instance's arena), and that state's monitors -> ctl.g.
// Thread l < N forms the five fields of cell l with the sum sample_batch_kernel writes a frame with - the same source expression,
// so that the state returned IS the frame at t_eval = t_stop, bit for bit (that kernel's comment says why each keeps its own copy) -
// then the cell's monitor terms as roots_batch_kernel's evaluation forms them, block_reduce, and thread 0 stores the seven
// monitors.  Every thread reaches every barrier; nothing waits for another workgroup; only D is read, only y and ctl.g written.
__global__ void __launch_bounds__(radau::WG_THREADS) stop_state_batch_kernel(const double* __restrict__ D, int64_t N, const BdfTerm* __restrict__ terms,
                                                                              double* __restrict__ y, const DevConsts* __restrict__ consts, BdfBatch B)
{
    using namespace radau;
    __shared__ double red[NQ * WG_THREADS];
    __shared__ double tabs[TABLE_DOUBLES];
    const Tables T = load_tables(tabs, WG_THREADS);
    const ZBatch zb = z_of(B);
    const int64_t inst = z_inst(zb);
    const BdfTerm& m = terms[inst];
    const DevConsts& C = consts[inst];
    D = z_shift(D, zb); y = z_shift(y, zb);
    const int64_t n = NF * N, l = threadIdx.x;
    const bool mine = l < N;
    const int order = m.order;
    double p[MAX_ORDER + 1];
    bdfctl::bdf_dense_weights(m.t, m.h, order, m.t_stop, p);
    const double rhorat = C.hot.rhorat, presum = C.hot.presum;
    double q[NQ];
    monitors_init(q);
    if (mine) {
        double u[NF];
#pragma unroll
        for (int f = 0; f < NF; f++) {
            double d[MAX_ORDER + 1];
#pragma unroll
            for (int j = 0; j <= MAX_ORDER; j++) d[j] = j <= order ? D[(int64_t)j * n + f * N + l] : 0.0;
            double a = 0;
#pragma unroll
            for (int j = 0; j < MAX_ORDER; j++)
                if (j < order) a += d[j + 1] * p[j];
            u[f] = a + d[0];
            y[f * N + l] = u[f];
        }
        const double Phi = u[4];
        const double F = 1.0 - fast_exp(10.0 - 10.0 * rcp_nr(Phi), T);
        const double rF = rhorat * F;
        monitors_accumulate(q, u, presum + rF * (Phi * Phi * Phi) * rcp_nr(1.0 - Phi), presum - rF * Phi * Phi);
    }
    block_reduce<WG_THREADS, NQ, NQMIN>(q, red);   // (begins and ends with a barrier; the result is thread 0's)
    if (threadIdx.x == 0) {
        const double gq[7] = {q[1], q[2], q[3], q[5] - 1.0, q[6] - 1.0, q[4], q[7]};   // record_to_events (marl_api.hip)
        BdfCtl* c = B.ctls + inst;
        for (int e = 0; e < 7; e++) c->g[e] = gq[e];
    }
}

// A_ACCEPT, one workgroup per instance: the accepted step's update of the differences and y = y_new (accept_kernel), then the norms
// of the order selection the controller asked for (want_norms) - each with the loop and the reduction tree of scaled_norm_kernel /
// scaled_norm2_kernel with one workgroup -> ctl.ss_m, ctl.ss_p.  order: the controller's (it changes in the cycle AFTER the norms).
__global__ void __launch_bounds__(1024) accept_norms_batch_kernel(double* __restrict__ D, const double* __restrict__ d, const double* __restrict__ ynew, int64_t n,
                                                                  double* __restrict__ y, BdfBatch B)
{
    __shared__ double red[1024];
    const ZBatch zb = z_of(B);
    BdfCtl* c = B.ctls + z_inst(zb);
    D = z_shift(D, zb); d = z_shift(d, zb); ynew = z_shift(ynew, zb); y = z_shift(y, zb);
    const int order = c->order, want = c->want_norms;
    const double rtol = c->rtol, atol = c->atol;
    for (int64_t i = threadIdx.x; i < n; i += 1024) {
        const double di = d[i];
        D[(int64_t)(order + 2) * n + i] = di - D[(int64_t)(order + 1) * n + i];
        D[(int64_t)(order + 1) * n + i] = di;
        double above = di;
        for (int j = order; j >= 0; j--) {
            const double v = D[(int64_t)j * n + i] + above;
            D[(int64_t)j * n + i] = v;
            above = v;
        }
        y[i] = ynew[i];
    }
    if (!want) return;   // (uniform)
    __syncthreads();     // (each thread reads back only what it wrote: i stays in its residue class; the barrier keeps the kernel plain)
    double r[2] = {0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 2; k++) {
        if (!((want >> k) & 1)) continue;   // (uniform)
        const double* v = D + (int64_t)(k ? order + 2 : order) * n;
        const double coef = k ? c->err_coef_p : c->err_coef_m;
        double ss = 0;
        for (int64_t i = threadIdx.x; i < n; i += 1024) {
            const double e = coef * v[i] / (atol + rtol * fabs(y[i]));
            ss += e * e;
        }
        __syncthreads();
        red[threadIdx.x] = ss;
        __syncthreads();
        for (int s = 512; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
            __syncthreads();
        }
        r[k] = red[0];
    }
    if (threadIdx.x == 0) {
        if (want & 1) c->ss_m = r[0];
        if (want & 2) c->ss_p = r[1];
    }
}

// A_LU: the real system  I - c J  of every listed instance - the group functions of pcr_factor_kernel / cr_init_kernel /
// cr_reduce_kernel with (mu, jscale) = (1, c) of the instance, as pcr_factor_launch(ctx, w, 1.0, {0, 0}, c, 1) passes them for one
__global__ void __launch_bounds__(256) pcr_factor_batch_kernel(const double* __restrict__ J, int64_t N, int level, radau::PcrSystem<double> Sr, BdfBatch B)
{
    using namespace radau;
    const ZBatch zb = z_of(B);
    const double jscale = B.ctls[z_inst(zb)].c;
    J = z_shift(J, zb); Sr = z_shift_system(Sr, zb);
    __shared__ PcrStage<double> stage[PCR_CELLS_PER_BLOCK];
    const int g = threadIdx.x >> 5, e = threadIdx.x & 31;
    const int64_t i = (int64_t)blockIdx.x * PCR_CELLS_PER_BLOCK + g;
    pcr_factor_group<double>(J, N, level, 1.0, Sr, stage[g], jscale, i, e);
}

__global__ void __launch_bounds__(256) cr_init_batch_kernel(const double* __restrict__ J, int64_t N, radau::CrSystem<double> Cr, BdfBatch B)
{
    using namespace radau;
    const ZBatch zb = z_of(B);
    const double jscale = B.ctls[z_inst(zb)].c;
    J = z_shift(J, zb); Cr = z_shift_cr(Cr, zb);
    __shared__ PcrStage<double> stage[PCR_CELLS_PER_BLOCK];
    const int g = threadIdx.x >> 5, e = threadIdx.x & 31;
    const int64_t i = (int64_t)blockIdx.x * PCR_CELLS_PER_BLOCK + g;
    cr_init_group<double>(J, N, 1.0, jscale, Cr, stage[g], i, e);
}

__global__ void __launch_bounds__(256) cr_reduce_batch_kernel(radau::CrSystem<double> Cr, radau::CrShape sh, int last, radau::PcrSystem<double> Sr, BdfBatch B)
{
    using namespace radau;
    const ZBatch zb = z_of(B);
    Cr = z_shift_cr(Cr, zb); Sr = z_shift_system(Sr, zb);
    __shared__ PcrStage<double> stage[PCR_CELLS_PER_BLOCK];
    const int g = threadIdx.x >> 5, e = threadIdx.x & 31;
    const int64_t i = (int64_t)blockIdx.x * PCR_CELLS_PER_BLOCK + g;
    double *Ln = last ? Sr.L[0] : Cr.L + sh.off_next * 25, *Dn = last ? Sr.D[0] : Cr.D + sh.off_next * 25;
    double *Un = last ? Sr.U[0] : Cr.U + sh.off_next * 25, *In = last ? Sr.Dinv[0] : Cr.Dinv + sh.off_next * 25;
    cr_reduce_group<double>(1.0, Cr, sh, last != 0, Ln, Dn, Un, In, stage[g], i, e);
}

// A_SOLVE: solve_bdf_system of every listed instance, one workgroup each - the single run's body with the scalars of the instance's
// controller; what the single run's kernel writes into the zero-copy words goes into the controller
template <bool VD>
__global__ void __launch_bounds__(radau::WG_THREADS) solve_batch_kernel(const double* __restrict__ D, Vec6 gamma, double* __restrict__ ypred, double* __restrict__ psi,
                                                                         double* __restrict__ scale, double* __restrict__ ynew, double* __restrict__ d,
                                                                         double* __restrict__ f, int64_t N, int nlevels, radau::PcrSystem<double> Sr,
                                                                         const DevConsts* __restrict__ consts, radau::CrPlan pl, radau::CrSystem<double> Cr, BdfBatch B)
{
    using namespace radau;
    const ZBatch zb = z_of(B);
    const int64_t inst = z_inst(zb);
    BdfCtl* c = B.ctls + inst;
    D = z_shift(D, zb); ypred = z_shift(ypred, zb); psi = z_shift(psi, zb); scale = z_shift(scale, zb); ynew = z_shift(ynew, zb); d = z_shift(d, zb); f = z_shift(f, zb);
    Sr = z_shift_system(Sr, zb); Cr = z_shift_cr(Cr, zb);
    const SolveOut r = solve_wg_body<VD>(c->mode, D, c->order, gamma, c->alpha_order, ypred, psi, scale, ynew, d, f, N, c->c, nlevels, Sr, consts[inst], c->newton_tol,
                                         c->err_coef, c->rtol, c->atol, pl, Cr);
    if (threadIdx.x == 0) {
        c->iters = r.iters;
        c->converged = r.converged;   // (0 when f was not finite: the iteration was abandoned, bdf.py:44-45)
        c->dy_ss = r.dy_ss;
        c->err_ss = r.err_ss;
        if (r.converged)
            for (int e = 0; e < 7; e++) c->g_new[e] = r.g_new[e];
    }
}

}  // namespace bdf
}  // namespace marl
