// marl_bdf_ctl.h - the step logic of scipy's BDF (scipy/integrate/_ivp/bdf.py:310-450 inside the solve_ivp loop, ivp.py:654-723; restated
// for one instance in marl_api.hip, bdf_run) as a RESUMABLE state machine for the BDF sweep (marl_bdf_batch.h): bdf_control_step runs
// one instance's scalar logic up to the next point where it needs a result of data-parallel work, publishes everything that needs no
// scalar decision in between as ONE action word (A_* bits) and resumes in the next cycle with the kernels' results.  The work of an
// action word is done in this fixed order (the host cycle's launch order, and what a CPU driver of this header has to do):
//     A_ACCEPT (+ the order-selection norms asked for by `want_norms`)  ->  A_CHANGE_D (RU, ru_order)  ->  A_JAC (f and J at y_predict)
//     ->  A_LU (I - c J)  ->  A_SOLVE (solve_bdf_system; mode 0: predictor first, 1: restart from y_predict)
// so that an accepted step without order selection costs one cycle (accept | solve of the next step) and one with it two.
//
// t_eval samples (the sampling form of bdf_control_step: BdfSample, one per instance beside its BdfCtl, and the shared sample times).
// scipy builds a step's dense output after _step_impl has returned (bdf.py:452-454), so a sample reads D[:order + 1], the order and
// h_abs AFTER the order / step-size selection and its change_D, and BEFORE the next step rescales D again (min_step in PC_STEP, the
// clipping at t_bound in PC_ATTEMPT).  An accepted step that covers a pending sample (t_eval[next] <= t) therefore snapshots
// (t, h = S_h_abs, order, [first, end) of its samples) at PC_STEP_END, sets A_SAMPLE and YIELDS there: the cycle's work becomes
//     A_ACCEPT  ->  A_CHANGE_D (the selection's)  ->  A_SAMPLE (D[0] + sum_j D[j + 1] p[j], bdf_dense_weights)
// and the next step's logic, with whatever rescaling it asks for, starts in the following cycle.  Only steps that hold samples pay
// that cycle (at most n_eval per instance); the last step's samples are published in the cycle that reaches PC_DONE; a run that
// ends with status -1 or 2 does so in PC_ATTEMPT of a later cycle and keeps the samples it has written.  Without a BdfSample, or with
// n_eval = 0, the action words and their cycles are those of the three-argument call.
//
// Root times of the monitors (BdfRoots, a third per-instance struct; A_ROOTS; bdf_locate_roots).  solve_ivp finds the roots of the events
// that changed sign over an accepted step on the same dense output, before it takes the t_eval samples (ivp.py:673-694, 706-723).  At
// acceptance (PC_SOLVED), where the sign changes are counted, every monitor that changed sign and whose count is still below max_events
// is marked pending with that count as its slot, and the step's start is kept; the marks survive PC_SELECT.  At PC_STEP_END a step
// with pending monitors snapshots (t_old, t, h = S_h_abs, order), sets A_ROOTS and yields exactly as a step with samples does (one
// shared extra cycle when it has both), so that a cycle's work reads
//     A_ACCEPT  ->  A_CHANGE_D  ->  A_ROOTS  ->  A_SAMPLE  ->  A_JAC  ->  A_LU  ->  A_SOLVE
// (events before t_eval, as in scipy; both only read D).  The last step's roots go out in the cycle that reaches PC_DONE, a run that
// ends with status -1 or 2 keeps the roots it has, t1 == t0 has none.  Without a BdfRoots, or with max_events <= 0, the action words,
// the cycles and the controller's bytes are those of the calls without it; n_events counts every sign change either way.
//
// Terminal monitors (BdfTerm, a fourth per-instance struct; A_TERM_ROOTS, A_STOP; the rule: marl_terminal.h, ivp.py:79-130, 681-723).
// At acceptance (PC_SOLVED) a step over which a monitor changed sign that thereby meets its limit is a TERMINAL STEP: all monitors that
// changed sign are recorded in BdfTerm::active, the step's start is kept, and none of the step's sign changes is counted or marked for
// A_ROOTS yet - which of them happened is known only once their roots are.  At PC_STEP_END such a step snapshots its dense output
// where A_ROOTS and A_SAMPLE do, sets A_TERM_ROOTS - the roots of every monitor of `active` -> BdfTerm::root[], with or without root
// slots - and yields:
//     A_ACCEPT  ->  A_CHANGE_D  ->  A_TERM_ROOTS
// The next cycle (PC_TERM) runs terminal_select on those roots: the monitors it keeps are counted and, where a BdfRoots has a free
// slot, their roots stored into t_events by the controller itself; the ones after the terminal monitor never happened.  Then
// c.t = t_stop, A_SAMPLE for the samples t_eval[k] <= t_stop (BdfSample::t stays the STEP's end: it is the dense output's t), A_STOP -
// y = the dense output at t_stop, sample_batch_kernel's sum, and c.g = that state's monitors - status 1 and PC_DONE, all in that cycle:
//     A_SAMPLE  ->  A_STOP
// (both only read D; nothing rescales it any more).  One extra cycle per stopped instance.  Every other step, a run that ends with
// status -1 or 2, and t1 == t0 are untouched; without a BdfTerm the action words, cycles and bytes are those of the calls without it.
// f(t0, y0), the first Jacobian, D[0] = y0, D[1] = f h and the monitors of y0 (BDF.__init__) are done before the first cycle.
// Like marl_brent.h: nothing but <math.h> / <stdint.h> (and marl_brent.h, marl_terminal.h), so that a host C++ compiler builds this header alone
// (tests/test_bdf_control_cpu.py holds it to scipy's solve_ivp(method="BDF") that way).
#pragma once
#include <math.h>
#include <stdint.h>

#include "marl_brent.h"
#include "marl_terminal.h"

#ifdef __HIPCC__
#define MARL_BDF_FN __host__ __device__ __forceinline__
#else
#define MARL_BDF_FN inline
#endif

namespace marl {
namespace bdfctl {

constexpr int MAX_ORDER = 5, NEWTON_MAXITER = 4;
constexpr double MIN_FACTOR = 0.2, MAX_FACTOR = 10;

enum : int32_t { A_ACCEPT = 1, A_CHANGE_D = 2, A_JAC = 4, A_LU = 8, A_SOLVE = 16, A_SAMPLE = 32, A_ROOTS = 64, A_TERM_ROOTS = 128, A_STOP = 256 };
enum : int32_t { PC_INIT = 0, PC_STEP, PC_ATTEMPT, PC_SOLVED, PC_SELECT, PC_STEP_END, PC_DONE, PC_TERM };

struct BdfCtl {
    // set once
    double t_bound, rtol, atol, newton_tol;
    int64_t max_attempts;
    // BDF._step_impl state
    double t, S_h_abs, h_abs, min_step, h, t_new, error_norm, safety;
    double g[7];                       // the monitors of the last accepted state
    int64_t n_events[7];
    int64_t nfev, njev, nlu, n_acc, n_rej, attempts;
    int32_t action;                    // A_* bits: the work of this cycle
    int32_t pc, status;
    int32_t order, n_equal_steps, have_lu, current_jac, n_iter;
    // what the kernels of this cycle read
    int32_t mode;                      // A_SOLVE: 0 = predictor first, 1 = restart from y_predict
    int32_t want_norms;                // A_ACCEPT: bit 0 = the norm of error_const[order - 1] D[order], bit 1 = of error_const[order + 1] D[order + 2]
    int32_t ru_order, pad;             // A_CHANGE_D: D[:ru_order + 1] = RU^T D[:ru_order + 1]
    double c;                          // h / alpha[order]
    double alpha_order, err_coef;      // alpha[order], error_const[order] of the solve
    double err_coef_m, err_coef_p;     // error_const[order -+ 1] of the order selection
    double RU[MAX_ORDER + 1][MAX_ORDER + 1];
    double ru_factor;                  // (the factor RU was built from: for the record)
    // what the kernels leave
    int32_t iters, converged;          // A_SOLVE: function evaluations; converged (0 too when f was not finite)
    double dy_ss, err_ss;              // sum (dy / scale)^2 of the last iteration; sum (error_const[order] d / scale)^2 of the converged state
    double g_new[7];                   // the monitors of the converged state
    double ss_m, ss_p;                 // A_ACCEPT: the two sums of want_norms
};

// The t_eval state of one instance: a parallel array beside the controllers (BdfCtl keeps its layout).
struct BdfSample {
    int64_t n_eval, next;              // samples asked for; the first one not yet written (at the end: the frames of the instance)
    // A_SAMPLE: the dense output of the step just accepted and the samples [first, end) it covers
    double t, h;                       // the step's end and S_h_abs after the selection (BdfDenseOutput's t, h)
    int64_t first, end;
    int32_t order, pad;
};

// The root-location state of one instance: a third parallel array (BdfCtl and BdfSample keep their layouts).
struct BdfRoots {
    int64_t max_events;                // roots kept per monitor (<= 0: none are located)
    // A_ROOTS: the dense output of the step just accepted (BdfDenseOutput's t_old, t, h, order) and the monitors to search on it
    double t_old, t, h;                // the step's start (kept at acceptance), its end and S_h_abs after the selection
    int32_t order;
    int32_t pending;                   // bit e: monitor e changed sign over the accepted step (set at acceptance, taken at PC_STEP_END)
    int32_t mask, pad;                 // bit e: monitor e is searched in this cycle
    int64_t slot[7];                   // monitor e's root goes to t_events[e * max_events + slot[e]]: its count before this sign change
};

// The terminal-monitor state of one instance: a fourth parallel array (BdfCtl, BdfSample and BdfRoots keep their layouts).
struct BdfTerm {
    int64_t terminal[7];               // monitor e ends the run at its terminal[e]-th occurrence (0: never)
    double root[7];                    // A_TERM_ROOTS: the root of every monitor of `active` over the terminal step
    // the dense output of the terminal step (BdfDenseOutput's t_old, t, h, order)
    double t_old, t, h;                // the step's start (kept at acceptance), its end and S_h_abs after the selection
    double t_stop;                     // the terminal monitor's root: where the run ended
    int32_t order;
    int32_t active;                    // bit e: monitor e changed sign over the terminal step (0: no terminal step so far)
    int32_t stopped, pad;              // 1: the run was stopped at t_stop
};

MARL_BDF_FN double kappa_of(int k) { return k == 1 ? -0.1850 : k == 2 ? -1.0 / 9 : k == 3 ? -0.0823 : k == 4 ? -0.0415 : 0.0; }
MARL_BDF_FN double gamma_of(int k)   // gamma = hstack((0, cumsum(1 / arange(1, MAX_ORDER + 1))))
{
    double g = 0;
    for (int j = 1; j <= k; j++) g = g + 1.0 / j;
    return g;
}
MARL_BDF_FN double alpha_of(int k) { return (1 - kappa_of(k)) * gamma_of(k); }
MARL_BDF_FN double error_const_of(int k) { return kappa_of(k) * gamma_of(k) + 1.0 / (k + 1); }

// compute_R (bdf.py:18-25).  R U has entries that cancel to zero in exact arithmetic, so the roundings are spelled out: numpy's
// (i - 1 - factor j) / i with every operation rounded, and below R.dot(U) as its BLAS sums it (a chain of fused multiply-adds over
// ascending k) - with both, RU is numpy's bit for bit and the CPU test's runs take scipy's steps to the last bit.
MARL_BDF_FN void compute_R(int order, double factor, double (&R)[MAX_ORDER + 1][MAX_ORDER + 1])
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    for (int j = 0; j <= order; j++) R[0][j] = 1;
    for (int i = 1; i <= order; i++) {
        R[i][0] = 0;
        for (int j = 1; j <= order; j++) R[i][j] = R[i - 1][j] * ((i - 1 - factor * j) / i);
    }
}

// change_D (bdf.py:28-33): the product R U of the rescaling by `factor`, left in the controller for the kernel (A_CHANGE_D)
MARL_BDF_FN void request_change_D(BdfCtl& c, double factor)
{
    double R[MAX_ORDER + 1][MAX_ORDER + 1], U[MAX_ORDER + 1][MAX_ORDER + 1];
    const int order = c.order;
    compute_R(order, factor, R);
    compute_R(order, 1.0, U);
    for (int i = 0; i <= order; i++)
        for (int j = 0; j <= order; j++) {
            double a = 0;
            for (int k = 0; k <= order; k++) a = fma(R[i][k], U[k][j], a);
            c.RU[i][j] = a;
        }
    c.ru_order = order;
    c.ru_factor = factor;
    c.action |= A_CHANGE_D;
}

// BdfDenseOutput (bdf.py:456-478) of the step that ended at `t` with step size `h`: p = cumprod((tq - (t - h j)) / (h (1 + j))), j < order;
// the sample is D[0] + sum_j D[j + 1] p[j].  Every operation rounded on its own, as numpy does them (and bdf_dense on the host).
MARL_BDF_FN void bdf_dense_weights(double t, double h, int order, double tq, double (&p)[MAX_ORDER + 1])
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double acc = 1;
    for (int j = 0; j <= MAX_ORDER; j++) {
        if (j < order) acc *= (tq - (t - h * j)) / (h * (1 + j));
        p[j] = j < order ? acc : 0.0;
    }
}

// A controller at (t0, first_step) in front of its first cycle.  rtol: already clamped to 100 eps (ivp's validate_tol).
MARL_BDF_FN void bdf_control_init(BdfCtl& c, double t0, double t1, double first_step, double rtol, double atol, int64_t max_attempts)
{
    c = BdfCtl{};
    c.t_bound = t1; c.rtol = rtol; c.atol = atol; c.max_attempts = max_attempts;
    c.newton_tol = fmax(10 * 2.220446049250313e-16 / rtol, fmin(0.03, sqrt(rtol)));
    c.t = t0; c.S_h_abs = first_step;
    c.order = 1;
    c.pc = PC_INIT; c.status = 1;
}

MARL_BDF_FN void bdf_sample_init(BdfSample& s, int64_t n_eval)
{
    s = BdfSample{};
    s.n_eval = n_eval;
}

MARL_BDF_FN void bdf_roots_init(BdfRoots& r, int64_t max_events)
{
    r = BdfRoots{};
    r.max_events = max_events;
}

MARL_BDF_FN void bdf_term_init(BdfTerm& m, const int64_t terminal[7])
{
    m = BdfTerm{};
    for (int e = 0; e < 7; e++) m.terminal[e] = terminal[e];
}

// A_ROOTS, the search itself (solve_event_equation, ivp.py:51-76, as accepted_step_epilogue in marl_api.hip runs it for a single run):
// for every monitor of the search's mask in ascending e over its [t_old, t] - `src` says where the three come from: a BdfRoots (A_ROOTS:
// mask) or a BdfTerm (A_TERM_ROOTS: active), read where it lies each time (on the device that is global memory, not registers) - a search of its own - both end values from the dense output (not the stored g), then the
// exact sequence of brent_root: an end point whose value is zero as it is, otherwise brent_advance / evaluate for at most 100 passes and
// the last iterate.  Equal signs at both ends are no special case (the loop is bounded).  eval(tq, e): monitor e of the step's
// dense output at tq.  put(e, root): called once for every monitor searched.
// On the device every thread of a workgroup runs this redundantly on the same values (eval holds the barriers): the control flow
// depends on nothing but src and what eval returns.
MARL_BDF_FN int32_t search_mask(const BdfRoots& r) { return r.mask; }
MARL_BDF_FN int32_t search_mask(const BdfTerm& m) { return m.active; }
template <class Src, class Eval, class Put>
MARL_BDF_FN void bdf_find_roots(const Src& src, Eval&& eval, Put&& put)
{
#if defined(__clang__)
#pragma clang loop unroll(disable)
#endif
    for (int e = 0; e < 7; e++) {
        if (!((search_mask(src) >> e) & 1)) continue;
        const double fa = eval(src.t_old, e), fb = eval(src.t, e);
        if (fa == 0) { put(e, src.t_old); continue; }
        if (fb == 0) { put(e, src.t); continue; }
        BrentState s = {src.t_old, src.t, 0, fa, fb, 0, 0, 0};
        for (int it = 0; it < 100; it++) {
            if (brent_advance(s)) break;
            s.fcur = eval(s.xcur, e);
        }
        put(e, s.xcur);
    }
}

// The same with the roots stored: t_events = the instance's [7][max_events] root times.
template <class Eval>
MARL_BDF_FN void bdf_locate_roots(const BdfRoots& r, Eval&& eval, double* t_events)
{
    bdf_find_roots(r, eval, [&](int e, double root) { t_events[e * r.max_events + r.slot[e]] = root; });
}

// A_TERM_ROOTS: the roots of every monitor that changed sign over the terminal step -> m.root[]
template <class Eval>
MARL_BDF_FN void bdf_locate_term_roots(BdfTerm& m, Eval&& eval)
{
    bdf_find_roots(m, eval, [&](int e, double root) { m.root[e] = root; });
}

// One instance from where it stopped to its next action word.  n: unknowns (5 N).  g0: the seven monitors of y0 (read at PC_INIT only).
// s, t_eval: the instance's sampling state and the n_eval sorted sample times (NULL: no samples).
// r: the instance's root-location state (NULL, or max_events <= 0: sign changes are counted only).
// m: the instance's terminal-monitor state (NULL: no monitor ends the run); t_events: the instance's [7][max_events] root times, where
// the controller stores the kept roots of the terminal step (NULL, or no r: they are counted only).
MARL_BDF_FN void bdf_control_step(BdfCtl& c, int64_t n, const double* g0, BdfSample* s = nullptr, const double* t_eval = nullptr, BdfRoots* r = nullptr,
                                  BdfTerm* m = nullptr, double* t_events = nullptr)
{
    c.action = 0;
    int pc = c.pc;
    // a small interpreter: `continue` = go on with the new pc in this cycle, `break` out of the loop = yield
    for (int guard = 0; guard < 64; guard++) {
        if (pc == PC_INIT) {                      // BDF.__init__: f = fun(t0, y0), J = jac(t0, y0), D[0] = y0, D[1] = f h - done before the first cycle
            for (int e = 0; e < 7; e++) c.g[e] = g0[e];
            c.nfev = 1; c.njev = 1;
            c.order = 1; c.n_equal_steps = 0; c.have_lu = 0;
            pc = PC_STEP;
            continue;
        }
        if (pc == PC_STEP) {                      // top of _step_impl
            if (c.t == c.t_bound) { c.status = 0; pc = PC_DONE; break; }
            c.min_step = 10 * fabs(nextafter(c.t, __builtin_inf()) - c.t);
            if (c.S_h_abs < c.min_step) {
                if (c.action & A_CHANGE_D) break;   // one rescaling of D per cycle: come back here once the pending one is done
                c.h_abs = c.min_step;
                request_change_D(c, c.min_step / c.S_h_abs);
                c.n_equal_steps = 0;
            } else {
                c.h_abs = c.S_h_abs;
            }
            c.current_jac = 0;
            pc = PC_ATTEMPT;
            continue;
        }
        if (pc == PC_ATTEMPT) {                   // top of `while not step_accepted`
            if (c.h_abs < c.min_step) { c.status = -1; pc = PC_DONE; break; }
            if (c.max_attempts > 0 && c.attempts >= c.max_attempts) { c.status = 2; pc = PC_DONE; break; }
            double t_new = c.t + c.h_abs;
            if (t_new - c.t_bound > 0) {          // clipping at t_bound
                if (c.action & A_CHANGE_D) break;
                t_new = c.t_bound;
                request_change_D(c, fabs(t_new - c.t) / c.h_abs);
                c.n_equal_steps = 0;
                c.have_lu = 0;
            }
            c.attempts++;
            c.t_new = t_new;
            c.h = t_new - c.t;
            c.h_abs = fabs(c.h);
            c.alpha_order = alpha_of(c.order);
            c.err_coef = error_const_of(c.order);
            c.c = c.h / c.alpha_order;
            if (!c.have_lu) { c.action |= A_LU; c.nlu++; c.have_lu = 1; }   // LU = self.lu(self.I - c * J)
            c.mode = 0;
            c.action |= A_SOLVE; pc = PC_SOLVED;
            break;
        }
        if (pc == PC_SOLVED) {                    // the result of solve_bdf_system
            c.nfev += c.iters;
            c.n_iter = c.iters;
            if (!c.converged) {
                if (c.current_jac) {              // the step failed: halve
                    c.h_abs *= 0.5;
                    request_change_D(c, 0.5);
                    c.n_equal_steps = 0;
                    c.have_lu = 0;
                    c.n_rej++;
                    pc = PC_ATTEMPT;
                    continue;
                }
                c.njev++;                         // J = self.jac(t_new, y_predict); LU = None; the solve starts again from y_predict
                c.current_jac = 1;
                c.nlu++; c.have_lu = 1;
                c.mode = 1;
                c.action = A_JAC | A_LU | A_SOLVE; pc = PC_SOLVED;
                break;
            }
            c.safety = 0.9 * (2 * NEWTON_MAXITER + 1) / (2 * NEWTON_MAXITER + c.n_iter);
            c.error_norm = sqrt(c.err_ss) / sqrt((double)n);
            if (c.error_norm > 1) {               // (the LU is kept)
                const double sf = c.safety * pow(c.error_norm, -1.0 / (c.order + 1));
                const double factor = (sf > MIN_FACTOR) ? sf : MIN_FACTOR;
                c.h_abs *= factor;
                request_change_D(c, factor);
                c.n_equal_steps = 0;
                c.n_rej++;
                pc = PC_ATTEMPT;
                continue;
            }
            // accepted
            c.n_equal_steps++;
            const double t_old = c.t;
            c.t = c.t_new;
            c.S_h_abs = c.h_abs;
            c.n_acc++;
            bool term = false;                    // a terminal step (ivp.py:681-704): its sign changes are counted at PC_TERM, once their roots say which happened
            if (m) {
                int32_t active = 0;
                for (int e = 0; e < 7; e++) {
                    const bool up = c.g[e] <= 0 && c.g_new[e] >= 0, down = c.g[e] >= 0 && c.g_new[e] <= 0;
                    if (up || down) {
                        active |= 1 << e;
                        if (terminal_met(c.n_events[e] + 1, m->terminal[e])) term = true;
                    }
                }
                if (term) { m->active = active; m->t_old = t_old; }
            }
            for (int e = 0; e < 7; e++) {         // non-terminal events, both directions (ivp.py:131-156): counted; located at PC_STEP_END (r)
                const bool up = c.g[e] <= 0 && c.g_new[e] >= 0, down = c.g[e] >= 0 && c.g_new[e] <= 0;
                if ((up || down) && !term) {
                    if (r && c.n_events[e] < r->max_events) {   // (max_events <= 0: never)
                        r->pending |= 1 << e;
                        r->slot[e] = c.n_events[e];
                        r->t_old = t_old;
                    }
                    c.n_events[e]++;
                }
                c.g[e] = c.g_new[e];
            }
            c.action = A_ACCEPT;
            c.want_norms = 0;
            if (c.n_equal_steps < c.order + 1) { pc = PC_STEP_END; continue; }
            if (c.order > 1) { c.want_norms |= 1; c.err_coef_m = error_const_of(c.order - 1); }
            if (c.order < MAX_ORDER) { c.want_norms |= 2; c.err_coef_p = error_const_of(c.order + 1); }
            pc = PC_SELECT;
            break;
        }
        if (pc == PC_SELECT) {                    // order / step-size selection (bdf.py:427-448) with the two norms
            const double em = (c.want_norms & 1) ? sqrt(c.ss_m) / sqrt((double)n) : __builtin_inf();
            const double ep = (c.want_norms & 2) ? sqrt(c.ss_p) / sqrt((double)n) : __builtin_inf();
            const double en[3] = {em, c.error_norm, ep};
            double factors[3];
            int best = 0;
            for (int i = 0; i < 3; i++) {
                factors[i] = pow(en[i], -1.0 / (c.order + i));
                if (factors[i] > factors[best]) best = i;
            }
            for (int i = 0; i < 3; i++)
                if (factors[i] != factors[i]) { best = i; break; }   // np.argmax: the first NaN
            c.order += best - 1;
            const double sf = c.safety * factors[best];
            const double factor = (sf < MAX_FACTOR) ? sf : MAX_FACTOR;   // python's min(MAX_FACTOR, x): a NaN x yields MAX_FACTOR
            c.S_h_abs *= factor;
            request_change_D(c, factor);
            c.n_equal_steps = 0;
            c.have_lu = 0;
            c.want_norms = 0;
            pc = PC_STEP_END;
            continue;
        }
        if (pc == PC_STEP_END) {                  // the solve_ivp loop (ivp.py:667-668)
            if (m && m->active) {                 // a terminal step: its dense output, as A_ROOTS and A_SAMPLE below snapshot it
                m->t = c.t; m->h = c.S_h_abs; m->order = c.order;
                c.action |= A_TERM_ROOTS;
                pc = PC_TERM;
                break;
            }
            bool sampled = false;                 // (or searched for roots: the cycle ends here either way)
            if (r && r->pending) {                // ivp.py:673-694: the roots of this step, on the dense output the samples below read
                r->mask = r->pending;
                r->pending = 0;
                r->t = c.t; r->h = c.S_h_abs; r->order = c.order;
                c.action |= A_ROOTS;
                sampled = true;
            }
            if (s && s->next < s->n_eval && t_eval[s->next] <= c.t) {   // ivp.py:706-723: searchsorted(t_eval, t, side="right")
                s->t = c.t; s->h = c.S_h_abs; s->order = c.order;
                s->first = s->next;
                int64_t e = s->next + 1;
                while (e < s->n_eval && t_eval[e] <= c.t) e++;
                s->end = s->next = e;
                c.action |= A_SAMPLE;
                sampled = true;
            }
            if (c.t - c.t_bound >= 0) { c.status = 0; pc = PC_DONE; break; }
            pc = PC_STEP;
            if (sampled) break;                   // the next step may rescale D: not in the cycle that reads it
            continue;
        }
        if (pc == PC_TERM) {                      // the roots of the terminal step are in m->root: handle_events (ivp.py:79-130, 696-704)
            int64_t counts[7];
            for (int e = 0; e < 7; e++) counts[e] = c.n_events[e] + 1;
            uint32_t keep = 0;
            double t_stop = m->t;
            terminal_select((uint32_t)m->active, m->root, counts, m->terminal, &keep, &t_stop);
            for (int e = 0; e < 7; e++) {
                if (!((keep >> e) & 1)) continue;
                if (r && t_events && c.n_events[e] < r->max_events) t_events[e * r->max_events + c.n_events[e]] = m->root[e];
                c.n_events[e]++;
            }
            m->t_stop = t_stop;
            m->stopped = 1;
            c.t = t_stop;
            if (s && s->next < s->n_eval && t_eval[s->next] <= t_stop) {   // the samples up to t_stop, from the terminal step's dense output
                s->t = m->t; s->h = m->h; s->order = m->order;
                s->first = s->next;
                int64_t e = s->next + 1;
                while (e < s->n_eval && t_eval[e] <= t_stop) e++;
                s->end = s->next = e;
                c.action |= A_SAMPLE;
            }
            c.action |= A_STOP;
            c.status = 1; pc = PC_DONE;
            break;
        }
        break;
    }
    c.pc = pc;
}

}  // namespace bdfctl
}  // namespace marl
