// marl_dop853.h - the native DOP853 loops (gfx950): scipy's DOP853 (scipy/integrate/_ivp/rk.py, class DOP853: Dormand-Prince 8(5,3)) for
// grids that fit one workgroup (N <= BLK cells, one cell per thread, one workgroup per instance), on the stencil engine, the monitors,
// the reductions, the Brent state machine and the step controller record of the RK45 kernels (marl_kernels.h).
//
// Shared with RK45 / RK23: StencilBlock and everything under it, load_cells, Rk45Ctrl and rk45_init_kernel (they hold no method constant),
// the monitors and their record (monitors_accumulate, rk45_monitor_of_record), the event bookkeeping (rk45_events), block_reduce,
// brent_advance.  NOT shared: the loop.  rk45_sweep_body keeps a step's stage derivatives in registers, carries ONE error sum through
// its record and seven dense-output weights through its scalars; DOP853 has 12 stages (16 with the dense output's), two error sums
// and 16 weights, so it has a body of its own (dop853_sweep_body), built for being right and small first:
//
//   * The stage derivatives K_1..K_16 live in a per-instance arena in global memory, [slot][field][thread]: every thread reads and
//     writes its own column only (coalesced, and no barrier orders it: a thread sees its own stores), the stage loop is a RUN-TIME loop
//     over the tableau's rows (dop853_row; zero coefficients skipped, the others summed left to right) around ONE inlined evaluation, and
//     nothing of the 12 x 5 derivatives sits in registers - the 1024-thread window, capped at 128 VGPRs, is as free of stage spills as
//     the 256-thread one.  What it costs is memory traffic per evaluation: DESIGN.md, section DOP853.
//   * The controller is Rk45Ctrl in LDS, run by thread 0 between barriers (the shape of rk45_sweep_body<FAST = false>).  Thread 0 also
//     says what the next trip of the loop is, through a small descriptor in LDS (Dop853Trip) that every thread reads behind one barrier:
//     an ATTEMPT, the replay of the step just accepted for a t_eval SAMPLE, or its replay for a PROBE of Brent's method.  Whether a trip
//     is one or the other therefore follows from ONE value that all waves read from the same address behind a barrier - every barrier
//     of a trip is reached by every wave or by none.
//   * A replay runs the 12 stages again on the same (y, K_1, h) - the same instructions on the same numbers: the same y_new and K_13,
//     bit for bit - then the three extra stages of the dense output (rk.py:520-535), and forms  y + h sum_j w_j K_j  with the 16
//     weights of dop853_dense_weights.  It decides nothing and counts nothing; the accepted step is committed (y <- y_new,
//     K_1 <- K_13) when its roots and samples are done.
//   * Two error sums: the 8-slot record reduction carries sum (err5 / scale)^2 in its sum slot beside the seven monitors of y_new;
//     sum (err3 / scale)^2 is butterflied per wave and added in wave order by thread 0, behind the same barriers.
//   * nfev: 12 per attempt, and 3 more for every accepted step with a monitor sign change or a sample in it
//     (dop853_count_dense_output) - what solve_ivp(method="DOP853", events=<the seven monitors>, t_eval=...) reports.
//
//   * Terminal monitors (TERM; dop853_sweep_stop_kernel): a fourth trip kind, the STOP - one more replay of the step that ends the run,
//     at the terminal monitor's root, whose result becomes the state - and a stop record in LDS that only that kernel has
//     (marl_dop853_stop.h; see dop853_control).  Without TERM the body is what it was, instruction for instruction.
//
// Every loop ends on its own: a NaN error norm is a rejection with MIN_FACTOR until the step falls below 10 ulp(t) (ST_TOO_SMALL),
// max_attempts gives ST_BUDGET, Brent's iteration is capped at 100 as everywhere (for each of at most seven monitors), the samples of
// a step are finitely many, and the STOP trip leaves the loop.
//
// Compiled as two translation units: marl_dop853.hip (the plain, eval and roots kernels) and marl_dop853_stop.hip (the stop kernel),
// which leaves the code generation of the other units, and of each other, alone.
#pragma once
#include "marl_kernels.h"
#include "marl_dop853_ctl.h"
#include "marl_dop853_stop.h"

namespace marl {

constexpr int DOP853_SLOTS = dop853::N_STAGES_EXTENDED;   // K_1..K_16 of a cell and field
constexpr int DOP853_BATCH = 4;                            // stage derivatives loaded together in a stage sum
static_assert(dop853::N_STAGES % DOP853_BATCH == 0, "the error sums walk K_1..K_12 in whole batches");

// doubles of the arena of `batch` instances at a BLK-thread window
__host__ __device__ constexpr int64_t dop853_arena_doubles(int64_t batch, int blk) { return batch * DOP853_SLOTS * NF * blk; }

enum : int { DOP853_ATTEMPT = 0, DOP853_SAMPLE = 1, DOP853_PROBE = 2, DOP853_STOP = 3 };
static_assert(DOP853_NEXT_SAMPLE == DOP853_SAMPLE && DOP853_NEXT_PROBE == DOP853_PROBE && DOP853_NEXT_STOP == DOP853_STOP,
              "dop853_stop_next (marl_dop853_stop.h) answers in trip kinds");

// What thread 0 asks of the next trip of the loop (LDS; read by every thread behind a barrier).
struct Dop853Trip {
    double h;          // the step: h_try of an attempt, h_prev of a replay
    double w[16];      // replay: the dense-output weights at its abscissa
    int64_t ie;        // SAMPLE: the frame to write
    int32_t kind;      // DOP853_* (DOP853_STOP: the stop kernel only)
    int32_t at_start;  // replay at t_old itself: the result is y_old, whatever 0 * K_j gives
    int32_t commit;    // first: y <- y_new, K_1 <- K_13 (the step accepted before is complete)
    int32_t leave;     // then: leave the loop
};

// What thread 0 carries from trip to trip (LDS, beside the controller): where it stands in the step just accepted.
struct Dop853Walk {
    int64_t ie;                          // the next sample, t_eval[ie]
    int32_t counted;                     // the dense output of the step just accepted is counted (dop853_count_dense_output)
    int32_t ev_mask;                     // monitors of that step still to be located (bit e)
    int32_t br_e, br_phase, br_iter;     // the monitor being located; phase 1 f(a) asked, 2 f(b) asked, 3 iterating
    double br_fa;
    BrentState bs;
};
struct Dop853Record { double q[NQ]; double s3; };   // the reduced record of a trip: {sum (err5 / scale)^2, monitors}, sum (err3 / scale)^2
// TERM: what thread 0's functions get beside the walk - the stop record (Dop853Stop, marl_dop853_stop.h; LDS of the stop kernel).
// Without TERM there is nothing to hand over: an empty argument, which costs the three older kernels no register and no instruction.
template <bool TERM> struct Dop853StopRef {};
template <> struct Dop853StopRef<true> { Dop853Stop* rec; };

// the next trip replays the step just accepted at time tp
__device__ __forceinline__ void dop853_replay_at(Rk45Ctrl& sc, Dop853Trip& trip, Dop853Walk& st, int kind, double tp)
{
    double w[16];
    dop853_dense_weights((tp - sc.t_old) / sc.h_prev, w);
    for (int j = 0; j < 16; j++) trip.w[j] = w[j];
    trip.kind = kind;
    trip.h = sc.h_prev;
    trip.at_start = tp == sc.t_old;
    trip.commit = 0;
    trip.leave = 0;
    if (!st.counted) {
        dop853_count_dense_output(sc);
        st.counted = 1;
    }
}

// what follows in the step just accepted: roots (Brent on the lowest monitor of ev_mask over [t_old, t]: f(a) first), then samples,
// then the commit and the next attempt - or the way out.  TERM, in a step that ends the run (its roots located and the rule applied:
// DOP853_STOP_SAMPLES): the samples up to t_stop, then the STOP trip - no commit, no further attempt.
template <bool EVAL, bool ROOTS, bool TERM = false>
__device__ __forceinline__ void dop853_schedule(Rk45Ctrl& sc, Dop853Trip& trip, Dop853Walk& st, const double* __restrict__ t_eval, int64_t n_eval,
                                                Dop853StopRef<TERM> stop = {})
{
    if constexpr (ROOTS) {
        if (st.ev_mask != 0) {
            st.br_e = __builtin_ctz((unsigned)st.ev_mask);
            st.br_phase = 1;
            st.br_iter = 0;
            dop853_replay_at(sc, trip, st, DOP853_PROBE, sc.t_old);
            return;
        }
    }
    if constexpr (TERM) {
        if (stop.rec->stage == DOP853_STOP_SAMPLES) {
            if (dop853_stop_next(*stop.rec, st.ie, n_eval, t_eval) == DOP853_NEXT_SAMPLE) {
                dop853_replay_at(sc, trip, st, DOP853_SAMPLE, t_eval[st.ie]);
                trip.ie = st.ie;
            } else {
                dop853_replay_at(sc, trip, st, DOP853_STOP, stop.rec->t_stop);
            }
            return;
        }
    }
    if constexpr (EVAL) {
        if (st.ie < n_eval) {
            const double te = t_eval[st.ie];
            if (te <= sc.t) {                    // (t_old, t] (ivp.py:706-723); t0 itself belongs to the first step
                dop853_replay_at(sc, trip, st, DOP853_SAMPLE, te);
                trip.ie = st.ie;
                return;
            }
        }
    }
    trip.kind = DOP853_ATTEMPT;
    trip.h = sc.h_try;
    trip.commit = 1;
    trip.leave = sc.status != ST_RUNNING;
}

// Thread 0 between the barriers of two trips: the trip of kind `kind` has left the record r; decide (an attempt), advance Brent's method
// (a probe) or the sample counter, and write the next trip.  A function of its own, not inlined: its registers (pow, the 16 x 7 weights)
// are thread 0's business and stay out of the stage loop's allocation.  tev: this instance's root times [7][max_events].
//   TERM (the marl_set_terminal block of include/marl_hip.h, as rk45_sweep_body<TERM> carries it out; the walk: marl_dop853_stop.h):
//   an accepted attempt in which a monitor that changed sign meets its limit books nothing of its monitors - sc.g and the counts stay -
//   and sends ALL monitors that changed sign through the probes, slot or no slot, tev or none; their roots stay in the stop record.
//   Behind the last of them rk_terminal_step speaks once: the kept monitors are booked as rk45_events books them and their roots stored
//   where a slot is free, the dropped ones never happened.  The samples up to t_stop follow, then the STOP trip, whose record holds the
//   monitors of the state at t_stop: sc.g, sc.t = t_stop, ST_TERMINAL, and the loop is left without a commit.  The attempt that was
//   prepared after the accepted step is never made (attempts--).  nfev: the sign change counted the step's dense output already.
template <bool EVAL, bool ROOTS, bool TERM = false>
__device__ __noinline__ void dop853_control(Rk45Ctrl& sc, Dop853Trip& trip, Dop853Walk& st, int kind, const Dop853Record& r,
                                            const double* __restrict__ t_eval, int64_t n_eval, double* __restrict__ tev, int64_t max_events,
                                            Dop853StopRef<TERM> stop = {})
{
    if constexpr (TERM) {
        if (kind == DOP853_STOP) {
            for (int e = 0; e < 7; e++) sc.g[e] = rk45_monitor_of_record(r.q, e);
            if (sc.status == ST_RUNNING) sc.attempts--;
            sc.t = stop.rec->t_stop;
            sc.status = ST_TERMINAL;
            trip.kind = DOP853_ATTEMPT;
            trip.h = sc.h_try;
            trip.commit = 0;
            trip.leave = 1;
            return;
        }
    }
    if (kind == DOP853_ATTEMPT) {
        if (dop853_decide(sc, r.q[0], r.s3)) {
            int changed = 0, locate = 0;
            for (int e = 0; e < 7; e++) {        // ivp.py:149-151, as rk45_event_one; beyond max_events a sign change is only counted
                const double go = sc.g[e], gn = rk45_monitor_of_record(r.q, e);
                if ((go <= 0.0 && gn >= 0.0) || (go >= 0.0 && gn <= 0.0)) {
                    changed |= 1 << e;
                    if (ROOTS && sc.n_events[e] < max_events) locate |= 1 << e;
                }
            }
            if constexpr (TERM) {
                if (dop853_stop_begin(*stop.rec, (uint32_t)changed, sc.n_events)) {
                    for (int e = 0; e < 7; e++) stop.rec->g_new[e] = rk45_monitor_of_record(r.q, e);
                    dop853_status_after_accept(sc);
                    if (sc.status == ST_RUNNING) dop853_prepare_attempt(sc);
                    dop853_count_dense_output(sc);
                    st.counted = 1;
                    st.ev_mask = (int32_t)stop.rec->locate;
                    dop853_schedule<EVAL, ROOTS, TERM>(sc, trip, st, t_eval, n_eval, stop);
                    return;
                }
            }
            rk45_events(sc, r.q);                // g <- g_new, the counts, ev_first / ev_last
            dop853_status_after_accept(sc);
            if (sc.status == ST_RUNNING) dop853_prepare_attempt(sc);
            st.counted = 0;
            if (changed != 0) {                  // solve_ivp builds the step's dense output (ivp.py:673-676)
                dop853_count_dense_output(sc);
                st.counted = 1;
            }
            st.ev_mask = locate;
            dop853_schedule<EVAL, ROOTS, TERM>(sc, trip, st, t_eval, n_eval, stop);
        } else {
            dop853_prepare_attempt(sc);
            trip.kind = DOP853_ATTEMPT;
            trip.h = sc.h_try;
            trip.commit = 0;
            trip.leave = sc.status != ST_RUNNING;
        }
        return;
    }
    if (kind == DOP853_SAMPLE) {
        st.ie++;
        dop853_schedule<EVAL, ROOTS, TERM>(sc, trip, st, t_eval, n_eval, stop);
        return;
    }
    if constexpr (ROOTS) {
        // the order of radau_control_step's PC_BRENT: f(a), f(b), the early returns, then brent_advance until the root or 100 iterations
        const double val = rk45_monitor_of_record(r.q, st.br_e);
        bool done = false;
        double root = 0.0;
        if (st.br_phase == 1) {
            st.br_fa = val;
            st.br_phase = 2;
            dop853_replay_at(sc, trip, st, DOP853_PROBE, sc.t);
            return;
        }
        if (st.br_phase == 2) {
            if (st.br_fa == 0.0) { done = true; root = sc.t_old; }
            else if (val == 0.0) { done = true; root = sc.t; }
            else {
                st.bs.xpre = sc.t_old; st.bs.xcur = sc.t; st.bs.fpre = st.br_fa; st.bs.fcur = val;
                st.bs.xblk = 0.0; st.bs.fblk = 0.0; st.bs.spre = 0.0; st.bs.scur = 0.0;
                st.br_phase = 3;
            }
        } else {
            st.bs.fcur = val;
            st.br_iter++;
            if (st.br_iter >= 100) { done = true; root = st.bs.xcur; }
        }
        if (!done && brent_advance(st.bs)) { done = true; root = st.bs.xcur; }
        if (!done) {
            dop853_replay_at(sc, trip, st, DOP853_PROBE, st.bs.xcur);
            return;
        }
        if constexpr (TERM) {
            if (stop.rec->stage == DOP853_STOP_ROOTS) {   // a step that ends the run: kept until the rule has said which of them happened
                st.ev_mask = (int32_t)dop853_stop_root(*stop.rec, st.br_e, root);
                st.br_phase = 0;
                if (st.ev_mask == 0) {
                    int64_t counts[7], slot[7];
                    dop853_stop_rule(*stop.rec, sc.n_events, max_events, counts, slot);
                    for (int e = 0; e < 7; e++) {
                        if (!((stop.rec->kept >> e) & 1)) continue;
                        rk45_event_one(sc, e, stop.rec->g_new[e]);   // the count, ev_first / ev_last, as rk45_events
                        if (slot[e] >= 0) tev[e * max_events + slot[e]] = stop.rec->root[e];
                    }
                }
                dop853_schedule<EVAL, ROOTS, TERM>(sc, trip, st, t_eval, n_eval, stop);
                return;
            }
        }
        // (the step's bookkeeping is done: n_events[br_e] - 1 is the count before the step, < max_events)
        tev[st.br_e * max_events + (sc.n_events[st.br_e] - 1)] = root;
        st.ev_mask &= ~(1 << st.br_e);
        st.br_phase = 0;
        dop853_schedule<EVAL, ROOTS, TERM>(sc, trip, st, t_eval, n_eval, stop);
    }
}

// EVAL: t_eval samples by dense-output replays (dop853_sweep_eval_kernel).  ROOTS (with EVAL): the monitors' root times by Brent's
// method on replays (dop853_sweep_roots_kernel); order within a step: roots (monitors ascending), samples, commit.
//   Y [batch][5][N] field-major, in place;  karena: dop853_arena_doubles(batch, BLK);  t_eval [n_eval] (device), Yeval
//   [batch][n_eval][5 N], n_done [batch];  t_events [batch][7][max_events] (device).
// TERM (with ROOTS; dop853_sweep_stop_kernel): terminal monitors with the limits `lim` - see dop853_control.  The stop record is LDS of
// its own, declared under TERM only: the LDS of the other kernels is what it was.  One more trip kind, DOP853_STOP: the replay at t_stop
// whose  y + h sum_j w_j K_j  - the expression that writes a frame - becomes the thread's y, and whose monitors are reduced like a
// probe's; the loop is left behind it.  t_events may be NULL with max_events = 0, n_eval may be 0.
template <int BLK, bool VD, bool EVAL, bool ROOTS, bool TERM = false>
__device__ __forceinline__ void dop853_sweep_body(double* __restrict__ Y, const DevConsts* __restrict__ consts, Rk45Ctrl* __restrict__ ctrls,
                                                  int64_t N, double* __restrict__ karena, const double* __restrict__ t_eval = nullptr,
                                                  int64_t n_eval = 0, double* __restrict__ Yeval = nullptr,
                                                  int64_t* __restrict__ n_done = nullptr, double* __restrict__ t_events = nullptr,
                                                  int64_t max_events = 0, TermLimits lim = {})
{
    static_assert(EVAL || !ROOTS, "a Brent function evaluation is a dense-output replay");
    static_assert(ROOTS || !TERM, "the stop is found by the root search");
    using SB = StencilBlock<BLK, false, VD>;
    static_assert(SB::EDGE_DOUBLES >= NQ * BLK, "block_reduce transposes the record through the edge buffers");
    __shared__ double lds[SB::LDS_DOUBLES];
    __shared__ Rk45Ctrl sc;
    __shared__ Dop853Trip trip;
    __shared__ Dop853Walk st;
    __shared__ double wsum3[BLK / 64];             // per-wave sums of (err3 / scale)^2
    Dop853StopRef<TERM> stop;
    if constexpr (TERM) {
        __shared__ Dop853Stop stop_rec;
        stop.rec = &stop_rec;
    }
    const DevConsts& C = consts[blockIdx.x];
    double* yg = Y + (int64_t)blockIdx.x * NF * N;
    const Slab S = {N, 0, N, 0, N};
    const int64_t l0 = threadIdx.x;
    SB sb(lds, l0, consts + blockIdx.x);
    if (threadIdx.x == 0) sc = ctrls[blockIdx.x];
    __syncthreads();
    if (sc.status != ST_RUNNING) return;
    const double rtol = sc.rtol, atol = sc.atol;
    // this thread's column of the arena: K_j of field f at  kcol[(j * NF + f) * BLK]
    double* kcol = karena + (int64_t)blockIdx.x * (DOP853_SLOTS * NF * BLK) + threadIdx.x;

    double y[NF], yn[NF], k[NF];
    PointAux aux;
    load_cells<LAYOUT_FIELD_MAJOR>(yg, l0, S, C, y);
    MARL_FIELDS yn[f] = y[f];
    sb.eval(y, k, aux);   // f(t, y): RungeKutta.__init__
    MARL_FIELDS kcol[f * BLK] = k[f];

    if (threadIdx.x == 0) {
        st = Dop853Walk{};
        if constexpr (TERM) dop853_stop_init(*stop.rec, lim.k);
        trip.kind = DOP853_ATTEMPT;
        trip.h = sc.h_try;
        trip.commit = 0;
        trip.leave = 0;
        trip.at_start = 0;
        trip.ie = 0;
    }
    __syncthreads();
    while (true) {
        const int kind = to_sgpr(trip.kind), commit = to_sgpr(trip.commit), leave = to_sgpr(trip.leave);
        const int at_start = to_sgpr(trip.at_start);
        const double h = to_sgpr(trip.h);
        if (commit) {
            MARL_FIELDS {
                y[f] = yn[f];
                kcol[f * BLK] = kcol[(dop853::N_STAGES * NF + f) * BLK];
            }
        }
        if (leave) break;
        // rows 1..11: K_2..K_12;  row 12: y_new and K_13 = f(y_new);  rows 13..15 (replays): K_14..K_16
        const int last = (kind == DOP853_ATTEMPT) ? dop853::N_STAGES : DOP853_SLOTS - 1;
#pragma nounroll
        for (int s = 1; s <= last; s++) {   // (a run-time loop on purpose: ONE inlined evaluation)
            const double* row = dop853_row(s);
            double acc[NF] = {0.0, 0.0, 0.0, 0.0, 0.0};
            // four K_j in flight at a time: the loads of a batch are issued together (clamped to the last K_j of the row, so every address is
            // one this thread has written), the sums follow in the order of j
#pragma nounroll
            for (int j0 = 0; j0 < s; j0 += DOP853_BATCH) {
                double kk[DOP853_BATCH][NF];
#pragma unroll
                for (int u = 0; u < DOP853_BATCH; u++) {
                    const int j = (j0 + u < s) ? j0 + u : s - 1;
                    MARL_FIELDS kk[u][f] = kcol[(j * NF + f) * BLK];
                }
#pragma unroll
                for (int u = 0; u < DOP853_BATCH; u++) {
                    if (j0 + u < s) {
                        const double a = row[j0 + u];
                        if (a != 0.0) {          // (the tableau's zeros: skipped, not added)
                            MARL_FIELDS acc[f] += a * kk[u][f];
                        }
                    }
                }
            }
            double ys[NF];
            MARL_FIELDS ys[f] = y[f] + acc[f] * h;
            if (s == dop853::N_STAGES) {
                MARL_FIELDS yn[f] = ys[f];
            }
            sb.eval(ys, k, aux);
            MARL_FIELDS kcol[(s * NF + f) * BLK] = k[f];
        }

        Dop853Record r;
        monitors_init(r.q);
        double q3[1] = {0.0};
        if (kind == DOP853_ATTEMPT) {
            MARL_ONCE if (l0 < N) {
                double e5[NF] = {0.0, 0.0, 0.0, 0.0, 0.0}, e3[NF] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma nounroll
                for (int j0 = 0; j0 < dop853::N_STAGES; j0 += DOP853_BATCH) {   // (E5[12] = E3[12] = 0: f(y_new) has weight 0 in both estimates)
                    double kk[DOP853_BATCH][NF];
#pragma unroll
                    for (int u = 0; u < DOP853_BATCH; u++) {
                        MARL_FIELDS kk[u][f] = kcol[((j0 + u) * NF + f) * BLK];
                    }
#pragma unroll
                    for (int u = 0; u < DOP853_BATCH; u++) {
                        const double a5 = dop853::E5[j0 + u], a3 = dop853::E3[j0 + u];
                        if (a5 != 0.0 || a3 != 0.0) {
                            MARL_FIELDS {
                                e5[f] += a5 * kk[u][f];
                                e3[f] += a3 * kk[u][f];
                            }
                        }
                    }
                }
                MARL_FIELDS {
                    const double scale = atol + fmax(fabs(y[f]), fabs(yn[f])) * rtol;
                    const double r5 = e5[f] / scale, r3 = e3[f] / scale;
                    r.q[0] += r5 * r5;
                    q3[0] += r3 * r3;
                }
                monitors_accumulate(r.q, yn, aux.U, aux.W);   // (aux: of the last evaluation, f(y_new))
            }
        } else {
            MARL_ONCE if (l0 < N) {
                double d[NF] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma nounroll
                for (int j = 0; j < DOP853_SLOTS; j++) {
                    const double wj = trip.w[j];
                    MARL_FIELDS d[f] += wj * kcol[(j * NF + f) * BLK];
                }
                MARL_FIELDS d[f] = at_start ? y[f] : h * d[f] + y[f];
                if (kind == DOP853_SAMPLE) {
                    if constexpr (EVAL) {
                        double* fr = Yeval + ((int64_t)blockIdx.x * n_eval + trip.ie) * (NF * N);
                        MARL_FIELDS fr[at<LAYOUT_FIELD_MAJOR>(f, l0, N)] = d[f];
                    }
                } else {
                    double U, W;
                    uw_point(d[4], C, sb.T, U, W);
                    monitors_accumulate(r.q, d, U, W);
                    if constexpr (TERM) {
                        if (kind == DOP853_STOP) {   // the state at t_stop: what the kernel leaves in Y
                            MARL_FIELDS y[f] = d[f];
                        }
                    }
                }
            }
        }
        if (kind != DOP853_SAMPLE) {
            // the second sum rides on the record reduction's barriers: every wave butterflies its own, lane 0 leaves it in wsum3, and
            // thread 0 adds the waves' sums in wave order behind block_reduce (deterministic)
            double e3w = q3[0];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) e3w += __shfl_xor(e3w, off, 64);
            if ((threadIdx.x & 63) == 0) wsum3[threadIdx.x >> 6] = e3w;
            block_reduce<BLK, NQ, NQMIN>(r.q, lds);   // (a barrier first: the edge-exchange buffers are free behind it)
        } else {
            __syncthreads();                        // every wave has read the trip's weights before thread 0 writes the next trip
        }
        if (threadIdx.x == 0) {
            double s3 = 0.0;
#pragma unroll
            for (int w = 0; w < BLK / 64; w++) s3 += wsum3[w];
            r.s3 = s3;
            dop853_control<EVAL, ROOTS, TERM>(sc, trip, st, kind, r, t_eval, n_eval,
                                              ROOTS ? t_events + (int64_t)blockIdx.x * 7 * max_events : nullptr, max_events, stop);
        }
        __syncthreads();
    }
    MARL_ONCE if (l0 < N) {
        MARL_FIELDS yg[at<LAYOUT_FIELD_MAJOR>(f, l0, N)] = y[f];
    }
    if (threadIdx.x == 0) {
        sc.cur = 0;
        ctrls[blockIdx.x] = sc;
        if constexpr (EVAL) n_done[blockIdx.x] = st.ie;   // frames written; the rest of the instance's frame memory is untouched
    }
}

// plain sweeps: neither samples nor roots (sign changes are still counted)
template <int BLK, bool VD = false>
__global__ void __launch_bounds__(BLK) dop853_sweep_kernel(double* __restrict__ Y, const DevConsts* __restrict__ consts,
                                                           Rk45Ctrl* __restrict__ ctrls, int64_t N, double* __restrict__ karena)
{
    dop853_sweep_body<BLK, VD, false, false>(Y, consts, ctrls, N, karena);
}

// sweeps with t_eval: frames by dense-output replays before the commit
template <int BLK, bool VD = false>
__global__ void __launch_bounds__(BLK) dop853_sweep_eval_kernel(double* __restrict__ Y, const DevConsts* __restrict__ consts,
                                                                Rk45Ctrl* __restrict__ ctrls, int64_t N, double* __restrict__ karena,
                                                                const double* __restrict__ t_eval, int64_t n_eval,
                                                                double* __restrict__ Yeval, int64_t* __restrict__ n_done)
{
    dop853_sweep_body<BLK, VD, true, false>(Y, consts, ctrls, N, karena, t_eval, n_eval, Yeval, n_done);
}

// sweeps (and single runs: an instance count of one) that also locate the monitors' roots by Brent's method on probe trips
template <int BLK, bool VD = false>
__global__ void __launch_bounds__(BLK) dop853_sweep_roots_kernel(double* __restrict__ Y, const DevConsts* __restrict__ consts,
                                                                 Rk45Ctrl* __restrict__ ctrls, int64_t N, double* __restrict__ karena,
                                                                 const double* __restrict__ t_eval, int64_t n_eval,
                                                                 double* __restrict__ Yeval, int64_t* __restrict__ n_done,
                                                                 double* __restrict__ t_events, int64_t max_events)
{
    dop853_sweep_body<BLK, VD, true, true>(Y, consts, ctrls, N, karena, t_eval, n_eval, Yeval, n_done, t_events, max_events);
}

// dop853_sweep_roots_kernel honouring terminal monitors (marl_sweep_dop853_stop_dev; `lim`: marl_set_terminal's limits): an instance
// whose monitor meets its limit ends at that root with ST_TERMINAL, the state the step's dense output there.  A unit of its own
// (marl_dop853_stop.hip).
template <int BLK, bool VD = false>
__global__ void __launch_bounds__(BLK) dop853_sweep_stop_kernel(double* __restrict__ Y, const DevConsts* __restrict__ consts,
                                                                Rk45Ctrl* __restrict__ ctrls, int64_t N, double* __restrict__ karena,
                                                                const double* __restrict__ t_eval, int64_t n_eval,
                                                                double* __restrict__ Yeval, int64_t* __restrict__ n_done,
                                                                double* __restrict__ t_events, int64_t max_events, TermLimits lim)
{
    dop853_sweep_body<BLK, VD, true, true, /*TERM=*/true>(Y, consts, ctrls, N, karena, t_eval, n_eval, Yeval, n_done, t_events, max_events, lim);
}

}  // namespace marl
