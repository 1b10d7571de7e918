/* marl_hip.h - C ABI of libmarl_hip.so: the MI355X (gfx950) implementation of the reference's hot
 * path - the five-field L'Heureux (2018) RHS and its explicit Runge-Kutta time loops.
 *
 * Every entry point names the reference interface it stands in for (paths relative to the
 * reference repository).  Plain pointers and sizes only; no C++ or torch types cross this ABI.
 * INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - all floating point data is float64; a state vector is float64[5*N] FIELD-MAJOR
 *     (CA | CC | cCa | cCO3 | Phi, each N contiguous: marlpde/Evolve_scenario.py:64-65,76-86) unless a
 *     `layout` argument says MARL_LAYOUT_TILED (device buffers only);
 *   - functions return 0 when they ran, <0 on error (invalid argument / HIP failure; text from
 *     marl_last_error); how an integration ENDED is in marl_stats.status (0 reached t1, -1 step size
 *     too small = scipy's status -1, 2 attempt budget exhausted) - a failed solve is not an API error,
 *     exactly as solve_ivp reports it in sol.status without raising (scipy/integrate/_ivp/ivp.py:659-661);
 *   - `*_dev` variants take DEVICE pointers (e.g. torch.Tensor.data_ptr()), enqueue on the context's
 *     stream and do not synchronise unless documented; the others take HOST pointers, copy in/out
 *     and return after the stream is idle;
 *   - a context is not thread safe (the reference's RHS object is stateful too:
 *     marlpde/LHeureux_model.py:90,168-172); use one context per thread/GPU/stream;
 *   - NaN/Inf in a state are data, not errors (the reference's numba path behaves the same way).
 */
#ifndef MARL_HIP_H
#define MARL_HIP_H

#include "marl_params.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct marl_ctx marl_ctx;

#define MARL_LAYOUT_FIELD_MAJOR 0 /* y[f*N + i]                                   (reference layout) */
#define MARL_LAYOUT_TILED 1       /* y[(i>>6)*320 + f*64 + (i&63)], ceil(N/64)*320 doubles            */

/* ---- model construction ---------------------------------------------------------------------
 * Replaces LMAHeureuxPorosityDiff.__init__ (marlpde/LHeureux_model.py:12-133): derives the
 * constants (:36-72, :130-133), the boundary rules (:26-30) and the depth mask
 * (marlpde/Evolve_scenario.py:51-54), and uploads them.  `params` holds n_instances blocks
 * (a parameter sweep: one block per instance; the reference runs one instance per process).
 * All instances share N. */
int marl_ctx_create(const marl_params* params, int64_t n_instances, int64_t N, int device, marl_ctx** out);
/* New parameters for an existing context (same N, same number of instances): what constructing the reference's model again with other
 * arguments does (marlpde/LHeureux_model.py:12-133), without giving up the buffers the context has allocated - a loop over scenarios
 * (the reference's tests, marlpde_amd.sweep.run_sweep_bdf) pays for its allocations once. */
int marl_ctx_set_params(marl_ctx* ctx, const marl_params* params, int64_t n_instances);

void marl_ctx_destroy(marl_ctx* ctx);
const char* marl_last_error(const marl_ctx* ctx); /* ctx may be NULL: error of the last failed create */
/* All work of a context is enqueued on one HIP stream: by default the device's default (null) stream -
 * which is also PyTorch's default current stream - or the one given here (a hipStream_t, e.g.
 * torch.cuda.current_stream().cuda_stream; NULL selects the default stream again). */
int marl_set_stream(marl_ctx* ctx, void* hip_stream);
int marl_synchronize(marl_ctx* ctx);
/* Terminal monitors: a property of the model, as in the reference, where `terminal` is an attribute of the model's event methods
 * (marlpde/LHeureux_model.py:113-122: "Make sure integration stops when we field values become less than zero or more than one, in some
 * cases. Or just register that this is happening and continue integration, which corresponds to `False`.").
 * terminal[e], e in the order of marl_events: 0 - monitor e only records (the reference's setting, and a new context's);
 * k > 0 - the run ends at the k-th occurrence of monitor e (scipy >= 1.13 takes an int for event.terminal; True is 1).
 * NULL: all zeros.  A negative entry: -1, nothing changed.  ctx == NULL: -1.
 * A run that a terminal monitor ends follows solve_ivp (ivp.py:79-130 handle_events, :681-723; the rule: csrc/marl_terminal.h):
 *   stats->status = 1 ("A termination event occurred."), stats->t = t_stop, the root of the terminal monitor;
 *   the state returned is the accepted step's dense output at t_stop - the expression that writes a t_eval frame, so it equals a
 *   frame at t_eval = t_stop bit for bit - and stats->event_value holds that state's monitors;
 *   t_events / n_events hold the roots up to and including the terminal one in the order of root times (equal roots: monitor order);
 *   a sign change after it in the same step is neither stored nor counted, so n_events[e] stays the number of roots scipy returns;
 *   t_eval samples with t_eval[k] <= t_stop are written from that step (n_done counts them), later frames are untouched;
 *   nfev / njev / nlu / n_accepted / n_rejected are those after the accepted step: roots and samples cost no evaluation.
 * In such a step the roots of ALL active monitors are located (the order needs them), with or without a free slot and also when the
 * caller passed no t_events; they are stored only where a slot is free.  A step that meets no limit runs exactly as without limits.
 * Entries that stop: marl_integrate_radau, marl_integrate_bdf, marl_sweep_radau_dev / _events_dev / _eval_dev,
 * marl_sweep_bdf_terminal_dev, marl_sweep_rk45_terminal_dev / rk23_terminal_dev, marl_integrate_rk45_terminal / rk23_terminal,
 * marl_sweep_dop853_stop_dev, marl_integrate_dop853_stop, marl_integrate_dop853_grid; and, by a rule of their own (the end of the step,
 * no interpolation: see there), marl_sweep_rk4_watch_dev and marl_integrate_rk4_watch.  The plain fixed-step entries
 * (marl_integrate_rk4, marl_integrate_rk4_dev, marl_sweep_rk4_dev) ignore the limits, as they always did.  Every other
 * integrator entry (marl_integrate_rk45 / rk23, marl_integrate_rk45_dev / rk23_dev, marl_sweep_rk45_dev / _eval_dev / _events_dev and their rk23
 * counterparts, marl_integrate_dop853, marl_sweep_dop853_dev / _eval_dev / _events_dev, marl_integrate_dop853_grid_dev,
 * marl_sweep_bdf_dev / _eval_dev / _events_dev,
 * marl_slab_init_control, marl_slab_run) returns -1 while a limit is set - "...: terminal monitors are not supported by this entry (marl_set_terminal)" -
 * before it touches the state, and is unchanged when none is. */
int marl_set_terminal(marl_ctx* ctx, const int64_t terminal[7]);
/* Tuning knobs; unknown names are an error.  See DESIGN.md.
 *   rk4_variant (fused RK4 steps per launch: 0..4 = 1 / 2 / 4 / 8 / 16; anything else, e.g. -1: chosen by grid size; with dPhi_variable
 *   always 4), sweep_variant (one-workgroup window: 0 / 1 / 2 = 256 / 512 / 1024 cells, used when it holds N; otherwise, e.g. -1, the
 *   smallest that does), rk45_variant (accepted, no effect: the adaptive kernels have one shape), host_layout (device layout used behind the
 *   host-pointer entry points), poll_interval (attempts enqueued between status reads), no_reuse (1: every RHS evaluation of
 *   the fused kernels takes its full transcendental path - the input-independent worst case, for benchmarks), radau_solver
 *   (linear systems of the implicit path: 0 block parallel cyclic reduction - the default; 1 sequential block Thomas, a cross-check that
 *   only lab builds compile in, -DMARL_LAB_BLOCK_THOMAS: an error otherwise),
 *   rk45_stream (the adaptive loop of ONE grid: 1, the default: one launch for a whole batch of attempts - resident workgroups meeting at a
 *   barrier in memory, rk45_stream_kernel - for grids of up to three rounds of resident workgroups (~750 000 cells on an MI355X), one launch
 *   per attempt above; 0 never; 2 always), rk45_stream_attempts (attempts per launch of that loop at most; 4096),
 *   dd_stream (library-side domain-decomposed loop: 0, the default: attempt + reduce + pack launches per attempt; 1 / 2: the slab's attempt as
 *   one launch of the persistent kernel whose last workgroup packs the rank's message - measured not faster),
 *   implicit_zero_copy (1, the default: marl_integrate_radau / marl_integrate_bdf read their per-iteration scalars from coherent host
 *   memory that the kernels write and the host polls; 0: a copy and a stream synchronisation per read - bit-identical),
 *   radau_fused_solve (systems of up to 2048 unknowns: 0 = one launch per cyclic-reduction level; 1 = every level of a solve in one
 *   launch; 2 = a Radau Newton iteration's linear algebra in one workgroup; 3, the default = 1 plus, for single Radau runs, two
 *   launches per Newton iteration - all bit-identical),
 *   radau_sweep_wg (Radau sweeps of grids of up to 409 cells: 3, the default: a persistent workgroup per instance runs the instance's
 *   sequential work and its Jacobians, launch kernels over work lists do the factorisations; 1: Jacobians by launch kernels too -
 *   bit-identical; 2: everything in the workgroup; 0: one launch cycle per action),
 *   radau_cr (single Radau / BDF runs: levels of block cyclic reduction in front of the parallel cyclic reduction; -1, the default:
 *   automatic for grids of radau_cr_min_n (2048) cells or more, down to a compact system of at most 204 rows; 0: none; k > 0: k levels),
 *   radau_cr_small / radau_cr_small_min_n (grids solved in one workgroup, up to 409 cells: 3 levels of cyclic reduction in front of PCR
 *   inside the one-launch solves, by default from 205 cells; min_n = 32 turns it on for the reference's N = 200 - faster sweeps, but no
 *   longer decision-by-decision equal to scipy in every pinned case),
 *   radau_cr_tail (1, the default: the launch-bound levels of such a solve in one launch each way; 0: one launch per level -
 *   bit-identical), bdf_solve_wg (1, the default: on grids of up to 409 cells marl_integrate_bdf runs solve_bdf_system as one launch of
 *   one workgroup; 0: one RHS launch, one linear-algebra launch and one wait per Newton iteration - bit-identical),
 *   rk4_stream (fixed-step RK4 of one grid as ONE dataflow launch over (level, tile) work items instead of one launch per
 *   fused level: 0 never, 1 - the default - for grids of 196 608 cells or more, 2 always; results are bit-identical),
 *   rk4_chain (the streamed loop with 4 steps per level and constant porosity diffusion: work items that are chains of K windows, of
 *   which only the first recomputes a left halo - rk4_chain_kernel; 0 never, 1 - the default - the longest chain of at most 8 windows
 *   that leaves every resident workgroup two items per level, which is none on grids under ~950 000 cells; 2 ... 8: chains of that many windows),
 *   rk4_stream_third (1, the default: a streamed call with an odd number of levels runs through a third state buffer instead of
 *   copying the state back afterwards; 0: copy - bit-identical),
 *   rk4_stream_test_raise (test hook: the next streamed run starts with its give-up flag raised - marl_synchronize must
 *   report error -2 and the context must recover), rk4_stream_max_items (test hook: work items per streamed launch, default
 *   2^31 - 1: a call with more (level, tile) items is split into several launches of an even number of levels). */
int marl_set_option(marl_ctx* ctx, const char* name, int64_t value);
/* Derived constants of instance `inst` in the order of tests/golden/derived_constants.json:
 * delta_x nu1 nu2 KRat dCa dCO3 delta Da lambda_ auxcon rhorat0 rhorat presum F_fixed dPhi_fixed
 * Peclet_min Peclet_max, then mask_lo, mask_hi (as doubles). */
int marl_get_constants(const marl_ctx* ctx, int64_t inst, double out[19]);
/* doubles needed for one instance's state in `layout` */
int64_t marl_state_doubles(const marl_ctx* ctx, int layout);

/* ---- RHS ---------------------------------------------------------------------------------------
 * Replaces the solve_ivp callable  fun(t, y, progress_proxy, progress_dt, t0) / fun_numba(...)
 * (marlpde/LHeureux_model.py:162-288, :290-359 -> pde_rhs :361-522).  `t` is accepted and ignored
 * (the system is autonomous; the reference only uses t for its progress bar).  y and dydt must not
 * alias.  For n_instances > 1 the buffers hold the instances one after another. */
int marl_rhs(marl_ctx* ctx, double t, const double* y, double* dydt);
int marl_rhs_dev(marl_ctx* ctx, double t, const double* y_dev, double* dydt_dev, int layout);

/* ---- monitors ----------------------------------------------------------------------------------
 * Replaces the seven event functions zeros, zeros_CA, zeros_CC, ones_CA_plus_CC, ones_Phi,
 * zeros_U, zeros_W (marlpde/LHeureux_model.py:524-593), in that order.  out: [n_instances][7] (host). */
int marl_events(marl_ctx* ctx, const double* y, double* out);
int marl_events_dev(marl_ctx* ctx, const double* y_dev, int layout, double* out); /* synchronises */

int marl_convert_layout_dev(marl_ctx* ctx, const double* src_dev, double* dst_dev, int src_layout, int dst_layout);

/* Test hook: y[i] = op(x[i]) with the kernels' own math primitives: op 0 log, 1 exp, 2 pow(x, e),
 * 3 reciprocal, 4 Fiadeiro-Veronis sigma(Pe = x, W = e).  Device pointers; asynchronous. */
int marl_debug_math(marl_ctx* ctx, int op, const double* x_dev, double* y_dev, int64_t n, double e);
/* Test hooks of the implicit path (marl_integrate_radau / marl_integrate_bdf below): one call of the finite-difference Jacobian and one
 * factorisation with its solves, through the very functions an integration calls.  HOST pointers; single-instance contexts; both
 * synchronise.
 * marl_debug_num_jac: f0 = f(y) by the RHS kernel, then scipy's num_jac (common.py:268-451) at (y, f0) as the integrators run it.
 *   y: float64[5N] field-major; threshold: num_jac's (the integrators pass atol); groups: int32[5N] or NULL, as for marl_integrate_radau;
 *   factor_inout: float64[5N] field-major, the persistent step factors: read when first == 0 (first != 0: every factor starts from
 *   sqrt(eps), as on the first Jacobian of a run), written with the adapted factors; J_out: float64[N][3][5][5], the device layout:
 *   J_out[((i*3 + d)*5 + f)*5 + fp] = d rate(f, i) / d y(fp, i + d - 1); entries outside the pattern or the grid are 0.
 * marl_debug_block_solve: factorises  mu I - jscale J  (J in the layout above) and solves nrhs right-hand sides one after another with
 *   that ONE factorisation.  systems = 1: the real system only (BDF: mu_r = 1, jscale = c); 2: the real system and the complex one,
 *   mu = mu_c_re + i mu_c_im (Radau: jscale = 1).  b_r / x_r: float64[nrhs][5N] CELL-MAJOR (unknown 5 i + f); b_c / x_c:
 *   [nrhs][5N] complex, (re, im) interleaved, NULL with systems = 1.  The path (parallel cyclic reduction alone, cyclic reduction in
 *   front of it, per-level / fused / tail launches) is chosen by the options radau_cr, radau_cr_small, radau_cr_small_min_n,
 *   radau_fused_solve and radau_cr_tail exactly as for a run. */
int marl_debug_num_jac(marl_ctx* ctx, const double* y, double threshold, const int32_t* groups, double* factor_inout, int first,
                       double* J_out);
int marl_debug_block_solve(marl_ctx* ctx, const double* J, double jscale, double mu_r, double mu_c_re, double mu_c_im, int systems,
                           int64_t nrhs, const double* b_r, const double* b_c, double* x_r, double* x_c);
/* Test hook of the BDF sweep (the marl_sweep_bdf entries below): ONE launch of one of its six data-parallel kernels, through the launcher
 * the sweep itself calls, on the sweep's arena (one per instance of the context, B = n_instances, at the sweep's stride).  HOST pointers;
 * whole-grid context with 5N <= 2048; synchronises.  n = 5N.
 *   op: MARL_BDF_INIT_D        D[0] = y, D[1] = f h
 *       MARL_BDF_CHANGE_D      D[:order + 1] = RU^T D[:order + 1]
 *       MARL_BDF_ACCEPT_NORMS  the accepted step's update of the differences from d (bdf.py:414-418), y = ynew, and the sums
 *                              sum (coef v / (atol + rtol |y|))^2 that want_norms asks for: bit 0 -> ss_m from D[order] with err_coef_m,
 *                              bit 1 -> ss_p from D[order + 2] with err_coef_p
 *       MARL_BDF_SAMPLE        frames [first, min(end, n_eval)) of the instance = D[0] + sum_j D[j + 1] p[j] at t_eval[k], p the weights of
 *                              BdfDenseOutput(t - h, t, h, order, D)
 *       MARL_BDF_ROOTS         the root times over [t_old, t] of the monitors in `mask` on the same dense output, monitor e's into
 *                              t_events[instance][e][slot[e]]
 *       MARL_BDF_STOP          the state a terminal monitor leaves (marl_sweep_bdf_terminal_dev): y = the same dense output at t_stop,
 *                              which dargs passes in the place of t_old, and that state's seven monitors, monitor e's into
 *                              t_events[instance][e][0] (max_events > 0)
 *   list, n_list: the instances launched, in this order (grid.z = n_list), each in [0, B), n_list <= B; NULL, 0: all B in order.
 *   iargs: int64[B][MARL_BDF_DEBUG_INTS] per instance {order, want_norms, first, end, mask, slot[0 .. 6]}.
 *   dargs: float64[B][MARL_BDF_DEBUG_DOUBLES] per instance {h, rtol, atol, err_coef_m, err_coef_p, t, t_old (STOP: t_stop), RU[6][6] row-major}.
 *   D_in: float64[B][8][n], all eight rows of every instance's differences; vec_in: float64[B][4][n], the instance's y, f, d, ynew.
 *   t_eval: float64[n_eval] (SAMPLE; n_eval may be 0).  max_events: root slots per monitor (ROOTS: > 0).
 *   Out - everything the kernel may write and its surroundings: D_out [B][8][n]; y_out [B][n]; frames [B][n_eval][n], t_events
 *   [B][7][max_events] and ss [B][2] = (ss_m, ss_p) are IN-OUT: what the caller puts there is on the device before the launch and
 *   comes back where the kernel wrote nothing.
 *   Returns -1 with a message, launching nothing, when an argument is out of range: an order outside 1 .. 5 (every op but INIT_D), a list
 *   entry outside [0, B) or n_list > B, first > end or first < 0, want_norms outside 0 .. 3, a mask outside 0 .. 127, ROOTS with
 *   max_events <= 0 or a searched monitor's slot outside [0, max_events), STOP with max_events <= 0, 5N > 2048. */
enum { MARL_BDF_INIT_D = 0, MARL_BDF_CHANGE_D = 1, MARL_BDF_ACCEPT_NORMS = 2, MARL_BDF_SAMPLE = 3, MARL_BDF_ROOTS = 4, MARL_BDF_STOP = 5 };
enum { MARL_BDF_DEBUG_INTS = 12, MARL_BDF_DEBUG_DOUBLES = 43 };
int marl_debug_bdf_batch(marl_ctx* ctx, int op, const int32_t* list, int64_t n_list, const int64_t* iargs, const double* dargs,
                         const double* D_in, const double* vec_in, const double* t_eval, int64_t n_eval, int64_t max_events,
                         double* D_out, double* y_out, double* frames, double* t_events, double* ss);

/* ---- fixed-step classical RK4 (BASELINE config 2; no counterpart in the reference, which only
 * remarks that forward Euler fails: README.md:9).  y is advanced in place by nsteps steps of dt. */
int marl_integrate_rk4(marl_ctx* ctx, double* y, double dt, int64_t nsteps);
int marl_integrate_rk4_dev(marl_ctx* ctx, double* y_dev, int layout, double dt, int64_t nsteps);
/* batched sweep: one dt per instance (host array, n_instances entries); FIELD-MAJOR device state */
int marl_sweep_rk4_dev(marl_ctx* ctx, double* y_dev, const double* dt, int64_t nsteps);
/* The MONITORED fixed-step sweep (rk4_watch_kernel, csrc/marl_rk4_watch.h; the rules: csrc/marl_rk4_watch_ctl.h): the step of
 * marl_sweep_rk4_dev with the reference's driver inside the kernel - the seven monitors after every step (Evolve_scenario.py:107-109),
 * frames, the `terminal` switch (LHeureux_model.py:113-122) - and word that the step was too large.  Grids of one workgroup, N <= 1024
 * (else -1); no slab contexts.  The three entries above are unchanged and go on ignoring marl_set_terminal.
 *   steps   step s (0-based) goes from t0 + s dt[b] to t0 + (s + 1) dt[b]; times are that product, never accumulated.  dt: host, one
 *           per instance.
 *   roots   a sign change of monitor e in a step (go <= 0 && gn >= 0 or the reverse, ivp.py:149-151) is counted in
 *           stats[b].n_events[e]; its time  t_s + dt go / (go - gn)  (t_(s+1) when go == gn) is stored in t_events (host,
 *           [n_instances][7][max_events], NaN beyond the stored ones) while a slot is free.  There is NO dense output and NO Brent: a
 *           fixed step takes no partial steps, and this secant estimate is O(dt^2) away from the root.  t_events == NULL or
 *           max_events <= 0: counted only.
 *   frames  frame_steps: host, n_frames strictly ascending step counts in [0, nsteps], shared by all instances - otherwise -1 before
 *           anything is touched.  Frame j is the state after frame_steps[j] steps (0: the initial state), written as the kernel passes it
 *           into frames_dev, device, [n_instances][n_frames][5N] field-major.  n_done (host, may be NULL): frames written per instance;
 *           frames an instance does not reach are not touched.  n_frames = 0: frame_steps / frames_dev may be NULL.
 *   stop    marl_set_terminal's limits are honoured: the instance ends at the END of the step in which monitor e has its k[e]-th
 *           occurrence - status 1, stats[b].t that step's end, the state that step's result, NOT interpolated to the root (a
 *           deliberate difference from the rule of csrc/marl_terminal.h: there is no dense output to cut the step with).  All sign
 *           changes of that step are counted and stored, a frame due at it is written.  No limit, or one never met: bit for bit the
 *           run without limits.
 *   -2      an instance whose state holds a non-finite value after a step ends there with status -2 (the step was too large):
 *           stats[b].t that step's end, no monitor processed for that step (event_value: the last finite state's monitors), no frame
 *           written at it, the state returned as it is.  The other instances are unaffected.
 *   stats   status 0 / 1 / -2; n_accepted = steps done, n_rejected = 0, nfev = 4 x steps done, h_next = dt, t = t0 + steps dt,
 *           event_value = the monitors of the returned state, n_events as counted.
 * Synchronises. */
int marl_sweep_rk4_watch_dev(marl_ctx* ctx, double* y_dev, double t0, const double* dt, int64_t nsteps, const int64_t* frame_steps,
                             int64_t n_frames, double* frames_dev, int64_t* n_done, double* t_events, int64_t max_events,
                             marl_stats* stats);
/* marl_sweep_rk4_watch_dev for ONE instance with host pointers throughout: y in / out, y_frames [n_frames][5N] (the first *n_done
 * frames are written), t_events [7][max_events].  Single-instance contexts, N <= 1024. */
int marl_integrate_rk4_watch(marl_ctx* ctx, double* y, double t0, double dt, int64_t nsteps, const int64_t* frame_steps,
                             int64_t n_frames, double* y_frames, int64_t* n_done, double* t_events, int64_t max_events,
                             marl_stats* stats);

/* ---- adaptive Dormand-Prince RK45 ---------------------------------------------------------------
 * Replaces  scipy.integrate.solve_ivp(fun, t_span, y0, method="RK45", first_step=, rtol=, atol=,
 * t_eval=, events=[7 monitors])  as called at marlpde/Evolve_scenario.py:104-109 (controller:
 * scipy/integrate/_ivp/rk.py:111-176; driver: ivp.py:654-723).  y: in y(t0), out y(stats->t).
 * t_eval (may be NULL): sorted sample times within [t0, t1]; y_eval receives n_eval x 5N doubles,
 * sample-major (dense output, rk.py:560-574).  t_events (may be NULL): 7 x max_events root times of the
 * monitors' sign changes, located like scipy does (dense output + Brent, ivp.py:51-76); the counts are
 * stats->n_events.  max_attempts = 0: unlimited. */
int marl_integrate_rk45(marl_ctx* ctx, double* y, double t0, double t1, double first_step, double rtol, double atol,
                        const double* t_eval, int64_t n_eval, double* y_eval, double* t_events, int64_t max_events,
                        int64_t max_attempts, marl_stats* stats);
int marl_integrate_rk45_dev(marl_ctx* ctx, double* y_dev, int layout, double t0, double t1, double first_step,
                            double rtol, double atol, int64_t max_attempts, marl_stats* stats); /* synchronises */
/* batched sweep: per-instance controller; all instances share t0, t1, first_step, tolerances.
 * stats: host array of n_instances entries.  FIELD-MAJOR device state.  Synchronises. */
int marl_sweep_rk45_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol,
                        double atol, int64_t max_attempts, marl_stats* stats);
/* the sweep with t_eval: what the reference stores of every run is the time series that solve_ivp(..., t_eval=) fills
 * (marlpde/Evolve_scenario.py:104-109).  As in scipy the samples never change the steps (ivp.py:706-723): after every
 * accepted step the kernel writes the samples inside it by dense output (rk.py:560-574) - no function evaluation is
 * counted, and state and statistics are those of marl_sweep_rk45_dev.
 * t_eval: host, n_eval times shared by all instances, strictly increasing within [t0, t1].
 * y_eval_dev: device, [n_instances][n_eval][5N], each frame field-major.  n_done: host, n_instances entries: the frames
 * written for that instance (the samples up to the time it reached); its later frames are not touched.
 * n_eval = 0 is marl_sweep_rk45_dev.  t1 == t0: no step; a sample at t0 receives y0.  Synchronises. */
int marl_sweep_rk45_eval_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol,
                             int64_t max_attempts, const double* t_eval, int64_t n_eval, double* y_eval_dev,
                             int64_t* n_done, marl_stats* stats);
/* the sweep with t_eval and the monitors' root times: the reference prints and stores the roots of its seven monitors for every
 * run (marlpde/Evolve_scenario.py:118-145, 175-177; solve_ivp(..., events=[7]), non-terminal, both directions).  Located inside
 * the sweep kernel as scipy locates them (ivp.py:673-694, solve_event_equation :51-76): Brent's method, xtol = rtol = 4 eps, on
 * the dense output of the accepted step in which a monitor changes sign.  Steps, state, frames and statistics are those of
 * marl_sweep_rk45_eval_dev (nfev included).
 * t_events: host, [n_instances][7][max_events]; entry k of monitor e is its k-th root, NaN beyond min(n_events[e], max_events);
 * stats[b].n_events[e] counts every sign change, located or not.  t_events == NULL or max_events <= 0 is
 * marl_sweep_rk45_eval_dev.  n_eval = 0 is allowed here (t_eval, y_eval_dev, n_done may then be NULL).  t1 == t0: no step, no
 * roots.  Synchronises. */
int marl_sweep_rk45_events_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol,
                               int64_t max_attempts, const double* t_eval, int64_t n_eval, double* y_eval_dev,
                               int64_t* n_done, double* t_events, int64_t max_events, marl_stats* stats);

/* The RK45 sweep HONOURING TERMINAL MONITORS (marl_set_terminal; the semantics of the block there; the rule: csrc/marl_terminal.h, its
 * bookkeeping for one accepted step: csrc/marl_rk_terminal.h): the reference's `terminal` switch (marlpde/LHeureux_model.py:113-122) for
 * the explicit sweeps.  The three entries above refuse a context with limits; this one ends every instance at its terminal monitor's
 * root inside the sweep kernel (rk45_sweep_term_kernel): in an accepted step in which a monitor that changed sign meets its limit, the
 * roots of ALL monitors that changed sign are located (Brent on replays of the step, with or without a free slot, also without
 * t_events), the rule says which of them happened - counted and, where a slot is free, stored - then the samples with
 * t_eval[k] <= t_stop are written, and one more replay writes the step's dense output at t_stop into the state: stats[b].status = 1,
 * stats[b].t = t_stop, stats[b].event_value = that state's monitors, counters those after the accepted step.  A stop in the step that
 * reaches t1 is a stop.  Instances that meet no limit, and every step before the terminal one, run exactly as under
 * marl_sweep_rk45_events_dev.  With no limit set this entry dispatches to the kernels of the three entries above (t_eval / n_eval = 0
 * and t_events == NULL / max_events <= 0 allowed) and is those entries bit for bit.  Arguments as for marl_sweep_rk45_events_dev.
 * Synchronises. */
int marl_sweep_rk45_terminal_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol,
                                 int64_t max_attempts, const double* t_eval, int64_t n_eval, double* y_eval_dev,
                                 int64_t* n_done, double* t_events, int64_t max_events, marl_stats* stats);
/* marl_integrate_rk45 HONOURING TERMINAL MONITORS: the same arguments (host pointers), the same loops - one workgroup for N <= 1024, the
 * streamed loop, one launch per attempt - which pause on every monitor sign change, also without t_events, while a limit is set.  At
 * such a pause the roots are located on the step's dense output as without limits; when a monitor meets its limit, those of all
 * monitors that changed sign, and the rule is applied: stats->status = 1, stats->t = t_stop, y = the dense output at t_stop (the launch
 * that writes a t_eval sample: bit-equal to a sample at t_stop), y_eval holds the samples with t_eval[k] <= t_stop, a dropped sign
 * change is neither stored nor counted.  With no limit set this is marl_integrate_rk45. */
int marl_integrate_rk45_terminal(marl_ctx* ctx, double* y, double t0, double t1, double first_step, double rtol, double atol,
                                 const double* t_eval, int64_t n_eval, double* y_eval, double* t_events, int64_t max_events,
                                 int64_t max_attempts, marl_stats* stats);

/* ---- adaptive Bogacki-Shampine RK23 -------------------------------------------------------------
 * Replaces  scipy.integrate.solve_ivp(fun, t_span, y0, method="RK23", ...): the reference's Solver forwards any solve_ivp method
 * (marlpde/parameters.py:212-213), and on these stability-limited equations RK23 reaches the same time with 1.6 - 3.1 times fewer
 * RHS evaluations than RK45.  The method is scipy/integrate/_ivp/rk.py, class RK23 (tableau, order 3, error_estimator_order 2,
 * n_stages 3) under RungeKutta._step_impl (rk.py:111-176): 3 evaluations per attempt (nfev), step factor 0.9 err^(-1/3), cubic
 * dense output (RkDenseOutput with the 4 x 3 P) that costs no evaluation.  Arguments, results, argument checks and status codes
 * are those of the RK45 entry of the same name; messages start with "rk23:".  Grids above one workgroup's window run one launch
 * per attempt. */
/* marl_integrate_rk45 with RK23 (rk.py, class RK23; marlpde/parameters.py:212-213) */
int marl_integrate_rk23(marl_ctx* ctx, double* y, double t0, double t1, double first_step, double rtol, double atol,
                        const double* t_eval, int64_t n_eval, double* y_eval, double* t_events, int64_t max_events,
                        int64_t max_attempts, marl_stats* stats);
/* marl_integrate_rk45_dev with RK23 (rk.py, class RK23; marlpde/parameters.py:212-213); synchronises */
int marl_integrate_rk23_dev(marl_ctx* ctx, double* y_dev, int layout, double t0, double t1, double first_step,
                            double rtol, double atol, int64_t max_attempts, marl_stats* stats);
/* marl_sweep_rk45_dev with RK23 (rk.py, class RK23; marlpde/parameters.py:212-213): N <= 1024 cells, else -1 */
int marl_sweep_rk23_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol,
                        double atol, int64_t max_attempts, marl_stats* stats);
/* marl_sweep_rk45_eval_dev with RK23 (rk.py, class RK23 and RkDenseOutput :560-574; marlpde/parameters.py:212-213) */
int marl_sweep_rk23_eval_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol,
                             int64_t max_attempts, const double* t_eval, int64_t n_eval, double* y_eval_dev,
                             int64_t* n_done, marl_stats* stats);
/* marl_sweep_rk45_events_dev with RK23 (rk.py, class RK23; roots as ivp.py:673-694, :51-76; marlpde/parameters.py:212-213) */
int marl_sweep_rk23_events_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol,
                               int64_t max_attempts, const double* t_eval, int64_t n_eval, double* y_eval_dev,
                               int64_t* n_done, double* t_events, int64_t max_events, marl_stats* stats);
/* marl_sweep_rk45_terminal_dev with RK23 (rk23_sweep_term_kernel) */
int marl_sweep_rk23_terminal_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol,
                                 int64_t max_attempts, const double* t_eval, int64_t n_eval, double* y_eval_dev,
                                 int64_t* n_done, double* t_events, int64_t max_events, marl_stats* stats);
/* marl_integrate_rk45_terminal with RK23 */
int marl_integrate_rk23_terminal(marl_ctx* ctx, double* y, double t0, double t1, double first_step, double rtol, double atol,
                                 const double* t_eval, int64_t n_eval, double* y_eval, double* t_events, int64_t max_events,
                                 int64_t max_attempts, marl_stats* stats);

/* ---- adaptive Dormand-Prince DOP853, grids of one workgroup ------------------------------------------
 * Replaces  scipy.integrate.solve_ivp(fun, t_span, y0, method="DOP853", first_step=, rtol=, atol=, t_eval=, events=[7 monitors]):
 * the reference's Solver forwards any solve_ivp method (marlpde/parameters.py:212-213), and DOP853 was the last explicit one that
 * scipy drove on marl_rhs.  The method is scipy/integrate/_ivp/rk.py, class DOP853 (order 8, error_estimator_order 7, n_stages 12;
 * coefficients: dop853_coefficients.py) under RungeKutta._step_impl (rk.py:111-176): 12 evaluations per attempt, step factor
 * 0.9 err^(-1/8), the error norm of DOP853._estimate_error_norm (rk.py:506-518), the dense output of Dop853DenseOutput
 * (rk.py:520-547, :577-601), whose three extra evaluations scipy counts once per accepted step that has a monitor sign change or a
 * t_eval sample in it:  nfev = 1 + 12 attempts + 3 (such steps) - also where the roots are not asked for: the monitors are always
 * watched and counted.  Arguments, results, argument checks, status codes and the t0 == t1 behaviour are those of the RK45 entry of
 * the same name; messages start with "dop853:".  On these stability-limited equations DOP853 needs about as many evaluations as
 * RK45: it is here for coverage of the reference's solver switch, not as the cheaper method.
 * Only grids that fit one workgroup: N > 1024 returns -1, "dop853: ... N <= 1024 ..." (larger single grids: the two _grid entries
 * further down).  Terminal monitors: the four entries below return -1 with the standard message while a limit is set
 * (marl_set_terminal), before the state is touched; the two _stop entries after them honour the limits.  No slab contexts. */
/* marl_integrate_rk45 with DOP853: one instance, host pointers; t_eval frames and root times come from the sweep kernel that
 * locates roots (dop853_sweep_roots_kernel) run for one instance - no host in the loop. */
int marl_integrate_dop853(marl_ctx* ctx, double* y, double t0, double t1, double first_step, double rtol, double atol,
                          const double* t_eval, int64_t n_eval, double* y_eval, double* t_events, int64_t max_events,
                          int64_t max_attempts, marl_stats* stats);
/* marl_sweep_rk45_dev with DOP853 (rk.py, class DOP853; marlpde/parameters.py:212-213) */
int marl_sweep_dop853_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol,
                          double atol, int64_t max_attempts, marl_stats* stats);
/* marl_sweep_rk45_eval_dev with DOP853 (rk.py, class DOP853 and Dop853DenseOutput :577-601; ivp.py:706-723) */
int marl_sweep_dop853_eval_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol,
                               int64_t max_attempts, const double* t_eval, int64_t n_eval, double* y_eval_dev,
                               int64_t* n_done, marl_stats* stats);
/* marl_sweep_rk45_events_dev with DOP853 (rk.py, class DOP853; roots as ivp.py:673-694, :51-76) */
int marl_sweep_dop853_events_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol,
                                 int64_t max_attempts, const double* t_eval, int64_t n_eval, double* y_eval_dev,
                                 int64_t* n_done, double* t_events, int64_t max_events, marl_stats* stats);
/* marl_sweep_dop853_events_dev honouring terminal monitors (marl_set_terminal; the arguments of marl_sweep_rk45_terminal_dev).  With a
 * limit set the sweep is one launch of dop853_sweep_stop_kernel, whatever else was asked for: t_eval may be NULL with n_eval = 0 and
 * t_events NULL with max_events = 0.  An instance whose monitor meets its limit ends at that root inside the kernel: all roots of that
 * step are located by probe replays of the step, the rule is applied once, the samples up to t_stop are written, and one more replay
 * of the step with the weights of t_stop becomes the state (the STOP trip, csrc/marl_dop853.h).  nfev counts nothing for the stop: the
 * sign change has counted the step's dense output.  Every step that meets no limit is a step of marl_sweep_dop853_events_dev.  With
 * no limit set the call is marl_sweep_dop853_dev / _eval_dev / _events_dev, whichever the arguments ask for, bit for bit.
 * N > 1024 and slab contexts are refused as above. */
int marl_sweep_dop853_stop_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol,
                               int64_t max_attempts, const double* t_eval, int64_t n_eval, double* y_eval_dev,
                               int64_t* n_done, double* t_events, int64_t max_events, marl_stats* stats);
/* marl_integrate_dop853 honouring terminal monitors (the arguments of marl_integrate_rk45_terminal): the sweep above run for one
 * instance.  A run that a monitor ends: stats->status = 1, stats->t = t_stop, y the state at t_stop, y_eval the samples up to t_stop.
 * With no limit set it is marl_integrate_dop853. */
int marl_integrate_dop853_stop(marl_ctx* ctx, double* y, double t0, double t1, double first_step, double rtol, double atol,
                               const double* t_eval, int64_t n_eval, double* y_eval, double* t_events, int64_t max_events,
                               int64_t max_attempts, marl_stats* stats);

/* ---- DOP853 on one grid of any size: one launch per stage (csrc/marl_dop853_grid.h) ----
 * The large-grid counterpart of marl_integrate_dop853: on a grid of many workgroups a stage state needs its neighbours' stage
 * derivatives, which other workgroups own, so an attempt is 12 launches of dop853_grid_stage_kernel (256-thread windows that write
 * 254 cells; K_1..K_16 in an arena of 16 state-shaped buffers owned by the context), a reduction of the per-workgroup records in a
 * fixed order (two error sums, no float atomics: a run is reproducible bit for bit) and a control kernel.  The host enqueues batches
 * of `poll_interval` attempts and reads the status once per batch, as marl_integrate_rk45 does on a large grid; at a pause it locates
 * roots by Brent's method on dense evaluations (dop853_grid_dense_kernel) and writes the samples.
 * Arguments, checks, messages ("dop853: ..."), status codes and the t0 == t1 behaviour are those of marl_integrate_dop853 /
 * marl_integrate_rk23_dev; nfev = 1 + 12 attempts + 3 (accepted steps with a monitor sign change or a sample).  Any N is accepted,
 * N <= 1024 included (the two paths order their sums differently and agree to rounding, not bit for bit).
 * Terminal monitors (marl_set_terminal): marl_integrate_dop853_grid honours them as marl_integrate_rk45_terminal does - all roots of
 * the step located, the rule applied, the samples with t_eval[k] <= t_stop written, the state the step's dense output at t_stop,
 * stats->status = 1; marl_integrate_dop853_grid_dev refuses a limit with the standard message.
 * Refused with -1 before the state is touched: slab contexts, contexts of more than one instance. */
int marl_integrate_dop853_grid(marl_ctx* ctx, double* y, double t0, double t1, double first_step, double rtol, double atol,
                               const double* t_eval, int64_t n_eval, double* y_eval, double* t_events, int64_t max_events,
                               int64_t max_attempts, marl_stats* stats);
int marl_integrate_dop853_grid_dev(marl_ctx* ctx, double* y_dev, int layout, double t0, double t1, double first_step,
                                   double rtol, double atol, int64_t max_attempts, marl_stats* stats);

/* ---- implicit Radau IIA (order 5): the reference's DEFAULT solver ------------------------------------------------
 * Replaces  scipy.integrate.solve_ivp(fun, t_span, y0, method="Radau", jac_sparsity=jacobian_sparsity(), first_step=,
 * rtol=, atol=, t_eval=, events=[7 monitors])  as called at marlpde/Evolve_scenario.py:104-109 with the defaults of
 * marlpde/parameters.py:201-240 (method "Radau" :213; the 27-diagonal sparsity pattern :150-199).  Step logic:
 * scipy/integrate/_ivp/radau.py; Jacobian: scipy's finite-difference num_jac (common.py:268-451) over column groups, with
 * the reference's pattern (rows (f, i) x columns (f', i-1..i+1) minus CA/CC rows x Phi columns) - evaluated on the device,
 * as are the block-tridiagonal factorisations of the real and the complex collocation system and every vector operation.
 * groups (may be NULL): int32[5N], the column grouping scipy derives from the pattern (scipy.optimize._numdiff.group_columns);
 * NULL selects a structured 15-colouring - the Jacobian entries are the same either way (and scipy's nfev does not count the
 * finite-difference columns).  stats->nfev / njev / nlu are counted as scipy counts them.  Other arguments as for
 * marl_integrate_rk45.  Single-instance contexts only.  Terminal monitors (marl_set_terminal) end the run: status 1. */
int marl_integrate_radau(marl_ctx* ctx, double* y, double t0, double t1, double first_step, double rtol, double atol,
                         const int32_t* groups, const double* t_eval, int64_t n_eval, double* y_eval, double* t_events,
                         int64_t max_events, int64_t max_attempts, marl_stats* stats);
/* The same with scipy's BDF (scipy/integrate/_ivp/bdf.py: variable order 1..5, quasi-constant step NDF) - the other implicit method
 * the reference's Solver names for its jac_sparsity (marlpde/parameters.py:205-219); replaces
 * solve_ivp(fun, method="BDF", jac_sparsity=...) at marlpde/Evolve_scenario.py:104-109.  The matrix factorised is I - c J (one real
 * block-tridiagonal system per step size / order change, by cyclic reduction); arguments and statistics as for marl_integrate_radau. */
int marl_integrate_bdf(marl_ctx* ctx, double* y, double t0, double t1, double first_step, double rtol, double atol,
                         const int32_t* groups, const double* t_eval, int64_t n_eval, double* y_eval, double* t_events,
                         int64_t max_events, int64_t max_attempts, marl_stats* stats);

/* A SWEEP of Radau integrations (the reference integrates one scenario per process with this solver; its tests loop over
 * scenarios: tests/Regression_test/test_regression.py:44,74,115-116): every instance of the context with its own parameters, step-size
 * history and Newton convergence, advanced together - each instance's step logic runs as a state machine on the device, every
 * launch works on all instances that currently need that kind of work (csrc/marl_radau_batch.h).  y_dev: [n_instances][5N] FIELD-MAJOR
 * device states, advanced in place; stats: host array of n_instances entries (nfev / njev / nlu / status / t as scipy counts them;
 * monitor sign changes are counted in n_events, root times are not located in a sweep).  N <= 1638.  Synchronises.
 * Terminal monitors (marl_set_terminal): an instance whose monitor meets its limit ends there with status 1 - its controller locates
 * the roots of that step although this entry stores none, and one more action (A_STOP) writes the dense output at t_stop into its
 * state; the other instances are bit for bit what they are without the limit. */
int marl_sweep_radau_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol,
                         const int32_t* groups, int64_t max_attempts, marl_stats* stats);
/* The same sweep with the monitors' ROOT TIMES located inside it, as solve_ivp returns them for every run (sol.t_events,
 * marlpde/Evolve_scenario.py:118-145, 175-177; scipy ivp.py:673-694 with solve_event_equation :51-76): after an accepted step in
 * which a monitor changed sign, the instance's device-side controller runs Brent's method on the step's dense output - one
 * dense-output evaluation + monitors per function evaluation.  t_events: host array [instances][7][max_events]; entry k of
 * monitor e of instance b is valid for k < stats[b].n_events[e], the rest is NaN; sign changes beyond max_events are counted only.
 * Terminal monitors (marl_set_terminal): in the step that ends an instance's run only the roots up to the terminal one are stored
 * and counted; a kept root without a free slot is counted. */
int marl_sweep_radau_events_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol,
                                const int32_t* groups, int64_t max_attempts, double* t_events, int64_t max_events, marl_stats* stats);
/* The same sweep with t_eval: what the reference keeps of every run is the time series that solve_ivp(..., t_eval=) fills with its
 * default solver (marlpde/parameters.py:213; marlpde/Evolve_scenario.py:104-109), next to the root times (:118-145, 175-177).  As in
 * scipy the samples never change the steps (ivp.py:706-723): after every accepted step, once its roots are located, the instance's
 * controller asks for the samples inside the step one by one and the step's dense output (radau.py:557-572) is written into the
 * frame - no function evaluation is counted; state, statistics and root times are those of the same call without samples.
 * t_eval: host, n_eval times shared by all instances, strictly increasing within [t0, t1].
 * y_eval_dev: device, [n_instances][n_eval][5N], each frame contiguous and field-major.  n_done: host, n_instances entries: the frames
 * written for that instance (the samples with t_eval[k] <= the time it reached); its later frames are not touched.
 * t_events, max_events: as for marl_sweep_radau_events_dev; may be NULL / 0 (sign changes are then only counted).
 * n_eval = 0 (t_eval, y_eval_dev, n_done may then be NULL) is marl_sweep_radau_events_dev, or marl_sweep_radau_dev without t_events.
 * t1 == t0: no step is taken; a sample at t0 receives y0.  Synchronises.
 * Terminal monitors (marl_set_terminal): roots, then the stop, then the samples - an instance that ends at t_stop has the frames with
 * t_eval[k] <= t_stop, the last of them written from the step that ended it, and its state equals a frame at t_stop bit for bit. */
int marl_sweep_radau_eval_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol,
                              const int32_t* groups, int64_t max_attempts, const double* t_eval, int64_t n_eval, double* y_eval_dev,
                              int64_t* n_done, double* t_events, int64_t max_events, marl_stats* stats);
/* A SWEEP of BDF integrations: the other implicit method the reference's Solver names for its jac_sparsity
 * (marlpde/parameters.py:205-219), for many scenarios at once.  It replaces a loop of solve_ivp(method="BDF") runs (and this library's
 * own loop of marl_integrate_bdf runs, one busy workgroup and a host round trip per solve each): every instance follows scipy's BDF
 * step logic (scipy/integrate/_ivp/bdf.py:310-450, restated for one instance in bdf_run) as a device-side state machine
 * (csrc/marl_bdf_ctl.h), and the host repeats one fixed cycle of launches over work lists (csrc/marl_bdf_batch.h) - every kernel runs
 * to completion, none waits for another workgroup.  Semantics of marl_sweep_radau_dev: y_dev [n_instances][5N] FIELD-MAJOR, advanced
 * in place; stats[b]: nfev / njev / nlu / n_accepted / n_rejected / status / t / h_next as scipy counts them, n_events the monitors'
 * sign changes over accepted steps, event_value the monitors of the final state.  t1 == t0: no step, the state is untouched,
 * status 0, nfev = njev = 1 (BDF.__init__).  A failed solve is a status, not an error.  Synchronises.
 * Root times and t_eval frames: marl_sweep_bdf_events_dev / marl_sweep_bdf_eval_dev below (this entry counts sign changes only).
 * It does NOT: take grids whose solve does
 * not fit one workgroup (5 N <= 2048, N <= 409; larger: -1, use marl_integrate_bdf), or keep an instance in a persistent workgroup. */
int marl_sweep_bdf_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol,
                       const int32_t* groups, int64_t max_attempts, marl_stats* stats);
/* The same sweep with t_eval: the time series the reference keeps of every run (marlpde/Evolve_scenario.py:104-109) with the BDF
 * method of its Solver.  As in scipy the samples never change the steps (ivp.py:706-723); they are read from the dense output scipy
 * builds once _step_impl has returned (bdf.py:452-478): D[:order + 1], the order and the step size as they stand after the accepted
 * step's order / step-size selection and before the next step rescales D.  An accepted step that covers samples costs the instance
 * one more cycle; state and statistics are those of the same call without samples.
 * t_eval, y_eval_dev, n_done: as for marl_sweep_radau_eval_dev (frames [n_instances][n_eval][5N]; n_done[b] = the samples with
 * t_eval[k] <= the time instance b reached, also when it ended with status -1 or 2; its later frames are not touched).
 * n_eval = 0 (t_eval, y_eval_dev, n_done may then be NULL) is marl_sweep_bdf_dev.  t1 == t0: no step is taken and no frame is written,
 * as marl_integrate_bdf writes none.  Synchronises. */
int marl_sweep_bdf_eval_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol,
                            const int32_t* groups, int64_t max_attempts, const double* t_eval, int64_t n_eval, double* y_eval_dev,
                            int64_t* n_done, marl_stats* stats);
/* The same sweep with the monitors' ROOT TIMES located inside it, what solve_ivp returns as sol.t_events for every run
 * (marlpde/Evolve_scenario.py:118-145, 175-177; ivp.py:673-694 with solve_event_equation :51-76) - with this entry every way of
 * integrating returns them.  The roots are read from the dense output the samples are read from (after the accepted step's order /
 * step-size selection, before the next step rescales D), events before t_eval as in scipy: an accepted step over which monitors
 * changed sign costs the instance one more cycle (shared with its samples), in which one workgroup runs the whole Brent search of all
 * those monitors on the step's dense output (csrc/marl_bdf_batch.h, roots_batch_kernel).  State, statistics and frames are those of
 * the same call without roots.
 * t_events: host, [n_instances][7][max_events]; entry k of monitor e of instance b is valid for k < min(stats[b].n_events[e], max_events),
 * the rest is NaN; sign changes beyond max_events are counted only.  A run that ends with status -1 or 2 keeps the roots it located;
 * t1 == t0: none.  t_events == NULL or max_events <= 0 is marl_sweep_bdf_eval_dev; n_eval = 0 leaves the samples out.  Synchronises. */
int marl_sweep_bdf_events_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol,
                              const int32_t* groups, int64_t max_attempts, const double* t_eval, int64_t n_eval, double* y_eval_dev,
                              int64_t* n_done, double* t_events, int64_t max_events, marl_stats* stats);
/* The same sweep HONOURING TERMINAL MONITORS (marl_set_terminal; scipy's handle_events and the end of a terminated run, ivp.py:79-130,
 * 681-723; the rule: csrc/marl_terminal.h): the reference's `terminal` switch (marlpde/LHeureux_model.py:113-122) for BDF sweeps.  The
 * three entries above refuse a context with limits; this one stops every instance at its terminal monitor's root on the device.
 * In an accepted step over which a monitor changed sign that thereby meets its limit, the instance's controller (csrc/marl_bdf_ctl.h,
 * BdfTerm) has the roots of ALL monitors that changed sign located on the step's dense output - the search of the entry above, one
 * workgroup, with or without root slots or t_events - and in its next cycle applies the rule: the monitors up to and including the
 * terminal one in the order of root times are counted and, where a slot is free, stored; later ones never happened.  Then
 * stats[b].status = 1, stats[b].t = t_stop, the state of instance b is the step's dense output at t_stop (stop_state_batch_kernel: the
 * expression that writes a frame, so a frame at t_eval = t_stop equals it bit for bit), stats[b].event_value are that state's monitors,
 * the samples with t_eval[k] <= t_stop are written and counted in n_done[b], later frames stay untouched, and the counters are those
 * after the accepted step.  A stopped instance costs one cycle more and takes no further part: the sweep ends with its last live
 * instance.  Instances that meet no limit, and every step before the terminal one, run exactly as under marl_sweep_bdf_events_dev;
 * with no limit set this entry IS that one, bit for bit.  Arguments as for marl_sweep_bdf_events_dev (t_eval / n_eval = 0 and
 * t_events == NULL / max_events <= 0 allowed).  Synchronises. */
int marl_sweep_bdf_terminal_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol,
                                const int32_t* groups, int64_t max_attempts, const double* t_eval, int64_t n_eval, double* y_eval_dev,
                                int64_t* n_done, double* t_events, int64_t max_events, marl_stats* stats);

/* ---- 1-D domain decomposition of ONE large grid (BASELINE config 5; the reference never decomposes the depth
 * axis).  One process per GPU holds a slab [g_begin, g_end) of the N_global cells in a slab context; the host
 * layer moves halo strips between neighbours and the per-rank reduction records to everybody (RCCL
 * send/recv + all-gather on the context's stream) between these calls - see domain.py.  Slab state lives in the
 * context (FIELD-MAJOR, `halo` >= 6 extra cells on each interior side).  Strips are 2 x 5 x halo doubles:
 * [y | f][field][cell].  `which`: 0/1 an explicit state buffer, -1 the buffer the attempt in flight wrote,
 * -2 the current one.  Sequence:
 *   load -> pack(0) <-> unpack(0) -> rhs0 -> pack(0) <-> unpack(0) -> monitors -> [all-gather] -> init_control
 *   per attempt: attempt -> pack(-1) <-> unpack(-1) -> [all-gather records] -> control;   finally store.
 * Every rank feeds the SAME gathered records (in rank order) to init_control / control, so all ranks take
 * bit-identical accept/reject decisions without further synchronisation. */
int marl_ctx_create_slab(const marl_params* params, int64_t N_global, int64_t g_begin, int64_t g_end, int64_t halo,
                         int device, marl_ctx** out);
int marl_slab_load(marl_ctx* ctx, const double* y_owned_dev);  /* [5][g_end - g_begin] */
int marl_slab_store(marl_ctx* ctx, double* y_owned_dev);
int marl_slab_pack(marl_ctx* ctx, int which, double* send_lo_dev, double* send_hi_dev);
int marl_slab_unpack(marl_ctx* ctx, int which, const double* recv_lo_dev, const double* recv_hi_dev);
int marl_slab_rhs0(marl_ctx* ctx);                             /* f(t0, y0) on the owned cells */
int marl_slab_monitors(marl_ctx* ctx, double* rec_dev);        /* 8-double record of y0's monitors (owned cells) */
int marl_slab_init_control(marl_ctx* ctx, const double* recs_dev, int64_t nrec, double t0, double t1,
                           double first_step, double rtol, double atol, int64_t max_attempts);
int marl_slab_attempt(marl_ctx* ctx, double* rec_dev);         /* one fused Dormand-Prince attempt + its record */
int marl_slab_control(marl_ctx* ctx, const double* recs_dev, int64_t nrec);
int marl_slab_status(marl_ctx* ctx, marl_stats* stats);        /* synchronises */
/* The same loop with the exchange INSIDE the library (no host language in the per-attempt path): the ranks' messages
 * [record (8) | lower strip | upper strip] travel in one ncclAllGather on the context's stream.  The RCCL API is taken by
 * dlopen from the librccl the process already has (`rccl_path`, e.g. the one PyTorch-ROCm bundles; NULL: the loader's
 * default) - this library does not link RCCL.  Rank 0 makes the id (marl_slab_comm_id) and the host layer sends it to every
 * rank (any transport); comm_init with world = 1 and id = NULL runs one slab with no communicator.
 * Sequence:  comm_init -> load -> exchange(0) -> rhs0 -> monitors(NULL) -> exchange(0) -> init_control(NULL, world, ...) -> run
 * -> store.  marl_slab_run enqueues  attempt -> reduce + pack -> all-gather -> unpack + control  `poll_interval` attempts at a
 * time (never more than the attempt budget has left) and reads the status once per batch.
 * ncclCommInitRank is collective: marl_slab_comm_probe checks everything that is local (librccl loadable, entry points
 * present) so that the host layer can agree on the transport BEFORE any rank enters it; comm_init rejects an id that
 * marl_slab_comm_id cannot have produced (all zero) without touching RCCL. */
int marl_slab_comm_probe(const char* rccl_path);
int marl_slab_comm_id(const char* rccl_path, char id_out[128]);
int marl_slab_comm_init(marl_ctx* ctx, const char* rccl_path, const char id[128], int rank, int world);
int marl_slab_exchange(marl_ctx* ctx, int which);
int marl_slab_run(marl_ctx* ctx, marl_stats* stats);           /* synchronises */

#ifdef __cplusplus
}
#endif
#endif /* MARL_HIP_H */
