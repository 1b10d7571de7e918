// marl_api.hip - host side of libmarl_hip.so: context management, constant derivation and kernel
// launches behind the C ABI declared in include/marl_hip.h.  gfx950 only; no CPU fallback - every
// entry point needs a HIP device and fails with an error text otherwise.
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/marl_hip.h"
#include "marl_kernels.h"
#include "marl_rk23_ctl.h"
#include "marl_rk4_watch_ctl.h"
#include "marl_radau.h"
#include "marl_radau_cr.h"
#include "marl_radau_batch.h"
#include "marl_radau_wg.h"
#include "marl_bdf.h"
#include "marl_bdf_wg.h"
#include "marl_bdf_batch.h"
#include "marl_devbuf.h"

using namespace marl;

static_assert(MARL_NFIELDS == NF, "field count");
constexpr int64_t kChainMax = 8;   // longest chain of windows: what automatic mode may pick, option rk4_chain may force and the tests run
static thread_local std::string g_create_error;   // marl_ctx_create failures, per calling thread (contexts are created from worker threads too)

struct marl_ctx {
    int device = 0;
    hipStream_t stream = nullptr;  // nullptr = the device's default (null) stream, which is also torch's default current stream
    int64_t N = 0, batch = 0;
    Slab slab{};
    int halo = 0;  // > 0: a slab context of a domain-decomposed grid
    bool var_dphi = false;  // marl_params.dPhi_variable (the same for every instance): selects the VD kernel instantiations
    std::vector<marl_params> params;
    std::vector<DevConsts> hconsts;
    std::vector<double> extra;  // per instance: delta_x, auxcon, rhorat0, F_fixed (not needed on device)
    DevConsts* dconsts = nullptr;
    // device scratch (grown on demand)
    double* buf[4] = {nullptr, nullptr, nullptr, nullptr};  // Y0, Y1, F0, F1 (or staging)
    size_t buf_cap[4] = {0, 0, 0, 0};
    double* part = nullptr;
    size_t part_cap = 0;
    // streamed RK4 (rk4_stream_kernel): item counter (+ one spare word) + one published-level counter per tile; never reset
    // between launches - sq_item_base / sq_level_base say where they stand
    unsigned* sq = nullptr;
    size_t sq_cap = 0;
    unsigned sq_item_base = 0, sq_level_base = 0;
    bool sq_test_raise = false;    // test hook (option rk4_stream_test_raise): the next streamed run starts with the flag raised
    int64_t sq_max_items = 0x7fffffff;   // items per launch (the counter is 32 bits wide); test hook rk4_stream_max_items lowers it
    unsigned* sq_sticky = nullptr; // device: raised by a streamed run that gave up waiting; cleared by the host only
    unsigned* sq_host = nullptr;   // pinned: copy of sq_sticky
    bool sq_pending = false;       // streamed runs since sq_sticky was last looked at
    int cus = 0;
    // persistent adaptive loop (rk45_stream_kernel): barrier / publication words, one record per resident workgroup; the ticket and
    // barrier counters are never reset between launches - rs_arrive_base / rs_epoch_base say where they stand
    Rk45Stream* rs = nullptr;
    double* rs_grec = nullptr;
    unsigned* rs_host = nullptr;   // pinned: copy of {arrive, sticky}
    unsigned rs_arrive_base = 0, rs_epoch_base = 0, rs_grab_base = 0, rs_G = 0, rs_grabs_per_attempt = 0;
    int rs_occ[3][2] = {{0, 0}, {0, 0}, {0, 0}};   // resident workgroups per CU of the instantiation [field-major / tiled / one attempt per launch][VD]
    int64_t rk45_stream = 1;       // the adaptive loop of one grid as ONE launch per batch of attempts (rk45_stream_kernel): 0 never, 1 where it is faster (grids of up to kRk45StreamRounds rounds of resident workgroups), 2 always
    int64_t dd_stream = 0;         // domain-decomposed loop inside the library: 0 (default) attempt + reduce + pack launches; 1 / 2: the slab's attempt as ONE launch of the persistent kernel whose last workgroup packs the rank's message (1: slabs of up to kRk45StreamRounds rounds, 2: always) - built for the 8-GPU shard size and measured there NOT faster (44.5 us against 34.9 + 4.7 + 4.7 us, profiles/r04_lab_rk45_stream.log)
    int64_t rk45_stream_attempts = 4096;   // attempts per launch at most (the host looks at the status and the sticky flag in between)
    double* rec = nullptr;  // [batch][NQ]
    Rk45Ctrl* dctrl = nullptr;
    Rk45Ctrl* hctrl = nullptr;  // pinned
    double* hrec = nullptr;     // pinned [batch][NQ]
    double* ddt = nullptr;      // [batch] per-instance dt
    double* hdt = nullptr;      // pinned [batch]: staging of the caller's dt array (the caller's buffer may die before the copy runs)
    // sweeps with t_eval (rk45_sweep_eval_kernel): the sample times and the frames written per instance, allocated on first use
    double* sw_teval = nullptr;
    size_t sw_teval_cap = 0;
    int64_t* sw_ndone = nullptr;   // [batch]
    // sweeps that locate the monitors' roots (rk45_sweep_roots_kernel): the root times [batch][7][max_events], allocated on first use or growth
    double* sw_tev = nullptr;
    size_t sw_tev_cap = 0;
    // DOP853 sweeps (marl_dop853.h): the stage derivatives of every instance, [batch][16][5][window]; allocated on first use or growth.
    // Large-grid DOP853 runs (marl_dop853_grid.h) keep their arena here too: 16 state-shaped buffers in the layout of the state.
    double* dop_k = nullptr;
    size_t dop_k_cap = 0;
    // monitored RK4 sweeps (marl_rk4_watch.h): the per-instance records, Rk4WatchRec[batch] as doubles, then the seven terminal limits; allocated on first use
    double* rk4w_recs = nullptr;
    size_t rk4w_recs_cap = 0;
    int64_t dop_grid_extra = -1;   // large-grid DOP853: the accepted step (its n_acc) whose extra stages K14..K16 lie in the arena; -1: none
    // domain decomposition: this rank's message / the gathered messages (device), and the RCCL communicator (dlopen'ed API)
    double* dd_send = nullptr;
    double* dd_gathered = nullptr;
    double* dd_recs = nullptr;
    int dd_rank = 0, dd_world = 1;
    int64_t dd_max_attempts = 0;   // the attempt budget given to marl_slab_init_control (marl_slab_run sizes its batches by it)
    void* rccl_lib = nullptr;
    void* rccl_comm = nullptr;
    int (*rccl_allgather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    int (*rccl_destroy)(void*) = nullptr;
    // implicit (Radau) path: one device arena + a small pinned read-back area
    double* rd_arena = nullptr;
    size_t rd_cap = 0;
    double* rd_host = nullptr;  // pinned: [0] norm^2, [1] flags (as int32), [2..] spare
    // zero-copy result words of the single-instance implicit drivers: coherent host memory the kernels write their scalar results
    // into and the host polls - no copy, no stream synchronisation per Newton iteration.  [0] a sum of squares, [1] the non-finite flag
    // (int32), [8..15] a monitors record.  A slot is "armed" with a NaN of a payload no computation produces until its kernel writes it.
    double* zc_h = nullptr;     // host view
    double* zc_d = nullptr;     // device view of the same memory
    bool zc_on = false;         // the run in progress uses it
    // options
    int64_t rk4_variant = -1, sweep_variant = -1, host_layout = LAYOUT_TILED, poll = 64;
    int64_t rk4_stream = 1;     // the fixed-step loop of one grid as ONE dataflow launch (rk4_stream_kernel): 0 never, 1 large grids, 2 always
    int64_t rk4_small = 1;      // grids of up to two workgroups per CU at 16 steps per launch: the build of marl_rk4_small.hip (0: the common one)
    // chained windows in the streamed loop (rk4_chain_kernel; 4 steps per level, constant porosity diffusion): 0 never, 1 automatic
    // (rk4_chain_auto below), K >= 2: chains of K windows whenever that path is taken
    int64_t rk4_chain = 1;
    // the LDS layout of the chained kernel: 0 = exchange buffer by field, cache slots one by one (rk4_chain_kernel); 1 = exchange buffer
    // by cell, cache slots in pairs (rk4_exchange_kernel: 16-byte LDS accesses, the same results bit for bit)
    int64_t rk4_exchange = 1;
    int64_t rk4_stream_third = 1;   // an odd number of levels goes through a third state buffer, so that no whole-state copy follows (0: copy)
    double* stream_c = nullptr;
    size_t stream_c_cap = 0;
    int64_t implicit_zero_copy = 1;  // scalar results of the implicit drivers through polled host memory (0: copy + synchronise)
    int64_t radau_fused_solve = 3;   // small systems (5 N <= 2048): >= 1: all levels of a solve in one launch (BDF: the whole Newton iteration / solve_bdf_system); Radau single runs: 3 (default) = two launches per Newton iteration (solves with their own right-hand sides | update + norm + the next stage derivatives), 2 = the whole iteration's linear algebra in ONE workgroup (bit-identical, measured slower: the two chains then share one compute unit), 1 = four launches; 0: one launch per level
    int64_t radau_solver = 0;   // 0: block parallel cyclic reduction (parallel over depth); 1: sequential block Thomas
    int64_t radau_cr = -1;      // single runs: levels of cyclic reduction in front of PCR; -1 = automatic (grids of >= radau_cr_min_n cells: down to a
                                // compact system that fits the one-launch solve with one unknown per thread), 0 = none
    int64_t radau_cr_min_n = 2048;
    int64_t radau_cr_small = 3; // grids solved in one workgroup (up to 409 cells): levels of cyclic reduction in front of PCR (0: none)
    int64_t radau_cr_small_min_n = 205;   // ... from this many cells on (below: plain PCR, which reproduces scipy's decisions on the reference's N = 200 runs)
    int64_t bdf_solve_wg = 1;   // small grids: solve_bdf_system as one launch of one workgroup (marl_bdf_wg.h); 0: one launch + wait per Newton iteration
    int64_t radau_cr_tail = 1;  // the launch-bound levels of a cyclic-reduction solve in one launch each way (0: one launch per level)
    int64_t radau_sweep_wg = 3; // sweeps of small grids: 3 hybrid (workgroup per instance for the sequential work and Jacobians, launch kernels for factorisations), 1 hybrid with launch kernels for Jacobians too, 2 all in the workgroup, 0 launch per action
    int64_t terminal[7] = {0, 0, 0, 0, 0, 0, 0};   // marl_set_terminal: monitor e ends a run at its terminal[e]-th occurrence (0: never - the reference's `terminal = False`)
    std::string err;
};

static bool has_terminal(const marl_ctx* ctx)
{
    for (int e = 0; e < 7; e++)
        if (ctx->terminal[e] > 0) return true;
    return false;
}

static int fail(marl_ctx* ctx, int code, const char* fmt, ...);
// the entries that do not stop at a terminal monitor yet refuse a context that has one, before they touch anything
#define NO_TERMINAL(ctx, entry) \
    if (has_terminal(ctx)) return fail(ctx, -1, "%s: terminal monitors are not supported by this entry (marl_set_terminal)", entry);

static int fail(marl_ctx* ctx, int code, const char* fmt, ...)
{
    char msg[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof msg, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = msg; else g_create_error = msg;
    return code;
}

#define HIP_OK(ctx, call)                                                                         \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) return fail(ctx, -100 - (int)e_, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

#define LAUNCH_OK(ctx)                                                                            \
    do {                                                                                          \
        hipError_t e_ = hipGetLastError();                                                        \
        if (e_ != hipSuccess) return fail(ctx, -100 - (int)e_, "kernel launch failed: %s", hipGetErrorString(e_)); \
    } while (0)

#ifdef MARL_LAB_CLOCK45
extern "C" int marl_lab_read_clock45(unsigned long long* dst, size_t n)
{
    return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(marl::marl_lab_clock45), n * sizeof(unsigned long long));
}
extern "C" int marl_lab_read_clock45t(unsigned long long* dst, size_t n)
{
    return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(marl::marl_lab_clock45t), n * sizeof(unsigned long long));
}
#endif

// ----------------------------------------------------------------------------------------------
// Derived constants: LMAHeureuxPorosityDiff.__init__, marlpde/LHeureux_model.py:23-24, :36-72,
// :87-88, :130-133; depth mask: marlpde/Evolve_scenario.py:51-54.
// ----------------------------------------------------------------------------------------------
static void derive_consts(const marl_params& p, int64_t N, DevConsts& c, double extra[4])
{
    const double g = 100 * 9.81;
    const double dx = p.length / (double)N;
    const double delta_x = (0.0 + 1.5 * dx) - (0.0 + 0.5 * dx);  // x[1] - x[0] of the cell centres (:23-24)
    const double dCa = p.DCa / p.D0Ca, dCO3 = p.DCO3 / p.D0Ca;
    const double auxcon = p.beta / (p.D0Ca * p.b * g * p.rhow * (p.PhiNR - p.PhiInfty));
    const double rhorat0 = (p.rhos0 / p.rhow - 1) * p.beta / p.sedimentationrate;
    const double F_fixed = 1 - std::exp(10 - 10 / p.PhiIni);
    memset(&c, 0, sizeof c);
    HotConsts& k = c.hot;
    k.inv_dx = 1.0 / dx;
    k.inv_dx2 = std::pow(dx, -2);
    k.dCa = dCa;
    k.dCO3 = dCO3;
    k.dPhi = auxcon * F_fixed * std::pow(p.PhiIni, 3) / (1 - p.PhiIni);
    k.pe_cCa = delta_x / (2. * dCa);
    k.pe_cCO3 = delta_x / (2. * dCO3);
    k.pe_Phi = delta_x / (2. * k.dPhi);
    k.presum = 1 - rhorat0 * std::pow(p.Phi0, 3) * (1 - std::exp(10 - 10 / p.Phi0)) / (1 - p.Phi0);
    k.rhorat = (p.rhos / p.rhow - 1) * p.beta / p.sedimentationrate;
    k.KRat = p.KC / p.KA;
    k.nu1 = p.k1 / p.k2;
    k.nu2 = p.k4 / p.k3;
    k.m1 = p.m1; k.m2 = p.m2; k.n1 = p.n1; k.n2 = p.n2;
    c.p0_m1 = std::pow(0.0, p.m1); c.p0_m2 = std::pow(0.0, p.m2);
    c.p0_n1 = std::pow(0.0, p.n1); c.p0_n2 = std::pow(0.0, p.n2);
    // exponents <= 0: pow(0, e) != 0, the clamp pairs need the general combination; exponents < 1: the stage-reuse
    // expansions' range check (|u| <= |n u|) does not hold - both take the general, cache-less evaluation
    k.generic_p0 = (c.p0_m1 != 0 || c.p0_m2 != 0 || c.p0_n1 != 0 || c.p0_n2 != 0 || !(p.m1 >= 1) || !(p.m2 >= 1) || !(p.n1 >= 1) || !(p.n2 >= 1)) ? 1 : 0;
    k.lambda_ = p.k3 / p.k2;
    k.Da = p.k2 * p.Tstar;
    k.delta = p.rhos / (p.muA * std::sqrt(p.KC));
    k.hdx = 0.5 * k.inv_dx;
    k.pe_smax = k.pe_cCa > k.pe_cCO3 ? k.pe_cCa : k.pe_cCO3;
    k.Dal = k.Da * k.lambda_;
    k.Da_nu1 = k.Da * k.nu1;
    k.Dal_nu2 = k.Dal * k.nu2;
    k.rr10 = 10.0 * k.rhorat;
    k.dPhi_dx2 = k.dPhi * k.inv_dx2;
    k.auxcon = auxcon;
    k.var_dphi = p.dPhi_variable ? 1 : 0;
    const double bc[NF] = {p.CA0, p.CC0, p.cCa0, p.cCO30, p.Phi0};
    for (int f = 0; f < NF; f++) c.bc[f] = bc[f];
    c.N = N;
    k.fv = p.FV_switch;
    // mask = H(x - shallow) * H(deep - x) with H(0) = 0 at the cell centres: a contiguous index range
    int64_t lo = N, hi = N;
    bool open = false;
    for (int64_t i = 0; i < N; i++) {
        const double x = 0.0 + ((double)i + 0.5) * dx;
        const bool in = (x - p.shallow_limit > 0) && (p.deep_limit - x > 0);
        if (in && !open) { lo = i; open = true; }
        if (!in && open) { hi = i; break; }
    }
    if (!open) lo = hi = 0;
    c.mask_lo = lo;
    c.mask_hi = hi;
    extra[0] = delta_x; extra[1] = auxcon; extra[2] = rhorat0; extra[3] = F_fixed;
}

static int ensure(marl_ctx* ctx, int which, size_t doubles)
{
    if (ctx->buf_cap[which] >= doubles) return 0;
    if (ctx->buf[which]) HIP_OK(ctx, hipFree(ctx->buf[which]));
    ctx->buf[which] = nullptr;
    ctx->buf_cap[which] = 0;
    HIP_OK(ctx, hipMalloc((void**)&ctx->buf[which], doubles * sizeof(double)));
    ctx->buf_cap[which] = doubles;
    return 0;
}

static int ensure_part(marl_ctx* ctx, size_t records)
{
    if (ctx->part_cap >= records) return 0;
    if (ctx->part) HIP_OK(ctx, hipFree(ctx->part));
    ctx->part = nullptr;
    ctx->part_cap = 0;
    HIP_OK(ctx, hipMalloc((void**)&ctx->part, records * NQ * sizeof(double)));
    ctx->part_cap = records;
    return 0;
}

// validate_tol (scipy/integrate/_ivp/common.py:44-51): rtol below 100 eps is raised to it
static double clamp_rtol(double rtol) { const double lo = 100 * 2.220446049250313e-16; return rtol < lo ? lo : rtol; }

static int64_t state_doubles(int64_t n, int layout)
{
    return layout == LAYOUT_TILED ? ((n + 63) / 64) * (int64_t)(NF * 64) : (int64_t)NF * n;
}

extern "C" {

int marl_ctx_create(const marl_params* params, int64_t n_instances, int64_t N, int device, marl_ctx** out)
{
    if (!params || !out || n_instances < 1 || N < 2) return fail(nullptr, -1, "marl_ctx_create: invalid argument");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
        return fail(nullptr, -2, "marl_ctx_create: no HIP device (%s); this library has no CPU path", hipGetErrorString(e));
    if (device < 0 || device >= ndev) return fail(nullptr, -1, "marl_ctx_create: device %d out of range (0..%d)", device, ndev - 1);
    marl_ctx* ctx = new marl_ctx;
    ctx->device = device;
    ctx->N = N;
    ctx->batch = n_instances;
    ctx->slab = Slab{N, 0, N, 0, N};
    ctx->params.assign(params, params + n_instances);
    ctx->hconsts.resize(n_instances);
    ctx->extra.resize(4 * n_instances);
    for (int64_t b = 0; b < n_instances; b++) {
        const marl_params& p = params[b];
        if (!(p.length > 0)) { delete ctx; return fail(nullptr, -1, "marl_ctx_create: instance %lld: length must be > 0", (long long)b); }
        if ((p.dPhi_variable != 0) != (params[0].dPhi_variable != 0)) {
            delete ctx;
            return fail(nullptr, -1, "marl_ctx_create: dPhi_variable must be the same for every instance of a sweep");
        }
        derive_consts(p, N, ctx->hconsts[b], &ctx->extra[4 * b]);
    }
    ctx->var_dphi = params[0].dPhi_variable != 0;
#define CREATE_OK(call)                                                                     \
    do {                                                                                    \
        hipError_t e2_ = (call);                                                            \
        if (e2_ != hipSuccess) {                                                            \
            fail(nullptr, -100 - (int)e2_, "%s failed: %s", #call, hipGetErrorString(e2_)); \
            marl_ctx_destroy(ctx);                                                          \
            return -100 - (int)e2_;                                                         \
        }                                                                                   \
    } while (0)
    CREATE_OK(hipSetDevice(device));
    CREATE_OK(hipMalloc((void**)&ctx->dconsts, sizeof(DevConsts) * n_instances));
    CREATE_OK(hipMemcpy(ctx->dconsts, ctx->hconsts.data(), sizeof(DevConsts) * n_instances, hipMemcpyHostToDevice));
    CREATE_OK(hipMalloc((void**)&ctx->rec, sizeof(double) * NQ * n_instances));
    CREATE_OK(hipMalloc((void**)&ctx->dctrl, sizeof(Rk45Ctrl) * n_instances));
    CREATE_OK(hipMalloc((void**)&ctx->ddt, sizeof(double) * n_instances));
    CREATE_OK(hipHostMalloc((void**)&ctx->hctrl, sizeof(Rk45Ctrl) * n_instances, hipHostMallocDefault));
    CREATE_OK(hipHostMalloc((void**)&ctx->hrec, sizeof(double) * NQ * n_instances, hipHostMallocDefault));
    CREATE_OK(hipHostMalloc((void**)&ctx->hdt, sizeof(double) * n_instances, hipHostMallocDefault));
#undef CREATE_OK
    *out = ctx;
    return 0;
}

// New parameters for an existing context (same N, same number of instances): the derived constants are recomputed and uploaded; every
// buffer the context has grown stays (a loop over scenarios pays for its allocations once).  The time-varying dPhi switch may change.
int marl_ctx_set_params(marl_ctx* ctx, const marl_params* params, int64_t n_instances)
{
    if (!ctx || !params) return ctx ? fail(ctx, -1, "marl_ctx_set_params: invalid argument") : -1;
    if (n_instances != ctx->batch) return fail(ctx, -1, "marl_ctx_set_params: the context holds %lld instance(s)", (long long)ctx->batch);
    if (ctx->halo > 0) return fail(ctx, -1, "marl_ctx_set_params: not for slab contexts");
    for (int64_t b = 0; b < n_instances; b++) {
        if (!(params[b].length > 0)) return fail(ctx, -1, "marl_ctx_set_params: instance %lld: length must be > 0", (long long)b);
        if ((params[b].dPhi_variable != 0) != (params[0].dPhi_variable != 0))
            return fail(ctx, -1, "marl_ctx_set_params: dPhi_variable must be the same for every instance of a sweep");
    }
    HIP_OK(ctx, hipSetDevice(ctx->device));
    HIP_OK(ctx, hipStreamSynchronize(ctx->stream));   // nothing in flight reads the old constants
    ctx->params.assign(params, params + n_instances);
    const int no_reuse = ctx->hconsts[0].hot.no_reuse;   // (an option of the context, kept)
    for (int64_t b = 0; b < n_instances; b++) {
        derive_consts(params[b], ctx->N, ctx->hconsts[b], &ctx->extra[4 * b]);
        ctx->hconsts[b].hot.no_reuse = no_reuse;
    }
    ctx->var_dphi = params[0].dPhi_variable != 0;
    HIP_OK(ctx, hipMemcpyAsync(ctx->dconsts, ctx->hconsts.data(), sizeof(DevConsts) * n_instances, hipMemcpyHostToDevice, ctx->stream));
    HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

void marl_ctx_destroy(marl_ctx* ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (int i = 0; i < 4; i++)
        if (ctx->buf[i]) (void)hipFree(ctx->buf[i]);
    if (ctx->part) (void)hipFree(ctx->part);
    if (ctx->stream_c) (void)hipFree(ctx->stream_c);
    if (ctx->sq) (void)hipFree(ctx->sq);
    if (ctx->sq_sticky) (void)hipFree(ctx->sq_sticky);
    if (ctx->sq_host) (void)hipHostFree(ctx->sq_host);
    if (ctx->rs) (void)hipFree(ctx->rs);
    if (ctx->rs_grec) (void)hipFree(ctx->rs_grec);
    if (ctx->rs_host) (void)hipHostFree(ctx->rs_host);
    if (ctx->rec) (void)hipFree(ctx->rec);
    if (ctx->dctrl) (void)hipFree(ctx->dctrl);
    if (ctx->ddt) (void)hipFree(ctx->ddt);
    if (ctx->dconsts) (void)hipFree(ctx->dconsts);
    if (ctx->hctrl) (void)hipHostFree(ctx->hctrl);
    if (ctx->hrec) (void)hipHostFree(ctx->hrec);
    if (ctx->hdt) (void)hipHostFree(ctx->hdt);
    if (ctx->sw_teval) (void)hipFree(ctx->sw_teval);
    if (ctx->sw_ndone) (void)hipFree(ctx->sw_ndone);
    if (ctx->sw_tev) (void)hipFree(ctx->sw_tev);
    if (ctx->dop_k) (void)hipFree(ctx->dop_k);
    if (ctx->rk4w_recs) (void)hipFree(ctx->rk4w_recs);
    if (ctx->rccl_comm && ctx->rccl_destroy) (void)ctx->rccl_destroy(ctx->rccl_comm);
    if (ctx->dd_send) (void)hipFree(ctx->dd_send);
    if (ctx->dd_gathered) (void)hipFree(ctx->dd_gathered);
    if (ctx->dd_recs) (void)hipFree(ctx->dd_recs);
    if (ctx->rd_arena) (void)hipFree(ctx->rd_arena);
    if (ctx->rd_host) (void)hipHostFree(ctx->rd_host);
    if (ctx->zc_h) (void)hipHostFree(ctx->zc_h);
    delete ctx;
}

const char* marl_last_error(const marl_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int marl_set_stream(marl_ctx* ctx, void* hip_stream)
{
    if (!ctx) return -1;
    ctx->stream = (hipStream_t)hip_stream;
    return 0;
}

// A streamed RK4 run (rk4_stream_kernel) that gave up waiting raises a sticky device flag; the device entry points stay
// asynchronous, so the flag is looked at where the caller synchronises anyway: marl_synchronize and the host-pointer entry points.
static int stream_check(marl_ctx* ctx)
{
    if (!ctx->sq_pending) return 0;
    HIP_OK(ctx, hipMemcpyAsync(ctx->sq_host, ctx->sq_sticky, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->sq_pending = false;
    if (*ctx->sq_host) {
        HIP_OK(ctx, hipMemsetAsync(ctx->sq_sticky, 0, sizeof(unsigned), ctx->stream));
        if (ctx->sq) HIP_OK(ctx, hipMemsetAsync(ctx->sq, 0, ctx->sq_cap * sizeof(unsigned), ctx->stream));
        ctx->sq_item_base = ctx->sq_level_base = 0;
        return fail(ctx, -2, "rk4: the streamed time loop gave up waiting for a neighbouring tile (rk4_stream_kernel); the state is invalid");
    }
    return 0;
}

int marl_set_terminal(marl_ctx* ctx, const int64_t terminal[7])
{
    if (!ctx) return -1;
    for (int e = 0; terminal && e < 7; e++)
        if (terminal[e] < 0) return fail(ctx, -1, "marl_set_terminal: limit %d is negative (0: never terminal; k > 0: stop at the k-th occurrence)", e);
    for (int e = 0; e < 7; e++) ctx->terminal[e] = terminal ? terminal[e] : 0;
    return 0;
}

int marl_synchronize(marl_ctx* ctx)
{
    if (!ctx) return -1;
    HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
    return stream_check(ctx);
}

int marl_set_option(marl_ctx* ctx, const char* name, int64_t value)
{
    if (!ctx || !name) return -1;
    const std::string n(name);
    if (n == "rk4_variant") ctx->rk4_variant = value;
    else if (n == "rk45_variant") { }   // accepted, no effect: the adaptive kernels have one shape
    else if (n == "sweep_variant") ctx->sweep_variant = value;
    else if (n == "host_layout") ctx->host_layout = value ? LAYOUT_TILED : LAYOUT_FIELD_MAJOR;
    else if (n == "poll_interval") ctx->poll = value > 0 ? value : 1;
    else if (n == "radau_solver") {
#ifdef MARL_LAB_BLOCK_THOMAS
        ctx->radau_solver = value ? 1 : 0;
#else
        if (value) return fail(ctx, -1, "marl_set_option: radau_solver = 1 (sequential block Thomas, the cross-check of the cyclic-reduction solver) is compiled into lab builds only (-DMARL_LAB_BLOCK_THOMAS)");
        ctx->radau_solver = 0;
#endif
    }
    else if (n == "radau_cr") ctx->radau_cr = (value < 0) ? -1 : std::min<int64_t>(value, radau::CR_MAX_LEVELS);
    else if (n == "radau_cr_min_n") ctx->radau_cr_min_n = std::max<int64_t>(value, 4);
    else if (n == "radau_cr_small") ctx->radau_cr_small = value < 0 ? 0 : std::min<int64_t>(value, radau::CR_WG_MAX_LEVELS);
    else if (n == "radau_cr_small_min_n") ctx->radau_cr_small_min_n = std::max<int64_t>(value, 32);
    else if (n == "radau_cr_tail") ctx->radau_cr_tail = value ? 1 : 0;
    else if (n == "bdf_solve_wg") ctx->bdf_solve_wg = value ? 1 : 0;
    else if (n == "radau_fused_solve") ctx->radau_fused_solve = value < 0 ? 0 : (value > 3 ? 3 : value);
    else if (n == "radau_sweep_wg") ctx->radau_sweep_wg = value < 0 ? 0 : (value > 3 ? 3 : value);
    else if (n == "implicit_zero_copy") ctx->implicit_zero_copy = value ? 1 : 0;
    else if (n == "rk4_stream") ctx->rk4_stream = value < 0 ? 0 : (value > 2 ? 2 : value);
    else if (n == "rk45_stream") ctx->rk45_stream = value < 0 ? 0 : (value > 2 ? 2 : value);
    else if (n == "dd_stream") ctx->dd_stream = value < 0 ? 0 : (value > 2 ? 2 : value);
    else if (n == "rk45_stream_attempts") ctx->rk45_stream_attempts = value < 1 ? 1 : std::min<int64_t>(value, 1 << 20);
    else if (n == "rk4_small") ctx->rk4_small = value ? 1 : 0;
    else if (n == "rk4_chain") ctx->rk4_chain = value < 0 ? 0 : std::min<int64_t>(value, kChainMax);
#ifdef MARL_LAB_XCH_PARTS   // (lab builds: 1 = by cell only, 2 = pairs only, 3 = both)
    else if (n == "rk4_exchange") ctx->rk4_exchange = value < 0 ? 0 : std::min<int64_t>(value, 3);
#else
    else if (n == "rk4_exchange") ctx->rk4_exchange = value ? 1 : 0;
#endif
    else if (n == "rk4_stream_third") ctx->rk4_stream_third = value ? 1 : 0;
    else if (n == "rk4_stream_test_raise") ctx->sq_test_raise = value != 0;
    else if (n == "rk4_stream_max_items") ctx->sq_max_items = value > 0 ? std::min<int64_t>(value, 0x7fffffff) : 0x7fffffff;
    else if (n == "no_reuse") {
        // every evaluation of the fused kernels takes its full path (what a rough state does wave by wave): re-upload the constants
        for (auto& c : ctx->hconsts) c.hot.no_reuse = value ? 1 : 0;
        HIP_OK(ctx, hipSetDevice(ctx->device));
        HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
        HIP_OK(ctx, hipMemcpy(ctx->dconsts, ctx->hconsts.data(), sizeof(DevConsts) * ctx->hconsts.size(), hipMemcpyHostToDevice));
    }
    else return fail(ctx, -1, "marl_set_option: unknown option '%s'", name);
    return 0;
}

int marl_get_constants(const marl_ctx* ctx, int64_t inst, double out[19])
{
    if (!ctx || inst < 0 || inst >= ctx->batch || !out) return -1;
    const DevConsts& d = ctx->hconsts[inst];
    const HotConsts& c = d.hot;
    const double* x = &ctx->extra[4 * inst];
    const double v[19] = {x[0], c.nu1, c.nu2, c.KRat, c.dCa, c.dCO3, c.delta, c.Da, c.lambda_, x[1], x[2], c.rhorat,
                          c.presum, x[3], c.dPhi, PECLET_MIN, PECLET_MAX, (double)d.mask_lo, (double)d.mask_hi};
    memcpy(out, v, sizeof v);
    return 0;
}

int64_t marl_state_doubles(const marl_ctx* ctx, int layout) { return ctx ? state_doubles(ctx->slab.n_buf, layout) : -1; }

}  // extern "C"

#ifndef MARL_LAB  // tools/rk4_lab.hip includes this file for context creation only
// ----------------------------------------------------------------------------------------------
// launch helpers
// ----------------------------------------------------------------------------------------------
static inline int64_t inst_stride(const marl_ctx* ctx, int layout) { return state_doubles(ctx->slab.n_buf, layout); }

static inline unsigned blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }

// "no batch": what every kernel with a trailing ZBatch takes by default - a single run is the cnt = 1 case of a batched launch
static const ZBatch kNoBatch{0, nullptr, 0, 0, nullptr};

// Field-major states -> their derivatives: `nstates` states one after another, for each of the `cnt` instances of `zb` (blockIdx.z).
// const_stride 0: the states of an instance share its ONE model (stage states, finite-difference columns); 1: one model per state.
// The stride between states is 5 n_buf doubles; on a whole-grid context (n_buf = N: marl_ctx_create) that is the 5 N of the implicit path.
static int launch_rhs_fm(marl_ctx* ctx, const double* y, double* dydt, int64_t nstates, unsigned cnt = 1, const ZBatch& zb = kNoBatch,
                         int const_stride = 0)
{
    const dim3 grid(blocks256(ctx->slab.n_buf), (unsigned)nstates, cnt);
    const int64_t stride = inst_stride(ctx, LAYOUT_FIELD_MAJOR);
    if (ctx->var_dphi)
        hipLaunchKernelGGL((rhs_kernel<LAYOUT_FIELD_MAJOR, true>), grid, dim3(256), 0, ctx->stream, y, dydt, ctx->dconsts, ctx->slab, stride, const_stride, zb);
    else
        hipLaunchKernelGGL(rhs_kernel<LAYOUT_FIELD_MAJOR>, grid, dim3(256), 0, ctx->stream, y, dydt, ctx->dconsts, ctx->slab, stride, const_stride, zb);
    LAUNCH_OK(ctx);
    return 0;
}

// nstates > 0: that many states of the ONE model of the context, one after another (implicit path); 0: one state per instance
static int launch_rhs(marl_ctx* ctx, const double* y, double* dydt, int layout, int64_t nstates = 0)
{
    if (layout != LAYOUT_TILED) return launch_rhs_fm(ctx, y, dydt, nstates > 0 ? nstates : ctx->batch, 1, kNoBatch, nstates > 0 ? 0 : 1);
    const dim3 grid(blocks256(ctx->slab.n_buf), (unsigned)(nstates > 0 ? nstates : ctx->batch));
    const int64_t stride = inst_stride(ctx, layout);
    const int cs = nstates > 0 ? 0 : 1;
    if (ctx->var_dphi)
        hipLaunchKernelGGL((rhs_kernel<LAYOUT_TILED, true>), grid, dim3(256), 0, ctx->stream, y, dydt, ctx->dconsts, ctx->slab, stride, cs);
    else
        hipLaunchKernelGGL(rhs_kernel<LAYOUT_TILED>, grid, dim3(256), 0, ctx->stream, y, dydt, ctx->dconsts, ctx->slab, stride, cs);
    LAUNCH_OK(ctx);
    return 0;
}

static int launch_convert(marl_ctx* ctx, const double* src, double* dst, int sl, int dl)
{
    const int64_t n = ctx->slab.n_buf;
    if (sl == dl) {
        HIP_OK(ctx, hipMemcpyAsync(dst, src, sizeof(double) * state_doubles(n, sl) * ctx->batch, hipMemcpyDeviceToDevice, ctx->stream));
        return 0;
    }
    const dim3 grid((unsigned)((n + 255) / 256), (unsigned)ctx->batch);
    if (sl == LAYOUT_FIELD_MAJOR)
        hipLaunchKernelGGL((convert_kernel<LAYOUT_FIELD_MAJOR, LAYOUT_TILED>), grid, dim3(256), 0, ctx->stream, src, dst, n,
                           ctx->slab.ld, (int64_t)0, state_doubles(n, sl), state_doubles(n, dl));
    else
        hipLaunchKernelGGL((convert_kernel<LAYOUT_TILED, LAYOUT_FIELD_MAJOR>), grid, dim3(256), 0, ctx->stream, src, dst, n,
                           (int64_t)0, ctx->slab.ld, state_doubles(n, sl), state_doubles(n, dl));
    LAUNCH_OK(ctx);
    return 0;
}

// monitors of `y` -> ctx->rec[batch][NQ] (device)
static int launch_monitors(marl_ctx* ctx, const double* y, int layout, double* rec_out = nullptr)
{
    const int64_t n = ctx->slab.out_hi - ctx->slab.out_lo;
    int64_t nb = (n + 255) / 256;
    if (nb > 1024) nb = 1024;
    if (int rc = ensure_part(ctx, (size_t)(nb * ctx->batch))) return rc;
    const dim3 grid((unsigned)nb, (unsigned)ctx->batch);
    double* rec = rec_out ? rec_out : ctx->rec;
    double* first = nb == 1 ? rec : ctx->part;   // one workgroup per instance (N <= 256): its record IS the result - no second level
    if (layout == LAYOUT_TILED)
        hipLaunchKernelGGL(monitors_kernel<LAYOUT_TILED>, grid, dim3(256), 0, ctx->stream, y, ctx->dconsts, ctx->slab, inst_stride(ctx, layout), first);
    else
        hipLaunchKernelGGL(monitors_kernel<LAYOUT_FIELD_MAJOR>, grid, dim3(256), 0, ctx->stream, y, ctx->dconsts, ctx->slab, inst_stride(ctx, layout), first);
    LAUNCH_OK(ctx);
    if (nb == 1) return 0;
    hipLaunchKernelGGL(reduce_records_kernel, dim3((unsigned)ctx->batch), dim3(256), 0, ctx->stream, ctx->part, nb, rec);
    LAUNCH_OK(ctx);
    return 0;
}

static void record_to_events(const double* r, double* g)
{
    g[0] = r[1]; g[1] = r[2]; g[2] = r[3]; g[3] = r[5] - 1.0; g[4] = r[6] - 1.0; g[5] = r[4]; g[6] = r[7];
}

// ---- fused RK4: launch depths -------------------------------------------------------------------
// One shape ships: 256-thread blocks, one cell per thread (4 waves per SIMD), at 1 / 2 / 4 / 8 / 16 steps per launch - the default
// depth depends on the grid size, the shallower ones also serve as the remainder chain.  Option rk4_variant = index into this list.
// (Other block sizes are timed in tools/rk4_lab.hip only.)
static const int kRk4Depths[] = {1, 2, 4, 8, 16};
constexpr int kNumRk4Depths = sizeof(kRk4Depths) / sizeof(kRk4Depths[0]);

template <int NSTEPS, bool VD = false>
static void launch_rk4_t(marl_ctx* ctx, const double* yin, double* yout, int layout, double dt)
{
    constexpr int V = 256 - 8 * NSTEPS;
    const int64_t n = ctx->slab.out_hi - ctx->slab.out_lo;
    const dim3 grid((unsigned)((n + V - 1) / V));
    if (layout == LAYOUT_TILED)
        hipLaunchKernelGGL((rk4_fused_kernel<256, LAYOUT_TILED, NSTEPS, VD>), grid, dim3(256), 0, ctx->stream, yin, yout, ctx->dconsts, ctx->slab, dt);
    else
        hipLaunchKernelGGL((rk4_fused_kernel<256, LAYOUT_FIELD_MAJOR, NSTEPS, VD>), grid, dim3(256), 0, ctx->stream, yin, yout, ctx->dconsts, ctx->slab, dt);
}

// The kernels instantiated with the time-varying porosity diffusion coefficient (dPhi_variable): RK4 depths 4 (the default) and 1
// (the remainder) and the one RK45 set - the option is a model variant, not a tuning surface.
constexpr int kVdRk4Depth = 4;

extern "C" int marl_small_rk4_16(int tiled, unsigned grid, hipStream_t stream, const double* yin, double* yout, const void* consts, const int64_t slab5[5],
                                 double dt);   // marl_rk4_small.hip

// nsteps: steps fused in this launch - the run's own depth, or a smaller instantiated one for the remainder
static int launch_rk4(marl_ctx* ctx, int nsteps, const double* yin, double* yout, int layout, double dt)
{
    switch (nsteps) {
        case 1: if (ctx->var_dphi) launch_rk4_t<1, true>(ctx, yin, yout, layout, dt); else launch_rk4_t<1>(ctx, yin, yout, layout, dt); break;
        case 2: launch_rk4_t<2>(ctx, yin, yout, layout, dt); break;
        case 4: if (ctx->var_dphi) launch_rk4_t<4, true>(ctx, yin, yout, layout, dt); else launch_rk4_t<4>(ctx, yin, yout, layout, dt); break;
        case 8: launch_rk4_t<8>(ctx, yin, yout, layout, dt); break;
        case 16: {
            // grids whose workgroups fit the chip at TWO per CU (N <= 65 536 on 256 CUs: BASELINE configs[1]) take the build of this kernel
            // that trades occupancy for registers and ILP (marl_rk4_small.hip: 3.43 against 3.65 us per step at N = 65 536); with a third
            // workgroup per CU that build needs a second round (N = 98 304: 6.39 against 4.47 us) - those keep the four-waves-per-SIMD one
            const int64_t n = ctx->slab.out_hi - ctx->slab.out_lo, V = 256 - 8 * 16, tiles = (n + V - 1) / V;
            if (!ctx->cus) {
                hipDeviceProp_t prop;
                HIP_OK(ctx, hipGetDeviceProperties(&prop, ctx->device));
                ctx->cus = prop.multiProcessorCount;
            }
            if (ctx->rk4_small && tiles <= 2 * (int64_t)ctx->cus) {
                const int64_t slab5[5] = {ctx->slab.n_buf, ctx->slab.goff, ctx->slab.ld, ctx->slab.out_lo, ctx->slab.out_hi};
                const int e = marl_small_rk4_16(layout == LAYOUT_TILED, (unsigned)tiles, ctx->stream, yin, yout, ctx->dconsts, slab5, dt);
                if (e != 0) return fail(ctx, -100 - e, "kernel launch failed: %s", hipGetErrorString((hipError_t)e));
                return 0;
            }
            launch_rk4_t<16>(ctx, yin, yout, layout, dt);
            break;
        }
        default: return fail(ctx, -1, "rk4: %d steps per launch not instantiated", nsteps);
    }
    LAUNCH_OK(ctx);
    return 0;
}

// steps per launch of a run
static int default_rk4_depth(const marl_ctx* ctx)
{
    if (ctx->var_dphi) return kVdRk4Depth;
    if (ctx->rk4_variant >= 0 && ctx->rk4_variant < kNumRk4Depths) return kRk4Depths[ctx->rk4_variant];
    const int64_t n = ctx->slab.out_hi - ctx->slab.out_lo;
    // 256-thread blocks; the smaller the grid, the more the launch boundary matters against the recomputed halo:
    // 16 / 8 / 4 steps per launch (tools/variant_sweep.sh)
    return n <= 98304 ? 16 : (n <= 262144 ? 8 : 4);
}

#ifndef MARL_LAB_STREAM_BLK   // (kernel-lab switch: threads per workgroup of the streamed loop; 512 = half the halo share, twice the waves per barrier)
#define MARL_LAB_STREAM_BLK 256
#endif
// One dataflow launch for `levels` x `per` steps (rk4_stream_kernel): bufA -> ... -> (levels odd ? bufB : bufA)
template <int NSTEPS, bool VD = false>
static void launch_stream_t(marl_ctx* ctx, double* a, double* b, int layout, double dt, unsigned levels, unsigned tiles, unsigned blocks, double* c = nullptr)
{
    if (layout == LAYOUT_TILED)
        hipLaunchKernelGGL((rk4_stream_kernel<MARL_LAB_STREAM_BLK, LAYOUT_TILED, NSTEPS, VD>), dim3(blocks), dim3(MARL_LAB_STREAM_BLK), 0, ctx->stream, a, b, ctx->dconsts, ctx->slab, dt,
                           levels, tiles, ctx->sq, ctx->sq + 2, ctx->sq_sticky, ctx->sq_item_base, ctx->sq_level_base, c);
    else
        hipLaunchKernelGGL((rk4_stream_kernel<MARL_LAB_STREAM_BLK, LAYOUT_FIELD_MAJOR, NSTEPS, VD>), dim3(blocks), dim3(MARL_LAB_STREAM_BLK), 0, ctx->stream, a, b, ctx->dconsts, ctx->slab,
                           dt, levels, tiles, ctx->sq, ctx->sq + 2, ctx->sq_sticky, ctx->sq_item_base, ctx->sq_level_base, c);
}

// The chained decomposition of a level (rk4_chain_kernel): the grid's last tile of the unchained decomposition, [bound, n) with
// bound = V * floor((n - 1) / V), stays an item of its own; `chains` chains of K windows, V + (K - 1) W cells each, tile [0, bound), the
// last one clipped there and `nsub_last` windows long.  V, W and therefore every chain start and the bound are multiples of the halo
// H = 16, so no chain is narrower than H cells: the last tile's left halo ends inside the last chain, and an item's producers stay
// "t-1, t, t+1 of the level before".
struct ChainShape {
    int64_t items, bound;
    unsigned K, nsub_last;
};
static ChainShape chain_shape(int64_t n, int64_t K)
{
    constexpr int64_t H = 16, V = 256 - 2 * H, W = 256 - H;
    static_assert(V % H == 0 && W % H == 0, "a clipped chain could be narrower than the halo");
    const int64_t bound = V * ((n - 1) / V), L = V + W * (K - 1);
    const int64_t chains = (bound + L - 1) / L;
    int64_t nsub_last = 0;
    if (chains > 0) {
        const int64_t R = bound - (chains - 1) * L;   // cells of the last chain
        nsub_last = R <= V ? 1 : 1 + (R - V + W - 1) / W;
    }
    return {chains + 1, bound, (unsigned)K, (unsigned)nsub_last};
}

// Automatic chain length: the longest chain (at most 8 windows) that still leaves every resident workgroup TWO items per level.  With
// fewer the dataflow waits for its producers and loses far more than the shorter halo gains (profiles/r08_lab_rk4_chain.log section 1,
// 1024 resident workgroups: N = 2^20 gains 2.7 % at K = 2, 2.2 items per workgroup, and loses 4 % at K = 3, 1.46 items, and 20 % at
// K = 4, 1.09 items; N = 2^21 is best at K = 4, 2.17 items; N = 2^22 gains 5.6 % at K = 8, 2.15 items).  Grids under ~950 000 cells keep
// rk4_stream_kernel.
static int64_t rk4_chain_auto(int64_t n, int64_t resident)
{
    for (int64_t K = 8; K >= 2; K--)
        if (chain_shape(n, K).items >= 2 * resident) return K;
    return 1;
}

template <int LAYOUT>
static void launch_chain_t(marl_ctx* ctx, double* a, double* b, double dt, unsigned levels, const ChainShape& sh, unsigned blocks, double* c)
{
#define MARL_CHAIN_LAUNCH(KERNEL)                                                                                                                \
    hipLaunchKernelGGL(KERNEL, dim3(blocks), dim3(256), 0, ctx->stream, a, b, ctx->dconsts, ctx->slab, dt, levels, (unsigned)sh.items, ctx->sq, \
                       ctx->sq + 2, ctx->sq_sticky, ctx->sq_item_base, ctx->sq_level_base, c, sh.K, sh.nsub_last, sh.bound)
    switch (ctx->rk4_exchange) {
        case 0: MARL_CHAIN_LAUNCH((rk4_chain_kernel<256, LAYOUT, 4>)); break;
#ifdef MARL_LAB_XCH_PARTS
        case 1: MARL_CHAIN_LAUNCH((rk4_exchange_kernel<256, LAYOUT, 4, XCH_CELL>)); break;
        case 2: MARL_CHAIN_LAUNCH((rk4_exchange_kernel<256, LAYOUT, 4, XCH_PAIRS>)); break;
#endif
        default: MARL_CHAIN_LAUNCH((rk4_exchange_kernel<256, LAYOUT, 4>)); break;
    }
#undef MARL_CHAIN_LAUNCH
}

// *result: where the state is afterwards (a or b)
static int rk4_stream(marl_ctx* ctx, double* a, double* b, int layout, double dt, int per, int64_t levels, double** result)
{
    const int64_t n = ctx->slab.out_hi - ctx->slab.out_lo, V = MARL_LAB_STREAM_BLK - 8 * per;
    if (!ctx->cus) {
        hipDeviceProp_t prop;
        HIP_OK(ctx, hipGetDeviceProperties(&prop, ctx->device));
        ctx->cus = prop.multiProcessorCount;
    }
    // items of a level: the tiles of rk4_stream_kernel, or the chains of rk4_chain_kernel + the last tile (`tiles` is that number below)
    int64_t K = 1;
    if (per == 4 && !ctx->var_dphi && MARL_LAB_STREAM_BLK == 256 && ctx->rk4_chain > 0)
        K = ctx->rk4_chain == 1 ? rk4_chain_auto(n, 4 * (int64_t)ctx->cus) : ctx->rk4_chain;
    const ChainShape shape = chain_shape(n, K);
    const int64_t tiles = K >= 2 ? shape.items : (n + V - 1) / V;
    if (!ctx->sq_host) HIP_OK(ctx, hipHostMalloc((void**)&ctx->sq_host, sizeof(unsigned), hipHostMallocDefault));
    if (!ctx->sq_sticky) {
        HIP_OK(ctx, hipMalloc((void**)&ctx->sq_sticky, sizeof(unsigned)));
        HIP_OK(ctx, hipMemsetAsync(ctx->sq_sticky, 0, sizeof(unsigned), ctx->stream));
    }
    if (ctx->sq_cap < (size_t)tiles + 2 || ctx->sq_level_base > (1u << 30)) {   // (re)start the counters
        if (ctx->sq_cap < (size_t)tiles + 2) {
            if (ctx->sq) HIP_OK(ctx, hipFree(ctx->sq));
            ctx->sq = nullptr;
            ctx->sq_cap = 0;
            HIP_OK(ctx, hipMalloc((void**)&ctx->sq, ((size_t)tiles + 2) * sizeof(unsigned)));
            ctx->sq_cap = (size_t)tiles + 2;
        }
        HIP_OK(ctx, hipMemsetAsync(ctx->sq, 0, ctx->sq_cap * sizeof(unsigned), ctx->stream));
        ctx->sq_item_base = ctx->sq_level_base = 0;
    }
    if (ctx->sq_test_raise) {   // as if a workgroup of an earlier launch had given up: waiting workgroups leave, marl_synchronize reports
        HIP_OK(ctx, hipMemsetAsync(ctx->sq_sticky, 1, sizeof(unsigned), ctx->stream));
        ctx->sq_test_raise = false;
    }
    while (levels > 0) {
        // (the item counter is 32 bits wide; an even number of levels per launch keeps the ping-pong orientation)
        const int64_t cap = (ctx->sq_max_items / tiles) & ~(int64_t)1;
        const int64_t lv = std::min<int64_t>(levels, std::max<int64_t>(cap, 2));
        const unsigned blocks = (unsigned)std::min<int64_t>(lv * tiles, (4 * 256 / MARL_LAB_STREAM_BLK) * (int64_t)ctx->cus);   // 4 workgroups of 256 per CU are resident
        // the LAST launch with an odd number (>= 3) of levels goes A -> B, B <-> C, ... -> A through a third buffer: the result lands where
        // the caller's state is and the whole-state copy afterwards goes away (12 us of a 20-step call at N = 2^20; option rk4_stream_third)
        double* c = nullptr;
        if (ctx->rk4_stream_third && levels == lv && (lv & 1) && lv >= 3) {
            const size_t need = (size_t)state_doubles(ctx->slab.n_buf, layout);
            if (ctx->stream_c_cap < need) {
                if (ctx->stream_c) HIP_OK(ctx, hipFree(ctx->stream_c));
                ctx->stream_c = nullptr; ctx->stream_c_cap = 0;
                HIP_OK(ctx, hipMalloc((void**)&ctx->stream_c, need * sizeof(double)));
                ctx->stream_c_cap = need;
            }
            c = ctx->stream_c;
        }
        if (K >= 2) {
            if (layout == LAYOUT_TILED) launch_chain_t<LAYOUT_TILED>(ctx, a, b, dt, (unsigned)lv, shape, blocks, c);
            else launch_chain_t<LAYOUT_FIELD_MAJOR>(ctx, a, b, dt, (unsigned)lv, shape, blocks, c);
        } else switch (per) {
            case 1: if (ctx->var_dphi) launch_stream_t<1, true>(ctx, a, b, layout, dt, (unsigned)lv, (unsigned)tiles, blocks, c);
                    else launch_stream_t<1>(ctx, a, b, layout, dt, (unsigned)lv, (unsigned)tiles, blocks, c);
                    break;
            case 2: launch_stream_t<2>(ctx, a, b, layout, dt, (unsigned)lv, (unsigned)tiles, blocks, c); break;
            case 4: if (ctx->var_dphi) launch_stream_t<4, true>(ctx, a, b, layout, dt, (unsigned)lv, (unsigned)tiles, blocks, c);
                    else launch_stream_t<4>(ctx, a, b, layout, dt, (unsigned)lv, (unsigned)tiles, blocks, c);
                    break;
            case 8: launch_stream_t<8>(ctx, a, b, layout, dt, (unsigned)lv, (unsigned)tiles, blocks, c); break;
            case 16: launch_stream_t<16>(ctx, a, b, layout, dt, (unsigned)lv, (unsigned)tiles, blocks, c); break;
            default: return fail(ctx, -1, "rk4 stream: %d steps per level not instantiated", per);
        }
        LAUNCH_OK(ctx);
        ctx->sq_pending = true;
        ctx->sq_item_base += (unsigned)(lv * tiles) + blocks;   // its items + one failing grab per workgroup (wraps with the counter)
        ctx->sq_level_base += (unsigned)lv;
        levels -= lv;
        if ((lv & 1) && !c) std::swap(a, b);   // (now `a` holds the state)
    }
    *result = a;
    return 0;
}

constexpr int64_t kStreamMinCells = 196608;

// y (device, `layout`) advanced in place; `tmp` is a second buffer of the same size
static int rk4_run(marl_ctx* ctx, double* y, double* tmp, int layout, double dt, int64_t nsteps)
{
    const int per = default_rk4_depth(ctx);
    double* a = y;
    double* b = tmp;
    int64_t left = nsteps;
    // One dataflow launch instead of one launch per level where it pays (tools/lab record in profiles/r02_lab_rk4_stream.log):
    // from ~200 000 cells (below, the tiles do not fill the resident workgroups and the state is served from the L2s anyway).
    const bool stream = ctx->rk4_stream == 2 ? left >= per
                                             : (ctx->rk4_stream == 1 && ctx->slab.out_hi - ctx->slab.out_lo >= kStreamMinCells && left >= 2 * per);
    if (stream && ctx->halo == 0) {
        const int64_t levels = left / per;
        double* now = nullptr;
        if (int rc = rk4_stream(ctx, a, b, layout, dt, per, levels, &now)) return rc;
        if (now != a) std::swap(a, b);
        left -= levels * per;
    }
    while (left >= per) {
        if (int rc = launch_rk4(ctx, per, a, b, layout, dt)) return rc;
        std::swap(a, b);
        left -= per;
    }
    // remainder: every power of two below the depth is instantiated (the dPhi_variable set: depths 4 and 1 only)
    const bool family = !ctx->var_dphi;
    for (int chunk = per / 2; chunk >= 1 && left > 0; chunk /= 2) {
        const int c = family ? chunk : 1;
        while (left >= c) {
            if (int rc = launch_rk4(ctx, c, a, b, layout, dt)) return rc;
            std::swap(a, b);
            left -= c;
            if (family) break;   // at most one launch per power of two
        }
    }
    if (a != y) HIP_OK(ctx, hipMemcpyAsync(y, a, sizeof(double) * state_doubles(ctx->slab.n_buf, layout), hipMemcpyDeviceToDevice, ctx->stream));
    return 0;
}

// ---- one-workgroup sweeps: window sizes ---------------------------------------------------------
// one cell per thread; the smallest window that holds the grid is taken (option sweep_variant = index of another one that holds it)
static const int kSweepBlocks[] = {256, 512, 1024};
constexpr int kNumSweepBlocks = sizeof(kSweepBlocks) / sizeof(kSweepBlocks[0]);

// threads (= cells) of the sweep window of this grid; 0: the grid does not fit one workgroup
static int sweep_block(const marl_ctx* ctx)
{
    if (ctx->sweep_variant >= 0 && ctx->sweep_variant < kNumSweepBlocks && (int64_t)kSweepBlocks[ctx->sweep_variant] >= ctx->N)
        return kSweepBlocks[ctx->sweep_variant];
    for (int i = 0; i < kNumSweepBlocks; i++)
        if ((int64_t)kSweepBlocks[i] >= ctx->N) return kSweepBlocks[i];
    return 0;
}

// (switches on `blk`, a sweep_block() of the caller)
#define SWEEP_DISPATCH(KERNEL, ...)                                                                           \
    switch (blk) {                                                                                            \
        case 256: if (ctx->var_dphi) hipLaunchKernelGGL((KERNEL<256, true>), grid, dim3(256), 0, ctx->stream, __VA_ARGS__); \
                else hipLaunchKernelGGL((KERNEL<256>), grid, dim3(256), 0, ctx->stream, __VA_ARGS__); break;       \
        case 512: if (ctx->var_dphi) hipLaunchKernelGGL((KERNEL<512, true>), grid, dim3(512), 0, ctx->stream, __VA_ARGS__); \
                else hipLaunchKernelGGL((KERNEL<512>), grid, dim3(512), 0, ctx->stream, __VA_ARGS__); break;       \
        case 1024: if (ctx->var_dphi) hipLaunchKernelGGL((KERNEL<1024, true>), grid, dim3(1024), 0, ctx->stream, __VA_ARGS__); \
                else hipLaunchKernelGGL((KERNEL<1024>), grid, dim3(1024), 0, ctx->stream, __VA_ARGS__); break;     \
        default: return fail(ctx, -1, "sweep: no %d-thread window", blk);                                     \
    }

// ---- fused RK45 --------------------------------------------------------------------------------
// One shape: 256-thread windows that write 256 - 2 * 6 cells (option rk45_variant is accepted and ignored: only 0 ever existed).
static int64_t rk_blocks(const marl_ctx* ctx, int written)
{
    const int64_t n = ctx->slab.out_hi - ctx->slab.out_lo;
    return (n + written - 1) / written;
}
static int64_t rk45_blocks(const marl_ctx* ctx) { return rk_blocks(ctx, 256 - 12); }

// ---- the explicit adaptive methods behind one set of host drivers (rk_run, sweep_rk) --------------------------------------------
// RK45: the kernels of marl_kernels.h, launched here.  RK23: those of marl_rk23.h, a translation unit of its own (marl_rk23.hip),
// reached through its launchers.  What differs between the two on the host is in this table and nowhere else.
enum : int { SWEEP_PLAIN = 0, SWEEP_EVENTS = 1, SWEEP_EVAL = 2, SWEEP_ROOTS = 3, SWEEP_TERM = 4 };   // the five one-workgroup kernels of a method
struct SweepLaunch {
    double *Y, *Yold, *Fold;
    const double* t_eval; int64_t n_eval; double* Yeval; int64_t* n_done;
    double* t_events; int64_t max_events;
    const int64_t* terminal;   // SWEEP_TERM: the seven limits (host); else NULL
};
struct RkMethod {
    const char* name;        // in front of error messages: "rk45", "rk23"
    const char* sweep_entry; // the entry named when a grid does not fit one workgroup
    int written;             // cells a 256-thread window of the attempt kernel writes: 256 - 2 * (evaluations after K1)
    bool can_stream;         // has a persistent device-wide-barrier loop (rk45_stream_kernel)
    int (*sweep)(marl_ctx*, int kind, int blk, unsigned batch, const SweepLaunch&);
    int (*attempt)(marl_ctx*, int64_t nb, int layout);
    int (*control)(marl_ctx*, const double* recs, int64_t nrec);
    int (*dense)(marl_ctx*, int64_t nb, int layout, const double* yold, const double* fold, double h, const DenseWeights& dw, double* yout);
    void (*weights)(double x, DenseWeights* dw);   // w_j(x) of the dense output
    // A method whose attempt is not "K1 in a buffer, the rest in one launch" (DOP853 on large grids: 16 stage derivatives in an arena,
    // 16 dense-output weights) replaces three steps of rk_run; NULL in the rows of RK45 and RK23, which run exactly as they did.
    const char* entry;       // the name behind "marl_integrate_" in messages, where it is not `name`
    bool grid_only;          // marl_integrate_<entry> takes the large-grid loop at every N (no one-workgroup sweep)
    int64_t (*part_records)(int64_t nb);   // records of ctx->part for nb windows, laid out by the method: `control` then reduces all of it
    int (*first_k)(marl_ctx*, int layout);   // K1 = f(t0, y0) of the state in buf[0], behind rk45_init_kernel; in place of launch_rhs into buf[2]
    // the dense output of the last accepted step at time t: the state into yout (may be NULL), one monitors record per workgroup into
    // ctx->part when want_part; *nb: how many.  In place of weights + dense.
    int (*dense_at)(marl_ctx*, int layout, const Rk45Ctrl& c, double t, double* yout, bool want_part, int64_t* nb);
};

constexpr int64_t kReduceGroups = 64;
template <bool VD = false>
static void launch_attempt_t(marl_ctx* ctx, int64_t nb, int layout)
{
    if (layout == LAYOUT_TILED)
        hipLaunchKernelGGL((rk45_attempt_kernel<256, LAYOUT_TILED, VD>), dim3((unsigned)nb), dim3(256), 0, ctx->stream, ctx->buf[0], ctx->buf[1],
                           ctx->buf[2], ctx->buf[3], ctx->dconsts, ctx->slab, ctx->dctrl, ctx->part);
    else
        hipLaunchKernelGGL((rk45_attempt_kernel<256, LAYOUT_FIELD_MAJOR, VD>), dim3((unsigned)nb), dim3(256), 0, ctx->stream, ctx->buf[0],
                           ctx->buf[1], ctx->buf[2], ctx->buf[3], ctx->dconsts, ctx->slab, ctx->dctrl, ctx->part);
}

// Records of a large grid are reduced in two levels: `*nrec` per-workgroup records at ctx->part -> at most kReduceGroups
// records behind them (same buffer, offset `*nrec`); returns where the second level reads and updates *nrec.
static const double* reduce_first_level(marl_ctx* ctx, int64_t* nrec)
{
    const int64_t nb = *nrec;
    if (nb <= 4 * kReduceGroups) return ctx->part;
    const int64_t chunk = (nb + kReduceGroups - 1) / kReduceGroups, groups = (nb + chunk - 1) / chunk;
    double* out = ctx->part + nb * NQ;
    hipLaunchKernelGGL(reduce_chunks_kernel, dim3((unsigned)groups), dim3(256), 0, ctx->stream, ctx->part, nb, chunk, out);
    *nrec = groups;
    return out;
}

static int launch_attempt(marl_ctx* ctx, int layout, const RkMethod& m)
{
    const int64_t nb = rk_blocks(ctx, m.written);
    if (int rc = m.attempt(ctx, nb, layout)) return rc;
    if (m.part_records) return m.control(ctx, ctx->part, nb);   // (a record buffer of the method's own layout: its control reduces it)
    int64_t nrec = nb;
    const double* recs = reduce_first_level(ctx, &nrec);
    LAUNCH_OK(ctx);
    return m.control(ctx, recs, nrec);
}

// ---- the adaptive loop of one grid as ONE launch per batch of attempts (rk45_stream_kernel) ----------------------------------
// barrier words zeroed, the grid-wide extrema armed (+inf); synchronises
static int rk45_stream_reset(marl_ctx* ctx)
{
    std::vector<double> inf((size_t)GREC_DOUBLES - MON_OFFSET, (double)INFINITY);
    HIP_OK(ctx, hipMemsetAsync(ctx->rs, 0, sizeof(Rk45Stream), ctx->stream));
    HIP_OK(ctx, hipMemsetAsync(ctx->rs_grec, 0, sizeof(double) * MON_OFFSET, ctx->stream));
    HIP_OK(ctx, hipMemcpyAsync(ctx->rs_grec + MON_OFFSET, inf.data(), inf.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->rs_arrive_base = ctx->rs_epoch_base = ctx->rs_grab_base = 0;
    return 0;
}

static int rk45_stream_setup(marl_ctx* ctx)
{
    if (!ctx->cus) {
        hipDeviceProp_t prop;
        HIP_OK(ctx, hipGetDeviceProperties(&prop, ctx->device));
        ctx->cus = prop.multiProcessorCount;
    }
    if (!ctx->rs) {
        HIP_OK(ctx, hipMalloc((void**)&ctx->rs, sizeof(Rk45Stream)));
        HIP_OK(ctx, hipMalloc((void**)&ctx->rs_grec, sizeof(double) * GREC_DOUBLES));
        HIP_OK(ctx, hipHostMalloc((void**)&ctx->rs_host, 2 * sizeof(unsigned), hipHostMallocDefault));
        if (int rc = rk45_stream_reset(ctx)) return rc;
    }
    if (ctx->rs_arrive_base > (1u << 30) || ctx->rs_epoch_base > (1u << 30) || ctx->rs_grab_base > (1u << 30))   // (the stream is idle between batches: the caller has synchronised)
        if (int rc = rk45_stream_reset(ctx)) return rc;
    return 0;
}

// dd: one attempt of a slab; the last workgroup packs the rank's message into ctx->dd_send and re-arms the counters (bases 0)
template <bool VD>
static int launch_rk45_stream_t(marl_ctx* ctx, int layout, int64_t tiles, int64_t max_attempts, bool dd = false)
{
    if (dd && layout != LAYOUT_FIELD_MAJOR) return fail(ctx, -1, "rk45 stream: slabs are field-major");
    auto kern = dd ? rk45_stream_kernel<256, LAYOUT_FIELD_MAJOR, VD, true>
                   : (layout == LAYOUT_TILED ? rk45_stream_kernel<256, LAYOUT_TILED, VD, false> : rk45_stream_kernel<256, LAYOUT_FIELD_MAJOR, VD, false>);
    int& occ = ctx->rs_occ[dd ? 2 : (layout == LAYOUT_TILED ? 1 : 0)][VD ? 1 : 0];   // (per instantiation: the resident-grid bound below rests on it)
    if (!occ) {
        HIP_OK(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kern, 256, 0));
        if (occ < 1) return fail(ctx, -3, "rk45 stream: the kernel does not fit a compute unit");
        if (occ > 16) occ = 16;
    }
    // every workgroup of the grid must be resident at once (they meet at a barrier in memory): at most what the device holds
    ctx->rs_G = (unsigned)std::min<int64_t>(std::min<int64_t>(tiles, (int64_t)occ * ctx->cus), MON_OFFSET);
    hipLaunchKernelGGL(kern, dim3(ctx->rs_G), dim3(256), 0, ctx->stream, ctx->buf[0], ctx->buf[1], ctx->buf[2], ctx->buf[3], ctx->dconsts, ctx->slab,
                       ctx->dctrl, ctx->rs_grec, ctx->rs, (unsigned)tiles, dd ? 0u : ctx->rs_arrive_base, dd ? 0u : ctx->rs_epoch_base, dd ? 0u : ctx->rs_grab_base,
                       dd ? 1u : (unsigned)max_attempts, dd ? ctx->dd_send : (double*)nullptr, dd ? ctx->halo : 0);
    const unsigned R = (unsigned)(tiles % ctx->rs_G);
    ctx->rs_grabs_per_attempt = R ? R + ctx->rs_G : 0;   // (what the kernel's workgroups take from the remainder counter per attempt)
    LAUNCH_OK(ctx);
    return 0;
}

// Where the persistent loop pays (profiles/r04_lab_rk45_stream.log; MI355X, 1024 resident workgroups): what it removes is the fixed
// cost per attempt - two small launches and every workgroup's prologue, ~8 us against a ~5 us barrier - and what it loses is the
// dispatcher's balancing: its workgroups own STATIC tiles, the SIMDs arbitrate oldest-first, so a CU's four workgroups finish
// one after the other and the last runs alone.  N = 65 536: +35 %, 2^19: +7 %, 2^20: -1 %, 2^22: -10 %.  Default: grids of up to
// three rounds of resident workgroups (N <= ~750 000 cells on 256 CUs); larger grids keep one launch per attempt.
constexpr int64_t kRk45StreamRounds = 3;
static bool rk45_use_stream(marl_ctx* ctx)
{
    if (ctx->rk45_stream == 0) return false;
    if (ctx->rk45_stream >= 2) return true;
    if (!ctx->cus) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, ctx->device) != hipSuccess) return false;
        ctx->cus = prop.multiProcessorCount;
    }
    return rk45_blocks(ctx) <= kRk45StreamRounds * 4 * (int64_t)ctx->cus;
}

static int launch_rk45_stream(marl_ctx* ctx, int layout, int64_t max_attempts, bool dd = false)
{
    if (int rc = rk45_stream_setup(ctx)) return rc;
    const int64_t tiles = rk45_blocks(ctx);
    if (tiles >= (1ll << 31)) return fail(ctx, -1, "rk45 stream: grid too large");
    return ctx->var_dphi ? launch_rk45_stream_t<true>(ctx, layout, tiles, max_attempts, dd) : launch_rk45_stream_t<false>(ctx, layout, tiles, max_attempts, dd);
}

// after the batch's status read-back (stream idle): where the ticket / barrier counters stand now, and the sticky flag
static int rk45_stream_account(marl_ctx* ctx, int64_t attempts_in_batch)
{
    HIP_OK(ctx, hipMemcpyAsync(ctx->rs_host, ctx->rs, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
    const bool consistent = ctx->rs_host[0] - ctx->rs_arrive_base == ctx->rs_G * (unsigned)attempts_in_batch;
    if (ctx->rs_host[1] || !consistent) {
        const unsigned took = ctx->rs_host[0] - ctx->rs_arrive_base;
        if (int rc = rk45_stream_reset(ctx)) return rc;
        if (ctx->rs_host[1]) return fail(ctx, -2, "rk45: the persistent time loop gave up waiting at its barrier (rk45_stream_kernel); the state is invalid");
        return fail(ctx, -2, "rk45: the persistent time loop took %u tickets for %lld attempts of %u workgroups", took, (long long)attempts_in_batch, ctx->rs_G);
    }
    ctx->rs_arrive_base += ctx->rs_G * (unsigned)attempts_in_batch;
    ctx->rs_epoch_base += (unsigned)attempts_in_batch;
    ctx->rs_grab_base += ctx->rs_grabs_per_attempt * (unsigned)attempts_in_batch;
    return 0;
}

template <bool VD = false>
static void launch_dense_t(marl_ctx* ctx, int64_t nb, int layout, const double* yold, const double* fold, double h,
                           const DenseWeights& dw, double* yout)
{
    if (layout == LAYOUT_TILED)
        hipLaunchKernelGGL((rk45_dense_kernel<256, LAYOUT_TILED, VD>), dim3((unsigned)nb), dim3(256), 0, ctx->stream, yold, fold, ctx->dconsts,
                           ctx->slab, h, dw, yout, ctx->part);
    else
        hipLaunchKernelGGL((rk45_dense_kernel<256, LAYOUT_FIELD_MAJOR, VD>), dim3((unsigned)nb), dim3(256), 0, ctx->stream, yold, fold,
                           ctx->dconsts, ctx->slab, h, dw, yout, ctx->part);
}

// Dense output P (dp::P, marl_kernels.h): w_j(x) = sum_m P[j][m] x^(m+1)
static constexpr auto& kDpP = dp::P;

// ---- the method table's two rows ------------------------------------------------------------------------------------------------
static int rk45_m_sweep(marl_ctx* ctx, int kind, int blk, unsigned batch, const SweepLaunch& a)
{
    const dim3 grid(batch);
    switch (kind) {
        case SWEEP_PLAIN: SWEEP_DISPATCH(rk45_sweep_kernel, a.Y, ctx->dconsts, ctx->dctrl, ctx->N, a.Yold, a.Fold) break;
        case SWEEP_EVENTS: SWEEP_DISPATCH(rk45_sweep_events_kernel, a.Y, ctx->dconsts, ctx->dctrl, ctx->N, a.Yold, a.Fold) break;
        case SWEEP_EVAL: SWEEP_DISPATCH(rk45_sweep_eval_kernel, a.Y, ctx->dconsts, ctx->dctrl, ctx->N, a.t_eval, a.n_eval, a.Yeval, a.n_done) break;
        case SWEEP_ROOTS: SWEEP_DISPATCH(rk45_sweep_roots_kernel, a.Y, ctx->dconsts, ctx->dctrl, ctx->N, a.t_eval, a.n_eval, a.Yeval, a.n_done, a.t_events,
                                         a.max_events) break;
        default: {
            TermLimits lim = {};
            for (int e = 0; e < 7; e++) lim.k[e] = a.terminal[e];
            SWEEP_DISPATCH(rk45_sweep_term_kernel, a.Y, ctx->dconsts, ctx->dctrl, ctx->N, a.t_eval, a.n_eval, a.Yeval, a.n_done, a.t_events,
                           a.max_events, lim) break;
        }
    }
    LAUNCH_OK(ctx);
    return 0;
}
static int rk45_m_attempt(marl_ctx* ctx, int64_t nb, int layout)
{
    if (ctx->var_dphi) launch_attempt_t<true>(ctx, nb, layout); else launch_attempt_t<>(ctx, nb, layout);
    LAUNCH_OK(ctx);
    return 0;
}
static int rk45_m_control(marl_ctx* ctx, const double* recs, int64_t nrec)
{
    hipLaunchKernelGGL(rk45_control_kernel, dim3(1), dim3(CONTROL_THREADS), 0, ctx->stream, recs, nrec, ctx->dctrl);
    LAUNCH_OK(ctx);
    return 0;
}
static int rk45_m_dense(marl_ctx* ctx, int64_t nb, int layout, const double* yold, const double* fold, double h, const DenseWeights& dw, double* yout)
{
    if (ctx->var_dphi) launch_dense_t<true>(ctx, nb, layout, yold, fold, h, dw, yout); else launch_dense_t<>(ctx, nb, layout, yold, fold, h, dw, yout);
    LAUNCH_OK(ctx);
    return 0;
}
static void rk45_m_weights(double x, DenseWeights* dw)
{
    double pw[4] = {x, x * x, x * x * x, x * x * x * x};
    for (int j = 0; j < 7; j++) {
        double a = 0;
        for (int m = 0; m < 4; m++) a += kDpP[j][m] * pw[m];
        dw->w[j] = a;
    }
}
static const RkMethod kRk45 = {"rk45", "marl_sweep_rk45_dev", 256 - 2 * 6, true, rk45_m_sweep, rk45_m_attempt, rk45_m_control, rk45_m_dense, rk45_m_weights};

// marl_rk23.hip
extern "C" {
int marl_rk23_launch_sweep(int kind, int blk, int vd, unsigned grid, hipStream_t stream, double* Y, const void* consts, void* ctrls, int64_t N,
                           double* Yold, double* Fold, const double* t_eval, int64_t n_eval, double* Yeval, int64_t* n_done, double* t_events,
                           int64_t max_events, const int64_t* terminal);
int marl_rk23_launch_attempt(int tiled, int vd, unsigned nb, hipStream_t stream, double* Y0, double* Y1, double* F0, double* F1, const void* consts,
                             const int64_t slab5[5], const void* ctrl, double* part);
int marl_rk23_launch_control(hipStream_t stream, const double* recs, int64_t nrec, void* ctrl);
int marl_rk23_launch_dense(int tiled, int vd, unsigned nb, hipStream_t stream, const double* yold, const double* fold, const void* consts,
                           const int64_t slab5[5], double h, const double w[7], double* yout, double* part);
}
static int rk23_launched(marl_ctx* ctx, int err)
{
    if (err != (int)hipSuccess) return fail(ctx, -3, "rk23: kernel launch failed: %s", hipGetErrorString((hipError_t)err));
    return 0;
}
static int rk23_m_sweep(marl_ctx* ctx, int kind, int blk, unsigned batch, const SweepLaunch& a)
{
    return rk23_launched(ctx, marl_rk23_launch_sweep(kind, blk, ctx->var_dphi ? 1 : 0, batch, ctx->stream, a.Y, ctx->dconsts, ctx->dctrl, ctx->N, a.Yold,
                                                     a.Fold, a.t_eval, a.n_eval, a.Yeval, a.n_done, a.t_events, a.max_events,
                                                     kind == SWEEP_TERM ? a.terminal : nullptr));
}
static int rk23_m_attempt(marl_ctx* ctx, int64_t nb, int layout)
{
    const Slab& S = ctx->slab;
    const int64_t slab5[5] = {S.n_buf, S.goff, S.ld, S.out_lo, S.out_hi};
    return rk23_launched(ctx, marl_rk23_launch_attempt(layout == LAYOUT_TILED, ctx->var_dphi ? 1 : 0, (unsigned)nb, ctx->stream, ctx->buf[0], ctx->buf[1],
                                                       ctx->buf[2], ctx->buf[3], ctx->dconsts, slab5, ctx->dctrl, ctx->part));
}
static int rk23_m_control(marl_ctx* ctx, const double* recs, int64_t nrec)
{
    return rk23_launched(ctx, marl_rk23_launch_control(ctx->stream, recs, nrec, ctx->dctrl));
}
static int rk23_m_dense(marl_ctx* ctx, int64_t nb, int layout, const double* yold, const double* fold, double h, const DenseWeights& dw, double* yout)
{
    const Slab& S = ctx->slab;
    const int64_t slab5[5] = {S.n_buf, S.goff, S.ld, S.out_lo, S.out_hi};
    return rk23_launched(ctx, marl_rk23_launch_dense(layout == LAYOUT_TILED, ctx->var_dphi ? 1 : 0, (unsigned)nb, ctx->stream, yold, fold, ctx->dconsts,
                                                     slab5, h, dw.w, yout, ctx->part));
}
static void rk23_m_weights(double x, DenseWeights* dw)
{
    double w[4];
    rk23_dense_weights(x, w);
    for (int j = 0; j < 7; j++) dw->w[j] = j < 4 ? w[j] : 0.0;
}
// (large grids always go launch-per-attempt: three evaluations after K1, so a window writes 256 - 2 * 3 = 250 cells)
static const RkMethod kRk23 = {"rk23", "marl_sweep_rk23_dev", 256 - 2 * 3, false, rk23_m_sweep, rk23_m_attempt, rk23_m_control, rk23_m_dense, rk23_m_weights};

// Evaluate the dense output of the LAST accepted step at time t: state into yout (may be NULL) and the
// seven monitors into g (may be NULL; synchronises when given).
static int dense_eval(marl_ctx* ctx, const RkMethod& m, int layout, bool small, const Rk45Ctrl& c, double t, double* yout, double* g)
{
    int64_t nb = rk_blocks(ctx, m.written);
    if (m.dense_at) {
        if (int rc = m.dense_at(ctx, layout, c, t, yout, g != nullptr, &nb)) return rc;
    } else {
        DenseWeights dw;
        m.weights((t - c.t_old) / c.h_prev, &dw);
        const double* yold = small ? ctx->buf[1] : ctx->buf[c.cur ^ 1];
        const double* fold = small ? ctx->buf[3] : ctx->buf[2 + (c.cur ^ 1)];
        if (int rc = m.dense(ctx, nb, layout, yold, fold, c.h_prev, dw, yout)) return rc;
    }
    if (g) {
        hipLaunchKernelGGL(reduce_records_kernel, dim3(1), dim3(256), 0, ctx->stream, ctx->part, nb, ctx->rec);
        LAUNCH_OK(ctx);
        HIP_OK(ctx, hipMemcpyAsync(ctx->hrec, ctx->rec, sizeof(double) * NQ, hipMemcpyDeviceToHost, ctx->stream));
        HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
        record_to_events(ctx->hrec, g);
    }
    return 0;
}

static void ctrl_to_stats(const Rk45Ctrl& c, marl_stats* st)
{
    memset(st, 0, sizeof *st);
    st->nfev = c.nfev;
    st->n_accepted = c.n_acc;
    st->n_rejected = c.n_rej;
    st->status = c.status == ST_TERMINAL ? 1 : c.status;   // scipy's "A termination event occurred."
    st->t = c.t;
    st->h_next = c.h_abs;
    for (int e = 0; e < 7; e++) { st->event_value[e] = c.g[e]; st->n_events[e] = c.n_events[e]; }
}

// Attempts to enqueue before the next status read: `poll`, but never more than an attempt budget has left - once the
// controller has stopped, every further attempt / reduce / control launch of the batch is a dispatch that does nothing
// (cheap, but it is time, and it dilutes per-launch profile averages).  Pauses for t_eval samples and events still cut a
// batch short; those are rare.
static int64_t attempts_per_batch(int64_t poll, int64_t max_attempts, int64_t executed)
{
    if (max_attempts <= 0) return poll;
    const int64_t left = max_attempts - executed;
    return left < 1 ? 1 : (left < poll ? left : poll);
}

// What every single run checks of its span, first step, tolerances and sample times before it starts; `name`: the solver, in front
// of the message.
static int check_ivp_args(marl_ctx* ctx, const char* name, double t0, double t1, double first_step, double rtol, double atol,
                          const double* t_eval, int64_t n_eval)
{
    if (!(first_step > 0) || !(t1 >= t0)) return fail(ctx, -1, "%s: need first_step > 0 and t1 >= t0 (forward integration)", name);
    if (t1 > t0 && first_step > t1 - t0) return fail(ctx, -1, "%s: `first_step` exceeds bounds", name);  // common.py:10-16
    if (!(rtol > 0) || !(atol >= 0)) return fail(ctx, -1, "%s: tolerances must be positive", name);
    for (int64_t i = 0; i < n_eval; i++)
        if (t_eval[i] < t0 || t_eval[i] > t1 || (i > 0 && t_eval[i] <= t_eval[i - 1]))
            return fail(ctx, -1, "%s: `t_eval` must be sorted and within t_span", name);  // ivp.py:603-609
    return 0;
}

// The adaptive loop on device buffers buf[0..3] (`layout`), state already in buf[0].
// small = true: the grid fits one workgroup -> the persistent sweep kernel runs all attempts on-chip
// (state in buf[0], FIELD-MAJOR; (y_old, f_old) of a paused step in buf[1], buf[3]).
// Terminal monitors (ctx->terminal; only marl_integrate_rk45_terminal / rk23_terminal arrive here with limits): the loop pauses on every
// sign change also without t_events; at such a pause rk_terminal_step (marl_rk_terminal.h, the rule the sweep kernels apply) says which
// of the step's sign changes happened - when a limit is met, after the roots of ALL of them are located - and where the run ends: the
// samples up to t_stop, then the step's dense output at t_stop as the state (the launch that writes a sample), status 1.
static int rk_run(const RkMethod& m, marl_ctx* ctx, int layout, bool small, double t0, double t1, double first_step, double rtol, double atol,
                    const double* t_eval, int64_t n_eval, double* y_eval_dev, double* t_events, int64_t max_events,
                    int64_t max_attempts, marl_stats* stats)
{
    if (int rc = check_ivp_args(ctx, m.name, t0, t1, first_step, rtol, atol, t_eval, n_eval)) return rc;
    rtol = clamp_rtol(rtol);
    const int blk = small ? sweep_block(ctx) : 0;
    const int64_t nb = rk_blocks(ctx, m.written);
    if (int rc = ensure_part(ctx, (size_t)std::max<int64_t>(m.part_records ? m.part_records(nb) : nb + kReduceGroups, 1024))) return rc;
    const int64_t sd = state_doubles(ctx->slab.n_buf, layout);
    // f(t0, y0) and the monitors at t0
    if (!small && !m.first_k)
        if (int rc = launch_rhs(ctx, ctx->buf[0], ctx->buf[2], layout)) return rc;
    if (int rc = launch_monitors(ctx, ctx->buf[0], layout)) return rc;
    hipLaunchKernelGGL(rk45_init_kernel, dim3(1), dim3(1), 0, ctx->stream, ctx->dctrl, ctx->rec, t0, t1, first_step, rtol, atol,
                       (int64_t)NF * ctx->N, max_attempts, 0);
    LAUNCH_OK(ctx);
    if (!small && m.first_k)
        if (int rc = m.first_k(ctx, layout)) return rc;
    int64_t eval_i = 0;
    // t_eval == t0 is emitted on the first step by scipy (dense output at x = 0 == y_old)
    const bool events_on = t_events != nullptr && max_events > 0, term = has_terminal(ctx);
    auto next_pause = [&]() { return eval_i < n_eval ? t_eval[eval_i] : (double)INFINITY; };
    hipLaunchKernelGGL(rk45_resume_kernel, dim3(1), dim3(1), 0, ctx->stream, ctx->dctrl, next_pause(), max_attempts);
    LAUNCH_OK(ctx);
    if (events_on || term) {
        // pause_on_event is a plain field: set it through a tiny host round trip once
        HIP_OK(ctx, hipMemcpyAsync(ctx->hctrl, ctx->dctrl, sizeof(Rk45Ctrl), hipMemcpyDeviceToHost, ctx->stream));
        HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
        ctx->hctrl->pause_on_event = 1;
        HIP_OK(ctx, hipMemcpyAsync(ctx->dctrl, ctx->hctrl, sizeof(Rk45Ctrl), hipMemcpyHostToDevice, ctx->stream));
    }
    int64_t seen_events[7] = {0, 0, 0, 0, 0, 0, 0};
    Rk45Ctrl& hc = *ctx->hctrl;
    int64_t executed = 0;   // attempts the device has finished, as of the last status read
    const bool streamed = !small && m.can_stream && rk45_use_stream(ctx);   // one launch per batch of attempts (rk45_stream_kernel)
    while (true) {
        if (small) {
            // events: pauses on monitor sign changes (root finding) - the loop shape that decides with this step's events
            const SweepLaunch a = {ctx->buf[0], ctx->buf[1], ctx->buf[3], nullptr, 0, nullptr, nullptr, nullptr, 0};
            if (int rc = m.sweep(ctx, (events_on || term) ? SWEEP_EVENTS : SWEEP_PLAIN, blk, 1, a)) return rc;
        } else if (streamed) {
            if (int rc = launch_rk45_stream(ctx, layout, ctx->rk45_stream_attempts)) return rc;
        } else {
            const int64_t batch = attempts_per_batch(ctx->poll, max_attempts, executed);
            for (int64_t i = 0; i < batch; i++)
                if (int rc = launch_attempt(ctx, layout, m)) return rc;
        }
        HIP_OK(ctx, hipMemcpyAsync(ctx->hctrl, ctx->dctrl, sizeof(Rk45Ctrl), hipMemcpyDeviceToHost, ctx->stream));
        HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
        const int64_t executed_before = executed;
        executed = hc.attempts - (hc.status == ST_RUNNING ? 1 : 0);   // (a running controller has already prepared the next one)
        if (streamed)
            if (int rc = rk45_stream_account(ctx, executed - executed_before)) return rc;
        if (hc.status == ST_RUNNING) continue;
        const bool stepped = hc.n_acc > 0;
        // event roots inside the last accepted step (ivp.py:673-694)
        double t_stop = INFINITY;   // < +inf: a terminal monitor ends the run inside this step (ivp.py:696-704)
        if ((events_on || term) && stepped) {
            uint32_t active = 0;
            double roots[7] = {0, 0, 0, 0, 0, 0, 0};
            for (int e = 0; e < 7; e++)
                if (hc.n_events[e] > seen_events[e]) active |= 1u << e;
            // with a limit met, every sign change of the step is located: the order of the roots decides which of them happened
            const bool met = term && rk_terminal_any_met(active, seen_events, ctx->terminal);
            for (int e = 0; e < 7; e++) {
                if (((active >> e) & 1) && (events_on || met)) {
                    // only the newest sign change can be refined (earlier ones were refined at their own pause)
                    double ga[7];
                    if (int rc = dense_eval(ctx, m, layout, small, hc, hc.t_old, nullptr, ga)) return rc;
                    double root = hc.ev_last[e];
                    auto monitor_at = [&](double tq, double* v) -> int {   // monitor e on the step's dense output (solve_event_equation, ivp.py:51-76)
                        double gq[7];
                        if (int rc = dense_eval(ctx, m, layout, small, hc, tq, nullptr, gq)) return rc;
                        *v = gq[e];
                        return 0;
                    };
                    if (int rc = brent_root(monitor_at, hc.t_old, ga[e], hc.t, hc.g[e], &root)) return rc;
                    roots[e] = root;
                    if (met) continue;   // stored and counted below, once the rule has spoken
                    for (int64_t k = seen_events[e]; k < hc.n_events[e]; k++)
                        if (k < max_events) t_events[e * max_events + k] = root;
                    seen_events[e] = hc.n_events[e];
                }
            }
            if (met) {
                uint32_t keep = 0;
                int64_t slot[7];
                rk_terminal_step(active, roots, seen_events, ctx->terminal, events_on ? max_events : 0, &keep, &t_stop, seen_events, slot);
                for (int e = 0; e < 7; e++) {
                    if (slot[e] >= 0) t_events[e * max_events + slot[e]] = roots[e];
                    hc.n_events[e] = seen_events[e];   // a dropped sign change is un-counted: it never happened
                }
            } else if (!events_on) {
                for (int e = 0; e < 7; e++) seen_events[e] = hc.n_events[e];
            }
        }
        const double t_lim = t_stop < hc.t ? t_stop : hc.t;   // the samples of this step: up to where it ends
        // t_eval samples inside (t_old, t]  (ivp.py:706-723)
        if (stepped) {
            while (eval_i < n_eval && t_eval[eval_i] <= t_lim) {
                double* dst = y_eval_dev + eval_i * sd;
                if (t_eval[eval_i] <= hc.t_old && hc.n_acc == 1 && t_eval[eval_i] == t0) {
                    HIP_OK(ctx, hipMemcpyAsync(dst, small ? ctx->buf[1] : ctx->buf[hc.cur ^ 1], sizeof(double) * sd, hipMemcpyDeviceToDevice, ctx->stream));
                } else if (int rc = dense_eval(ctx, m, layout, small, hc, t_eval[eval_i], dst, nullptr)) return rc;
                eval_i++;
            }
        } else {
            while (eval_i < n_eval && t_eval[eval_i] <= hc.t) {  // t0 == t1: no step was taken
                HIP_OK(ctx, hipMemcpyAsync(y_eval_dev + eval_i * sd, ctx->buf[small ? 0 : hc.cur], sizeof(double) * sd, hipMemcpyDeviceToDevice, ctx->stream));
                eval_i++;
            }
        }
        if (t_stop <= hc.t) {   // the state there (the expression that writes a sample), its monitors, scipy's status 1
            double g[7];
            if (int rc = dense_eval(ctx, m, layout, small, hc, t_stop, ctx->buf[small ? 0 : hc.cur], g)) return rc;
            for (int e = 0; e < 7; e++) hc.g[e] = g[e];
            hc.t = t_stop;
            hc.status = ST_TERMINAL;
            break;
        }
        if (hc.status != ST_PAUSED) break;
        hipLaunchKernelGGL(rk45_resume_kernel, dim3(1), dim3(1), 0, ctx->stream, ctx->dctrl, next_pause(), max_attempts);
        LAUNCH_OK(ctx);
    }
    ctrl_to_stats(hc, stats);
    if (!small && hc.cur != 0) {
        HIP_OK(ctx, hipMemcpyAsync(ctx->buf[0], ctx->buf[1], sizeof(double) * sd, hipMemcpyDeviceToDevice, ctx->stream));
        HIP_OK(ctx, hipMemcpyAsync(ctx->buf[2], ctx->buf[3], sizeof(double) * sd, hipMemcpyDeviceToDevice, ctx->stream));
    }
    HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// A device buffer of *cap doubles to at least n (the contents are not kept; the stream is idle before the old one is freed)
static int grow_dev(marl_ctx* ctx, double** buf, size_t* cap, size_t n)
{
    if (*cap >= n) return 0;
    HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
    if (*buf) HIP_OK(ctx, hipFree(*buf));
    *buf = nullptr;
    *cap = 0;
    HIP_OK(ctx, hipMalloc((void**)buf, sizeof(double) * n));
    *cap = n;
    return 0;
}

// The RK45 sweep behind marl_sweep_rk45_dev / _eval_dev / _events_dev (`entry`: the one the caller used).  Neither samples (n_eval == 0)
// nor roots (no t_events or max_events <= 0): rk45_sweep_kernel; samples only: rk45_sweep_eval_kernel; roots, with samples or
// without: rk45_sweep_roots_kernel.  terminal_ok: the entry honours ctx->terminal (marl_sweep_rk45_terminal_dev / rk23; the others refuse a
// context with limits): with a limit set the sweep is one launch of rk45_sweep_term_kernel, whatever else was asked for; with none it is
// the dispatch above.
static int sweep_rk(const RkMethod& m, const char* entry, marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol,
                      int64_t max_attempts, const double* t_eval, int64_t n_eval, double* y_eval_dev, int64_t* n_done, double* t_events,
                      int64_t max_events, marl_stats* stats, bool terminal_ok = false)
{
    if (!ctx || !y_dev || !stats || n_eval < 0 || (n_eval > 0 && (!t_eval || !y_eval_dev || !n_done)))
        return ctx ? fail(ctx, -1, "%s: invalid argument", entry) : -1;
    if (!terminal_ok) { NO_TERMINAL(ctx, entry) }
    const bool frames = n_eval > 0, roots = t_events && max_events > 0, term = has_terminal(ctx);
    if (!frames && !roots && n_done) memset(n_done, 0, sizeof(int64_t) * ctx->batch);   // nothing to sample: the plain sweep itself
    if (!(first_step > 0) || !(t1 >= t0)) return fail(ctx, -1, "%s: need first_step > 0 and t1 >= t0 (forward integration)", m.name);
    if (t1 > t0 && first_step > t1 - t0) return fail(ctx, -1, "%s: `first_step` exceeds bounds", m.name);
    for (int64_t i = 0; i < n_eval; i++)
        if (!(t_eval[i] >= t0) || !(t_eval[i] <= t1) || (i > 0 && t_eval[i] <= t_eval[i - 1]))
            return fail(ctx, -1, "%s: `t_eval` must be sorted and within t_span", m.name);  // ivp.py:603-609
    HIP_OK(ctx, hipSetDevice(ctx->device));
    const int blk = sweep_block(ctx);
    if (!blk) return fail(ctx, -1, "%s: N = %lld exceeds the largest one-workgroup window (1024 cells)", m.sweep_entry, (long long)ctx->N);
    const size_t n_tev = roots ? (size_t)ctx->batch * 7 * (size_t)max_events : 0;
    if (frames)
        if (int rc = grow_dev(ctx, &ctx->sw_teval, &ctx->sw_teval_cap, (size_t)n_eval)) return rc;
    if ((frames || roots || term) && !ctx->sw_ndone) HIP_OK(ctx, hipMalloc((void**)&ctx->sw_ndone, sizeof(int64_t) * ctx->batch));
    if (roots) {
        if (int rc = grow_dev(ctx, &ctx->sw_tev, &ctx->sw_tev_cap, n_tev)) return rc;
        HIP_OK(ctx, hipMemsetAsync(ctx->sw_tev, 0xff, sizeof(double) * n_tev, ctx->stream));   // NaN beyond the roots found (all bits set is a quiet NaN)
    }
    // (pageable host memory: the copy has left the caller's array when the call returns)
    if (frames) HIP_OK(ctx, hipMemcpyAsync(ctx->sw_teval, t_eval, sizeof(double) * n_eval, hipMemcpyHostToDevice, ctx->stream));
    if (frames || roots || term) HIP_OK(ctx, hipMemsetAsync(ctx->sw_ndone, 0, sizeof(int64_t) * ctx->batch, ctx->stream));   // an instance that never runs writes none
    if (int rc = launch_monitors(ctx, y_dev, LAYOUT_FIELD_MAJOR)) return rc;
    hipLaunchKernelGGL(rk45_init_kernel, dim3((unsigned)ctx->batch), dim3(1), 0, ctx->stream, ctx->dctrl, ctx->rec, t0, t1, first_step, clamp_rtol(rtol),
                       atol, (int64_t)NF * ctx->N, max_attempts, 0);
    LAUNCH_OK(ctx);
    const SweepLaunch a = {y_dev, nullptr, nullptr, frames ? ctx->sw_teval : nullptr, n_eval, y_eval_dev, ctx->sw_ndone, roots ? ctx->sw_tev : nullptr,
                           roots ? max_events : 0, term ? ctx->terminal : nullptr};
    if (int rc = m.sweep(ctx, term ? SWEEP_TERM : (roots ? SWEEP_ROOTS : (frames ? SWEEP_EVAL : SWEEP_PLAIN)), blk, (unsigned)ctx->batch, a)) return rc;
    HIP_OK(ctx, hipMemcpyAsync(ctx->hctrl, ctx->dctrl, sizeof(Rk45Ctrl) * ctx->batch, hipMemcpyDeviceToHost, ctx->stream));
    if ((frames || roots) && n_done) HIP_OK(ctx, hipMemcpyAsync(n_done, ctx->sw_ndone, sizeof(int64_t) * ctx->batch, hipMemcpyDeviceToHost, ctx->stream));
    if (roots) HIP_OK(ctx, hipMemcpyAsync(t_events, ctx->sw_tev, sizeof(double) * n_tev, hipMemcpyDeviceToHost, ctx->stream));
    HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
    for (int64_t b = 0; b < ctx->batch; b++) ctrl_to_stats(ctx->hctrl[b], &stats[b]);
    if (t1 == t0 && frames && t_eval[0] == t0) {   // no step is taken (base.py:189-194), so no roots; the sample at t0 is y0, as rk45_run gives it to single runs
        const size_t row = sizeof(double) * NF * ctx->N;
        HIP_OK(ctx, hipMemcpy2DAsync(y_eval_dev, row * n_eval, y_dev, row, row, (size_t)ctx->batch, hipMemcpyDeviceToDevice, ctx->stream));
        HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
        for (int64_t b = 0; b < ctx->batch; b++) n_done[b] = 1;
    }
    return 0;
}

extern "C" {

int marl_rhs_dev(marl_ctx* ctx, double t, const double* y_dev, double* dydt_dev, int layout)
{
    (void)t;
    if (!ctx || !y_dev || !dydt_dev || y_dev == dydt_dev) return ctx ? fail(ctx, -1, "marl_rhs_dev: invalid argument") : -1;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    return launch_rhs(ctx, y_dev, dydt_dev, layout);
}

int marl_rhs(marl_ctx* ctx, double t, const double* y, double* dydt)
{
    (void)t;
    if (!ctx || !y || !dydt) return ctx ? fail(ctx, -1, "marl_rhs: invalid argument") : -1;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)NF * ctx->N * ctx->batch;
    if (int rc = ensure(ctx, 0, n)) return rc;
    if (int rc = ensure(ctx, 1, n)) return rc;
    HIP_OK(ctx, hipMemcpyAsync(ctx->buf[0], y, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (int rc = launch_rhs(ctx, ctx->buf[0], ctx->buf[1], LAYOUT_FIELD_MAJOR)) return rc;
    HIP_OK(ctx, hipMemcpyAsync(dydt, ctx->buf[1], n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int marl_events_dev(marl_ctx* ctx, const double* y_dev, int layout, double* out)
{
    if (!ctx || !y_dev || !out) return ctx ? fail(ctx, -1, "marl_events_dev: invalid argument") : -1;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    if (int rc = launch_monitors(ctx, y_dev, layout)) return rc;
    HIP_OK(ctx, hipMemcpyAsync(ctx->hrec, ctx->rec, sizeof(double) * NQ * ctx->batch, hipMemcpyDeviceToHost, ctx->stream));
    HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
    for (int64_t b = 0; b < ctx->batch; b++) record_to_events(ctx->hrec + b * NQ, out + b * MARL_NEVENTS);
    return 0;
}

int marl_events(marl_ctx* ctx, const double* y, double* out)
{
    if (!ctx || !y || !out) return ctx ? fail(ctx, -1, "marl_events: invalid argument") : -1;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)NF * ctx->N * ctx->batch;
    if (int rc = ensure(ctx, 0, n)) return rc;
    HIP_OK(ctx, hipMemcpyAsync(ctx->buf[0], y, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    return marl_events_dev(ctx, ctx->buf[0], LAYOUT_FIELD_MAJOR, out);
}

int marl_debug_math(marl_ctx* ctx, int op, const double* x_dev, double* y_dev, int64_t n, double e)
{
    if (!ctx || !x_dev || !y_dev || n < 0) return ctx ? fail(ctx, -1, "marl_debug_math: invalid argument") : -1;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    if (n == 0) return 0;
    hipLaunchKernelGGL(math_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, op, x_dev, y_dev, n, e);
    LAUNCH_OK(ctx);
    return 0;
}

int marl_convert_layout_dev(marl_ctx* ctx, const double* src_dev, double* dst_dev, int src_layout, int dst_layout)
{
    if (!ctx || !src_dev || !dst_dev || src_dev == dst_dev) return ctx ? fail(ctx, -1, "marl_convert_layout_dev: invalid argument") : -1;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    return launch_convert(ctx, src_dev, dst_dev, src_layout, dst_layout);
}

int marl_integrate_rk4_dev(marl_ctx* ctx, double* y_dev, int layout, double dt, int64_t nsteps)
{
    if (!ctx || !y_dev || nsteps < 0) return ctx ? fail(ctx, -1, "marl_integrate_rk4_dev: invalid argument") : -1;
    if (ctx->batch != 1) return fail(ctx, -1, "marl_integrate_rk4_dev: single-instance context required (use marl_sweep_rk4_dev)");
    HIP_OK(ctx, hipSetDevice(ctx->device));
    if (int rc = ensure(ctx, 1, (size_t)state_doubles(ctx->slab.n_buf, layout))) return rc;
    return rk4_run(ctx, y_dev, ctx->buf[1], layout, dt, nsteps);
}

int marl_sweep_rk4_dev(marl_ctx* ctx, double* y_dev, const double* dt, int64_t nsteps)
{
    if (!ctx || !y_dev || !dt || nsteps < 0) return ctx ? fail(ctx, -1, "marl_sweep_rk4_dev: invalid argument") : -1;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    const int blk = sweep_block(ctx);
    if (!blk) return fail(ctx, -1, "marl_sweep_rk4_dev: N = %lld exceeds the largest one-workgroup window (1024 cells)", (long long)ctx->N);
    // through the context's pinned buffer: `dt` may be a temporary of the caller (the previous use of hdt has long completed
    // in stream order only if we wait for it - a sweep launch is milliseconds, the wait is free)
    HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(ctx->hdt, dt, sizeof(double) * ctx->batch);
    HIP_OK(ctx, hipMemcpyAsync(ctx->ddt, ctx->hdt, sizeof(double) * ctx->batch, hipMemcpyHostToDevice, ctx->stream));
    const dim3 grid((unsigned)ctx->batch);
    SWEEP_DISPATCH(rk4_sweep_kernel, y_dev, ctx->dconsts, ctx->ddt, ctx->N, nsteps)
    LAUNCH_OK(ctx);
    return 0;
}

int marl_integrate_rk4(marl_ctx* ctx, double* y, double dt, int64_t nsteps)
{
    if (!ctx || !y || nsteps < 0) return ctx ? fail(ctx, -1, "marl_integrate_rk4: invalid argument") : -1;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)NF * ctx->N * ctx->batch;
    if (int rc = ensure(ctx, 2, n)) return rc;
    HIP_OK(ctx, hipMemcpyAsync(ctx->buf[2], y, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (ctx->batch > 1 || sweep_block(ctx) > 0) {
        // small grids (one workgroup each, on-chip for all steps) and sweeps
        std::vector<double> dts((size_t)ctx->batch, dt);
        if (int rc = marl_sweep_rk4_dev(ctx, ctx->buf[2], dts.data(), nsteps)) return rc;
    } else {
        const int layout = (int)ctx->host_layout;
        const size_t sd = (size_t)state_doubles(ctx->N, layout);
        if (int rc = ensure(ctx, 0, sd)) return rc;
        if (int rc = ensure(ctx, 1, sd)) return rc;
        if (int rc = launch_convert(ctx, ctx->buf[2], ctx->buf[0], LAYOUT_FIELD_MAJOR, layout)) return rc;
        if (int rc = rk4_run(ctx, ctx->buf[0], ctx->buf[1], layout, dt, nsteps)) return rc;
        if (int rc = launch_convert(ctx, ctx->buf[0], ctx->buf[2], layout, LAYOUT_FIELD_MAJOR)) return rc;
    }
    HIP_OK(ctx, hipMemcpyAsync(y, ctx->buf[2], n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
    return stream_check(ctx);
}

// ---- monitored fixed-step RK4, grids of one workgroup (include/marl_hip.h; kernel: marl_rk4_watch.h, a translation unit of its own;
// rules and record: marl_rk4_watch_ctl.h) ----
int marl_rk4_watch_launch(int blk, int vd, unsigned grid, hipStream_t stream, double* Y, const void* consts, void* recs, int64_t N, int64_t nsteps,
                          const int64_t* frame_steps, int64_t n_frames, double* frames, double* t_events, int64_t max_events, const int64_t* terminal);

static void rk4_watch_to_stats(const Rk4WatchRec& r, marl_stats* st)
{
    memset(st, 0, sizeof *st);
    st->nfev = 4 * r.steps;
    st->n_accepted = r.steps;
    st->status = r.status;
    st->t = r.t;
    st->h_next = r.dt;
    for (int e = 0; e < 7; e++) { st->event_value[e] = r.g[e]; st->n_events[e] = r.n_events[e]; }
}

int marl_sweep_rk4_watch_dev(marl_ctx* ctx, double* y_dev, double t0, const double* dt, int64_t nsteps, const int64_t* frame_steps, int64_t n_frames,
                             double* frames_dev, int64_t* n_done, double* t_events, int64_t max_events, marl_stats* stats)
{
    if (!ctx || !y_dev || !dt || !stats || nsteps < 0 || n_frames < 0 || (n_frames > 0 && (!frame_steps || !frames_dev)))
        return ctx ? fail(ctx, -1, "marl_sweep_rk4_watch_dev: invalid argument") : -1;
    if (ctx->halo > 0) return fail(ctx, -1, "marl_sweep_rk4_watch_dev: slab contexts (domain decomposition) are not supported");
    const int blk = sweep_block(ctx);
    if (!blk)
        return fail(ctx, -1, "marl_sweep_rk4_watch_dev: N = %lld exceeds the largest one-workgroup window: the monitored RK4 loop runs N <= 1024 cells",
                    (long long)ctx->N);
    if (const int64_t bad = rk4_watch_check_frames(frame_steps, n_frames, nsteps); bad >= 0)
        return fail(ctx, -1, "marl_sweep_rk4_watch_dev: frame_steps[%lld] = %lld: the step counts must be strictly ascending within [0, nsteps = %lld]",
                    (long long)bad, (long long)frame_steps[bad], (long long)nsteps);
    HIP_OK(ctx, hipSetDevice(ctx->device));
    const bool roots = t_events && max_events > 0;
    const size_t B = (size_t)ctx->batch, n_tev = roots ? B * 7 * (size_t)max_events : 0;
    static_assert(sizeof(Rk4WatchRec) % sizeof(double) == 0 && sizeof(int64_t) == sizeof(double), "the records and step counts live in buffers of doubles");
    if (int rc = grow_dev(ctx, &ctx->rk4w_recs, &ctx->rk4w_recs_cap, B * (sizeof(Rk4WatchRec) / sizeof(double)) + 7)) return rc;
    if (n_frames > 0)
        if (int rc = grow_dev(ctx, &ctx->sw_teval, &ctx->sw_teval_cap, (size_t)n_frames)) return rc;
    if (roots) {
        if (int rc = grow_dev(ctx, &ctx->sw_tev, &ctx->sw_tev_cap, n_tev)) return rc;
        HIP_OK(ctx, hipMemsetAsync(ctx->sw_tev, 0xff, sizeof(double) * n_tev, ctx->stream));   // NaN beyond the roots stored
    }
    std::vector<Rk4WatchRec> recs(B);
    memset(recs.data(), 0, sizeof(Rk4WatchRec) * B);
    for (size_t b = 0; b < B; b++) { recs[b].t0 = recs[b].t = t0; recs[b].dt = dt[b]; }
    // (pageable host memory: the copies have left the vector and the caller's array when the calls return)
    HIP_OK(ctx, hipMemcpyAsync(ctx->rk4w_recs, recs.data(), sizeof(Rk4WatchRec) * B, hipMemcpyHostToDevice, ctx->stream));
    if (n_frames > 0) HIP_OK(ctx, hipMemcpyAsync(ctx->sw_teval, frame_steps, sizeof(int64_t) * n_frames, hipMemcpyHostToDevice, ctx->stream));
    int64_t* dlim = reinterpret_cast<int64_t*>(ctx->rk4w_recs + B * (sizeof(Rk4WatchRec) / sizeof(double)));   // the limits, behind the records
    if (has_terminal(ctx)) HIP_OK(ctx, hipMemcpyAsync(dlim, ctx->terminal, sizeof(int64_t) * 7, hipMemcpyHostToDevice, ctx->stream));
    const int err = marl_rk4_watch_launch(blk, ctx->var_dphi ? 1 : 0, (unsigned)ctx->batch, ctx->stream, y_dev, ctx->dconsts, ctx->rk4w_recs, ctx->N, nsteps,
                                          n_frames > 0 ? reinterpret_cast<const int64_t*>(ctx->sw_teval) : nullptr, n_frames, frames_dev,
                                          roots ? ctx->sw_tev : nullptr, roots ? max_events : 0, has_terminal(ctx) ? dlim : nullptr);
    if (err != (int)hipSuccess) return fail(ctx, -3, "rk4 watch: kernel launch failed: %s", hipGetErrorString((hipError_t)err));
    HIP_OK(ctx, hipMemcpyAsync(recs.data(), ctx->rk4w_recs, sizeof(Rk4WatchRec) * B, hipMemcpyDeviceToHost, ctx->stream));
    if (roots) HIP_OK(ctx, hipMemcpyAsync(t_events, ctx->sw_tev, sizeof(double) * n_tev, hipMemcpyDeviceToHost, ctx->stream));
    HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t b = 0; b < B; b++) {
        rk4_watch_to_stats(recs[b], &stats[b]);
        if (n_done) n_done[b] = recs[b].next_frame;
    }
    return 0;
}

int marl_integrate_rk4_watch(marl_ctx* ctx, double* y, double t0, double dt, int64_t nsteps, const int64_t* frame_steps, int64_t n_frames,
                             double* y_frames, int64_t* n_done, double* t_events, int64_t max_events, marl_stats* stats)
{
    if (!ctx || !y || !stats || nsteps < 0 || n_frames < 0 || (n_frames > 0 && (!frame_steps || !y_frames)))
        return ctx ? fail(ctx, -1, "marl_integrate_rk4_watch: invalid argument") : -1;
    if (ctx->batch != 1) return fail(ctx, -1, "marl_integrate_rk4_watch: single-instance context required (use marl_sweep_rk4_watch_dev)");
    if (!sweep_block(ctx))
        return fail(ctx, -1, "marl_integrate_rk4_watch: N = %lld exceeds the largest one-workgroup window: the monitored RK4 loop runs N <= 1024 cells",
                    (long long)ctx->N);
    if (const int64_t bad = rk4_watch_check_frames(frame_steps, n_frames, nsteps); bad >= 0)
        return fail(ctx, -1, "marl_integrate_rk4_watch: frame_steps[%lld] = %lld: the step counts must be strictly ascending within [0, nsteps = %lld]",
                    (long long)bad, (long long)frame_steps[bad], (long long)nsteps);
    HIP_OK(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)NF * ctx->N;
    if (int rc = ensure(ctx, 2, n)) return rc;
    if (n_frames > 0)
        if (int rc = ensure(ctx, 3, n * (size_t)n_frames)) return rc;
    HIP_OK(ctx, hipMemcpyAsync(ctx->buf[2], y, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    int64_t done = 0;
    if (int rc = marl_sweep_rk4_watch_dev(ctx, ctx->buf[2], t0, &dt, nsteps, frame_steps, n_frames, n_frames > 0 ? ctx->buf[3] : nullptr, &done, t_events,
                                          max_events, stats))
        return rc;
    HIP_OK(ctx, hipMemcpyAsync(y, ctx->buf[2], n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (done > 0) HIP_OK(ctx, hipMemcpyAsync(y_frames, ctx->buf[3], n * (size_t)done * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
    if (n_done) *n_done = done;
    return 0;
}

int marl_sweep_rk45_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol,
                        int64_t max_attempts, marl_stats* stats)
{
    return sweep_rk(kRk45, "marl_sweep_rk45_dev", ctx, y_dev, t0, t1, first_step, rtol, atol, max_attempts, nullptr, 0, nullptr, nullptr, nullptr, 0, stats);
}

int marl_sweep_rk45_eval_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol,
                             int64_t max_attempts, const double* t_eval, int64_t n_eval, double* y_eval_dev, int64_t* n_done,
                             marl_stats* stats)
{
    return sweep_rk(kRk45, "marl_sweep_rk45_eval_dev", ctx, y_dev, t0, t1, first_step, rtol, atol, max_attempts, t_eval, n_eval, y_eval_dev, n_done,
                      nullptr, 0, stats);
}

int marl_sweep_rk45_events_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol,
                               int64_t max_attempts, const double* t_eval, int64_t n_eval, double* y_eval_dev, int64_t* n_done,
                               double* t_events, int64_t max_events, marl_stats* stats)
{
    return sweep_rk(kRk45, "marl_sweep_rk45_events_dev", ctx, y_dev, t0, t1, first_step, rtol, atol, max_attempts, t_eval, n_eval, y_eval_dev, n_done,
                      t_events, max_events, stats);
}

int marl_sweep_rk45_terminal_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol,
                                 int64_t max_attempts, const double* t_eval, int64_t n_eval, double* y_eval_dev, int64_t* n_done,
                                 double* t_events, int64_t max_events, marl_stats* stats)
{
    return sweep_rk(kRk45, "marl_sweep_rk45_terminal_dev", ctx, y_dev, t0, t1, first_step, rtol, atol, max_attempts, t_eval, n_eval, y_eval_dev, n_done,
                    t_events, max_events, stats, true);
}

// marl_integrate_<method>_dev
static int integrate_rk_dev(const RkMethod& m, marl_ctx* ctx, double* y_dev, int layout, double t0, double t1, double first_step, double rtol,
                            double atol, int64_t max_attempts, marl_stats* stats)
{
    const char* en = m.entry ? m.entry : m.name;
    if (!ctx || !y_dev || !stats) return ctx ? fail(ctx, -1, "marl_integrate_%s_dev: invalid argument", en) : -1;
    NO_TERMINAL(ctx, (std::string("marl_integrate_") + en + "_dev").c_str())
    if (ctx->batch != 1) return fail(ctx, -1, "marl_integrate_%s_dev: single-instance context required (use %s)", en, m.sweep_entry);
    if (!m.can_stream && ctx->halo > 0) return fail(ctx, -1, "%s: slab contexts (domain decomposition) are not supported", m.name);
    HIP_OK(ctx, hipSetDevice(ctx->device));
    const size_t sd = (size_t)state_doubles(ctx->slab.n_buf, layout);
    for (int i = 0; i < 4; i++)
        if (int rc = ensure(ctx, i, sd)) return rc;
    HIP_OK(ctx, hipMemcpyAsync(ctx->buf[0], y_dev, sd * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    if (int rc = rk_run(m, ctx, layout, false, t0, t1, first_step, rtol, atol, nullptr, 0, nullptr, nullptr, 0, max_attempts, stats)) return rc;
    HIP_OK(ctx, hipMemcpyAsync(y_dev, ctx->buf[0], sd * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// marl_integrate_<method>
static int integrate_rk(const RkMethod& m, marl_ctx* ctx, double* y, double t0, double t1, double first_step, double rtol, double atol,
                        const double* t_eval, int64_t n_eval, double* y_eval, double* t_events, int64_t max_events,
                        int64_t max_attempts, marl_stats* stats, bool terminal_ok = false)
{
    const char* en = m.entry ? m.entry : m.name;
    if (!ctx || !y || !stats || (n_eval > 0 && (!t_eval || !y_eval)))
        return ctx ? fail(ctx, -1, "marl_integrate_%s%s: invalid argument", en, terminal_ok && !m.entry ? "_terminal" : "") : -1;
    if (!terminal_ok) { NO_TERMINAL(ctx, (std::string("marl_integrate_") + en).c_str()) }
    if (ctx->batch != 1) return fail(ctx, -1, "marl_integrate_%s: single-instance context required (use %s)", en, m.sweep_entry);
    if (!m.can_stream && ctx->halo > 0) return fail(ctx, -1, "%s: slab contexts (domain decomposition) are not supported", m.name);
    HIP_OK(ctx, hipSetDevice(ctx->device));
    const bool small = !m.grid_only && sweep_block(ctx) > 0;
    const int layout = small ? LAYOUT_FIELD_MAJOR : (int)ctx->host_layout;
    const size_t n = (size_t)NF * ctx->N;
    const size_t sd = (size_t)state_doubles(ctx->N, layout);
    for (int i = 0; i < 4; i++)
        if (int rc = ensure(ctx, i, sd > n ? sd : n)) return rc;
    // upload field-major into buf[1], convert into buf[0]
    HIP_OK(ctx, hipMemcpyAsync(ctx->buf[1], y, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (int rc = launch_convert(ctx, ctx->buf[1], ctx->buf[0], LAYOUT_FIELD_MAJOR, layout)) return rc;
    double* yev = nullptr;
    if (n_eval > 0) HIP_OK(ctx, hipMalloc((void**)&yev, sizeof(double) * sd * (size_t)(n_eval + 1)));
    int rc = rk_run(m, ctx, layout, small, t0, t1, first_step, rtol, atol, t_eval, n_eval, yev, t_events, max_events, max_attempts, stats);
    if (rc == 0) {
        // results back to field-major through a spare slot.  The large-grid DOP853 entry returns the frames it wrote - the samples up to
        // stats->t, where the run ended (t1, a terminal monitor's root, or the attempt budget) - and leaves the caller's later frames untouched.
        int64_t n_back = n_eval;
        if (m.grid_only) {
            n_back = 0;
            while (n_back < n_eval && t_eval[n_back] <= stats->t) n_back++;
        }
        for (int64_t i = 0; i < n_back && rc == 0; i++) {
            rc = launch_convert(ctx, yev + i * sd, yev + n_eval * sd, layout, LAYOUT_FIELD_MAJOR);
            if (rc == 0 && hipMemcpyAsync(y_eval + i * n, yev + n_eval * sd, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
                rc = fail(ctx, -3, "copy of t_eval sample failed");
            if (rc == 0 && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = fail(ctx, -3, "sync failed");
        }
        if (rc == 0) rc = launch_convert(ctx, ctx->buf[0], ctx->buf[1], layout, LAYOUT_FIELD_MAJOR);
        if (rc == 0 && hipMemcpyAsync(y, ctx->buf[1], n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
            rc = fail(ctx, -3, "copy of final state failed");
        if (rc == 0 && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = fail(ctx, -3, "sync failed");
    }
    if (yev) (void)hipFree(yev);
    return rc;
}

int marl_integrate_rk45_dev(marl_ctx* ctx, double* y_dev, int layout, double t0, double t1, double first_step, double rtol,
                            double atol, int64_t max_attempts, marl_stats* stats)
{
    return integrate_rk_dev(kRk45, ctx, y_dev, layout, t0, t1, first_step, rtol, atol, max_attempts, stats);
}

int marl_integrate_rk45(marl_ctx* ctx, double* y, double t0, double t1, double first_step, double rtol, double atol,
                        const double* t_eval, int64_t n_eval, double* y_eval, double* t_events, int64_t max_events,
                        int64_t max_attempts, marl_stats* stats)
{
    return integrate_rk(kRk45, ctx, y, t0, t1, first_step, rtol, atol, t_eval, n_eval, y_eval, t_events, max_events, max_attempts, stats);
}

// ---- RK23: the RK45 entries with the method swapped (include/marl_hip.h) ----
int marl_integrate_rk23_dev(marl_ctx* ctx, double* y_dev, int layout, double t0, double t1, double first_step, double rtol,
                            double atol, int64_t max_attempts, marl_stats* stats)
{
    return integrate_rk_dev(kRk23, ctx, y_dev, layout, t0, t1, first_step, rtol, atol, max_attempts, stats);
}

int marl_integrate_rk23(marl_ctx* ctx, double* y, double t0, double t1, double first_step, double rtol, double atol,
                        const double* t_eval, int64_t n_eval, double* y_eval, double* t_events, int64_t max_events,
                        int64_t max_attempts, marl_stats* stats)
{
    return integrate_rk(kRk23, ctx, y, t0, t1, first_step, rtol, atol, t_eval, n_eval, y_eval, t_events, max_events, max_attempts, stats);
}

int marl_sweep_rk23_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol,
                        int64_t max_attempts, marl_stats* stats)
{
    return sweep_rk(kRk23, "marl_sweep_rk23_dev", ctx, y_dev, t0, t1, first_step, rtol, atol, max_attempts, nullptr, 0, nullptr, nullptr, nullptr, 0, stats);
}

int marl_sweep_rk23_eval_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol,
                             int64_t max_attempts, const double* t_eval, int64_t n_eval, double* y_eval_dev, int64_t* n_done,
                             marl_stats* stats)
{
    return sweep_rk(kRk23, "marl_sweep_rk23_eval_dev", ctx, y_dev, t0, t1, first_step, rtol, atol, max_attempts, t_eval, n_eval, y_eval_dev, n_done,
                    nullptr, 0, stats);
}

int marl_sweep_rk23_events_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol,
                               int64_t max_attempts, const double* t_eval, int64_t n_eval, double* y_eval_dev, int64_t* n_done,
                               double* t_events, int64_t max_events, marl_stats* stats)
{
    return sweep_rk(kRk23, "marl_sweep_rk23_events_dev", ctx, y_dev, t0, t1, first_step, rtol, atol, max_attempts, t_eval, n_eval, y_eval_dev, n_done,
                    t_events, max_events, stats);
}

int marl_sweep_rk23_terminal_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol,
                                 int64_t max_attempts, const double* t_eval, int64_t n_eval, double* y_eval_dev, int64_t* n_done,
                                 double* t_events, int64_t max_events, marl_stats* stats)
{
    return sweep_rk(kRk23, "marl_sweep_rk23_terminal_dev", ctx, y_dev, t0, t1, first_step, rtol, atol, max_attempts, t_eval, n_eval, y_eval_dev, n_done,
                    t_events, max_events, stats, true);
}

// the single runs that stop at a terminal monitor's root (rk_run)
int marl_integrate_rk45_terminal(marl_ctx* ctx, double* y, double t0, double t1, double first_step, double rtol, double atol,
                                 const double* t_eval, int64_t n_eval, double* y_eval, double* t_events, int64_t max_events,
                                 int64_t max_attempts, marl_stats* stats)
{
    return integrate_rk(kRk45, ctx, y, t0, t1, first_step, rtol, atol, t_eval, n_eval, y_eval, t_events, max_events, max_attempts, stats, true);
}

int marl_integrate_rk23_terminal(marl_ctx* ctx, double* y, double t0, double t1, double first_step, double rtol, double atol,
                                 const double* t_eval, int64_t n_eval, double* y_eval, double* t_events, int64_t max_events,
                                 int64_t max_attempts, marl_stats* stats)
{
    return integrate_rk(kRk23, ctx, y, t0, t1, first_step, rtol, atol, t_eval, n_eval, y_eval, t_events, max_events, max_attempts, stats, true);
}


// ---- DOP853: grids of one workgroup only (include/marl_hip.h; kernels: marl_dop853.h, a translation unit of its own) ----
}  // extern "C"
extern "C" {
int64_t marl_dop853_arena_doubles(int64_t grid, int blk);
int marl_dop853_launch_sweep(int kind, int blk, int vd, unsigned grid, hipStream_t stream, double* Y, const void* consts, void* ctrls, int64_t N,
                             double* karena, const double* t_eval, int64_t n_eval, double* Yeval, int64_t* n_done, double* t_events,
                             int64_t max_events);
// marl_dop853_stop.hip: the kernel that stops at a terminal monitor's root (SWEEP_TERM), a unit of its own
int marl_dop853_stop_launch(int blk, int vd, unsigned grid, hipStream_t stream, double* Y, const void* consts, void* ctrls, int64_t N, double* karena,
                            const double* t_eval, int64_t n_eval, double* Yeval, int64_t* n_done, double* t_events, int64_t max_events,
                            const int64_t* terminal);
}
static int dop853_m_sweep(marl_ctx* ctx, int kind, int blk, unsigned batch, const SweepLaunch& a)
{
    if (kind != SWEEP_PLAIN && kind != SWEEP_EVAL && kind != SWEEP_ROOTS && kind != SWEEP_TERM) return fail(ctx, -1, "dop853: no kernel of kind %d", kind);
    if (int rc = grow_dev(ctx, &ctx->dop_k, &ctx->dop_k_cap, (size_t)marl_dop853_arena_doubles((int64_t)batch, blk))) return rc;
    const int err = kind == SWEEP_TERM
                        ? marl_dop853_stop_launch(blk, ctx->var_dphi ? 1 : 0, batch, ctx->stream, a.Y, ctx->dconsts, ctx->dctrl, ctx->N, ctx->dop_k,
                                                  a.t_eval, a.n_eval, a.Yeval, a.n_done, a.t_events, a.max_events, a.terminal)
                        : marl_dop853_launch_sweep(kind, blk, ctx->var_dphi ? 1 : 0, batch, ctx->stream, a.Y, ctx->dconsts, ctx->dctrl, ctx->N,
                                                   ctx->dop_k, a.t_eval, a.n_eval, a.Yeval, a.n_done, a.t_events, a.max_events);
    if (err != (int)hipSuccess) return fail(ctx, -3, "dop853: kernel launch failed: %s", hipGetErrorString((hipError_t)err));
    return 0;
}
// (only the one-workgroup kernels exist: sweep_rk is the one driver, single runs included)
static const RkMethod kDop853 = {"dop853", "marl_sweep_dop853_dev", 0, false, dop853_m_sweep, nullptr, nullptr, nullptr, nullptr};

// what every DOP853 entry refuses before it touches anything: terminal monitors (but for the entries that stop: terminal_ok), grids
// above one workgroup, slabs
static int dop853_refuse(marl_ctx* ctx, const char* entry, bool terminal_ok = false)
{
    if (!terminal_ok) { NO_TERMINAL(ctx, entry) }
    if (ctx->N > 1024)
        return fail(ctx, -1, "dop853: N = %lld: the native DOP853 loop runs grids of one workgroup only, N <= 1024 cells (%s)", (long long)ctx->N, entry);
    if (ctx->halo > 0) return fail(ctx, -1, "dop853: slab contexts (domain decomposition) are not supported");
    return 0;
}

extern "C" {
int marl_sweep_dop853_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol,
                          int64_t max_attempts, marl_stats* stats)
{
    if (ctx)
        if (int rc = dop853_refuse(ctx, "marl_sweep_dop853_dev")) return rc;
    return sweep_rk(kDop853, "marl_sweep_dop853_dev", ctx, y_dev, t0, t1, first_step, rtol, atol, max_attempts, nullptr, 0, nullptr, nullptr, nullptr, 0, stats);
}

int marl_sweep_dop853_eval_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol,
                               int64_t max_attempts, const double* t_eval, int64_t n_eval, double* y_eval_dev, int64_t* n_done,
                               marl_stats* stats)
{
    if (ctx)
        if (int rc = dop853_refuse(ctx, "marl_sweep_dop853_eval_dev")) return rc;
    return sweep_rk(kDop853, "marl_sweep_dop853_eval_dev", ctx, y_dev, t0, t1, first_step, rtol, atol, max_attempts, t_eval, n_eval, y_eval_dev, n_done,
                    nullptr, 0, stats);
}

int marl_sweep_dop853_events_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol,
                                 int64_t max_attempts, const double* t_eval, int64_t n_eval, double* y_eval_dev, int64_t* n_done,
                                 double* t_events, int64_t max_events, marl_stats* stats)
{
    if (ctx)
        if (int rc = dop853_refuse(ctx, "marl_sweep_dop853_events_dev")) return rc;
    return sweep_rk(kDop853, "marl_sweep_dop853_events_dev", ctx, y_dev, t0, t1, first_step, rtol, atol, max_attempts, t_eval, n_eval, y_eval_dev, n_done,
                    t_events, max_events, stats);
}

// marl_sweep_dop853_events_dev honouring terminal monitors: with a limit set one launch of dop853_sweep_stop_kernel, whatever else was
// asked for; with none the dispatch of the three entries above
int marl_sweep_dop853_stop_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol,
                               int64_t max_attempts, const double* t_eval, int64_t n_eval, double* y_eval_dev, int64_t* n_done,
                               double* t_events, int64_t max_events, marl_stats* stats)
{
    if (ctx)
        if (int rc = dop853_refuse(ctx, "marl_sweep_dop853_stop_dev", true)) return rc;
    return sweep_rk(kDop853, "marl_sweep_dop853_stop_dev", ctx, y_dev, t0, t1, first_step, rtol, atol, max_attempts, t_eval, n_eval, y_eval_dev, n_done,
                    t_events, max_events, stats, true);
}
}  // extern "C"

// One instance, host pointers: the sweep that locates roots, for an instance count of one - frames and root times are written by the
// kernel, the host only moves them.  terminal_ok: marl_integrate_dop853_stop, the sweep that stops.
static int integrate_dop853(const char* entry, bool terminal_ok, marl_ctx* ctx, double* y, double t0, double t1, double first_step, double rtol,
                            double atol, const double* t_eval, int64_t n_eval, double* y_eval, double* t_events, int64_t max_events,
                            int64_t max_attempts, marl_stats* stats)
{
    if (!ctx || !y || !stats || n_eval < 0 || (n_eval > 0 && (!t_eval || !y_eval))) return ctx ? fail(ctx, -1, "%s: invalid argument", entry) : -1;
    if (int rc = dop853_refuse(ctx, entry, terminal_ok)) return rc;
    if (ctx->batch != 1) return fail(ctx, -1, "%s: single-instance context required (use marl_sweep_dop853_dev)", entry);
    if (int rc = check_ivp_args(ctx, "dop853", t0, t1, first_step, rtol, atol, t_eval, n_eval)) return rc;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)NF * ctx->N;
    if (int rc = ensure(ctx, 0, n)) return rc;
    HIP_OK(ctx, hipMemcpyAsync(ctx->buf[0], y, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    double* yev = nullptr;
    if (n_eval > 0) HIP_OK(ctx, hipMalloc((void**)&yev, sizeof(double) * n * (size_t)n_eval));
    const bool roots = t_events != nullptr && max_events > 0;
    int64_t n_done = 0;
    int rc = sweep_rk(kDop853, entry, ctx, ctx->buf[0], t0, t1, first_step, rtol, atol, max_attempts, t_eval, n_eval, yev, &n_done,
                      roots ? t_events : nullptr, roots ? max_events : 0, stats, terminal_ok);
    if (rc == 0 && n_done > 0 && hipMemcpyAsync(y_eval, yev, sizeof(double) * n * (size_t)n_done, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
        rc = fail(ctx, -3, "copy of t_eval samples failed");
    if (rc == 0 && hipMemcpyAsync(y, ctx->buf[0], n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
        rc = fail(ctx, -3, "copy of final state failed");
    if (rc == 0 && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = fail(ctx, -3, "sync failed");
    if (yev) (void)hipFree(yev);
    return rc;
}

extern "C" {
int marl_integrate_dop853(marl_ctx* ctx, double* y, double t0, double t1, double first_step, double rtol, double atol,
                          const double* t_eval, int64_t n_eval, double* y_eval, double* t_events, int64_t max_events,
                          int64_t max_attempts, marl_stats* stats)
{
    return integrate_dop853("marl_integrate_dop853", false, ctx, y, t0, t1, first_step, rtol, atol, t_eval, n_eval, y_eval, t_events, max_events,
                            max_attempts, stats);
}

// marl_integrate_dop853 honouring terminal monitors: the run ends at the terminal monitor's root (stats->status 1, stats->t the root,
// y the state there, y_eval the samples up to it); without a limit it is marl_integrate_dop853
int marl_integrate_dop853_stop(marl_ctx* ctx, double* y, double t0, double t1, double first_step, double rtol, double atol,
                               const double* t_eval, int64_t n_eval, double* y_eval, double* t_events, int64_t max_events,
                               int64_t max_attempts, marl_stats* stats)
{
    return integrate_dop853("marl_integrate_dop853_stop", true, ctx, y, t0, t1, first_step, rtol, atol, t_eval, n_eval, y_eval, t_events, max_events,
                            max_attempts, stats);
}
}  // extern "C"

// ---- DOP853 on one grid of any size: one launch per stage (kernels: marl_dop853_grid.h, a translation unit of its own) ----
// The loop is rk_run's - batches of ctx->poll attempts, one status read per batch, Brent on dense evaluations at a pause, terminal
// monitors by rk_terminal_step - with a third row of the method table: an attempt is 12 stage launches, the reduction and the control;
// K_1..K_16 live in an arena of 16 state-shaped buffers (ctx->dop_k) instead of the FSAL pair buf[2], buf[3]; the dense output has 16
// weights and, once per step that needs it, three more stage launches (K_14..K_16).  nfev is counted by the control kernel alone.
extern "C" {
int64_t marl_dop853_grid_part_doubles(int64_t nb);
int marl_dop853_grid_launch_stage(int tiled, int vd, unsigned nb, hipStream_t stream, double* Y0, double* Y1, double* karena, int64_t kstride,
                                  const void* consts, const int64_t slab5[5], const void* ctrl, int s, int replay, double* part);
int marl_dop853_grid_launch_control(hipStream_t stream, double* part, int64_t nb, void* ctrl);
int marl_dop853_grid_launch_dense(int tiled, unsigned nb, hipStream_t stream, const double* yold, const double* karena, int64_t kstride, int frame,
                                  const void* consts, const int64_t slab5[5], double h, double x, int at_start, double* yout, double* part);
}
constexpr int kDop853GridWritten = 256 - 2, kDop853GridSlots = 16, kDop853GridStages = 12;
static int dop853_grid_launched(marl_ctx* ctx, int err)
{
    if (err != (int)hipSuccess) return fail(ctx, -3, "dop853: kernel launch failed: %s", hipGetErrorString((hipError_t)err));
    return 0;
}
static int dop853_grid_stage(marl_ctx* ctx, int64_t nb, int layout, int s, int replay)
{
    const Slab& S = ctx->slab;
    const int64_t slab5[5] = {S.n_buf, S.goff, S.ld, S.out_lo, S.out_hi};
    return dop853_grid_launched(ctx, marl_dop853_grid_launch_stage(layout == LAYOUT_TILED, ctx->var_dphi ? 1 : 0, (unsigned)nb, ctx->stream, ctx->buf[0],
                                                                   ctx->buf[1], ctx->dop_k, state_doubles(S.n_buf, layout), ctx->dconsts, slab5, ctx->dctrl,
                                                                   s, replay, ctx->part));
}
static int64_t dop853_grid_m_part_records(int64_t nb) { return (marl_dop853_grid_part_doubles(nb) + NQ - 1) / NQ; }
// the arena (grown here: nothing of a run is in it yet) and K_1 = f(t0, y0) into the slot of frame 0
static int dop853_grid_m_first_k(marl_ctx* ctx, int layout)
{
    if (int rc = grow_dev(ctx, &ctx->dop_k, &ctx->dop_k_cap, (size_t)kDop853GridSlots * (size_t)state_doubles(ctx->slab.n_buf, layout))) return rc;
    ctx->dop_grid_extra = -1;
    return dop853_grid_stage(ctx, rk_blocks(ctx, kDop853GridWritten), layout, 0, 0);
}
static int dop853_grid_m_attempt(marl_ctx* ctx, int64_t nb, int layout)
{
    for (int s = 1; s <= kDop853GridStages; s++)
        if (int rc = dop853_grid_stage(ctx, nb, layout, s, 0)) return rc;
    return 0;
}
// (launch_attempt's first reduction level is skipped: the control launcher reduces both of the attempt's sums, in one or two levels)
static int dop853_grid_m_control(marl_ctx* ctx, const double*, int64_t)
{
    return dop853_grid_launched(ctx, marl_dop853_grid_launch_control(ctx->stream, ctx->part, rk_blocks(ctx, kDop853GridWritten), ctx->dctrl));
}
static int dop853_grid_m_dense_at(marl_ctx* ctx, int layout, const Rk45Ctrl& c, double t, double* yout, bool want_part, int64_t* nb)
{
    const Slab& S = ctx->slab;
    const int64_t slab5[5] = {S.n_buf, S.goff, S.ld, S.out_lo, S.out_hi};
    if (ctx->dop_grid_extra != c.n_acc) {   // K_14..K_16 of this step, once (rk.py:520-535); the control kernel has counted them
        for (int s = kDop853GridStages + 1; s < kDop853GridSlots; s++)
            if (int rc = dop853_grid_stage(ctx, rk_blocks(ctx, kDop853GridWritten), layout, s, 1)) return rc;
        ctx->dop_grid_extra = c.n_acc;
    }
    *nb = (S.out_hi - S.out_lo + 255) / 256;
    const int frame = c.cur ^ 1;   // the accepted step's first state and slots
    return dop853_grid_launched(ctx, marl_dop853_grid_launch_dense(layout == LAYOUT_TILED, (unsigned)*nb, ctx->stream, ctx->buf[frame], ctx->dop_k,
                                                                   state_doubles(S.n_buf, layout), frame, ctx->dconsts, slab5, c.h_prev,
                                                                   (t - c.t_old) / c.h_prev, t == c.t_old ? 1 : 0, yout, want_part ? ctx->part : nullptr));
}
static const RkMethod kDop853Grid = {"dop853", "marl_sweep_dop853_dev", kDop853GridWritten, false, nullptr, dop853_grid_m_attempt, dop853_grid_m_control,
                                     nullptr, nullptr, "dop853_grid", true, dop853_grid_m_part_records, dop853_grid_m_first_k, dop853_grid_m_dense_at};

extern "C" {
int marl_integrate_dop853_grid_dev(marl_ctx* ctx, double* y_dev, int layout, double t0, double t1, double first_step, double rtol,
                                   double atol, int64_t max_attempts, marl_stats* stats)
{
    return integrate_rk_dev(kDop853Grid, ctx, y_dev, layout, t0, t1, first_step, rtol, atol, max_attempts, stats);
}

// honours terminal monitors (marl_set_terminal), as marl_integrate_rk45_terminal does
int marl_integrate_dop853_grid(marl_ctx* ctx, double* y, double t0, double t1, double first_step, double rtol, double atol,
                               const double* t_eval, int64_t n_eval, double* y_eval, double* t_events, int64_t max_events,
                               int64_t max_attempts, marl_stats* stats)
{
    return integrate_rk(kDop853Grid, ctx, y, t0, t1, first_step, rtol, atol, t_eval, n_eval, y_eval, t_events, max_events, max_attempts, stats, true);
}

// ---- domain decomposition building blocks --------------------------------------------------------
int marl_ctx_create_slab(const marl_params* params, int64_t N_global, int64_t g_begin, int64_t g_end, int64_t halo, int device,
                         marl_ctx** out)
{
    if (!params || !out || N_global < 2 || g_begin < 0 || g_end > N_global || g_end <= g_begin)
        return fail(nullptr, -1, "marl_ctx_create_slab: invalid argument");
    if (halo < 6) return fail(nullptr, -1, "marl_ctx_create_slab: halo must be >= 6 (one Dormand-Prince attempt consumes 6 cells per side)");
    if (g_end - g_begin < halo) return fail(nullptr, -1, "marl_ctx_create_slab: slab narrower than the halo");
    marl_ctx* ctx = nullptr;
    if (int rc = marl_ctx_create(params, 1, N_global, device, &ctx)) return rc;
    const int64_t hl = g_begin > 0 ? halo : 0, hr = g_end < N_global ? halo : 0, n_own = g_end - g_begin;
    ctx->halo = (int)halo;
    ctx->slab = Slab{hl + n_own + hr, g_begin - hl, hl + n_own + hr, hl, hl + n_own};
    *out = ctx;
    return 0;
}

#define SLAB_OK(ctx, fn)                                                                       \
    if (!(ctx)) return -1;                                                                     \
    if ((ctx)->halo <= 0) return fail(ctx, -1, fn ": not a slab context (marl_ctx_create_slab)"); \
    HIP_OK(ctx, hipSetDevice((ctx)->device));

int marl_slab_load(marl_ctx* ctx, const double* y_owned_dev)
{
    SLAB_OK(ctx, "marl_slab_load")
    if (!y_owned_dev) return fail(ctx, -1, "marl_slab_load: invalid argument");
    const size_t sd = (size_t)NF * ctx->slab.n_buf;
    for (int i = 0; i < 4; i++) {
        if (int rc = ensure(ctx, i, sd)) return rc;
        HIP_OK(ctx, hipMemsetAsync(ctx->buf[i], 0, sd * sizeof(double), ctx->stream));
    }
    const int64_t n_own = ctx->slab.out_hi - ctx->slab.out_lo;
    hipLaunchKernelGGL(slab_copy_kernel, dim3((unsigned)((n_own + 255) / 256)), dim3(256), 0, ctx->stream, ctx->buf[0], ctx->buf[1], ctx->dctrl, 0,
                       ctx->slab, const_cast<double*>(y_owned_dev), 0);
    LAUNCH_OK(ctx);
    return 0;
}

int marl_slab_store(marl_ctx* ctx, double* y_owned_dev)
{
    SLAB_OK(ctx, "marl_slab_store")
    if (!y_owned_dev) return fail(ctx, -1, "marl_slab_store: invalid argument");
    const int64_t n_own = ctx->slab.out_hi - ctx->slab.out_lo;
    hipLaunchKernelGGL(slab_copy_kernel, dim3((unsigned)((n_own + 255) / 256)), dim3(256), 0, ctx->stream, ctx->buf[0], ctx->buf[1], ctx->dctrl, -2,
                       ctx->slab, y_owned_dev, 1);
    LAUNCH_OK(ctx);
    return 0;
}

int marl_slab_pack(marl_ctx* ctx, int which, double* send_lo_dev, double* send_hi_dev)
{
    SLAB_OK(ctx, "marl_slab_pack")
    hipLaunchKernelGGL(slab_pack_kernel, dim3(1), dim3(128), 0, ctx->stream, ctx->buf[0], ctx->buf[1], ctx->buf[2], ctx->buf[3], ctx->dctrl, which,
                       ctx->slab, ctx->halo, send_lo_dev, send_hi_dev);
    LAUNCH_OK(ctx);
    return 0;
}

int marl_slab_unpack(marl_ctx* ctx, int which, const double* recv_lo_dev, const double* recv_hi_dev)
{
    SLAB_OK(ctx, "marl_slab_unpack")
    // a side without a neighbour (physical boundary) has no halo cells: ignore its strip
    const double* lo = ctx->slab.out_lo > 0 ? recv_lo_dev : nullptr;
    const double* hi = ctx->slab.out_hi < ctx->slab.n_buf ? recv_hi_dev : nullptr;
    hipLaunchKernelGGL(slab_unpack_kernel, dim3(1), dim3(128), 0, ctx->stream, ctx->buf[0], ctx->buf[1], ctx->buf[2], ctx->buf[3], ctx->dctrl, which,
                       ctx->slab, ctx->halo, lo, hi);
    LAUNCH_OK(ctx);
    return 0;
}

int marl_slab_rhs0(marl_ctx* ctx)
{
    SLAB_OK(ctx, "marl_slab_rhs0")
    return launch_rhs(ctx, ctx->buf[0], ctx->buf[2], LAYOUT_FIELD_MAJOR);
}

int marl_slab_monitors(marl_ctx* ctx, double* rec_dev)
{
    SLAB_OK(ctx, "marl_slab_monitors")
    if (!rec_dev) rec_dev = ctx->dd_send;   // library-side exchange: straight into this rank's message
    if (!rec_dev) return fail(ctx, -1, "marl_slab_monitors: invalid argument");
    if (int rc = launch_monitors(ctx, ctx->buf[0], LAYOUT_FIELD_MAJOR)) return rc;
    HIP_OK(ctx, hipMemcpyAsync(rec_dev, ctx->rec, sizeof(double) * NQ, hipMemcpyDeviceToDevice, ctx->stream));
    return 0;
}

int marl_slab_init_control(marl_ctx* ctx, const double* recs_dev, int64_t nrec, double t0, double t1, double first_step, double rtol,
                           double atol, int64_t max_attempts)
{
    SLAB_OK(ctx, "marl_slab_init_control")
    NO_TERMINAL(ctx, "marl_slab_init_control")
    if (!recs_dev) recs_dev = ctx->dd_recs;   // library-side exchange: the records gathered by marl_slab_exchange
    if (!recs_dev || nrec < 1) return fail(ctx, -1, "marl_slab_init_control: invalid argument");
    if (!(first_step > 0) || !(t1 >= t0) || (t1 > t0 && first_step > t1 - t0)) return fail(ctx, -1, "rk45: `first_step` must be in (0, t1 - t0]");
    hipLaunchKernelGGL(reduce_records_kernel, dim3(1), dim3(256), 0, ctx->stream, recs_dev, nrec, ctx->rec);
    LAUNCH_OK(ctx);
    hipLaunchKernelGGL(rk45_init_kernel, dim3(1), dim3(1), 0, ctx->stream, ctx->dctrl, ctx->rec, t0, t1, first_step, clamp_rtol(rtol), atol,
                       (int64_t)NF * ctx->N, max_attempts, 0);
    LAUNCH_OK(ctx);
    ctx->dd_max_attempts = max_attempts;
    return 0;
}

int marl_slab_attempt(marl_ctx* ctx, double* rec_dev)
{
    SLAB_OK(ctx, "marl_slab_attempt")
    if (!rec_dev) return fail(ctx, -1, "marl_slab_attempt: invalid argument");
    const int64_t nb = rk45_blocks(ctx);
    if (int rc = ensure_part(ctx, (size_t)std::max<int64_t>(nb + kReduceGroups, 1024))) return rc;
    if (ctx->var_dphi) launch_attempt_t<true>(ctx, nb, LAYOUT_FIELD_MAJOR); else launch_attempt_t<>(ctx, nb, LAYOUT_FIELD_MAJOR);
    LAUNCH_OK(ctx);
    int64_t nrec = nb;
    const double* recs = reduce_first_level(ctx, &nrec);
    LAUNCH_OK(ctx);
    // one record for this rank; harmless (stale partials) when the controller is no longer running: control ignores it
    hipLaunchKernelGGL(reduce_records_kernel, dim3(1), dim3(256), 0, ctx->stream, recs, nrec, rec_dev);
    LAUNCH_OK(ctx);
    return 0;
}

int marl_slab_control(marl_ctx* ctx, const double* recs_dev, int64_t nrec)
{
    SLAB_OK(ctx, "marl_slab_control")
    if (!recs_dev || nrec < 1) return fail(ctx, -1, "marl_slab_control: invalid argument");
    hipLaunchKernelGGL(rk45_control_kernel, dim3(1), dim3(CONTROL_THREADS), 0, ctx->stream, recs_dev, nrec, ctx->dctrl);
    LAUNCH_OK(ctx);
    return 0;
}

int marl_slab_status(marl_ctx* ctx, marl_stats* stats)
{
    SLAB_OK(ctx, "marl_slab_status")
    if (!stats) return fail(ctx, -1, "marl_slab_status: invalid argument");
    HIP_OK(ctx, hipMemcpyAsync(ctx->hctrl, ctx->dctrl, sizeof(Rk45Ctrl), hipMemcpyDeviceToHost, ctx->stream));
    HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
    ctrl_to_stats(*ctx->hctrl, stats);
    return 0;
}

}  // extern "C"
// ---- domain decomposition with the exchange inside the library -------------------------------------------------------------
// The RCCL API is taken from the librccl the process already has (PyTorch-ROCm bundles one; `rccl_path` names it) through
// dlopen - this library does not link RCCL, single-GPU users never load it.
namespace {
constexpr int kNcclDouble = 8;   // ncclFloat64 (rccl.h)
struct NcclId { char internal[128]; };   // ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES 128)

void* open_rccl(const char* path)
{
    void* lib = nullptr;
    if (path && *path) lib = dlopen(path, RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    return lib;
}

inline int dd_msg(const marl_ctx* ctx) { return NQ + 2 * (2 * NF * ctx->halo); }

int dd_buffers(marl_ctx* ctx)
{
    if (ctx->dd_send) return 0;
    const size_t msg = (size_t)dd_msg(ctx);
    HIP_OK(ctx, hipMalloc((void**)&ctx->dd_send, msg * sizeof(double)));
    HIP_OK(ctx, hipMalloc((void**)&ctx->dd_gathered, msg * sizeof(double) * (size_t)ctx->dd_world));
    HIP_OK(ctx, hipMalloc((void**)&ctx->dd_recs, NQ * sizeof(double) * (size_t)ctx->dd_world));
    HIP_OK(ctx, hipMemsetAsync(ctx->dd_send, 0, msg * sizeof(double), ctx->stream));
    return 0;
}

// all-gather of the ranks' messages (one slab: the message itself is the gathered buffer)
int dd_allgather(marl_ctx* ctx, const double** gathered)
{
    if (!ctx->rccl_comm) { *gathered = ctx->dd_send; return 0; }   // one slab, no communicator
    const int rc = ctx->rccl_allgather(ctx->dd_send, ctx->dd_gathered, (size_t)dd_msg(ctx), kNcclDouble, ctx->rccl_comm, ctx->stream);
    if (rc != 0) return fail(ctx, -3, "ncclAllGather failed (ncclResult %d)", rc);
    *gathered = ctx->dd_gathered;
    return 0;
}
}  // namespace

extern "C" {

int marl_slab_comm_probe(const char* rccl_path)
{
    void* lib = open_rccl(rccl_path);
    if (!lib) return fail(nullptr, -2, "marl_slab_comm_probe: cannot load librccl (%s)", dlerror());
    for (const char* sym : {"ncclGetUniqueId", "ncclCommInitRank", "ncclAllGather", "ncclCommDestroy"})
        if (!dlsym(lib, sym)) return fail(nullptr, -2, "marl_slab_comm_probe: %s not found in librccl", sym);
    return 0;
}

int marl_slab_comm_id(const char* rccl_path, char id_out[128])
{
    if (!id_out) return -1;
    void* lib = open_rccl(rccl_path);
    if (!lib) return fail(nullptr, -2, "marl_slab_comm_id: cannot load librccl (%s)", dlerror());
    auto get_id = (int (*)(NcclId*))dlsym(lib, "ncclGetUniqueId");
    if (!get_id) return fail(nullptr, -2, "marl_slab_comm_id: ncclGetUniqueId not found");
    NcclId id;
    const int rc = get_id(&id);
    if (rc != 0) return fail(nullptr, -3, "ncclGetUniqueId failed (ncclResult %d)", rc);
    memcpy(id_out, id.internal, 128);
    return 0;
}

int marl_slab_comm_init(marl_ctx* ctx, const char* rccl_path, const char id[128], int rank, int world)
{
    SLAB_OK(ctx, "marl_slab_comm_init")
    if (world < 1 || rank < 0 || rank >= world) return fail(ctx, -1, "marl_slab_comm_init: invalid rank / world");
    if (ctx->dd_send) return fail(ctx, -1, "marl_slab_comm_init: already initialised");
    ctx->dd_rank = rank;
    ctx->dd_world = world;
    if (world > 1 || id) {   // (world == 1 with an id: a one-rank communicator - exercises the RCCL path on one GPU)
        if (!id) return fail(ctx, -1, "marl_slab_comm_init: a unique id is required for world > 1");
        bool zero = true;
        for (int i = 0; i < 128; i++) zero = zero && id[i] == 0;
        if (zero) return fail(ctx, -1, "marl_slab_comm_init: the unique id is all zero (not made by marl_slab_comm_id / ncclGetUniqueId)");
        ctx->rccl_lib = open_rccl(rccl_path);
        if (!ctx->rccl_lib) return fail(ctx, -2, "marl_slab_comm_init: cannot load librccl (%s)", dlerror());
        auto init_rank = (int (*)(void**, int, NcclId, int))dlsym(ctx->rccl_lib, "ncclCommInitRank");
        ctx->rccl_allgather = (int (*)(const void*, void*, size_t, int, void*, hipStream_t))dlsym(ctx->rccl_lib, "ncclAllGather");
        ctx->rccl_destroy = (int (*)(void*))dlsym(ctx->rccl_lib, "ncclCommDestroy");
        if (!init_rank || !ctx->rccl_allgather || !ctx->rccl_destroy) return fail(ctx, -2, "marl_slab_comm_init: RCCL symbols not found");
        NcclId nid;
        memcpy(nid.internal, id, 128);
        const int rc = init_rank(&ctx->rccl_comm, world, nid, rank);
        if (rc != 0) { ctx->rccl_comm = nullptr; return fail(ctx, -3, "ncclCommInitRank failed (ncclResult %d)", rc); }
    }
    if (world > 1 && !ctx->rccl_comm) return fail(ctx, -1, "marl_slab_comm_init: no communicator for world > 1");
    return dd_buffers(ctx);
}

// pack(which) -> all-gather -> unpack(which); the ranks' records end up in the context (marl_slab_init_control with recs NULL)
int marl_slab_exchange(marl_ctx* ctx, int which)
{
    SLAB_OK(ctx, "marl_slab_exchange")
    if (!ctx->dd_send) return fail(ctx, -1, "marl_slab_exchange: call marl_slab_comm_init first");
    hipLaunchKernelGGL(slab_reduce_pack_kernel, dim3(1), dim3(256), 0, ctx->stream, ctx->buf[0], ctx->buf[1], ctx->buf[2], ctx->buf[3], ctx->dctrl, which,
                       ctx->slab, ctx->halo, ctx->part, (int64_t)0, ctx->dd_send);
    LAUNCH_OK(ctx);
    const double* gathered;
    if (int rc = dd_allgather(ctx, &gathered)) return rc;
    hipLaunchKernelGGL(slab_unpack_control_kernel, dim3(1), dim3(256), 0, ctx->stream, ctx->buf[0], ctx->buf[1], ctx->buf[2], ctx->buf[3], ctx->dctrl, which,
                       ctx->slab, ctx->halo, gathered, ctx->dd_rank, ctx->dd_world, dd_msg(ctx), 0);
    LAUNCH_OK(ctx);
    hipLaunchKernelGGL(slab_records_kernel, dim3(1), dim3(64), 0, ctx->stream, gathered, ctx->dd_world, dd_msg(ctx), ctx->dd_recs);
    LAUNCH_OK(ctx);
    return 0;
}

// The whole adaptive loop of a domain-decomposed run: per attempt  attempt kernel -> reduce + pack -> all-gather -> unpack +
// control, enqueued `poll_interval` attempts at a time; the status is read once per batch (every rank reads the same status:
// all decisions are computed from the same gathered records).  Before: load, exchange(0), rhs0, monitors(NULL), exchange(0),
// init_control(NULL, world, ...).  After: store.
int marl_slab_run(marl_ctx* ctx, marl_stats* stats)
{
    SLAB_OK(ctx, "marl_slab_run")
    NO_TERMINAL(ctx, "marl_slab_run")
    if (!stats) return fail(ctx, -1, "marl_slab_run: invalid argument");
    if (!ctx->dd_send) return fail(ctx, -1, "marl_slab_run: call marl_slab_comm_init first");
    const int64_t nb = rk45_blocks(ctx);
    if (int rc = ensure_part(ctx, (size_t)std::max<int64_t>(nb + kReduceGroups, 1024))) return rc;
    const int msg = dd_msg(ctx);
    int64_t executed = 0;
    if (ctx->dd_world == 1 && !ctx->rccl_comm) {
        // ONE slab and no communicator: nothing is exchanged - the single-grid integrator's loop (same kernels, same bits): the persistent
        // launch up to ~750 000 cells, attempt + reduction + control launches above (one launch less per attempt than packing a message
        // nobody reads and unpacking it again)
        const bool streamed = rk45_use_stream(ctx);
        while (true) {
            if (streamed) {
                if (int rc = launch_rk45_stream(ctx, LAYOUT_FIELD_MAJOR, ctx->rk45_stream_attempts)) return rc;
            } else {
                const int64_t batch = attempts_per_batch(ctx->poll, ctx->dd_max_attempts, executed);
                for (int64_t i = 0; i < batch; i++)
                    if (int rc = launch_attempt(ctx, LAYOUT_FIELD_MAJOR, kRk45)) return rc;
            }
            HIP_OK(ctx, hipMemcpyAsync(ctx->hctrl, ctx->dctrl, sizeof(Rk45Ctrl), hipMemcpyDeviceToHost, ctx->stream));
            HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
            const int64_t before = executed;
            executed = ctx->hctrl->attempts - (ctx->hctrl->status == ST_RUNNING ? 1 : 0);
            if (streamed)
                if (int rc = rk45_stream_account(ctx, executed - before)) return rc;
            if (ctx->hctrl->status != ST_RUNNING) break;
        }
        ctrl_to_stats(*ctx->hctrl, stats);
        return 0;
    }
    // the slab's attempt as ONE launch (rk45_stream_kernel, one attempt, its last workgroup packs the message): two launches + the
    // all-gather per attempt instead of four.  A batch of them is enqueued blindly (attempts after the controller has stopped return
    // at once), so the counters are re-armed by the kernel itself; they must be at zero when the first one starts.
    const bool dd_stream = ctx->dd_stream == 2 || (ctx->dd_stream == 1 && rk45_use_stream(ctx));
    if (dd_stream) {
        if (int rc = rk45_stream_setup(ctx)) return rc;
        if (ctx->rs_arrive_base || ctx->rs_epoch_base || ctx->rs_grab_base)
            if (int rc = rk45_stream_reset(ctx)) return rc;
    }
    while (true) {
        // (every rank computes the same batch size: the budget and the status are the same everywhere)
        const int64_t batch = attempts_per_batch(ctx->poll, ctx->dd_max_attempts, executed);
        for (int64_t i = 0; i < batch; i++) {
            if (dd_stream) {
                if (int rc = launch_rk45_stream(ctx, LAYOUT_FIELD_MAJOR, 1, true)) return rc;
            } else {
                if (ctx->var_dphi) launch_attempt_t<true>(ctx, nb, LAYOUT_FIELD_MAJOR); else launch_attempt_t<>(ctx, nb, LAYOUT_FIELD_MAJOR);
                LAUNCH_OK(ctx);
                int64_t nrec = nb;
                const double* recs = reduce_first_level(ctx, &nrec);
                LAUNCH_OK(ctx);
                hipLaunchKernelGGL(slab_reduce_pack_kernel, dim3(1), dim3(256), 0, ctx->stream, ctx->buf[0], ctx->buf[1], ctx->buf[2], ctx->buf[3], ctx->dctrl, -1,
                                   ctx->slab, ctx->halo, recs, nrec, ctx->dd_send);
                LAUNCH_OK(ctx);
            }
            const double* gathered;
            if (int rc = dd_allgather(ctx, &gathered)) return rc;
            hipLaunchKernelGGL(slab_unpack_control_kernel, dim3(1), dim3(256), 0, ctx->stream, ctx->buf[0], ctx->buf[1], ctx->buf[2], ctx->buf[3], ctx->dctrl,
                               -1, ctx->slab, ctx->halo, gathered, ctx->dd_rank, ctx->dd_world, msg, 1);
            LAUNCH_OK(ctx);
        }
        HIP_OK(ctx, hipMemcpyAsync(ctx->hctrl, ctx->dctrl, sizeof(Rk45Ctrl), hipMemcpyDeviceToHost, ctx->stream));
        HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->hctrl->status != ST_RUNNING) break;
        executed = ctx->hctrl->attempts - 1;
    }
    ctrl_to_stats(*ctx->hctrl, stats);
    return 0;
}

}  // extern "C"

// ==============================================================================================
// Implicit path: scipy's Radau as the reference runs it by default (marlpde/parameters.py:213, jac_sparsity :150-199;
// call site marlpde/Evolve_scenario.py:104-109).  Host = the scalar step logic of scipy/integrate/_ivp/radau.py
// (_step_impl :404-537, solve_collocation_system :47-130, predict_factor :133-173) and of the solve_ivp driver
// (ivp.py:654-723: events with Brent on the dense output, t_eval); device = marl_radau.h.
// ==============================================================================================
namespace {
using radau::cplx;

constexpr int kRadauPartials = 256;   // workgroups of the norm + update kernels on large grids

struct RadauWork {
    double *y, *f, *fnew, *ynew, *err, *yerr, *yold, *scale, *tmp;
    double *Z, *W, *F, *Z0, *Q, *YS;
    double *fac, *h, *yscale, *maxdiff, *scl, *hnew, *Jraw, *YP, *FN;
    double *J, *Dinv_r, *Up_r, *rhs_r, *out, *partial;
    cplx *Dinv_c, *Up_c, *rhs_c;
    int32_t *small, *groups, *flags;
    int ng = 0;
    bool have_factor = false;
    // block parallel cyclic reduction (default linear solver)
    radau::PcrSystem<double> Sr{};
    radau::PcrSystem<cplx> Sc{};
    int nlevels = 0;
    bool pcr = true;
    // cyclic reduction in front of it (marl_radau_cr.h; large grids of single runs): cr_k levels, level l has cr_n[l] rows stored from row
    // cr_off[l]; Sr / Sc / nlevels then describe the COMPACT system of the cr_n[cr_k] rows that are left
    int cr_k = 0;
    int64_t cr_n[radau::CR_MAX_LEVELS + 1] = {}, cr_off[radau::CR_MAX_LEVELS + 2] = {};
    radau::CrSystem<double> Cr{};
    radau::CrSystem<cplx> Cc{};
    radau::CrPlan plan{};   // the same levels for the one-launch solve kernels (plan.k == 0: they run PCR alone)
};

// Zero-copy slots: arm = store the sentinel; wait = poll until the kernel has overwritten it (bounded, then fall back to a synchronise).
constexpr uint64_t kZcSentinel = 0x7ff8dead5eed0001ull;   // a quiet NaN with a payload arithmetic does not produce
inline void zc_arm(marl_ctx* ctx, int slot, int count = 1)
{
    for (int i = 0; i < count; i++) reinterpret_cast<volatile uint64_t*>(ctx->zc_h)[slot + i] = kZcSentinel;
}
// the mapped, coherent host words ctx->zc_h / zc_d, allocated on first use (they live as long as the context)
int zc_ensure(marl_ctx* ctx)
{
    if (ctx->zc_h) return 0;
    HIP_OK(ctx, hipHostMalloc((void**)&ctx->zc_h, 32 * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent));
    HIP_OK(ctx, hipHostGetDevicePointer((void**)&ctx->zc_d, ctx->zc_h, 0));
    return 0;
}
// poll until arrived() holds; after 2^28 spins (~seconds: something is wrong with the stream) let the runtime say what, and look once more
template <class Arrived>
int zc_spin(marl_ctx* ctx, Arrived&& arrived, const char* never)
{
    for (int64_t spins = 0; !arrived();) {
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
        if (++spins > (int64_t)1 << 28) {
            HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
            if (!arrived()) return fail(ctx, -3, "%s", never);
        }
    }
    return 0;
}
inline int zc_wait(marl_ctx* ctx, int slot, int count = 1)
{
    volatile uint64_t* p = reinterpret_cast<volatile uint64_t*>(ctx->zc_h);
    for (int i = 0; i < count; i++)
        if (int rc = zc_spin(ctx, [&] { return p[slot + i] != kZcSentinel; }, "implicit driver: a result word was never written")) return rc;
    return 0;
}

// `instances` > 1: one arena per instance, all with the layout of instance 0 (`w`), `*zstride` bytes apart
int radau_alloc(marl_ctx* ctx, RadauWork& w, const int32_t* groups_host, int64_t instances = 1, int64_t* zstride = nullptr)
{
    const int64_t N = ctx->N, n = NF * N;
    std::vector<int32_t> g(n);
    if (groups_host) g.assign(groups_host, groups_host + n);
    else for (int64_t j = 0; j < n; j++) g[j] = (int32_t)(3 * (j / N) + (j % N) % 3);   // structured colouring: 15 groups
    int ng = 0;
    for (int64_t j = 0; j < n; j++) {
        if (g[j] < 0 || g[j] > 4096) return fail(ctx, -1, "radau: invalid column group %d", (int)g[j]);
        ng = std::max(ng, g[j] + 1);
    }
    // a valid grouping never puts two columns that share a pattern row (same cell neighbourhood) into one group
    for (int64_t j = 0; j < n; j++) {
        const int64_t ip = j % N;
        for (int fp = 0; fp < NF; fp++)
            for (int64_t i2 = std::max<int64_t>(0, ip - 2); i2 <= std::min<int64_t>(N - 1, ip + 2); i2++) {
                const int64_t j2 = fp * N + i2;
                if (j2 != j && g[j2] == g[j]) return fail(ctx, -1, "radau: columns %lld and %lld share rows but are in one group", (long long)j, (long long)j2);
            }
    }
    // cyclic-reduction levels in front of PCR (single runs with the PCR solver only)
    w.cr_k = 0;
    w.cr_n[0] = N; w.cr_off[0] = 0;
    // Small grids whose solves run in one workgroup (5 N <= PCR_FUSED_MAX, single runs and sweeps): radau_cr_small levels (default 3) -
    // the chain of levels in one workgroup is bound by the factor bytes that pass through one compute unit, and cyclic reduction
    // in front of PCR cuts them 2.4 - 2.8 times (marl_radau.h, crpcr_solve_all).  The all-in-workgroup sweep mode keeps plain PCR.
    // By default only from radau_cr_small_min_n = 205 cells (two unknowns per thread of the chain): on the reference's N = 200 grid
    // plain PCR is what takes every decision scipy takes in single runs AND sweeps (with 1 - 3 levels in front, one knife-edge Newton
    // test or another falls the other way in one of the pinned cases - profiles/r03_lab_radau_wg.log); set radau_cr_small_min_n = 32
    // for throughput there (4096 scenarios: 1.58 -> 1.17 s).
    const bool one_wg = n <= radau::PCR_FUSED_MAX && N >= 32 && (instances == 1 || ctx->radau_fused_solve);   // (single runs with radau_fused_solve = 0: the same levels, one launch each)
    const bool small_cr = one_wg && ctx->radau_cr < 0 && ctx->radau_cr_small > 0 && N >= ctx->radau_cr_small_min_n && !(instances > 1 && ctx->radau_sweep_wg == 2);
    const bool large_cr = instances == 1 && ctx->radau_cr != 0 && (ctx->radau_cr > 0 || N >= ctx->radau_cr_min_n);
    if (ctx->radau_solver == 0 && (small_cr || large_cr)) {
        const int64_t want = small_cr ? ctx->radau_cr_small : ctx->radau_cr;
        int k = 0;
        while (k < radau::CR_MAX_LEVELS && w.cr_n[k] / 2 >= 2 && (want > 0 ? k < want : NF * w.cr_n[k] > radau::PCR_FUSED_THREADS)) {
            w.cr_n[k + 1] = w.cr_n[k] / 2;
            w.cr_off[k + 1] = w.cr_off[k] + w.cr_n[k];
            k++;
        }
        w.cr_k = k;
    }
    // the levels as the one-launch solve kernels take them (k <= CR_WG_MAX_LEVELS; else they are not used)
    w.plan = radau::CrPlan{};
    if (w.cr_k > 0 && w.cr_k <= radau::CR_WG_MAX_LEVELS && n <= radau::PCR_FUSED_MAX) {
        w.plan.k = w.cr_k;
        for (int l = 0; l <= w.cr_k; l++) { w.plan.n[l] = w.cr_n[l]; w.plan.off[l] = w.cr_off[l]; }
    }
    const int64_t M = w.cr_n[w.cr_k];                                      // rows of the system PCR works on
    const int64_t cr_rows = w.cr_k ? w.cr_off[w.cr_k] + M : 0;             // rows of all levels together (< 2 N)
    int nlev = 0;
    while (((int64_t)1 << nlev) < M) nlev++;
    const size_t pcr_real = (size_t)M * 25 * (8 + 2 * (size_t)nlev) + 2 * (size_t)NF * M;   // L, D, U, Dinv ping-pong; alpha, gamma per level; b ping-pong
    const size_t cr_real = (size_t)cr_rows * (8 * 25 + NF);                             // L, D, U, Dinv, P, Q, alpha, gamma; b
    const size_t doubles = (size_t)n * (9 + 6 * 3 + 6 + 15 + 2 * (size_t)ng + 15 + 10 + 20 + 1 + 2) + 64 + kRadauPartials + (size_t)n + 3 * pcr_real + 3 * cr_real;
    const size_t per = (doubles + 1) & ~(size_t)1;   // 16-byte multiples: complex members stay aligned in every instance
    if (zstride) *zstride = (int64_t)(per * sizeof(double));
    if (ctx->rd_cap < per * (size_t)instances) {
        if (ctx->rd_arena) HIP_OK(ctx, hipFree(ctx->rd_arena));
        ctx->rd_arena = nullptr; ctx->rd_cap = 0;
        HIP_OK(ctx, hipMalloc((void**)&ctx->rd_arena, per * (size_t)instances * sizeof(double)));
        ctx->rd_cap = per * (size_t)instances;
    }
    if (!ctx->rd_host) HIP_OK(ctx, hipHostMalloc((void**)&ctx->rd_host, 16 * sizeof(double), hipHostMallocDefault));
    double* p = ctx->rd_arena;
    auto take = [&](size_t k) { double* r = p; p += k; return r; };
    w.y = take(n); w.f = take(n); w.fnew = take(n); w.ynew = take(n); w.err = take(n); w.yerr = take(n); w.yold = take(n); w.scale = take(n); w.tmp = take(n);
    w.Z = take(3 * n); w.W = take(3 * n); w.F = take(3 * n); w.Z0 = take(3 * n); w.Q = take(3 * n); w.YS = take(3 * n);
    w.fac = take(n); w.h = take(n); w.yscale = take(n); w.maxdiff = take(n); w.scl = take(n); w.hnew = take(n); w.Jraw = take(15 * n);
    w.YP = take((size_t)ng * n); w.FN = take((size_t)ng * n);
    w.J = take(15 * n); w.Dinv_r = take(5 * n); w.Up_r = take(5 * n);
    w.Dinv_c = (cplx*)take(10 * n); w.Up_c = (cplx*)take(10 * n);
    w.rhs_r = take(n); w.rhs_c = (cplx*)take(2 * n); w.out = take(8); w.partial = take(kRadauPartials);
    w.small = (int32_t*)take((n + 1) / 2 + 1); w.groups = (int32_t*)take((n + 1) / 2 + 1); w.flags = (int32_t*)take(2);
    ctx->zc_on = false;
    if (instances == 1 && ctx->implicit_zero_copy) {
        if (int rc = zc_ensure(ctx)) return rc;
        HIP_OK(ctx, hipStreamSynchronize(ctx->stream));   // nothing of an earlier run may still write the words
        memset(ctx->zc_h, 0, 32 * sizeof(double));
        zc_arm(ctx, 0);
        w.out = ctx->zc_d;
        w.flags = reinterpret_cast<int32_t*>(ctx->zc_d + 1);
        ctx->zc_on = true;
    }
    w.ng = ng;
    w.nlevels = nlev;
    w.pcr = ctx->radau_solver == 0;
    for (int k = 0; k < 2; k++) {
        w.Sr.L[k] = take(25 * M); w.Sr.D[k] = take(25 * M); w.Sr.U[k] = take(25 * M); w.Sr.Dinv[k] = take(25 * M); w.Sr.b[k] = take(NF * M);
        w.Sc.L[k] = (cplx*)take(50 * M); w.Sc.D[k] = (cplx*)take(50 * M); w.Sc.U[k] = (cplx*)take(50 * M); w.Sc.Dinv[k] = (cplx*)take(50 * M);
        w.Sc.b[k] = (cplx*)take(2 * NF * M);
    }
    w.Sr.alpha = take((size_t)nlev * 25 * M); w.Sr.gamma = take((size_t)nlev * 25 * M);
    w.Sc.alpha = (cplx*)take((size_t)nlev * 50 * M); w.Sc.gamma = (cplx*)take((size_t)nlev * 50 * M);
    if (w.cr_k) {
        const size_t R = (size_t)cr_rows;
        double** pr[8] = {&w.Cr.L, &w.Cr.D, &w.Cr.U, &w.Cr.Dinv, &w.Cr.P, &w.Cr.Q, &w.Cr.alpha, &w.Cr.gamma};
        cplx** pc[8] = {&w.Cc.L, &w.Cc.D, &w.Cc.U, &w.Cc.Dinv, &w.Cc.P, &w.Cc.Q, &w.Cc.alpha, &w.Cc.gamma};
        for (int a = 0; a < 8; a++) { *pr[a] = take(25 * R); *pc[a] = (cplx*)take(50 * R); }
        w.Cr.b = take(NF * R); w.Cc.b = (cplx*)take(2 * NF * R);
    }
    if (instances > 1) HIP_OK(ctx, hipMemsetAsync(ctx->rd_arena, 0, per * (size_t)instances * sizeof(double), ctx->stream));
    else HIP_OK(ctx, hipMemsetAsync(w.J, 0, sizeof(double) * 15 * n, ctx->stream));
    HIP_OK(ctx, hipMemcpyAsync(w.groups, g.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, ctx->stream));   // (one copy serves every instance)
    HIP_OK(ctx, hipStreamSynchronize(ctx->stream));   // g dies with this frame
    return 0;
}

// workgroups of the norm kernels: one up to 8192 unknowns, then one per 4096, at most kRadauPartials
inline int radau_norm_blocks(int64_t n) { return n <= 8192 ? 1 : (int)std::min<int64_t>(256, (n + 4095) / 4096); }

inline unsigned pcr_groups(int64_t rows) { return (unsigned)((rows + radau::PCR_CELLS_PER_BLOCK - 1) / radau::PCR_CELLS_PER_BLOCK); }

// factorise  mu I - jscale J  for the real system (systems = 1) or the real and the complex one (2): block PCR over all N rows
// (1 + ceil(log2 N) launches), or - large grids of single runs - cr_k levels of cyclic reduction and PCR over the rows that are left
// The `cnt` instances of `zb` (a sweep's work list; their mu then comes from their controllers) or, by default, the single run's arena.
int pcr_factor_launch(marl_ctx* ctx, RadauWork& w, double mu_r, cplx mu_c, double jscale, int systems, unsigned cnt = 1, const ZBatch& zb = kNoBatch)
{
    const int64_t N = ctx->N;
    if (!w.cr_k) {
        const dim3 grid(pcr_groups(N), systems, cnt);
        for (int level = -1; level < w.nlevels; level++) {
            hipLaunchKernelGGL(radau::pcr_factor_kernel, grid, dim3(256), 0, ctx->stream, w.J, N, level, mu_r, mu_c, w.Sr, w.Sc, zb, jscale);
            LAUNCH_OK(ctx);
        }
        return 0;
    }
    hipLaunchKernelGGL(radau::cr_init_kernel, dim3(pcr_groups((N + 1) / 2), systems, cnt), dim3(256), 0, ctx->stream, w.J, N, mu_r, mu_c, jscale, w.Cr, w.Cc, zb);
    LAUNCH_OK(ctx);
    for (int l = 0; l < w.cr_k; l++) {
        const radau::CrShape sh{w.cr_n[l], w.cr_off[l], w.cr_n[l + 1], w.cr_off[l + 1]};
        hipLaunchKernelGGL(radau::cr_reduce_kernel, dim3(pcr_groups(sh.n_next), systems, cnt), dim3(256), 0, ctx->stream, mu_r, mu_c, w.Cr, w.Cc, sh,
                           l + 1 == w.cr_k ? 1 : 0, w.Sr, w.Sc, zb);
        LAUNCH_OK(ctx);
    }
    const int64_t M = w.cr_n[w.cr_k];
    for (int level = 0; level < w.nlevels; level++) {   // (level -1 - blocks from J and their inverses - is what the last reduction left in set 0)
        hipLaunchKernelGGL(radau::pcr_factor_kernel, dim3(pcr_groups(M), systems, cnt), dim3(256), 0, ctx->stream, w.J, M, level, mu_r, mu_c, w.Sr, w.Sc, zb, jscale);
        LAUNCH_OK(ctx);
    }
    return 0;
}

// PCR solve of M rows, in place in x_r (and, with `both`, x_c).  One launch where the system fits a workgroup - with `plan` (k > 0: M = N
// rows) that launch also runs the reduction levels in front of PCR and the back-substitution (crpcr_solve_all); plan.k == 0: PCR alone,
// and the kernel reads neither the plan's levels nor w.Cr / w.Cc.
int pcr_solve_launch(marl_ctx* ctx, RadauWork& w, int64_t M, bool both, double* x_r, cplx* x_c, const radau::CrPlan& plan, unsigned cnt = 1,
                     const ZBatch& zb = kNoBatch)
{
    const int64_t n = NF * M;
    if (n <= radau::PCR_FUSED_MAX && ctx->radau_fused_solve) {   // small systems: every level in one launch
        hipLaunchKernelGGL(radau::pcr_solve_fused_kernel, dim3(1, both ? 2 : 1, cnt), dim3(radau::PCR_FUSED_THREADS), 0, ctx->stream, M, w.nlevels, 0, w.Sr, w.Sc,
                           x_r, x_r, x_c, x_c, zb, plan, w.Cr, w.Cc);
        LAUNCH_OK(ctx);
        return 0;
    }
    const dim3 grid(blocks256(n), both ? 2 : 1, cnt);
    // ping-pong: x -> b[0] -> b[1] -> ... ; the last launch (x = D^-1 b) writes back into x
    const double* in_r = x_r;
    const cplx* in_c = x_c;
    for (int level = 0; level <= w.nlevels; level++) {
        double* out_r = (level == w.nlevels) ? x_r : w.Sr.b[level & 1];
        cplx* out_c = (level == w.nlevels) ? x_c : w.Sc.b[level & 1];
        hipLaunchKernelGGL(radau::pcr_solve_kernel, grid, dim3(256), 0, ctx->stream, M, level, w.nlevels, 0, w.Sr, w.Sc, in_r, out_r, in_c, out_c, zb);
        LAUNCH_OK(ctx);
        in_r = out_r;
        in_c = out_c;
    }
    return 0;
}

// factorise  mu_r I - J  and  mu_c I - J  (block PCR: 1 + ceil(log2 N) launches; or sequential block Thomas: 1 launch)
int radau_factor(marl_ctx* ctx, RadauWork& w, double mu_r, cplx mu_c)
{
#ifdef MARL_LAB_BLOCK_THOMAS
    const int64_t N = ctx->N;
    if (!w.pcr) {
        hipLaunchKernelGGL(radau::factor_kernel, dim3(2), dim3(64), 0, ctx->stream, w.J, N, mu_r, mu_c, w.Dinv_r, w.Up_r, w.Dinv_c, w.Up_c);
        LAUNCH_OK(ctx);
        return 0;
    }
#endif
    return pcr_factor_launch(ctx, w, mu_r, mu_c, 1.0, 2);
}

// solve in place: w.rhs_r (and, with `both`, w.rhs_c), cell-major; of the single run, or of the `cnt` instances of `zb`
int radau_solve(marl_ctx* ctx, RadauWork& w, bool both, unsigned cnt = 1, const ZBatch& zb = kNoBatch)
{
    const int64_t N = ctx->N;
#ifdef MARL_LAB_BLOCK_THOMAS
    if (!w.pcr && cnt == 1 && !zb.zstride) {
        hipLaunchKernelGGL(radau::solve_kernel, dim3(both ? 2 : 1), dim3(64), 0, ctx->stream, w.J, N, w.Dinv_r, w.Up_r, w.Dinv_c, w.Up_c, w.rhs_r, w.rhs_c,
                           both ? 3 : 1);
        LAUNCH_OK(ctx);
        return 0;
    }
#endif
    // plain PCR, or - small grids - reduction levels, compact PCR and back-substitution in one launch.  A sweep only ever gets here:
    // radau_alloc gives it reduction levels only with the one-workgroup solve (small_cr needs one_wg, which for instances > 1 needs
    // radau_fused_solve, and at most CR_WG_MAX_LEVELS of them: marl_set_option), and large_cr needs instances == 1.
    if (!w.cr_k || (w.plan.k && ctx->radau_fused_solve)) return pcr_solve_launch(ctx, w, N, both, w.rhs_r, w.rhs_c, w.plan, cnt, zb);
    if (cnt != 1 || zb.zstride) return fail(ctx, -3, "radau_solve: the level-by-level cyclic-reduction solve is for single runs");
    // right-hand sides down the reduction levels, the compact system by PCR, solutions back up (in place from level to level); from the
    // first level of at most CR_TAIL_ROWS rows on, all remaining levels in one launch each way (option radau_cr_tail = 0: level by level)
    const unsigned gy = both ? 2 : 1;
    int tail0 = w.cr_k;
    if (ctx->radau_cr_tail) {
        while (tail0 > 0 && w.cr_n[tail0 - 1] <= radau::CR_TAIL_ROWS && w.cr_k - (tail0 - 1) <= radau::CR_TAIL_MAX_LEVELS) tail0--;
    }
    const int tailJ = w.cr_k - tail0;
    radau::CrTail tail{};
    tail.l0 = tail0;
    for (int j = 0; j <= tailJ; j++) { tail.n[j] = w.cr_n[tail0 + j]; tail.off[j] = w.cr_off[tail0 + j]; }
    for (int l = 0; l < tail0; l++) {
        const radau::CrShape sh{w.cr_n[l], w.cr_off[l], w.cr_n[l + 1], w.cr_off[l + 1]};
        hipLaunchKernelGGL(radau::cr_rhs_kernel, dim3(blocks256(NF * sh.n_next), gy), dim3(256), 0, ctx->stream, w.Cr, w.Cc, sh, l, w.rhs_r, w.rhs_c);
        LAUNCH_OK(ctx);
    }
#define MARL_TAIL(KERNEL, BLOCKS)                                                                                                               \
    switch (tailJ) {                                                                                                                            \
        case 1: hipLaunchKernelGGL(radau::KERNEL<1>, dim3(BLOCKS, gy), dim3(radau::CR_TAIL_THREADS), 0, ctx->stream, w.Cr, w.Cc, tail, w.rhs_r, w.rhs_c); break; \
        case 2: hipLaunchKernelGGL(radau::KERNEL<2>, dim3(BLOCKS, gy), dim3(radau::CR_TAIL_THREADS), 0, ctx->stream, w.Cr, w.Cc, tail, w.rhs_r, w.rhs_c); break; \
        case 3: hipLaunchKernelGGL(radau::KERNEL<3>, dim3(BLOCKS, gy), dim3(radau::CR_TAIL_THREADS), 0, ctx->stream, w.Cr, w.Cc, tail, w.rhs_r, w.rhs_c); break; \
        case 4: hipLaunchKernelGGL(radau::KERNEL<4>, dim3(BLOCKS, gy), dim3(radau::CR_TAIL_THREADS), 0, ctx->stream, w.Cr, w.Cc, tail, w.rhs_r, w.rhs_c); break; \
        case 5: hipLaunchKernelGGL(radau::KERNEL<5>, dim3(BLOCKS, gy), dim3(radau::CR_TAIL_THREADS), 0, ctx->stream, w.Cr, w.Cc, tail, w.rhs_r, w.rhs_c); break; \
        default: hipLaunchKernelGGL(radau::KERNEL<6>, dim3(BLOCKS, gy), dim3(radau::CR_TAIL_THREADS), 0, ctx->stream, w.Cr, w.Cc, tail, w.rhs_r, w.rhs_c); break; \
    }                                                                                                                                           \
    LAUNCH_OK(ctx);
    if (tailJ > 0) {
        const unsigned nb = (unsigned)((tail.n[tailJ] + radau::CR_TAIL_TOP - 1) / radau::CR_TAIL_TOP);
        MARL_TAIL(cr_rhs_tail_kernel, nb)
    }
    const int64_t offk = w.cr_off[w.cr_k];
    if (int rc = pcr_solve_launch(ctx, w, w.cr_n[w.cr_k], both, w.Cr.b + offk * NF, w.Cc.b + offk * NF, radau::CrPlan{})) return rc;
    if (tailJ > 0) {
        const int64_t rows = (int64_t)radau::CR_TAIL_TOP << tailJ;
        const unsigned nb = (unsigned)((tail.n[0] + rows - 1) / rows);
        MARL_TAIL(cr_back_tail_kernel, nb)
    }
#undef MARL_TAIL
    for (int l = tail0 - 1; l >= 0; l--) {
        const radau::CrShape sh{w.cr_n[l], w.cr_off[l], w.cr_n[l + 1], w.cr_off[l + 1]};
        hipLaunchKernelGGL(radau::cr_back_kernel, dim3((unsigned)((sh.n_cur + radau::CR_ROWS_PER_BLOCK - 1) / radau::CR_ROWS_PER_BLOCK), gy),
                           dim3(radau::CR_ROWS_PER_BLOCK * NF), 0, ctx->stream, w.Cr, w.Cc, sh, l, w.rhs_r, w.rhs_c);
        LAUNCH_OK(ctx);
    }
    return 0;
}

// J = finite-difference Jacobian at (y, f0)  (num_jac; njev is the caller's), of the single run or of the `cnt` instances of `zb`.
// first: no step-size factors yet (a list with an action word - the Radau sweep's - takes that from each instance's controller)
int radau_num_jac(marl_ctx* ctx, RadauWork& w, const double* y, const double* f0, double threshold, int first, unsigned cnt = 1,
                  const ZBatch& zb = kNoBatch)
{
    const int64_t N = ctx->N, n = NF * N;
    const dim3 grid(blocks256(n), 1, cnt);
    hipLaunchKernelGGL(radau::fd_prepare_kernel, grid, dim3(256), 0, ctx->stream, y, f0, w.fac, threshold, first, w.groups, w.ng, n, w.h, w.yscale, w.YP, zb);
    LAUNCH_OK(ctx);
    if (int rc = launch_rhs_fm(ctx, w.YP, w.FN, w.ng, cnt, zb)) return rc;
    hipLaunchKernelGGL(radau::fd_columns_kernel, grid, dim3(256), 0, ctx->stream, y, f0, w.FN, w.groups, w.ng, N, w.fac, w.yscale, w.Jraw, w.maxdiff, w.scl,
                       w.small, w.hnew, w.YP, zb);
    LAUNCH_OK(ctx);
    // second trial step of the columns whose difference drowned in rounding (all groups in one launch; the columns that
    // were fine are perturbed by 0 - scipy evaluates only the groups that need it, with the same numbers)
    if (int rc = launch_rhs_fm(ctx, w.YP, w.FN, w.ng, cnt, zb)) return rc;
    hipLaunchKernelGGL(radau::fd_finish_kernel, grid, dim3(256), 0, ctx->stream, f0, w.FN, w.groups, N, w.fac, w.h, w.maxdiff, w.scl, w.small, w.hnew, w.Jraw,
                       w.J, zb);
    LAUNCH_OK(ctx);
    return 0;
}
// ... of a single run, which keeps "first" itself
int radau_num_jac_run(marl_ctx* ctx, RadauWork& w, const double* y, const double* f0, double threshold)
{
    const int first = w.have_factor ? 0 : 1;
    w.have_factor = true;
    return radau_num_jac(ctx, w, y, f0, threshold, first);
}

// err = the solved right-hand side; sum (err / scale)^2 -> w.out[0]
int radau_error_norm(marl_ctx* ctx, RadauWork& w, double rtol, double atol)
{
    const int64_t N = ctx->N;
    const int nbk = radau_norm_blocks(NF * N);
    hipLaunchKernelGGL(radau::error_norm_kernel, dim3(nbk), dim3(1024), 0, ctx->stream, w.rhs_r, w.y, w.ynew, N, rtol, atol, w.err, w.yerr,
                       nbk > 1 ? w.partial : w.out);
    LAUNCH_OK(ctx);
    if (nbk > 1) {
        hipLaunchKernelGGL(radau::sum_partials_kernel, dim3(1), dim3(1), 0, ctx->stream, w.partial, nbk, w.out);
        LAUNCH_OK(ctx);
    }
    return 0;
}

// read back w.out[0] (a sum of squares) and the non-finite flag; resets the flag
int radau_read(marl_ctx* ctx, RadauWork& w, double* sumsq, int* flag)
{
    if (ctx->zc_on) {
        if (int rc = zc_wait(ctx, 0)) return rc;
        *sumsq = const_cast<const volatile double*>(ctx->zc_h)[0];
        volatile int32_t* fl = reinterpret_cast<volatile int32_t*>(ctx->zc_h + 1);
        if (flag) *flag = *fl;
        if (*fl) *fl = 0;     // (every kernel that could set it has completed: the word that was waited for is written after them)
        zc_arm(ctx, 0);       // for the next producer
        return 0;
    }
    HIP_OK(ctx, hipMemcpyAsync(ctx->rd_host, w.out, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_OK(ctx, hipMemcpyAsync(ctx->rd_host + 1, w.flags, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
    *sumsq = ctx->rd_host[0];
    int32_t fl;
    memcpy(&fl, ctx->rd_host + 1, sizeof fl);
    if (flag) *flag = fl;
    if (fl) HIP_OK(ctx, hipMemsetAsync(w.flags, 0, sizeof(int32_t), ctx->stream));
    return 0;
}

int radau_monitors(marl_ctx* ctx, const double* y, double g[7])
{
    if (ctx->zc_on) {
        zc_arm(ctx, 8, NQ);
        if (int rc = launch_monitors(ctx, y, LAYOUT_FIELD_MAJOR, ctx->zc_d + 8)) return rc;
        if (int rc = zc_wait(ctx, 8, NQ)) return rc;
        double r[NQ];
        for (int j = 0; j < NQ; j++) r[j] = const_cast<const volatile double*>(ctx->zc_h)[8 + j];
        record_to_events(r, g);
        return 0;
    }
    if (int rc = launch_monitors(ctx, y, LAYOUT_FIELD_MAJOR)) return rc;
    HIP_OK(ctx, hipMemcpyAsync(ctx->hrec, ctx->rec, sizeof(double) * NQ, hipMemcpyDeviceToHost, ctx->stream));
    HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
    record_to_events(ctx->hrec, g);
    return 0;
}

// The tail of an accepted step in the solve_ivp loop of the implicit single runs: events (ivp.py:673-694), their roots by Brent's
// method on the step's dense output (solve_event_equation, ivp.py:51-76), and the t_eval samples (ivp.py:706-723).  g: the monitors at
// t_old, on return g_new, those at t; dense(tq, out): the state of the step's dense output at tq -> out (device).
// Terminal monitors (ctx->terminal, marl_terminal.h): in a step where an active monitor meets its limit the roots of all active monitors
// are located, terminal_select says which of them happened, and *t_stop < +inf on return is where the run ends: the samples stop there,
// and the caller writes dense(*t_stop) into its state.  Every other step: *t_stop = +inf, and exactly what happened without limits.
template <class Dense>
int accepted_step_epilogue(marl_ctx* ctx, RadauWork& w, double g[7], const double g_new[7], double t_old, double t, Dense&& dense,
                           const double* t_eval, int64_t n_eval, int64_t& eval_i, double* y_eval_host, double* t_events, int64_t max_events,
                           marl_stats* st, double* t_stop)
{
    const int64_t n = NF * ctx->N;
    auto locate = [&](int e, double* root) -> int {
        auto monitor_at = [&](double tq, double* v) -> int {
            double gq[7];
            if (int rc = dense(tq, w.tmp)) return rc;
            if (int rc = radau_monitors(ctx, w.tmp, gq)) return rc;
            *v = gq[e];
            return 0;
        };
        double fa, fb;
        if (int rc = monitor_at(t_old, &fa)) return rc;
        if (int rc = monitor_at(t, &fb)) return rc;
        return brent_root(monitor_at, t_old, fa, t, fb, root);
    };
    *t_stop = INFINITY;
    uint32_t active = 0;
    bool met = false;
    for (int e = 0; e < 7; e++) {
        const bool up = g[e] <= 0 && g_new[e] >= 0, down = g[e] >= 0 && g_new[e] <= 0;
        if (up || down) {
            active |= 1u << e;
            if (terminal_met(st->n_events[e] + 1, ctx->terminal[e])) met = true;
        }
        g[e] = g_new[e];
    }
    if (met) {
        double roots[7] = {0, 0, 0, 0, 0, 0, 0};
        int64_t counts[7];
        for (int e = 0; e < 7; e++) {
            counts[e] = st->n_events[e] + 1;
            if ((active >> e) & 1)
                if (int rc = locate(e, &roots[e])) return rc;
        }
        uint32_t keep = 0;
        terminal_select(active, roots, counts, ctx->terminal, &keep, t_stop);
        for (int e = 0; e < 7; e++) {
            if (!((keep >> e) & 1)) continue;
            if (t_events && st->n_events[e] < max_events) t_events[e * max_events + st->n_events[e]] = roots[e];
            st->n_events[e]++;
        }
        t = *t_stop;
    } else
        for (int e = 0; e < 7; e++) {
            if (!((active >> e) & 1)) continue;
            if (t_events && st->n_events[e] < max_events) {
                double root;
                if (int rc = locate(e, &root)) return rc;
                t_events[e * max_events + st->n_events[e]] = root;
            }
            st->n_events[e]++;
        }
    while (t_eval && eval_i < n_eval && t_eval[eval_i] <= t) {
        if (int rc = dense(t_eval[eval_i], w.tmp)) return rc;
        HIP_OK(ctx, hipMemcpyAsync(y_eval_host + eval_i * n, w.tmp, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
        HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
        eval_i++;
    }
    return 0;
}

struct RadauDense { double t_old, h; };

// state of the dense output at time t -> out (device)
int radau_dense(marl_ctx* ctx, RadauWork& w, const RadauDense& d, double t, double* out)
{
    radau::X3 X = {{(t - d.t_old) / d.h, 0, 0}};
    const int64_t n = NF * ctx->N;
    hipLaunchKernelGGL(radau::dense_eval_kernel, dim3(blocks256(n)), dim3(256), 0, ctx->stream, w.Q, w.yold, (const double*)nullptr, n, X, 1, out);
    LAUNCH_OK(ctx);
    return 0;
}

double radau_predict_factor(double h_abs, double h_abs_old, double error_norm, double error_norm_old)   // radau.py:133-173; < 0 = None
{
    double multiplier;
    if (error_norm_old < 0 || h_abs_old < 0 || error_norm == 0) multiplier = 1;
    else multiplier = h_abs / h_abs_old * std::pow(error_norm_old / error_norm, 0.25);
    return (multiplier < 1 ? multiplier : 1) * std::pow(error_norm, -0.25);
}

// y0 in w.y (device, field-major).  y_eval_host: n_eval x 5N (host).  On return w.y holds the state at stats->t.
int radau_run(marl_ctx* ctx, RadauWork& w, double t0, double t1, double first_step, double rtol, double atol, const double* t_eval,
              int64_t n_eval, double* y_eval_host, double* t_events, int64_t max_events, int64_t max_attempts, marl_stats* st)
{
    const int64_t N = ctx->N, n = NF * N;
    const double S6 = std::sqrt(6.0);
    const double C3[3] = {(4 - S6) / 10, (4 + S6) / 10, 1};
    const double E3[3] = {(-13 - 7 * S6) / 3, (-13 + 7 * S6) / 3, -1.0 / 3};
    const double MU_REAL = 3 + std::pow(3, 2.0 / 3) - std::pow(3, 1.0 / 3);
    const cplx MU_COMPLEX = {3 + 0.5 * (std::pow(3, 1.0 / 3) - std::pow(3, 2.0 / 3)), -0.5 * (std::pow(3, 5.0 / 6) + std::pow(3, 7.0 / 6))};
    const radau::P33 P = {{{13.0 / 3 + 7 * S6 / 3, -23.0 / 3 - 22 * S6 / 3, 10.0 / 3 + 5 * S6},
                           {13.0 / 3 - 7 * S6 / 3, -23.0 / 3 + 22 * S6 / 3, 10.0 / 3 - 5 * S6},
                           {1.0 / 3, -8.0 / 3, 10.0 / 3}}};
    constexpr int NEWTON_MAXITER = 6;
    constexpr double MIN_FACTOR = 0.2, MAX_FACTOR = 10;
    memset(st, 0, sizeof *st);
    rtol = clamp_rtol(rtol);
    const dim3 gn(blocks256(n)), b256(256);

    // Radau.__init__ (radau.py:290-343)
    double t = t0;
    if (int rc = launch_rhs(ctx, w.y, w.f, LAYOUT_FIELD_MAJOR)) return rc;
    st->nfev = 1;
    double S_h_abs = first_step, S_h_abs_old = -1, S_err_old = -1;
    const double newton_tol = std::fmax(10 * radau::EPS / rtol, std::fmin(0.03, std::sqrt(rtol)));
    if (!ctx->zc_on) HIP_OK(ctx, hipMemsetAsync(w.flags, 0, sizeof(int32_t) * 2, ctx->stream));
    if (int rc = radau_num_jac_run(ctx, w, w.y, w.f, atol)) return rc;
    st->njev = 1;
    bool current_jac = true, have_lu = false, have_sol = false;
    RadauDense dense = {t0, 0};
    double g[7], g_new[7];
    if (int rc = radau_monitors(ctx, w.y, g)) return rc;   // ivp.py:645
    int64_t eval_i = 0, attempts = 0;
    int status = 1;   // (running; what a run returns with status 1 is `stopped`)
    bool stopped = false;

    while (status == 1) {
        if (t == t1) { status = 0; break; }
        const double min_step = 10 * std::fabs(std::nextafter(t, INFINITY) - t);
        double h_abs = S_h_abs, h_abs_o = S_h_abs_old, err_o = S_err_old;
        if (S_h_abs < min_step) { h_abs = min_step; h_abs_o = -1; err_o = -1; }
        bool rejected = false, accepted = false;
        int n_iter = 0;
        double rate = -1, h = 0, t_new = t, error_norm = 0, safety = 0;
        while (!accepted) {
            if (h_abs < min_step) { status = -1; break; }
            if (max_attempts > 0 && attempts >= max_attempts) { status = 2; break; }
            attempts++;
            h = h_abs;
            t_new = t + h;
            if (t_new - t1 > 0) t_new = t1;
            h = t_new - t;
            h_abs = std::fabs(h);
            if (!have_sol) {
                HIP_OK(ctx, hipMemsetAsync(w.Z0, 0, sizeof(double) * 3 * n, ctx->stream));
            } else {   // Z0 = self.sol(t + h * C).T - y
                radau::X3 X;
                for (int s = 0; s < 3; s++) X.x[s] = ((t + h * C3[s]) - dense.t_old) / dense.h;
                hipLaunchKernelGGL(radau::dense_eval_kernel, gn, b256, 0, ctx->stream, w.Q, w.yold, (const double*)w.y, n, X, 3, w.Z0);
                LAUNCH_OK(ctx);
            }
            bool converged = false;
            while (!converged) {
                if (!have_lu) {
                    const cplx muc = {MU_COMPLEX.re / h, MU_COMPLEX.im / h};
                    if (int rc = radau_factor(ctx, w, MU_REAL / h, muc)) return rc;
                    st->nlu += 2;
                    have_lu = true;
                }
                // ---- solve_collocation_system ----
                const double M_real = MU_REAL / h;
                const cplx M_c = {MU_COMPLEX.re / h, MU_COMPLEX.im / h};
                hipLaunchKernelGGL(radau::newton_begin_kernel, gn, b256, 0, ctx->stream, w.y, w.Z0, n, rtol, atol, w.scale, w.Z, w.W, w.YS);
                LAUNCH_OK(ctx);
                double dW_norm_old = -1;
                rate = -1;
                int k;
                // small grids, radau_fused_solve = 3 (default there): two launches per iteration - the solve workgroups assemble their own
                // right-hand sides, the update workgroup evaluates the next iteration's stage derivatives (marl_radau_wg.h)
                const bool two_launch = w.pcr && (!w.cr_k || w.plan.k) && n <= radau::PCR_FUSED_MAX && ctx->radau_fused_solve == 3 && ctx->zc_on;
                for (k = 0; k < NEWTON_MAXITER; k++) {
                    if (!two_launch || k == 0)
                        if (int rc = launch_rhs(ctx, w.YS, w.F, LAYOUT_FIELD_MAJOR, 3)) return rc;
                    st->nfev += 3;
                    if (two_launch) {
                        hipLaunchKernelGGL(radau::newton_solve2_kernel, dim3(1, 2), dim3(radau::PCR_FUSED_THREADS), 0, ctx->stream, w.F, w.W, N, M_real, M_c, w.nlevels, w.Sr,
                                           w.Sc, w.rhs_r, w.rhs_c, w.flags, w.plan, w.Cr, w.Cc);
                        LAUNCH_OK(ctx);
                        if (ctx->var_dphi)
                            hipLaunchKernelGGL(radau::newton_update_rhs_kernel<true>, dim3(1), dim3(radau::WG_THREADS), 0, ctx->stream, w.y, w.rhs_r, w.rhs_c, w.scale, N, w.W,
                                               w.Z, w.YS, w.F, ctx->dconsts, w.out);
                        else
                            hipLaunchKernelGGL(radau::newton_update_rhs_kernel<false>, dim3(1), dim3(radau::WG_THREADS), 0, ctx->stream, w.y, w.rhs_r, w.rhs_c, w.scale, N, w.W,
                                               w.Z, w.YS, w.F, ctx->dconsts, w.out);
                        LAUNCH_OK(ctx);
                    } else
                    if (w.pcr && (!w.cr_k || w.plan.k) && n <= radau::PCR_FUSED_MAX && ctx->radau_fused_solve == 2) {   // right-hand sides + both solves + update + norm: one launch
                        hipLaunchKernelGGL(radau::newton_fused_kernel, dim3(1), dim3(radau::PCR_FUSED_THREADS), 0, ctx->stream, w.y, w.F, N, M_real, M_c, w.nlevels, w.Sr,
                                           w.Sc, w.scale, w.W, w.Z, w.YS, w.rhs_r, w.rhs_c, w.flags, w.out, w.plan, w.Cr, w.Cc);
                        LAUNCH_OK(ctx);
                    } else {
                    hipLaunchKernelGGL(radau::newton_rhs_kernel, gn, b256, 0, ctx->stream, w.F, w.W, N, M_real, M_c, w.rhs_r, w.rhs_c, w.flags);
                    LAUNCH_OK(ctx);
                    if (int rc = radau_solve(ctx, w, true)) return rc;
                    {
                        const int nbk = radau_norm_blocks(n);
                        hipLaunchKernelGGL(radau::newton_update_kernel, dim3(nbk), dim3(1024), 0, ctx->stream, w.y, w.rhs_r, w.rhs_c, w.scale, N, w.W, w.Z, w.YS,
                                           nbk > 1 ? w.partial : w.out);
                        LAUNCH_OK(ctx);
                        if (nbk > 1) {
                            hipLaunchKernelGGL(radau::sum_partials_kernel, dim3(1), dim3(1), 0, ctx->stream, w.partial, nbk, w.out);
                            LAUNCH_OK(ctx);
                        }
                    }
                    }
                    double ss;
                    int nonfinite;
                    if (int rc = radau_read(ctx, w, &ss, &nonfinite)) return rc;
                    if (nonfinite) break;   // `if not np.all(np.isfinite(F)): break` (the solve above is then unused)
                    const double dW_norm = std::sqrt(ss) / std::sqrt((double)(3 * n));
                    if (dW_norm_old >= 0) rate = dW_norm / dW_norm_old;
                    if (rate >= 0 && (rate >= 1 || std::pow(rate, NEWTON_MAXITER - k) / (1 - rate) * dW_norm > newton_tol)) break;
                    // (W += dW, Z = T W were applied by newton_update_kernel)
                    if (dW_norm == 0 || (rate >= 0 && rate / (1 - rate) * dW_norm < newton_tol)) { converged = true; break; }
                    dW_norm_old = dW_norm;
                }
                n_iter = (k < NEWTON_MAXITER ? k : NEWTON_MAXITER - 1) + 1;
                if (!converged) {
                    if (current_jac) break;
                    if (int rc = radau_num_jac_run(ctx, w, w.y, w.f, atol)) return rc;
                    st->njev++;
                    current_jac = true;
                    have_lu = false;
                }
            }
            if (!converged) {
                h_abs *= 0.5;
                have_lu = false;
                st->n_rejected++;
                continue;
            }
            // error estimate (radau.py:466-478); small grids: one launch (error_fused_kernel)
            const bool err_fused = w.pcr && (!w.cr_k || w.plan.k) && n <= radau::PCR_FUSED_MAX && ctx->radau_fused_solve == 3;
            auto error_estimate = [&](const double* fvec) -> int {
                if (err_fused) {
                    hipLaunchKernelGGL(radau::error_fused_kernel, dim3(1), dim3(radau::PCR_FUSED_THREADS), 0, ctx->stream, fvec, w.Z, w.y, N, E3[0], E3[1], E3[2], h, w.nlevels,
                                       w.Sr, rtol, atol, w.ynew, w.err, w.yerr, w.out, w.plan, w.Cr);
                    LAUNCH_OK(ctx);
                    return 0;
                }
                hipLaunchKernelGGL(radau::error_rhs_kernel, gn, b256, 0, ctx->stream, fvec, w.Z, w.y, N, E3[0], E3[1], E3[2], h, w.rhs_r, w.ynew);
                LAUNCH_OK(ctx);
                if (int rc = radau_solve(ctx, w, false)) return rc;
                return radau_error_norm(ctx, w, rtol, atol);
            };
            if (int rc = error_estimate(w.f)) return rc;
            double ss;
            if (int rc = radau_read(ctx, w, &ss, nullptr)) return rc;
            error_norm = std::sqrt(ss) / std::sqrt((double)n);
            safety = 0.9 * (2 * NEWTON_MAXITER + 1) / (2 * NEWTON_MAXITER + n_iter);
            if (rejected && error_norm > 1) {
                if (int rc = launch_rhs(ctx, w.yerr, w.tmp, LAYOUT_FIELD_MAJOR)) return rc;   // fun(t, y + error)
                st->nfev++;
                if (int rc = error_estimate(w.tmp)) return rc;
                if (int rc = radau_read(ctx, w, &ss, nullptr)) return rc;
                error_norm = std::sqrt(ss) / std::sqrt((double)n);
            }
            if (error_norm > 1) {
                const double sf = safety * radau_predict_factor(h_abs, h_abs_o, error_norm, err_o);
                h_abs *= (sf > MIN_FACTOR) ? sf : MIN_FACTOR;
                have_lu = false;
                rejected = true;
                st->n_rejected++;
            } else {
                accepted = true;
            }
        }
        if (status != 1) break;
        const bool recompute_jac = n_iter > 2 && rate > 1e-3;
        double factor = radau_predict_factor(h_abs, h_abs_o, error_norm, err_o);
        { const double sf = safety * factor; factor = (sf < MAX_FACTOR) ? sf : MAX_FACTOR; }
        if (!recompute_jac && factor < 1.2) factor = 1;
        else have_lu = false;
        // small grids: f(y_new), the dense-output coefficients and the monitors of y_new in one launch (accept_fused_kernel)
        const bool acc_fused = w.pcr && n <= radau::PCR_FUSED_MAX && ctx->radau_fused_solve == 3 && ctx->zc_on;
        if (acc_fused) {
            if (ctx->var_dphi)
                hipLaunchKernelGGL(radau::accept_fused_kernel<true>, dim3(1), dim3(radau::WG_THREADS), 0, ctx->stream, w.ynew, w.fnew, w.Z, N, P, w.Q, ctx->dconsts, ctx->zc_d);
            else
                hipLaunchKernelGGL(radau::accept_fused_kernel<false>, dim3(1), dim3(radau::WG_THREADS), 0, ctx->stream, w.ynew, w.fnew, w.Z, N, P, w.Q, ctx->dconsts, ctx->zc_d);
            LAUNCH_OK(ctx);
        } else if (int rc = launch_rhs(ctx, w.ynew, w.fnew, LAYOUT_FIELD_MAJOR)) return rc;
        st->nfev++;
        if (recompute_jac) {
            if (int rc = radau_num_jac_run(ctx, w, w.ynew, w.fnew, atol)) return rc;
            st->njev++;
            current_jac = true;
        } else {
            current_jac = false;
        }
        S_h_abs_old = S_h_abs;      // radau.py:512: the value self.h_abs had when this step started
        S_err_old = error_norm;
        S_h_abs = h_abs * factor;
        st->n_accepted++;
        std::swap(w.yold, w.y);      // y_old = y
        std::swap(w.y, w.ynew);      // y = y_new   (w.ynew now holds the state before last: scratch)
        std::swap(w.f, w.fnew);
        const double t_old = t;
        t = t_new;
        if (!acc_fused) {
            hipLaunchKernelGGL(radau::dense_q_kernel, gn, b256, 0, ctx->stream, w.Z, n, P, w.Q);
            LAUNCH_OK(ctx);
        }
        have_sol = true;
        dense = {t_old, t - t_old};
        if (t - t1 >= 0) status = 0;

        // events (ivp.py:673-694) and t_eval (ivp.py:706-723)
        if (acc_fused) {
            double marker;
            if (int rc = radau_read(ctx, w, &marker, nullptr)) return rc;
            for (int e = 0; e < 7; e++) g_new[e] = const_cast<const volatile double*>(ctx->zc_h)[16 + e];
        } else if (int rc = radau_monitors(ctx, w.y, g_new)) return rc;
        auto dense_at = [&](double tq, double* out) { return radau_dense(ctx, w, dense, tq, out); };
        double t_stop;
        if (int rc = accepted_step_epilogue(ctx, w, g, g_new, t_old, t, dense_at, t_eval, n_eval, eval_i, y_eval_host, t_events, max_events, st, &t_stop))
            return rc;
        if (t_stop <= t) {   // a terminal monitor ended the run inside this step (ivp.py:696-704): the state there, scipy's status 1
            if (int rc = dense_at(t_stop, w.y)) return rc;
            t = t_stop;
            stopped = true;
            break;
        }
    }
    if (stopped) status = 1;
    st->status = status;
    st->t = t;
    st->h_next = S_h_abs;
    if (int rc = radau_monitors(ctx, w.y, st->event_value)) return rc;
    return 0;
}

// ---- BDF (scipy/integrate/_ivp/bdf.py), the other implicit method the reference's Solver names --------------------------------------
// compute_R / change_D (bdf.py:18-33): D[:order + 1] = (R U)^T D[:order + 1]
void bdf_compute_R(int order, double factor, double R[6][6])
{
    for (int j = 0; j <= order; j++) R[0][j] = 1;
    for (int i = 1; i <= order; i++) {
        R[i][0] = 0;
        for (int j = 1; j <= order; j++) R[i][j] = R[i - 1][j] * ((i - 1 - factor * j) / i);
    }
}

int bdf_change_D(marl_ctx* ctx, double* D, int64_t n, int order, double factor)
{
    double R[6][6], U[6][6];
    bdf::Mat6 RU = {};
    bdf_compute_R(order, factor, R);
    bdf_compute_R(order, 1.0, U);
    for (int i = 0; i <= order; i++)
        for (int j = 0; j <= order; j++) {
            double a = 0;
            for (int k = 0; k <= order; k++) a += R[i][k] * U[k][j];
            RU.m[i][j] = a;
        }
    hipLaunchKernelGGL(bdf::change_D_kernel, dim3(blocks256(n)), dim3(256), 0, ctx->stream, D, n, order, RU);
    LAUNCH_OK(ctx);
    return 0;
}

// sum (coef v / (atol + rtol |yref|))^2 -> host
int bdf_scaled_sumsq(marl_ctx* ctx, RadauWork& w, const double* v, double coef, const double* yref, double rtol, double atol, double* ss)
{
    const int64_t n = NF * ctx->N;
    const int nbk = radau_norm_blocks(n);
    hipLaunchKernelGGL(bdf::scaled_norm_kernel, dim3(nbk), dim3(1024), 0, ctx->stream, v, coef, yref, rtol, atol, n, nbk > 1 ? w.partial : w.out);
    LAUNCH_OK(ctx);
    if (nbk > 1) {
        hipLaunchKernelGGL(radau::sum_partials_kernel, dim3(1), dim3(1), 0, ctx->stream, w.partial, nbk, w.out);
        LAUNCH_OK(ctx);
    }
    return radau_read(ctx, w, ss, nullptr);
}

struct BdfDense { double t, h; int order; const double* D; };

int bdf_dense(marl_ctx* ctx, const BdfDense& d, double tq, double* out)
{
    bdf::Vec6 p = {};
    double acc = 1;
    for (int j = 0; j < d.order; j++) {   // x_j = (t - (t_end - h j)) / (h (1 + j)); p = cumprod(x)
        acc *= (tq - (d.t - d.h * j)) / (d.h * (1 + j));
        p.v[j] = acc;
    }
    const int64_t n = NF * ctx->N;
    hipLaunchKernelGGL(bdf::dense_kernel, dim3(blocks256(n)), dim3(256), 0, ctx->stream, d.D, n, d.order, p, out);
    LAUNCH_OK(ctx);
    return 0;
}

// BDF.__init__ + the solve_ivp loop (ivp.py:654-723) around BDF._step_impl (bdf.py:310-450).  Buffers of the Radau arena are reused:
// D = [Z | W | F] (8 n of 9 n), f = Z0, y_predict / psi / d = Q.
int bdf_run(marl_ctx* ctx, RadauWork& w, double t0, double t1, double first_step, double rtol, double atol, const double* t_eval,
            int64_t n_eval, double* y_eval_host, double* t_events, int64_t max_events, int64_t max_attempts, marl_stats* st)
{
    const int64_t N = ctx->N, n = NF * N;
    constexpr int NEWTON_MAXITER = 4, MAX_ORDER = 5;
    constexpr double MIN_FACTOR = 0.2, MAX_FACTOR = 10;
    memset(st, 0, sizeof *st);
    rtol = clamp_rtol(rtol);
    const dim3 gn(blocks256(n)), b256(256);
    const double kappa[6] = {0, -0.1850, -1.0 / 9, -0.0823, -0.0415, 0};
    bdf::Vec6 gamma = {};
    double alpha[6], error_const[6];
    for (int k = 1; k <= MAX_ORDER; k++) gamma.v[k] = gamma.v[k - 1] + 1.0 / k;
    for (int k = 0; k <= MAX_ORDER; k++) { alpha[k] = (1 - kappa[k]) * gamma.v[k]; error_const[k] = kappa[k] * gamma.v[k] + 1.0 / (k + 1); }
    double* D = w.Z;            // [MAX_ORDER + 3][n]
    double* f = w.Z0;           // f(t_new, y) of the Newton iteration
    double* ypred = w.Q, *psi = w.Q + n, *d = w.Q + 2 * n;
    w.pcr = true;               // (the sequential block-Thomas option serves the Radau path only)

    double t = t0;
    if (int rc = launch_rhs(ctx, w.y, w.f, LAYOUT_FIELD_MAJOR)) return rc;
    st->nfev = 1;
    double S_h_abs = first_step;
    const double newton_tol = std::fmax(10 * radau::EPS / rtol, std::fmin(0.03, std::sqrt(rtol)));
    if (!ctx->zc_on) HIP_OK(ctx, hipMemsetAsync(w.flags, 0, sizeof(int32_t) * 2, ctx->stream));
    // jac_wrapped(t0, y0): f = fun_single(t, y) (not counted; the same values as w.f), J by finite differences
    if (int rc = radau_num_jac_run(ctx, w, w.y, w.f, atol)) return rc;
    st->njev = 1;
    hipLaunchKernelGGL(bdf::init_D_kernel, gn, b256, 0, ctx->stream, w.y, w.f, S_h_abs, n, D);
    LAUNCH_OK(ctx);
    int order = 1, n_equal_steps = 0;
    bool have_lu = false;
    double g[7], g_new[7], g_spec[7];
    bool have_g_spec = false;   // g_spec: the monitors of the state the last converged solve left in w.ynew (solve_wg)
    const bool solve_wg = ctx->bdf_solve_wg && ctx->zc_on && (!w.cr_k || w.plan.k) && n <= radau::PCR_FUSED_MAX && ctx->radau_fused_solve;
    if (int rc = radau_monitors(ctx, w.y, g)) return rc;
    int64_t eval_i = 0, attempts = 0;
    int status = 1;   // (running; what a run returns with status 1 is `stopped`)
    bool stopped = false;

    while (status == 1) {
        if (t == t1) { status = 0; break; }
        const double min_step = 10 * std::fabs(std::nextafter(t, INFINITY) - t);
        double h_abs;
        if (S_h_abs < min_step) {
            h_abs = min_step;
            if (int rc = bdf_change_D(ctx, D, n, order, min_step / S_h_abs)) return rc;
            n_equal_steps = 0;
        } else {
            h_abs = S_h_abs;
        }
        bool current_jac = false, accepted = false;
        int n_iter = 0;
        double h = 0, t_new = t, error_norm = 0, safety = 0;
        while (!accepted) {
            if (h_abs < min_step) { status = -1; break; }
            if (max_attempts > 0 && attempts >= max_attempts) { status = 2; break; }
            attempts++;
            h = h_abs;
            t_new = t + h;
            if (t_new - t1 > 0) {
                t_new = t1;
                if (int rc = bdf_change_D(ctx, D, n, order, std::fabs(t_new - t) / h_abs)) return rc;
                n_equal_steps = 0;
                have_lu = false;
            }
            h = t_new - t;
            h_abs = std::fabs(h);
            if (!solve_wg) {
                hipLaunchKernelGGL(bdf::predict_kernel, gn, b256, 0, ctx->stream, D, n, order, gamma, alpha[order], rtol, atol, ypred, w.scale, psi, w.ynew, d);
                LAUNCH_OK(ctx);
            }
            bool converged = false;
            bool fused_err = false;   // the converged iteration's launch also left the local error sum (small systems, zero-copy words)
            const double c = h / alpha[order];
            bool first_pass = true;
            while (!converged) {
                if (!have_lu) {   // LU = self.lu(self.I - c * J)
                    if (int rc = pcr_factor_launch(ctx, w, 1.0, cplx{0, 0}, c, 1)) return rc;
                    st->nlu++;
                    have_lu = true;
                }
                if (!first_pass && !solve_wg) {
                    hipLaunchKernelGGL(bdf::newton_restart_kernel, gn, b256, 0, ctx->stream, ypred, n, w.ynew, d);
                    LAUNCH_OK(ctx);
                }
                const int wg_mode = first_pass ? 0 : 1;
                first_pass = false;
                // ---- solve_bdf_system (bdf.py:36-68) ----
                double dy_norm_old = -1;
                int k;
                if (solve_wg) {   // predictor / restart, every Newton iteration with its tests, error sum and monitors: one launch, one wait
                    if (ctx->var_dphi)
                        hipLaunchKernelGGL(bdf::solve_wg_kernel<true>, dim3(1), dim3(radau::WG_THREADS), 0, ctx->stream, wg_mode, D, order, gamma, alpha[order], ypred,
                                           psi, w.scale, w.ynew, d, f, N, c, w.nlevels, w.Sr, ctx->dconsts, newton_tol, error_const[order], rtol, atol, ctx->zc_d, w.plan, w.Cr);
                    else
                        hipLaunchKernelGGL(bdf::solve_wg_kernel<false>, dim3(1), dim3(radau::WG_THREADS), 0, ctx->stream, wg_mode, D, order, gamma, alpha[order], ypred,
                                           psi, w.scale, w.ynew, d, f, N, c, w.nlevels, w.Sr, ctx->dconsts, newton_tol, error_const[order], rtol, atol, ctx->zc_d, w.plan, w.Cr);
                    LAUNCH_OK(ctx);
                    double ss;
                    int nonfinite;
                    if (int rc = radau_read(ctx, w, &ss, &nonfinite)) return rc;
                    const volatile double* zw = const_cast<const volatile double*>(ctx->zc_h);
                    const int iters = (int)zw[bdf::SW_ITERS];
                    st->nfev += iters;
                    converged = zw[bdf::SW_CONVERGED] != 0;
                    fused_err = converged;
                    if (converged) {
                        for (int e = 0; e < 7; e++) g_spec[e] = zw[bdf::SW_G + e];
                        have_g_spec = true;
                    }
                    k = iters - 1;
                } else
                for (k = 0; k < NEWTON_MAXITER; k++) {
                    if (int rc = launch_rhs(ctx, w.ynew, f, LAYOUT_FIELD_MAJOR)) return rc;
                    st->nfev++;
                    if ((!w.cr_k || w.plan.k) && n <= radau::PCR_FUSED_MAX && ctx->radau_fused_solve) {   // right-hand side + every level + update + norm in one launch
                        // (with the zero-copy result words: the step's local error norm rides along - bdf.py:398-400 - one launch and
                        //  one wait less per step)
                        fused_err = ctx->zc_on;
                        hipLaunchKernelGGL(bdf::newton_fused_kernel, dim3(1), dim3(radau::PCR_FUSED_THREADS), 0, ctx->stream, f, psi, N, c, w.nlevels, w.Sr, w.scale,
                                           w.ynew, d, w.flags, w.out, error_const[order], rtol, atol, fused_err ? ctx->zc_d + 2 : (double*)nullptr, w.plan, w.Cr);
                        LAUNCH_OK(ctx);
                    } else {
                    hipLaunchKernelGGL(bdf::newton_rhs_kernel, gn, b256, 0, ctx->stream, f, psi, d, N, c, w.rhs_r, w.flags);
                    LAUNCH_OK(ctx);
                    if (int rc = radau_solve(ctx, w, false)) return rc;
                    {
                        const int nbk = radau_norm_blocks(n);
                        hipLaunchKernelGGL(bdf::newton_update_kernel, dim3(nbk), dim3(1024), 0, ctx->stream, w.rhs_r, w.scale, N, w.ynew, d, nbk > 1 ? w.partial : w.out);
                        LAUNCH_OK(ctx);
                        if (nbk > 1) {
                            hipLaunchKernelGGL(radau::sum_partials_kernel, dim3(1), dim3(1), 0, ctx->stream, w.partial, nbk, w.out);
                            LAUNCH_OK(ctx);
                        }
                    }
                    }
                    double ss;
                    int nonfinite;
                    if (int rc = radau_read(ctx, w, &ss, &nonfinite)) return rc;
                    if (nonfinite) break;
                    const double dy_norm = std::sqrt(ss) / std::sqrt((double)n);
                    double rate = -1;
                    if (dy_norm_old >= 0) rate = dy_norm / dy_norm_old;
                    if (rate >= 0 && (rate >= 1 || std::pow(rate, NEWTON_MAXITER - k) / (1 - rate) * dy_norm > newton_tol)) break;
                    if (dy_norm == 0 || (rate >= 0 && rate / (1 - rate) * dy_norm < newton_tol)) { converged = true; break; }
                    dy_norm_old = dy_norm;
                }
                n_iter = (k < NEWTON_MAXITER ? k : NEWTON_MAXITER - 1) + 1;
                if (!converged) {
                    if (current_jac) break;
                    // J = self.jac(t_new, y_predict): f = fun_single(t_new, y_predict) - not counted
                    if (int rc = launch_rhs(ctx, ypred, w.fnew, LAYOUT_FIELD_MAJOR)) return rc;
                    if (int rc = radau_num_jac_run(ctx, w, ypred, w.fnew, atol)) return rc;
                    st->njev++;
                    have_lu = false;
                    current_jac = true;
                }
            }
            if (!converged) {
                h_abs *= 0.5;
                if (int rc = bdf_change_D(ctx, D, n, order, 0.5)) return rc;
                n_equal_steps = 0;
                have_lu = false;
                st->n_rejected++;
                continue;
            }
            safety = 0.9 * (2 * NEWTON_MAXITER + 1) / (2 * NEWTON_MAXITER + n_iter);
            double ss;
            if (fused_err) ss = const_cast<const volatile double*>(ctx->zc_h)[2];   // written before the word radau_read waited for
            else if (int rc = bdf_scaled_sumsq(ctx, w, d, error_const[order], w.ynew, rtol, atol, &ss)) return rc;
            error_norm = std::sqrt(ss) / std::sqrt((double)n);
            if (error_norm > 1) {
                const double sf = safety * std::pow(error_norm, -1.0 / (order + 1));
                const double factor = (sf > MIN_FACTOR) ? sf : MIN_FACTOR;
                h_abs *= factor;
                if (int rc = bdf_change_D(ctx, D, n, order, factor)) return rc;
                n_equal_steps = 0;
                st->n_rejected++;   // (bdf.py:405-406: the LU is kept)
            } else {
                accepted = true;
            }
        }
        if (status != 1) break;
        n_equal_steps++;
        const double t_old = t;
        t = t_new;
        S_h_abs = h_abs;
        st->n_accepted++;
        hipLaunchKernelGGL(bdf::accept_kernel, gn, b256, 0, ctx->stream, D, d, w.ynew, n, order, w.y);
        LAUNCH_OK(ctx);
        if (n_equal_steps >= order + 1) {   // order / step-size selection (bdf.py:427-448); scale = atol + rtol |y_new| = |y| now
            double em = INFINITY, ep = INFINITY, ss;
            if (order > 1 && order < MAX_ORDER && ctx->zc_on && radau_norm_blocks(n) == 1) {   // both norms: one launch, one wait
                hipLaunchKernelGGL(bdf::scaled_norm2_kernel, dim3(1), dim3(1024), 0, ctx->stream, D + (int64_t)order * n, error_const[order - 1],
                                   D + (int64_t)(order + 2) * n, error_const[order + 1], w.y, rtol, atol, n, w.out, ctx->zc_d + 3);
                LAUNCH_OK(ctx);
                if (int rc = radau_read(ctx, w, &ss, nullptr)) return rc;
                em = std::sqrt(ss) / std::sqrt((double)n);
                ep = std::sqrt(const_cast<const volatile double*>(ctx->zc_h)[3]) / std::sqrt((double)n);
            } else {
            if (order > 1) {
                if (int rc = bdf_scaled_sumsq(ctx, w, D + (int64_t)order * n, error_const[order - 1], w.y, rtol, atol, &ss)) return rc;
                em = std::sqrt(ss) / std::sqrt((double)n);
            }
            if (order < MAX_ORDER) {
                if (int rc = bdf_scaled_sumsq(ctx, w, D + (int64_t)(order + 2) * n, error_const[order + 1], w.y, rtol, atol, &ss)) return rc;
                ep = std::sqrt(ss) / std::sqrt((double)n);
            }
            }
            const double en[3] = {em, error_norm, ep};
            double factors[3];
            int best = 0;
            for (int i = 0; i < 3; i++) {
                factors[i] = std::pow(en[i], -1.0 / (order + i));
                if (factors[i] > factors[best]) best = i;
            }
            for (int i = 0; i < 3; i++)
                if (factors[i] != factors[i]) { best = i; break; }   // np.argmax: the first NaN
            order += best - 1;
            const double sf = safety * factors[best];
            const double factor = (sf < MAX_FACTOR) ? sf : MAX_FACTOR;   // python's min(MAX_FACTOR, x): a NaN x yields MAX_FACTOR (bdf.py:442)
            S_h_abs *= factor;
            if (int rc = bdf_change_D(ctx, D, n, order, factor)) return rc;
            n_equal_steps = 0;
            have_lu = false;
        }
        if (t - t1 >= 0) status = 0;

        // events and t_eval on the dense output built AFTER the order / step-size update (bdf.py:452-454)
        const BdfDense dense = {t, S_h_abs, order, D};
        if (solve_wg && have_g_spec) {   // y = the state of the last converged solve: its monitors came with the solve
            for (int e = 0; e < 7; e++) g_new[e] = g_spec[e];
        } else if (int rc = radau_monitors(ctx, w.y, g_new)) return rc;
        have_g_spec = false;
        auto dense_at = [&](double tq, double* out) { return bdf_dense(ctx, dense, tq, out); };
        double t_stop;
        if (int rc = accepted_step_epilogue(ctx, w, g, g_new, t_old, t, dense_at, t_eval, n_eval, eval_i, y_eval_host, t_events, max_events, st, &t_stop))
            return rc;
        if (t_stop <= t) {   // a terminal monitor ended the run inside this step (ivp.py:696-704): the state there, scipy's status 1
            if (int rc = dense_at(t_stop, w.y)) return rc;
            t = t_stop;
            stopped = true;
            break;
        }
    }
    if (stopped) status = 1;
    st->status = status;
    st->t = t;
    st->h_next = S_h_abs;
    if (int rc = radau_monitors(ctx, w.y, st->event_value)) return rc;
    return 0;
}
}  // namespace

// marl_integrate_radau / marl_integrate_bdf: `entry` and `solver` in front of the messages, `run` = radau_run or bdf_run
static int integrate_implicit(const char* entry, const char* solver, decltype(radau_run)* run, marl_ctx* ctx, double* y, double t0, double t1,
                              double first_step, double rtol, double atol, const int32_t* groups, const double* t_eval, int64_t n_eval,
                              double* y_eval, double* t_events, int64_t max_events, int64_t max_attempts, marl_stats* stats)
{
    if (!ctx || !y || !stats || (n_eval > 0 && (!t_eval || !y_eval))) return ctx ? fail(ctx, -1, "%s: invalid argument", entry) : -1;
    if (ctx->batch != 1 || ctx->halo > 0) return fail(ctx, -1, "%s: single-instance, whole-grid context required", entry);
    if (int rc = check_ivp_args(ctx, solver, t0, t1, first_step, rtol, atol, t_eval, n_eval)) return rc;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    RadauWork w;
    if (int rc = radau_alloc(ctx, w, groups)) return rc;
    const size_t n = (size_t)NF * ctx->N;
    HIP_OK(ctx, hipMemcpyAsync(w.y, y, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (int rc = run(ctx, w, t0, t1, first_step, rtol, atol, t_eval, n_eval, y_eval, t_events, max_events, max_attempts, stats)) return rc;
    HIP_OK(ctx, hipMemcpyAsync(y, w.y, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int marl_integrate_radau(marl_ctx* ctx, double* y, double t0, double t1, double first_step, double rtol, double atol,
                                    const int32_t* groups, const double* t_eval, int64_t n_eval, double* y_eval, double* t_events,
                                    int64_t max_events, int64_t max_attempts, marl_stats* stats)
{
    return integrate_implicit("marl_integrate_radau", "radau", radau_run, ctx, y, t0, t1, first_step, rtol, atol, groups, t_eval, n_eval, y_eval,
                              t_events, max_events, max_attempts, stats);
}

extern "C" int marl_integrate_bdf(marl_ctx* ctx, double* y, double t0, double t1, double first_step, double rtol, double atol, const int32_t* groups,
                                  const double* t_eval, int64_t n_eval, double* y_eval, double* t_events, int64_t max_events, int64_t max_attempts,
                                  marl_stats* stats)
{
    return integrate_implicit("marl_integrate_bdf", "bdf", bdf_run, ctx, y, t0, t1, first_step, rtol, atol, groups, t_eval, n_eval, y_eval,
                              t_events, max_events, max_attempts, stats);
}

// ---- test hooks of the implicit path: ONE Jacobian, ONE factorisation and its solves (tests/test_gpu_implicit_parts.py) -------
// Both go through the functions radau_run / bdf_run call - radau_alloc, radau_num_jac, pcr_factor_launch, radau_solve - so that what
// the tests see is what an integration runs, chosen by the same options.
extern "C" int marl_debug_num_jac(marl_ctx* ctx, const double* y, double threshold, const int32_t* groups, double* factor_inout, int first,
                                  double* J_out)
{
    if (!ctx || !y || !factor_inout || !J_out) return ctx ? fail(ctx, -1, "marl_debug_num_jac: invalid argument") : -1;
    if (ctx->batch != 1 || ctx->halo > 0) return fail(ctx, -1, "marl_debug_num_jac: single-instance, whole-grid context required");
    HIP_OK(ctx, hipSetDevice(ctx->device));
    RadauWork w;
    if (int rc = radau_alloc(ctx, w, groups)) return rc;
    const size_t n = (size_t)NF * ctx->N;
    HIP_OK(ctx, hipMemcpyAsync(w.y, y, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (!first) HIP_OK(ctx, hipMemcpyAsync(w.fac, factor_inout, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (int rc = launch_rhs(ctx, w.y, w.f, LAYOUT_FIELD_MAJOR)) return rc;
    if (int rc = radau_num_jac(ctx, w, w.y, w.f, threshold, first ? 1 : 0)) return rc;
    HIP_OK(ctx, hipMemcpyAsync(J_out, w.J, 15 * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_OK(ctx, hipMemcpyAsync(factor_inout, w.fac, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int marl_debug_block_solve(marl_ctx* ctx, const double* J, double jscale, double mu_r, double mu_c_re, double mu_c_im, int systems,
                                      int64_t nrhs, const double* b_r, const double* b_c, double* x_r, double* x_c)
{
    if (!ctx || !J || !b_r || !x_r || nrhs < 0 || (systems != 1 && systems != 2) || (systems == 2 && (!b_c || !x_c)))
        return ctx ? fail(ctx, -1, "marl_debug_block_solve: invalid argument") : -1;
    if (ctx->batch != 1 || ctx->halo > 0) return fail(ctx, -1, "marl_debug_block_solve: single-instance, whole-grid context required");
    HIP_OK(ctx, hipSetDevice(ctx->device));
    RadauWork w;
    if (int rc = radau_alloc(ctx, w, nullptr)) return rc;
    if (!w.pcr) return fail(ctx, -1, "marl_debug_block_solve: the cyclic-reduction solver (radau_solver = 0) only");
    const size_t n = (size_t)NF * ctx->N;
    const bool both = systems == 2;
    HIP_OK(ctx, hipMemcpyAsync(w.J, J, 15 * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (int rc = pcr_factor_launch(ctx, w, mu_r, cplx{mu_c_re, mu_c_im}, jscale, systems)) return rc;
    for (int64_t k = 0; k < nrhs; k++) {   // one factorisation, nrhs solves: a solve must leave the factors as it found them
        HIP_OK(ctx, hipMemcpyAsync(w.rhs_r, b_r + k * n, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        if (both) HIP_OK(ctx, hipMemcpyAsync(w.rhs_c, b_c + k * 2 * n, 2 * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        if (int rc = radau_solve(ctx, w, both)) return rc;
        HIP_OK(ctx, hipMemcpyAsync(x_r + k * n, w.rhs_r, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        if (both) HIP_OK(ctx, hipMemcpyAsync(x_c + k * 2 * n, w.rhs_c, 2 * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// ---- what the sweeps of Radau and of BDF instances share: the host's end of a cycle, and the end of a sweep ----------------------
// The lengths of this cycle's work lists -> hcounts[0 .. ncounts).  Zero-copy mode: a one-thread kernel copies them into mapped host
// words, zeroes them and writes cycle + 1 behind them, which the host polls for; else a copy, a memset and a synchronise.
// The caller zeroes dcounts before the first cycle; from then on they are zero again, in stream order, right after they were read, and
// nothing between here and the next cycle's controllers touches them - the same as zeroing them at the top of that cycle.
static int sweep_read_counts(marl_ctx* ctx, int32_t* dcounts, int ncounts, int64_t cycle, int32_t* hcounts)
{
    if (ctx->implicit_zero_copy) {
        if (int rc = zc_ensure(ctx)) return rc;
        volatile int32_t* words = reinterpret_cast<volatile int32_t*>(ctx->zc_h + 16);
        const int32_t seq = (int32_t)(cycle + 1);
        if (cycle == 0) words[radau::L_COUNT] = 0;   // (an earlier sweep's last sequence number; nothing of it still runs)
        hipLaunchKernelGGL(radau::publish_counts_kernel, dim3(1), dim3(1), 0, ctx->stream, dcounts, reinterpret_cast<int32_t*>(ctx->zc_d + 16), seq);
        LAUNCH_OK(ctx);
        if (int rc = zc_spin(ctx, [&] { return words[radau::L_COUNT] == seq; }, "sweep: the work-list lengths never arrived")) return rc;
        for (int i = 0; i < ncounts; i++) hcounts[i] = words[i];
    } else {
        HIP_OK(ctx, hipMemcpyAsync(hcounts, dcounts, sizeof(int32_t) * ncounts, hipMemcpyDeviceToHost, ctx->stream));
        HIP_OK(ctx, hipMemsetAsync(dcounts, 0, sizeof(int32_t) * radau::L_COUNT, ctx->stream));
        HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
    }
    for (int i = 0; i < ncounts; i++)   // (every instance adds at most one to a count: a longer list is a corrupted word, not a grid.z)
        if ((uint32_t)hcounts[i] > (uint64_t)ctx->batch) return fail(ctx, -3, "sweep: a work list is longer than the sweep");
    return 0;
}

template <class Ctl>   // radau::RadauCtl, bdf::BdfCtl
static void ctl_to_stats(const Ctl& c, marl_stats& st)
{
    memset(&st, 0, sizeof st);
    st.nfev = c.nfev; st.njev = c.njev; st.nlu = c.nlu; st.n_accepted = c.n_acc; st.n_rejected = c.n_rej;
    st.status = c.status; st.t = c.t; st.h_next = c.S_h_abs;
    for (int e = 0; e < 7; e++) { st.event_value[e] = c.g[e]; st.n_events[e] = c.n_events[e]; }
}

// the arena of instance 0 as the one-workgroup-per-instance kernels take it (marl_radau_wg.h)
static radau::WgWork wg_work_of(const RadauWork& w, int64_t zs)
{
    radau::WgWork ww{};
    ww.y = w.y; ww.f = w.f; ww.fnew = w.fnew; ww.ynew = w.ynew; ww.err = w.err; ww.yerr = w.yerr; ww.yold = w.yold; ww.scale = w.scale; ww.tmp = w.tmp;
    ww.Z = w.Z; ww.W = w.W; ww.F = w.F; ww.Q = w.Q; ww.YS = w.YS; ww.fac = w.fac; ww.h = w.h; ww.yscale = w.yscale; ww.maxdiff = w.maxdiff; ww.scl = w.scl;
    ww.hnew = w.hnew; ww.Jraw = w.Jraw; ww.YP = w.YP; ww.FN = w.FN; ww.J = w.J; ww.rhs_r = w.rhs_r; ww.rhs_c = w.rhs_c; ww.small = w.small; ww.groups = w.groups;
    ww.Sr = w.Sr; ww.Sc = w.Sc; ww.ng = w.ng; ww.nlevels = w.nlevels; ww.zs = zs;
    ww.plan = w.plan; ww.Cr = w.Cr; ww.Cc = w.Cc;
    return ww;
}

// ---- a sweep of Radau instances (marl_radau_batch.h) -------------------------------------------------------------------------
// The Radau sweep behind marl_sweep_radau_dev / _events_dev / _eval_dev.
// t_events (host, may be NULL): [instance][7][max_events] root times of the seven monitors, located inside the sweep as the single run
// locates them (dense output of the accepted step + Brent, one A_DENSE action per function evaluation); entries beyond n_events are NaN.
// t_eval (host, n_eval times), y_eval_dev (device, [instance][n_eval][5N]), n_done (host, [instance]): the samples inside every accepted
// step by the same dense output, one A_FRAME action each, after the step's roots (PC_FRAMES); n_eval = 0: none, and the same cycles.
static int sweep_radau(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol, const int32_t* groups,
                       int64_t max_attempts, const double* t_eval, int64_t n_eval, double* y_eval_dev, int64_t* n_done, double* t_events,
                       int64_t max_events, marl_stats* stats)
{
    if (!ctx || !y_dev || !stats) return ctx ? fail(ctx, -1, "marl_sweep_radau_dev: invalid argument") : -1;
    if (n_eval < 0 || (n_eval > 0 && (!t_eval || !y_eval_dev || !n_done))) return fail(ctx, -1, "marl_sweep_radau_eval_dev: invalid argument");
    const bool locate = t_events != nullptr && max_events > 0, frames = n_eval > 0, term = has_terminal(ctx);
    if (ctx->halo > 0) return fail(ctx, -1, "marl_sweep_radau_dev: whole-grid context required");
    if (!(first_step > 0) || !(t1 >= t0)) return fail(ctx, -1, "radau: need first_step > 0 and t1 >= t0 (forward integration)");
    if (t1 > t0 && first_step > t1 - t0) return fail(ctx, -1, "radau: `first_step` exceeds bounds");
    if (!(rtol > 0) || !(atol >= 0)) return fail(ctx, -1, "radau: tolerances must be positive");
    for (int64_t i = 0; i < n_eval; i++)
        if (!(t_eval[i] >= t0) || !(t_eval[i] <= t1) || (i > 0 && t_eval[i] <= t_eval[i - 1]))
            return fail(ctx, -1, "radau: `t_eval` must be sorted and within t_span");  // ivp.py:603-609
    if (ctx->batch > 65535) return fail(ctx, -1, "marl_sweep_radau_dev: at most 65535 instances per call");
    const int64_t N = ctx->N, n = NF * N, B = ctx->batch;
    if (n > 8192) return fail(ctx, -1, "marl_sweep_radau_dev: sweeps are for small grids (N <= 1638); use marl_integrate_radau for one large grid");
    if (n_done) memset(n_done, 0, sizeof(int64_t) * (size_t)B);
    HIP_OK(ctx, hipSetDevice(ctx->device));
    rtol = clamp_rtol(rtol);
    RadauWork w;
    int64_t zs = 0;
    if (int rc = radau_alloc(ctx, w, groups, B, &zs)) return rc;
    using radau::RadauCtl;
    std::vector<RadauCtl> hctl((size_t)B);   // (before the device buffers: they wait for the stream when they go, this must still be there)
    // controllers, monitors records, work lists + their counts; every return from here on frees them (DevBuf)
    DevBuf b_ctl(ctx->stream), b_rec(ctx->stream), b_counts(ctx->stream), b_rec_dense(ctx->stream), b_tev(ctx->stream), b_teval(ctx->stream), b_wg(ctx->stream);
    HIP_OK(ctx, b_ctl.alloc(sizeof(RadauCtl) * B));
    HIP_OK(ctx, b_rec.alloc(sizeof(double) * NQ * B));
    HIP_OK(ctx, b_counts.alloc(sizeof(int32_t) * (size_t)(radau::L_COUNT * (B + 1))));
    RadauCtl* const dctl = b_ctl.as<RadauCtl>();
    double* const drec = b_rec.as<double>();
    int32_t* const dcounts = b_counts.as<int32_t>();   // [L_COUNT] then lists [L_COUNT][B]
    int32_t* dlists = dcounts + radau::L_COUNT;
    if (locate || term) {   // event root finding: monitors of the dense-output states (a step that meets a limit locates its roots with no t_events too)
        HIP_OK(ctx, b_rec_dense.alloc(sizeof(double) * NQ * B));
        HIP_OK(ctx, hipMemsetAsync(b_rec_dense.p, 0, sizeof(double) * NQ * B, ctx->stream));
    }
    if (locate) {   // the root times
        HIP_OK(ctx, b_tev.alloc(sizeof(double) * (size_t)(7 * max_events) * B));
        HIP_OK(ctx, hipMemsetAsync(b_tev.p, 0xff, sizeof(double) * (size_t)(7 * max_events) * B, ctx->stream));   // (all bits set: NaN)
    }
    if (frames) {   // the sample times, for the controllers (pageable host memory: the copy has left the caller's array when the call returns)
        HIP_OK(ctx, b_teval.alloc(sizeof(double) * (size_t)n_eval));
        HIP_OK(ctx, hipMemcpyAsync(b_teval.p, t_eval, sizeof(double) * (size_t)n_eval, hipMemcpyHostToDevice, ctx->stream));
    }
    double *const drec_dense = b_rec_dense.as<double>(), *const dtev = b_tev.as<double>(), *const dteval = b_teval.as<double>();
    for (auto& c : hctl) {
        memset(&c, 0, sizeof c);
        c.t_bound = t1; c.rtol = rtol; c.atol = atol; c.max_attempts = max_attempts;
        c.newton_tol = std::fmax(10 * radau::EPS / rtol, std::fmin(0.03, std::sqrt(rtol)));
        c.t = t0; c.S_h_abs = first_step; c.S_h_abs_old = -1; c.S_err_old = -1;
        c.pc = radau::PC_INIT; c.status = radau::STATUS_RUNNING;
        c.locate_events = locate ? 1 : 0; c.max_events = max_events;
        c.n_eval = n_eval;
        for (int e = 0; e < 7; e++) c.terminal[e] = ctx->terminal[e];
    }
    HIP_OK(ctx, hipMemcpyAsync(dctl, hctl.data(), sizeof(RadauCtl) * B, hipMemcpyHostToDevice, ctx->stream));
    HIP_OK(ctx, hipMemcpy2DAsync(w.y, (size_t)zs, y_dev, n * sizeof(double), n * sizeof(double), (size_t)B, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_OK(ctx, hipMemsetAsync(drec, 0, sizeof(double) * NQ * B, ctx->stream));
    HIP_OK(ctx, hipMemsetAsync(dcounts, 0, sizeof(int32_t) * radau::L_COUNT, ctx->stream));   // (sweep_read_counts keeps them zero between cycles)
    const double S6 = std::sqrt(6.0);
    const double E3[3] = {(-13 - 7 * S6) / 3, (-13 + 7 * S6) / 3, -1.0 / 3};
    const radau::P33 P = {{{13.0 / 3 + 7 * S6 / 3, -23.0 / 3 - 22 * S6 / 3, 10.0 / 3 + 5 * S6},
                           {13.0 / 3 - 7 * S6 / 3, -23.0 / 3 + 22 * S6 / 3, 10.0 / 3 - 5 * S6},
                           {1.0 / 3, -8.0 / 3, 10.0 / 3}}};
    const int32_t* act0 = reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(dctl) + offsetof(RadauCtl, action));
    // a launch over the instances of work list `which` (no action mask needed: the list IS the mask)
    auto Z = [&](int which) { return ZBatch{zs, act0, (int64_t)sizeof(RadauCtl), ~0, dlists + (int64_t)which * B}; };
    const dim3 b256(256);
    const unsigned gx = blocks256(n), gc = blocks256(N);
    const int64_t nbm = std::min<int64_t>((N + 255) / 256, 1024);
    if (int rc = ensure_part(ctx, (size_t)(nbm * B))) return rc;
    int32_t* hcounts = reinterpret_cast<int32_t*>(ctx->rd_host);
    using namespace radau;
    // Sweeps of small grids (5 N <= PCR_FUSED_MAX: the reference's N = 200), option radau_sweep_wg:
    //   1            HYBRID: one persistent workgroup per instance runs everything of the instance that is sequential and small (step
    //                logic, Newton iterations, error estimates, accepted steps, event roots - marl_radau_wg.h) and hands it back for
    //                Jacobians and factorisations, which the launch kernels do over work lists on the whole chip: one host cycle per
    //                Jacobian / factorisation instead of one per action;
    //   3 (default)  HYBRID with the finite-difference Jacobian in the workgroup too (60 us there against a host cycle of ~100 us): only
    //                factorisations come back to the host cycle - bit-identical to 1;
    //   2            the workgroup does those as well (no host in the loop; measured slower: cyclic reduction on ONE compute unit);
    //   0            the launch-per-action cycle (larger grids always take it).
    const int wg_mode = (n <= PCR_FUSED_MAX) ? (int)ctx->radau_sweep_wg : 0;
    const bool use_wg = wg_mode == 2 && !locate && !frames && !term;
    const WgWork ww = wg_mode ? wg_work_of(w, zs) : WgWork{};
    if (wg_mode) {
        if (!ctx->cus) {
            hipDeviceProp_t prop;
            HIP_OK(ctx, hipGetDeviceProperties(&prop, ctx->device));
            ctx->cus = prop.multiProcessorCount;
        }
        HIP_OK(ctx, b_wg.alloc(sizeof(unsigned) * (size_t)(2 + 2 * B)));
    }
    unsigned* const wg_next = b_wg.as<unsigned>();   // one-workgroup-per-instance paths: the instance queue, then the list of instances a pass visits [2 B]
    // nrun < 0: the pass visits every instance; else the instances run_list[0 .. nrun) (those the last pass handed back)
    auto launch_wg = [&](int hybrid, int64_t nrun) {
        (void)hipMemsetAsync(wg_next, 0, sizeof(unsigned), ctx->stream);
        const int64_t todo = nrun < 0 ? B : nrun;
        const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>(todo, (int64_t)ctx->cus)));
        const int32_t* run_list = nrun < 0 ? nullptr : reinterpret_cast<const int32_t*>(wg_next + 2);
#define MARL_WG_LAUNCH(VD_, H_, T_)                                                                                                         \
        hipLaunchKernelGGL((radau_wg_kernel<VD_, H_, T_>), grid, dim3(WG_THREADS), 0, ctx->stream, dctl, B, N, ww, ctx->dconsts, atol, P, E3[0], E3[1], E3[2], \
                           wg_next, dcounts, dlists, dtev, run_list, todo, (const double*)dteval, y_eval_dev)
        // (a sweep with a terminal monitor never takes hybrid == 0: use_wg below; its two hybrid kinds have instantiations of their own)
        if (ctx->var_dphi) {
            if (hybrid == 0) MARL_WG_LAUNCH(true, 0, false);
            else if (hybrid == 1) { if (term) MARL_WG_LAUNCH(true, 1, true); else MARL_WG_LAUNCH(true, 1, false); }
            else { if (term) MARL_WG_LAUNCH(true, 2, true); else MARL_WG_LAUNCH(true, 2, false); }
        } else {
            if (hybrid == 0) MARL_WG_LAUNCH(false, 0, false);
            else if (hybrid == 1) { if (term) MARL_WG_LAUNCH(false, 1, true); else MARL_WG_LAUNCH(false, 1, false); }
            else { if (term) MARL_WG_LAUNCH(false, 2, true); else MARL_WG_LAUNCH(false, 2, false); }
        }
#undef MARL_WG_LAUNCH
    };
    if (use_wg) {
        launch_wg(0, -1);
        LAUNCH_OK(ctx);
    }
    int64_t wg_nrun = -1;
    const bool hybrid = wg_mode == 1 || wg_mode == 3 || (wg_mode == 2 && (locate || frames || term));
    const int hybrid_kind = wg_mode == 3 ? 2 : 1;   // 2: Jacobians stay in the workgroup, only factorisations come back to the host cycle
    for (int64_t cycle = 0; !use_wg; cycle++) {
        // the controllers advance every instance to its next piece of work and sort the instances into work lists; the host
        // reads the list lengths (sweep_read_counts) and launches each kind of work over its list only
        if (hybrid) launch_wg(hybrid_kind, wg_nrun);   // every running instance up to its next Jacobian / factorisation (or its end)
        else if (term) hipLaunchKernelGGL(radau_control_kernel<true>, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, ctx->stream, dctl, drec, B, n, dcounts, dlists, drec_dense, dtev, dteval);
        else hipLaunchKernelGGL(radau_control_kernel<false>, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, ctx->stream, dctl, drec, B, n, dcounts, dlists, drec_dense, dtev, dteval);
        LAUNCH_OK(ctx);
        if (int rc = sweep_read_counts(ctx, dcounts, L_COUNT, cycle, hcounts)) return rc;
        if (hcounts[L_RUNNING] == 0) break;
        if (hybrid) {   // the instances handed back in this pass are the ones the next pass visits (after their Jacobian / factorisation below)
            const int64_t nj = hcounts[L_JAC], nl = hcounts[L_LU];
            int32_t* run_list = reinterpret_cast<int32_t*>(wg_next + 2);
            if (nj) HIP_OK(ctx, hipMemcpyAsync(run_list, dlists + (int64_t)L_JAC * B, sizeof(int32_t) * (size_t)nj, hipMemcpyDeviceToDevice, ctx->stream));
            if (nl) HIP_OK(ctx, hipMemcpyAsync(run_list + nj, dlists + (int64_t)L_LU * B, sizeof(int32_t) * (size_t)nl, hipMemcpyDeviceToDevice, ctx->stream));
            wg_nrun = nj + nl;
        }
        const unsigned nR = (unsigned)hcounts[L_RHS1], nA = (unsigned)hcounts[L_ACCEPT], nJ = (unsigned)hcounts[L_JAC], nL = (unsigned)hcounts[L_LU],
                       nN = (unsigned)hcounts[L_NEWTON], nE = (unsigned)hcounts[L_ERR], nD = (unsigned)hcounts[L_DENSE], nF = (unsigned)hcounts[L_FRAME],
                       nS = (unsigned)hcounts[L_STOP];
        if (nF) {   // t_eval samples inside the accepted step: its dense output into the instances' frames (no monitors: nothing reads a frame)
            hipLaunchKernelGGL(frame_eval_batch_kernel, dim3(gx, 1, nF), b256, 0, ctx->stream, w.Q, w.yold, n, y_eval_dev, n_eval, Z(L_FRAME));
            LAUNCH_OK(ctx);
        }
        if (nD) {   // event root finding: the dense output of the accepted step at the abscissa Brent asks for, and that state's monitors
            hipLaunchKernelGGL(dense_eval_batch_kernel, dim3(gx, 1, nD), b256, 0, ctx->stream, w.Q, w.yold, n, w.tmp, Z(L_DENSE));
            LAUNCH_OK(ctx);
            hipLaunchKernelGGL(monitors_kernel<LAYOUT_FIELD_MAJOR>, dim3((unsigned)nbm, (unsigned)B), b256, 0, ctx->stream, w.tmp, ctx->dconsts, ctx->slab, zs / 8, ctx->part);
            LAUNCH_OK(ctx);
            hipLaunchKernelGGL(reduce_records_kernel, dim3((unsigned)B), b256, 0, ctx->stream, ctx->part, nbm, drec_dense);
            LAUNCH_OK(ctx);
        }
        if (nR) {   // a single state -> its derivative: y -> f (start), y + err -> tmp (second error estimate), y_new -> f_new (accepted step)
            if (ctx->var_dphi)
                hipLaunchKernelGGL((rhs_pick_kernel<LAYOUT_FIELD_MAJOR, true>), dim3(gc, 1, nR), b256, 0, ctx->stream, w.y, w.f, w.yerr, w.tmp, w.ynew, w.fnew, ctx->dconsts,
                                   ctx->slab, Z(L_RHS1));
            else
                hipLaunchKernelGGL((rhs_pick_kernel<LAYOUT_FIELD_MAJOR, false>), dim3(gc, 1, nR), b256, 0, ctx->stream, w.y, w.f, w.yerr, w.tmp, w.ynew, w.fnew, ctx->dconsts,
                                   ctx->slab, Z(L_RHS1));
            LAUNCH_OK(ctx);
        }
        if (nA) {
            hipLaunchKernelGGL(accept_kernel, dim3(gx, 1, nA), b256, 0, ctx->stream, w.Z, w.Q, w.y, w.yold, w.ynew, w.f, w.fnew, n, P, Z(L_ACCEPT));
            LAUNCH_OK(ctx);
        }
        if (nS) {   // a terminal monitor ended these instances' runs inside the step just accepted: its dense output at t_stop is their state
            hipLaunchKernelGGL(stop_state_batch_kernel, dim3(gx, 1, nS), b256, 0, ctx->stream, w.Q, w.yold, n, w.y, Z(L_STOP));
            LAUNCH_OK(ctx);
        }
        if ((nA || nS || cycle == 0) && !hybrid) {   // monitors of every instance's y (read by the controllers after the start, after each accepted step and after a stop)
            hipLaunchKernelGGL(monitors_kernel<LAYOUT_FIELD_MAJOR>, dim3((unsigned)nbm, (unsigned)B), b256, 0, ctx->stream, w.y, ctx->dconsts, ctx->slab, zs / 8, ctx->part);
            LAUNCH_OK(ctx);
            hipLaunchKernelGGL(reduce_records_kernel, dim3((unsigned)B), b256, 0, ctx->stream, ctx->part, nbm, drec);
            LAUNCH_OK(ctx);
        }
        if (nJ)   // finite-difference Jacobian at (y, f); which instances have step-size factors already, their controllers say
            if (int rc = radau_num_jac(ctx, w, w.y, w.f, atol, 0, nJ, Z(L_JAC))) return rc;
        if (nL)   // both factorisations, mu from the controllers (small grids: cyclic reduction in front of PCR - radau_alloc)
            if (int rc = pcr_factor_launch(ctx, w, 0.0, cplx{0, 0}, 1.0, 2, nL, Z(L_LU))) return rc;
        if (nN) {   // one Newton iteration
            hipLaunchKernelGGL(newton_begin_batch_kernel, dim3(gx, 1, nN), b256, 0, ctx->stream, w.y, w.Q, w.yold, n, w.scale, w.Z, w.W, w.YS, Z(L_NEWTON));
            LAUNCH_OK(ctx);
            if (int rc = launch_rhs_fm(ctx, w.YS, w.F, 3, nN, Z(L_NEWTON))) return rc;
            hipLaunchKernelGGL(newton_rhs_batch_kernel, dim3(gx, 1, nN), b256, 0, ctx->stream, w.F, w.W, N, w.rhs_r, w.rhs_c, dctl, Z(L_NEWTON));
            LAUNCH_OK(ctx);
        }
        for (int which = 0; which < 2; which++) {   // 0: both systems of the Newton iteration; 1: the real system of the error estimate
            const unsigned cnt = which == 0 ? nN : nE;
            if (!cnt) continue;
            const ZBatch zb = Z(which == 0 ? L_NEWTON : L_ERR);
            if (which == 1) {
                hipLaunchKernelGGL(error_rhs_batch_kernel, dim3(gx, 1, cnt), b256, 0, ctx->stream, w.f, w.tmp, w.Z, w.y, N, E3[0], E3[1], E3[2], w.rhs_r, w.ynew, zb);
                LAUNCH_OK(ctx);
            }
            if (int rc = radau_solve(ctx, w, which == 0, cnt, zb)) return rc;
            if (which == 0)
                hipLaunchKernelGGL(newton_update_batch_kernel, dim3(1, 1, cnt), dim3(1024), 0, ctx->stream, w.y, w.rhs_r, w.rhs_c, w.scale, N, w.W, w.Z, w.YS, dctl, zb);
            else
                hipLaunchKernelGGL(error_norm_batch_kernel, dim3(1, 1, cnt), dim3(1024), 0, ctx->stream, w.rhs_r, w.y, w.ynew, N, w.err, w.yerr, dctl, zb);
            LAUNCH_OK(ctx);
        }
    }
    // results (the synchronise is also what the sweep's buffers wait for before they go)
    HIP_OK(ctx, hipMemcpy2DAsync(y_dev, n * sizeof(double), w.y, (size_t)zs, n * sizeof(double), (size_t)B, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_OK(ctx, hipMemcpyAsync(hctl.data(), dctl, sizeof(RadauCtl) * B, hipMemcpyDeviceToHost, ctx->stream));
    if (locate) HIP_OK(ctx, hipMemcpyAsync(t_events, dtev, sizeof(double) * (size_t)(7 * max_events) * B, hipMemcpyDeviceToHost, ctx->stream));
    HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
    for (int64_t b = 0; b < B; b++) {
        ctl_to_stats(hctl[(size_t)b], stats[b]);
        if (hctl[(size_t)b].pc != radau::PC_DONE) return fail(ctx, -3, "marl_sweep_radau_dev: instance %lld did not finish", (long long)b);
        if (frames) n_done[b] = hctl[(size_t)b].fr_next;
    }
    if (t1 == t0 && frames && t_eval[0] == t0) {   // no step is taken (base.py:189-194): the sample at t0 is y0, as the single run gives it
        const size_t row = sizeof(double) * (size_t)n;
        HIP_OK(ctx, hipMemcpy2DAsync(y_eval_dev, row * (size_t)n_eval, y_dev, row, row, (size_t)B, hipMemcpyDeviceToDevice, ctx->stream));
        HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
        for (int64_t b = 0; b < B; b++) n_done[b] = 1;
    }
    return 0;
}

extern "C" int marl_sweep_radau_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol,
                                    const int32_t* groups, int64_t max_attempts, marl_stats* stats)
{
    return sweep_radau(ctx, y_dev, t0, t1, first_step, rtol, atol, groups, max_attempts, nullptr, 0, nullptr, nullptr, nullptr, 0, stats);
}

extern "C" int marl_sweep_radau_events_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol,
                                           const int32_t* groups, int64_t max_attempts, double* t_events, int64_t max_events, marl_stats* stats)
{
    return sweep_radau(ctx, y_dev, t0, t1, first_step, rtol, atol, groups, max_attempts, nullptr, 0, nullptr, nullptr, t_events, max_events, stats);
}

extern "C" int marl_sweep_radau_eval_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol,
                                         const int32_t* groups, int64_t max_attempts, const double* t_eval, int64_t n_eval, double* y_eval_dev,
                                         int64_t* n_done, double* t_events, int64_t max_events, marl_stats* stats)
{
    return sweep_radau(ctx, y_dev, t0, t1, first_step, rtol, atol, groups, max_attempts, t_eval, n_eval, y_eval_dev, n_done, t_events, max_events, stats);
}

// ---- the launches of the BDF sweep's vector kernels (marl_bdf_batch.h): one launcher each, called by sweep_bdf and by the test hook
// marl_debug_bdf_batch below, so that a test launches what a sweep launches.  zb: the instances' stride, their controllers and the work
// list (NULL: every instance in order); cnt: the instances launched (grid.z).
struct BdfArena { double *D, *f, *ypred, *psi, *d; };   // where bdf_run's vectors live in an instance's arena (marl_bdf_batch.h)
static BdfArena bdf_arena_of(const RadauWork& w, int64_t n) { return BdfArena{w.Z, w.Z0, w.Q, w.Q + n, w.Q + 2 * n}; }

static int bdf_launch_init_D(marl_ctx* ctx, const RadauWork& w, int64_t n, unsigned cnt, const bdf::BdfBatch& zb)
{
    hipLaunchKernelGGL(bdf::init_D_batch_kernel, dim3(blocks256(n), 1, cnt), dim3(256), 0, ctx->stream, w.y, w.f, n, bdf_arena_of(w, n).D, zb);
    LAUNCH_OK(ctx);
    return 0;
}

static int bdf_launch_accept_norms(marl_ctx* ctx, const RadauWork& w, int64_t n, unsigned cnt, const bdf::BdfBatch& zb)
{
    const BdfArena a = bdf_arena_of(w, n);
    hipLaunchKernelGGL(bdf::accept_norms_batch_kernel, dim3(1, 1, cnt), dim3(1024), 0, ctx->stream, a.D, a.d, w.ynew, n, w.y, zb);
    LAUNCH_OK(ctx);
    return 0;
}

static int bdf_launch_change_D(marl_ctx* ctx, const RadauWork& w, int64_t n, unsigned cnt, const bdf::BdfBatch& zb)
{
    hipLaunchKernelGGL(bdf::change_D_batch_kernel, dim3(blocks256(n), 1, cnt), dim3(256), 0, ctx->stream, bdf_arena_of(w, n).D, n, zb);
    LAUNCH_OK(ctx);
    return 0;
}

// dterm: the instances' terminal-monitor states in a sweep that has limits (listed instances with A_TERM_ROOTS search on theirs), else NULL
static int bdf_launch_roots(marl_ctx* ctx, const RadauWork& w, int64_t N, const bdfctl::BdfRoots* droots, double* dtev, unsigned cnt, const bdf::BdfBatch& zb,
                            bdfctl::BdfTerm* dterm = nullptr)
{
    if (dterm)
        hipLaunchKernelGGL(bdf::roots_batch_kernel<true>, dim3(1, 1, cnt), dim3(radau::WG_THREADS), 0, ctx->stream, bdf_arena_of(w, NF * N).D, N, droots, dtev, ctx->dconsts,
                           zb, dterm);
    else
        hipLaunchKernelGGL(bdf::roots_batch_kernel<false>, dim3(1, 1, cnt), dim3(radau::WG_THREADS), 0, ctx->stream, bdf_arena_of(w, NF * N).D, N, droots, dtev, ctx->dconsts,
                           zb, dterm);
    LAUNCH_OK(ctx);
    return 0;
}

static int bdf_launch_stop_state(marl_ctx* ctx, const RadauWork& w, int64_t N, const bdfctl::BdfTerm* dterm, unsigned cnt, const bdf::BdfBatch& zb)
{
    hipLaunchKernelGGL(bdf::stop_state_batch_kernel, dim3(1, 1, cnt), dim3(radau::WG_THREADS), 0, ctx->stream, bdf_arena_of(w, NF * N).D, N, dterm, w.y, ctx->dconsts, zb);
    LAUNCH_OK(ctx);
    return 0;
}

static int bdf_launch_sample(marl_ctx* ctx, const RadauWork& w, int64_t n, const double* dteval, int64_t n_eval, const bdfctl::BdfSample* dsmp, double* y_eval_dev,
                             unsigned cnt, const bdf::BdfBatch& zb)
{
    hipLaunchKernelGGL(bdf::sample_batch_kernel, dim3(blocks256(n), 1, cnt), dim3(256), 0, ctx->stream, bdf_arena_of(w, n).D, n, dteval, n_eval, dsmp, y_eval_dev, zb);
    LAUNCH_OK(ctx);
    return 0;
}

// ---- a sweep of BDF instances (marl_bdf_batch.h, marl_bdf_ctl.h) ---------------------------------------------------------------
// BDF.__init__ of every instance (f, the first Jacobian, D, the monitors) in front of the cycle, then the cycle of sweep_radau's
// launch-per-action mode: controllers, the list lengths (sweep_read_counts), then every kind of work over its list in the order
// marl_bdf_ctl.h documents - Jacobians and right-hand sides through the launchers the single runs use, the factorisation and the
// one-workgroup solve through the kernels of marl_bdf_batch.h.  No kernel waits for another workgroup.
// t_eval (host, n_eval times), y_eval_dev (device, [instance][n_eval][5N]), n_done (host, [instance]): the samples inside every accepted
// step by the step's dense output, built as bdf_run builds it - after the order / step-size selection, before the next step rescales D
// (A_SAMPLE, marl_bdf_ctl.h); n_eval = 0: none, and the same cycles.  A run with t1 == t0 takes no step and writes no frame.
// t_events (host, [instance][7][max_events]), max_events: the monitors' root times, located on the same dense output in front of the
// samples (A_ROOTS: roots_batch_kernel runs the whole search of a step's monitors in one launch) into a NaN-filled device buffer that
// comes back once at the end; NULL or max_events <= 0: sign changes are counted only, and neither the buffer nor the instances'
// BdfRoots exist - the kernels and cycles are those of the sweep without roots.
// terminal_ok: the entry honours ctx->terminal (marl_sweep_bdf_terminal_dev; the others refuse a context with limits).  With limits the
// instances get a BdfTerm each, the controllers are the TERM instantiations, and a cycle's work reads
//     A_ACCEPT  ->  A_CHANGE_D  ->  A_ROOTS / A_TERM_ROOTS  ->  A_SAMPLE  ->  A_STOP  ->  A_JAC  ->  A_LU  ->  A_SOLVE
// (marl_bdf_ctl.h); a stopped instance is PC_DONE and leaves BL_RUNNING, so the sweep ends with its last live instance.  Without limits
// nothing of this exists and the launches are those of the other entries.
static int sweep_bdf(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol, const int32_t* groups,
                     int64_t max_attempts, const double* t_eval, int64_t n_eval, double* y_eval_dev, int64_t* n_done, double* t_events,
                     int64_t max_events, marl_stats* stats, bool terminal_ok = false)
{
    if (!ctx || !y_dev || !stats) return ctx ? fail(ctx, -1, "marl_sweep_bdf_dev: invalid argument") : -1;
    if (n_eval < 0 || (n_eval > 0 && (!t_eval || !y_eval_dev || !n_done))) return fail(ctx, -1, "marl_sweep_bdf_eval_dev: invalid argument");
    if (!terminal_ok) { NO_TERMINAL(ctx, "marl_sweep_bdf_dev") }
    if (ctx->halo > 0) return fail(ctx, -1, "marl_sweep_bdf_dev: whole-grid context required");
    if (int rc = check_ivp_args(ctx, "bdf", t0, t1, first_step, rtol, atol, t_eval, n_eval)) return rc;
    const bool frames = n_eval > 0, locate = t_events && max_events > 0, term = has_terminal(ctx);
    if (ctx->batch > 65535) return fail(ctx, -1, "marl_sweep_bdf_dev: at most 65535 instances per call");
    const int64_t N = ctx->N, n = NF * N, B = ctx->batch;
    if (n > radau::PCR_FUSED_MAX)
        return fail(ctx, -1, "marl_sweep_bdf_dev: a solve must fit one workgroup (N <= %d); use marl_integrate_bdf (run_sweep_bdf without batched) for larger grids",
                    (int)(radau::PCR_FUSED_MAX / NF));
    if (ctx->radau_solver != 0) return fail(ctx, -1, "marl_sweep_bdf_dev: needs the PCR solver (option radau_solver = 0)");
    if (n_done) memset(n_done, 0, sizeof(int64_t) * (size_t)B);
    HIP_OK(ctx, hipSetDevice(ctx->device));
    rtol = clamp_rtol(rtol);
    RadauWork w;
    int64_t zs = 0;
    if (int rc = radau_alloc(ctx, w, groups, B, &zs)) return rc;
    if (w.cr_k && !w.plan.k) return fail(ctx, -1, "marl_sweep_bdf_dev: the cyclic-reduction levels of this context do not fit the one-launch solve");
    using bdf::BdfCtl;
    using namespace bdf;
    std::vector<BdfCtl> hctl((size_t)B);   // (before the device buffers: they wait for the stream when they go, this must still be there)
    for (auto& c : hctl) bdfctl::bdf_control_init(c, t0, t1, first_step, rtol, atol, max_attempts);
    std::vector<BdfSample> hsmp(frames ? (size_t)B : 0);
    for (auto& s : hsmp) bdfctl::bdf_sample_init(s, n_eval);
    std::vector<BdfRoots> hroots(locate ? (size_t)B : 0);
    for (auto& r : hroots) bdfctl::bdf_roots_init(r, max_events);
    std::vector<bdfctl::BdfTerm> hterm(term ? (size_t)B : 0);
    for (auto& m : hterm) bdfctl::bdf_term_init(m, ctx->terminal);
    const size_t tev_bytes = locate ? sizeof(double) * (size_t)B * 7 * (size_t)max_events : 0;
    DevBuf b_ctl(ctx->stream), b_rec(ctx->stream), b_counts(ctx->stream), b_smp(ctx->stream), b_teval(ctx->stream), b_roots(ctx->stream),
        b_tev(ctx->stream), b_term(ctx->stream);   // every return from here on frees them
    HIP_OK(ctx, b_ctl.alloc(sizeof(BdfCtl) * B));
    HIP_OK(ctx, b_rec.alloc(sizeof(double) * NQ * B));
    HIP_OK(ctx, b_counts.alloc(sizeof(int32_t) * (size_t)(radau::L_COUNT + BL_COUNT * B)));
    BdfCtl* const dctl = b_ctl.as<BdfCtl>();
    double* const drec = b_rec.as<double>();
    int32_t* const dcounts = b_counts.as<int32_t>();   // [L_COUNT] then lists [BL_COUNT][B]
    int32_t* dlists = dcounts + radau::L_COUNT;
    HIP_OK(ctx, hipMemcpyAsync(dctl, hctl.data(), sizeof(BdfCtl) * B, hipMemcpyHostToDevice, ctx->stream));
    if (frames) {   // the instances' t_eval states and the sample times (pageable host memory: the copies have left it when the calls return)
        HIP_OK(ctx, b_smp.alloc(sizeof(BdfSample) * B));
        HIP_OK(ctx, b_teval.alloc(sizeof(double) * (size_t)n_eval));
        HIP_OK(ctx, hipMemcpyAsync(b_smp.p, hsmp.data(), sizeof(BdfSample) * B, hipMemcpyHostToDevice, ctx->stream));
        HIP_OK(ctx, hipMemcpyAsync(b_teval.p, t_eval, sizeof(double) * (size_t)n_eval, hipMemcpyHostToDevice, ctx->stream));
    }
    if (locate) {   // the instances' root-location states and their root times, NaN (all bits set) until a root is stored
        HIP_OK(ctx, b_roots.alloc(sizeof(BdfRoots) * B));
        HIP_OK(ctx, b_tev.alloc(tev_bytes));
        HIP_OK(ctx, hipMemcpyAsync(b_roots.p, hroots.data(), sizeof(BdfRoots) * B, hipMemcpyHostToDevice, ctx->stream));
        HIP_OK(ctx, hipMemsetAsync(b_tev.p, 0xFF, tev_bytes, ctx->stream));
    }
    if (term) {   // the instances' terminal-monitor states
        HIP_OK(ctx, b_term.alloc(sizeof(bdfctl::BdfTerm) * B));
        HIP_OK(ctx, hipMemcpyAsync(b_term.p, hterm.data(), sizeof(bdfctl::BdfTerm) * B, hipMemcpyHostToDevice, ctx->stream));
    }
    BdfSample* const dsmp = b_smp.as<BdfSample>();
    const double* const dteval = b_teval.as<double>();
    BdfRoots* const droots = b_roots.as<BdfRoots>();
    double* const dtev = b_tev.as<double>();
    bdfctl::BdfTerm* const dterm = b_term.as<bdfctl::BdfTerm>();
    HIP_OK(ctx, hipMemcpy2DAsync(w.y, (size_t)zs, y_dev, n * sizeof(double), n * sizeof(double), (size_t)B, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_OK(ctx, hipMemsetAsync(dcounts, 0, sizeof(int32_t) * radau::L_COUNT, ctx->stream));   // (sweep_read_counts keeps them zero between cycles)
    bdf::Vec6 gamma = {};
    for (int k = 1; k <= bdf::MAX_ORDER; k++) gamma.v[k] = gamma.v[k - 1] + 1.0 / k;
    const BdfArena arena = bdf_arena_of(w, n);
    double *const D = arena.D, *const f = arena.f, *const ypred = arena.ypred, *const psi = arena.psi, *const d = arena.d;
    const dim3 b256(256);
    const int64_t nbm = std::min<int64_t>((N + 255) / 256, 1024);
    if (int rc = ensure_part(ctx, (size_t)(nbm * B))) return rc;
    auto L = [&](int which) { return BdfBatch{zs, dctl, dlists + (int64_t)which * B}; };
    auto Z = [&](int which) { return ZBatch{zs, nullptr, 0, 0, dlists + (int64_t)which * B}; };
    // BDF.__init__ of every instance: f = fun(t0, y0); J = jac(t0, y0) (no step-size factors yet); D[0] = y0, D[1] = f h; g = events(t0, y0)
    {
        const ZBatch all{zs, nullptr, 0, 0, nullptr};
        if (int rc = launch_rhs_fm(ctx, w.y, w.f, 1, (unsigned)B, all)) return rc;
        if (int rc = radau_num_jac(ctx, w, w.y, w.f, atol, 1, (unsigned)B, all)) return rc;
        if (int rc = bdf_launch_init_D(ctx, w, n, (unsigned)B, BdfBatch{zs, dctl, nullptr})) return rc;
        hipLaunchKernelGGL(monitors_kernel<LAYOUT_FIELD_MAJOR>, dim3((unsigned)nbm, (unsigned)B), b256, 0, ctx->stream, w.y, ctx->dconsts, ctx->slab, zs / 8, ctx->part);
        LAUNCH_OK(ctx);
        hipLaunchKernelGGL(reduce_records_kernel, dim3((unsigned)B), b256, 0, ctx->stream, ctx->part, nbm, drec);
        LAUNCH_OK(ctx);
    }
    int32_t* hcounts = reinterpret_cast<int32_t*>(ctx->rd_host);
    constexpr int64_t kStallCycles = 1000;   // cycles without any instance moving (pc, attempts, status): every cycle moves each running one
    int64_t stalled = 0;
    for (int64_t cycle = 0;; cycle++) {
        const dim3 gctl((unsigned)((B + 63) / 64)), bctl(64);
        double* const no_tev = nullptr;   // (the controllers without TERM store no root themselves)
        bdfctl::BdfTerm* const no_term = nullptr;
        if (term) {
            if (frames && locate) hipLaunchKernelGGL((bdf_control_kernel<true, true, true>), gctl, bctl, 0, ctx->stream, dctl, drec, B, n, dcounts, dlists, dsmp, dteval, droots, dterm, dtev);
            else if (locate) hipLaunchKernelGGL((bdf_control_kernel<false, true, true>), gctl, bctl, 0, ctx->stream, dctl, drec, B, n, dcounts, dlists, dsmp, dteval, droots, dterm, dtev);
            else if (frames) hipLaunchKernelGGL((bdf_control_kernel<true, false, true>), gctl, bctl, 0, ctx->stream, dctl, drec, B, n, dcounts, dlists, dsmp, dteval, droots, dterm, dtev);
            else hipLaunchKernelGGL((bdf_control_kernel<false, false, true>), gctl, bctl, 0, ctx->stream, dctl, drec, B, n, dcounts, dlists, dsmp, dteval, droots, dterm, dtev);
        }
        else if (frames && locate) hipLaunchKernelGGL((bdf_control_kernel<true, true, false>), gctl, bctl, 0, ctx->stream, dctl, drec, B, n, dcounts, dlists, dsmp, dteval, droots, no_term, no_tev);
        else if (locate) hipLaunchKernelGGL((bdf_control_kernel<false, true, false>), gctl, bctl, 0, ctx->stream, dctl, drec, B, n, dcounts, dlists, dsmp, dteval, droots, no_term, no_tev);
        else if (frames) hipLaunchKernelGGL((bdf_control_kernel<true, false, false>), gctl, bctl, 0, ctx->stream, dctl, drec, B, n, dcounts, dlists, dsmp, dteval, droots, no_term, no_tev);
        else hipLaunchKernelGGL((bdf_control_kernel<false, false, false>), gctl, bctl, 0, ctx->stream, dctl, drec, B, n, dcounts, dlists, dsmp, dteval, droots, no_term, no_tev);
        LAUNCH_OK(ctx);
        if (int rc = sweep_read_counts(ctx, dcounts, BL_COUNT, cycle, hcounts)) return rc;
        const unsigned nA = (unsigned)hcounts[BL_ACCEPT], nC = (unsigned)hcounts[BL_CHANGE_D], nJ = (unsigned)hcounts[BL_JAC], nL = (unsigned)hcounts[BL_LU],
                       nS = (unsigned)hcounts[BL_SOLVE], nP = (unsigned)hcounts[BL_SAMPLE], nR = (locate || term) ? (unsigned)hcounts[BL_ROOTS] : 0u,
                       nT = term ? (unsigned)hcounts[BL_STOP] : 0u;
        stalled = hcounts[BL_PROGRESS] ? 0 : stalled + 1;
        if (stalled >= kStallCycles)
            return fail(ctx, -3, "marl_sweep_bdf_dev: no instance moved for %lld cycles (%d still running)", (long long)kStallCycles, (int)hcounts[BL_RUNNING]);
        if (nA)   // the accepted step: differences, y = y_new, the norms of the order selection
            if (int rc = bdf_launch_accept_norms(ctx, w, n, nA, L(BL_ACCEPT))) return rc;
        if (nC)
            if (int rc = bdf_launch_change_D(ctx, w, n, nC, L(BL_CHANGE_D))) return rc;
        if (nR)   // root times of the step just accepted: the same D as the samples below, events first (ivp.py:673-723)
            if (int rc = bdf_launch_roots(ctx, w, N, droots, dtev, nR, L(BL_ROOTS), dterm)) return rc;   // (with limits: a terminal step's roots too)
        if (nP)   // t_eval samples of the step just accepted: D after the selection's rescaling, before the next step's
            if (int rc = bdf_launch_sample(ctx, w, n, dteval, n_eval, dsmp, y_eval_dev, nP, L(BL_SAMPLE))) return rc;
        if (nT)   // a terminal monitor ended these runs inside the step just accepted: the dense output at t_stop is their state
            if (int rc = bdf_launch_stop_state(ctx, w, N, dterm, nT, L(BL_STOP))) return rc;
        if (nJ) {   // J = jac(t_new, y_predict), with f = fun(t_new, y_predict) (not counted)
            if (int rc = launch_rhs_fm(ctx, ypred, w.fnew, 1, nJ, Z(BL_JAC))) return rc;
            if (int rc = radau_num_jac(ctx, w, ypred, w.fnew, atol, 0, nJ, Z(BL_JAC))) return rc;
        }
        if (nL) {   // LU of I - c J (pcr_factor_launch, real system)
            if (w.cr_k) {
                hipLaunchKernelGGL(cr_init_batch_kernel, dim3(pcr_groups((N + 1) / 2), 1, nL), b256, 0, ctx->stream, w.J, N, w.Cr, L(BL_LU));
                LAUNCH_OK(ctx);
                for (int l = 0; l < w.cr_k; l++) {
                    const radau::CrShape sh{w.cr_n[l], w.cr_off[l], w.cr_n[l + 1], w.cr_off[l + 1]};
                    hipLaunchKernelGGL(cr_reduce_batch_kernel, dim3(pcr_groups(sh.n_next), 1, nL), b256, 0, ctx->stream, w.Cr, sh, l + 1 == w.cr_k ? 1 : 0, w.Sr, L(BL_LU));
                    LAUNCH_OK(ctx);
                }
                const int64_t M = w.cr_n[w.cr_k];
                for (int level = 0; level < w.nlevels; level++) {
                    hipLaunchKernelGGL(pcr_factor_batch_kernel, dim3(pcr_groups(M), 1, nL), b256, 0, ctx->stream, w.J, M, level, w.Sr, L(BL_LU));
                    LAUNCH_OK(ctx);
                }
            } else {
                for (int level = -1; level < w.nlevels; level++) {
                    hipLaunchKernelGGL(pcr_factor_batch_kernel, dim3(pcr_groups(N), 1, nL), b256, 0, ctx->stream, w.J, N, level, w.Sr, L(BL_LU));
                    LAUNCH_OK(ctx);
                }
            }
        }
        if (nS) {   // solve_bdf_system: one workgroup per instance
            if (ctx->var_dphi)
                hipLaunchKernelGGL(solve_batch_kernel<true>, dim3(1, 1, nS), dim3(radau::WG_THREADS), 0, ctx->stream, D, gamma, ypred, psi, w.scale, w.ynew, d, f, N, w.nlevels,
                                   w.Sr, ctx->dconsts, w.plan, w.Cr, L(BL_SOLVE));
            else
                hipLaunchKernelGGL(solve_batch_kernel<false>, dim3(1, 1, nS), dim3(radau::WG_THREADS), 0, ctx->stream, D, gamma, ypred, psi, w.scale, w.ynew, d, f, N, w.nlevels,
                                   w.Sr, ctx->dconsts, w.plan, w.Cr, L(BL_SOLVE));
            LAUNCH_OK(ctx);
        }
        if (hcounts[BL_RUNNING] == 0) break;   // (the last cycle's accepted steps are launched above)
    }
    // results (the synchronise is also what the sweep's buffers wait for before they go)
    HIP_OK(ctx, hipMemcpy2DAsync(y_dev, n * sizeof(double), w.y, (size_t)zs, n * sizeof(double), (size_t)B, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_OK(ctx, hipMemcpyAsync(hctl.data(), dctl, sizeof(BdfCtl) * B, hipMemcpyDeviceToHost, ctx->stream));
    if (frames) HIP_OK(ctx, hipMemcpyAsync(hsmp.data(), dsmp, sizeof(BdfSample) * B, hipMemcpyDeviceToHost, ctx->stream));
    if (locate) HIP_OK(ctx, hipMemcpyAsync(t_events, dtev, tev_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
    for (int64_t b = 0; b < B; b++) {
        ctl_to_stats(hctl[(size_t)b], stats[b]);
        if (frames) n_done[b] = hsmp[(size_t)b].next;
    }
    return 0;
}

extern "C" int marl_sweep_bdf_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol,
                                  const int32_t* groups, int64_t max_attempts, marl_stats* stats)
{
    return sweep_bdf(ctx, y_dev, t0, t1, first_step, rtol, atol, groups, max_attempts, nullptr, 0, nullptr, nullptr, nullptr, 0, stats);
}

extern "C" int marl_sweep_bdf_eval_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol,
                                       const int32_t* groups, int64_t max_attempts, const double* t_eval, int64_t n_eval, double* y_eval_dev,
                                       int64_t* n_done, marl_stats* stats)
{
    return sweep_bdf(ctx, y_dev, t0, t1, first_step, rtol, atol, groups, max_attempts, t_eval, n_eval, y_eval_dev, n_done, nullptr, 0, stats);
}

extern "C" int marl_sweep_bdf_events_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol,
                                         const int32_t* groups, int64_t max_attempts, const double* t_eval, int64_t n_eval, double* y_eval_dev,
                                         int64_t* n_done, double* t_events, int64_t max_events, marl_stats* stats)
{
    return sweep_bdf(ctx, y_dev, t0, t1, first_step, rtol, atol, groups, max_attempts, t_eval, n_eval, y_eval_dev, n_done, t_events, max_events, stats);
}

extern "C" int marl_sweep_bdf_terminal_dev(marl_ctx* ctx, double* y_dev, double t0, double t1, double first_step, double rtol, double atol,
                                           const int32_t* groups, int64_t max_attempts, const double* t_eval, int64_t n_eval, double* y_eval_dev,
                                           int64_t* n_done, double* t_events, int64_t max_events, marl_stats* stats)
{
    return sweep_bdf(ctx, y_dev, t0, t1, first_step, rtol, atol, groups, max_attempts, t_eval, n_eval, y_eval_dev, n_done, t_events, max_events, stats, true);
}

// ---- test hook of the BDF sweep's vector kernels: ONE launch (tests/test_gpu_bdf_batch_parts.py) ------------------------------------
// The sweep's arena (radau_alloc with the context's instances: the real stride), each instance's BdfCtl / BdfSample / BdfRoots built
// here from plain scalars, one launch through the launcher sweep_bdf calls, and everything the kernel may write - with its
// surroundings - back to the host.  Every argument a kernel would index with is checked first: nothing out of range reaches the device.
extern "C" int marl_debug_bdf_batch(marl_ctx* ctx, int op, const int32_t* list, int64_t n_list, const int64_t* iargs, const double* dargs,
                                    const double* D_in, const double* vec_in, const double* t_eval, int64_t n_eval, int64_t max_events,
                                    double* D_out, double* y_out, double* frames, double* t_events, double* ss)
{
    using namespace bdf;
    if (!ctx || !iargs || !dargs || !D_in || !vec_in || !D_out || !y_out || !ss) return ctx ? fail(ctx, -1, "marl_debug_bdf_batch: invalid argument") : -1;
    if (op < MARL_BDF_INIT_D || op > MARL_BDF_STOP) return fail(ctx, -1, "marl_debug_bdf_batch: unknown op %d", op);
    if (ctx->halo > 0) return fail(ctx, -1, "marl_debug_bdf_batch: whole-grid context required");
    if (ctx->batch > 65535) return fail(ctx, -1, "marl_debug_bdf_batch: at most 65535 instances per call");
    const int64_t N = ctx->N, n = NF * N, B = ctx->batch;
    if (n > radau::PCR_FUSED_MAX) return fail(ctx, -1, "marl_debug_bdf_batch: the BDF sweep takes N <= %d", (int)(radau::PCR_FUSED_MAX / NF));
    if (list ? (n_list < 1 || n_list > B) : n_list != 0) return fail(ctx, -1, "marl_debug_bdf_batch: a list holds 1 .. %lld instances (no list: n_list = 0)", (long long)B);
    for (int64_t k = 0; list && k < n_list; k++)
        if (list[k] < 0 || list[k] >= B) return fail(ctx, -1, "marl_debug_bdf_batch: list entry %lld = %d is no instance", (long long)k, (int)list[k]);
    if (n_eval < 0 || (n_eval > 0 && (!t_eval || !frames))) return fail(ctx, -1, "marl_debug_bdf_batch: n_eval samples need t_eval and frames");
    if (max_events < 0 || (max_events > 0 && !t_events)) return fail(ctx, -1, "marl_debug_bdf_batch: max_events root slots need t_events");
    if (op == MARL_BDF_ROOTS && max_events <= 0) return fail(ctx, -1, "marl_debug_bdf_batch: ROOTS needs max_events > 0");
    if (op == MARL_BDF_STOP && max_events <= 0) return fail(ctx, -1, "marl_debug_bdf_batch: STOP needs max_events > 0 (the monitors come back in slot 0)");
    std::vector<BdfCtl> hctl((size_t)B);   // (before the device buffers, as in sweep_bdf)
    std::vector<BdfSample> hsmp((size_t)B);
    std::vector<BdfRoots> hroots((size_t)B);
    std::vector<BdfTerm> hterm((size_t)B);
    for (int64_t b = 0; b < B; b++) {
        const int64_t* ia = iargs + b * MARL_BDF_DEBUG_INTS;
        const double* da = dargs + b * MARL_BDF_DEBUG_DOUBLES;
        const int64_t order = ia[0], want = ia[1], first = ia[2], end = ia[3], mask = ia[4];
        if (op != MARL_BDF_INIT_D && (order < 1 || order > MAX_ORDER)) return fail(ctx, -1, "marl_debug_bdf_batch: instance %lld: order %lld outside 1 .. 5", (long long)b, (long long)order);
        if (want < 0 || want > 3) return fail(ctx, -1, "marl_debug_bdf_batch: instance %lld: want_norms outside 0 .. 3", (long long)b);
        if (first < 0 || first > end) return fail(ctx, -1, "marl_debug_bdf_batch: instance %lld: samples [first, end) need 0 <= first <= end", (long long)b);
        if (mask < 0 || mask > 127) return fail(ctx, -1, "marl_debug_bdf_batch: instance %lld: mask outside 0 .. 127", (long long)b);
        BdfCtl& c = hctl[(size_t)b];
        bdfctl::bdf_control_init(c, 0.0, 1.0, da[0], da[1], da[2], 0);
        c.order = c.ru_order = (int32_t)order;
        c.want_norms = (int32_t)want;
        c.err_coef_m = da[3]; c.err_coef_p = da[4];
        for (int j = 0; j <= MAX_ORDER; j++)
            for (int k = 0; k <= MAX_ORDER; k++) c.RU[j][k] = da[7 + j * (MAX_ORDER + 1) + k];
        c.ss_m = ss[2 * b]; c.ss_p = ss[2 * b + 1];
        BdfSample& s = hsmp[(size_t)b];
        bdfctl::bdf_sample_init(s, n_eval);
        s.t = da[5]; s.h = da[0]; s.order = (int32_t)order; s.first = first; s.end = end;
        BdfRoots& r = hroots[(size_t)b];
        bdfctl::bdf_roots_init(r, max_events);
        r.t_old = da[6]; r.t = da[5]; r.h = da[0]; r.order = (int32_t)order; r.mask = (int32_t)mask;
        BdfTerm& m = hterm[(size_t)b];   // STOP: the terminal step's snapshot; da[6] is t_stop
        bdfctl::bdf_term_init(m, ctx->terminal);
        m.t = da[5]; m.h = da[0]; m.order = (int32_t)order; m.t_stop = da[6];
        for (int e = 0; e < 7; e++) {
            r.slot[e] = ia[5 + e];
            if (op == MARL_BDF_ROOTS && ((mask >> e) & 1) && (r.slot[e] < 0 || r.slot[e] >= max_events))
                return fail(ctx, -1, "marl_debug_bdf_batch: instance %lld: slot of monitor %d outside [0, max_events)", (long long)b, e);
        }
    }
    HIP_OK(ctx, hipSetDevice(ctx->device));
    RadauWork w;
    int64_t zs = 0;
    if (int rc = radau_alloc(ctx, w, nullptr, B, &zs)) return rc;
    const size_t nb = (size_t)n * sizeof(double), fr_bytes = (size_t)B * (size_t)n_eval * nb, tev_bytes = sizeof(double) * (size_t)B * 7 * (size_t)max_events;
    DevBuf b_ctl(ctx->stream), b_smp(ctx->stream), b_roots(ctx->stream), b_list(ctx->stream), b_teval(ctx->stream), b_fr(ctx->stream), b_tev(ctx->stream),
        b_term(ctx->stream);
    HIP_OK(ctx, b_ctl.alloc(sizeof(BdfCtl) * B));
    HIP_OK(ctx, b_smp.alloc(sizeof(BdfSample) * B));
    HIP_OK(ctx, b_roots.alloc(sizeof(BdfRoots) * B));
    HIP_OK(ctx, hipMemcpyAsync(b_ctl.p, hctl.data(), sizeof(BdfCtl) * B, hipMemcpyHostToDevice, ctx->stream));
    HIP_OK(ctx, hipMemcpyAsync(b_smp.p, hsmp.data(), sizeof(BdfSample) * B, hipMemcpyHostToDevice, ctx->stream));
    HIP_OK(ctx, hipMemcpyAsync(b_roots.p, hroots.data(), sizeof(BdfRoots) * B, hipMemcpyHostToDevice, ctx->stream));
    if (op == MARL_BDF_STOP) {
        HIP_OK(ctx, b_term.alloc(sizeof(BdfTerm) * B));
        HIP_OK(ctx, hipMemcpyAsync(b_term.p, hterm.data(), sizeof(BdfTerm) * B, hipMemcpyHostToDevice, ctx->stream));
    }
    if (list) {
        HIP_OK(ctx, b_list.alloc(sizeof(int32_t) * (size_t)n_list));
        HIP_OK(ctx, hipMemcpyAsync(b_list.p, list, sizeof(int32_t) * (size_t)n_list, hipMemcpyHostToDevice, ctx->stream));
    }
    if (n_eval > 0) {
        HIP_OK(ctx, b_teval.alloc(sizeof(double) * (size_t)n_eval));
        HIP_OK(ctx, b_fr.alloc(fr_bytes));
        HIP_OK(ctx, hipMemcpyAsync(b_teval.p, t_eval, sizeof(double) * (size_t)n_eval, hipMemcpyHostToDevice, ctx->stream));
        HIP_OK(ctx, hipMemcpyAsync(b_fr.p, frames, fr_bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    if (max_events > 0) {
        HIP_OK(ctx, b_tev.alloc(tev_bytes));
        HIP_OK(ctx, hipMemcpyAsync(b_tev.p, t_events, tev_bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    const BdfArena a = bdf_arena_of(w, n);
    auto at = [&](double* p, int64_t b) { return reinterpret_cast<double*>(reinterpret_cast<char*>(p) + b * zs); };   // p of instance b
    for (int64_t b = 0; b < B; b++) {
        const double* v = vec_in + b * 4 * n;   // y, f, d, ynew
        HIP_OK(ctx, hipMemcpyAsync(at(a.D, b), D_in + b * 8 * n, 8 * nb, hipMemcpyHostToDevice, ctx->stream));
        HIP_OK(ctx, hipMemcpyAsync(at(w.y, b), v, nb, hipMemcpyHostToDevice, ctx->stream));
        HIP_OK(ctx, hipMemcpyAsync(at(w.f, b), v + n, nb, hipMemcpyHostToDevice, ctx->stream));
        HIP_OK(ctx, hipMemcpyAsync(at(a.d, b), v + 2 * n, nb, hipMemcpyHostToDevice, ctx->stream));
        HIP_OK(ctx, hipMemcpyAsync(at(w.ynew, b), v + 3 * n, nb, hipMemcpyHostToDevice, ctx->stream));
    }
    const BdfBatch zb{zs, b_ctl.as<BdfCtl>(), list ? b_list.as<int32_t>() : nullptr};
    const unsigned cnt = (unsigned)(list ? n_list : B);
    int rc = 0;
    if (op == MARL_BDF_INIT_D) rc = bdf_launch_init_D(ctx, w, n, cnt, zb);
    else if (op == MARL_BDF_CHANGE_D) rc = bdf_launch_change_D(ctx, w, n, cnt, zb);
    else if (op == MARL_BDF_ACCEPT_NORMS) rc = bdf_launch_accept_norms(ctx, w, n, cnt, zb);
    else if (op == MARL_BDF_SAMPLE) rc = bdf_launch_sample(ctx, w, n, b_teval.as<double>(), n_eval, b_smp.as<BdfSample>(), b_fr.as<double>(), cnt, zb);
    else if (op == MARL_BDF_ROOTS) rc = bdf_launch_roots(ctx, w, N, b_roots.as<BdfRoots>(), b_tev.as<double>(), cnt, zb);
    else rc = bdf_launch_stop_state(ctx, w, N, b_term.as<BdfTerm>(), cnt, zb);
    if (rc) return rc;
    for (int64_t b = 0; b < B; b++) {
        HIP_OK(ctx, hipMemcpyAsync(D_out + b * 8 * n, at(a.D, b), 8 * nb, hipMemcpyDeviceToHost, ctx->stream));
        HIP_OK(ctx, hipMemcpyAsync(y_out + b * n, at(w.y, b), nb, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_OK(ctx, hipMemcpyAsync(hctl.data(), b_ctl.p, sizeof(BdfCtl) * B, hipMemcpyDeviceToHost, ctx->stream));
    if (n_eval > 0) HIP_OK(ctx, hipMemcpyAsync(frames, b_fr.p, fr_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (max_events > 0) HIP_OK(ctx, hipMemcpyAsync(t_events, b_tev.p, tev_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
    for (int64_t b = 0; b < B; b++) { ss[2 * b] = hctl[(size_t)b].ss_m; ss[2 * b + 1] = hctl[(size_t)b].ss_p; }
    if (op == MARL_BDF_STOP)   // the monitors of the listed instances' stop states (ctl.g; the kernel has no root slot to write)
        for (int64_t k = 0; k < (list ? n_list : B); k++) {
            const int64_t b = list ? list[k] : k;
            for (int e = 0; e < 7; e++) t_events[(b * 7 + e) * max_events] = hctl[(size_t)b].g[e];
        }
    return 0;
}

#endif  // MARL_LAB
