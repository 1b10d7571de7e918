// marl_kernels.h - HIP kernels for the five-field RHS and the fused explicit RK time loops (gfx950).
//
// Work decomposition (all kernels): a workgroup of BLK threads owns a WINDOW of BLK consecutive
// depth cells, ONE cell per thread, all five fields of the cell in that thread's registers.  A
// Runge-Kutta stage needs u[i-1], u[i], u[i+1] of the current STAGE state: every thread publishes
// its cell through a double-buffered LDS edge array and reads its two neighbours' (one barrier per
// stage).  Stage vectors K1..Ks never leave registers.  A window is wider than the cells it finally
// writes by H cells per side; every RHS evaluation invalidates one more cell at each window edge
// (the halo is recomputed, never communicated), so one launch can advance several stages - a whole
// RK4 step, NSTEPS RK4 steps, or a whole Dormand-Prince attempt - with ONE read and ONE write of the
// state: 80 algorithmic bytes per grid-point-step.  Physical boundaries (global cell 0 / N-1) use
// the ghost-cell rules instead of a halo and are therefore always valid.
//
// Why only this shape: two others were built, measured and lost.  Several cells per thread (a
// cells-per-thread template parameter on every kernel here): 2 cells per thread was no faster at any grid size
// (profiles/r01_lab_reuse_experiments.log).  A one-wave window whose neighbours come
// from DPP lane shifts instead of LDS, with no barrier (BLK = 64): 3.3 - 3.8 us per
// additional step at N = 65 536 against 3.64 us for the 256-thread / 16-step kernel - a lone wave
// of this instruction stream issues one VALU instruction per ~12 cycles with or without the
// exchange (profiles/r03_lab_n65536.log).  Neither was ever shipped or tested; their code is in the
// history at the parent of the commit that removed them.
//
// State layouts (`LAYOUT`):
//   FIELD_MAJOR  y[f*ld + i]                         the reference's layout (Evolve_scenario.py:64-65)
//   TILED        y[(i>>6)*320 + f*64 + (i&63)]       five 512-byte field rows interleaved per 64-cell
//                                                    tile: one window = one contiguous 40*BLK-byte run
#pragma once
#include <type_traits>

#include "marl_math.h"
#include "marl_brent.h"
#include "marl_rk_ctrl.h"
#include "marl_rk_terminal.h"

namespace marl {

enum : int { LAYOUT_FIELD_MAJOR = 0, LAYOUT_TILED = 1 };

template <int LAYOUT>
__device__ __forceinline__ int64_t at(int f, int64_t i, int64_t ld)
{
    if constexpr (LAYOUT == LAYOUT_FIELD_MAJOR)
        return (int64_t)f * ld + i;
    else
        return (i >> 6) * (int64_t)(NF * 64) + f * 64 + (i & 63);
}

// A contiguous piece of the global grid held in one buffer: local cell l is global cell l + goff.
// Single-GPU runs: n_buf = N, goff = 0.  Domain decomposition: the buffer carries exchanged halo
// cells on interior sides.
struct Slab {
    int64_t n_buf;   // cells in the buffer
    int64_t goff;    // global index of local cell 0
    int64_t ld;      // field stride of FIELD_MAJOR buffers (>= n_buf)
    int64_t out_lo;  // local cells [out_lo, out_hi) are written by fused kernels
    int64_t out_hi;
};

__device__ __forceinline__ double nanmin(double a, double b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ double nanmax(double a, double b) { return (a > b || a != a) ? a : b; }
// FINITE: the caller only uses the result when every input is finite (the monitors of an ACCEPTED Dormand-Prince attempt: a
// non-finite y_new, f(y_new), U or W makes the error norm NaN and the attempt is rejected; its record is never read) - plain
// v_min_f64 / v_max_f64 then (one instruction instead of the four of a NaN-propagating select; np.min / np.max agree with them
// on finite values).
template <bool FINITE = false>
__device__ __forceinline__ double mon_min(double a, double b) { return FINITE ? __builtin_fmin(a, b) : nanmin(a, b); }
template <bool FINITE = false>
__device__ __forceinline__ double mon_max(double a, double b) { return FINITE ? __builtin_fmax(a, b) : nanmax(a, b); }

// ---------------------------------------------------------------------------------------------
// Per-block stencil engine
// ---------------------------------------------------------------------------------------------
// REUSE = false: no transcendental cache (one-workgroup sweeps on coarse grids, where the stage displacements
// are far outside the expansions' range).  The cache (marl_math.h, PointCache) also needs its LDS slots to fit
// the 64 KB a workgroup may declare: the wide blocks (512 threads and more) run without it.
// VD: the time-varying porosity diffusion coefficient (marl_params.dPhi_variable), see marl_math.h.

#ifdef MARL_LAB_PHASE_CLOCK   // kernel-lab build only (tools/rk4_lab.hip): shader-clock cycles per phase of an RHS evaluation, summed over every
// evaluation of wave 0 of every workgroup: [0] edge writes, [1] own-cell phase (point_local), [2] wait at the exchange barrier, [3] neighbour
// reads + boundary branch + stencil phase (point_rates), [4] between evaluations (RK combination, loads, stores), [5] evaluations counted
__device__ unsigned long long marl_lab_phase[8];
#define MARL_PHASE_MARK(k) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); ph_acc[k] += t_ - ph_last; ph_last = t_; } while (0)
#else
#define MARL_PHASE_MARK(k) do { } while (0)
#endif

// A loop of ONE trip - for the optimiser, not for the reader.  It stands wherever this file used to loop over the cells of a thread
// around something other than plain arithmetic: the two phases of an evaluation, and the guarded loads and stores of the kernels.  With
// one cell per thread those loops have no meaning left, but the compiler had been using them: as long as the (later fully unrolled) loop
// exists, loop-invariant code motion lifts np.sign(W) of the three Peclet weights (marl_math.h, fv_sigma) out of their branches, where
// value numbering merges them; the physical-boundary branch is laid out without copies on the path that skips it; and the guards keep
// their polarity and block order, on which the register allocation of the kernels at their cap turns.  Without any of them the fixed-step
// headline ran 2.1 % slower, N = 65 536 4 %, rk45_single 0.8 %, and rk45_sweep_events_kernel<1024, dPhi_variable> spilled 8 B more; with
// them every kernel compiles to the machine code it had with the cell loops (profiles/r06_one_cell_per_thread_isa.log).  Nothing but
// that comparison and the literal-move bounds of tests/test_hot_path_isa.py guards this: after a compiler change, build with and without
// and keep what measures better.
#define MARL_ONCE _Pragma("unroll") for (int once_ = 0; once_ < 1; once_++)
// the five fields of a cell, unrolled (the Runge-Kutta combinations)
#define MARL_FIELDS _Pragma("unroll") for (int f = 0; f < NF; f++)

// SEAM (rk4_chain_kernel only; 0 = none, and then nothing of it exists): the lane whose stage state is recorded at every evaluation
// for the next window of a chain, whose thread 0 takes its left neighbour from that record instead of from a recomputed halo.
// XCH (rk4_exchange_kernel only; 0 = what every other kernel has): how the exchange buffer and the cache slots lie in LDS.
//   XCH_CELL   the exchange buffer by cell, [parity][thread][6 doubles] (the five fields and one pad double: a pitch of 48 bytes),
//              instead of by field, [parity][field][thread].  By field a cell's values lie 2 KB apart and the compiler pairs their
//              accesses into two-address forms (ds_read2st64_b64: 128 B/clk); by cell they are 16-byte accesses (ds_read_b128:
//              256 B/clk).  Banks: lane l starts at dword 12 l, bank 4 (3 l mod 16) - 3 is invertible mod 16, so the 16 lanes that a
//              128-bit read serves per pass cover the 64 banks once, and the 8 lanes of a 128-bit write pass the 32 store banks once.
//   XCH_PAIRS  the four LDS cache slots as two pairs, [pair][thread][2] (marl_math.h, PointCache): two 16-byte reads per evaluation.
// The same bytes and values in the same order of use either way: nothing but LDS addresses differs.
enum : int { XCH_CELL = 1, XCH_PAIRS = 2 };
template <int BLK, bool REUSE = true, bool VD = false, int SEAM = 0, int XCH = 0>
struct StencilBlock {
    static constexpr bool CELL = (XCH & XCH_CELL) != 0, PAIRS = (XCH & XCH_PAIRS) != 0;
    static constexpr int PITCH = NF + 1;                    // CELL: doubles between the cells of the exchange buffer
    static constexpr int EDGE_DOUBLES = 2 * (CELL ? PITCH : NF) * BLK;       // edges [parity][field][thread] (CELL: [parity][thread][PITCH])
    static constexpr bool CACHE_LDS = PC_LDS_SLOTS > 0;
    static constexpr bool CACHE = REUSE && (EDGE_DOUBLES + TABLE_DOUBLES + PC_LDS_SLOTS * BLK) * 8 <= 60 * 1024;
    static constexpr int CACHE_DOUBLES = CACHE ? PC_LDS_SLOTS * BLK : 0;
    static constexpr int LDS_DOUBLES = EDGE_DOUBLES + TABLE_DOUBLES + CACHE_DOUBLES;  // edges, log/exp tables, cache slots [slot][thread]

    double* lds;
    Tables T;
    HotConsts K;                 // hot constants, in registers for the whole kernel
    const DevConsts* C;          // full constant block (cold members are read on rare paths only)
    int tid;
    int parity;
    // the thread's cell is global cell 0 (bit 0) / global cell N-1 (bit 8) / in the dissolution zone (bit 16): ONE register
    // instead of three (it lives across every stage, and the fused integrators sit at their register cap)
    unsigned masks;
    // wave-uniform: set when the cell of SOME lane of the wave is global cell 0 or N-1 (the ballot of is_edge(), taken
    // once per window: re-taken in every evaluation it rebuilt a lane mask in vector registers - two VALU instructions per stage).
    // Only where the transcendental cache is (the fine-grid kernels): in the 1024-thread one-workgroup sweeps, one more value carried
    // through the kernel grows the scratch spill of rk45_sweep_kernel (184 -> 192 B); they keep the ballot per evaluation
    static constexpr bool EDGE_ONCE = CACHE;
    unsigned edge_cells;
    __device__ __forceinline__ bool edge_wave() const
    {
        if constexpr (SEAM > 0) {   // (tested where it is used, on an opaque copy: hoisted out of the step loop the test becomes a lane mask - a pair, spilled)
            unsigned e = edge_cells;
            asm volatile("" : "+s"(e));
            return e & 1u;
        } else if constexpr (EDGE_ONCE) return edge_cells & 1u;
        else return __builtin_amdgcn_ballot_w64(is_edge() != 0) != 0;
    }
    // SEAM (rk4_chain_kernel): the three bits as three flags instead - an interior window sets them on the scalar side (set_interior), and
    // merged with a packed word they would be unpacked again per lane in every window
    bool w_zone = false;
    // (SEAM: compared where they are asked for, inside the boundary branch, on an opaque copy of the word - formed in front of the step
    // loop the two compares are lane masks, two pairs carried and spilled across every stage for a branch one wave of the grid takes)
    __device__ __forceinline__ unsigned edge_word() const { unsigned e = edge_cells; asm volatile("" : "+s"(e)); return e; }
    __device__ __forceinline__ unsigned is_first() const { if constexpr (SEAM > 0) return (unsigned)tid + 1u == ((edge_word() >> 8) & 0x1ffu); else return masks & 1u; }
    __device__ __forceinline__ unsigned is_last() const { if constexpr (SEAM > 0) return (unsigned)tid + 1u == ((edge_word() >> 20) & 0x1ffu); else return (masks >> 8) & 1u; }
    __device__ __forceinline__ unsigned in_zone() const { if constexpr (SEAM > 0) return w_zone; else return (masks >> 16) & 1u; }
    __device__ __forceinline__ unsigned is_edge() const { return masks & 0x101u; }   // first or last: non-zero
    static_assert(XCH == 0 || (CACHE && PC_LDS_SLOTS == 4 && (EDGE_DOUBLES + TABLE_DOUBLES) % 2 == 0), "XCH: 16-byte accesses, two pairs of cache slots");
    PointCache<(CACHE && CACHE_LDS) ? BLK : 0, PAIRS> cache;  // centre of the transcendental expansions (TR_FILL / TR_REUSE / TR_AUTO)
    __device__ __forceinline__ double* cache_slots(double* l, int t) const { return l + EDGE_DOUBLES + TABLE_DOUBLES + (PAIRS ? 2 * t : t); }
    bool reuse_live = false;     // wave-uniform: the centre is filled and no evaluation since has fallen out of range
    // SEAM: the record in LDS, [evaluation][parity][8 doubles, NF used], and - ONE scalar register, the loop sits at its cap of those too -
    // where the current evaluation writes in it (bits 0-15: 16 * evaluation + 8 * parity; the other parity is what it reads) and whether
    // it reads at all (SEAM_READS: not in a window with a left halo of its own), and whether this is the workgroup's wave 0 (SEAM_WAVE0:
    // its thread 0 reads) or the recording lane's wave (SEAM_WAVEW)
    static constexpr int SEAM_STRIDE = 16, SEAM_READS = 0x10000, SEAM_WAVE0 = 0x20000, SEAM_WAVEW = 0x40000;
    static_assert(SEAM < BLK, "the recording lane is a lane of the window");
    double* seam = nullptr;
    int seam_pos = 0;
#ifdef MARL_LAB_PHASE_CLOCK
    unsigned long long ph_acc[6] = {0, 0, 0, 0, 0, 0}, ph_last = __builtin_amdgcn_s_memtime();
    __device__ __forceinline__ void phase_flush()
    {
        if (threadIdx.x == 0)
            for (int k = 0; k < 6; k++) atomicAdd(&marl_lab_phase[k], ph_acc[k]);
    }
#endif

    // lds: LDS_DOUBLES doubles = edge exchange buffers followed by the log/exp tables (copied here; barrier inside).
    // g0: global index of this thread's cell.
    __device__ __forceinline__ StencilBlock(double* lds_, int64_t g0, const DevConsts* __restrict__ c)
        : lds(lds_), T(load_tables(lds_ + EDGE_DOUBLES, BLK)), K(load_hot(c)), C(c), tid(threadIdx.x), parity(0)
    {
        if constexpr (SEAM > 0) set_interior(false);   // (every window sets its own)
        else set_window(g0);
        if constexpr (CACHE && CACHE_LDS) cache.s = cache_slots(lds_, tid);
    }

    // Persistent kernels: the per-thread members again, from an index the caller has made opaque inside its work loop - everything
    // derived from the thread index is then recomputed per work item (a few instructions) instead of being hoisted out of the loop and
    // kept in (or spilled from) vector registers across it.
    __device__ __forceinline__ void rebind(int t)
    {
        tid = t;
        if constexpr (CACHE && CACHE_LDS) cache.s = cache_slots(lds, t);
    }

    // (Re)position the window: g = global index of this thread's cell.
    __device__ __forceinline__ void set_window(int64_t g)
    {
        const int64_t N = C->N, mlo = C->mask_lo, mhi = C->mask_hi;
        masks = ((g == 0) ? 1u : 0u) | ((g == N - 1) ? 0x100u : 0u) | ((g >= mlo && g < mhi) ? 0x10000u : 0u);
        edge_cells = 0;
        if constexpr (EDGE_ONCE) edge_cells = (__builtin_amdgcn_ballot_w64(is_edge() != 0) != 0) ? 1u : 0u;
    }

    // SEAM: the same from the scalar side.  gw: global index of the cell of the window's thread 0 (wave-uniform).  The one word says
    // whether this WAVE holds a boundary cell (bit 0, what set_window's ballot gives) and which thread of the window sits on cell 0
    // (bits 8-16: 1 + thread, 0 = none) and on cell N - 1 (bits 20-28): the stages carry one scalar register for the two boundary
    // cells of the grid instead of two lane masks, and the lanes are told apart only inside the branch that one wave of the grid takes.
    __device__ __forceinline__ void set_window_seam(int64_t gw)
    {
        const int64_t N = C->N, mlo = C->mask_lo, mhi = C->mask_hi;
        const int64_t g = gw + tid;
        w_zone = g >= mlo && g < mhi;
        masks = 0;
        const int wave = __builtin_amdgcn_readfirstlane(tid) >> 6;
        const int64_t t0 = -gw, t1 = N - 1 - gw;   // the threads on cell 0 and on cell N - 1
        unsigned e = 0;
        if (t0 >= 0 && t0 < BLK) e |= (((unsigned)t0 + 1u) << 8) | ((int)(t0 >> 6) == wave ? 1u : 0u);
        if (t1 >= 0 && t1 < BLK) e |= (((unsigned)t1 + 1u) << 20) | ((int)(t1 >> 6) == wave ? 1u : 0u);
        edge_cells = __builtin_amdgcn_readfirstlane(e);
    }

    // SEAM: a window that holds neither cell 0 nor cell N - 1 and lies wholly inside (zone) or wholly outside the dissolution zone -
    // what set_window gives for every lane of it, without a per-lane instruction.  `zone` is wave-uniform.
    __device__ __forceinline__ void set_interior(bool zone)
    {
        w_zone = zone;
        masks = 0;
        edge_cells = 0;
    }

    // k = RHS(stage state ys) for the thread's cell.  Contains exactly one __syncthreads(): the own-cell phase
    // of the evaluation (marl_math.h, point_local) runs between the edge writes and the barrier, the stencil phase
    // after it - the neighbour values are not live during the transcendental part.
    // MODE: see marl_math.h (TR_FILL / TR_AUTO for a first stage, TR_REUSE for the following ones, TR_PLAIN otherwise).
    template <int MODE = TR_PLAIN>
    __device__ __forceinline__ void eval(const double (&ys)[NF], double (&k)[NF], PointAux& aux)
    {
        MARL_PHASE_MARK(4);
        double* e = lds + parity * ((CELL ? PITCH : NF) * BLK);
        if constexpr (CELL) {   // (CA, CC), (c, o) as 16-byte stores, Phi as one of 8
            double* own = e + PITCH * tid;
            reinterpret_cast<double2v*>(own)[0] = double2v{ys[0], ys[1]};
            reinterpret_cast<double2v*>(own)[1] = double2v{ys[2], ys[3]};
            own[4] = ys[4];
        } else {
#pragma unroll
            for (int f = 0; f < NF; f++) e[f * BLK + tid] = ys[f];
        }
        if constexpr (SEAM > 0) {
            // The recording lane also writes its stage state into the seam record - here, in front of the own-cell phase, so that nothing
            // of the seam lies between the barrier and the stencil phase of its wave.  A scalar branch: three waves of four skip it, no
            // wave executes a select.  (The lane mask is rebuilt from an opaque copy, one v_cmp in that one wave: held across the
            // evaluations it costs a scalar pair, and the loop sits at its cap of those: profiles/r08_lab_rk4_chain.log, section 6.)
            if (seam_pos & SEAM_WAVEW) {
                int tw = tid;
                asm volatile("" : "+v"(tw));
                if (tw == SEAM) {
                    double* rec = seam + (seam_pos & 0xffff);
#pragma unroll
                    for (int f = 0; f < NF; f++) rec[f] = ys[f];
                }
            }
        }
        MARL_PHASE_MARK(0);
        PointLocal pl;
        MARL_ONCE point_local<CACHE ? MODE : TR_PLAIN, (CACHE && CACHE_LDS) ? BLK : 0, VD>(ys, in_zone(), K, C, T, pl, aux, cache, reuse_live);
        MARL_PHASE_MARK(1);
        __syncthreads();
        MARL_PHASE_MARK(2);
        const int tl = tid > 0 ? tid - 1 : 0;
        const int tr = tid < BLK - 1 ? tid + 1 : BLK - 1;
        double left[NF], right[NF];
        if constexpr (CELL) {
            const double* lc = e + PITCH * tl;
            const double2v s01 = reinterpret_cast<const double2v*>(lc)[0], s23 = reinterpret_cast<const double2v*>(lc)[1];
            left[0] = s01.x; left[1] = s01.y; left[2] = s23.x; left[3] = s23.y;
            left[4] = lc[4];   // (8 bytes: lanes l and l + 16 meet in a bank; read as 16 with the pad, the compiler narrows it to this)
        } else {
#pragma unroll
            for (int f = 0; f < NF; f++) left[f] = e[f * BLK + tl];
        }
        if constexpr (SEAM > 0) {
            // Thread 0 of a chained window takes its left neighbour from what the recording lane of the window before wrote at the same
            // evaluation (the other parity; 4 * NSTEPS barriers ago, and the slot is next written 4 * NSTEPS barriers from now).  Wave 0
            // only, and only in a window that reads: one scalar test.
            if ((seam_pos & (SEAM_WAVE0 | SEAM_READS)) == (SEAM_WAVE0 | SEAM_READS)) {
                int t0 = tid;
                asm volatile("" : "+v"(t0));
                if (t0 == 0) {
                    const double* prev = seam + ((seam_pos & 0xffff) ^ 8);
#pragma unroll
                    for (int f = 0; f < NF; f++) left[f] = prev[f];
                }
            }
            seam_pos += SEAM_STRIDE;
        }
        // the solids are differenced against the upwind neighbour only: with U > 0 in every lane (burial - the normal
        // case) the right-hand values of CA and CC are never used and their two LDS reads are skipped
        const bool need_right_solids = __builtin_amdgcn_ballot_w64(!pl.upw) != 0;
        if constexpr (CELL) {
            const double* rc = e + PITCH * tr;
            const double2v s23 = reinterpret_cast<const double2v*>(rc)[1];
            right[2] = s23.x; right[3] = s23.y;
            right[4] = rc[4];
            asm volatile("" : "=v"(right[0]), "=v"(right[1]));   // (see below)
            if (need_right_solids) {
                const double2v s01 = reinterpret_cast<const double2v*>(rc)[0];
                right[0] = s01.x; right[1] = s01.y;
            }
        } else if constexpr (CACHE) {
#pragma unroll
            for (int f = 2; f < NF; f++) right[f] = e[f * BLK + tr];
            // a wave-uniform branch around the two reads; without them right[0], right[1] hold whatever their registers held: point_rates,
            // told that no lane mixes upwind directions, does not read them (a 0.0 put there instead costs a v_mov_b64 each, every stage;
            // so does a plain unset value, which the compiler materialises as 0 - the empty asm defines them without an instruction)
            asm volatile("" : "=v"(right[0]), "=v"(right[1]));
            if (need_right_solids) {
                right[0] = e[tr];
                right[1] = e[BLK + tr];
            }
        } else {   // (the one-workgroup sweeps keep the select form: the branch grows rk45_sweep_kernel's scratch)
#pragma unroll
            for (int f = 0; f < NF; f++) right[f] = (f >= 2 || need_right_solids) ? e[f * BLK + tr] : 0.0;
        }
        parity ^= 1;
        MARL_ONCE {   // the stencil phase: the neighbours as read, or the ghost cells in their place
            double um[NF], up[NF];
#pragma unroll
            for (int f = 0; f < NF; f++) { um[f] = left[f]; up[f] = right[f]; }
            // physical boundaries: two cells of the whole grid - a wave-uniform branch, skipped by every other wave
            if (edge_wave()) {
                if (is_last()) {
#pragma unroll
                    for (int f = 0; f < NF; f++) up[f] = ghost_upper(f, ys[f], um[f]);
                }
                if constexpr (SEAM > 0) {
                    // The boundary values through an opaque address, read HERE, in the wave-uniform part of the branch: hoisted to the kernel's
                    // start they are scalar pairs that live across the step loop, and the allocator reloads their spilled copies in every step.
                    // (the OFFSET is what is opaque: an opaque copy of the pointer counts as captured, and every scalar load of the
                    // constants behind it becomes a vector load)
                    size_t off = offsetof(DevConsts, bc);
                    asm volatile("" : "+s"(off));
                    const double* bcp = reinterpret_cast<const double*>(reinterpret_cast<const char*>(C) + off);
                    double bcv[NF];
#pragma unroll
                    for (int f = 0; f < NF; f++) bcv[f] = bcp[f];
                    if (is_first()) {
#pragma unroll
                        for (int f = 0; f < NF; f++) um[f] = ghost_lower(bcv[f], ys[f]);
                    }
                } else if (is_first()) {
#pragma unroll
                    for (int f = 0; f < NF; f++) um[f] = ghost_lower(C->bc[f], ys[f]);
                }
            }
            point_rates<VD, true, !CACHE>(ys, um, up, K, T, pl, k, need_right_solids);
        }
#ifdef MARL_LAB_PHASE_CLOCK
        asm volatile("" :: "v"(k[0]), "v"(k[4]));   // (the rates are complete before the mark)
        MARL_PHASE_MARK(3);
        ph_acc[5]++;
#endif
    }
};

// Block-wide reduction of NQ quantities: q[0] summed, q[1..NMIN] min-reduced, the rest max-reduced, in a fixed
// order (deterministic).  Result valid in thread 0.  `scratch`: NQ * BLK doubles of LDS that no thread still reads
// for another purpose once it has arrived here (the stencil kernels pass their edge-exchange buffers).
// The quantities are transposed through LDS so that each wave reduces whole quantities: NQ/waves butterfly
// reductions per wave instead of NQ (a 64-lane butterfly of one double costs 12 ds_bpermute + the combines).
// FINITE: the extrema without NaN propagation (mon_min); the sum q[0] is unaffected - a NaN error norm still rejects the attempt.
template <int BLK, int NQ, int NMIN, bool FINITE = false>
__device__ __forceinline__ void block_reduce(double (&q)[NQ], double* scratch)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int NW = BLK / 64;
    auto combine = [](int j, double a, double o) { return (j == 0) ? a + o : (j <= NMIN ? mon_min<FINITE>(a, o) : mon_max<FINITE>(a, o)); };
    if constexpr (NW > 1) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NQ; j++) scratch[j * BLK + threadIdx.x] = q[j];
        __syncthreads();
#pragma unroll
        for (int jj = 0; jj < (NQ + NW - 1) / NW; jj++) {
            const int j = wave + jj * NW;   // wave-uniform
            if (j < NQ) {
                double a = scratch[j * BLK + lane];
#pragma unroll
                for (int i = 1; i < NW; i++) a = combine(j, a, scratch[j * BLK + lane + 64 * i]);
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) a = combine(j, a, __shfl_xor(a, off, 64));
                if (lane == 0) scratch[j * BLK] = a;
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
#pragma unroll
            for (int j = 0; j < NQ; j++) q[j] = scratch[j * BLK];
        }
        __syncthreads();
    } else {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
            for (int j = 0; j < NQ; j++) q[j] = combine(j, q[j], __shfl_xor(q[j], off, 64));
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Stand-alone RHS: dydt = f(y).  The drop-in for the reference's fun / fun_numba callable
// (marlpde/LHeureux_model.py:162, :290).  One thread per cell, neighbours straight from L1/L2.
// ---------------------------------------------------------------------------------------------
// Batches of instances that each follow their own control flow (the batched implicit path): blockIdx.z = instance, whose data
// sit `zstride` BYTES behind instance 0's, and whose 32-bit action word (at act + z * act_stride bytes) says what it needs in this
// cycle: a kernel launched for the actions `want` (a bit mask) returns at once for every other instance.  act == NULL: no masking.
// `list` (may be NULL): the launch covers only the instances list[0 .. gridDim.z) - a compacted index list the controller wrote for
// this kind of work - instead of all of them.
struct ZBatch {
    int64_t zstride;
    const int32_t* act;
    int64_t act_stride;
    int want;
    const int32_t* list;
};
// (readfirstlane: the index is the same in every lane, but a load through a struct member is not provably so - without it every
// shifted pointer becomes a per-lane 64-bit address and the PCR kernels of a single large grid ran 3x slower)
__device__ __forceinline__ int64_t z_inst(const ZBatch& B)
{
    return B.list ? (int64_t)__builtin_amdgcn_readfirstlane(B.list[blockIdx.z]) : (int64_t)blockIdx.z;
}
__device__ __forceinline__ bool z_masked_out(const ZBatch& B)
{
    return B.act && !(*reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(B.act) + z_inst(B) * B.act_stride) & B.want);
}
template <class P>
__device__ __forceinline__ P* z_shift(P* p, const ZBatch& B)
{
    return reinterpret_cast<P*>(reinterpret_cast<char*>(const_cast<typename std::remove_const<P>::type*>(p)) + z_inst(B) * B.zstride);
}

// blockIdx.y: instance (state at y + blockIdx.y * inst_stride, constants consts[blockIdx.y * const_stride]; const_stride = 0:
// several states of ONE model - the stage states / finite-difference columns of the implicit path); blockIdx.z: ZBatch instance
// (constants consts[blockIdx.z] then)
template <int LAYOUT, bool VD = false>
__global__ void __launch_bounds__(256) rhs_kernel(const double* __restrict__ y, double* __restrict__ dydt,
                                                  const DevConsts* __restrict__ consts, Slab S, int64_t inst_stride, int const_stride,
                                                  ZBatch B = ZBatch{0, nullptr, 0, 0, nullptr})
{
    if (z_masked_out(B)) return;
    __shared__ double tabs[TABLE_DOUBLES];
    const Tables T = load_tables(tabs, 256);
    const DevConsts& C = consts[blockIdx.y * const_stride + z_inst(B)];
    y = z_shift(y, B) + blockIdx.y * inst_stride;
    dydt = z_shift(dydt, B) + blockIdx.y * inst_stride;
    const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (l < S.out_lo || l >= S.out_hi) return;
    const int64_t g = l + S.goff;
    double uc[NF], um[NF], up[NF], r[NF];
    PointAux aux;
#pragma unroll
    for (int f = 0; f < NF; f++) {
        uc[f] = y[at<LAYOUT>(f, l, S.ld)];
        um[f] = (g > 0) ? y[at<LAYOUT>(f, l - 1, S.ld)] : ghost_lower(C.bc[f], uc[f]);
    }
#pragma unroll
    for (int f = 0; f < NF; f++) up[f] = (g < C.N - 1) ? y[at<LAYOUT>(f, l + 1, S.ld)] : ghost_upper(f, uc[f], um[f]);
    const HotConsts K = load_hot(&C);
    PointCache<0> pc;
    bool live = false;
    rhs_point<TR_PLAIN, 0, VD>(uc, um, up, g >= C.mask_lo && g < C.mask_hi, K, &C, T, r, aux, pc, live);
#pragma unroll
    for (int f = 0; f < NF; f++) dydt[at<LAYOUT>(f, l, S.ld)] = r[f];
}

// Element-wise evaluation of the device math primitives (accuracy tests only; marl_debug_math).
__global__ void __launch_bounds__(256) math_probe_kernel(int op, const double* __restrict__ x, double* __restrict__ y, int64_t n, double e)
{
    __shared__ double tabs[TABLE_DOUBLES];
    const Tables T = load_tables(tabs, 256);
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double v = x[i];
    double r;
    switch (op) {
        case 0: r = fast_log(v, T); break;
        case 1: r = fast_exp(v, T); break;
        case 2: r = pow_sat(v, e, T); break;
        case 3: r = rcp_nr(v); break;
        case 4: r = fv_sigma<false>(v, e, T); break;
        default: r = fv_sigma<true>(v, e, T); break;
    }
    y[i] = r;
}

// Layout conversion FIELD_MAJOR <-> TILED (entry / exit of the fused integrators only).
template <int SRC, int DST>
__global__ void __launch_bounds__(256) convert_kernel(const double* __restrict__ src, double* __restrict__ dst, int64_t n,
                                                      int64_t ld_src, int64_t ld_dst, int64_t stride_src, int64_t stride_dst)
{
    src += blockIdx.y * stride_src;
    dst += blockIdx.y * stride_dst;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int f = 0; f < NF; f++) dst[at<DST>(f, i, ld_dst)] = src[at<SRC>(f, i, ld_src)];
}

// ---------------------------------------------------------------------------------------------
// The seven monitors (marlpde/LHeureux_model.py:524-593) as per-block partials:
//   part[b][0] unused (sum slot), [1] min(y) [2] min CA [3] min CC [4] min U [5] max(CA+CC) [6] max Phi [7] max W
// ---------------------------------------------------------------------------------------------
constexpr int NQ = 8;    // reduction record: sum-of-squares + 7 monitor extrema
constexpr int NQMIN = 4; // slots 1..4 are minima, 5..7 maxima

__device__ __forceinline__ void monitors_init(double (&q)[NQ])
{
    q[0] = 0.0;
    q[1] = q[2] = q[3] = q[4] = __builtin_inf();
    q[5] = q[6] = q[7] = -__builtin_inf();
}

template <bool FINITE = false>   // (see mon_min)
__device__ __forceinline__ void monitors_accumulate(double (&q)[NQ], const double (&u)[NF], double U, double W)
{
    q[1] = mon_min<FINITE>(mon_min<FINITE>(mon_min<FINITE>(mon_min<FINITE>(mon_min<FINITE>(q[1], u[0]), u[1]), u[2]), u[3]), u[4]);
    q[2] = mon_min<FINITE>(q[2], u[0]);
    q[3] = mon_min<FINITE>(q[3], u[1]);
    q[4] = mon_min<FINITE>(q[4], U);
    q[5] = mon_max<FINITE>(q[5], u[0] + u[1]);
    q[6] = mon_max<FINITE>(q[6], u[4]);
    q[7] = mon_max<FINITE>(q[7], W);
}

template <int LAYOUT>
__global__ void __launch_bounds__(256) monitors_kernel(const double* __restrict__ y, const DevConsts* __restrict__ consts,
                                                       Slab S, int64_t inst_stride, double* __restrict__ part)
{
    __shared__ double scratch[NQ * 256];
    __shared__ double tabs[TABLE_DOUBLES];
    const Tables T = load_tables(tabs, 256);
    const DevConsts& C = consts[blockIdx.y];
    y += blockIdx.y * inst_stride;
    double q[NQ];
    monitors_init(q);
    for (int64_t l = S.out_lo + (int64_t)blockIdx.x * 256 + threadIdx.x; l < S.out_hi; l += (int64_t)gridDim.x * 256) {
        double u[NF];
#pragma unroll
        for (int f = 0; f < NF; f++) u[f] = y[at<LAYOUT>(f, l, S.ld)];
        const double Phi = u[4];
        const double F = 1.0 - fast_exp(10.0 - 10.0 * rcp_nr(Phi), T);
        const double rF = C.hot.rhorat * F;
        monitors_accumulate(q, u, C.hot.presum + rF * (Phi * Phi * Phi) * rcp_nr(1.0 - Phi), C.hot.presum - rF * Phi * Phi);
    }
    block_reduce<256, NQ, NQMIN>(q, scratch);
    if (threadIdx.x == 0) {
        double* p = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * NQ;
#pragma unroll
        for (int j = 0; j < NQ; j++) p[j] = q[j];
    }
}

// Deterministic second-level reduction: `nblocks` records -> one record per instance.
__global__ void __launch_bounds__(256) reduce_records_kernel(const double* __restrict__ part, int64_t nblocks, double* __restrict__ out)
{
    __shared__ double scratch[NQ * 256];
    part += (int64_t)blockIdx.x * nblocks * NQ;
    double q[NQ];
    monitors_init(q);
    for (int64_t b = threadIdx.x; b < nblocks; b += 256) {
#pragma unroll
        for (int j = 0; j < NQ; j++) {
            const double o = part[b * NQ + j];
            q[j] = (j == 0) ? q[j] + o : (j <= NQMIN ? nanmin(q[j], o) : nanmax(q[j], o));
        }
    }
    block_reduce<256, NQ, NQMIN>(q, scratch);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < NQ; j++) out[(int64_t)blockIdx.x * NQ + j] = q[j];
    }
}

// First level of a two-level reduction of MANY records (one per workgroup of a large grid): workgroup b reduces the records
// [b * chunk, min(nrec, (b + 1) * chunk)) into out[b] - a fixed partition, so the result is reproducible.  One workgroup reading
// thousands of records alone is latency-bound (17 000 records at N = 2^22: ~60 us); 64 workgroups take ~3 us.
__global__ void __launch_bounds__(256) reduce_chunks_kernel(const double* __restrict__ part, int64_t nrec, int64_t chunk, double* __restrict__ out)
{
    __shared__ double scratch[NQ * 256];
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = (lo + chunk < nrec) ? lo + chunk : nrec;
    double q[NQ];
    monitors_init(q);
    for (int64_t b = lo + threadIdx.x; b < hi; b += 256) {
#pragma unroll
        for (int j = 0; j < NQ; j++) {
            const double o = part[b * NQ + j];
            q[j] = (j == 0) ? q[j] + o : (j <= NQMIN ? nanmin(q[j], o) : nanmax(q[j], o));
        }
    }
    block_reduce<256, NQ, NQMIN>(q, scratch);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < NQ; j++) out[(int64_t)blockIdx.x * NQ + j] = q[j];
    }
}

// ---------------------------------------------------------------------------------------------
// Shared load of a thread's cell
// ---------------------------------------------------------------------------------------------
template <int LAYOUT>
__device__ __forceinline__ void load_cells(const double* __restrict__ y, int64_t l, const Slab& S, const DevConsts& C, double (&u)[NF])
{
    const bool in = l >= 0 && l < S.n_buf;
#pragma unroll
    for (int f = 0; f < NF; f++) u[f] = in ? y[at<LAYOUT>(f, l, S.ld)] : C.bc[f];
}

// ---------------------------------------------------------------------------------------------
// Fused classical RK4: NSTEPS whole steps per launch (BASELINE config 2 / headline).
//   k1 = f(y); k2 = f(y + dt/2 k1); k3 = f(y + dt/2 k2); k4 = f(y + dt k3)
//   y <- y + dt/6 (((k1 + 2 k2) + 2 k3) + k4)                 (the order the CPU checker uses too)
// ---------------------------------------------------------------------------------------------
#ifdef MARL_LAB_CLOCK  // kernel-lab diagnostic build only: in-kernel shader clock (s_memtime) vs 100 MHz s_memrealtime
__device__ unsigned long long marl_lab_clock[3 * 16384];
#endif
// NSTEPS classical RK4 steps on the thread's cell (every evaluation invalidates one more cell per window edge).
template <int NSTEPS, class SB>
__device__ __forceinline__ void rk4_advance(SB& sb, double (&y)[NF], double dt)
{
    double ys[NF], k[NF], acc[NF];
    PointAux aux;
    const double h2 = 0.5 * dt, h6 = dt / 6.0;
#pragma unroll 1
    for (int step = 0; step < NSTEPS; step++) {
        sb.template eval<TR_AUTO>(y, k, aux);   // the centre of the expansions survives from step to step
        MARL_FIELDS { acc[f] = k[f]; ys[f] = y[f] + h2 * k[f]; }
        sb.template eval<TR_REUSE>(ys, k, aux);
        MARL_FIELDS { acc[f] = acc[f] + 2.0 * k[f]; ys[f] = y[f] + h2 * k[f]; }
        sb.template eval<TR_REUSE>(ys, k, aux);
        MARL_FIELDS { acc[f] = acc[f] + 2.0 * k[f]; ys[f] = y[f] + dt * k[f]; }
        sb.template eval<TR_REUSE>(ys, k, aux);
        MARL_FIELDS y[f] = y[f] + h6 * (acc[f] + k[f]);
    }
}

// 4 waves per SIMD (<= 128 VGPRs; 4 workgroups of 256 share the CU's 160 KB of LDS).
#ifndef MARL_LAB_RK4_WAVES_MIN   // kernel-lab switch: occupancy window the register allocator aims at
#define MARL_LAB_RK4_WAVES_MIN 4
#define MARL_LAB_RK4_WAVES_MAX 8
#endif
template <int BLK, int LAYOUT, int NSTEPS, bool VD = false>
__global__ void __launch_bounds__(BLK) __attribute__((amdgpu_waves_per_eu(MARL_LAB_RK4_WAVES_MIN, MARL_LAB_RK4_WAVES_MAX))) rk4_fused_kernel(const double* __restrict__ yin, double* __restrict__ yout,
                                                        const DevConsts* __restrict__ consts, Slab S, double dt)
{
#ifdef MARL_LAB_CLOCK
    const unsigned long long lab_t0 = __builtin_amdgcn_s_memtime(), lab_r0 = __builtin_amdgcn_s_memrealtime();
#endif
    constexpr int H = 4 * NSTEPS;
    constexpr int V = BLK - 2 * H;
    static_assert(V > 0, "window too small for the fused halo");
    using SB = StencilBlock<BLK, true, VD>;
    __shared__ double lds[SB::LDS_DOUBLES];
    const DevConsts& C = consts[0];

    const int64_t w0 = S.out_lo + (int64_t)blockIdx.x * V - H;  // window start, local index
    const int64_t l = w0 + (int64_t)threadIdx.x;
    double y[NF];
    load_cells<LAYOUT>(yin, l, S, C, y);              // in flight while the tables are staged
    SB sb(lds, l + S.goff, consts);   // (table copy + barrier inside)
    rk4_advance<NSTEPS>(sb, y, dt);

    const int wi = threadIdx.x;
    // (MARL_ONCE: see its definition - here it keeps the prologue's scalar loads and spills where they were; without it the 16-step
    // kernel of marl_rk4_small.hip, opcode for opcode the same in its stages, ran 2.1 % slower at N = 65 536)
    MARL_ONCE if (wi >= H && wi < BLK - H && l >= S.out_lo && l < S.out_hi) {
#pragma unroll
        for (int f = 0; f < NF; f++) yout[at<LAYOUT>(f, l, S.ld)] = y[f];
    }
#ifdef MARL_LAB_PHASE_CLOCK
    sb.phase_flush();
#endif
#ifdef MARL_LAB_CLOCK
    if (threadIdx.x == 0 && blockIdx.x < 16384) {
        marl_lab_clock[3 * blockIdx.x] = __builtin_amdgcn_s_memtime() - lab_t0;
        marl_lab_clock[3 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime() - lab_r0;
        marl_lab_clock[3 * blockIdx.x + 2] = lab_r0;
    }
#endif
}

// ---------------------------------------------------------------------------------------------
// The whole fixed-step loop of ONE large grid in ONE launch: a dataflow schedule over (level, tile) work items.
//
// A launch of rk4_fused_kernel is a global barrier: with waves that run ~20 us and only ~4.6 "rounds" of them per launch
// (N = 2^20: 18 728 waves on 4096 slots), the partially filled last round and the ramp-up leave the SIMDs with 3.3 instead
// of 4 resident waves on average (SQ counters) - and tile t of the next level only needs tiles t-1, t, t+1 of
// this one.  So: `levels` x `tiles` work items (a tile = the V cells one window writes, a level = NSTEPS steps), handed out in
// level-major order by an atomic counter to a grid of resident workgroups; an item waits until the three tiles it reads have
// published the previous level, computes exactly what the workgroup of the per-level launch computes (bit-identical results),
// and publishes its tile.  Ping-pong between two buffers is safe: neighbours can never be more than one level apart.
//   * Progress: an item only waits for items with smaller numbers, which were handed out earlier to workgroups that are
//     running - the smallest unfinished item never waits.  Every wait is bounded (STREAM_SPIN_LIMIT polls, ~1 s): on expiry,
//     or when any workgroup has raised the sticky flag, the workgroup raises it and leaves; the host reports the error.
//   * Coherence: tiles cross XCDs (one L2 each).  A release fence at agent scope writes back the XCD's whole L2 (measured 4x
//     slower, profiles/r02_lab_rk45_fused_control.log); instead the state itself moves with agent-scope (sc1: write-through /
//     L2-bypassing) stores and loads, and a tile is published - done[tile] = level_base + level + 1, also sc1 - only after every thread's
//     stores have been acknowledged (s_waitcnt vmcnt(0) + barrier).  The path is bound by the fp64 VALU, not by memory:
//     80 MB per level through the Infinity Fabric instead of the L2s costs nothing measurable.
// Nothing is reset between launches (a call is ONE launch, no memset in front of it): queue[0], the item counter, and done[t], the
// levels tile t has published, only ever grow; a launch is told where they stand (item_base: every earlier launch took its
// items plus one failing grab per workgroup; level_base: the levels of all earlier launches) and compares wrap-safely.  A stale
// value can only be too SMALL - it makes a reader wait, never pass.  sticky: raised by a workgroup that gives up; checked by
// waiting workgroups, never cleared by the device: the host looks at it at its next synchronisation point (marl_synchronize)
// and then resets counters and bases.
// ---------------------------------------------------------------------------------------------
constexpr unsigned STREAM_SPIN_LIMIT = 1u << 19;

template <int BLK, int LAYOUT, int NSTEPS, bool VD = false>
__global__ void __launch_bounds__(BLK) __attribute__((amdgpu_waves_per_eu(4, 8)))
rk4_stream_kernel(double* bufA, double* bufB, const DevConsts* __restrict__ consts, Slab S, double dt, unsigned levels, unsigned tiles,
                  unsigned* queue, unsigned* done, unsigned* sticky, unsigned item_base, unsigned level_base, double* bufC = nullptr)
{
    // bufC != NULL (an ODD number of levels >= 3 in this launch): A -> B, then B <-> C, the last level back into A - the result lands in the
    // caller's buffer and the whole-state copy that an odd level count used to need afterwards (42 MB at N = 2^20: 12 us of a 20-step
    // call) goes away.  The write-after-read distance is that of the two-buffer scheme (a level writes what the level before reads, and
    // done[tile +- 1] orders it); the last level writes A, which only level 0 reads - five or more tiles of dependency away.
    constexpr int H = 4 * NSTEPS;
    constexpr int V = BLK - 2 * H;
    using SB = StencilBlock<BLK, true, VD>;
    __shared__ double lds[SB::LDS_DOUBLES];
    __shared__ unsigned s_item, s_abort;
    const DevConsts& C = consts[0];
    SB sb(lds, 0, consts);   // tables once per workgroup (barrier inside)
    const unsigned total = levels * tiles;   // (host: < 2^31)

#ifdef MARL_LAB_BROKEN_STREAM_LATCH   // tests/test_stream_isa.py only: the round-2 loop shape whose code the invariant checker must REJECT
    if (threadIdx.x == 0) {
        s_item = __hip_atomic_fetch_add(&queue[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - item_base;
        s_abort = 0;
    }
    while (true) {
        __syncthreads();
#else
    while (true) {
        // (barrier 1: every wave has left the previous item - s_item / s_abort may be rewritten.  It also separates the
        // thread-0 block below from the one at the end of the loop body: without it the two are fused across the back-edge
        // into a private loop of lane 0, whose wave then arrives at the barriers twice per item - seen with NSTEPS = 1: hang.
        // Taking the next item at the END of the body instead puts the LDS write of s_item into the loop latch, and the
        // compiler then emits the barrier at the loop header without the s_waitcnt lgkmcnt(0) in front of it: waves read the
        // previous s_item - seen as partly stale tiles.  tools/lab_src, profiles/r02_lab_rk4_stream.log.)
        __syncthreads();
        if (threadIdx.x == 0) {
            s_item = __hip_atomic_fetch_add(&queue[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - item_base;
            s_abort = 0;
        }
        __syncthreads();
#endif
        const unsigned item = s_item;
        if (item >= total) break;
        const unsigned level = item / tiles, tile = item - level * tiles;
        if (level > 0) {
            if (threadIdx.x < 3) {
                const int64_t t = (int64_t)tile - 1 + threadIdx.x;
                if (t >= 0 && t < (int64_t)tiles) {
                    unsigned spins = 0;
                    while ((int)(__hip_atomic_load(&done[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - (level_base + level)) < 0) {
                        __builtin_amdgcn_s_sleep(4);
                        if (++spins > STREAM_SPIN_LIMIT ||
                            ((spins & 255u) == 0 && __hip_atomic_load(sticky, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
                            __hip_atomic_store(sticky, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            s_abort = 1;
                            break;
                        }
                    }
                }
            }
            __syncthreads();
            if (s_abort) break;
        }
        const double* src = bufC ? (level == 0 ? bufA : ((level & 1u) ? bufB : bufC)) : ((level & 1u) ? bufB : bufA);
        double* dst = bufC ? (level + 1 == levels ? bufA : ((level & 1u) ? bufC : bufB)) : ((level & 1u) ? bufA : bufB);
        const int64_t l = S.out_lo + (int64_t)tile * V - H + threadIdx.x;
        const bool in = l >= 0 && l < S.n_buf;
        double y[NF];
#pragma unroll
        for (int f = 0; f < NF; f++)
            y[f] = in ? __hip_atomic_load(src + at<LAYOUT>(f, l, S.ld), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : C.bc[f];
        sb.set_window(l + S.goff);
        sb.reuse_live = false;
        rk4_advance<NSTEPS>(sb, y, dt);
        if ((int)threadIdx.x >= H && (int)threadIdx.x < BLK - H && l >= S.out_lo && l < S.out_hi) {
#pragma unroll
            for (int f = 0; f < NF; f++) __hip_atomic_store(dst + at<LAYOUT>(f, l, S.ld), y[f], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
        __builtin_amdgcn_s_waitcnt(0);   // this thread's stores have been acknowledged (vmcnt = expcnt = lgkmcnt = 0)
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
        __syncthreads();                 // ... and everybody else's (and everybody has read s_item, s_abort)
        if (threadIdx.x == 0) {
            __hip_atomic_store(&done[tile], level_base + level + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#ifdef MARL_LAB_BROKEN_STREAM_LATCH
            s_item = __hip_atomic_fetch_add(&queue[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - item_base;   // the item grab in the loop latch
            s_abort = 0;
#endif
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The streamed loop with CHAINED windows: a work item is `nsub` windows processed left to right by the same workgroup.
//
// A window of rk4_stream_kernel recomputes a halo of H = 4 * NSTEPS cells on each side and writes BLK - 2 H cells: one lane in
// eight (BLK = 256, NSTEPS = 4) works for nothing.  Here only the first window of an item has a left halo.  While a window
// runs, the stage state that lane BLK - H - 1 - the last cell it writes - passes to each of the 4 * NSTEPS evaluations is
// recorded (StencilBlock, SEAM).  The next window starts with thread 0 on the first cell its predecessor did not write, and thread 0
// takes its left neighbour at evaluation e from that record: it needs no left halo and writes BLK - H cells.
//   * Validity: thread BLK - 1 - m has a valid state up to evaluation m + 1, so lane BLK - H - 1 is valid through all of them,
//     and so is every value it records.  Thread 0's cell itself is loaded from the level's input like every other cell.
//   * The record has two parities that alternate by window: the lane's write at evaluation e (in front of the exchange barrier), the
//     successor's read of it (behind the barrier of its evaluation e) and the next write to the same slot are 4 * NSTEPS barriers
//     apart each - the chain needs no barrier of its own.
//   * Stores of a window are not waited for before the next one starts; the item ends as in rk4_stream_kernel.
// Items of a level (host: rk4_stream): `items - 1` chains tile [out_lo, out_lo + bound), each V + (K - 1) (BLK - H) cells, the last
// one `nsub_last` windows and clipped at the bound; the LAST item is the grid's last tile of the unchained decomposition,
// [bound, out_hi), as ONE plain window with both halos - so the waves that hold the two physical boundary cells consist of the
// same cells as in rk4_stream_kernel and in the per-level launches, and take the same tier of the transcendental reuse.
// Everything else - queue, done[], sticky flag, ping-pong / third buffer, the shape of the work loop and why it has that shape -
// is rk4_stream_kernel's; an item still depends on items t-1, t, t+1 of the level before (host, chain_shape: no item but the
// last is narrower than H cells).  tools/check_stream_isa.py checks I1-I5 on this kernel too (tests/test_chain_isa.py).
// ---------------------------------------------------------------------------------------------
// rk4_chain_kernel's arguments as they lie in its kernel-argument segment.  The kernel reads those it needs once per item or per window
// through an opaque pointer to that segment (scalar loads) instead of holding them: held, they are spilled to lanes of a vector register
// - the loop sits at its cap of scalar registers - and every use costs a v_readlane.
struct ChainArgs {
    double *bufA, *bufB;
    const DevConsts* consts;
    Slab S;
    double dt;
    unsigned levels, items;
    unsigned *queue, *done, *sticky;
    unsigned item_base, level_base;
    double* bufC;
    unsigned K, nsub_last;
    int64_t bound;
};
static_assert(offsetof(ChainArgs, S) == 24 && offsetof(ChainArgs, dt) == 64 && offsetof(ChainArgs, queue) == 80 && offsetof(ChainArgs, bufC) == 112 &&
              offsetof(ChainArgs, bound) == 128 && sizeof(ChainArgs) == 136, "the argument list of rk4_chain_kernel, in order");
typedef const __attribute__((address_space(4))) ChainArgs* ChainArgsPtr;
__device__ __forceinline__ ChainArgsPtr chain_args()
{
    ChainArgsPtr a = (ChainArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(a));   // opaque: a load through it is not merged with an earlier one and kept
    return a;
}

template <int BLK, int LAYOUT, int NSTEPS>
__global__ void __launch_bounds__(BLK) __attribute__((amdgpu_waves_per_eu(4, 8)))
rk4_chain_kernel(double* bufA, double* bufB, const DevConsts* __restrict__ consts, Slab S, double dt, unsigned levels, unsigned items,
                 unsigned* queue, unsigned* done, unsigned* sticky, unsigned item_base, unsigned level_base, double* bufC,
                 unsigned K, unsigned nsub_last, int64_t bound)
{
    constexpr int H = 4 * NSTEPS;
    constexpr int V = BLK - 2 * H;     // cells the first window of an item writes
    constexpr int W = BLK - H;         // ... and every later one
    static_assert(V > 0, "window too small for the fused halo");
    using SB = StencilBlock<BLK, true, false, BLK - H - 1>;
    __shared__ double lds[SB::LDS_DOUBLES];
    __shared__ double seam[H * SB::SEAM_STRIDE];
    __shared__ unsigned s_item, s_abort;
    const DevConsts& C = consts[0];
    SB sb(lds, 0, consts);   // tables once per workgroup (barrier inside)
    sb.seam = seam;
    // (the step in a scalar pair of its own: it arrives in one wide load with `levels`, `items`, `queue`, `done`, and the allocator keeps -
    // and, where cold code borrows the registers, reloads in every step - the whole tuple for as long as one member is live)
    dt = pin_uniform(dt);
    const unsigned total = levels * items;   // (host: < 2^31)
    const unsigned chains = items - 1;

    while (true) {
        // (the shape of this loop: see rk4_stream_kernel)
        __syncthreads();
        // the queue's arguments through the segment too, once per item (they shadow the parameters): they arrive in one wide load with the
        // step size, and while any member of it is held the allocator keeps - and reloads in every step - the whole tuple
        typedef __attribute__((address_space(1))) unsigned* GlobalWords;
        ChainArgsPtr G = chain_args();
        unsigned *const queue = (unsigned*)(GlobalWords)G->queue, *const done = (unsigned*)(GlobalWords)G->done,
                 *const sticky = (unsigned*)(GlobalWords)G->sticky;
        const unsigned items = G->items, item_base = G->item_base, level_base = G->level_base;
        if (threadIdx.x == 0) {
            s_item = __hip_atomic_fetch_add(&queue[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - item_base;
            s_abort = 0;
        }
        __syncthreads();
        const unsigned item = __builtin_amdgcn_readfirstlane(s_item);   // (in a scalar register: the trip count below derives from it)
        if (item >= total) break;
        const unsigned level = item / items, tile = item - level * items;
        if (level > 0) {
            if (threadIdx.x < 3) {
                const int64_t t = (int64_t)tile - 1 + threadIdx.x;
                if (t >= 0 && t < (int64_t)items) {
                    unsigned spins = 0;
                    while ((int)(__hip_atomic_load(&done[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - (level_base + level)) < 0) {
                        __builtin_amdgcn_s_sleep(4);
                        if (++spins > STREAM_SPIN_LIMIT ||
                            ((spins & 255u) == 0 && __hip_atomic_load(sticky, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
                            __hip_atomic_store(sticky, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            s_abort = 1;
                            break;
                        }
                    }
                }
            }
            __syncthreads();
            if (s_abort) break;
        }
        const double* src;
        double* dst;
        unsigned nsub;
        int64_t first, clip;
        {   // (the arguments through the segment: see ChainArgs)
            ChainArgsPtr A = chain_args();
            double *const pA = A->bufA, *const pB = A->bufB, *const pC = A->bufC;
            const unsigned nlev = A->levels, KK = A->K, nlast = A->nsub_last;
            const int64_t olo = A->S.out_lo, ohi = A->S.out_hi, bnd = A->bound;
            src = (const double*)(const __attribute__((address_space(1))) double*)(pC ? (level == 0 ? pA : ((level & 1u) ? pB : pC)) : ((level & 1u) ? pB : pA));
            dst = (double*)(__attribute__((address_space(1))) double*)(pC ? (level + 1 == nlev ? pA : ((level & 1u) ? pC : pB)) : ((level & 1u) ? pA : pB));
            // the item's windows (all wave-uniform): window j has its thread 0 on local cell first + j W
            const bool chain = tile < chains;
            nsub = chain ? (tile + 1 == chains ? nlast : KK) : 1u;
            first = olo - H + (chain ? (int64_t)tile * (V + (int64_t)W * (KK - 1)) : bnd);
            clip = chain ? olo + bnd : ohi;
        }
#pragma unroll 1
        for (unsigned j = 0; j < nsub; j++) {
            int tid = threadIdx.x;
            asm volatile("" : "+v"(tid));   // opaque: what derives from the thread index is recomputed per window, not carried across the loops
            sb.rebind(tid);
            // An INTERIOR window - wholly inside the buffer, neither cell 0 nor cell N - 1 in it, wholly inside or wholly outside the
            // dissolution zone: all but three or four windows of a grid - is recognised once on the scalar side (wave-uniform).  Its
            // masks are constants and its loads need no guard: the per-lane 64-bit compares of set_window, the ballot and the
            // boundary selects run only in the other windows.  Same values either way.
            // (The tests are signs of 64-bit differences, formed modulo 2^64 - every operand is below 2^62 - and taken from the high
            // words: scalar subtractions and one 32-bit compare, where a signed 64-bit compare of two scalars is a vector instruction.)
            ChainArgsPtr A = chain_args();
            const int64_t n_buf = A->S.n_buf, goff = A->S.goff, ld = A->S.ld;
            const int64_t lw = first + (int64_t)j * W, gw = lw + goff;
            const int64_t mlo = C.mask_lo, mhi = C.mask_hi;
            // (each sign word opaque: combined freely, they are merged back into 64-bit values and compared on the vector side)
            auto neg = [](int64_t a, int64_t b) {   // < 0: a < b
                int32_t hi = (int32_t)(((uint64_t)a - (uint64_t)b) >> 32);
                asm("" : "+s"(hi));
                return hi;
            };
            const int32_t out_any = neg(lw, 0) | neg(n_buf, lw + BLK) | neg(gw, 1) | neg(C.N - 1, gw + BLK);   // < 0: not interior
            const int32_t zone_part = neg(gw, mlo) | neg(mhi, gw + BLK);       // >= 0: wholly inside the zone
            const int32_t zone_some = neg(mlo, gw + BLK) & neg(gw, mhi);       // >= 0: wholly outside
            const bool interior = out_any >= 0 && (zone_part >= 0 || zone_some >= 0);
            const int64_t l = lw + tid;
            bool in = true;
            int64_t la = l;   // the cell the lane loads: its own, or - outside the buffer - a valid one (the value is replaced below)
            if (!interior) {
                asm volatile("");   // a real branch
                in = l >= 0 && l < n_buf;
                la = in ? l : 0;
            }
            double y[NF];
#pragma unroll
            for (int f = 0; f < NF; f++) y[f] = __hip_atomic_load(src + at<LAYOUT>(f, la, ld), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (interior) {
                sb.set_interior(zone_part >= 0);
            } else {
                asm volatile("");
#pragma unroll
                for (int f = 0; f < NF; f++) y[f] = in ? y[f] : C.bc[f];
                sb.set_window_seam(gw);
            }
            sb.reuse_live = false;   // every window fills its own expansion centre, as an item of rk4_stream_kernel does
            // (the wave's number through readfirstlane: everything else is then scalar arithmetic; left to itself the compiler builds the
            // word per lane from lane masks)
            const int wave = __builtin_amdgcn_readfirstlane(tid) >> 6;
            sb.seam_pos = (int)(j & 1u) * 8 + (j ? SB::SEAM_READS : 0) + (wave == 0 ? SB::SEAM_WAVE0 : 0)
                          + (wave == (BLK - H - 1) / 64 ? SB::SEAM_WAVEW : 0);
            // the lanes that store, [lo, hi): both bounds are scalars of 32 bits.  hi - the window's end or the clip - is formed here, in front
            // of the evaluations (one word carried instead of the 64-bit clip); lo is read off the seam word behind them (a window with a left
            // halo of its own is the one that does not read the seam), where `j == 0` itself would be carried as a lane mask, a spilled pair.
            const int64_t room = clip - lw;
            int hi = neg(room, BLK - H) < 0 ? (int)room : BLK - H;
            asm volatile("" : "+s"(hi));
            rk4_advance<NSTEPS>(sb, y, dt);
            int sp = sb.seam_pos;
            asm volatile("" : "+s"(sp));
            const int lo = (sp & SB::SEAM_READS) ? 0 : H;
            int ts = threadIdx.x;
            asm volatile("" : "+v"(ts));    // (the cell index again: two registers less across the evaluations)
            const int64_t ls = first + (int64_t)j * W + ts;
            if (ts >= lo && ts < hi) {
                int64_t lds_ = 0;   // (the tiled layout has no field stride: no pointer to the segment is formed for it)
                if constexpr (LAYOUT == LAYOUT_FIELD_MAJOR) lds_ = chain_args()->S.ld;
#pragma unroll
                for (int f = 0; f < NF; f++) __hip_atomic_store(dst + at<LAYOUT>(f, ls, lds_), y[f], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
        __builtin_amdgcn_s_waitcnt(0);   // this thread's stores - of every window of the item - have been acknowledged
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
        __syncthreads();                 // ... and everybody else's (and everybody has read s_item, s_abort)
        if (threadIdx.x == 0) __hip_atomic_store(&done[tile], level_base + level + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// rk4_chain_kernel with the LDS exchange laid out by cell and the cache slots in pairs (StencilBlock, XCH): the same arguments, the same
// item loop, the same arithmetic on the same operands in the same order - bit-identical results - and 16-byte LDS accesses where
// rk4_chain_kernel has two-address 64-bit ones.  The exchange buffer grows by the pad double of each cell, 4 KB: 37 896 B, and four
// workgroups still share a CU's 160 KB.
// The body is rk4_chain_kernel's, line for line, written out a second time: moved into a function that both kernels inline, it changed the
// machine code of rk4_chain_kernel (scalar spills and the order of the prologue; profiles/r11_lab_chain_exchange.log) - and that kernel stays
// what it is.  What differs: the StencilBlock and the alignment of the LDS block.  A change to one loop belongs in the other too.
// XCH: which parts of the layout the kernel takes (XCH_CELL | XCH_PAIRS is what ships; lab builds instantiate each part alone too).
template <int BLK, int LAYOUT, int NSTEPS, int XCH = XCH_CELL | XCH_PAIRS>
__global__ void __launch_bounds__(BLK) __attribute__((amdgpu_waves_per_eu(4, 8)))
rk4_exchange_kernel(double* bufA, double* bufB, const DevConsts* __restrict__ consts, Slab S, double dt, unsigned levels, unsigned items,
                    unsigned* queue, unsigned* done, unsigned* sticky, unsigned item_base, unsigned level_base, double* bufC,
                    unsigned K, unsigned nsub_last, int64_t bound)
{
    constexpr int H = 4 * NSTEPS;
    constexpr int V = BLK - 2 * H;     // cells the first window of an item writes
    constexpr int W = BLK - H;         // ... and every later one
    static_assert(V > 0, "window too small for the fused halo");
    using SB = StencilBlock<BLK, true, false, BLK - H - 1, XCH>;
    __shared__ __attribute__((aligned(16))) double lds[SB::LDS_DOUBLES];   // (the 128-bit forms need 16 bytes)
    __shared__ double seam[H * SB::SEAM_STRIDE];
    __shared__ unsigned s_item, s_abort;
    static_assert((SB::LDS_DOUBLES + H * SB::SEAM_STRIDE) * 8 + 8 <= 40960, "four workgroups per CU: 160 KB of LDS");
    const DevConsts& C = consts[0];
    SB sb(lds, 0, consts);   // tables once per workgroup (barrier inside)
    sb.seam = seam;
    // (the step in a scalar pair of its own: it arrives in one wide load with `levels`, `items`, `queue`, `done`, and the allocator keeps -
    // and, where cold code borrows the registers, reloads in every step - the whole tuple for as long as one member is live)
    dt = pin_uniform(dt);
    const unsigned total = levels * items;   // (host: < 2^31)
    const unsigned chains = items - 1;

    while (true) {
        // (the shape of this loop: see rk4_stream_kernel)
        __syncthreads();
        // the queue's arguments through the segment too, once per item (they shadow the parameters): they arrive in one wide load with the
        // step size, and while any member of it is held the allocator keeps - and reloads in every step - the whole tuple
        typedef __attribute__((address_space(1))) unsigned* GlobalWords;
        ChainArgsPtr G = chain_args();
        unsigned *const queue = (unsigned*)(GlobalWords)G->queue, *const done = (unsigned*)(GlobalWords)G->done,
                 *const sticky = (unsigned*)(GlobalWords)G->sticky;
        const unsigned items = G->items, item_base = G->item_base, level_base = G->level_base;
        if (threadIdx.x == 0) {
            s_item = __hip_atomic_fetch_add(&queue[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - item_base;
            s_abort = 0;
        }
        __syncthreads();
        const unsigned item = __builtin_amdgcn_readfirstlane(s_item);   // (in a scalar register: the trip count below derives from it)
        if (item >= total) break;
        const unsigned level = item / items, tile = item - level * items;
        if (level > 0) {
            if (threadIdx.x < 3) {
                const int64_t t = (int64_t)tile - 1 + threadIdx.x;
                if (t >= 0 && t < (int64_t)items) {
                    unsigned spins = 0;
                    while ((int)(__hip_atomic_load(&done[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - (level_base + level)) < 0) {
                        __builtin_amdgcn_s_sleep(4);
                        if (++spins > STREAM_SPIN_LIMIT ||
                            ((spins & 255u) == 0 && __hip_atomic_load(sticky, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
                            __hip_atomic_store(sticky, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            s_abort = 1;
                            break;
                        }
                    }
                }
            }
            __syncthreads();
            if (s_abort) break;
        }
        const double* src;
        double* dst;
        unsigned nsub;
        int64_t first, clip;
        {   // (the arguments through the segment: see ChainArgs)
            ChainArgsPtr A = chain_args();
            double *const pA = A->bufA, *const pB = A->bufB, *const pC = A->bufC;
            const unsigned nlev = A->levels, KK = A->K, nlast = A->nsub_last;
            const int64_t olo = A->S.out_lo, ohi = A->S.out_hi, bnd = A->bound;
            src = (const double*)(const __attribute__((address_space(1))) double*)(pC ? (level == 0 ? pA : ((level & 1u) ? pB : pC)) : ((level & 1u) ? pB : pA));
            dst = (double*)(__attribute__((address_space(1))) double*)(pC ? (level + 1 == nlev ? pA : ((level & 1u) ? pC : pB)) : ((level & 1u) ? pA : pB));
            // the item's windows (all wave-uniform): window j has its thread 0 on local cell first + j W
            const bool chain = tile < chains;
            nsub = chain ? (tile + 1 == chains ? nlast : KK) : 1u;
            first = olo - H + (chain ? (int64_t)tile * (V + (int64_t)W * (KK - 1)) : bnd);
            clip = chain ? olo + bnd : ohi;
        }
#pragma unroll 1
        for (unsigned j = 0; j < nsub; j++) {
            int tid = threadIdx.x;
            asm volatile("" : "+v"(tid));   // opaque: what derives from the thread index is recomputed per window, not carried across the loops
            sb.rebind(tid);
            // An INTERIOR window - wholly inside the buffer, neither cell 0 nor cell N - 1 in it, wholly inside or wholly outside the
            // dissolution zone: all but three or four windows of a grid - is recognised once on the scalar side (wave-uniform).  Its
            // masks are constants and its loads need no guard: the per-lane 64-bit compares of set_window, the ballot and the
            // boundary selects run only in the other windows.  Same values either way.
            // (The tests are signs of 64-bit differences, formed modulo 2^64 - every operand is below 2^62 - and taken from the high
            // words: scalar subtractions and one 32-bit compare, where a signed 64-bit compare of two scalars is a vector instruction.)
            ChainArgsPtr A = chain_args();
            const int64_t n_buf = A->S.n_buf, goff = A->S.goff, ld = A->S.ld;
            const int64_t lw = first + (int64_t)j * W, gw = lw + goff;
            const int64_t mlo = C.mask_lo, mhi = C.mask_hi;
            // (each sign word opaque: combined freely, they are merged back into 64-bit values and compared on the vector side)
            auto neg = [](int64_t a, int64_t b) {   // < 0: a < b
                int32_t hi = (int32_t)(((uint64_t)a - (uint64_t)b) >> 32);
                asm("" : "+s"(hi));
                return hi;
            };
            const int32_t out_any = neg(lw, 0) | neg(n_buf, lw + BLK) | neg(gw, 1) | neg(C.N - 1, gw + BLK);   // < 0: not interior
            const int32_t zone_part = neg(gw, mlo) | neg(mhi, gw + BLK);       // >= 0: wholly inside the zone
            const int32_t zone_some = neg(mlo, gw + BLK) & neg(gw, mhi);       // >= 0: wholly outside
            const bool interior = out_any >= 0 && (zone_part >= 0 || zone_some >= 0);
            const int64_t l = lw + tid;
            bool in = true;
            int64_t la = l;   // the cell the lane loads: its own, or - outside the buffer - a valid one (the value is replaced below)
            if (!interior) {
                asm volatile("");   // a real branch
                in = l >= 0 && l < n_buf;
                la = in ? l : 0;
            }
            double y[NF];
#pragma unroll
            for (int f = 0; f < NF; f++) y[f] = __hip_atomic_load(src + at<LAYOUT>(f, la, ld), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (interior) {
                sb.set_interior(zone_part >= 0);
            } else {
                asm volatile("");
#pragma unroll
                for (int f = 0; f < NF; f++) y[f] = in ? y[f] : C.bc[f];
                sb.set_window_seam(gw);
            }
            sb.reuse_live = false;   // every window fills its own expansion centre, as an item of rk4_stream_kernel does
            // (the wave's number through readfirstlane: everything else is then scalar arithmetic; left to itself the compiler builds the
            // word per lane from lane masks)
            const int wave = __builtin_amdgcn_readfirstlane(tid) >> 6;
            sb.seam_pos = (int)(j & 1u) * 8 + (j ? SB::SEAM_READS : 0) + (wave == 0 ? SB::SEAM_WAVE0 : 0)
                          + (wave == (BLK - H - 1) / 64 ? SB::SEAM_WAVEW : 0);
            // the lanes that store, [lo, hi): both bounds are scalars of 32 bits.  hi - the window's end or the clip - is formed here, in front
            // of the evaluations (one word carried instead of the 64-bit clip); lo is read off the seam word behind them (a window with a left
            // halo of its own is the one that does not read the seam), where `j == 0` itself would be carried as a lane mask, a spilled pair.
            const int64_t room = clip - lw;
            int hi = neg(room, BLK - H) < 0 ? (int)room : BLK - H;
            asm volatile("" : "+s"(hi));
            rk4_advance<NSTEPS>(sb, y, dt);
            int sp = sb.seam_pos;
            asm volatile("" : "+s"(sp));
            const int lo = (sp & SB::SEAM_READS) ? 0 : H;
            int ts = threadIdx.x;
            asm volatile("" : "+v"(ts));    // (the cell index again: two registers less across the evaluations)
            const int64_t ls = first + (int64_t)j * W + ts;
            if (ts >= lo && ts < hi) {
                int64_t lds_ = 0;   // (the tiled layout has no field stride: no pointer to the segment is formed for it)
                if constexpr (LAYOUT == LAYOUT_FIELD_MAJOR) lds_ = chain_args()->S.ld;
#pragma unroll
                for (int f = 0; f < NF; f++) __hip_atomic_store(dst + at<LAYOUT>(f, ls, lds_), y[f], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
        __builtin_amdgcn_s_waitcnt(0);   // this thread's stores - of every window of the item - have been acknowledged
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
        __syncthreads();                 // ... and everybody else's (and everybody has read s_item, s_abort)
        if (threadIdx.x == 0) __hip_atomic_store(&done[tile], level_base + level + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---------------------------------------------------------------------------------------------
// Dormand-Prince 5(4) coefficients: scipy/integrate/_ivp/rk.py:377-391
// ---------------------------------------------------------------------------------------------
namespace dp {
constexpr double A21 = 1.0 / 5;
constexpr double A31 = 3.0 / 40, A32 = 9.0 / 40;
constexpr double A41 = 44.0 / 45, A42 = -56.0 / 15, A43 = 32.0 / 9;
constexpr double A51 = 19372.0 / 6561, A52 = -25360.0 / 2187, A53 = 64448.0 / 6561, A54 = -212.0 / 729;
constexpr double A61 = 9017.0 / 3168, A62 = -355.0 / 33, A63 = 46732.0 / 5247, A64 = 49.0 / 176, A65 = -5103.0 / 18656;
constexpr double B1 = 35.0 / 384, B3 = 500.0 / 1113, B4 = 125.0 / 192, B5 = -2187.0 / 6784, B6 = 11.0 / 84;
constexpr double E1 = -71.0 / 57600, E3 = 71.0 / 16695, E4 = -71.0 / 1920, E5 = 17253.0 / 339200, E6 = -22.0 / 525, E7 = 1.0 / 40;
constexpr double SAFETY = 0.9, MIN_FACTOR = 0.2, MAX_FACTOR = 10.0;
// Dense output P (scipy/integrate/_ivp/rk.py:393-407): w_j(x) = sum_m P[j][m] x^(m+1); host (dense_eval) and device (dense_weights)
constexpr double P[7][4] = {
    {1, -8048581381.0 / 2820520608, 8663915743.0 / 2820520608, -12715105075.0 / 11282082432},
    {0, 0, 0, 0},
    {0, 131558114200.0 / 32700410799, -68118460800.0 / 10900136933, 87487479700.0 / 32700410799},
    {0, -1754552775.0 / 470086768, 14199869525.0 / 1410260304, -10690763975.0 / 1880347072},
    {0, 127303824393.0 / 49829197408, -318862633887.0 / 49829197408, 701980252875.0 / 199316789632},
    {0, -282668133.0 / 205662961, 2019193451.0 / 616988883, -1453857185.0 / 822651844},
    {0, 40617522.0 / 29380423, -110615467.0 / 29380423, 69997945.0 / 29380423}};
}  // namespace dp


// (ST_* and struct Rk45Ctrl, the device-resident step controller: marl_rk_ctrl.h)

// Top of RungeKutta._step_impl: choose the step of the next attempt (rk.py:119-142).
__device__ __forceinline__ void rk45_prepare_attempt(Rk45Ctrl& c)
{
    const double min_step = 10.0 * fabs(nextafter(c.t, __builtin_inf()) - c.t);
    if (!c.rejected) {
        if (c.h_abs < min_step) c.h_abs = min_step;
    } else if (c.h_abs < min_step) {
        c.status = ST_TOO_SMALL;
        return;
    }
    if (c.max_attempts > 0 && c.attempts >= c.max_attempts) {
        c.status = ST_BUDGET;
        return;
    }
    double t_new = c.t + c.h_abs;
    if (t_new - c.t_bound > 0.0) t_new = c.t_bound;
    c.t_new = t_new;
    c.h_try = t_new - c.t;
    c.h_abs = fabs(c.h_try);
    c.attempts++;
}

// Bottom of _step_impl + the driver's per-step bookkeeping, in three pieces (rk45_finish_attempt = all three in order):
//   rk45_decide         error norm -> accept / reject and the step-size factor (rk.py:146-165)
//   rk45_events         the seven monitors of an accepted step against those of the step before (ivp.py:149-151, :673-694)
//   rk45_advance_status end of interval / pause, and the next attempt's step (rk.py:119-142)
// The one-workgroup sweep kernel runs decide + advance_status in EVERY wave (replicated scalar work, no publish barrier) and the
// event bookkeeping one barrier later, off the critical path.
// T: the log / exp tables when the caller has them in LDS: err^-0.2 is then exp(-0.2 log err) at a fifth of OCML pow's
// instructions, ~3 ulp instead of 1.
__device__ __forceinline__ bool rk45_decide(Rk45Ctrl& c, double sumsq, const Tables* T = nullptr)
{
    const double err = sqrt(sumsq) / sqrt((double)c.n_total);  // common.py:63-65
    c.err_norm = err;
    c.nfev += 6;
    double f;
    if (T && err > 1e-300 && err < 1e300) f = dp::SAFETY * fast_exp(-0.2 * fast_log(err, *T), *T);
    else f = dp::SAFETY * pow(err, -0.2);
    if (err < 1.0) {  // rk.py:149-161
        double factor = (err == 0.0) ? dp::MAX_FACTOR : ((f < dp::MAX_FACTOR) ? f : dp::MAX_FACTOR);
        if (c.rejected && !(factor < 1.0)) factor = 1.0;
        c.h_abs *= factor;
        c.accepted_last = 1;
        c.rejected = 0;
        c.n_acc++;
        c.t_old = c.t;
        c.h_prev = c.h_try;
        c.t = c.t_new;
        c.cur ^= 1;
        return true;
    }
    // rk.py:162-165; a NaN norm lands here with factor 0.2
    c.h_abs *= (f > dp::MIN_FACTOR) ? f : dp::MIN_FACTOR;
    c.accepted_last = 0;
    c.rejected = 1;
    c.n_rej++;
    return false;
}

// The same decision from the MEAN square error (sum / n) for the replicated controller of the one-workgroup sweep kernel, where
// every wave pays for these instructions: err < 1 <=> err^2 < 1, and 0.9 err^-0.2 = 0.9 exp(-0.1 log err^2) - no square roots, no
// division (inv_n = 1 / n_total, formed once), always through the LDS tables.  c.err_norm holds err^2 until the kernel leaves
// (rk45_lean_finish).  Against rk45_decide the factor differs in the last bits (as the table path does from OCML pow already).
__device__ __forceinline__ bool rk45_decide_lean(Rk45Ctrl& c, double sumsq, double inv_n, const Tables& T)
{
    const double e2 = sumsq * inv_n;
    c.err_norm = e2;
    c.nfev += 6;
    double f;
    if (e2 > 1e-300 && e2 < 1e300) f = dp::SAFETY * fast_exp(-0.1 * fast_log(e2, T), T);
    else f = dp::SAFETY * pow(sqrt(e2), -0.2);
    if (e2 < 1.0) {
        double factor = (e2 == 0.0) ? dp::MAX_FACTOR : ((f < dp::MAX_FACTOR) ? f : dp::MAX_FACTOR);
        if (c.rejected && !(factor < 1.0)) factor = 1.0;
        c.h_abs *= factor;
        c.accepted_last = 1;
        c.rejected = 0;
        c.n_acc++;
        c.t_old = c.t;
        c.h_prev = c.h_try;
        c.t = c.t_new;
        c.cur ^= 1;
        return true;
    }
    c.h_abs *= (f > dp::MIN_FACTOR) ? f : dp::MIN_FACTOR;
    c.accepted_last = 0;
    c.rejected = 1;
    c.n_rej++;
    return false;
}

// rk45_prepare_attempt with the minimum-step test (10 ulp(t)) behind a cheap sufficient condition: h_abs > |t| 2^-48 > 10 ulp(t)
// holds on every attempt of a healthy run, and nextafter costs ~20 instructions in every wave
__device__ __forceinline__ void rk45_prepare_attempt_lean(Rk45Ctrl& c)
{
    if (!(c.h_abs > fabs(c.t) * 0x1p-48) || c.t == 0.0) {   // (t = 0: nextafter gives the smallest subnormal)
        rk45_prepare_attempt(c);
        return;
    }
    if (c.max_attempts > 0 && c.attempts >= c.max_attempts) {
        c.status = ST_BUDGET;
        return;
    }
    double t_new = c.t + c.h_abs;
    if (t_new - c.t_bound > 0.0) t_new = c.t_bound;
    c.t_new = t_new;
    c.h_try = t_new - c.t;
    c.h_abs = fabs(c.h_try);
    c.attempts++;
}

// Monitor e of the step just accepted ([c.t_old, c.t], size c.h_prev): gn against the stored c.g[e]; returns 1 on a sign change.
__device__ __forceinline__ int rk45_event_one(Rk45Ctrl& c, int e, double gn)
{
    const double go = c.g[e];
    int fired = 0;
    const bool up = go <= 0.0 && gn >= 0.0, down = go >= 0.0 && gn <= 0.0;  // ivp.py:149-151
    if (up || down) {
        const double d = go - gn;
        const double tc = (d != 0.0) ? c.t_old + c.h_prev * (go / d) : c.t;
        if (c.n_events[e] == 0) c.ev_first[e] = tc;
        c.ev_last[e] = tc;
        c.n_events[e]++;
        fired = 1;
    }
    c.g[e] = gn;
    return fired;
}

// monitor e (the reference's order, Evolve_scenario.py:107-109) from a reduction record {sum, min y, min CA, min CC, min U, max CA+CC, max Phi, max W}
__device__ __forceinline__ double rk45_monitor_of_record(const double* rec, int e)
{
    const int slot = (e < 3) ? e + 1 : (e == 3 ? 5 : (e == 4 ? 6 : (e == 5 ? 4 : 7)));
    return (e == 3 || e == 4) ? rec[slot] - 1.0 : rec[slot];
}

// the record slot (1..7) behind monitor e, as rk45_monitor_of_record reads it; monitors 3 and 4 are that slot minus one
__device__ __forceinline__ int rk45_monitor_slot(int e)
{
    return (e < 3) ? e + 1 : (e == 3 ? 5 : (e == 4 ? 6 : (e == 5 ? 4 : 7)));
}

__device__ __forceinline__ int rk45_events(Rk45Ctrl& c, const double (&rec)[NQ])
{
    int fired = 0;
#pragma unroll
    for (int e = 0; e < 7; e++) fired |= rk45_event_one(c, e, rk45_monitor_of_record(rec, e));
    return fired;
}

__device__ __forceinline__ void rk45_advance_status(Rk45Ctrl& c, bool accepted, int fired)
{
    if (accepted) {
        if (c.t - c.t_bound >= 0.0) {  // base.py:203-204
            c.status = ST_DONE;
        } else if (c.t >= c.pause_t || (fired && c.pause_on_event)) {
            c.status = ST_PAUSED;
            c.event_fired = fired;
        }
    }
    if (c.status == ST_RUNNING) rk45_prepare_attempt(c);
}

// rk45_advance_status after an ACCEPTED step of a run that does not pause on monitor sign changes (the events are then pure
// bookkeeping and may follow later)
__device__ __forceinline__ void rk45_advance_status_no_events(Rk45Ctrl& c)
{
    if (c.t - c.t_bound >= 0.0) c.status = ST_DONE;
    else if (c.t >= c.pause_t) c.status = ST_PAUSED;
    if (c.status == ST_RUNNING) rk45_prepare_attempt(c);
}

// rec = {sum (err/scale)^2, monitors of y_new}.
__device__ __forceinline__ void rk45_finish_attempt(Rk45Ctrl& c, const double (&rec)[NQ], const Tables* T = nullptr)
{
    const bool accepted = rk45_decide(c, rec[0], T);
    const int fired = accepted ? rk45_events(c, rec) : 0;
    rk45_advance_status(c, accepted, fired);
}

// rec0: monitors record of y(t0).  RungeKutta.__init__ (rk.py:94-102) + ivp.py:645.
__global__ void rk45_init_kernel(Rk45Ctrl* ctrl, const double* __restrict__ rec0, double t0, double t1, double first_step,
                                 double rtol, double atol, int64_t n_total, int64_t max_attempts, int32_t cur)
{
    Rk45Ctrl c = {};
    c.t = t0; c.t_bound = t1; c.h_abs = first_step; c.rtol = rtol; c.atol = atol;
    c.t_old = t0; c.pause_t = __builtin_inf();
    c.n_total = n_total; c.max_attempts = max_attempts; c.cur = cur;
    c.nfev = 1;
    c.status = (t0 == t1) ? ST_DONE : ST_RUNNING;  // base.py:189-194
    const double* r = rec0 + (int64_t)blockIdx.x * NQ;
    const double g0[7] = {r[1], r[2], r[3], r[5] - 1.0, r[6] - 1.0, r[4], r[7]};
    for (int e = 0; e < 7; e++) c.g[e] = g0[e];
    if (c.status == ST_RUNNING) rk45_prepare_attempt(c);
    ctrl[blockIdx.x] = c;
}

// Resume a paused / budget-stopped controller (host sets new pause_t / max_attempts first).
__global__ void rk45_resume_kernel(Rk45Ctrl* ctrl, double pause_t, int64_t max_attempts)
{
    Rk45Ctrl& c = ctrl[blockIdx.x];
    c.pause_t = pause_t;
    c.max_attempts = max_attempts;
    if (c.status == ST_PAUSED || c.status == ST_BUDGET) {
        c.status = ST_RUNNING;
        c.event_fired = 0;
        rk45_prepare_attempt(c);
    }
}

// Combine `nrec` reduction records (per-block partials on one GPU, or one record per rank after the
// all-gather of a domain-decomposed run) in index order and finish the attempt.
// One workgroup of 512 threads: with thousands of block records the reduction is latency-bound, so it is spread
// over many lanes (4 300 records at N = 2^20: ~8 per thread).
constexpr int CONTROL_THREADS = 512;
__global__ void __launch_bounds__(CONTROL_THREADS) rk45_control_kernel(const double* __restrict__ recs, int64_t nrec, Rk45Ctrl* ctrl)
{
    __shared__ double scratch[NQ * CONTROL_THREADS];
#ifdef MARL_CTL_CLOCK
    const unsigned long long c0 = __builtin_amdgcn_s_memrealtime();
#endif
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
#ifdef MARL_CTL_CLOCK
    const unsigned long long c1 = __builtin_amdgcn_s_memrealtime();
#endif
    block_reduce<CONTROL_THREADS, NQ, NQMIN>(q, scratch);
#ifdef MARL_CTL_CLOCK
    const unsigned long long c2 = __builtin_amdgcn_s_memrealtime();
#endif
    if (threadIdx.x == 0) {
        Rk45Ctrl c = *ctrl;
        rk45_finish_attempt(c, q);
        *ctrl = c;
#ifdef MARL_CTL_CLOCK
        const unsigned long long c3 = __builtin_amdgcn_s_memrealtime();
        if (c.attempts == 300) printf("CTLCLOCK load %llu reduce %llu finish %llu (x10 ns)\n", c1 - c0, c2 - c1, c3 - c2);
#endif
    }
}

// One Dormand-Prince attempt on the per-thread cells: k1 given; returns y_new in `yn`, f(y_new) in `k7`
// and the error-estimate numerator  sum_j E_j K_j  in `esum` (rk_step, rk.py:61-69; _estimate_error :103-104).
// With DENSE, `esum` instead receives  sum_j w_j K_j  for the dense-output weights w_j = sum_m P[j][m] x^(m+1)
// (RkDenseOutput, rk.py:560-574; w_2 = 0 because row 2 of P is zero).
struct DenseWeights { double w[7]; };

// PARK = number of fields (0..5) of the step's first state y that are NOT held in registers but in this thread's LDS column
// `pk` (pk[f * BLK], f < PARK) and re-read where a stage state is formed - up to five live doubles less across every
// evaluation (kernels that sit just above a register cap: 128 VGPRs = 4 waves per SIMD).
// EITHER (rk45_sweep_eval_kernel; DENSE = false): one call site serves attempts and dense-output replays - `esum` is summed with the
// weights `dw` when `dense_now` (workgroup-uniform) and with the constants E_j otherwise, in two separate blocks.  The constant block
// is the statement of the plain attempt, so that it is compiled as there (with E_j as run-time values the compiler rounds other
// products of  k1 E1 + k3 E3 + ...: E1, E4, E6 are negative, and  a + x (-c)  becomes  a - x c  before the multiply-adds are formed);
// the run-time block hands its sums through an empty asm, which keeps the optimiser from merging the two blocks into one with selected
// operands (phi of two sums -> sum of phis: the weights would be run-time values again, and the multiply and the add end up in
// different blocks, unfused).
template <int BLK, bool DENSE = false, class SB = StencilBlock<BLK>, int PARK = 0, bool EITHER = false>
__device__ __forceinline__ void dp45_attempt(SB& sb, double h, const double (&y)[NF], const double (&k1)[NF],
                                             double (&yn)[NF], double (&k7)[NF], double (&esum)[NF],
                                             PointAux& aux, const DenseWeights& dw = DenseWeights{}, const double* pk = nullptr,
                                             bool dense_now = false)
{
    static_assert(!(EITHER && DENSE), "EITHER chooses at run time");
#define MARL_SEPARATE_BLOCKS() MARL_FIELDS asm volatile("" : "+v"(esum[f]))
    const double e1 = DENSE ? dw.w[0] : dp::E1, e3 = DENSE ? dw.w[2] : dp::E3, e4 = DENSE ? dw.w[3] : dp::E4;
    const double e5 = DENSE ? dw.w[4] : dp::E5, e6 = DENSE ? dw.w[5] : dp::E6, e7 = DENSE ? dw.w[6] : dp::E7;
    // K1..K4 are folded into the partial sums of everything that still needs them as soon as K4 exists, so that at
    // most five vectors (instead of seven) are live across an evaluation.  The order of every
    // sum is the left-to-right order of np.dot(K[:s].T, a[:s]) (rk.py:61-69).
    double ys[NF], k2[NF], k3[NF], k4[NF], kk[NF], s6[NF], bn[NF];
#define MARL_Y(f) ((f) < PARK ? pk[(f) * BLK] : y[f])
    MARL_FIELDS ys[f] = MARL_Y(f) + (k1[f] * dp::A21) * h;
    sb.template eval<TR_FILL>(ys, k2, aux);
    MARL_FIELDS ys[f] = MARL_Y(f) + (k1[f] * dp::A31 + k2[f] * dp::A32) * h;
    sb.template eval<TR_REUSE>(ys, k3, aux);
    MARL_FIELDS ys[f] = MARL_Y(f) + (k1[f] * dp::A41 + k2[f] * dp::A42 + k3[f] * dp::A43) * h;
    sb.template eval<TR_REUSE>(ys, k4, aux);
    MARL_FIELDS {
        ys[f] = MARL_Y(f) + (k1[f] * dp::A51 + k2[f] * dp::A52 + k3[f] * dp::A53 + k4[f] * dp::A54) * h;
        s6[f] = k1[f] * dp::A61 + k2[f] * dp::A62 + k3[f] * dp::A63 + k4[f] * dp::A64;
        bn[f] = k1[f] * dp::B1 + k3[f] * dp::B3 + k4[f] * dp::B4;
        if constexpr (!EITHER) esum[f] = k1[f] * e1 + k3[f] * e3 + k4[f] * e4;
    }
    if constexpr (EITHER) {
        if (dense_now) {
            MARL_FIELDS esum[f] = k1[f] * dw.w[0] + k3[f] * dw.w[2] + k4[f] * dw.w[3];
            MARL_SEPARATE_BLOCKS();
        } else {
            MARL_FIELDS esum[f] = k1[f] * dp::E1 + k3[f] * dp::E3 + k4[f] * dp::E4;
        }
    }
    sb.template eval<TR_REUSE>(ys, kk, aux);   // K5
    MARL_FIELDS {
        ys[f] = MARL_Y(f) + (s6[f] + kk[f] * dp::A65) * h;
        bn[f] = bn[f] + kk[f] * dp::B5;
        if constexpr (!EITHER) esum[f] = esum[f] + kk[f] * e5;
    }
    if constexpr (EITHER) {
        if (dense_now) {
            MARL_FIELDS esum[f] = esum[f] + kk[f] * dw.w[4];
            MARL_SEPARATE_BLOCKS();
        } else {
            MARL_FIELDS esum[f] = esum[f] + kk[f] * dp::E5;
        }
    }
    sb.template eval<TR_REUSE>(ys, kk, aux);   // K6
    MARL_FIELDS {
        yn[f] = MARL_Y(f) + h * (bn[f] + kk[f] * dp::B6);
        if constexpr (!EITHER) esum[f] = esum[f] + kk[f] * e6;
    }
    if constexpr (EITHER) {
        if (dense_now) {
            MARL_FIELDS esum[f] = esum[f] + kk[f] * dw.w[5];
            MARL_SEPARATE_BLOCKS();
        } else {
            MARL_FIELDS esum[f] = esum[f] + kk[f] * dp::E6;
        }
    }
    sb.template eval<TR_REUSE>(yn, k7, aux);
    if constexpr (EITHER) {
        if (dense_now) {
            MARL_FIELDS esum[f] = esum[f] + k7[f] * dw.w[6];
            MARL_SEPARATE_BLOCKS();
        } else {
            MARL_FIELDS esum[f] = esum[f] + k7[f] * dp::E7;
        }
    } else {
        MARL_FIELDS esum[f] = esum[f] + k7[f] * e7;
    }
#undef MARL_SEPARATE_BLOCKS
#undef MARL_Y
}

// (err/scale)^2 of one component; scale = atol + max(|y|, |y_new|) * rtol  (rk.py:146-147)
__device__ __forceinline__ double dp45_err2(double esum, double h, double y, double yn, double rtol, double atol)
{
    const double ay = fabs(y), an = fabs(yn);
    const double scale = atol + ((ay > an || ay != ay) ? ay : an) * rtol;
    const double e = esum * h * rcp_nr(scale);
    return e * e;
}

// ---------------------------------------------------------------------------------------------
// Reduction of a tile's eight quantities over its 256 threads with ONE barrier (round 4; the round-1 block_reduce takes four).
// Each thread writes its q[j] into column j of an LDS area [8][BLK]; after the barrier HALF-WAVE j (32 lanes) reduces column j:
// lane i combines rows i, i + 32, ..., i + 224 in that order, then a 5-step butterfly over the 32 lanes - a fixed order.
// Quantity 0 is a sum (NaN-propagating), 1..NQMIN minima, the rest maxima, carried NEGATED through the columns so that every
// half-wave but the first runs the same v_min_f64 (finite values: see monitors_accumulate<true>).  Result in lane 0 of half-wave j
// (threads 0, 32, ..., 224), maxima still negated; other lanes hold garbage.
// Where the columns live when a Dormand-Prince attempt has just finished (no barrier needed in FRONT of the writes): columns 0..6 =
// the four cache-slot columns + the three park columns (contiguous; both hold thread-PRIVATE data that the thread has finished
// with), column 7 = field 0 of the parity-0 edge buffer (last read in the fifth evaluation; every wave has passed the sixth's
// barrier).  The caller must put a barrier between this function's reads and the next writes to those areas.
// ---------------------------------------------------------------------------------------------
template <int BLK>
__device__ __forceinline__ double* attempt_reduce_column(double* lds, int edge_doubles, int j)
{
    return j < 7 ? lds + edge_doubles + TABLE_DOUBLES + j * BLK : lds;
}
template <int BLK, class SB>
__device__ __forceinline__ double tile_reduce_halfwaves(const double (&q)[NQ], double* lds, int tid)
{
    static_assert(BLK == 256 && NQ == 8, "eight quantities, eight half-waves");
    static_assert(PC_LDS_SLOTS >= 4 && SB::CACHE, "columns 0..6 = the cache-slot columns (four at least) + three park columns");
#pragma unroll
    for (int j = 0; j < NQ; j++) attempt_reduce_column<BLK>(lds, SB::EDGE_DOUBLES, j)[tid] = (j > NQMIN) ? -q[j] : q[j];
    __syncthreads();
    const int j = tid >> 5, i = tid & 31;
    const bool is_sum = j == 0;
    const double* col = (j < 7 ? lds + SB::EDGE_DOUBLES + TABLE_DOUBLES + j * BLK : lds) + i;
    double a = col[0];
#pragma unroll
    for (int m = 1; m < BLK / 32; m++) {
        const double o = col[32 * m];
        a = is_sum ? a + o : __builtin_fmin(a, o);
    }
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) {
        const double o = __shfl_xor(a, off, 64);
        a = is_sum ? a + o : __builtin_fmin(a, o);
    }
    return a;
}

// ---------------------------------------------------------------------------------------------
// Fused adaptive attempt for ONE large grid (or one slab of a domain-decomposed grid): reads
// (y, f) from buffer `cur`, writes (y_new, f_new) into the other buffer and one reduction record per
// block; rk45_control_kernel then accepts (flips `cur`) or rejects.  FSAL: f_new becomes K1.
// ---------------------------------------------------------------------------------------------
// 256-thread blocks: 4 waves per SIMD (<= 128 VGPRs) with ATTEMPT_PARK fields of y parked in LDS
// (4 blocks per CU leave 9 KB of LDS per block beside the edge buffers, tables and cache slots; three parked doubles = 6 KB suffice: 128 VGPRs, no scratch).
#ifndef MARL_ATTEMPT_PARK
#define MARL_ATTEMPT_PARK 3
#endif
template <int BLK>
constexpr int ATTEMPT_PARK = (BLK == 256) ? MARL_ATTEMPT_PARK : 0;

template <int BLK, int LAYOUT, bool VD = false>
__global__ void __launch_bounds__(BLK) __attribute__((amdgpu_waves_per_eu((BLK == 256 && MARL_ATTEMPT_PARK > 0) ? 4 : 1, 8)))
rk45_attempt_kernel(double* __restrict__ Y0, double* __restrict__ Y1,
                                                           double* __restrict__ F0, double* __restrict__ F1,
                                                           const DevConsts* __restrict__ consts, Slab S,
                                                           const Rk45Ctrl* __restrict__ ctrl, double* __restrict__ part)
{
    constexpr int H = 6;
    constexpr int V = BLK - 2 * H;
    constexpr int PARK = ATTEMPT_PARK<BLK>;
    using SB = StencilBlock<BLK, true, VD>;
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

    double y[NF], k1[NF], yn[NF], k7[NF], esum[NF];
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
    dp45_attempt<BLK, false, SB, PARK>(sb, h, y, k1, yn, k7, esum, aux, DenseWeights{}, pk);

    double q[NQ];
    monitors_init(q);
    const int wi = threadIdx.x;
    MARL_ONCE if (wi >= H && wi < BLK - H && l >= S.out_lo && l < S.out_hi) {
#pragma unroll
        for (int f = 0; f < NF; f++) {
            yout[at<LAYOUT>(f, l, S.ld)] = yn[f];
            fout[at<LAYOUT>(f, l, S.ld)] = k7[f];
            q[0] += dp45_err2(esum[f], h, f < PARK ? pk[f * BLK] : y[f], yn[f], rtol, atol);
        }
        monitors_accumulate<true>(q, yn, aux.U, aux.W);   // (the controller reads the extrema of ACCEPTED attempts only: all finite)
    }
#ifndef MARL_LAB_ATTEMPT_BLOCK_REDUCE   // (kernel-lab switch: the round-1 four-barrier reduction)
    if constexpr (BLK == 256 && PARK >= 3 && SB::CACHE && PC_LDS_SLOTS >= 4) {
        // one barrier instead of four: columns in LDS areas this thread / every wave has finished with (tile_reduce_halfwaves)
        const double r = tile_reduce_halfwaves<BLK, SB>(q, lds, threadIdx.x);
        if ((threadIdx.x & 31) == 0) {
            const int j = threadIdx.x >> 5;
            part[(int64_t)blockIdx.x * NQ + j] = (j > NQMIN) ? -r : r;
        }
    } else
#endif
    {
        block_reduce<BLK, NQ, NQMIN, true>(q, lds);   // the edge-exchange buffers are free now
        if (threadIdx.x == 0) {
#pragma unroll
            for (int j = 0; j < NQ; j++) part[(int64_t)blockIdx.x * NQ + j] = q[j];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The whole adaptive loop of ONE large grid in ONE launch (round 4): resident workgroups, one device-wide barrier per attempt.
//
// What a launch per attempt costs (rk45_attempt_kernel, N = 2^20: 63 us + two small launches): every workgroup pays a prologue
// (kernel arguments -> the controller's cur / h -> the state loads that depend on cur -> tables into LDS -> barrier), a four-barrier
// block reduction, and the dispatcher's turnover of its slot; 4 297 tiles on 1 024 slots leave a fifth, 20 % filled round.  Here a
// grid of G resident workgroups (4 per CU) stages the tables once, keeps (h, cur, status) in scalar registers and walks a STATIC
// set of tiles per attempt (tile = g, g + G, ...; the remainder round is SPREAD over the grid, see extra_tile) with the loads of the
// next tile in flight while the present one is reduced; the attempt ends in ONE barrier across the grid:
//   * each workgroup folds its tiles' records (tile order) into one group record: the sum of squares into gsum[g], the seven
//     extrema into gmon[g][7] (sc1 stores), waits for all its stores to be acknowledged, and takes a ticket (one agent-scope atomic);
//   * the workgroup that takes the LAST ticket of the attempt adds the G sums in a fixed order (thread t: groups t, t + BLK, ...;
//     wave butterflies; waves in order - deterministic, independent of who is last), takes scipy's accept / reject and step-size
//     decision (rk45_decide, the function the control kernel runs) and PUBLISHES what the next attempt needs - h, cur, status, the
//     barrier's number - as one 16-byte record replicated over PUB_COPIES cache lines; only then, off the critical path, it reduces
//     the extrema of an accepted step, does the event bookkeeping and writes the controller back (pause_on_event: the events
//     decide the status, so they come first);
//   * everybody polls its copy of the record (bounded; a time-out raises the sticky flag and every workgroup leaves).
// Coherence across the 8 XCDs as in rk4_stream_kernel: state, records and the controller move with agent-scope (sc1) loads /
// stores; a ticket is taken only after s_waitcnt vmcnt(0) + barrier.  Needs all G workgroups resident at once (the host sizes G by
// hipOccupancyMaxActiveBlocksPerMultiprocessor); counters are never reset between launches (arrive_base / epoch_base say where
// they stand).  The published record carries a 24-bit hash of h beside the barrier number, so a torn read cannot pass.
// ---------------------------------------------------------------------------------------------
// a value that is the same in every lane, moved into scalar registers (readfirstlane)
__device__ __forceinline__ double to_sgpr(double v)
{
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}
__device__ __forceinline__ int32_t to_sgpr(int32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int64_t to_sgpr(int64_t v)
{
    return (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int32_t)((uint64_t)v >> 32)) << 32) |
                     (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)(uint32_t)v));
}
constexpr int MON_STRIDE = 16;          // doubles between the grid-wide extrema (one 128-byte line each)
constexpr int MON_OFFSET = 4096;        // grec: [0, MON_OFFSET) the workgroups' sums, then [2][NQ - 1][MON_STRIDE] extrema
constexpr int GREC_DOUBLES = MON_OFFSET + 2 * (NQ - 1) * MON_STRIDE;
constexpr int PUB_COPIES = 32;          // replicas of the published record, PUB_STRIDE words apart (pollers spread over channels)
constexpr int PUB_STRIDE = 32;          // 64-bit words (256 B)
struct Rk45Stream {
    unsigned arrive;                    // tickets taken since the words were zeroed
    unsigned sticky;                    // raised by a workgroup that gave up waiting
    unsigned pad0[30];
    unsigned grab;                      // remainder-round tiles handed out (own cache line)
    unsigned pad1[31];
    unsigned long long pub[PUB_COPIES * PUB_STRIDE];   // copy k: pub[k * PUB_STRIDE + 0] = bits of h_try, [+ 1] = hash24(h) << 40 | epoch << 8 | (status + 1) << 1 | cur
};
__device__ __forceinline__ unsigned long long pub_word(unsigned long long hbits, unsigned epoch, int status, int cur)
{
    const unsigned long long hash = (hbits ^ (hbits >> 24) ^ (hbits >> 48)) & 0xffffffull;
    return (hash << 40) | ((unsigned long long)epoch << 8) | (unsigned long long)(((status + 1) & 7) << 1) | (unsigned long long)(cur & 1);
}
// The tiles of an attempt: `full` = tiles / G rounds are STATIC (workgroup g: tiles g, g + G, ...; the next tile's loads in flight
// while the present one is reduced); the R = tiles mod G tiles of the remainder round are handed out by an atomic counter to whoever
// has finished its static tiles.  The SIMDs arbitrate oldest-first, so the four workgroups of a CU finish their static tiles one
// after the other (measured at N = 2^20: after 31 ... 65 us) and the remainder goes to the early finishers, about one per CU - a
// static owner (every ~G/R-th workgroup) left some CUs with 18 tiles and others with 16 (profiles/r04_lab_rk45_stream.log).
// Determinism: a static tile's sum of squares goes into its workgroup's sum (tile order), a remainder tile's into its own slot
// gextra[e]; the barrier's last workgroup adds G + R numbers in index order - the same numbers whoever computed them; extrema are
// exact under any order.  The counter is never reset: every attempt takes exactly R successful and G failing grabs.
#ifdef MARL_LAB_CLOCK45  // kernel-lab diagnostic build only: s_memrealtime (100 MHz) stamps per (attempt < 64, workgroup < 2048): attempt start, tiles done, ticket taken, decision seen
__device__ unsigned long long marl_lab_clock45[64 * 2048 * 4 + 64 * 8];   // (+ the last arriver's phases: [64][8])
#define MARL_STAMP45(k) do { if (threadIdx.x == 0 && a < 64 && g < 2048) marl_lab_clock45[(a * 2048 + g) * 4 + (k)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define MARL_STAMP45L(k) do { if (threadIdx.x == 0 && a < 64) marl_lab_clock45[64 * 2048 * 4 + a * 8 + (k)] = __builtin_amdgcn_s_memrealtime(); } while (0)
__device__ unsigned long long marl_lab_clock45t[2048 * 8 * 8];   // tiles of attempt 20: [g][tile index < 8][phase < 8]
#define MARL_STAMP45T(k) do { if (threadIdx.x == 0 && a == 20 && g < 2048 && ti < 8 && tile < tiles) marl_lab_clock45t[(g * 8 + ti) * 8 + (k)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define MARL_STAMP45(k) do { } while (0)
#define MARL_STAMP45L(k) do { } while (0)
#define MARL_STAMP45T(k) do { } while (0)
#endif
#ifdef MARL_LAB_STREAM_PLAIN   // kernel-lab cost probe ONLY (results are wrong across XCDs): the state through the non-coherent L2s
#define MARL_STREAM_LOAD(p) (*(p))
#define MARL_STREAM_STORE(p, v) (*(p) = (v))
#else
#define MARL_STREAM_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define MARL_STREAM_STORE(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#endif
#ifndef MARL_STREAM_PARK   // fields of y parked in LDS (dp45_attempt): 4 leave LDS for exactly four workgroups per CU (40 448 of 40 960 bytes)
#define MARL_STREAM_PARK 4
#endif
template <int BLK, int LAYOUT, bool VD = false, bool DD = false>
__global__ void __launch_bounds__(BLK) __attribute__((amdgpu_waves_per_eu(4, 8)))
rk45_stream_kernel(double* Y0, double* Y1, double* F0, double* F1, const DevConsts* __restrict__ consts, Slab S, Rk45Ctrl* ctrl,
                   double* grec, Rk45Stream* sync, unsigned tiles, unsigned arrive_base, unsigned epoch_base, unsigned grab_base, unsigned max_attempts,
                   double* send = nullptr, int halo = 0)
{
    // DD (one slab of a domain-decomposed grid; max_attempts = 1, all three bases 0; option dd_stream): ONE attempt per launch, and the
    // barrier's last workgroup, instead of deciding, writes the rank's message [record (8) | lower strip | upper strip] (what
    // reduce_chunks_kernel + slab_reduce_pack_kernel did) and re-arms the counters; the all-gather and slab_unpack_control_kernel
    // follow, and the next launch reads the common decision out of *ctrl.
    constexpr int H = 6;
    constexpr int V = BLK - 2 * H;
    constexpr int PARK = MARL_STREAM_PARK;
    constexpr int NW = BLK / 64;
    constexpr int CTRL_WORDS = (int)(sizeof(Rk45Ctrl) / 8);
    static_assert(sizeof(Rk45Ctrl) % 8 == 0 && CTRL_WORDS <= BLK, "the controller moves as 64-bit words, one per thread");
    static_assert(PARK >= 3, "the reduction columns of a tile use three park columns");
    using SB = StencilBlock<BLK, true, VD>;
    __shared__ double lds[SB::LDS_DOUBLES + PARK * BLK];
    __shared__ double s_acc[NQ];         // this workgroup's record of the attempt (maxima negated), slot j touched by thread 32 j only
    __shared__ double s_wsum[NW];
    __shared__ double s_rec[NQ];         // last workgroup of a barrier: the grid's record {-, seven extrema of y_new}
    __shared__ Rk45Ctrl sc;
    __shared__ unsigned long long s_pub[2];
    __shared__ int s_last, s_abort;
    __shared__ unsigned s_next;
    SB sb(lds, 0, consts);   // tables once per workgroup (barrier inside)
    const unsigned G = gridDim.x, g = blockIdx.x;
    const unsigned n_full = tiles / G, R = tiles - n_full * G;         // n_full >= 1: the host launches G <= tiles workgroups
    double* const gsum = grec;                      // [G + R]: the workgroups' sums of squares over their static tiles, then the remainder tiles' sums
    double* const gmon = grec + MON_OFFSET;         // [2][NQ - 1][MON_STRIDE]: the grid's seven extrema (maxima negated) by attempt parity, +inf when idle
    // the controller as the previous launch (or rk45_init / rk45_resume) left it
    int cur = ctrl->cur, status = ctrl->status;
    double h = ctrl->h_try;
    const double rtol = ctrl->rtol, atol = ctrl->atol;
    const int pause_on_event = ctrl->pause_on_event;
    unsigned long long* const my_pub = sync->pub + (g % PUB_COPIES) * PUB_STRIDE;


    for (unsigned a = 0; a < max_attempts && status == ST_RUNNING; a++) {
        const double* yin = cur ? Y1 : Y0;
        const double* fin = cur ? F1 : F0;
        double* yout = cur ? Y0 : Y1;
        double* fout = cur ? F0 : F1;
        MARL_STAMP45(0);
#ifdef MARL_LAB_CLOCK45
        if (threadIdx.x == 0 && g == 0 && (a == 8 || a == 56)) {   // shader clock (s_memtime) against the 100 MHz reference: the clock this kernel runs at
            marl_lab_clock45t[2048 * 8 * 8 - 4 + (a == 8 ? 0 : 2)] = __builtin_amdgcn_s_memtime();
            marl_lab_clock45t[2048 * 8 * 8 - 4 + (a == 8 ? 1 : 3)] = __builtin_amdgcn_s_memrealtime();
        }
#endif
        double y[NF], k1[NF];
        // (a thread's cell of tile t: local index l = out_lo + t V - H + tid; lanes outside the buffer - beyond a physical boundary, where the
        // ghost-cell rules apply and nothing reads them - load a copy of the edge cell: no predicate, no branch, finite values)
#define MARL_LOAD_TILE(t, tid_)                                                                                                        \
        do {                                                                                                                           \
            int64_t l_ = S.out_lo + (int64_t)(t) * V - H + (tid_);                                                                     \
            l_ = l_ < 0 ? 0 : (l_ < S.n_buf ? l_ : S.n_buf - 1);                                                                       \
            _Pragma("unroll") for (int f = 0; f < NF; f++)                                                                             \
                y[f] = MARL_STREAM_LOAD(yin + at<LAYOUT>(f, l_, S.ld));                                                                \
            _Pragma("unroll") for (int f = 0; f < NF; f++)                                                                             \
                k1[f] = MARL_STREAM_LOAD(fin + at<LAYOUT>(f, l_, S.ld));                                                               \
        } while (0)
        {
            int tid0 = threadIdx.x;
            asm volatile("" : "+v"(tid0));
            MARL_LOAD_TILE(g, tid0);
        }
        if ((threadIdx.x & 31) == 0) {   // thread 32 j owns s_acc[j]
            const int j = threadIdx.x >> 5;
            s_acc[j] = (j == 0) ? 0.0 : __builtin_inf();
        }
        const unsigned grab0 = grab_base + a * (R + G);
        for (unsigned ti = 0;; ti++) {
            unsigned tile = g + ti * G, extra = 0;
            MARL_STAMP45T(0);
            int tid = threadIdx.x;
            asm volatile("" : "+v"(tid));   // opaque: what derives from the thread index is recomputed per tile, not carried across the loop
            if (ti >= n_full) {             // the remainder round: first come, first served
                if (R == 0) break;
                if (threadIdx.x == 0) s_next = __hip_atomic_fetch_add(&sync->grab, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - grab0;
                __syncthreads();            // (also: every wave has finished the reduction of the previous tile)
                extra = (unsigned)to_sgpr((int32_t)s_next);
                if (extra >= R) break;
                tile = n_full * G + extra;
                MARL_LOAD_TILE(tile, tid);  // (no prefetch here: whoever works on the remainder has time)
            } else {
                // every wave has finished the reduction of the previous tile (whose columns this tile's park / cache / edge writes
                // reuse) - or, first tile, has read the decision out of s_pub; the loads issued before it are in flight meanwhile
                __syncthreads();
            }
            sb.rebind(tid);
            double* pk = lds + SB::LDS_DOUBLES + tid;
            double yn[NF], k7[NF], esum[NF];
            PointAux aux;
            {
                const int64_t l = S.out_lo + (int64_t)tile * V - H + tid;
                sb.set_window(l + S.goff);
            }
            sb.reuse_live = false;
#pragma unroll
            for (int f = 0; f < PARK; f++) pk[f * BLK] = y[f];
            MARL_STAMP45T(1);
            dp45_attempt<BLK, false, SB, PARK>(sb, h, y, k1, yn, k7, esum, aux, DenseWeights{}, pk);
            MARL_STAMP45T(2);
            // everything below is recomputed from the thread index again (nothing but the results is carried across the stages)
            int tid2 = threadIdx.x;
            asm volatile("" : "+v"(tid2));
            const int64_t l2 = S.out_lo + (int64_t)tile * V - H + tid2;
            const bool owned = tid2 >= H && tid2 < BLK - H && l2 >= S.out_lo && l2 < S.out_hi;
            double q[NQ];
            monitors_init(q);
            if (owned) {
                const double* pk2 = lds + SB::LDS_DOUBLES + tid2;
#pragma unroll
                for (int f = 0; f < NF; f++) q[0] += dp45_err2(esum[f], h, f < PARK ? pk2[f * BLK] : y[f], yn[f], rtol, atol);
                monitors_accumulate<true>(q, yn, aux.U, aux.W);
            }
            // the next tile's loads first, the stores behind them: vector memory operations return in order, so waiting for
            // those loads does not wait for the stores' acknowledgements (write-through to memory: ~2 us)
            // (unconditional - after the last tile it re-reads that tile: a conditional prefetch makes y, k1 of THIS tile the other
            // operand of the loop's phi, i.e. twenty more registers live across the six evaluations)
            MARL_LOAD_TILE(ti + 1 < n_full ? tile + G : tile, tid2);
            if (owned) {
#pragma unroll
                for (int f = 0; f < NF; f++) {
                    MARL_STREAM_STORE(yout + at<LAYOUT>(f, l2, S.ld), yn[f]);
                    MARL_STREAM_STORE(fout + at<LAYOUT>(f, l2, S.ld), k7[f]);
                }
            }
            MARL_STAMP45T(3);
            const double r = tile_reduce_halfwaves<BLK, SB>(q, lds, tid2);   // (one barrier inside)
            if ((tid2 & 31) == 0) {
                const int j = tid2 >> 5;
                if (j > 0) s_acc[j] = __builtin_fmin(s_acc[j], r);
                else if (ti < n_full) s_acc[0] += r;
                else __hip_atomic_store(gsum + G + extra, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            MARL_STAMP45T(4);
        }
#undef MARL_LOAD_TILE
        // ---- the barrier of the attempt ----
        MARL_STAMP45(1);
        if ((threadIdx.x & 31) == 0) {   // the sum into this workgroup's slot; the extrema by fp64 atomic minimum (exact whatever the order)
            const int j = threadIdx.x >> 5;
            if (j == 0) __hip_atomic_store(gsum + g, s_acc[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else __hip_atomic_fetch_min(gmon + (((epoch_base + a) & 1u) * (NQ - 1) + (j - 1)) * MON_STRIDE, s_acc[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
        __builtin_amdgcn_s_waitcnt(0);   // this thread's stores (state, record) have been acknowledged
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
        __syncthreads();                 // ... and everybody else's
        if (threadIdx.x == 0) {
            const unsigned old = __hip_atomic_fetch_add(&sync->arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_last = (old + 1u - arrive_base) == G * (a + 1u);
            s_abort = 0;
        }
        MARL_STAMP45(2);
        __syncthreads();
        const unsigned epoch = epoch_base + a + 1u;
        if (s_last) {   // (the whole workgroup) every workgroup's record of this attempt is in memory
            MARL_STAMP45L(0);
            // one round trip: the controller (one word per thread), the grid's extrema (threads 64..70), the workgroups' sums
            // (thread t: groups t, t + BLK, ... - four per pass, issued together)
            double* const mon = gmon + ((epoch_base + a) & 1u) * (NQ - 1) * MON_STRIDE;
            if ((int)threadIdx.x < CTRL_WORDS)
                reinterpret_cast<unsigned long long*>(&sc)[threadIdx.x] =
                    __hip_atomic_load(reinterpret_cast<unsigned long long*>(ctrl) + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (threadIdx.x >= 64 && threadIdx.x < 64 + NQ - 1) {
                const int j = threadIdx.x - 64 + 1;
                const double v = __hip_atomic_load(mon + (j - 1) * MON_STRIDE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                s_rec[j] = (j > NQMIN) ? -v : v;
            }
            double e2 = 0.0;
            const unsigned GS = G + R;
            for (unsigned base = 0; base < GS; base += 4 * BLK) {
                double v[4];
                const unsigned r0 = base + threadIdx.x, last = GS - 1;
                const double* p0 = gsum + (r0 < GS ? r0 : last);
                const double* p1 = gsum + (r0 + BLK < GS ? r0 + BLK : last);
                const double* p2 = gsum + (r0 + 2 * BLK < GS ? r0 + 2 * BLK : last);
                const double* p3 = gsum + (r0 + 3 * BLK < GS ? r0 + 3 * BLK : last);
                asm volatile("global_load_dwordx2 %0, %4, off sc1\n\tglobal_load_dwordx2 %1, %5, off sc1\n\tglobal_load_dwordx2 %2, %6, off sc1\n\t"
                             "global_load_dwordx2 %3, %7, off sc1\n\ts_waitcnt vmcnt(0)"
                             : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]) : "v"(p0), "v"(p1), "v"(p2), "v"(p3) : "memory");
                e2 += (r0 < GS) ? v[0] : 0.0;
                e2 += (r0 + BLK < GS) ? v[1] : 0.0;
                e2 += (r0 + 2 * BLK < GS) ? v[2] : 0.0;
                e2 += (r0 + 3 * BLK < GS) ? v[3] : 0.0;
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) e2 += __shfl_xor(e2, off, 64);
            if ((threadIdx.x & 63) == 0) s_wsum[threadIdx.x >> 6] = e2;
            MARL_STAMP45L(1);
            __syncthreads();
            if constexpr (DD) {   // domain decomposition: the slab's record and strips into the rank's message; nothing is decided here
                if (threadIdx.x == 0) {
                    double sumsq = 0.0;
#pragma unroll
                    for (int w = 0; w < NW; w++) sumsq += s_wsum[w];
                    send[0] = sumsq;
                    __hip_atomic_store(&sync->arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // re-armed for the next launch
                    __hip_atomic_store(&sync->grab, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                if (threadIdx.x >= 64 && threadIdx.x < 64 + NQ - 1) {
                    send[threadIdx.x - 64 + 1] = s_rec[threadIdx.x - 64 + 1];
                    __hip_atomic_store(mon + (threadIdx.x - 64) * MON_STRIDE, __builtin_inf(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                const int n = 2 * NF * halo;
                for (int i = threadIdx.x; i < n; i += BLK) {
                    const int aa = i / (NF * halo), f = (i / halo) % NF, j = i % halo;
                    const double* src = aa ? fout : yout;
                    send[NQ + i] = __hip_atomic_load(src + at<LAYOUT>(f, S.out_lo + j, S.ld), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    send[NQ + n + i] = __hip_atomic_load(src + at<LAYOUT>(f, S.out_hi - halo + j, S.ld), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                break;
            }
            if (threadIdx.x == 0) {
                double sumsq = 0.0;
#pragma unroll
                for (int w = 0; w < NW; w++) sumsq += s_wsum[w];
                const bool accepted = rk45_decide(sc, sumsq, &sb.T);
                if (!pause_on_event) {   // the status does not depend on this step's events: publish now, bookkeeping afterwards
                    if (accepted) rk45_advance_status_no_events(sc); else if (sc.status == ST_RUNNING) rk45_prepare_attempt(sc);
                } else {
                    s_rec[0] = 0.0;
                    const int fired = accepted ? rk45_events(sc, s_rec) : 0;
                    rk45_advance_status(sc, accepted, fired);
                }
                const unsigned long long hb = (unsigned long long)__double_as_longlong(sc.h_try);
                s_pub[0] = hb;
                s_pub[1] = pub_word(hb, epoch, sc.status, sc.cur);
                s_last = accepted ? 2 : 1;
            }
            MARL_STAMP45L(2);
            __syncthreads();
            if ((int)threadIdx.x < PUB_COPIES) {   // one 16-byte store per copy
                unsigned long long* p = sync->pub + threadIdx.x * PUB_STRIDE;
                const unsigned long long w0 = s_pub[0], w1 = s_pub[1];
                asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(__uint128_t(w0) | (__uint128_t(w1) << 64)) : "memory");
            }
            MARL_STAMP45L(3);
            // off the critical path: the driver's event bookkeeping of an accepted step (lanes 0..6: one monitor each), the extrema
            // re-armed for the attempt after next, the controller back to memory.  The next reader of either is the last workgroup
            // of a LATER barrier, which this workgroup joins only after these stores have been acknowledged; the host reads the
            // controller after the kernel.
            if (!pause_on_event && s_last == 2 && threadIdx.x < 7) rk45_event_one(sc, threadIdx.x, rk45_monitor_of_record(s_rec, threadIdx.x));
            if (threadIdx.x >= 64 && threadIdx.x < 64 + NQ - 1)
                __hip_atomic_store(mon + (threadIdx.x - 64) * MON_STRIDE, __builtin_inf(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();
            if ((int)threadIdx.x < CTRL_WORDS)
                __hip_atomic_store(reinterpret_cast<unsigned long long*>(ctrl) + threadIdx.x, reinterpret_cast<unsigned long long*>(&sc)[threadIdx.x],
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            MARL_STAMP45L(4);
        }
        if constexpr (DD) break;   // (one attempt per launch: nothing to wait for)
        if (threadIdx.x == 0) {
            unsigned spins = 0;
            while (true) {
                __uint128_t v;
                asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(my_pub) : "memory");
                const unsigned long long w0 = (unsigned long long)v, w1 = (unsigned long long)(v >> 64);
                if ((unsigned)(w1 >> 8) == epoch && w1 == pub_word(w0, epoch, (int)((w1 >> 1) & 7) - 1, (int)(w1 & 1))) {
                    s_pub[0] = w0;
                    s_pub[1] = w1;
                    break;
                }
                __builtin_amdgcn_s_sleep(8);
                if (++spins > STREAM_SPIN_LIMIT || ((spins & 63u) == 0 && __hip_atomic_load(&sync->sticky, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
                    __hip_atomic_store(&sync->sticky, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    s_abort = 1;
                    break;
                }
            }
        }
        __syncthreads();
        MARL_STAMP45(3);
        if (s_abort) break;
        // (LDS reads are not known to be uniform: without readfirstlane h, cur and the four buffer pointers live in vector registers)
        h = to_sgpr(__longlong_as_double((long long)s_pub[0]));
        const int32_t flags = to_sgpr((int32_t)(s_pub[1] & 0xff));
        status = ((flags >> 1) & 7) - 1;
        cur = flags & 1;
        // (the barrier in front of the next attempt's first tile - or the end of the kernel - separates these reads from thread 0's next writes)
    }
}

// U and W of a state (monitors zeros_U / zeros_W, LHeureux_model.py:567-593)
__device__ __forceinline__ void uw_point(double Phi, const DevConsts& C, const Tables& T, double& U, double& W)
{
    const double F = 1.0 - fast_exp(10.0 - 10.0 * rcp_nr(Phi), T);
    const double rF = C.hot.rhorat * F;
    U = C.hot.presum + rF * (Phi * Phi * Phi) * rcp_nr(1.0 - Phi);
    W = C.hot.presum - rF * Phi * Phi;
}

// Dense output of the step that starts at (yold, fold) with size h: replays the step's stages and
// writes  y(t_old + x h) = y_old + h sum_j w_j(x) K_j  (t_eval samples, ivp.py:706-723) and/or the
// monitors record of that state (event root finding, ivp.py:51-76).  yout may be NULL.
template <int BLK, int LAYOUT, bool VD = false>
__global__ void __launch_bounds__(BLK) rk45_dense_kernel(const double* __restrict__ yold, const double* __restrict__ fold,
                                                         const DevConsts* __restrict__ consts, Slab S, double h,
                                                         DenseWeights dw, double* __restrict__ yout, double* __restrict__ part)
{
    constexpr int H = 6;
    constexpr int V = BLK - 2 * H;
    using SB = StencilBlock<BLK, true, VD>;
    __shared__ double lds[SB::LDS_DOUBLES];
    const DevConsts& C = consts[0];
    const int64_t w0 = S.out_lo + (int64_t)blockIdx.x * V - H;
    const int64_t l = w0 + (int64_t)threadIdx.x;
    SB sb(lds, l + S.goff, consts);
    double y[NF], k1[NF], yn[NF], k7[NF], dsum[NF];
    PointAux aux;
    load_cells<LAYOUT>(yold, l, S, C, y);
    MARL_ONCE {
        const bool in = l >= 0 && l < S.n_buf;
#pragma unroll
        for (int f = 0; f < NF; f++) k1[f] = in ? fold[at<LAYOUT>(f, l, S.ld)] : 0.0;
    }
    dp45_attempt<BLK, true, SB>(sb, h, y, k1, yn, k7, dsum, aux, dw);
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
    block_reduce<BLK, NQ, NQMIN>(q, lds);   // the edge-exchange buffers are free now
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < NQ; j++) part[(int64_t)blockIdx.x * NQ + j] = q[j];
    }
}

// ---------------------------------------------------------------------------------------------
// Domain decomposition (BASELINE config 5): a rank's slab buffer carries `halo` exchanged cells on each
// interior side.  pack: the slab's first / last `halo` OWNED cells of (y, f) -> contiguous strips
// [array(2)][field(5)][halo] for the neighbours; unpack: received strips -> the halo cells.
// `which`: 0 / 1 = explicit buffer; -1 = the buffer the attempt in flight wrote (cur ^ 1); -2 = cur.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int slab_which(int which, const Rk45Ctrl* ctrl)
{
    return which >= 0 ? which : (which == -1 ? (ctrl->cur ^ 1) : ctrl->cur);
}

__global__ void __launch_bounds__(128) slab_pack_kernel(const double* __restrict__ Y0, const double* __restrict__ Y1,
                                                        const double* __restrict__ F0, const double* __restrict__ F1,
                                                        const Rk45Ctrl* __restrict__ ctrl, int which, Slab S, int halo,
                                                        double* __restrict__ send_lo, double* __restrict__ send_hi)
{
    const int w = slab_which(which, ctrl);
    const double* Y = w ? Y1 : Y0;
    const double* F = w ? F1 : F0;
    const int n = 2 * NF * halo;
    for (int i = threadIdx.x; i < n; i += 128) {
        const int a = i / (NF * halo), f = (i / halo) % NF, j = i % halo;
        const double* src = a ? F : Y;
        if (send_lo) send_lo[i] = src[at<LAYOUT_FIELD_MAJOR>(f, S.out_lo + j, S.ld)];
        if (send_hi) send_hi[i] = src[at<LAYOUT_FIELD_MAJOR>(f, S.out_hi - halo + j, S.ld)];
    }
}

__global__ void __launch_bounds__(128) slab_unpack_kernel(double* __restrict__ Y0, double* __restrict__ Y1,
                                                          double* __restrict__ F0, double* __restrict__ F1,
                                                          const Rk45Ctrl* __restrict__ ctrl, int which, Slab S, int halo,
                                                          const double* __restrict__ recv_lo, const double* __restrict__ recv_hi)
{
    const int w = slab_which(which, ctrl);
    double* Y = w ? Y1 : Y0;
    double* F = w ? F1 : F0;
    const int n = 2 * NF * halo;
    for (int i = threadIdx.x; i < n; i += 128) {
        const int a = i / (NF * halo), f = (i / halo) % NF, j = i % halo;
        double* dst = a ? F : Y;
        if (recv_lo) dst[at<LAYOUT_FIELD_MAJOR>(f, S.out_lo - halo + j, S.ld)] = recv_lo[i];
        if (recv_hi) dst[at<LAYOUT_FIELD_MAJOR>(f, S.out_hi + j, S.ld)] = recv_hi[i];
    }
}


// ---- the per-attempt pair of the domain-decomposed loop (marl_slab_run) --------------------------------------------------
// After the attempt kernel: combine the slab's per-block records into ONE record and pack the strips the neighbours need, into
// the rank's message  send = [record (8) | lower strip (2*5*halo) | upper strip].  nb = 0: keep send[0..8) (set by the caller).
__global__ void __launch_bounds__(256) slab_reduce_pack_kernel(const double* __restrict__ Y0, const double* __restrict__ Y1,
                                                               const double* __restrict__ F0, const double* __restrict__ F1,
                                                               const Rk45Ctrl* __restrict__ ctrl, int which, Slab S, int halo,
                                                               const double* __restrict__ part, int64_t nb, double* __restrict__ send)
{
    __shared__ double scratch[NQ * 256];
    const int w = slab_which(which, ctrl);
    const double* Y = w ? Y1 : Y0;
    const double* F = w ? F1 : F0;
    const int n = 2 * NF * halo;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int a = i / (NF * halo), f = (i / halo) % NF, j = i % halo;
        const double* src = a ? F : Y;
        send[NQ + i] = src[at<LAYOUT_FIELD_MAJOR>(f, S.out_lo + j, S.ld)];
        send[NQ + n + i] = src[at<LAYOUT_FIELD_MAJOR>(f, S.out_hi - halo + j, S.ld)];
    }
    if (nb <= 0) return;
    double q[NQ];
    monitors_init(q);
    for (int64_t b = threadIdx.x; b < nb; b += 256) {
#pragma unroll
        for (int j = 0; j < NQ; j++) {
            const double o = part[b * NQ + j];
            q[j] = (j == 0) ? q[j] + o : (j <= NQMIN ? nanmin(q[j], o) : nanmax(q[j], o));
        }
    }
    block_reduce<256, NQ, NQMIN>(q, scratch);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < NQ; j++) send[j] = q[j];
    }
}

// After the all-gather: copy the neighbours' strips out of the gathered messages into this slab's halo cells, then (do_control)
// combine the ranks' records IN RANK ORDER and finish the attempt - every rank computes the same decision from the same numbers.
__global__ void __launch_bounds__(256) slab_unpack_control_kernel(double* __restrict__ Y0, double* __restrict__ Y1, double* __restrict__ F0,
                                                                  double* __restrict__ F1, Rk45Ctrl* __restrict__ ctrl, int which, Slab S, int halo,
                                                                  const double* __restrict__ gathered, int rank, int world, int msg, int do_control)
{
    if (do_control && ctrl->status != ST_RUNNING) return;
    const int w = slab_which(which, ctrl);      // read before thread 0 may flip ctrl->cur below
    double* Y = w ? Y1 : Y0;
    double* F = w ? F1 : F0;
    const int n = 2 * NF * halo;
    const double* lo = (rank > 0 && S.out_lo > 0) ? gathered + (int64_t)(rank - 1) * msg + NQ + n : nullptr;          // lower neighbour's UPPER strip
    const double* hi = (rank < world - 1 && S.out_hi < S.n_buf) ? gathered + (int64_t)(rank + 1) * msg + NQ : nullptr;  // upper neighbour's LOWER strip
    for (int i = threadIdx.x; i < n; i += 256) {
        const int a = i / (NF * halo), f = (i / halo) % NF, j = i % halo;
        double* dst = a ? F : Y;
        if (lo) dst[at<LAYOUT_FIELD_MAJOR>(f, S.out_lo - halo + j, S.ld)] = lo[i];
        if (hi) dst[at<LAYOUT_FIELD_MAJOR>(f, S.out_hi + j, S.ld)] = hi[i];
    }
    __syncthreads();
    if (do_control && threadIdx.x == 0) {
        double q[NQ];
        monitors_init(q);
        for (int r = 0; r < world; r++) {
            const double* o = gathered + (int64_t)r * msg;
#pragma unroll
            for (int j = 0; j < NQ; j++) q[j] = (j == 0) ? q[j] + o[j] : (j <= NQMIN ? nanmin(q[j], o[j]) : nanmax(q[j], o[j]));
        }
        Rk45Ctrl c = *ctrl;
        rk45_finish_attempt(c, q);
        *ctrl = c;
    }
}

// records of all ranks (stride msg) -> dense [world][8]
__global__ void slab_records_kernel(const double* __restrict__ gathered, int world, int msg, double* __restrict__ recs)
{
    for (int i = threadIdx.x; i < world * NQ; i += blockDim.x) recs[i] = gathered[(int64_t)(i / NQ) * msg + (i % NQ)];
}

// owned cells of a slab <-> a dense [5][n_own] array
__global__ void __launch_bounds__(256) slab_copy_kernel(double* __restrict__ Y0, double* __restrict__ Y1,
                                                        const Rk45Ctrl* __restrict__ ctrl, int which, Slab S,
                                                        double* __restrict__ dense, int to_dense)
{
    double* Y = slab_which(which, ctrl) ? Y1 : Y0;
    const int64_t n_own = S.out_hi - S.out_lo;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_own) return;
#pragma unroll
    for (int f = 0; f < NF; f++) {
        if (to_dense) dense[f * n_own + i] = Y[at<LAYOUT_FIELD_MAJOR>(f, S.out_lo + i, S.ld)];
        else Y[at<LAYOUT_FIELD_MAJOR>(f, S.out_lo + i, S.ld)] = dense[f * n_own + i];
    }
}

// ---------------------------------------------------------------------------------------------
// Batched parameter sweep (BASELINE configs 3-4): ONE workgroup integrates ONE instance
// (N <= BLK cells) for all its steps.  State, stage vectors and the step controller stay
// on-chip for the whole integration; global memory is touched at entry and exit only.
//   Y: [batch][5][N] field-major per instance (the reference's layout, one instance after another).
// ---------------------------------------------------------------------------------------------
// (1024-thread workgroups cap a thread at 128 VGPRs, which this kernel overruns: 38 spilled VGPRs.  Parking the step's first state in
// LDS, and a 6th-order reuse tier for coarse grids, were measured and dropped - profiles/r02_lab_sweep_experiments.log)
//
// Two loop shapes, one arithmetic (dp45_attempt, the error norm, the monitors, rk45_decide / rk45_events / rk45_advance_status):
//   FAST = false  the round-1/2 loop: 8-quantity block reduction (4 barriers), scipy's controller on ONE lane while 1023 wait,
//                 2 more barriers to publish it.  Kept for single small runs that pause on a monitor sign change (root finding:
//                 the decision to pause needs the events of THIS step).
//   FAST = true   (round 3; sweeps, and single runs without event pauses) the step controller off the critical path: each wave
//                 butterflies its own sum of squares, ONE barrier makes the 16 partial sums visible, and EVERY wave adds them in
//                 wave order and runs decide + advance_status itself - replicated scalar work, but no single-lane section and no
//                 publish barriers; the controller's scalars are pushed into SGPRs (readfirstlane) so the replication costs no
//                 vector registers.  The seven monitors go through LDS columns written before that one barrier; waves 0..6 reduce
//                 one quantity each after it, and lanes 0..6 of wave 0 do the event bookkeeping (rk45_event_one) one barrier
//                 later - after the first evaluation of the NEXT attempt, whose exchange barrier orders it - or after the loop.
//                 Per attempt: 7 barriers instead of 12 (profiles/r03_lab_sweep.log).
// the fields of the step controller that rk45_decide / rk45_advance_status / rk45_prepare_attempt read or write
__device__ __forceinline__ void ctrl_to_sgpr(Rk45Ctrl& c)
{
    c.t = to_sgpr(c.t); c.h_abs = to_sgpr(c.h_abs); c.t_bound = to_sgpr(c.t_bound); c.h_try = to_sgpr(c.h_try); c.t_new = to_sgpr(c.t_new);
    c.t_old = to_sgpr(c.t_old); c.h_prev = to_sgpr(c.h_prev); c.pause_t = to_sgpr(c.pause_t);
    c.nfev = to_sgpr(c.nfev); c.n_acc = to_sgpr(c.n_acc); c.n_rej = to_sgpr(c.n_rej); c.attempts = to_sgpr(c.attempts);
    c.max_attempts = to_sgpr(c.max_attempts); c.n_total = to_sgpr(c.n_total);
    c.status = to_sgpr(c.status); c.cur = to_sgpr(c.cur); c.rejected = to_sgpr(c.rejected); c.accepted_last = to_sgpr(c.accepted_last);
    c.pause_on_event = to_sgpr(c.pause_on_event);
}

#ifndef MARL_SWEEP_PARK
#define MARL_SWEEP_PARK 2
#endif
// the dense-output weights w_j(x) of a Dormand-Prince step, summed as the host's dense_eval sums them
__device__ __forceinline__ DenseWeights dense_weights(double x)
{
    const double pw[4] = {x, x * x, x * x * x, x * x * x * x};
    DenseWeights dw;
#pragma unroll
    for (int j = 0; j < 7; j++) {
        double a = 0;
#pragma unroll
        for (int m = 0; m < 4; m++) a += dp::P[j][m] * pw[m];
        dw.w[j] = a;
    }
    return dw;
}

// What rk45_sweep_body asks of a method M other than Dormand-Prince (Bs23Method, marl_rk23.h): N_WEIGHTS, the slots of DenseWeights
// its dense output fills, and static members attempt<BLK, SB, PARK, EITHER> (the arguments of dp45_attempt), finish_attempt,
// decide_lean, prepare_attempt_lean and weights, the counterparts of dp45_attempt, rk45_finish_attempt, rk45_decide_lean, rk45_prepare_attempt_lean and dense_weights.  For Dp45Method
// itself the body calls those functions BY NAME, as it did before it had this parameter: through forwarding members the RK45 kernels
// came out with the same instructions in another order (the ghost-cell arithmetic of the boundary branch moved), and they are pinned.
struct Dp45Method { static constexpr int N_WEIGHTS = 7; };

// EVAL (FAST only; rk45_sweep_eval_kernel): the t_eval samples that fall into an accepted step are written by dense-output replays of
// that step inside the loop (see there); without it the four trailing arguments are unused and the code is what it was without them.
// ROOTS (FAST and EVAL only; rk45_sweep_roots_kernel): the root times of the monitors that change sign in an accepted step are located
// by Brent's method on dense-output replays of that step, before its samples and its commit (see there); two more arguments.
// TERM (ROOTS only; rk45_sweep_term_kernel): terminal monitors (marl_set_terminal) - a step in which an active monitor meets its limit
// `lim` ends the instance at that monitor's root (see there; the rule: marl_rk_terminal.h); every other step is a ROOTS step.
struct TermLimits { int64_t k[7]; };   // marl_set_terminal's limits, a kernel argument by value
template <int BLK, bool VD, bool FAST, bool EVAL = false, bool ROOTS = false, class M = Dp45Method, bool TERM = false>
__device__ __forceinline__ void rk45_sweep_body(double* __restrict__ Y, const DevConsts* __restrict__ consts, Rk45Ctrl* __restrict__ ctrls, int64_t N,
                                                double* __restrict__ Yold, double* __restrict__ Fold,
                                                const double* __restrict__ t_eval = nullptr, int64_t n_eval = 0,
                                                double* __restrict__ Yeval = nullptr, int64_t* __restrict__ n_done = nullptr,
                                                double* __restrict__ t_events = nullptr, int64_t max_events = 0, TermLimits lim = {})
{
    constexpr bool DP = std::is_same_v<M, Dp45Method>;
    static_assert(ROOTS || !TERM, "the stop is found by the root search");
    static_assert(FAST || !EVAL, "the sampling loop is built on the replicated controller");
    static_assert((FAST && EVAL) || !ROOTS, "a Brent function evaluation is a dense-output replay");
    using SB = StencilBlock<BLK, false, VD>;
    constexpr int NW = BLK / 64;
    constexpr int NMON = NQ - 1;                                  // the seven monitor extrema (record slots 1..7)
    constexpr int FAST_DOUBLES = FAST ? NMON * BLK + NW + NQ : 0; // monitor columns [slot][thread], per-wave sums, the reduced record
    // PARK fields of the step's first state y live in the thread's LDS column instead of registers (dp45_attempt): the 1024-thread
    // shape is capped at 128 VGPRs and every scratch reload in the stage loop stalls all 16 waves in front of their barrier
    // (measured: 6.6 -> 21.7 reloads per attempt = -17 %); two columns are what the 160 KB of LDS still hold beside the monitor columns
    constexpr int PARK = (FAST && BLK == 1024) ? MARL_SWEEP_PARK : 0;
    __shared__ double lds[SB::LDS_DOUBLES + FAST_DOUBLES + PARK * BLK];
    __shared__ Rk45Ctrl sc;
    const DevConsts& C = consts[blockIdx.x];
    double* yg = Y + (int64_t)blockIdx.x * NF * N;
    Slab S = {N, 0, N, 0, N};
    const int64_t l0 = threadIdx.x;
    SB sb(lds, l0, consts + blockIdx.x);
    if (threadIdx.x == 0) sc = ctrls[blockIdx.x];
    __syncthreads();
    if (sc.status != ST_RUNNING) return;
    const double rtol = FAST ? to_sgpr(sc.rtol) : sc.rtol, atol = FAST ? to_sgpr(sc.atol) : sc.atol;

    double y[NF], k1[NF], yn[NF], k7[NF], esum[NF];
    PointAux aux;
    load_cells<LAYOUT_FIELD_MAJOR>(yg, l0, S, C, y);
    sb.eval(y, k1, aux);  // f(t, y): RungeKutta.__init__ (first launch) or re-derived on resume
    double* pk = lds + SB::LDS_DOUBLES + FAST_DOUBLES + threadIdx.x;
#pragma unroll
    for (int f = 0; f < PARK; f++) pk[f * BLK] = y[f];
#define MARL_Y(f) ((f) < PARK ? pk[(f) * BLK] : y[f])
#define MARL_KEEP_OLD_STEP()                                                                                           \
    MARL_ONCE if (l0 < N) {                                                                                            \
        _Pragma("unroll") for (int f = 0; f < NF; f++) {                                                               \
            Yold[(int64_t)blockIdx.x * NF * N + at<LAYOUT_FIELD_MAJOR>(f, l0, N)] = MARL_Y(f);                         \
            Fold[(int64_t)blockIdx.x * NF * N + at<LAYOUT_FIELD_MAJOR>(f, l0, N)] = k1[f];                             \
        }                                                                                                              \
    }

    if constexpr (!FAST) {
        while (true) {
            const double h = sc.h_try;
            if constexpr (DP) dp45_attempt<BLK, false, SB>(sb, h, y, k1, yn, k7, esum, aux);
            else M::template attempt<BLK, SB, 0, false>(sb, h, y, k1, yn, k7, esum, aux, DenseWeights{}, nullptr, false);
            double q[NQ];
            monitors_init(q);
            MARL_ONCE if (l0 < N) {
#pragma unroll
                for (int f = 0; f < NF; f++) q[0] += dp45_err2(esum[f], h, MARL_Y(f), yn[f], rtol, atol);
                monitors_accumulate(q, yn, aux.U, aux.W);
            }
            block_reduce<BLK, NQ, NQMIN>(q, lds);   // the edge-exchange buffers are free now
            if (threadIdx.x == 0) {
                if constexpr (DP) rk45_finish_attempt(sc, q, &sb.T); else M::finish_attempt(sc, q, &sb.T);
            }
            __syncthreads();
            const int status = sc.status;
            if (sc.accepted_last) {
                if (status != ST_RUNNING && Yold) {
                    // keep (y_old, f_old) of the step just accepted: the host replays it for dense output
                    MARL_KEEP_OLD_STEP()
                }
#pragma unroll
                for (int f = 0; f < NF; f++) {
                    y[f] = yn[f];
                    k1[f] = k7[f];
                }
            }
            __syncthreads();  // everyone has read sc before thread 0 may touch it again
            if (status != ST_RUNNING) break;
        }
    } else {
        double* mon = lds + SB::LDS_DOUBLES;         // [slot 1..7][thread]: never touched by the evaluations' edge exchange
        double* wsum = mon + NMON * BLK;             // [wave]
        double* rec = wsum + NW;                     // [NQ]: the reduced monitors of the last accepted step (slots 1..7)
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        // the controller, replicated: every lane holds the same values; what lives across an attempt sits in SGPRs
        // (tried: the controller in a double-buffered LDS block re-read after the barrier - fewer SGPRs, but the register
        // allocator then spilled more vector registers: 21.7 instead of 6.6 - 15.7 scratch reloads per attempt, -17 %)
        Rk45Ctrl c = sc;
        ctrl_to_sgpr(c);
        const double inv_n = to_sgpr(1.0 / (double)c.n_total);
        bool events_pending = false;                 // an accepted step whose monitors (rec) have not been compared with sc.g yet
        // EVAL: t_eval samples inside an accepted step, (t_old, t] (ivp.py:706-723), are written BEFORE the step is committed, while
        // (y, k1) still describe it: the loop runs once more per sample with `sampling` set - the SAME dp45_attempt call (EITHER), with h = h_prev
        // and the dense-output weights w_j(x) in place of the error weights E_j, so that `esum` returns  sum_j w_j K_j  and
        // y + h esum  is the sample (rk.py:560-574).  One call site for attempts and replays is what keeps the ordinary path at the plain
        // kernel's register pressure (a second inlined copy of the six evaluations: 184 -> 540 B of scratch at 1024 threads, spill
        // stores inside the stage sequence; profiles/r07_sweep_frames_isa.log), and it answers where y_new / k7 wait during a replay:
        // nowhere.  The replay executes the instructions of the accepted attempt on the same (y, k1, h), so it leaves the same y_new,
        // k7 (and aux) in the same registers, bit for bit, and the commit that follows the last replay finds them there.
        //   - uniformity: whether to replay follows from c (replicated, SGPRs), ie, and t_eval[ie], which every wave reads from the same
        //     address - the exchange barriers of a replay are reached by every wave or by none;
        //   - a replay is no attempt: it skips the error norm, the ONE barrier, the decision and the monitors, and touches neither c
        //     (nfev included: scipy's dense output costs no evaluation) nor sc, rec or the monitor columns (the evaluations write the
        //     edge buffers and read the park columns only);
        //   - event bookkeeping: the ordering argument at the head of the loop asks that rec / sc.t_old / sc.h_prev / sc.t of an accepted
        //     step are read after one more workgroup barrier and before the next DECISION replaces them.  Replays sit between that decision
        //     and the next attempt, add barriers and decide nothing; events_pending stays set through them, so the bookkeeping still
        //     follows the evaluations of the next attempt - or the loop, when the step was the last.
        //   TERM: in an accepted step in which a monitor that changed sign meets its limit (rk_terminal_any_met: replicated scalars,
        //   from rec, sc.g, sc.n_events and the kernel argument) ALL monitors that changed sign are located, with or without a slot, the
        //   roots stay in replicated scalars (term_root) and nothing is written to sc until the last of them is known; then every wave
        //   applies rk_terminal_step to the same numbers, one barrier lets every wave finish reading sc.n_events, and thread 0 does the
        //   bookkeeping of the kept monitors and stores their roots where a slot is free.  The samples up to t_stop follow (next_sample),
        //   then ONE more replay with the weights of t_stop: the frame expression becomes the state (parked fields through pk[]), its
        //   monitors go through the monitor columns into rec and sc.g, c.t = t_stop, ST_TERMINAL, and the loop ends.  term_step,
        //   stopping, t_stop and the kept mask are replicated scalars like br_phase, so every barrier of these trips is reached by every
        //   wave or by none; a step that meets no limit takes none of these branches and is a ROOTS step instruction for instruction.
        bool term_step = false, stopping = false;    // TERM: the step just accepted ends the run; this trip replays it at t_stop
        int term_act = 0;                            // the monitors that changed sign in that step (bit e)
        double t_stop = 0.0, term_root[7] = {};      // where the run ends; the roots of that step's monitors
        int64_t ie = 0;                              // the next sample, t_eval[ie]; the same in every lane (SGPRs)
        bool sampling = false;                       // this trip of the loop replays the step just accepted for sample ie
        double te = 0.0;                             // t_eval[ie] of that replay
        DenseWeights dw = {};                        // w_j(x) of that replay (SGPRs)
        auto weights_of = [&](double x) -> DenseWeights {
            if constexpr (DP) return dense_weights(x); else return M::weights(x);
        };
        auto next_sample = [&]() -> bool {           // is sample ie inside the step just accepted?  then dw = its weights
            if (!(ie < n_eval)) return false;
            te = to_sgpr(t_eval[ie]);
            if constexpr (TERM) {
                if (!(te <= (term_step ? t_stop : c.t))) return false;   // a step that ends the run: the samples up to t_stop
            } else {
                if (!(te <= c.t)) return false;
            }
            const DenseWeights w = weights_of((te - c.t_old) / c.h_prev);
#pragma unroll
            for (int j = 0; j < M::N_WEIGHTS; j++) dw.w[j] = to_sgpr(w.w[j]);
            return true;
        };
        auto event_bookkeeping = [&]() {             // lanes 0..6 of wave 0: one monitor each; sc.t_old / sc.h_prev / sc.t describe that step
            if (threadIdx.x < 7) rk45_event_one(sc, threadIdx.x, rk45_monitor_of_record(rec, threadIdx.x));
        };
        // ROOTS: the roots of the monitors that changed sign in an accepted step (ivp.py:673-694, solve_event_equation :51-76) are
        // located before its samples and its commit, by the same replays: one Brent function evaluation is one PROBE trip of the loop -
        // the dp45_attempt call with h = h_prev and the weights of the abscissa, the monitors of  y + h esum  through the monitor columns,
        // and one pass of the Brent state machine, replicated in every wave like the controller (its state in SGPRs).
        //   - the sign test cannot wait for the next attempt: one barrier after the reduction into rec, then every wave forms the same mask
        //     of monitors to locate from rec, sc.g and sc.n_events.  No monitor to locate (nearly every step): the bookkeeping stays
        //     deferred as above - it writes sc.g, and the next attempt's barriers separate it from these reads.  Otherwise a second
        //     barrier, the bookkeeping at once (g <- g_new for all seven, counts, ev_first / ev_last), and the probes: they overwrite the
        //     monitor columns, which every wave has finished with, and leave rec alone;
        //   - a probe decides no step: c (nfev included), sc, rec, y_new / k7, ie are untouched, and whether a trip is a probe follows
        //     from replicated scalars only, so its barriers are reached by every wave or by none;
        //   - order within a step: roots (monitors ascending), then samples, then the commit and, for the last step, the way out.
        int ev_mask = 0;                             // monitors of the step just accepted still to be located (bit e)
        int br_e = 0, br_phase = 0, br_iter = 0;     // the monitor being located; 0 no probe, 1 f(a) asked, 2 f(b) asked, 3 iterating
        double br_fa = 0.0, br_t = 0.0;              // f(a); the time of the probe in flight
        BrentState bs = {};
        auto probe_at = [&](double tp) {             // the next trip evaluates the monitors at time tp of the step just accepted
            br_t = to_sgpr(tp);
            const DenseWeights w = weights_of((br_t - c.t_old) / c.h_prev);
#pragma unroll
            for (int j = 0; j < M::N_WEIGHTS; j++) dw.w[j] = to_sgpr(w.w[j]);
        };
        auto first_probe = [&]() {                   // Brent on the lowest monitor of ev_mask over [t_old, t]: f(a) first
            br_e = to_sgpr((int32_t)__builtin_ctz((unsigned)ev_mask));
            br_phase = 1;
            br_iter = 0;
            probe_at(c.t_old);
        };
        while (true) {
            bool replay = sampling;                  // workgroup-uniform: this trip is no attempt
            if constexpr (ROOTS) replay = sampling || br_phase != 0;
            if constexpr (TERM) replay = replay || stopping;
            const double h = (EVAL && replay) ? c.h_prev : c.h_try;
            // (the first evaluation's exchange barrier also orders the monitor reduction of the previous attempt before the
            // event bookkeeping below; dp45_attempt is opaque, so the bookkeeping follows the whole attempt's evaluations -
            // still before this attempt's own decision changes c.t_old / c.h_prev / c.t)
            if constexpr (DP) {
                if constexpr (EVAL) dp45_attempt<BLK, false, SB, PARK, true>(sb, h, y, k1, yn, k7, esum, aux, dw, pk, replay);
                else dp45_attempt<BLK, false, SB, PARK>(sb, h, y, k1, yn, k7, esum, aux, DenseWeights{}, pk);
            } else {
                if constexpr (EVAL) M::template attempt<BLK, SB, PARK, true>(sb, h, y, k1, yn, k7, esum, aux, dw, pk, replay);
                else M::template attempt<BLK, SB, PARK, false>(sb, h, y, k1, yn, k7, esum, aux, DenseWeights{}, pk, false);
            }
            if constexpr (TERM) {
                if (stopping) {                      // workgroup-uniform: the state at t_stop, its monitors, and the way out
                    double q[NQ];
                    monitors_init(q);
                    MARL_ONCE if (l0 < N) {
                        double d[NF];
#pragma unroll
                        for (int f = 0; f < NF; f++) d[f] = (t_stop == c.t_old) ? MARL_Y(f) : h * esum[f] + MARL_Y(f);   // (as the frames)
                        double U, W;
                        uw_point(d[4], C, sb.T, U, W);
                        monitors_accumulate<true>(q, d, U, W);
#pragma unroll
                        for (int f = 0; f < NF; f++) {
                            if (f < PARK) pk[f * BLK] = d[f]; else y[f] = d[f];
                        }
                    }
#pragma unroll
                    for (int j = 1; j < NQ; j++) mon[(j - 1) * BLK + threadIdx.x] = q[j];
                    __syncthreads();
#pragma unroll
                    for (int jj = 0; jj < (NMON + NW - 1) / NW; jj++) {   // the reduction of an accepted step's monitors, below
                        const int j = wave + jj * NW + 1;
                        if (j < NQ) {
                            const double sgn = (j <= NQMIN) ? 1.0 : -1.0;
                            double a = sgn * mon[(j - 1) * BLK + lane];
#pragma unroll
                            for (int i = 1; i < NW; i++) a = __builtin_fmin(a, sgn * mon[(j - 1) * BLK + lane + 64 * i]);
#pragma unroll
                            for (int off = 32; off > 0; off >>= 1) a = __builtin_fmin(a, __shfl_xor(a, off, 64));
                            if (lane == 0) rec[j] = sgn * a;
                        }
                    }
                    __syncthreads();
                    if (threadIdx.x < 7) sc.g[threadIdx.x] = rk45_monitor_of_record(rec, threadIdx.x);
                    if (c.status == ST_RUNNING) c.attempts--;   // (the attempt prepared after the accepted step is never made)
                    c.t = t_stop;
                    c.status = ST_TERMINAL;
                    break;
                }
            }
            if constexpr (ROOTS) {
                if (br_phase != 0) {                 // workgroup-uniform
                    double q[NQ];
                    monitors_init(q);
                    MARL_ONCE if (l0 < N) {
                        double d[NF];
#pragma unroll
                        for (int f = 0; f < NF; f++) d[f] = (br_t == c.t_old) ? MARL_Y(f) : h * esum[f] + MARL_Y(f);   // (x = 0: as the frames)
                        double U, W;
                        uw_point(d[4], C, sb.T, U, W);
                        monitors_accumulate<true>(q, d, U, W);   // (a state inside an accepted step: all finite)
                    }
#pragma unroll
                    for (int j = 1; j < NQ; j++) mon[(j - 1) * BLK + threadIdx.x] = q[j];
                    __syncthreads();
                    // monitor br_e of the probed state: EVERY wave reduces that one column, in the same order - the same value everywhere
                    const int slot = rk45_monitor_slot(br_e);
                    const double sgn = (slot <= NQMIN) ? 1.0 : -1.0;
                    double a = sgn * mon[(slot - 1) * BLK + lane];
#pragma unroll
                    for (int i = 1; i < NW; i++) a = __builtin_fmin(a, sgn * mon[(slot - 1) * BLK + lane + 64 * i]);
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) a = __builtin_fmin(a, __shfl_xor(a, off, 64));
                    const double val = to_sgpr((br_e == 3 || br_e == 4) ? sgn * a - 1.0 : sgn * a);
                    // the order of radau_control_step's PC_BRENT: f(a), f(b), the early returns, then brent_advance until the root or 100 iterations
                    if (br_phase == 1) {
                        br_fa = val;
                        br_phase = 2;
                        probe_at(c.t);
                        continue;
                    }
                    bool done = false;
                    double root = 0.0;
                    if (br_phase == 2) {
                        if (br_fa == 0.0) { done = true; root = c.t_old; }
                        else if (val == 0.0) { done = true; root = c.t; }
                        else {
                            bs.xpre = c.t_old; bs.xcur = c.t; bs.fpre = br_fa; bs.fcur = val;
                            bs.xblk = 0.0; bs.fblk = 0.0; bs.spre = 0.0; bs.scur = 0.0;
                            br_phase = 3;
                        }
                    } else {
                        bs.fcur = val;
                        br_iter++;
                        if (br_iter >= 100) { done = true; root = bs.xcur; }
                    }
                    if (!done) {
                        if (brent_advance(bs)) { done = true; root = bs.xcur; }
                    }
                    bs.xpre = to_sgpr(bs.xpre); bs.xcur = to_sgpr(bs.xcur); bs.xblk = to_sgpr(bs.xblk); bs.fpre = to_sgpr(bs.fpre);
                    bs.fcur = to_sgpr(bs.fcur); bs.fblk = to_sgpr(bs.fblk); bs.spre = to_sgpr(bs.spre); bs.scur = to_sgpr(bs.scur);
                    if (!done) {
                        probe_at(bs.xcur);
                        continue;
                    }
                    // (wave 0 did this step's bookkeeping before its first probe: n_events[br_e] - 1 is the count before the step, < max_events)
                    if constexpr (TERM) {
                        if (term_step) {             // kept until the rule has said which of them happened
#pragma unroll
                            for (int e = 0; e < 7; e++)
                                if (e == br_e) term_root[e] = to_sgpr(root);
                        } else if (threadIdx.x == 0) t_events[((int64_t)blockIdx.x * 7 + br_e) * max_events + (sc.n_events[br_e] - 1)] = root;
                    } else {
                        if (threadIdx.x == 0) t_events[((int64_t)blockIdx.x * 7 + br_e) * max_events + (sc.n_events[br_e] - 1)] = root;
                    }
                    ev_mask = to_sgpr((int32_t)(ev_mask & ~(1 << br_e)));
                    if (ev_mask != 0) {
                        first_probe();
                        continue;
                    }
                    br_phase = 0;
                    if constexpr (TERM) {
                        if (term_step) {             // every root of the step is known: the rule, the same in every lane
                            int64_t nev[7], slot[7];
#pragma unroll
                            for (int e = 0; e < 7; e++) nev[e] = sc.n_events[e];
                            uint32_t keep = 0;
                            double ts = c.t;
                            rk_terminal_step((uint32_t)term_act, term_root, nev, lim.k, max_events, &keep, &ts, nev, slot);
                            t_stop = to_sgpr(ts);
                            const int kept = to_sgpr((int32_t)keep);
                            __syncthreads();         // every wave has read sc.n_events
                            if (threadIdx.x == 0) {
#pragma unroll
                                for (int e = 0; e < 7; e++) {
                                    if (!((kept >> e) & 1)) continue;
                                    rk45_event_one(sc, e, rk45_monitor_of_record(rec, e));
                                    if (slot[e] >= 0) t_events[((int64_t)blockIdx.x * 7 + e) * max_events + slot[e]] = term_root[e];
                                }
                            }
                            if (next_sample()) {     // the samples up to t_stop
                                sampling = true;
                                continue;
                            }
                            stopping = true;
                            probe_at(t_stop);
                            continue;
                        }
                    }
                    if (next_sample()) {             // then the step's samples
                        sampling = true;
                        continue;
                    }
#pragma unroll
                    for (int f = 0; f < NF; f++) {   // the postponed commit, as after the last sample
                        if (f < PARK) pk[f * BLK] = yn[f]; else y[f] = yn[f];
                        k1[f] = k7[f];
                    }
                    if (c.status != ST_RUNNING) break;
                    continue;
                }
            }
            if constexpr (EVAL) {
                if (sampling) {                      // workgroup-uniform
                    double* fr = Yeval + ((int64_t)blockIdx.x * n_eval + ie) * (NF * N);
                    MARL_ONCE if (l0 < N) {
#pragma unroll
                        for (int f = 0; f < NF; f++)   // (x = 0, a sample at t0: y_old itself, whatever 0 * K_j gives)
                            fr[at<LAYOUT_FIELD_MAJOR>(f, l0, N)] = (te == c.t_old) ? MARL_Y(f) : h * esum[f] + MARL_Y(f);
                    }
                    ie = to_sgpr(ie + 1);
                    if (next_sample()) continue;     // another sample in the same step
                    sampling = false;
                    if constexpr (TERM) {
                        if (term_step) {             // then the stop
                            stopping = true;
                            probe_at(t_stop);
                            continue;
                        }
                    }
#pragma unroll
                    for (int f = 0; f < NF; f++) {   // the commit the accepted attempt postponed: y_new, k7 as the replay left them
                        if (f < PARK) pk[f * BLK] = yn[f]; else y[f] = yn[f];
                        k1[f] = k7[f];
                    }
                    if (c.status != ST_RUNNING) break;
                    continue;
                }
            }
            if (events_pending) {                    // wave-uniform
                event_bookkeeping();
                events_pending = false;
            }
            double q[NQ];
            monitors_init(q);
            MARL_ONCE if (l0 < N) {
#pragma unroll
                for (int f = 0; f < NF; f++) q[0] += dp45_err2(esum[f], h, MARL_Y(f), yn[f], rtol, atol);
                monitors_accumulate<true>(q, yn, aux.U, aux.W);   // (only read for accepted attempts: all finite)
            }
            double e2 = q[0];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) e2 += __shfl_xor(e2, off, 64);   // every lane: the wave's sum (same order in every lane pair)
            if (lane == 0) wsum[wave] = e2;
#pragma unroll
            for (int j = 1; j < NQ; j++) mon[(j - 1) * BLK + threadIdx.x] = q[j];
            __syncthreads();                         // the ONE barrier between the attempt and the decision
            double sumsq = 0.0;
#pragma unroll
            for (int w = 0; w < NW; w++) sumsq += wsum[w];                          // wave order: the same sum in every wave
            sumsq = to_sgpr(sumsq);
            bool accepted;
            if constexpr (DP) accepted = rk45_decide_lean(c, sumsq, inv_n, sb.T); else accepted = M::decide_lean(c, sumsq, inv_n, sb.T);
            if (accepted) {
                if (threadIdx.x == 0) { sc.t_old = c.t_old; sc.h_prev = c.h_prev; sc.t = c.t; }   // the step the pending events belong to
                if (c.t - c.t_bound >= 0.0) c.status = ST_DONE;   // (rk45_advance_status without the event pause, which this loop shape does not have)
                else if (c.t >= c.pause_t) c.status = ST_PAUSED;
            }
            if (c.status == ST_RUNNING) {
                if constexpr (DP) rk45_prepare_attempt_lean(c); else M::prepare_attempt_lean(c);
            }
            c.t = to_sgpr(c.t); c.h_abs = to_sgpr(c.h_abs); c.h_try = to_sgpr(c.h_try); c.t_new = to_sgpr(c.t_new);
            const int status = c.status;
            if (accepted) {
                // monitors of y_new: wave w reduces record slot w + 1 (+ NW, ...) over the workgroup's columns
#pragma unroll
                for (int jj = 0; jj < (NMON + NW - 1) / NW; jj++) {
                    const int j = wave + jj * NW + 1;   // wave-uniform
                    if (j < NQ) {
                        // (finite values: see monitors_accumulate<true>; a maximum is the negated minimum of the negated values)
                        const double sgn = (j <= NQMIN) ? 1.0 : -1.0;
                        double a = sgn * mon[(j - 1) * BLK + lane];
#pragma unroll
                        for (int i = 1; i < NW; i++) a = __builtin_fmin(a, sgn * mon[(j - 1) * BLK + lane + 64 * i]);
#pragma unroll
                        for (int off = 32; off > 0; off >>= 1) a = __builtin_fmin(a, __shfl_xor(a, off, 64));
                        if (lane == 0) rec[j] = sgn * a;
                    }
                }
                events_pending = true;
                if (status != ST_RUNNING && Yold) {
                    MARL_KEEP_OLD_STEP()
                }
                if constexpr (ROOTS) {
                    __syncthreads();                 // rec is whole: the sign test of this step, the same in every wave
                    int m = 0;
#pragma unroll
                    for (int e = 0; e < 7; e++) {    // ivp.py:149-151, as rk45_event_one; beyond max_events a sign change is only counted
                        const double go = sc.g[e], gn = rk45_monitor_of_record(rec, e);
                        const bool up = go <= 0.0 && gn >= 0.0, down = go >= 0.0 && gn <= 0.0;
                        if ((up || down) && sc.n_events[e] < max_events) m |= 1 << e;
                        if constexpr (TERM) {
                            if (up || down) term_act |= 1 << e;
                        }
                    }
                    ev_mask = to_sgpr((int32_t)m);
                    if constexpr (TERM) {
                        term_act = to_sgpr((int32_t)term_act);
                        int64_t nev[7];
#pragma unroll
                        for (int e = 0; e < 7; e++) nev[e] = sc.n_events[e];
                        if (to_sgpr((int32_t)rk_terminal_any_met((uint32_t)term_act, nev, lim.k)) != 0) {
                            // a limit is met: all of the step's roots first, kept in registers; sc stays as it is until the rule has spoken
                            term_step = true;
                            ev_mask = term_act;
                            events_pending = false;
                            first_probe();
                            continue;
                        }
                        term_act = 0;
                    }
                    if (ev_mask != 0) {              // roots inside this step: locate them first
                        __syncthreads();             // every wave has read sc.g / sc.n_events
                        event_bookkeeping();
                        events_pending = false;
                        first_probe();
                        continue;
                    }
                }
                if constexpr (EVAL) {
                    if (next_sample()) {             // samples inside this step: replay it first, commit afterwards
                        sampling = true;
                        continue;
                    }
                }
#pragma unroll
                for (int f = 0; f < NF; f++) {
                    if (f < PARK) pk[f * BLK] = yn[f]; else y[f] = yn[f];
                    k1[f] = k7[f];
                }
            }
            if (status != ST_RUNNING) break;
        }
        __syncthreads();                             // the last accepted step's monitors are reduced
        if (events_pending) event_bookkeeping();
        __syncthreads();
        if (threadIdx.x == 0) {                      // the replicated controller back into the record that leaves the kernel
            sc.t = c.t; sc.h_abs = c.h_abs; sc.h_try = c.h_try; sc.t_new = c.t_new;
            sc.err_norm = sqrt(c.err_norm);          // (rk45_decide_lean keeps the mean square)
            sc.nfev = c.nfev; sc.n_acc = c.n_acc; sc.n_rej = c.n_rej; sc.attempts = c.attempts;
            sc.status = c.status; sc.rejected = c.rejected; sc.accepted_last = c.accepted_last; sc.cur = c.cur;
            if constexpr (EVAL) n_done[blockIdx.x] = ie;   // frames written; the rest of the instance's frame memory is untouched
        }
    }
    MARL_ONCE if (l0 < N) {
#pragma unroll
        for (int f = 0; f < NF; f++) yg[at<LAYOUT_FIELD_MAJOR>(f, l0, N)] = MARL_Y(f);
    }
#undef MARL_Y
#undef MARL_KEEP_OLD_STEP
    if (threadIdx.x == 0) {
        sc.cur = 0;
        ctrls[blockIdx.x] = sc;
    }
}

// sweeps and single small runs that never pause on a monitor sign change
template <int BLK, bool VD = false>
__global__ void __launch_bounds__(BLK) rk45_sweep_kernel(double* __restrict__ Y, const DevConsts* __restrict__ consts,
                                                         Rk45Ctrl* __restrict__ ctrls, int64_t N,
                                                         double* __restrict__ Yold, double* __restrict__ Fold)
{
    rk45_sweep_body<BLK, VD, true>(Y, consts, ctrls, N, Yold, Fold);
}

// single small runs with event root finding (Rk45Ctrl.pause_on_event): the decision to pause needs this step's events
template <int BLK, bool VD = false>
__global__ void __launch_bounds__(BLK) rk45_sweep_events_kernel(double* __restrict__ Y, const DevConsts* __restrict__ consts,
                                                                Rk45Ctrl* __restrict__ ctrls, int64_t N,
                                                                double* __restrict__ Yold, double* __restrict__ Fold)
{
    rk45_sweep_body<BLK, VD, false>(Y, consts, ctrls, N, Yold, Fold);
}

// sweeps with t_eval: the loop of rk45_sweep_kernel, and after every accepted step the samples inside it by dense output.
//   t_eval: n_eval sorted times, shared by all instances; Yeval: [instance][n_eval][5][N]; n_done: [instance] frames written
//   (an instance that stops early leaves the later frames alone; one that is not running at entry writes nothing, n_done included).
template <int BLK, bool VD = false>
__global__ void __launch_bounds__(BLK) rk45_sweep_eval_kernel(double* __restrict__ Y, const DevConsts* __restrict__ consts,
                                                              Rk45Ctrl* __restrict__ ctrls, int64_t N,
                                                              const double* __restrict__ t_eval, int64_t n_eval,
                                                              double* __restrict__ Yeval, int64_t* __restrict__ n_done)
{
    rk45_sweep_body<BLK, VD, true, true>(Y, consts, ctrls, N, nullptr, nullptr, t_eval, n_eval, Yeval, n_done);
}

// sweeps that also locate the monitors' roots (the reference's events=[7], Evolve_scenario.py:118-145, 175-177): the loop of
// rk45_sweep_eval_kernel with one more barrier per accepted step, and in a step in which a monitor changes sign Brent's method on
// dense-output replays of that step (scipy ivp.py:673-694, solve_event_equation :51-76).
//   t_events: [instance][7][max_events], filled by the caller (NaN); root k of monitor e of instance b at (b * 7 + e) * max_events + k,
//   k < max_events - further sign changes are only counted (Rk45Ctrl.n_events).  n_eval may be 0 (t_eval, Yeval unused).
template <int BLK, bool VD = false>
__global__ void __launch_bounds__(BLK) rk45_sweep_roots_kernel(double* __restrict__ Y, const DevConsts* __restrict__ consts,
                                                               Rk45Ctrl* __restrict__ ctrls, int64_t N,
                                                               const double* __restrict__ t_eval, int64_t n_eval,
                                                               double* __restrict__ Yeval, int64_t* __restrict__ n_done,
                                                               double* __restrict__ t_events, int64_t max_events)
{
    rk45_sweep_body<BLK, VD, true, true, true>(Y, consts, ctrls, N, nullptr, nullptr, t_eval, n_eval, Yeval, n_done, t_events, max_events);
}

// rk45_sweep_roots_kernel honouring terminal monitors (marl_sweep_rk45_terminal_dev; `lim`: marl_set_terminal's limits): an instance
// whose monitor meets its limit ends at that root with ST_TERMINAL, the state the step's dense output there.  t_events may be NULL with
// max_events = 0 (the roots of a terminal step are located all the same), n_eval may be 0.
template <int BLK, bool VD = false>
__global__ void __launch_bounds__(BLK) rk45_sweep_term_kernel(double* __restrict__ Y, const DevConsts* __restrict__ consts,
                                                              Rk45Ctrl* __restrict__ ctrls, int64_t N,
                                                              const double* __restrict__ t_eval, int64_t n_eval,
                                                              double* __restrict__ Yeval, int64_t* __restrict__ n_done,
                                                              double* __restrict__ t_events, int64_t max_events, TermLimits lim)
{
    rk45_sweep_body<BLK, VD, true, true, true, Dp45Method, true>(Y, consts, ctrls, N, nullptr, nullptr, t_eval, n_eval, Yeval, n_done, t_events,
                                                                 max_events, lim);
}

template <int BLK, bool VD = false>
__global__ void __launch_bounds__(BLK) rk4_sweep_kernel(double* __restrict__ Y, const DevConsts* __restrict__ consts,
                                                        const double* __restrict__ dts, int64_t N, int64_t nsteps)
{
    using SB = StencilBlock<BLK, false, VD>;
    __shared__ double lds[SB::LDS_DOUBLES];
    const DevConsts& C = consts[blockIdx.x];
    double* yg = Y + (int64_t)blockIdx.x * NF * N;
    Slab S = {N, 0, N, 0, N};
    const int64_t l0 = threadIdx.x;
    SB sb(lds, l0, consts + blockIdx.x);
    const double dt = dts[blockIdx.x];
    const double h2 = 0.5 * dt, h6 = dt / 6.0;
    double y[NF], ys[NF], k[NF], acc[NF];
    PointAux aux;
    load_cells<LAYOUT_FIELD_MAJOR>(yg, l0, S, C, y);
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
    }
    MARL_ONCE if (l0 < N) {
#pragma unroll
        for (int f = 0; f < NF; f++) yg[at<LAYOUT_FIELD_MAJOR>(f, l0, N)] = y[f];
    }
}

}  // namespace marl
