// marl_dop853_grid_ctl.h - the scalar bookkeeping of the large-grid DOP853 loop (marl_dop853_grid.h; host driver: marl_api.hip) that
// is neither scipy's controller (marl_dop853_ctl.h) nor arithmetic on the grid: which physical slot of the stage-derivative arena holds
// K_j, how the per-workgroup records of an attempt are cut for the first level of their reduction, and where the pieces lie in the
// record buffer.  Kernels and host use the SAME functions, so the two sides cannot drift apart.  Nothing but <stdint.h>: a host C++
// compiler builds this header alone (tests/test_dop853_grid_cpu.py pins it to a numpy restatement that way).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define MARL_DOP853_GRID_FN __host__ __device__ __forceinline__
#else
#define MARL_DOP853_GRID_FN inline
#endif

namespace marl {

constexpr int DOP853_GRID_SLOTS = 16;                    // K_1..K_16 of a step, one state-shaped buffer each
constexpr int DOP853_GRID_BLK = 256;                     // threads of a window, one cell each
constexpr int DOP853_GRID_HALO = 1;                      // ONE evaluation per launch: one cell per side is invalid behind it
constexpr int DOP853_GRID_WRITTEN = DOP853_GRID_BLK - 2 * DOP853_GRID_HALO;
constexpr int64_t DOP853_GRID_REDUCE_GROUPS = 64;        // workgroups of the first reduction level, at most
constexpr int64_t DOP853_GRID_DIRECT_RECORDS = 256;      // up to this many records the control kernel reads them itself

// The physical slot of K_(j+1), j = 0..15, of the step whose first state lies in state buffer `frame` (0 or 1; Rk45Ctrl.cur while the
// step is being attempted, cur ^ 1 once it is accepted).  f(y_new) = K_13 of an accepted step is K_1 of the next one (FSAL), so slots
// 0 and 12 swap their roles with every acceptance - the same flip that swaps the two state buffers, and nothing is copied.
MARL_DOP853_GRID_FN int dop853_grid_slot(int j, int frame)
{
    if (j == 0) return frame ? 12 : 0;
    if (j == 12) return frame ? 0 : 12;
    return j;
}

// First level of the record reduction: `nrec` per-workgroup records are cut into `*groups` chunks of `*chunk` consecutive records
// (the last one shorter), one workgroup each, in index order - a fixed partition, so the sums are reproducible bit for bit.
// Returns false (and *groups = nrec, *chunk = 1) when the control kernel reads the records itself.
MARL_DOP853_GRID_FN bool dop853_grid_first_level(int64_t nrec, int64_t* chunk, int64_t* groups)
{
    if (nrec <= DOP853_GRID_DIRECT_RECORDS) {
        *chunk = 1;
        *groups = nrec;
        return false;
    }
    *chunk = (nrec + DOP853_GRID_REDUCE_GROUPS - 1) / DOP853_GRID_REDUCE_GROUPS;
    *groups = (nrec + *chunk - 1) / *chunk;
    return true;
}

// The record buffer of a grid of `nb` windows, in doubles: [nb records of 8] [<= 64 first-level records of 8] [nb second sums]
// [<= 64 first-level second sums].  Offsets of the four pieces and the total.
struct Dop853GridParts { int64_t rec, rec1, sum3, sum3_1, total; };
MARL_DOP853_GRID_FN Dop853GridParts dop853_grid_parts(int64_t nb)
{
    Dop853GridParts p;
    p.rec = 0;
    p.rec1 = nb * 8;
    p.sum3 = p.rec1 + DOP853_GRID_REDUCE_GROUPS * 8;
    p.sum3_1 = p.sum3 + nb;
    p.total = p.sum3_1 + DOP853_GRID_REDUCE_GROUPS;
    return p;
}

// scipy builds the dense output of an accepted step when a monitor changed sign in it or a sample falls into it
// (dop853_count_dense_output, marl_dop853_ctl.h).  pause_t is the first sample not yet written (+inf: none): it lies behind t_old
// (or is t0 itself, which belongs to the first step), so the step [t_old, t] holds a sample exactly when t >= pause_t.
MARL_DOP853_GRID_FN bool dop853_grid_step_is_dense(int fired, double t, double pause_t) { return fired != 0 || t >= pause_t; }

}  // namespace marl
