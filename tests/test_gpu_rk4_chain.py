"""The streamed RK4 loop with chained windows (rk4_chain_kernel, option rk4_chain) against per-level launches and the oracle.

A chained work item is K windows run one after another by the same workgroup; only the first recomputes a left halo, every later one
takes the left neighbour of its thread 0 from the stage states that lane 239 of its predecessor recorded.  Decomposition (marl_api.hip,
chain_shape): the grid's last tile [224 t_last, N), t_last = (N - 1) // 224, is a plain window of its own; chains of 224 + 240 (K - 1)
cells tile [0, 224 t_last), the last one clipped there.

Fixed settings: rk4_variant = 2 (4 steps per level), rk4_stream = 2 plus a forced rk4_chain, reference rk4_stream = 0, dt = 0.25 dx^2,
synthetic_state.  Every streamed case runs three times: a race does not show every time.

On the case "a last sub-window one cell wide": it cannot occur.  Chain starts are multiples of 224 + 240 (K - 1) and the bound is a
multiple of 224, so the cells left for a last chain, and with them the width of its last window, are multiples of 16.  The narrowest
shapes that do occur are tested instead: a last window 16 cells wide behind a full one (N = 6300, K = 2) and a last chain that is one
window of 16 cells (N = 6100, K = 2) - exactly the halo that the last tile reads from it.
"""
import numpy as np
import pytest

from common import assert_increment, rel_to_max, scenario, synthetic_state

pytestmark = pytest.mark.gpu

VARIANT_4_STEPS = 2


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def make_model(N):
    from marlpde_amd.LHeureux_model import LMAHeureuxPorosityDiff
    p = scenario("default", N)
    return p, LMAHeureuxPorosityDiff.from_scenario(p, device=0)


def run(torch, eq, y, dt, nsteps, layout, stream, chain):
    """One fixed-step run from the host state y (field-major) in `layout`; returns the field-major result as a numpy array."""
    eq.set_option("rk4_stream", stream)
    eq.set_option("rk4_chain", chain)
    yd = torch.from_numpy(y).cuda()
    buf = torch.zeros(eq.state_doubles(layout), dtype=torch.float64, device="cuda")
    eq.convert_layout_device(yd.data_ptr(), buf.data_ptr(), 0, layout)
    eq.integrate_rk4_device(buf.data_ptr(), dt, nsteps, layout)
    eq.synchronize()
    got = torch.empty_like(yd)
    eq.convert_layout_device(buf.data_ptr(), got.data_ptr(), layout, 0)
    eq.synchronize()
    return got.cpu().numpy()


def chained_equals_per_level(torch, N, K, nsteps, layout, amplitude=0.02, no_reuse=0, max_items=0):
    p, eq = make_model(N)
    eq.use_stream(torch.cuda.current_stream().cuda_stream)
    eq.set_option("rk4_variant", VARIANT_4_STEPS)
    eq.set_option("no_reuse", no_reuse)
    eq.set_option("rk4_stream_max_items", max_items)
    y = synthetic_state(p, N, amplitude=amplitude)
    dt = 0.25 * (eq.Depths.length / N) ** 2
    ref = run(torch, eq, y, dt, nsteps, layout, 0, 0)
    assert np.all(np.isfinite(ref)) and not np.array_equal(ref, y)
    for _ in range(3):
        got = run(torch, eq, y, dt, nsteps, layout, 2, K)
        differ = np.flatnonzero(np.any(got.reshape(5, N) != ref.reshape(5, N), axis=0))
        assert differ.size == 0, f"{differ.size} cells differ, first {differ[:8]}, last {differ[-8:]}"
    eq.close()


# With no_reuse = 1 every evaluation takes the full path: no value depends on which cells share a wave, so the chained result must
# have the per-level bits at any size.
EXACT_SHAPES = [
    # N, K, steps, max_items
    (150, 4, 4 * 6, 0),           # grid smaller than one chain: the last tile is the only item
    (700, 2, 4 * 5, 0),           # two chains + the last tile; the second chain a single clipped window
    (1121, 2, 4 * 4, 0),          # N = 224 * 5 + 1: a last tile of one cell
    (6300, 2, 4 * 4, 0),          # the last chain's second window is 16 cells wide (the narrowest possible: see the module docstring)
    (6100, 2, 4 * 4, 0),          # the last chain is one window of 16 cells: all of the last tile's left halo
    (5003, 2, 4 * 7 + 3, 30),     # 12 items per level, 2 levels per launch: 7 levels in launches of 2, 2, 2, 1
]


@pytest.mark.parametrize("N,K,nsteps,max_items", EXACT_SHAPES)
def test_chained_windows_without_reuse_are_bit_identical_to_per_level_launches(torch_cuda, N, K, nsteps, max_items):
    chained_equals_per_level(torch_cuda, N, K, nsteps, 1, no_reuse=1, max_items=max_items)


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("K", [2, 3, 4, 8])
def test_chained_windows_without_reuse_odd_level_count_and_remainder(torch_cuda, K, layout):
    """N = 5003, 4 * 7 + 3 steps: an odd number of levels (the third buffer) and a remainder of per-level launches behind the chain."""
    chained_equals_per_level(torch_cuda, 5003, K, 4 * 7 + 3, layout, no_reuse=1)


@pytest.mark.parametrize("layout", [0, 1])
def test_chained_windows_with_reuse_against_oracle(torch_cuda, oracle, layout):
    """Reuse on at N = 5003, amplitude 0.05: the expansion variables sit between the second- and third-order tiers here and which one a
    wave takes depends on its lanes, so bits need not match the per-level path; the project's bounds for exactly this input
    (test_rk4_fused_variants_against_oracle) must hold."""
    torch = torch_cuda
    N, K, nsteps = 5003, 4, 4 * 2 + 3
    p, eq = make_model(N)
    eq.use_stream(torch.cuda.current_stream().cuda_stream)
    eq.set_option("rk4_variant", VARIANT_4_STEPS)
    y = synthetic_state(p, N, amplitude=0.05)
    dt = 0.25 * (eq.Depths.length / N) ** 2
    ref = oracle.rk4(oracle.params_from_model(eq), N, y, dt, nsteps)
    for _ in range(3):
        got = run(torch, eq, y, dt, nsteps, layout, 2, K)
        assert rel_to_max(got, ref) <= 1e-10
        assert_increment(got, ref, y, "rk4_fused_variants", nsteps)
    eq.close()


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("K", [2, 4])
def test_chained_windows_with_reuse_on_a_fine_grid_are_bit_identical(torch_cuda, K, layout):
    """N = 300 001, amplitude 0.02, 36 steps.  Outside cell N - 1 the range variable of the expansions stays five times under REUSE_TINY
    over the 4 steps a centre lives, so every interior wave takes the second-order tier in either decomposition; the wave that holds
    cell N - 1 consists of the same cells in both (the last tile is a plain window)."""
    chained_equals_per_level(torch_cuda, 300001, K, 36, layout)


def test_chained_loop_reports_a_raised_flag_and_recovers(torch_cuda):
    """The safety net through the new kernel: with the flag raised the waiting workgroups leave and marl_synchronize reports it; the
    next run has the per-level bits again."""
    torch = torch_cuda
    from marlpde_amd._abi import MarlError
    N, nsteps, layout, K = 300001, 24, 1, 4
    p, eq = make_model(N)
    eq.use_stream(torch.cuda.current_stream().cuda_stream)
    eq.set_option("rk4_variant", VARIANT_4_STEPS)
    y = synthetic_state(p, N, amplitude=0.02)
    dt = 0.25 * (eq.Depths.length / N) ** 2
    ref = run(torch, eq, y, dt, nsteps, layout, 0, 0)
    assert np.array_equal(run(torch, eq, y, dt, nsteps, layout, 2, K), ref)
    eq.set_option("rk4_stream_test_raise", 1)
    with pytest.raises(MarlError, match="state is invalid"):
        run(torch, eq, y, dt, nsteps, layout, 2, K)
    for _ in range(3):
        assert np.array_equal(run(torch, eq, y, dt, nsteps, layout, 2, K), ref)
    eq.close()
