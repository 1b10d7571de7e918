"""rk4_exchange_kernel (option rk4_exchange = 1: the chained streamed RK4 loop with its LDS exchange laid out by cell and its cache slots in
pairs) against rk4_chain_kernel (rk4_exchange = 0) and against per-level launches (rk4_stream = 0), bit for bit.

The two kernels differ in LDS addresses only, so the new one must reproduce rk4_chain_kernel exactly in every case, with the
transcendental reuse and without it.  Against per-level launches the chained decomposition is bit-identical where no value depends on
which cells share a wave: with no_reuse = 1 always (tests/test_gpu_rk4_chain.py), which is where that comparison is made here.  With reuse
on, the new kernel is held to whatever rk4_chain_kernel gives: equal to the per-level bits exactly where rk4_chain_kernel is.  (On an
MI355X that is every case below but N = 5003, K = 3 with reuse, both layouts, where rk4_chain_kernel's waves take another reuse tier than
the per-level windows do - test_gpu_rk4_chain.py, test_chained_windows_with_reuse_against_oracle - and the new kernel follows it bit for bit.)

Shapes - the smallest at which the addressing can go wrong (decomposition: tests/test_gpu_rk4_chain.py):
  * N = 6100 and 6300, K = 2: a last chain of one 16-cell window; a 16-cell last window behind a full one;
  * N = 5003, K = 2 and 3: windows that hold cell 0 and cell N - 1, windows that straddle both ends of the dissolution zone;
  * N = 20 011, K = 8, 8 and 20 steps: two levels (ping-pong, both parities of the exchange and of the seam record) and five (the
    third buffer);
  * N = 1050, K = 2, a 15 % porosity modulation with a period of 75 cells: the burial velocity changes sign inside waves
    (test_gpu_parity.py, test_mixed_upwind_direction_inside_waves), so waves take the mixed-upwind branch and with it the 16-byte read of
    the right neighbour's solids.
Both device layouts.  Fixed settings: rk4_variant = 2 (4 steps per level), rk4_stream = 2 with a forced rk4_chain, dt = 0.25 dx^2 (0.1 dx^2
in the mixed-upwind case, as in its model), synthetic_state.
"""
import numpy as np
import pytest

from common import scenario, synthetic_state

pytestmark = pytest.mark.gpu

VARIANT_4_STEPS = 2


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def run(torch, eq, y, dt, nsteps, layout, stream, chain, exchange):
    """One fixed-step run from the host state y (field-major) in `layout`; returns the field-major result as a numpy array."""
    eq.set_option("rk4_stream", stream)
    eq.set_option("rk4_chain", chain)
    eq.set_option("rk4_exchange", exchange)
    yd = torch.from_numpy(y).cuda()
    buf = torch.zeros(eq.state_doubles(layout), dtype=torch.float64, device="cuda")
    eq.convert_layout_device(yd.data_ptr(), buf.data_ptr(), 0, layout)
    eq.integrate_rk4_device(buf.data_ptr(), dt, nsteps, layout)
    eq.synchronize()
    got = torch.empty_like(yd)
    eq.convert_layout_device(buf.data_ptr(), got.data_ptr(), layout, 0)
    eq.synchronize()
    return got.cpu().numpy()


def differing_cells(a, b, N):
    return np.flatnonzero(np.any(a.reshape(5, N) != b.reshape(5, N), axis=0))


def exchange_equals_chain_and_per_level(torch, N, K, nsteps, layout, no_reuse, amplitude=0.02, waves=8, dt_factor=0.25, mixed_upwind=False):
    from marlpde_amd.LHeureux_model import LMAHeureuxPorosityDiff
    p = scenario("default", N)
    eq = LMAHeureuxPorosityDiff.from_scenario(p, device=0)
    eq.use_stream(torch.cuda.current_stream().cuda_stream)
    eq.set_option("rk4_variant", VARIANT_4_STEPS)
    eq.set_option("no_reuse", no_reuse)
    y = synthetic_state(p, N, amplitude=amplitude, waves=waves)
    if mixed_upwind:
        Phi = y.reshape(5, N)[4]
        U = eq.presum + eq.rhorat * Phi ** 3 * (1 - np.exp(10 - 10 / Phi)) / (1 - Phi)
        up = (U > 0).reshape(-1)
        assert 0.2 < np.mean(up) < 0.8
        in_wave = np.convolve(up.astype(np.int64), np.ones(64, dtype=np.int64), mode="valid")   # cells with U > 0 among any 64 in a row
        assert in_wave.min() > 0 and in_wave.max() < 64, "every wave mixes both directions, wherever the windows start"
    dt = dt_factor * (eq.Depths.length / N) ** 2
    per_level = run(torch, eq, y, dt, nsteps, layout, 0, 0, 0)
    assert np.all(np.isfinite(per_level)) and not np.array_equal(per_level, y)
    chain = run(torch, eq, y, dt, nsteps, layout, 2, K, 0)
    chain_is_per_level = np.array_equal(chain, per_level)
    if no_reuse:
        assert chain_is_per_level, "rk4_chain_kernel itself differs from the per-level launches"
    for _ in range(2):   # (a race does not show every time)
        got = run(torch, eq, y, dt, nsteps, layout, 2, K, 1)
        d = differing_cells(got, chain, N)
        assert d.size == 0, f"against rk4_exchange = 0: {d.size} cells differ, first {d[:8]}, last {d[-8:]}"
        assert np.array_equal(got, chain)
        assert np.array_equal(got, per_level) == chain_is_per_level
    print(f"\nN={N} K={K} steps={nsteps} layout={layout} no_reuse={no_reuse}: rk4_chain_kernel equals per-level launches: {chain_is_per_level}")
    eq.close()


SHAPES = [
    # N, K, steps
    (6100, 2, 8),
    (6300, 2, 8),
    (5003, 2, 8),
    (5003, 3, 12),
    (20011, 8, 8),
    (20011, 8, 20),
]


@pytest.mark.parametrize("no_reuse", [0, 1])
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("N,K,nsteps", SHAPES)
def test_cell_major_exchange_has_the_bits_of_the_chained_kernel_and_of_per_level_launches(torch_cuda, N, K, nsteps, layout, no_reuse):
    exchange_equals_chain_and_per_level(torch_cuda, N, K, nsteps, layout, no_reuse)


@pytest.mark.parametrize("no_reuse", [0, 1])
@pytest.mark.parametrize("layout", [0, 1])
def test_mixed_upwind_waves_read_the_right_neighbours_solids(torch_cuda, layout, no_reuse):
    N = 1050
    exchange_equals_chain_and_per_level(torch_cuda, N, 2, 12, layout, no_reuse, amplitude=0.15, waves=N // 75, dt_factor=0.1, mixed_upwind=True)
