"""The chained streamed RK4 loop (rk4_chain_kernel) keeps the bits it had: SHA-256 of the final state against recorded digests.

Work on the code around the arithmetic of rk4_chain_kernel (spill traffic, the window prologue, statement order in the reuse path) must
not change a single fp64 result.  The digests below were recorded on an MI355X from a build of the parent commit

    d551514  "Radau sweeps: t_eval frames by dense output inside the sweep"

with exactly the calls of this file (print the digests of a build with `pytest -s`).  The shapes are the smallest that hold every window
the interior fast path must NOT take - cell 0, cell N - 1, both edges of the dissolution zone, a clipped last window:

  * N = 6300, K = 2: the last chain's second window is 16 cells wide, behind a full one;
  * N = 6100, K = 2: the last chain is one window of 16 cells;
  * N = 5003, K = 2, amplitude 0.05: waves that mix the reuse tiers and the full path;
  * N = 9000, K = 3;
  * 8 steps (two levels: ping-pong) and 12 steps (three levels: the third-buffer route), both layouts, one case with no_reuse = 1.

Fixed settings as in test_gpu_rk4_chain.py: rk4_variant = 2 (4 steps per level), rk4_stream = 2, a forced rk4_chain, dt = 0.25 dx^2,
synthetic_state.
"""
import hashlib

import numpy as np
import pytest

from common import scenario, synthetic_state

pytestmark = pytest.mark.gpu

PARENT = "d551514"
VARIANT_4_STEPS = 2

# (N, K, steps, layout [1 tiled, 0 field-major], amplitude, no_reuse): sha256 of the field-major float64 result
RECORDED = {
    (6300, 2, 8, 1, 0.02, 0): "a1a5b16053c13c420e41bc907e4fa3514651de28912ae2a8217cea013b021b2e",
    (6300, 2, 8, 0, 0.02, 0): "a1a5b16053c13c420e41bc907e4fa3514651de28912ae2a8217cea013b021b2e",
    (6300, 2, 12, 1, 0.02, 0): "0eedef4ce80936faa60b0a463e60ec2f6c1912aa61029f17c4a9e0aa95c3bb1c",
    (6300, 2, 12, 0, 0.02, 0): "0eedef4ce80936faa60b0a463e60ec2f6c1912aa61029f17c4a9e0aa95c3bb1c",
    (6100, 2, 8, 1, 0.02, 0): "6a62606ba42627e1bf71e34c802ea28dd24b1ae013cab8b77373d64e414bfc51",
    (6100, 2, 12, 1, 0.02, 0): "9aeb20b1691b726909ec236e5afa64a531dd0eca07f488da3d1e3c330f5e01be",
    (5003, 2, 8, 1, 0.05, 0): "432377930096da5d0151b6c3075fda7dd242ae74baed7f3c30fc25e2b04a1498",
    (5003, 2, 12, 1, 0.05, 0): "87c5667f95ff8a27da2b7468c1ea667f6ac7738536e941ffb0a3509c7f38bfda",
    (9000, 3, 8, 1, 0.02, 0): "b6022c30189bbacfda3a91bdc522a761bdf64fbb10490974a20973c7b743a781",
    (9000, 3, 12, 1, 0.02, 0): "a803152430ca2a53c2de470152c499de7742f9a0b42be96f8c8cfc6d570aa521",
    (6300, 2, 12, 1, 0.02, 1): "fa298e5b56f3cc78990a2528f7d105127c7a755e6c885dba19a0e85e49c127e2",
}


def digest(case):
    import torch
    from marlpde_amd.LHeureux_model import LMAHeureuxPorosityDiff
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    N, K, nsteps, layout, amplitude, no_reuse = case
    p = scenario("default", N)
    eq = LMAHeureuxPorosityDiff.from_scenario(p, device=0)
    eq.use_stream(torch.cuda.current_stream().cuda_stream)
    eq.set_option("rk4_variant", VARIANT_4_STEPS)
    eq.set_option("no_reuse", no_reuse)
    eq.set_option("rk4_stream", 2)
    eq.set_option("rk4_chain", K)
    y = synthetic_state(p, N, amplitude=amplitude)
    dt = 0.25 * (eq.Depths.length / N) ** 2
    yd = torch.from_numpy(y).cuda()
    buf = torch.zeros(eq.state_doubles(layout), dtype=torch.float64, device="cuda")
    eq.convert_layout_device(yd.data_ptr(), buf.data_ptr(), 0, layout)
    eq.integrate_rk4_device(buf.data_ptr(), dt, nsteps, layout)
    eq.synchronize()
    got = torch.empty_like(yd)
    eq.convert_layout_device(buf.data_ptr(), got.data_ptr(), layout, 0)
    eq.synchronize()
    out = got.cpu().numpy()
    eq.close()
    assert out.dtype == np.float64 and out.shape == (5 * N,)
    assert np.all(np.isfinite(out)) and not np.array_equal(out, y)
    return hashlib.sha256(np.ascontiguousarray(out).tobytes()).hexdigest()


@pytest.mark.parametrize("case", sorted(RECORDED), ids=lambda c: "N%d-K%d-s%d-l%d-a%g-nr%d" % c)
def test_final_state_has_the_bits_of_the_parent_commit(case):
    got = digest(case)
    print(f"\n{case!r}: \"{got}\",")
    assert got == RECORDED[case], f"{case}: sha256 {got}, parent {PARENT} gave {RECORDED[case]}"
