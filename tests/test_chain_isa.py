"""Build-time checks of rk4_chain_kernel (the streamed RK4 loop with chained windows) on the code object that ships (CPU suite).

The kernel passes tiles between workgroups exactly as rk4_stream_kernel does, so the same invariants of the generated code must hold
(tools/check_stream_isa.py, I1-I5), and its speed rests on the same resources: four waves per SIMD, four workgroups' LDS per CU, no
scratch inside the evaluations, and nothing but arithmetic added to the evaluation of every wave - the recorded seam is written and
read under scalar branches that one wave each takes.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from check_stream_isa import DEFAULT_SO, check_text, disassemble_so, functions  # noqa: E402
from test_hot_path_isa import STREAM, literal_moves, mask_round_trips  # noqa: E402

CHAIN = "rk4_chain_kernel"
CHAIN_TILED = "rk4_chain_kernelILi256ELi1ELi4EE"
CHAIN_FIELD_MAJOR = "rk4_chain_kernelILi256ELi0ELi4EE"

# Literal v_mov_b32 of the build that ships, as upper bounds.  rk4_stream_kernel<256, tiled, 4, false> has 575 in the same build
# (tests/test_hot_path_isa.py).  The four stage blocks (from each exchange barrier to the next: 82, 82, 82 and 293 with the tail of the
# step loop) hold the same moves in both kernels and both layouts.  The differences sit outside them: the tiled instantiation has one
# more in the window prologue in front of the first stage barrier (24 against 23); the field-major one has 23 there and one fewer
# behind the last stage barrier.
LITERAL_MOVES = {CHAIN_TILED: 576, CHAIN_FIELD_MAJOR: 574}


@pytest.fixture(scope="module")
def text():
    if not os.path.exists(DEFAULT_SO):
        pytest.skip("libmarl_hip.so has not been built")
    return disassemble_so(DEFAULT_SO)


def test_both_instantiations_keep_the_stream_invariants(text):
    res = check_text(text, pattern=CHAIN)
    assert len(res) == 2, sorted(res)   # <256, tiled, 4> and <256, field-major, 4>, constant porosity diffusion only
    assert {n: bad for n, bad in res.items() if bad} == {}


def test_resources_of_the_persistent_loop():
    from test_kernel_resources import kernel_records, pick
    if not os.path.exists(DEFAULT_SO):
        pytest.skip("libmarl_hip.so has not been built")
    hits = pick(kernel_records(), CHAIN)
    assert len(hits) == 2, sorted(hits)
    for name, r in hits.items():
        assert r["vgpr_count"] <= 128 and r["private_segment_fixed_size"] <= 28 and r["group_segment_fixed_size"] <= 40960, (name, r)


@pytest.mark.parametrize("kern", sorted(LITERAL_MOVES))
def test_no_lane_mask_round_trips_or_literal_moves_beyond_the_unchained_kernel(text, kern):
    fns = functions(text, kern)
    assert len(fns) == 1, (kern, sorted(fns))
    ins = next(iter(fns.values()))
    old = functions(text, STREAM)
    assert len(old) == 1, sorted(old)
    cnd, max_cnd = mask_round_trips(ins), mask_round_trips(next(iter(old.values())))
    assert cnd <= max_cnd, f"{kern}: {cnd} v_cndmask_b32 ..., 0, 1 (rk4_stream_kernel<256, 1, 4, false>: {max_cnd})"
    lit = literal_moves(ins)
    assert lit <= LITERAL_MOVES[kern], f"{kern}: {lit} literal v_mov_b32 (bound {LITERAL_MOVES[kern]})"
