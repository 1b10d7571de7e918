"""Guard rails on the instruction stream of the headline kernels, read from the code object that ships (CPU suite).

The fixed-step fine-grid path (rk4_stream_kernel<256, 1, 4, false>, and the per-level rk4_fused_kernel<256, 1, 4> that computes the
same bits) is bound by fp64 VALU issue, so every vector instruction that is not arithmetic costs time.  Two kinds used to sit on the
path taken by 15 of every 16 evaluations: wave-uniform conditions turned into a lane mask in vector registers (`v_cndmask_b32 vN, 0, 1, s[..]`
followed by `v_cmp`) and fp64 literals copied into vector registers with `v_mov_b32` pairs.  Removing them took the dynamic VALU count
from 10.15 to 9.27 instructions per grid-point-step (profiles/r05_lab_hot_path_valu.log).  The static counts below are upper bounds
taken from that build: an edit that puts such moves back onto the evaluation raises them and fails here, before a GPU run would show
it.  The resource records that the headline's occupancy rests on (four waves per SIMD) are pinned beside them.
"""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from check_stream_isa import DEFAULT_SO, disassemble_so, functions  # noqa: E402

STREAM = "rk4_stream_kernelILi256ELi1ELi4ELb0EE"      # the headline kernel (tiled layout, 4 steps per level)
FUSED = "rk4_fused_kernelILi256ELi1ELi4ELb0EE"        # the same evaluations, one launch per level

# kernel -> (literal v_mov_b32, v_cndmask_b32 vN, 0, 1, ...): the counts of the build that removed them from the evaluation
BOUNDS = {STREAM: (575, 20), FUSED: (563, 20)}


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(DEFAULT_SO):
        pytest.skip("libmarl_hip.so has not been built")
    text = disassemble_so(DEFAULT_SO)
    out = {}
    for pat in BOUNDS:
        fns = functions(text, pat)
        assert len(fns) == 1, (pat, sorted(fns))
        out[pat] = next(iter(fns.values()))
    return out


def literal_moves(ins):
    return sum(1 for _a, op, o, _t in ins if op.startswith("v_mov_b32") and re.match(r"v\d+,\s*(0x[0-9a-fA-F]+|-?\d+)$", o.strip()))


def mask_round_trips(ins):
    return sum(1 for _a, op, o, _t in ins if op.startswith("v_cndmask_b32") and re.match(r"v\d+,\s*0,\s*1,", o.strip()))


@pytest.mark.parametrize("kern", sorted(BOUNDS))
def test_no_literal_moves_or_lane_mask_round_trips_come_back(kernels, kern):
    ins = kernels[kern]
    lit, cnd = literal_moves(ins), mask_round_trips(ins)
    max_lit, max_cnd = BOUNDS[kern]
    assert lit <= max_lit, f"{kern}: {lit} literal v_mov_b32 (bound {max_lit})"
    assert cnd <= max_cnd, f"{kern}: {cnd} v_cndmask_b32 ..., 0, 1 (bound {max_cnd})"


def test_headline_kernels_keep_their_resources():
    from test_kernel_resources import kernel_records, pick
    if not os.path.exists(DEFAULT_SO):
        pytest.skip("libmarl_hip.so has not been built")
    recs = kernel_records()
    # persistent loop: scratch only for the item prologue (28 B in this build, 36 B before), four waves per SIMD, LDS as before
    for name, r in pick(recs, STREAM).items():
        assert r["private_segment_fixed_size"] <= 28 and r["vgpr_count"] <= 128 and r["group_segment_fixed_size"] == 31752, (name, r)
    # per-level launch: no scratch at all
    for name, r in pick(recs, FUSED).items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_count"] <= 128 and r["group_segment_fixed_size"] == 31744, (name, r)
