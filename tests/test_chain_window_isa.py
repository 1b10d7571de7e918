"""Per-window overhead of rk4_chain_kernel, read from the code object that ships (CPU suite).

The chained streamed loop is bound by fp64 VALU issue; what is left to gain around its arithmetic is the scalar spill traffic
(v_readlane / v_writelane: VALU instructions) and the per-lane bookkeeping of a window.  Both instantiations are split at their nine
s_barrier, in address order, as tools/kernel_isa.py does:

    block 4      from the barrier behind the neighbour wait to the first exchange barrier: the item's scalars, the window prologue and
                 the own-cell phase of the first evaluation of a step
    blocks 5-7   from each exchange barrier to the next
    block 8      from the last exchange barrier to the publish barrier: the fourth evaluation's stencil phase, the tail of the step loop,
                 the window's stores, and the out-of-line full-path code of every evaluation

(a) v_readlane + v_writelane of each of these blocks against the same block of rk4_stream_kernel<256, LAYOUT, 4, false> of the same build.
(b) the multiset of fp64 arithmetic opcodes of each block against the census of a build of the parent commit: a changed contraction, a
    lost or a duplicated operation shows here before any GPU run.

Where (a) stands (static counts of the build that ships, chain against stream; the parent commit d551514 in brackets):

                 tiled                       field-major
    block 4      26 against 35  (65)         30 against 57  (88)
    blocks 5-7   0, 0, 0 against 0, 0, 0  (2, 0, 0) in both layouts
    block 8       8 against 10  (18)          8 against 28  (28)

How it got there, and the forms that did not: profiles/r10_lab_chain_window.log.
"""
import collections
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from check_stream_isa import DEFAULT_SO, disassemble_so, functions  # noqa: E402

CHAIN = {"tiled": "rk4_chain_kernelILi256ELi1ELi4EE", "field_major": "rk4_chain_kernelILi256ELi0ELi4EE"}
STREAM = {"tiled": "rk4_stream_kernelILi256ELi1ELi4ELb0EE", "field_major": "rk4_stream_kernelILi256ELi0ELi4ELb0EE"}
PROLOGUE, STAGES = 4, (5, 6, 7, 8)

FP64 = re.compile(r"^v_(fma|fmac|mul|add|rcp|ldexp|rndne|min|max)_f64$|^v_cmpx?_\w+_f64$")

# fp64 census per block of rk4_chain_kernel<256, LAYOUT, 4> (the same in both layouts), recorded from a build of the parent commit
# d551514 "Radau sweeps: t_eval frames by dense output inside the sweep" with the Makefile's flags
PARENT_CENSUS = {
    4: {"v_add_f64": 13, "v_cmp_class_f64": 4, "v_cmp_eq_f64": 1, "v_cmp_lt_f64": 1, "v_cmp_neq_f64": 3, "v_cmp_ngt_f64": 5, "v_fma_f64": 44,
        "v_fmac_f64": 45, "v_ldexp_f64": 4, "v_max_f64": 5, "v_mul_f64": 56, "v_rcp_f64": 3, "v_rndne_f64": 4},
    5: {"v_add_f64": 40, "v_cmp_class_f64": 4, "v_cmp_eq_f64": 1, "v_cmp_le_f64": 3, "v_cmp_lt_f64": 1, "v_cmp_neq_f64": 3, "v_cmp_ngt_f64": 8,
        "v_cmp_nlg_f64": 1, "v_cmp_nlt_f64": 5, "v_fma_f64": 91, "v_fmac_f64": 108, "v_ldexp_f64": 7, "v_max_f64": 1, "v_mul_f64": 92,
        "v_rcp_f64": 8, "v_rndne_f64": 7},
    6: {"v_add_f64": 42, "v_cmp_class_f64": 4, "v_cmp_eq_f64": 1, "v_cmp_le_f64": 3, "v_cmp_lt_f64": 1, "v_cmp_neq_f64": 3, "v_cmp_ngt_f64": 8,
        "v_cmp_nlg_f64": 1, "v_cmp_nlt_f64": 5, "v_fma_f64": 90, "v_fmac_f64": 108, "v_ldexp_f64": 7, "v_max_f64": 1, "v_mul_f64": 91,
        "v_rcp_f64": 8, "v_rndne_f64": 7},
    7: {"v_add_f64": 42, "v_cmp_class_f64": 4, "v_cmp_eq_f64": 1, "v_cmp_le_f64": 3, "v_cmp_lt_f64": 1, "v_cmp_neq_f64": 3, "v_cmp_ngt_f64": 8,
        "v_cmp_nlg_f64": 1, "v_cmp_nlt_f64": 5, "v_fma_f64": 90, "v_fmac_f64": 108, "v_ldexp_f64": 7, "v_max_f64": 1, "v_mul_f64": 91,
        "v_rcp_f64": 8, "v_rndne_f64": 7},
    8: {"v_add_f64": 734, "v_cmp_class_f64": 4, "v_cmp_gt_f64": 16, "v_cmp_le_f64": 3, "v_cmp_neq_f64": 28, "v_cmp_nge_f64": 4,
        "v_cmp_ngt_f64": 8, "v_cmp_nlg_f64": 1, "v_cmp_nlt_f64": 5, "v_fma_f64": 162, "v_fmac_f64": 241, "v_ldexp_f64": 51, "v_mul_f64": 164,
        "v_rcp_f64": 22, "v_rndne_f64": 3},
}


@pytest.fixture(scope="module")
def text():
    if not os.path.exists(DEFAULT_SO):
        pytest.skip("libmarl_hip.so has not been built")
    return disassemble_so(DEFAULT_SO)


def blocks(text, kern):
    """The kernel's instructions (opcode only), split at its s_barrier in address order."""
    fns = functions(text, kern)
    assert len(fns) == 1, (kern, sorted(fns))
    out = [[]]
    for _a, op, _o, _t in next(iter(fns.values())):
        if op == "s_barrier":
            out.append([])
        else:
            out[-1].append(op)
    assert len(out) == 10, (kern, len(out))   # nine barriers (tools/check_stream_isa.py, I4)
    return out


def lane_traffic(ops):
    return sum(op.startswith(("v_readlane", "v_writelane")) for op in ops)


def census(ops):
    c = collections.Counter()
    for op in ops:
        base = re.sub(r"_e(32|64)$", "", op)   # (the encoding of an opcode is not part of the operation)
        if FP64.match(base):
            c[base] += 1
    return dict(c)


@pytest.mark.parametrize("layout", sorted(CHAIN))
@pytest.mark.parametrize("block", (PROLOGUE,) + STAGES)
def test_no_more_scalar_spill_traffic_than_the_unchained_kernel(text, layout, block):
    chain, stream = lane_traffic(blocks(text, CHAIN[layout])[block]), lane_traffic(blocks(text, STREAM[layout])[block])
    print(f"\n{layout} block {block}: v_readlane + v_writelane {chain} (rk4_stream_kernel: {stream})")
    assert chain <= stream, f"{layout}, block {block}: {chain} v_readlane + v_writelane, rk4_stream_kernel<256, {layout}, 4, false> has {stream}"


@pytest.mark.parametrize("layout", sorted(CHAIN))
@pytest.mark.parametrize("block", (PROLOGUE,) + STAGES)
def test_fp64_census_is_that_of_the_parent_commit(text, layout, block):
    got = census(blocks(text, CHAIN[layout])[block])
    assert got == PARENT_CENSUS[block], (layout, block, {k: (got.get(k, 0), PARENT_CENSUS[block].get(k, 0))
                                                        for k in sorted(set(got) | set(PARENT_CENSUS[block]))
                                                        if got.get(k, 0) != PARENT_CENSUS[block].get(k, 0)})
