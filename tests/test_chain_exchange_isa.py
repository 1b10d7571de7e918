"""rk4_exchange_kernel - rk4_chain_kernel with the LDS exchange laid out by cell and the cache slots in pairs - on the code object that
ships (CPU suite).

The kernel differs from rk4_chain_kernel in LDS addresses only (csrc/marl_kernels.h, StencilBlock, XCH).  Checked here, for both
instantiations, <256, tiled, 4> and <256, field-major, 4>:

  * the invariants I1-I5 of the streamed loop (tools/check_stream_isa.py), nine s_barrier among them;
  * resources: at most 128 VGPRs, no more scratch than rk4_chain_kernel, at most 40 960 B of LDS (four workgroups per CU);
  * the fp64 opcode census of every barrier-to-barrier stage block is rk4_chain_kernel's of the same build and layout - no arithmetic
    moved, none was added or lost;
  * v_readlane + v_writelane per stage block: no more than rk4_chain_kernel;
  * the stage blocks hold ds_read_b128 and no two-address 64-bit LDS form with a stride (ds_read2st64_b64, ds_write2st64_b64: how the
    field-major exchange and the slot columns compile).  What is left of ds_read2_b64 / ds_write2_b64 (adjacent doubles) belongs to the seam
    record, five consecutive doubles written by one lane and read by one lane per evaluation, and is bounded by rk4_chain_kernel's count;
  * per stage block, the LDS cycles of its instructions, summed with the per-instruction costs of CDNA4 below, are fewer than in
    rk4_chain_kernel.

The blocks are those of tests/test_chain_window_isa.py: block 4 ends at the first exchange barrier, blocks 5-7 run from one exchange
barrier to the next, block 8 from the last one to the publish barrier.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from check_stream_isa import DEFAULT_SO, check_text, disassemble_so, functions  # noqa: E402
from test_chain_window_isa import census, lane_traffic  # noqa: E402

EXCHANGE = "rk4_exchange_kernel"
NEW = {"tiled": "rk4_exchange_kernelILi256ELi1ELi4ELi3EE", "field_major": "rk4_exchange_kernelILi256ELi0ELi4ELi3EE"}
OLD = {"tiled": "rk4_chain_kernelILi256ELi1ELi4EE", "field_major": "rk4_chain_kernelILi256ELi0ELi4EE"}
STAGE_BLOCKS = (4, 5, 6, 7, 8)

# LDS cycles per wave-instruction on CDNA4 (gfx950), conflict-free.  Reads: cycles of the LDS array - 64- and 128-bit reads move
# 256 B/clk, a two-address 64-bit read 128 B/clk.  Stores: the transfer of address and data registers to the LDS, which is longer than
# the array's part.  The st64 forms are taken to cost what the plain two-address forms cost.
LDS_CYCLES = {
    "ds_read_b32": 2, "ds_read_b64": 2, "ds_read_b128": 4, "ds_read2_b32": 4, "ds_read2st64_b32": 4, "ds_read2_b64": 8, "ds_read2st64_b64": 8,
    "ds_write_b32": 4, "ds_write_b64": 6, "ds_write2_b32": 6, "ds_write2st64_b32": 6, "ds_write_b128": 13, "ds_write2_b64": 13,
    "ds_write2st64_b64": 13,
}
STRIDED_PAIRS = ("ds_read2st64_b64", "ds_write2st64_b64")
ADJACENT_PAIRS = ("ds_read2_b64", "ds_write2_b64")


@pytest.fixture(scope="module")
def text():
    if not os.path.exists(DEFAULT_SO):
        pytest.skip("libmarl_hip.so has not been built")
    return disassemble_so(DEFAULT_SO)


def blocks(text, kern):
    """The kernel's opcodes, split at its s_barrier in address order."""
    fns = functions(text, kern)
    assert len(fns) == 1, (kern, sorted(fns))
    out = [[]]
    for _a, op, _o, _t in next(iter(fns.values())):
        if op == "s_barrier":
            out.append([])
        else:
            out[-1].append(op)
    assert len(out) == 10, (kern, len(out))   # nine barriers (I4)
    return out


def lds_cycles(ops):
    total = 0
    for op in ops:
        if op.startswith("ds_"):
            assert op in LDS_CYCLES, f"{op}: no cycle count on record"
            total += LDS_CYCLES[op]
    return total


def test_both_instantiations_keep_the_stream_invariants(text):
    res = check_text(text, pattern=EXCHANGE)
    assert sorted(res) == sorted(n for n in functions(text, EXCHANGE)) and len(res) == 2, sorted(res)
    assert all(any(key in name for name in res) for key in NEW.values()), sorted(res)
    assert {n: bad for n, bad in res.items() if bad} == {}   # (I4: exactly nine s_barrier)


def test_resources():
    from test_kernel_resources import kernel_records, pick
    if not os.path.exists(DEFAULT_SO):
        pytest.skip("libmarl_hip.so has not been built")
    recs = kernel_records()
    for layout in sorted(NEW):
        (name, new), = pick(recs, NEW[layout]).items()
        (_, old), = pick(recs, OLD[layout]).items()
        print(f"\n{layout}: {new} (rk4_chain_kernel: {old})")
        assert new["vgpr_count"] <= 128, (name, new)
        assert new["private_segment_fixed_size"] <= old["private_segment_fixed_size"], (name, new, old)
        assert new["group_segment_fixed_size"] <= 40960, (name, new)


@pytest.mark.parametrize("layout", sorted(NEW))
@pytest.mark.parametrize("block", STAGE_BLOCKS)
def test_fp64_census_is_that_of_the_chained_kernel(text, layout, block):
    got, want = census(blocks(text, NEW[layout])[block]), census(blocks(text, OLD[layout])[block])
    assert want and got == want, (layout, block, {k: (got.get(k, 0), want.get(k, 0)) for k in sorted(set(got) | set(want))
                                                  if got.get(k, 0) != want.get(k, 0)})


@pytest.mark.parametrize("layout", sorted(NEW))
@pytest.mark.parametrize("block", STAGE_BLOCKS)
def test_no_more_scalar_spill_traffic_than_the_chained_kernel(text, layout, block):
    new, old = lane_traffic(blocks(text, NEW[layout])[block]), lane_traffic(blocks(text, OLD[layout])[block])
    print(f"\n{layout} block {block}: v_readlane + v_writelane {new} (rk4_chain_kernel: {old})")
    assert new <= old, f"{layout}, block {block}: {new} v_readlane + v_writelane, rk4_chain_kernel has {old}"


@pytest.mark.parametrize("layout", sorted(NEW))
@pytest.mark.parametrize("block", STAGE_BLOCKS)
def test_wide_lds_forms_in_the_stage_blocks(text, layout, block):
    new, old = blocks(text, NEW[layout])[block], blocks(text, OLD[layout])[block]
    assert new.count("ds_read_b128") > old.count("ds_read_b128"), (layout, block, new.count("ds_read_b128"), old.count("ds_read_b128"))
    strided = {op: new.count(op) for op in STRIDED_PAIRS if new.count(op)}
    assert not strided, f"{layout}, block {block}: two-address 64-bit LDS accesses of the exchange or the cache slots: {strided}"
    assert any(old.count(op) for op in STRIDED_PAIRS), "rk4_chain_kernel no longer has them: this test compares against nothing"
    # the seam's accesses (adjacent doubles of one record) are all that is left of the two-address forms
    for op in ADJACENT_PAIRS:
        assert new.count(op) <= old.count(op), (layout, block, op, new.count(op), old.count(op))


@pytest.mark.parametrize("layout", sorted(NEW))
@pytest.mark.parametrize("block", STAGE_BLOCKS)
def test_fewer_lds_cycles_per_stage_block(text, layout, block):
    new, old = lds_cycles(blocks(text, NEW[layout])[block]), lds_cycles(blocks(text, OLD[layout])[block])
    print(f"\n{layout} block {block}: LDS cycles {new} (rk4_chain_kernel: {old})")
    assert new < old, f"{layout}, block {block}: {new} LDS cycles by the table, rk4_chain_kernel has {old}"
