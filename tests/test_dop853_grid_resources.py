"""Build-time resource records of the large-grid DOP853 kernels (csrc/marl_dop853_grid.h), read from the code object that ships (CPU
suite): the amdhsa metadata of libmarl_hip.so, as tests/test_dop853_resources.py reads it - from the translation unit that holds
dop853_grid_stage_kernel and from none of the others.

What is pinned:
  * exactly the shipped instantiations are there: the stage kernel for both layouts and both porosity-diffusion variants, the dense
    kernel for both layouts (it evaluates nothing, so it has no dPhi_variable variant), one reduction and one control kernel - and no
    dop853_sweep* kernel: the one-workgroup kernels stay in the units of their own;
  * no scratch in the stage and dense kernels: a 256-thread workgroup may use 512 VGPRs per lane, and nothing of a stage's 12 x 5
    derivatives is held across the evaluation;
  * VGPRs and LDS as DESIGN.md (section 5.10) records them from this build - not allowed to grow."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from check_stream_isa import DEFAULT_SO, LLVM  # noqa: E402

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FIELDS = r"private_segment_fixed_size|group_segment_fixed_size|vgpr_count|sgpr_count|vgpr_spill_count"

# kernel (as it appears in the mangled name): (VGPRs, LDS bytes) - as the compiler reports them for this build
STAGE = {"dop853_grid_stage_kernelILi0ELb0E": (95, 23584), "dop853_grid_stage_kernelILi0ELb1E": (95, 23584),
         "dop853_grid_stage_kernelILi1ELb0E": (101, 23584), "dop853_grid_stage_kernelILi1ELb1E": (101, 23584)}
DENSE = {"dop853_grid_dense_kernelILi0EE": (70, 19456), "dop853_grid_dense_kernelILi1EE": (80, 19456)}
PLAIN = {"dop853_grid_reduce_kernel": (44, 16416), "dop853_grid_control_kernel": (94, 32832)}


def grid_records():
    """mangled kernel name -> resource record, for the DOP853 kernels of the unit whose code object holds dop853_grid_stage_kernel"""
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.run([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", DEFAULT_SO], check=True)
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
        for i, a in enumerate(starts):
            one, co = os.path.join(d, f"bundle{i}.bin"), os.path.join(d, f"dev{i}.co")
            with open(one, "wb") as f:
                f.write(blob[a:starts[i + 1] if i + 1 < len(starts) else len(blob)])
            subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={one}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                            f"--output={co}"], check=True)
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
            if "dop853_grid_stage_kernel" not in notes:
                continue
            recs = {}
            for blk in re.split(r"\n\s*- (?=\.agpr_count:)", notes)[1:]:
                name = re.search(r"\.name:\s+(\S+)", blk)
                if name and "dop853" in name.group(1).replace("marl_dop853_grid", ""):      # (the unit's namespace names the method too)
                    recs[name.group(1)] = {k: int(v) for k, v in re.findall(rf"\.({FIELDS}):\s+(\d+)", blk)}
            return recs
    return {}


@pytest.fixture(scope="module")
def recs():
    if not os.path.exists(DEFAULT_SO):
        pytest.skip("libmarl_hip.so has not been built")
    r = grid_records()
    assert r, "no code object of libmarl_hip.so holds the large-grid DOP853 kernels"
    return r


def _one(recs, key):
    hits = {n: r for n, r in recs.items() if key in n}
    assert len(hits) == 1, (key, sorted(recs))
    return next(iter(hits.items()))


def test_every_shipped_instantiation_is_there_and_nothing_else(recs):
    assert len(recs) == len(STAGE) + len(DENSE) + len(PLAIN), sorted(recs)
    for key in (*STAGE, *DENSE, *PLAIN):
        _one(recs, key)
    assert not any("dop853_sweep" in n for n in recs), sorted(recs)


@pytest.mark.parametrize("key", [*STAGE, *DENSE, *PLAIN])
def test_registers_scratch_and_lds_are_what_design_md_records(recs, key):
    vgprs, lds = {**STAGE, **DENSE, **PLAIN}[key]
    name, r = _one(recs, key)
    print(f"DOP853 grid {key}: {r}")
    assert r["vgpr_count"] <= min(vgprs, 512), (name, r)
    assert r["group_segment_fixed_size"] == lds, (name, r)
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, (name, r)
