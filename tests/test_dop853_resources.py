"""Build-time resource records of the DOP853 kernels (csrc/marl_dop853.h), read from the code object that ships (CPU suite): the amdhsa
metadata of libmarl_hip.so, as tests/test_kernel_resources.py reads it - but from the translation unit that holds these kernels (the
library's fat binary carries one code object per unit; this file looks at none of the others).

What is pinned, per window and porosity-diffusion variant, for the plain, eval and roots kernels:
  * the VGPR cap the shape implies (a SIMD's 512 registers over the waves of one workgroup: 512 / 256 / 128 at 256 / 512 / 1024 threads);
  * scratch and LDS as DESIGN.md (section "DOP853") records them from this build - not allowed to grow.  The scratch is the reduced
    record handed to the controller function and that function's frame (thread 0's business, outside the stage loop): the stage
    derivatives live in a global arena, so no window spills them.
"""
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

# window: (VGPR cap of the shape, LDS bytes, scratch bytes [dPhi constant, dPhi_variable]) - as the compiler reports them for this build
RECORDED = {256: (512, 24240, (80, 80)), 512: (256, 44752, (80, 80)), 1024: (128, 85768, (96, 112))}
KERNELS = ("dop853_sweep_kernel", "dop853_sweep_eval_kernel", "dop853_sweep_roots_kernel")


def dop853_records():
    """mangled kernel name -> resource record, for the kernels of the unit whose code object holds dop853_sweep_kernel"""
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
            if "dop853_sweep_kernel" not in notes:
                continue
            recs = {}
            for blk in re.split(r"\n\s*- (?=\.agpr_count:)", notes)[1:]:
                name = re.search(r"\.name:\s+(\S+)", blk)
                if name and "dop853" in name.group(1):
                    recs[name.group(1)] = {k: int(v) for k, v in re.findall(rf"\.({FIELDS}):\s+(\d+)", blk)}
            return recs
    return {}


@pytest.fixture(scope="module")
def recs():
    if not os.path.exists(DEFAULT_SO):
        pytest.skip("libmarl_hip.so has not been built")
    r = dop853_records()
    assert r, "no code object of libmarl_hip.so holds the DOP853 kernels"
    return r


def test_every_shipped_instantiation_is_there_and_nothing_else(recs):
    want = {f"{k}ILi{blk}ELb{vd}E" for k in KERNELS for blk in RECORDED for vd in (0, 1)}
    got = {re.search(r"(dop853_\w+?ILi\d+ELb[01]E)", name).group(1) for name in recs if "_kernelI" in name}
    assert got == want and len([n for n in recs if "_kernelI" in n]) == 18, sorted(recs)


@pytest.mark.parametrize("blk", sorted(RECORDED))
def test_registers_scratch_and_lds_are_what_design_md_records(recs, blk):
    cap, lds, scratch = RECORDED[blk]
    for kernel in KERNELS:
        for vd in (0, 1):
            hits = {n: r for n, r in recs.items() if f"{kernel}ILi{blk}ELb{vd}E" in n}
            assert len(hits) == 1, (kernel, blk, vd)
            (name, r), = hits.items()
            print(f"DOP853 {kernel}<{blk}, {bool(vd)}>: {r}")
            assert r["vgpr_count"] <= cap, (name, r)
            assert r["group_segment_fixed_size"] == lds, (name, r)
            assert r["private_segment_fixed_size"] <= scratch[vd], (name, r)
