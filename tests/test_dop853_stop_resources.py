"""Build-time resource records of the DOP853 kernel that stops at a terminal monitor's root (dop853_sweep_stop_kernel, csrc/marl_dop853.h,
unit csrc/marl_dop853_stop.hip), read from the code object that ships (CPU suite) as tests/test_dop853_resources.py reads those of the three
older kernels - from the unit that holds this kernel, and from no other.

What is pinned, per window and porosity-diffusion variant:
  * exactly the six instantiations <256 | 512 | 1024, 0 | 1> and no other DOP853 kernel: the three older kernels stay in their own unit;
  * the VGPR cap the shape implies (512 / 256 / 128 at 256 / 512 / 1024 threads);
  * LDS and scratch as DESIGN.md (section "DOP853") records them from this build - not allowed to grow.  The LDS is that of the roots
    kernel plus the 192 bytes of the stop record (Dop853Stop).
"""
import os
import re
import subprocess
import tempfile

import pytest

from test_dop853_resources import DEFAULT_SO, FIELDS, LLVM, MAGIC

# window: (VGPR cap of the shape, LDS bytes, scratch bytes [dPhi constant, dPhi_variable]) - as the compiler reports them for this build
RECORDED = {256: (512, 24432, (80, 80)), 512: (256, 44944, (80, 80)), 1024: (128, 85960, (112, 112))}
KERNEL = "dop853_sweep_stop_kernel"
STOP_RECORD_BYTES = 192
ROOTS_KERNEL_LDS = {256: 24240, 512: 44752, 1024: 85768}      # tests/test_dop853_resources.py


def stop_records():
    """mangled kernel name -> resource record, for the DOP853 kernels of the unit whose code object holds dop853_sweep_stop_kernel"""
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
            if KERNEL not in notes:
                continue
            recs = {}
            for blk in re.split(r"\n\s*- (?=\.agpr_count:)", notes)[1:]:
                name = re.search(r"\.name:\s+(\S+)", blk)
                if name and "dop853" in re.sub(r"^_ZN\d+marl_dop853_stop", "", name.group(1)):      # (the unit's namespace is not a kernel name)
                    recs[name.group(1)] = {k: int(v) for k, v in re.findall(rf"\.({FIELDS}):\s+(\d+)", blk)}
            return recs
    return {}


@pytest.fixture(scope="module")
def recs():
    if not os.path.exists(DEFAULT_SO):
        pytest.skip("libmarl_hip.so has not been built")
    r = stop_records()
    assert r, "no code object of libmarl_hip.so holds dop853_sweep_stop_kernel"
    return r


def test_the_six_instantiations_are_there_and_nothing_else(recs):
    want = {f"{KERNEL}ILi{blk}ELb{vd}E" for blk in RECORDED for vd in (0, 1)}
    got = {re.search(r"\d+(dop853_\w+?ILi\d+ELb[01]E)", re.sub(r"^_ZN\d+marl_dop853_stop", "", name)).group(1) for name in recs if "_kernelI" in name}
    assert got == want and len(recs) == 6, sorted(recs)


@pytest.mark.parametrize("blk", sorted(RECORDED))
def test_registers_scratch_and_lds_are_what_design_md_records(recs, blk):
    cap, lds, scratch = RECORDED[blk]
    assert lds == ROOTS_KERNEL_LDS[blk] + STOP_RECORD_BYTES
    for vd in (0, 1):
        hits = {n: r for n, r in recs.items() if f"{KERNEL}ILi{blk}ELb{vd}E" in n}
        assert len(hits) == 1, (blk, vd)
        (name, r), = hits.items()
        print(f"DOP853 {KERNEL}<{blk}, {bool(vd)}>: {r}")
        assert r["vgpr_count"] <= cap, (name, r)
        assert r["group_segment_fixed_size"] <= lds, (name, r)
        assert r["private_segment_fixed_size"] <= scratch[vd], (name, r)
