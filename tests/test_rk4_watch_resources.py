"""Build-time resource records of the monitored fixed-step RK4 kernel (csrc/marl_rk4_watch.h), read from the code object that ships (CPU
suite): the amdhsa metadata of libmarl_hip.so, as tests/test_dop853_resources.py reads it - from the translation unit that holds
rk4_watch_kernel and from none of the others.

What is pinned:
  * exactly the six shipped instantiations are there: windows of 256 / 512 / 1024 threads, constant and variable porosity diffusion;
  * VGPRs within what a workgroup of that size may use per lane (512 / 256 / 128);
  * LDS and scratch as DESIGN.md (section 5.11) records them from this build - not allowed to grow: LDS is rk4_sweep_kernel's plus the
    eight monitor columns (64 B per thread), the reduced record, the instance's record and the decision words (240 B), within the
    160 KB of a compute unit at 1024 threads; scratch only at 1024 threads, where the plain kernel's dPhi_variable variant
    spills too."""
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

# instantiation (as it appears in the mangled name): (VGPR limit of the window, LDS bytes, scratch bytes) - the last two as the compiler
# reports them for this build
WATCH = {"rk4_watch_kernelILi256ELb0E": (512, 40176, 0), "rk4_watch_kernelILi256ELb1E": (512, 40176, 0),
         "rk4_watch_kernelILi512ELb0E": (256, 77040, 0), "rk4_watch_kernelILi512ELb1E": (256, 77040, 0),
         "rk4_watch_kernelILi1024ELb0E": (128, 150768, 12), "rk4_watch_kernelILi1024ELb1E": (128, 150768, 44)}


def watch_records():
    """mangled kernel name -> resource record, for the rk4_watch kernels of the unit whose code object holds them"""
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.run([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", DEFAULT_SO], check=True)
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
        found = {}
        for i, a in enumerate(starts):
            one, co = os.path.join(d, f"bundle{i}.bin"), os.path.join(d, f"dev{i}.co")
            with open(one, "wb") as f:
                f.write(blob[a:starts[i + 1] if i + 1 < len(starts) else len(blob)])
            subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={one}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                            f"--output={co}"], check=True)
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
            for blk in re.split(r"\n\s*- (?=\.agpr_count:)", notes)[1:]:
                name = re.search(r"\.name:\s+(\S+)", blk)
                if name and "rk4_watch_kernel" in name.group(1):
                    assert name.group(1) not in found, f"{name.group(1)} is in two code objects"
                    found[name.group(1)] = (i, {k: int(v) for k, v in re.findall(rf"\.({FIELDS}):\s+(\d+)", blk)})
        return found


@pytest.fixture(scope="module")
def recs():
    if not os.path.exists(DEFAULT_SO):
        pytest.skip("libmarl_hip.so has not been built")
    r = watch_records()
    assert r, "no code object of libmarl_hip.so holds rk4_watch_kernel"
    return r


def _one(recs, key):
    hits = {n: r for n, r in recs.items() if key in n}
    assert len(hits) == 1, (key, sorted(recs))
    return next(iter(hits.items()))


def test_the_six_instantiations_live_in_one_unit_of_their_own(recs):
    assert len(recs) == len(WATCH), sorted(recs)
    for key in WATCH:
        _one(recs, key)
    assert len({unit for unit, _ in recs.values()}) == 1
    assert all("marl_rk4w" in n for n in recs), sorted(recs)          # the unit's own namespace: no other unit instantiates the kernel


@pytest.mark.parametrize("key", list(WATCH))
def test_registers_lds_and_scratch_are_what_design_md_records(recs, key):
    vgpr_limit, lds, scratch = WATCH[key]
    name, (_, r) = _one(recs, key)
    print(f"rk4 watch {key}: {r}")
    assert r["vgpr_count"] <= vgpr_limit, (name, r)
    assert r["group_segment_fixed_size"] == lds, (name, r)
    assert r["private_segment_fixed_size"] == scratch, (name, r)
