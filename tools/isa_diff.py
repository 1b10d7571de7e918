#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 machine code of two builds (a refactor's proof that the shipped code did not change).

    python tools/isa_diff.py OLD NEW [--rename REGEX REPLACEMENT]

OLD / NEW: a HIP object file or shared library each (marl_api.o, marl_rk4_small.o, libmarl_hip.so: the first code object).  Kernels
are paired by mangled name, after `--rename` has been applied to OLD's names (a template parameter that the refactor removed).  A pair
is identical when the (opcode, operand text) sequences, the branch targets as offsets from the function start, and the amdhsa resource
records (VGPR, SGPR, scratch, LDS, spills) all agree; the pc-relative distance to a global is masked (it moves with the code around it).
Prints one line per kernel - name, instruction count, identical yes/no - then the kernels only one build has, and the first differing
instructions of every pair that differs.  Exit code 0 = same set, all identical.  (The resource records are read as
tests/test_kernel_resources.py reads them, but from any object file, with the spill counts.)
"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_stream_isa import LLVM, disassemble_so, functions  # noqa: E402

FIELDS = r"private_segment_fixed_size|group_segment_fixed_size|vgpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count|agpr_count"


def records(path):
    """mangled kernel name -> amdhsa resource record of the gfx950 code object in `path`"""
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "dev.co")
        subprocess.run([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", path], check=True)
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        f"--output={co}"], check=True)
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    recs = {}
    for blk in re.split(r"\n\s*- (?=\.agpr_count:)", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if name:
            recs[name.group(1)] = {k: int(v) for k, v in re.findall(rf"\.({FIELDS}):\s+(\d+)", blk)}
    return recs


def load(path, rename=None):
    """name -> ([(opcode, operands, branch offset or None)], resource record or None)"""
    fns, recs = functions(disassemble_so(path), ""), records(path)
    out = {}
    for name, ins in fns.items():
        start = ins[0][0] if ins else 0
        key = re.sub(rename[0], rename[1], name) if rename else name
        assert key not in out, f"{path}: two kernels are named {key} after renaming"
        body = []
        for k, (_a, op, args, tgt) in enumerate(ins):
            # `s_getpc_b64 s[n:n+1]; s_add_u32 sn, sn, literal`: the literal is the distance to a global (the log / exp tables), which moves
            # with the size of every function in front of it - not a property of this kernel
            if op == "s_add_u32" and k > 0 and ins[k - 1][1] == "s_getpc_b64" and re.match(r"s\d+, s\d+, 0x[0-9a-f]+\s*$", args):
                args = re.sub(r"0x[0-9a-f]+\s*$", "<pc-relative>", args)
            body.append((op, args.strip(), None if tgt is None else tgt - start))
        out[key] = (body, recs.get(name))
    return out


def main(argv):
    rename = None
    if "--rename" in argv:
        i = argv.index("--rename")
        rename = (argv[i + 1], argv[i + 2])
        argv = argv[:i] + argv[i + 3:]
    old, new = load(argv[1], rename), load(argv[2])
    print(f"# old: {os.path.basename(argv[1])} ({len(old)} functions)   new: {os.path.basename(argv[2])} ({len(new)} functions)")
    if rename:
        print(f"# old names renamed: s/{rename[0]}/{rename[1]}/")
    bad = []
    for name in sorted(set(old) & set(new)):
        (oi, orec), (ni, nrec) = old[name], new[name]
        same = oi == ni and orec == nrec
        print(f"{name}  {len(ni)}  {'yes' if same else 'NO'}")
        if not same:
            bad.append(name)
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    print(f"# paired {len(set(old) & set(new))}, identical {len(set(old) & set(new)) - len(bad)}, only in old {len(only_old)}, only in new {len(only_new)}")
    for name in only_old:
        print(f"# only in old: {name}")
    for name in only_new:
        print(f"# only in new: {name}")
    for name in bad:
        (oi, orec), (ni, nrec) = old[name], new[name]
        print(f"# --- {name}: {len(oi)} -> {len(ni)} instructions, records {orec} -> {nrec}")
        shown = 0
        for k in range(max(len(oi), len(ni))):
            a, b = (oi[k] if k < len(oi) else None), (ni[k] if k < len(ni) else None)
            if a != b and shown < 20:
                print(f"#   [{k}] {a}  ->  {b}")
                shown += 1
    return 1 if bad or only_old or only_new else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
