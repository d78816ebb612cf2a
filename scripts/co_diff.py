#!/usr/bin/env python3
"""scripts/co_diff.py A.so B.so: do two builds of the library (scripts/ab_build.sh) hold the same device code?  Unbundles the
gfx950 code objects of each (one per translation unit) and compares, kernel by kernel whatever their order in the file: the set of kernel symbols, the
code size of each and its resource metadata (VGPRs, AGPRs, SGPRs, spills, LDS, scratch, kernarg size, workgroup size).
Prints the differences and one summary line; exit status 1 if there are any.  A host-only change must print none."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size",
          "private_segment_fixed_size", "kernarg_segment_size", "max_flat_workgroup_size", "uses_dynamic_stack")


def kernels(lib, tmp):
    """{kernel symbol: {"size": code bytes, field: value}} of the gfx950 code object in `lib`"""
    fat = os.path.join(tmp, "fatbin")
    subprocess.check_call([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, fat])
    # one bundle per translation unit of the library, side by side in the section
    blob = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), blob)]
    out = {}
    for k, a in enumerate(starts):
        part, co = os.path.join(tmp, f"fatbin{k}"), os.path.join(tmp, f"co{k}")
        with open(part, "wb") as f:
            f.write(blob[a:starts[k + 1] if k + 1 < len(starts) else len(blob)])
        subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                               f"--input={part}", f"--output={co}", "--unbundle"])
        out.update(code_object(co))
    return out


def code_object(co):
    """{kernel symbol: ...} of one unbundled code object"""
    out = {}
    entry = None
    for line in subprocess.check_output([f"{LLVM}/llvm-readelf", "--notes", co], text=True).splitlines():
        if line.startswith("  - ."):                       # a new element of amdhsa.kernels
            entry = {}
        m = re.match(r"^  [- ] \.(\w+):\s+(\S+)$", line)
        if entry is not None and m:
            if m.group(1) == "name":
                out[m.group(2)] = entry
            elif m.group(1) in FIELDS:
                entry[m.group(1)] = m.group(2)
    for line in subprocess.check_output([f"{LLVM}/llvm-readelf", "-sW", co], text=True).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC" and f[7] in out:
            out[f[7]]["size"] = f[2]
    return out


def main(a, b):
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        ka, kb = kernels(a, ta), kernels(b, tb)
    diffs = [f"only in {a}: {k}" for k in sorted(ka.keys() - kb.keys())] + [f"only in {b}: {k}" for k in sorted(kb.keys() - ka.keys())]
    diffs += [f"{k}: {ka[k]} != {kb[k]}" for k in sorted(ka.keys() & kb.keys()) if ka[k] != kb[k]]
    print("\n".join(diffs + [f"{len(ka)} / {len(kb)} kernels, {len(diffs)} differences in symbols, code sizes and resources"]))
    return 1 if diffs else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
