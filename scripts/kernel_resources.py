"""Per-kernel resource usage of a built libk3m_hip.so, read from the code object's metadata: VGPRs, AGPRs, SGPRs,
scratch (private segment) bytes, static LDS bytes, spilled registers.  With two libraries: the kernels of the first
whose figures differ in the second, and the kernels only one of them has (scripts/isa_stats.py counts scratch and MFMA
instructions in a ``hipcc -S`` listing; this reads what the loader is told, for every kernel of the library at once).

A template parameter added with a default (``bool SAVE = true``) changes a kernel's mangled name, not its code: names
are compared after ``normalize()`` drops such a trailing ``Lb1E`` argument, so an instantiation that existed before
lines up with itself.

usage: python scripts/kernel_resources.py LIB [OTHER_LIB] [name-regex]
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("K3M_LLVM_BIN", "/opt/rocm/llvm/bin")
FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size",
          ".vgpr_spill_count", ".sgpr_spill_count")


def code_objects(lib, tmp):
    """The gfx950 code objects of a host library: its .hip_fatbin section holds one offload bundle per translation
    unit, each unbundled on its own."""
    fat = os.path.join(tmp, "fat.bin")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat],
                   check=True)
    blob = open(fat, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    starts = [m.start() for m in re.finditer(re.escape(magic), blob)]
    outs = []
    for i, st in enumerate(starts):
        part = os.path.join(tmp, "bundle%d.bin" % i)
        open(part, "wb").write(blob[st:starts[i + 1] if i + 1 < len(starts) else len(blob)])
        out = os.path.join(tmp, "dev%d.co" % i)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + part,
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + out], check=True)
        outs.append(out)
    return outs


def resources(lib):
    txt = ""
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(lib, tmp):
            txt += subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True,
                                  text=True).stdout
    res = {}
    for blk in re.split(r"\n\s*- \.agpr_count:", txt)[1:]:
        blk = ".agpr_count:" + blk
        name = re.search(r"\.name:\s+(\S+)", blk)
        if not name:
            continue
        vals = []
        for f in FIELDS:
            m = re.search(re.escape(f) + r":\s+(\d+)", blk)
            vals.append(int(m.group(1)) if m else 0)
        res[name.group(1)] = tuple(vals)
    return res


def normalize(name):
    """Drop trailing ``true`` template arguments (a defaulted ``bool SAVE = true`` added to an existing kernel)."""
    while True:
        n = re.sub(r"Lb1EEE?v", lambda m: m.group(0).replace("Lb1E", "", 1), name, count=1)
        if n == name:
            return name
        name = n


def main(argv):
    libs = [a for a in argv if os.path.exists(a)]
    pat = next((a for a in argv if not os.path.exists(a)), ".")
    a = {normalize(k): v for k, v in resources(libs[0]).items() if re.search(pat, k)}
    if len(libs) == 1:
        print("%-6s %-6s %-6s %-8s %-8s %-6s %-6s  kernel" % ("vgpr", "agpr", "sgpr", "scratch", "lds", "vspill", "sspill"))
        for k, v in sorted(a.items()):
            print("%-6d %-6d %-6d %-8d %-8d %-6d %-6d  %s" % (v + (k,)))
        return 0
    b = {normalize(k): v for k, v in resources(libs[1]).items() if re.search(pat, k)}
    changed = [(k, a[k], b[k]) for k in sorted(a) if k in b and a[k] != b[k]]
    print("%d kernels in %s, %d in %s; %d in both, %d of them with different figures; %d only in the first, %d only in "
          "the second" % (len(a), libs[0], len(b), libs[1], len(set(a) & set(b)), len(changed), len(set(a) - set(b)),
                          len(set(b) - set(a))))
    for k, x, y in changed:
        print("changed", k, dict(zip(FIELDS, x)), "->", dict(zip(FIELDS, y)))
    for k in sorted(set(a) - set(b)):
        print("only in the first", k)
    new = sorted(set(b) - set(a))
    print("only in the second: %d kernels; worst of them: vgpr %d, scratch %d B, spilled vgprs %d" % (
        len(new), max((b[k][0] for k in new), default=0), max((b[k][3] for k in new), default=0),
        max((b[k][5] for k in new), default=0)))
    return 1 if changed or set(a) - set(b) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
