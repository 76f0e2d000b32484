#!/usr/bin/env python3
"""kcompare.py OLD_OBJDIR NEW_OBJDIR [OBJ ...]: the gfx950 kernels of two builds
of the step objects, side by side (tools/kmeta.sh's metadata plus a hash of each
kernel's code bytes). Kernels are matched by name; a bool template pack of the
old build (positional, before the form words of csrc/mg_forms.h) is first
rewritten as its form word. Prints one line per kernel and a verdict per
object; exit status 1 when a kernel is missing, extra or differs."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
OBJS = ["mg_rigid", "mg_env", "mg_env_sens", "mg_env_crep", "mg_env_jfr", "mg_chain", "mg_pile"]
# kernel -> (positions of the leading integer parameters kept, (position, bit) of each bool, trailing integers kept)
PACKS = {
    "k_rigid_step1": ([], [(0, 1), (1, 2), (2, 4), (3, 8), (4, 16), (5, 32), (6, 64)], []),
    "k_rigid_step": ([], [(0, 1), (3, 8), (4, 32)], [1, 2]),
    "k_artic_chain_q": ([0], [(1, 1), (2, 2), (3, 8)], []),
    "k_artic_chain": ([0], [(1, 1), (2, 2), (3, 4), (4, 8)], []),
    "k_env_step": ([0, 1], [(2, 1), (3, 2), (4, 4), (5, 8), (6, 16)], []),
    "k_artic_lanes": ([0, 1], [(2, 1), (3, 2), (4, 4)], []),
    "k_pile_step": ([], [(0, 1)], []),
}


def canon(name):
    m = re.search(r"(\w+)<(.*)>\(", name)
    if not m:
        return name
    k, args = m.group(1), [a.strip() for a in m.group(2).split(",")]
    if k in PACKS and any(a in ("true", "false") for i, a in enumerate(args) if (k, i) != ("k_rigid_step", 2)):
        lead, bits, trail = PACKS[k]
        f = sum(b for i, b in bits if args[i] == "true")
        args = [args[i] for i in lead] + ["%du" % f] + [args[i] for i in trail]
    return "%s<%s>" % (k, ", ".join(args))


def kernels(obj):
    with tempfile.TemporaryDirectory() as t:
        fb, elf = os.path.join(t, "fb.bin"), os.path.join(t, "dev.elf")
        subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fb])
        subprocess.check_call([LLVM + "/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fb,
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + elf])
        out = subprocess.check_output([LLVM + "/llvm-readelf", "-S", "-s", "-W", "--notes", elf], text=True)
        data = open(elf, "rb").read()
    sec = re.search(r"\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)", out)
    addr, off = int(sec.group(1), 16), int(sec.group(2), 16)
    code = {}
    for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+FUNC\s+\w+\s+\w+\s+\d+\s+(\S+)$", out, re.M):
        a, n = int(m.group(1), 16), int(m.group(2))
        h = hashlib.sha256(data[off + a - addr:off + a - addr + n]).hexdigest()[:16]
        assert code.setdefault(m.group(3), (n, h)) == (n, h)   # listed twice (.symtab, .dynsym): the same bytes
    res = {}
    fields = ["vgpr_count", "agpr_count", "private_segment_fixed_size", "vgpr_spill_count", "group_segment_fixed_size"]
    for blk in re.split(r"\n\s+- \.agpr_count:", out)[1:]:
        blk = ".agpr_count:" + blk
        sym = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta = tuple(int(re.search(r"\.%s:\s+(\d+)" % f, blk).group(1)) for f in fields)
        res[sym] = meta + code[sym]
    names = subprocess.check_output(["c++filt"] + list(res), text=True).split("\n")
    return {canon(n): v for n, v in zip(names, res.values())}


def main():
    old_dir, new_dir = sys.argv[1:3]
    bad = 0
    print("# object kernel | vgpr agpr scratch spills lds code_bytes sha256[:16] | verdict")
    total = 0
    for o in sys.argv[3:] or OBJS:
        a, b = kernels("%s/%s.hip.o" % (old_dir, o)), kernels("%s/%s.hip.o" % (new_dir, o))
        total += len(b)
        for k in sorted(set(a) | set(b)):
            v = "same" if a.get(k) == b.get(k) else "only old" if k not in b else "only new" if k not in a else \
                "META DIFFERS" if a[k][:5] != b[k][:5] else "code differs"
            bad += v != "same"
            x = b.get(k) or a[k]
            print("%s %s | %s | %s" % (o, k, " ".join(str(f) for f in x), v))
            if v not in ("same", "only old", "only new"):
                print("%s %s | %s | (old)" % (o, k, " ".join(str(f) for f in a[k])))
        print("# %s: %d kernels old, %d new" % (o, len(a), len(b)))
    print("# total %d kernels, %d not the same" % (total, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
