#!/usr/bin/env python3
"""Compare the gfx950 code of two builds of libvdf_hip.so's objects, kernel by kernel (CPU only; no GPU is touched).

  tools/compare_device_code.py <build dir A> <build dir B> [--new TEXT ...]
                                                                 e.g. a checkout of the parent's vdf_amd/csrc/build and this one's

--new TEXT: a change that ADDS a kernel names it here; symbols whose name contains TEXT and that only B has are listed as new
and are no difference (every symbol both sides have is compared as always).

For each of abi, msm, msm_direct, vecops, snark, minroot, rounds (a unit one side has no object of is skipped): the device code object is taken out of the .o, and the two sides are
compared by (1) the set of kernel names, (2) each kernel's register, scratch, LDS and spill figures from the code object's
notes, (3) each kernel's disassembly.  A host-only change (a launcher refactor) must leave all three identical.
Exit status 1 when anything differs."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
UNITS = ("abi", "msm", "msm_direct", "vecops", "snark", "minroot", "rounds")
FIGURES = (".vgpr_count", ".sgpr_count", ".agpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size",
           ".vgpr_spill_count", ".sgpr_spill_count")


def tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name), *args], check=True, capture_output=True, text=True).stdout


def code_object(obj, tmp, tag):
    """The gfx950 code object inside a host object, or None when the object holds no device code."""
    fat, co = os.path.join(tmp, tag + ".fat"), os.path.join(tmp, tag + ".co")
    if ".hip_fatbin" not in tool("llvm-readelf", "-S", obj):
        return None
    tool("llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, obj)
    tool("clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fat, "--targets=" + TARGET, "--output=" + co)
    return co if os.path.getsize(co) else None


def kernels(co):
    """name -> {figure: value} from the AMDGPU metadata note (one record per kernel under amdhsa.kernels)."""
    out, cur = {}, None
    for line in tool("llvm-readelf", "--notes", co).splitlines():
        m = re.match(r"^(  - |    )(\.[a-z_]+):\s*(.*)$", line)       # a kernel's own keys; its arguments' sit deeper
        if not m:
            continue
        if m.group(1) == "  - ":
            cur = {}
        if cur is None:
            continue
        cur[m.group(2)] = m.group(3).strip().strip("'")
        if m.group(2) == ".name":
            out[cur[".name"]] = cur
    return out


def symbols(co):
    """Sorted (address, size, name) of the code object's functions and data objects."""
    out = []
    for line in tool("llvm-readelf", "-sW", co).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] in ("FUNC", "OBJECT") and f[6] != "UND":
            out.append((int(f[1], 16), int(f[2]), f[7]))
    return sorted(out)


def disassembly(co):
    """symbol -> hash of its instructions.  Addresses and encodings are left out, and so is the one thing in an instruction
    that depends on where the linker put OTHER symbols: the 32-bit displacement a kernel adds to s_getpc_b64 to reach an
    out-of-line function or a constant table.  It is replaced by the name (+ offset) of what it reaches, so that two code
    objects whose kernels only sit in another order compare equal, and a call that reaches something else does not."""
    syms = symbols(co)

    def name_of(addr):
        for a, size, n in syms:
            if a <= addr < a + max(size, 1):
                return f"{n}+{addr - a:#x}"
        return f"?{addr:#x}"

    out, name, lines, pc = {}, None, [], {}

    def flush():
        if name:
            out[name] = hashlib.sha256("\n".join(lines).encode()).hexdigest()

    for line in tool("llvm-objdump", "-d", co).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            flush()
            name, lines, pc = m.group(1), [], {}
            continue
        m = re.match(r"^\t(.*?)\s*// ([0-9A-F]+):", line)
        if not name or not m:
            continue
        ins, addr = m.group(1), int(m.group(2), 16)
        g = re.match(r"s_getpc_b64 s\[(\d+):\d+\]$", ins)
        a = re.match(r"s_add_u32 s(\d+), s(\d+), (0x[0-9a-f]+|-?\d+)$", ins)
        c = re.match(r"s_addc_u32 s(\d+), s(\d+), (0x[0-9a-f]+|-?\d+)$", ins)
        if g:
            pc[int(g.group(1))] = addr + 4
        elif a and a.group(1) == a.group(2) and int(a.group(1)) in pc:
            lo = int(a.group(1))
            ins = f"s_add_u32 s{lo}, s{lo}, lo({name_of((pc.pop(lo) + int(a.group(3), 0)) & 0xffffffff)})"
            pc[("hi", lo + 1)] = True
        elif c and c.group(1) == c.group(2) and ("hi", int(c.group(1))) in pc:
            del pc[("hi", int(c.group(1)))]
            ins = f"s_addc_u32 s{c.group(1)}, s{c.group(1)}, hi"
        lines.append(ins)
    flush()
    return out


def main():
    args, new = sys.argv[1:], []
    while "--new" in args:
        k = args.index("--new")
        if k + 1 >= len(args):
            sys.exit(__doc__)
        new.append(args[k + 1])
        del args[k:k + 2]
    if len(args) != 2:
        sys.exit(__doc__)
    a_dir, b_dir = args
    is_new = lambda n, a_side: n not in a_side and any(t in n for t in new)
    bad = False
    with tempfile.TemporaryDirectory() as tmp:
        for unit in UNITS:
            if not os.path.exists(os.path.join(a_dir, unit + ".o")) or not os.path.exists(os.path.join(b_dir, unit + ".o")):
                print(f"{unit}: no object on one side, skipped")
                continue
            a = code_object(os.path.join(a_dir, unit + ".o"), tmp, unit + "_a")
            b = code_object(os.path.join(b_dir, unit + ".o"), tmp, unit + "_b")
            if a is None and b is None:
                print(f"{unit}: no device code on either side")
                continue
            if a is None or b is None:
                print(f"{unit}: device code on one side only")
                bad = True
                continue
            same_file = open(a, "rb").read() == open(b, "rb").read()
            ka, kb = kernels(a), kernels(b)
            da, db = disassembly(a), disassembly(b)
            diffs = [f"only in A: {n}" for n in sorted(set(ka) - set(kb))] + [f"only in B: {n}" for n in sorted(set(kb) - set(ka)) if not is_new(n, ka)]
            for n in sorted(set(ka) & set(kb)):
                fa = {f: ka[n].get(f) for f in FIGURES}
                fb = {f: kb[n].get(f) for f in FIGURES}
                if fa != fb:
                    diffs.append(f"resources differ: {n}: {fa} -> {fb}")
            for n in sorted(set(da) | set(db) | set(ka) | set(kb)):          # kernels and the functions they call
                if is_new(n, da) and is_new(n, ka):
                    print(f"   new in B: {n}")
                elif da.get(n) is None or da.get(n) != db.get(n):
                    diffs.append(f"instructions differ: {n}")
            print(f"{unit}: {len(ka)} kernels in A, {len(kb)} in B, " +
                  ("identical" if not diffs else f"{len(diffs)} differences") +
                  (" (code objects byte-identical)" if same_file else " (code objects differ as files)"))
            for d in diffs:
                print("   " + d)
            bad = bad or bool(diffs)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
