"""Instruction counts of the kernels' marked stretches, from their gfx950 assembly.

Compiles cairo_amd/csrc/kernels.hip with the Makefile's flags plus
-DCAIRO_ASM_MARKS=1 (device only, -S; no GPU needed) and prints, for every
kernel that has marked stretches, its VGPR count, scratch, LDS, occupancy and
SGPR / VGPR spill counts and, per
stretch between a `cairo-mark <name> begin` and its `end`, the instructions by
class.  An instruction is classified by its mnemonic's prefix alone: `v_`
(VALU), `s_` (SALU; of those `s_cbranch` / `s_branch` are branches, `s_waitcnt`
waits, `s_load` / `s_buffer_load` scalar loads and `s_barrier` barriers),
`ds_` (LDS), `global_` / `buffer_` / `flat_` / `scratch_` (vector memory).

A stretch is counted straight through the text: cold blocks the compiler moved
elsewhere are not in it, and both sides of a branch inside it are.  The marks
are `asm volatile` comments: they keep their order among themselves, while the
compiler may still move an instruction across one, so a count is good to a few
instructions.
usage: python tools/asm_counts.py [--src PATH] [--asm FILE.s] [--kernel SUBSTR] [-DFOO=1 ...]
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-pthread", "-munsafe-fp-atomics"]

FUNC = re.compile(r"^(_Z\w+):\s*(;.*)?$")
END = re.compile(r"^\.Lfunc_end\d+:")
MARK = re.compile(r";\s*cairo-mark (\w+) (begin|end)")
INSN = re.compile(r"^\s+([a-z]\w*)\b")
KNAME = re.compile(r"^    \.name:\s+(\S+)")  # a kernel's entry in the code object's metadata
KSPILL = re.compile(r"^    \.(sgpr_spill_count|vgpr_spill_count):\s+(\d+)")
META = re.compile(r"^; (NumVgprs|NumAgprs|NumSgprs|ScratchSize|Occupancy|LDSByteSize|"
                  r"SGPRSpillCount|VGPRSpillCount|sgpr_spill_count|vgpr_spill_count): (\d+)")
# class by prefix, first match wins
CLASSES = (("branch", ("s_cbranch", "s_branch")), ("wait", ("s_waitcnt",)), ("barrier", ("s_barrier",)),
           ("smem", ("s_load", "s_buffer_load")), ("salu", ("s_",)), ("valu", ("v_",)), ("lds", ("ds_",)),
           ("vmem", ("global_", "buffer_", "flat_", "scratch_")))
COLUMNS = [c for c, _ in CLASSES] + ["other"]


def classify(mnemonic):
    for name, prefixes in CLASSES:
        if mnemonic.startswith(prefixes):
            return name
    return "other"


def count(lines):
    c = dict.fromkeys(COLUMNS, 0)
    for ln in lines:
        m = INSN.match(ln)
        if m and not ln.lstrip().startswith((".", ";")):
            c[classify(m.group(1))] += 1
    return c


def kernels(asm):
    """{mangled name: (body lines, {resource: value})} of every function."""
    out, name, body, meta = {}, None, [], None
    for ln in asm.splitlines():
        m = FUNC.match(ln)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if END.match(ln):
                meta = out[name] = (body, {})
                name = None
            else:
                body.append(ln)
        elif meta is not None:  # the resource comments follow the function's end
            m = META.match(ln)
            if m:
                meta[1].setdefault(m.group(1), int(m.group(2)))
    return out


def stretches(lines):
    out, open_at, marks = {}, {}, []
    for i, ln in enumerate(lines):
        m = MARK.search(ln)
        if not m:
            continue
        marks.append(i)
        if m.group(2) == "begin":
            open_at[m.group(1)] = i
        elif m.group(1) in open_at:
            out.setdefault(m.group(1), []).append(count(lines[open_at.pop(m.group(1)):i]))
    # a stretch whose end the compiler laid out before its begin (the tail of
    # a rotated loop): counted up to the next mark of any name
    for name, i in open_at.items():
        nxt = [k for k in marks if k > i]
        if nxt:
            out.setdefault(name + " (to next mark)", []).append(count(lines[i:nxt[0]]))
    return out


def spills(asm):
    """{mangled kernel name: {sgpr_spill_count, vgpr_spill_count}} from the metadata."""
    out, cur = {}, None
    for ln in asm.splitlines():
        m = KNAME.match(ln)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = KSPILL.match(ln)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def report(asm, only=""):
    ks = kernels(asm)
    names = demangle(list(ks))
    sp = spills(asm)
    lines = []
    for n, (body, meta) in ks.items():
        if ".amdhsa_kernel " + n not in asm:  # device functions that were not inlined
            continue
        s = stretches(body)
        short = names[n].split("(")[0]
        if not s or only not in short:
            continue
        lines.append(short)
        meta = {**meta, **sp.get(n, {})}
        lines.append("  " + "  ".join(f"{k} {v}" for k, v in meta.items()))
        lines.append("  " + f"{'stretch':<30}" + "".join(f"{c:>8}" for c in COLUMNS))
        for name, occ in s.items():
            for i, c in enumerate(occ):
                label = name if len(occ) == 1 else f"{name}#{i}"
                lines.append("  " + f"{label:<30}" + "".join(f"{c[k]:>8}" for k in COLUMNS))
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=os.path.join(ROOT, "cairo_amd", "csrc", "kernels.hip"))
    ap.add_argument("--asm", default="", help="count this assembly file instead of compiling")
    ap.add_argument("--keep", default="", help="keep the assembly in this file")
    ap.add_argument("--kernel", default="", help="only kernels whose name contains this")
    a, defs = ap.parse_known_args()
    if a.asm:
        asm = open(a.asm).read()
    else:
        with tempfile.TemporaryDirectory() as d:
            out = a.keep or os.path.join(d, "kernels.s")
            subprocess.run([HIPCC, *FLAGS, "-DCAIRO_ASM_MARKS=1", *defs, "--cuda-device-only", "-S", "-I",
                            os.path.dirname(a.src), a.src, "-o", out], check=True)
            asm = open(out).read()
    print(report(asm, a.kernel))


if __name__ == "__main__":
    sys.exit(main())
