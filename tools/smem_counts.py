"""Scalar-load and wait counts of the kernels, from their gfx950 assembly.

Compiles cairo_amd/csrc/kernels.hip with the Makefile's flags (plus any extra
-D given), keeps the assembly and counts per kernel: scalar loads (by width),
`s_waitcnt` instructions that wait for lgkmcnt(0), and lane reads / writes of
spilled SGPRs.  With -DCAIRO_ASM_MARKS=1 the row coder brackets its
macroblock-start stretch (loop header to the barrier before the search) and
the helper its group start with assembly comments; the stretches between a
`cairo-mark <name> begin` and its `end` are counted too (straight through the
text, so a stretch's cold blocks that the compiler moved elsewhere are not in
it).  No GPU needed.
usage: python tools/smem_counts.py [--src PATH] [--asm FILE.s] [--json OUT] [-DFOO=1 ...]
"""
import argparse
import json
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
SLOAD = re.compile(r"^\s+s_(?:buffer_)?load_(dword(?:x\d+)?)\b")
WAIT = re.compile(r"^\s+s_waitcnt\b(.*)$")
MARK = re.compile(r";\s*cairo-mark (\w+) (begin|end)")


def count(lines):
    c = {"s_load": 0, "s_load_by_width": {}, "lgkmcnt0_waits": 0, "v_readlane": 0, "v_writelane": 0}
    for ln in lines:
        m = SLOAD.match(ln)
        if m:
            c["s_load"] += 1
            c["s_load_by_width"][m.group(1)] = c["s_load_by_width"].get(m.group(1), 0) + 1
            continue
        m = WAIT.match(ln)
        if m:
            # "s_waitcnt lgkmcnt(0)", combined forms, and the bare immediate forms the assembler prints
            if "lgkmcnt(0)" in m.group(1):
                c["lgkmcnt0_waits"] += 1
            continue
        if re.match(r"^\s+v_readlane_b32\b", ln):
            c["v_readlane"] += 1
        elif re.match(r"^\s+v_writelane_b32\b", ln):
            c["v_writelane"] += 1
    return c


def kernels(asm):
    out, name, body = {}, None, []
    for ln in asm.splitlines():
        m = FUNC.match(ln)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if END.match(ln):
                out[name] = body
                name = None
            else:
                body.append(ln)
    return out


def stretches(lines):
    out, open_at = {}, {}
    for i, ln in enumerate(lines):
        m = MARK.search(ln)
        if not m:
            continue
        if m.group(2) == "begin":
            open_at[m.group(1)] = i
        elif m.group(1) in open_at:
            seg = lines[open_at.pop(m.group(1)):i]
            c = count(seg)
            c["lines"] = len(seg)
            out.setdefault(m.group(1), []).append(c)
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=os.path.join(ROOT, "cairo_amd", "csrc", "kernels.hip"))
    ap.add_argument("--asm", default="", help="count this assembly file instead of compiling")
    ap.add_argument("--json", default="")
    a, defs = ap.parse_known_args()
    if a.asm:
        asm = open(a.asm).read()
    else:
        with tempfile.TemporaryDirectory() as d:
            out = os.path.join(d, "kernels.s")
            subprocess.run([HIPCC, *FLAGS, *defs, "--cuda-device-only", "-S", "-I", os.path.dirname(a.src), a.src,
                            "-o", out], check=True)
            asm = open(out).read()
    ks = kernels(asm)
    names = demangle(list(ks))
    res = {}
    for n, body in ks.items():
        if ".amdhsa_kernel " + n not in asm:  # device functions that were not inlined
            continue
        c = count(body)
        s = stretches(body)
        if s:
            c["stretches"] = s
        res[names[n].split("(")[0]] = c
    print(json.dumps(res, indent=1))
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    sys.exit(main())
