#!/usr/bin/env python3
"""ISA fingerprint of every kernel of both translation units, for refactors that must not change the code generated.

Compiles the units as csrc/Makefile does (pass ITS flags through --flags / --xflags / --hipcc, as for check_asm_stream.py)
to ISA and prints, per kernel: unit, mangled name, instruction count, SHA-256 of its code lines, SHA-256 of its
.amdhsa_kernel descriptor block (registers, LDS, scratch).  Basic-block and function-end labels lose their function number
(it shifts when files are reordered) and comments are dropped; register numbers, instruction order, every s_waitcnt operand
and every descriptor value are hashed as they are.

    python tools/isa_fingerprint.py > before.txt          # on the tree before the change
    python tools/isa_fingerprint.py --against before.txt  # after: names every kernel missing, new or different; exit 1 if any

A tool, not a test: a pinned listing would break on every intended kernel change.
"""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_asm_stream as cas


def code_lines(K):
    """A kernel's lines as hashed: no comments, no blank lines, function numbers taken out of local labels."""
    out = []
    for l in K:
        t = l.split(";")[0].strip()
        if t:
            t = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", t)
            out.append(re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", t))
    return out


def descriptors(lines):
    """name -> the lines of its .amdhsa_kernel ... .end_amdhsa_kernel block"""
    out, name = {}, None
    for l in lines:
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", l)
        if m:
            name = m.group(1)
            out[name] = []
        elif name and re.match(r"^\s*\.end_amdhsa_kernel", l):
            name = None
        elif name:
            out[name].append(l.split(";")[0].strip())
    return out


def fingerprint(lines, unit):
    """-> {"unit name": (instructions, code hash, descriptor hash)}"""
    sha = lambda ls: hashlib.sha256("\n".join(ls).encode()).hexdigest()
    desc, out = descriptors(lines), {}
    for k, K in cas.kernels(lines):
        code = code_lines(K)
        n = sum(1 for t in code if not t.startswith(".") and not t.endswith(":"))
        out[f"{unit} {k}"] = (str(n), sha(code), sha(desc[k]))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--flags", default=cas.FLAGS, help="csrc/Makefile: $(CXXFLAGS)")
    ap.add_argument("--xflags", default=cas.XFLAGS, help="csrc/Makefile: $(XFLAGS), on top of --flags for the split-fp16 unit")
    ap.add_argument("--hipcc", default=cas.HIPCC)
    ap.add_argument("--csrc", default=cas.CSRC, help="directory of the two units (default: this tree's)")
    ap.add_argument("--against", metavar="FILE", help="a listing saved earlier: compare instead of printing")
    args = ap.parse_args()
    found = {}
    with tempfile.TemporaryDirectory() as d:
        procs = []
        for u in cas.UNITS:                                    # both units compile side by side
            unit = os.path.basename(u["src"])
            out = os.path.join(d, unit + ".s")
            cmd = f"{args.hipcc} {args.flags} {args.xflags if u['x'] else ''} -S --cuda-device-only -o {out} {os.path.join(args.csrc, unit)}"
            procs.append((unit, out, subprocess.Popen(cmd, shell=True, stderr=subprocess.DEVNULL)))
        for unit, out, pr in procs:
            if pr.wait() != 0:
                raise SystemExit(f"compiling {unit} failed")
            found.update(fingerprint(open(out).read().split("\n"), unit))
    if not args.against:
        for k in sorted(found):
            print(k, *found[k])
        return 0
    saved = {}
    for l in open(args.against):
        f = l.split()
        if len(f) == 5:
            saved[f"{f[0]} {f[1]}"] = tuple(f[2:])
    bad = 0
    for k in sorted(set(saved) | set(found)):
        if k not in found:
            what = "missing"
        elif k not in saved:
            what = "new"
        elif found[k] != saved[k]:
            what = "different: " + ", ".join(n for n, a, b in zip(("instructions", "code", "descriptor"), saved[k], found[k]) if a != b)
        else:
            continue
        print(f"{k}: {what}")
        bad += 1
    print(f"{len(saved)} kernels saved, {len(found)} now, {bad} missing, new or different")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
