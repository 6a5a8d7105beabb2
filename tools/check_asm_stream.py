#!/usr/bin/env python3
"""Static check of every kernel that fills registers with inline-asm loads (the fp32 MLP kernels' weight ring, the
weight-gradient kernels' operand rings, the split-fp16 inference kernels' LDS reads, ...).  The kernels are found by
what they contain, in both translation units: a new kernel or instance with such a load is checked without being named.

The asm `global_load_dwordx4` loads are asynchronous behind the compiler's back: between a load and the asm
`s_waitcnt vmcnt(N)` that covers it, NO instruction may read or write the destination registers (the compiler could
spill, copy or reuse them -- it believes the asm's outputs are ready immediately).  This script compiles the kernels to
ISA and verifies exactly that for every asm load; csrc/Makefile runs it on every build of the library (with the
build's own flags; a hazard fails the build) and tests/test_abi_symbols.py runs it with a negative self-test.

It also holds the fp32 inference instances to "no scratch" and a code-size limit (RESOURCE_RULE below).

    python tools/check_asm_stream.py        # exit status 0 = no hazard
"""
import bisect
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# code-generation flags: the Makefile passes ITS OWN ($(CXXFLAGS)) through --flags, so the ISA checked here is the ISA
# of the library being built; the default below mirrors csrc/Makefile for stand-alone runs
FLAGS = "-O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -mllvm -large-interval-freq-threshold=100000000 --offload-arch=gfx950"
HIPCC = "/opt/rocm/bin/hipcc"
# The library is two translation units (csrc/Makefile): the split-fp16 kernels are compiled with XFLAGS on top of the common
# flags (nerf_kernels_x.hip says why); each unit is checked on the flags IT is built with.
XFLAGS = "-mllvm -amdgpu-mfma-vgpr-form=1"
CSRC = os.path.join(REPO, "nerf_replication_amd", "csrc")
MAX_CNT = 64       # above every count an s_waitcnt can encode (vmcnt: 6 bits, lgkmcnt: 4 bits)
UNITS = [{"src": os.path.join(CSRC, "nerf_kernels.hip"), "x": False}, {"src": os.path.join(CSRC, "nerf_kernels_x.hip"), "x": True}]


def vregs(text):
    out = set()
    for m in re.finditer(r"\bv\[(\d+):(\d+)\]", text):
        out |= set(range(int(m.group(1)), int(m.group(2)) + 1))
    for m in re.finditer(r"\bv(\d+)\b", text):
        out.add(int(m.group(1)))
    return out


def kernels(lines):
    """(name, code lines) of every kernel of a unit's ISA: from its label to its .amdhsa_kernel descriptor."""
    label = {}
    for i, l in enumerate(lines):
        m = re.match(r"^([A-Za-z_$][\w$.]*):", l)
        if m:
            label.setdefault(m.group(1), i)
    out = []
    for i, l in enumerate(lines):
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", l)
        if m:
            out.append((m.group(1), lines[label[m.group(1)]:i]))
    return sorted(out)


# The fp32 inference instances (nerf_mlp_f32_kernel<*, SAVE = false, ...>) run one wave per SIMD on the whole register file and
# must not spill: a spill of a ring register is exactly the hazard above, and scratch traffic at the MFMA issue limit is time.
# That property hangs on a register-coalescer option of the build (csrc/Makefile, -large-interval-freq-threshold): without it
# the same source compiles to 290-310 KB of accumulator copies with 512 registers and 20-44 bytes of scratch, silently.  So
# every run also reads the compiler's own resource lines: scratch must be 0 and the code below 128 KiB (84-108 KB with the
# option; a tripwire far from both, twice the 64-KiB instruction cache, not a tuned figure).
RESOURCE_RULE = re.compile(r"^_Z19nerf_mlp_f32_kernelILb[01]ELb0E")
MAX_CODE_BYTES = 128 * 1024


def check_resources(lines):
    """-> [(kernel, what is wrong)] for the kernels RESOURCE_RULE names; none of them found is an error too."""
    name, code, found, bad = None, None, 0, []
    for l in lines:
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", l)
        if m:
            name, code = m.group(1), None
        m = re.match(r"^; codeLenInByte = (\d+)", l)
        if m:
            code = int(m.group(1))
        m = re.match(r"^; ScratchSize: (\d+)", l)
        if m and name is not None and RESOURCE_RULE.match(name):
            found += 1
            scratch = int(m.group(1))
            print(f"{name}: {code} code bytes, {scratch} scratch bytes")
            if scratch != 0:
                bad.append((name, f"{scratch} bytes of scratch (must be 0)"))
            if code is None or code > MAX_CODE_BYTES:
                bad.append((name, f"{code} code bytes (limit {MAX_CODE_BYTES})"))
            name = None
    return found, bad


def check(K):
    """K: the code lines of one kernel.  -> (number of inline-asm loads, hazards)"""
    ins, label_at = [], {}
    for i, l in enumerate(K):
        t = l.strip()
        if re.match(r"^\.L\w+:", t):                                  # the compiler's blocks, and labels inside asm statements
            label_at[t.split(":")[0]] = len(ins)                 # index of the first instruction after the label
        elif t and not t.startswith((";", ".")):
            ins.append((i, t))
    # source line -> inside an inline-asm block (";;#ASMSTART" ... ";;#ASMEND"; a block may hold several instructions)
    asm_line, inside = set(), False
    for i, l in enumerate(K):
        if "ASMSTART" in l:
            inside = True
        elif "ASMEND" in l:
            inside = False
        elif inside:
            asm_line.add(i)
    in_asm = lambda idx: ins[idx][0] in asm_line
    is_vmem = lambda l: l.startswith(("global_", "buffer_", "scratch_", "flat_"))
    is_lds = lambda l: l.startswith("ds_")
    asm_vm_load = lambda idx: re.match(r"global_load_dword(x2|x4)?\b", ins[idx][1]) and "s[" in ins[idx][1] and in_asm(idx)
    # asm LDS reads (nerf_mlp_f32x.hip.inc and friends): covered by `s_waitcnt lgkmcnt(N)`.  LDS operations return in order, so a
    # read has landed once at most N operations may be outstanding and >= N LDS operations were issued after it (scalar loads share
    # the counter but complete out of order: they are NOT counted as younger operations -- that is the conservative direction)
    asm_lds_load = lambda idx: re.match(r"ds_read_b(32|64|96|128)\b", ins[idx][1]) and in_asm(idx)
    asm_load = lambda idx: asm_vm_load(idx) or asm_lds_load(idx)
    loads = [idx for idx in range(len(ins)) if asm_load(idx)]
    hazards = []

    def walk(start, dst, lds):
        """Follow EVERY control-flow path from instruction `start` until a wait covers the load (at most `cnt` younger
        memory operations outstanding); report every instruction on the way that touches dst.  Both sides of every
        conditional branch are followed, however many lie between a load and its wait (the k-step skipping of the fp32
        inference kernels puts up to four more there): the states (instruction, younger operations) are memoised, and
        `younger` never needs to exceed the largest wait count of the kernel, so the walk is finite without a depth limit.
        Labels and branches inside an asm statement are followed like the compiler's (the leading-dead-group fetch of the fp32
        inference kernels is one asm statement with a branch around its loads), and a branch is followed both ways whatever it
        tests: paths the kernel cannot take (a group stepped over after the prefix was left) are proven hazard-free as well.
        A path that leaves the kernel's code without a wait is reported, not dropped."""
        pat = r"lgkmcnt\((\d+)\)" if lds else r"vmcnt\((\d+)\)"
        seen, todo = set(), [(start, 0)]
        while todo:
            idx, younger = todo.pop()
            while True:
                if idx >= len(ins):
                    hazards.append(("path runs off the end of the kernel without a wait", ld_text, ""))
                    break
                younger = min(younger, MAX_CNT)                   # (every count a wait can ask for is <= MAX_CNT)
                if (idx, younger) in seen:
                    break
                seen.add((idx, younger))
                l = ins[idx][1]
                m = re.search(pat, l) if l.startswith("s_waitcnt") else None
                if m and younger >= int(m.group(1)):
                    break                                         # covered on this path
                touched = vregs(l.split(",")[0]) if asm_load(idx) else vregs(l)
                if touched & dst:
                    hazards.append(("touched before its wait", ld_text, l))
                    break
                if (is_lds(l) if lds else is_vmem(l)):
                    younger += 1
                if l.startswith("s_endpgm"):                      # no load may be outstanding when the wave ends
                    hazards.append(("never waited for before the end of the program", ld_text, l))
                    break
                if l.startswith("s_branch"):
                    idx = label_at[l.split()[1]]
                    continue
                if l.startswith("s_cbranch"):
                    todo.append((label_at[l.split()[1]], younger))
                idx += 1

    for ld in loads:
        ld_text = ins[ld][1]
        walk(ld + 1, vregs(ld_text.split(",")[0]), bool(asm_lds_load(ld)))
    return len(loads), hazards


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--flags", default=FLAGS, help="code-generation flags of the build being checked (csrc/Makefile: $(CXXFLAGS))")
    ap.add_argument("--xflags", default=XFLAGS, help="what the split-fp16 unit is compiled with on top of --flags (csrc/Makefile: $(XFLAGS))")
    ap.add_argument("--hipcc", default=HIPCC)
    args = ap.parse_args()
    extra = os.environ.get("NERF_CHECK_EXTRA_FLAGS", "")     # e.g. -DNERF_F32_ASM_OVERRUN=1 -DNERF_TIMING_BUILD: must report hazards
    bad = 0
    with tempfile.TemporaryDirectory() as d:
        procs = []
        for i, u in enumerate(UNITS):                          # both units compile side by side
            out = os.path.join(d, f"k{i}.s")
            cmd = f"{args.hipcc} {args.flags} {args.xflags if u['x'] else ''} -S --cuda-device-only {extra} -o {out} {u['src']}"
            procs.append((u, out, subprocess.Popen(cmd, shell=True, stderr=subprocess.DEVNULL)))
        for u, out, pr in procs:
            if pr.wait() != 0:
                raise SystemExit(f"compiling {u['src']} failed")
            lines = open(out).read().split("\n")
            checked = 0
            for k, K in kernels(lines):
                n, hz = check(K)
                if n == 0:
                    continue                                   # no inline-asm load: nothing the compiler cannot see
                checked += 1
                print(f"{k}: {n} asm loads, {len(hz)} hazards")
                for kind, ld, use in hz[:10]:
                    print("   ", kind, "|", ld, "|", use)
                bad += len(hz)
            if not u["x"]:                                     # the unit of the fp32 kernels: scratch and code size
                found, wrong = check_resources(lines)
                for k, what in wrong:
                    print("   ", k, "|", what)
                if found != 4:
                    print(f"    ({found} fp32 inference instances found, 4 expected: RESOURCE_RULE no longer names them)")
                bad += len(wrong) + (found != 4)
            if checked == 0:                                   # both units have such kernels: their loads were not recognised
                print(f"    (no kernel with an inline-asm load found in {os.path.basename(u['src'])})")
                bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
