#!/usr/bin/env python3
"""Basic-block census of the device assembly (hipcc --cuda-device-only -S).

    hipcc --offload-arch=gfx950 -O3 -ffp-contract=off --cuda-device-only -S \
          -o engine.s aes-fhe_amd/csrc/ext/engine_ext.hip
    python tools/isa_blocks.py engine.s                      # one line per kernel
    python tools/isa_blocks.py engine.s --filter bconv_cols  # only kernels whose name contains it
    python tools/isa_blocks.py engine.s --blocks 'k_nttf_rows_ks_p<256, true, 1>'

Per kernel: instructions, VALU instructions (v_*, the matrix instructions counted apart), conditional
branches (s_cbranch_*), basic blocks, VGPRs, scratch bytes, LDS bytes and code bytes (the last four
from the compiler's own per-function comments).  A basic block starts at a label that some branch
names or after any branch.  --blocks prints the kernel's block list: first source line of the
assembly, instructions, VALU, matrix, memory instructions, and how the block ends.

The tool counts branches and blocks; it looks for no particular instruction.
"""
import argparse
import re
import shutil
import subprocess
import sys

_LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")
_INSN = re.compile(r"^\s+([a-z][a-z0-9_]*)\b")
_FUNC_END = re.compile(r"^\.Lfunc_end\d+:")
_STAT = {
    "vgprs": re.compile(r";\s*NumVgprs:\s*(\d+)"),
    "agprs": re.compile(r";\s*NumAgprs:\s*(\d+)"),
    "total_vgprs": re.compile(r";\s*TotalNumVgprs:\s*(\d+)"),
    "scratch": re.compile(r";\s*ScratchSize:\s*(\d+)"),
    "lds": re.compile(r";\s*LDSByteSize:\s*(\d+)"),
    "code": re.compile(r";\s*codeLenInByte\s*=\s*(\d+)"),
    "occupancy": re.compile(r";\s*Occupancy:\s*(\d+)"),
}


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    try:
        out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        res = out.split("\n")[:len(names)]
        return dict(zip(names, res)) if len(res) == len(names) else {n: n for n in names}
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def is_branch(op):
    return op.startswith("s_cbranch") or op in ("s_branch", "s_endpgm", "s_setpc_b64", "s_swappc_b64")


def parse(path):
    """[(mangled name, [block, ...], stats)]; block = dict(line, label, ops)."""
    kernels, globl = [], set()
    lines = open(path, errors="replace").read().split("\n")
    for ln in lines:
        if ln.startswith("\t.amdhsa_kernel ") or ln.startswith(".amdhsa_kernel "):
            globl.add(ln.split()[1])
    # labels that a branch names: only those start a block
    targets = set()
    for ln in lines:
        m = _INSN.match(ln)
        if m and (m.group(1).startswith("s_cbranch") or m.group(1) == "s_branch"):
            targets.add(ln.split()[-1])
    cur = None
    for no, ln in enumerate(lines, 1):
        m = _LABEL.match(ln)
        if m:
            name = m.group(1)
            if name in globl and cur is None:
                cur = dict(name=name, blocks=[dict(line=no, label=name, ops=[])], stats={})
                continue
            if cur is not None and _FUNC_END.match(ln):
                cur["closed"] = True
                continue
            if cur is not None and not cur.get("closed") and name in targets and cur["blocks"][-1]["ops"]:
                cur["blocks"].append(dict(line=no, label=name, ops=[]))
            elif cur is not None and not cur.get("closed") and name in targets:
                cur["blocks"][-1]["label"] = name
            continue
        if cur is None:
            continue
        if cur.get("closed"):
            for k, rx in _STAT.items():
                s = rx.search(ln)
                if s and k not in cur["stats"]:
                    cur["stats"][k] = int(s.group(1))
            if "occupancy" in cur["stats"] or ln.startswith("\t.text") or ln.startswith("\t.section"):
                if cur["stats"]:
                    kernels.append(cur)
                    cur = None
            continue
        m = _INSN.match(ln)
        if not m or ln.lstrip().startswith((".", ";")):
            continue
        op = m.group(1)
        blk = cur["blocks"][-1]
        if blk["ops"] and is_branch(blk["ops"][-1]):
            blk = dict(line=no, label="", ops=[])
            cur["blocks"].append(blk)
        blk["ops"].append(op)
    if cur is not None and cur["stats"]:
        kernels.append(cur)
    return kernels


def census(ops):
    valu = sum(o.startswith("v_") and "mfma" not in o for o in ops)
    mfma = sum("mfma" in o for o in ops)
    mem = sum(o.startswith(("global_", "buffer_", "flat_", "scratch_", "ds_", "s_load", "s_buffer_load")) for o in ops)
    cbr = sum(o.startswith("s_cbranch") for o in ops)
    return valu, mfma, mem, cbr


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("asm")
    ap.add_argument("--filter", action="append", default=[], help="only kernels whose demangled name contains this")
    ap.add_argument("--blocks", metavar="KERNEL", help="print the block list of the kernels whose demangled name "
                    "contains this (spaces ignored)")
    a = ap.parse_args()
    ks = parse(a.asm)
    names = demangle([k["name"] for k in ks])
    squash = lambda s: s.replace(" ", "")  # noqa: E731
    if a.blocks:
        hit = [k for k in ks if squash(a.blocks) in squash(names[k["name"]].split("(")[0])]
        if not hit:
            sys.exit(f"no kernel named {a.blocks!r}")
        for k in hit:
            print(f"# {names[k['name']].split('(')[0]}: {len(k['blocks'])} blocks")
            print(f"{'#':>4} {'line':>8} {'insts':>6} {'valu':>6} {'mfma':>5} {'mem':>5}  ends with")
            for i, b in enumerate(k["blocks"]):
                valu, mfma, mem, _ = census(b["ops"])
                end = b["ops"][-1] if b["ops"] and is_branch(b["ops"][-1]) else "(falls through)"
                print(f"{i:>4} {b['line']:>8} {len(b['ops']):>6} {valu:>6} {mfma:>5} {mem:>5}  {end}")
        return
    print(f"{'insts':>7} {'valu':>7} {'mfma':>5} {'cbr':>4} {'blocks':>6} {'vgpr':>5} {'scratch':>7} {'lds':>6} "
          f"{'code B':>7}  kernel")
    for k in sorted(ks, key=lambda k: names[k["name"]]):
        dn = names[k["name"]].split("(")[0].replace("void ", "", 1)
        if a.filter and not any(f in dn for f in a.filter):
            continue
        ops = [o for b in k["blocks"] for o in b["ops"]]
        valu, mfma, _, cbr = census(ops)
        s = k["stats"]
        vg = s.get("total_vgprs", s.get("vgprs", 0))
        print(f"{len(ops):>7} {valu:>7} {mfma:>5} {cbr:>4} {len(k['blocks']):>6} {vg:>5} {s.get('scratch', 0):>7} "
              f"{s.get('lds', 0):>6} {s.get('code', 0):>7}  {dn}")


if __name__ == "__main__":
    main()
