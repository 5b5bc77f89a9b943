#!/usr/bin/env python3
"""Compare the kernels of two `hipcc -S --cuda-device-only` listings.

    hipcc --offload-arch=gfx950 <flags of the Makefile> -S --cuda-device-only \
        csrc/qpsk_kernels.hip -o child.s        (and the parent's file -> parent.s)
    tools/asm_compare.py parent.s child.s [--report REGEX]

Every kernel of the first listing must exist in the second with the same
instruction stream (labels and instructions; comments, directives and blank
lines dropped) and the same register, scratch and LDS counts.  Kernels only
the second has are listed, those matching --report with their counts.  Exit
status 1 on any difference.  Needs no GPU.
"""
import argparse
import re
import sys

META = ("NumVgprs", "NumAgprs", "TotalNumSgprs", "ScratchSize", "LDSByteSize", "Occupancy")


def kernels(path):
    """name -> (instruction lines, {meta: value})"""
    out, name, body = {}, None, []
    with open(path) as f:
        lines = f.read().splitlines()
    funcs = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", "\n".join(lines), flags=re.M))
    i = 0
    while i < len(lines):
        ln = lines[i]
        m = re.match(r"^(\S+):\s*(;.*)?$", ln)
        if m and m.group(1) in funcs and name is None:
            name, body = m.group(1), []
        elif name is not None:
            if re.match(r"^\s*\.section\s+\.rodata", ln) or re.match(r"^\s*\.Lfunc_end", ln):
                meta = {}
                for j in range(i, min(i + 80, len(lines))):
                    mm = re.match(r"^\s*;\s*(\w+):\s*(\d+)", lines[j])
                    if mm and mm.group(1) in META and mm.group(1) not in meta:
                        meta[mm.group(1)] = int(mm.group(2))
                out[name] = (body, meta)
                name = None
            else:
                code = ln.split(";", 1)[0].rstrip()
                if code.strip() and not code.lstrip().startswith("."):
                    body.append(code.strip())
                elif re.match(r"^\.LBB\S+:", code.strip() or ""):
                    body.append(code.strip())
        i += 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("child")
    ap.add_argument("--report", default=None, help="regex of child-only kernels whose counts to print")
    a = ap.parse_args()
    pk, ck = kernels(a.parent), kernels(a.child)
    bad = 0
    for name, (body, meta) in sorted(pk.items()):
        if name not in ck:
            print(f"MISSING  {name}")
            bad += 1
            continue
        cbody, cmeta = ck[name]
        # local labels carry the function's ordinal in the file: compare them by position
        norm = lambda b: [re.sub(r"\.LBB\d+_", ".LBB_", x) for x in b]
        same = norm(body) == norm(cbody) and meta == cmeta
        if not same:
            bad += 1
        print(f"{'same    ' if same else 'DIFFERS '} {len(body):6d} lines  {meta.get('NumVgprs', '?'):>3} VGPRs  {name}")
    new = sorted(set(ck) - set(pk))
    print(f"{len(pk)} kernels of the parent, {bad} differ or are missing; {len(new)} new")
    for name in new:
        if a.report and re.search(a.report, name):
            body, meta = ck[name]
            print(f"new      {len(body):6d} lines  " + "  ".join(f"{k}={meta.get(k, '?')}" for k in META) + f"  {name}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
