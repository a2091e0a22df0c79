#!/usr/bin/env python3
"""Compare the gfx950 code of the kernels two builds of one translation unit have in common.

    hipcc --offload-arch=gfx950 <build.OPTS> --cuda-device-only -S -o before.s <the unit at the parent commit>
    hipcc --offload-arch=gfx950 <build.OPTS> --cuda-device-only -S -o after.s  <the unit now>
    python tools/compare_kernel_isa.py before.s after.s

A kernel of ``after`` whose template arguments are those of a kernel of ``before`` followed by defaulted ``false`` ones is the same
instantiation under its new name (a trailing defaulted template parameter changes the mangled name and nothing else).  For every such
pair the instruction stream (mnemonics and operands, block labels renumbered) and the .amdhsa_ resource directives are compared;
kernels only ``after`` has are listed as new.  Exit status 1 if a pair differs.  DESIGN.md section 4.22 records a run."""
import re
import subprocess
import sys


def kernels(path):
    """{demangled kernel name without its parameter list: (instructions, directives)}"""
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        sym, body = m.group(1), m.group(2)
        code = []
        for ln in body.splitlines():
            ln = ln.split(";")[0].rstrip()
            if not ln or ln.lstrip().startswith((".p2align", ".loc", ".cfi", ".file")):
                continue
            code.append(re.sub(r"_Z\w+", "SYM", re.sub(r"\.LBB\d+_", ".LBB_", ln.strip())))
        d = re.search(r"\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel" % re.escape(sym), text, re.S)
        if d is None:      # a device function, not a kernel
            continue
        out[sym] = (code, [re.sub(r"_Z\w+", "SYM", ln.strip()) for ln in d.group(1).splitlines() if ln.strip()])
    names = subprocess.run(["c++filt"], input="\n".join(out).encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    named = {}
    for sym, name in zip(out, names):
        name = re.sub(r"^void ", "", name)
        m = re.match(r"(.*?<.*?>)\(", name)      # name<args> up to the parameter list
        named[m.group(1) if m else name.split("(")[0]] = out[sym]
    return named


def main(before, after):
    a, b = kernels(before), kernels(after)
    same = differ = 0
    matched = set()
    for name, (code, meta) in sorted(a.items()):
        twin = name
        while twin not in b and twin.endswith(">") and twin.count(",") < 16:
            twin = twin[:-1] + ", false>"
        if twin not in b:
            print("GONE     ", name)
            differ += 1
            continue
        matched.add(twin)
        code2, meta2 = b[twin]
        if code == code2 and meta == meta2:
            same += 1
        else:
            differ += 1
            what = "instructions" if code != code2 else "directives"
            print("DIFFERENT", name, f"({what}: {len(code)} -> {len(code2)} instructions)")
            if code == code2:
                for x, y in zip(meta, meta2):
                    if x != y:
                        print("    ", x, "->", y)
    new = sorted(set(b) - matched)
    print(f"{same} kernels identical, {differ} different or gone, {len(new)} new")
    for name in new:
        print("NEW      ", name, f"({len(b[name][0])} instructions)")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
