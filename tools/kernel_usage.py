#!/usr/bin/env python3
"""Print VGPR/SGPR/LDS/scratch and a few instruction counts of every kernel in csrc/tome_kernels.hip
(compiles to assembly with hipcc; no GPU needed).

    tools/kernel_usage.py [PATTERN] [-DNAME ...] [--keep] [--against FILE.s]

--keep writes the assembly to /tmp/tome_kernels.s.  --against FILE.s compares every printed kernel with the kernel of
the same name in a kept assembly file (comments stripped, labels renumbered in order of appearance): "identical", or
the resource figures that moved, the number of basic blocks without an equal in the other file and the opcodes whose
counts differ."""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "video-how-do-your-tokens-merge_amd", "csrc", "tome_kernels.hip")  # includes tome_*.h
FIGURES = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")


def kernels(s):
    """name -> (descriptor text, code up to the first s_endpgm, whole function body) of every kernel in assembly s"""
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", s, re.S):
        name = m.group(1)
        i = s.index(name + ":")
        out[name] = (m.group(2), s[i:s.index("s_endpgm", i)], s[i:s.index(".Lfunc_end", i)])
    return out


def figures(desc, code):
    g = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, desc).group(1))
    return [g(k) for k in FIGURES] + [code.count("v_mfma"), len(re.findall(r"global_load", code)),
                                      len(re.findall(r"global_store", code))]


def blocks(body):
    """The function body as a list of basic blocks (tuples of instruction lines) and its opcode histogram."""
    labels = {}
    norm = lambda m: labels.setdefault(m.group(0), "L%d" % len(labels))
    out, cur, ops = [], [], collections.Counter()
    for line in body.split("\n")[1:]:
        line = re.sub(r"\s+", " ", re.sub(r";.*|//.*", "", line)).strip()
        if not line:
            continue
        if re.match(r"\.?\w+:$", line):  # a label opens a block
            out.append(tuple(cur))
            cur = []
            continue
        if line.startswith("."):  # directives (alignment, ...)
            continue
        cur.append(re.sub(r"\.LBB\d+_\d+", norm, line))
        ops[line.split(" ")[0]] += 1
    out.append(tuple(cur))
    return out, ops


def compare(new, old):
    fn, fo = figures(new[0], new[1]), figures(old[0], old[1])
    bn, on = blocks(new[2])
    bo, oo = blocks(old[2])
    if fn == fo and bn == bo:
        return "identical"
    names = ("vgpr", "sgpr", "lds", "scratch", "mfma", "gload", "gstore")
    moved = ", ".join(f"{k} {o} -> {n}" for k, n, o in zip(names, fn, fo) if n != o) or "figures equal"
    cn, co = collections.Counter(bn), collections.Counter(bo)
    nblk = max(sum((cn - co).values()), sum((co - cn).values()))
    hist = ", ".join(f"{op} {oo[op]} -> {on[op]}" for op in sorted(set(on) | set(oo)) if on[op] != oo[op])
    return f"{moved}; {nblk} of {len(bn)} blocks differ; opcodes: {hist or 'same histogram'}"


def main():
    args = sys.argv[1:]
    against = None
    if "--against" in args:
        i = args.index("--against")
        against = kernels(open(args[i + 1]).read())
        del args[i:i + 2]
    pats = [a for a in args if not a.startswith("-")]
    pat = pats[0] if pats else ""
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                        "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt", "-S", "--cuda-device-only", "-o", out, SRC]
                       + [a for a in args if a.startswith("-D")], check=True,
                       stderr=subprocess.DEVNULL)
        s = open(out).read()
        if "--keep" in args:
            open("/tmp/tome_kernels.s", "w").write(s)
    ks = kernels(s)
    demangle = subprocess.run(["c++filt"], input="\n".join(ks), capture_output=True, text=True).stdout.split("\n")
    pretty = dict(zip(ks, demangle))
    same = 0
    for name, (desc, code, body) in ks.items():
        short = re.sub(r"\(.*", "", pretty.get(name, name))
        if pat and pat not in short:
            continue
        vgpr, sgpr, lds, scratch, mfma, gload, gstore = figures(desc, code)
        line = (f"{short[:70]:70s} vgpr {vgpr:>3} sgpr {sgpr:>3} lds {lds:>6} scratch {scratch:>4} | mfma {mfma:3d} "
                f"gload {gload:3d} gstore {gstore:3d} lines {code.count(chr(10)):5d}")
        if against is None:
            print(line)
            continue
        verdict = compare(ks[name], against[name]) if name in against else "not in " + sys.argv[sys.argv.index("--against") + 1]
        if verdict == "identical":
            same += 1
        else:
            print(line + "\n    " + verdict)
    if against is not None:
        gone = [n for n in against if n not in ks and (not pat or pat in n)]
        print(f"{same} kernels identical" + (f"; {len(gone)} kernels of the kept file are gone: {' '.join(gone)}" if gone else ""))


if __name__ == "__main__":
    main()
