#!/usr/bin/env python3
"""Compare two device assembly files (hipcc --offload-device-only -S) function
by function: the proof that a refactor left the device code as it was.

    python tools/asm_same.py A.s B.s [--ignore-kernel NAME ...]

A file is cut at every function's preamble and at every other global label
into functions (a kernel's chunk runs on through its .amdhsa_kernel descriptor) and its metadata into one entry per
kernel.  Lines naming the per-file __hip_cuid_ symbol are dropped and the
function ordinal in local labels (.LBB12_3, .Lfunc_end12) is masked, so a
renamed file or a function removed further up compares equal.  Prints `same`
or the first differing line per function; exit status 1 on any difference, on
a function present on one side only, or on a different order.  NAME matches
a function whose (mangled) name contains it.
"""
import argparse
import re
import sys

BEGIN = re.compile(r"; -- Begin function (\S+)")  # on the first line of a function's preamble
LABEL = re.compile(r"^([A-Za-z_$][\w$.]*):")
ORDINAL = re.compile(r"\b(LBB|BB|Lfunc_begin|Lfunc_end)\d+")


def functions(path, ignore):
    """[(name, lines)] in file order; the text before the first label is '<head>'."""
    out, cur, meta = [("<head>", [])], None, False
    for line in open(path):
        line = line.rstrip()
        if "__hip_cuid_" in line:
            continue
        if line.strip() == ".amdgpu_metadata":
            meta = True
        m = BEGIN.search(line) or LABEL.match(line)
        if meta and line.startswith("  - ."):  # one metadata entry per kernel
            out.append(["<meta>", []])
        elif meta and line.startswith("amdhsa."):  # the file's own keys (target, version)
            out.append(["meta:" + line.split(":")[0], []])
        elif not meta and m and not m.group(1).startswith(".L") and m.group(1) != out[-1][0]:
            out.append([m.group(1), []])
        if meta and ".name:" in line and out[-1][0] == "<meta>":
            out[-1][0] = "meta:" + line.split(".name:")[1].strip()
        out[-1][1].append(ORDINAL.sub(r"\1#", line))
    return [(n, l) for n, l in out if not any(i in n for i in ignore)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--ignore-kernel", action="append", default=[], metavar="NAME")
    args = ap.parse_args()
    fa, fb = functions(args.a, args.ignore_kernel), functions(args.b, args.ignore_kernel)
    da, db, bad = dict(fa), dict(fb), 0
    for name, la in fa:
        if name not in db:
            print("%-72s only in %s" % (name, args.a))
            bad += 1
            continue
        lb = db[name]
        diff = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), None)
        if diff is None and len(la) != len(lb):
            diff = min(len(la), len(lb))
        if diff is None:
            short = name if len(name) <= 120 else name[:117] + "..."  # (rocPRIM's names run to 1 KB)
            print("%-72s same (%d lines)" % (short, len(la)))
        else:
            print("%-72s DIFFERS at its line %d:\n  < %s\n  > %s" %
                  (name, diff + 1, la[diff] if diff < len(la) else "<end>", lb[diff] if diff < len(lb) else "<end>"))
            bad += 1
    for name, _ in fb:
        if name not in da:
            print("%-72s only in %s" % (name, args.b))
            bad += 1
    if not bad and [n for n, _ in fa] != [n for n, _ in fb]:
        print("the functions come in a different order")
        bad += 1
    kernels = sum(1 for n, _ in fa if n.startswith("meta:") and not n.startswith("meta:amdhsa."))
    print("%s: %d functions, %d kernels%s" % ("SAME" if not bad else "DIFFERENT", len(fa), kernels,
                                              ", ignoring " + ", ".join(args.ignore_kernel) if args.ignore_kernel else ""))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
