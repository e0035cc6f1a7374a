#!/usr/bin/env python3
"""tools/isa_compare.py OLD.s NEW.s: do the kernels two tools/isa_dump.sh outputs share hold the same instructions?

A kernel's text runs from its label to its .Lfunc_end. Comments are dropped and the numbers of local labels (.LBB12_3, .Ltmp7, ...) are
masked: they count the functions and blocks of the whole file, so a kernel added elsewhere shifts them. Prints the kernels only one file
has and those that differ; exits 1 if a shared kernel differs."""
import re
import sys


def kernels(path):
    out, name, buf = {}, None, []
    for line in open(path):
        if name is None:
            m = re.match(r"^(_Z\w+|\w+_kernel\w*):", line)
            if m:
                name, buf = m.group(1), []
        elif line.startswith(".Lfunc_end"):
            out[name] = re.sub(r"\.L(BB|tmp|func_begin|func_end|JTI|__unnamed_)\d+", r".L\1N", "".join(buf))
            name = None
        else:
            buf.append(line.split(";")[0].rstrip() + "\n")
    return out


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    shared = sorted(set(old) & set(new))
    differ = [k for k in shared if old[k] != new[k]]
    print(f"{len(old)} and {len(new)} kernels, {len(shared)} in both, {len(differ)} of them differ")
    for k in sorted(set(new) - set(old)):
        print("only in", sys.argv[2] + ":", k)
    for k in sorted(set(old) - set(new)):
        print("only in", sys.argv[1] + ":", k)
    for k in differ:
        print("differs:", k)
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
