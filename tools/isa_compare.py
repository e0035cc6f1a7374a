#!/usr/bin/env python3
"""tools/isa_compare.py OLD.s NEW.s: do the kernels two tools/isa_dump.sh outputs share hold the same instructions?

A kernel's text runs from its label to its .Lfunc_end. Comments are dropped and the numbers of local labels (.LBB12_3, .Ltmp7, ...) are
masked, and so are the numbers of the labels of inline assembly (.Lwfpt_loop24): they count the functions, blocks and assembly
statements of the whole file, so a kernel added elsewhere shifts them. Prints the kernels only one file
has and those that differ; exits 1 if a shared kernel differs. A kernel whose argument struct grew at its end keeps its instructions but
for the size of the argument block and the offset of the hidden arguments behind it (.amdhsa_kernarg_size and one immediate): such
kernels are listed apart and do not count as different."""
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
            text = re.sub(r"\.L(BB|tmp|func_begin|func_end|JTI|__unnamed_)\d+", r".L\1N", "".join(buf))
            out[name] = re.sub(r"\.L(wfpt_[a-z_]+?)\d+\b", r".L\1N", text)  # inline assembly's own labels (%=)
            name = None
        else:
            buf.append(line.split(";")[0].rstrip() + "\n")
    return out


def only_the_argument_block(a, b):
    """the two texts have the same lines but for .amdhsa_kernarg_size and lines that differ in one immediate (the hidden arguments' offset)"""
    a, b = a.splitlines(), b.splitlines()
    if len(a) != len(b):
        return False
    imm = r"\b(0x[0-9a-f]+|\d+)$"
    for x, y in zip(a, b):
        if x != y and not (".amdhsa_kernarg_size" in x and ".amdhsa_kernarg_size" in y) and \
                not (re.search(imm, x) and re.sub(imm, "", x) == re.sub(imm, "", y) and x.lstrip().startswith(("s_load_dword", "s_add_u32"))):
            return False
    return True


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    shared = sorted(set(old) & set(new))
    differ = [k for k in shared if old[k] != new[k]]
    grown = [k for k in differ if only_the_argument_block(old[k], new[k])]
    differ = [k for k in differ if k not in grown]
    print(f"{len(old)} and {len(new)} kernels, {len(shared)} in both, {len(differ)} of them differ, {len(grown)} only in the size of their argument block")
    for k in sorted(set(new) - set(old)):
        print("only in", sys.argv[2] + ":", k)
    for k in sorted(set(old) - set(new)):
        print("only in", sys.argv[1] + ":", k)
    for k in differ:
        print("differs:", k)
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
