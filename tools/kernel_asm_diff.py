"""Compare the device assembly of two builds of one translation unit kernel by kernel.

    hipcc <the flags of csrc/build.py plan()> -S --cuda-device-only FILE.hip -o a.s     (each tree)
    python tools/kernel_asm_diff.py a.s b.s

The order in which a compiler emits template instantiations follows the host code, so the files are
cut into kernels first: per kernel the instructions (local labels, which carry the function's index
in the file, renumbered; comments dropped) and its .amdhsa_kernel descriptor (registers, LDS,
scratch).  Exit status 0: the same set of kernels with identical code and descriptors.
"""

import re
import sys


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(\w+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S):
        body = re.sub(r"\.L(BB|tmp|func_begin)\d+_?", lambda g: ".L" + g.group(1) + "_", m.group(2))
        out[m.group(1)] = [re.sub(r"[ \t]*;.*$", "", body, flags=re.M)]  # comments shift with the label width
    for m in re.finditer(r"^\t\.amdhsa_kernel (\w+)\n(.*?)^\t\.end_amdhsa_kernel", text, re.M | re.S):
        out[m.group(1)].append(m.group(2))
    return out


def main(a, b):
    ka, kb = kernels(a), kernels(b)
    print(f"{a}: {len(ka)} kernels, {b}: {len(kb)} kernels")
    bad = sorted(set(ka) ^ set(kb))
    for n in bad:
        print("only in", a if n in ka else b, ":", n)
    for n in sorted(set(ka) & set(kb)):
        if ka[n] != kb[n]:
            bad.append(n)
            print("differs:", n)
            for d in (ka[n][1], kb[n][1]):
                print("   ", " ".join(re.findall(r"\.amdhsa_(?:next_free_vgpr|accum_offset|group_segment_fixed_size|"
                                                 r"private_segment_fixed_size) \d+", d)))
    print("IDENTICAL kernel for kernel" if not bad else f"{len(bad)} kernel(s) differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
