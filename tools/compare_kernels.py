#!/usr/bin/env python3
"""Are the kernels of two builds the same instructions?  For a change that only moves kernels between translation units.

    python tools/compare_kernels.py ASM_DIR_A ASM_DIR_B

ASM_DIR_*: the temporaries of a `hipcc --save-temps` build of the library's sources (the command `python -m
stochvolmodels_amd.build --force` prints, run in a directory of its own).  Every kernel of every unit's device assembly is
compared by name: the instruction text after dropping comments and the .loc / .cfi / .Ltmp lines and renumbering the
.LBB<function>_<block> labels, and the kernel's registers, scratch and LDS (build.kernel_metadata: what libsvmc.isa.json records).
Exit status 1 if the sets of kernels differ or any kernel does.
"""
import glob
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stochvolmodels_amd.build import ASM_GLOB, kernel_metadata  # noqa: E402


def kernels(asm_dir):
    """{kernel symbol: (instruction text, metadata)} over all units of a build; a kernel with two bodies is an error"""
    meta, out = kernel_metadata(asm_dir), {}
    for path in sorted(glob.glob(os.path.join(asm_dir, ASM_GLOB))):
        text = open(path).read()
        for name in meta:
            m = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(name), text, re.M | re.S)
            if m is None:
                continue
            if name in out:
                raise SystemExit("%s defined twice (again in %s)" % (name, path))
            lines = []
            for line in m.group(0).split("\n"):
                line = line.split(";")[0].rstrip()
                if not line or re.match(r"\s*\.(loc|cfi_\w+|file)\b", line) or re.match(r"\.Ltmp\d+:", line):
                    continue
                lines.append(re.sub(r"\.(LBB|Lfunc_end)\d+", r".\1N", line))
            out[name] = ("\n".join(lines), meta[name])
    missing = sorted(set(meta) - set(out))
    if missing:
        raise SystemExit("%s: no body of %s" % (asm_dir, missing[0]))
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    only = sorted(set(a) ^ set(b))
    differ = sorted(k for k in set(a) & set(b) if a[k] != b[k])
    print("kernels: %d and %d, in one build only: %d, compared: %d, differ: %d" %
          (len(a), len(b), len(only), len(set(a) & set(b)), len(differ)))
    for k in only:
        print("  only in %s: %s" % (sys.argv[1] if k in a else sys.argv[2], k))
    for k in differ:
        print("  differs (%s): %s" % ("instructions" if a[k][0] != b[k][0] else "metadata", k))
    return 1 if only or differ else 0


if __name__ == "__main__":
    sys.exit(main())
