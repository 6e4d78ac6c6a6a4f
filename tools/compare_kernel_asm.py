"""Are the kernels of two builds of one .hip file the same? Compares two device-only assembly listings kernel by kernel, by symbol:
  hipcc <the Makefile's HIPFLAGS> --cuda-device-only -S csrc/FILE.hip -o FILE.s      (once per tree)
  python tools/compare_kernel_asm.py PARENT.s BRANCH.s
The set of kernel symbols (.amdhsa_kernel) must be the same and each kernel's instruction text identical; the order of the kernels
in the file may differ (the number of the function in local labels is ignored, and so are comments). Exit status 0 if so."""
import re
import sys


def kernels(path):
    text = open(path).read()
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    out = {}
    for name in names:
        m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), text, re.M | re.S)   # the code and the kernel descriptor behind it
        assert m, "no body for " + name
        body = [re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0].rstrip()) for line in m.group(1).split("\n")]
        out[name] = [line for line in body if line.strip()]
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = sorted(n for n in a if n in b and a[n] != b[n])
    print("%d kernels in %s, %d in %s" % (len(a), sys.argv[1], len(b), sys.argv[2]))
    print("only in the first: %s\nonly in the second: %s" % (only_a or "none", only_b or "none"))
    print("%d kernels compared by symbol, %d instruction lines; %d differ%s" % (len(set(a) & set(b)), sum(len(a[n]) for n in a if n in b), len(differ),
                                                                             ": " + ", ".join(differ) if differ else ""))
    sys.exit(1 if only_a or only_b or differ else 0)


if __name__ == "__main__":
    main()
