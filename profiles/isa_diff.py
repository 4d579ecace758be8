"""Kernel-by-kernel comparison of two directories of gfx950 assembly kept by `ISA_KEEP=<dir> bash profiles/check_isa.sh`:
    python profiles/isa_diff.py <before dir> <after dir>
For every kernel of <before>: "identical" when its instruction stream (labels renumbered, comments dropped) is the same in <after>,
else how many instructions differ; kernels only in <after> are listed as new."""
import glob, os, re, subprocess, sys


def kernels(d):
    out = {}
    for path in sorted(glob.glob(os.path.join(d, "*.s"))):
        txt = open(path).read()
        for m in re.finditer(r"^(_Z\w+):.*?^\.Lfunc_end\d+:", txt, re.S | re.M):
            body = []
            for l in m.group(0).split("\n")[1:-1]:
                l = l.split(";")[0].strip()
                if l and not l.startswith("."):
                    body.append(re.sub(r"\.LBB\d+_", ".LBB_", l))
            out[(os.path.basename(path), m.group(1))] = body
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    names = lambda k: subprocess.run(["c++filt", k[1]], capture_output=True, text=True).stdout.strip().replace("(anonymous namespace)::", "").split("(")[0]
    moved = 0
    for k in sorted(a):
        if k not in b:
            print("%-12s GONE       %s" % (k[0], names(k))); moved += 1
        elif a[k] != b[k]:
            n = sum(1 for x, y in zip(a[k], b[k]) if x != y) + abs(len(a[k]) - len(b[k]))
            print("%-12s MOVED %5d %s" % (k[0], n, names(k))); moved += 1
    for k in sorted(b):
        if k not in a:
            print("%-12s new        %s" % (k[0], names(k)))
    print("kernels of the first build: %d, identical: %d, moved or gone: %d" % (len(a), len(a) - moved, moved))


if __name__ == "__main__":
    main()
