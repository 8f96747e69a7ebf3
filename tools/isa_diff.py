"""Compare the device code of two builds, kernel instance by kernel instance.

Each side is one or more device-assembly files; a kernel may move between files (csrc/knn.hip and csrc/radius.hip were
one file once).  Every __global__ kernel (.amdhsa_kernel) is keyed by its mangled symbol -- the name, every template
argument (type arguments such as RadPeriod / KnnQuerySet included) and the parameter types -- and so is every device
function that was not inlined.  Instruction lines are compared with block labels and comments removed, and so is each
kernel's descriptor (.amdhsa_kernel ... .end_amdhsa_kernel: argument-block size, LDS, scratch, register counts).
Exit 1 if a line differs, an instance exists on one side only, or a side defines an instance twice.

    FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -DNDEBUG --cuda-device-only -S"
    hipcc $FLAGS deepmetv2_amd/csrc/knn.hip -o new_knn.s       (radius.hip -> new_radius.s; the other tree -> old_*.s)
    python tools/isa_diff.py old_knn.s -- new_knn.s new_radius.s"""
import difflib
import re
import shutil
import subprocess
import sys


def read_side(paths):
    """{symbol: instruction lines + descriptor lines}, the set of kernel symbols, the symbols defined more than once."""
    funcs, kernels, twice = {}, set(), []
    for path in paths:
        with open(path) as f:
            lines = f.read().split("\n")
        name = desc = None
        for ln in lines:
            m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", ln)
            if m:
                desc = m.group(1)
                kernels.add(desc)
                continue
            if desc is not None:     # the descriptor follows the body: its directives join the kernel's lines
                if ln.strip() == ".end_amdhsa_kernel":
                    desc = None
                else:
                    funcs.setdefault(desc, []).append(ln.strip())
                continue
            m = re.match(r"^(_Z\S+):\s*(;.*)?$", ln)
            if m:
                name = m.group(1)
                if name in funcs:
                    twice.append(name)
                funcs[name] = []
            elif name and (ln.startswith("\t.section") or re.match(r"^\s*\.Lfunc_end", ln)):
                name = None
            elif name is not None:
                funcs[name].append(re.sub(r"\s*;.*$", "", re.sub(r"\.LBB\d+_\d+", "LBB", ln)))
    return funcs, kernels, twice


def demangler():
    exe = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if exe is None:
        return lambda s: s
    return lambda s: subprocess.run([exe, s], capture_output=True, text=True).stdout.strip() or s


def main(argv):
    if "--" not in argv or argv[0] == "--" or argv[-1] == "--":
        print(__doc__)
        return 2
    cut = argv.index("--")
    (a, ka, ta), (b, kb, tb) = read_side(argv[:cut]), read_side(argv[cut + 1:])
    show = demangler()
    differing = 0
    for sym in sorted(set(a) & set(b)):
        d = [ln for ln in difflib.unified_diff(a[sym], b[sym], lineterm="", n=0) if not ln.startswith(("@@", "---", "+++"))]
        if d:
            print(f"{show(sym)}: {len(a[sym])} lines, {len(d)} differing")
            differing += len(d)
    one_side = sorted(set(a) ^ set(b))
    for sym in one_side:
        print(f"{show(sym)}: only on the {'first' if sym in a else 'second'} side")
    for sym in ta + tb:
        print(f"{show(sym)}: defined twice on one side")
    both = set(a) & set(b)
    print(f"{len(both & ka & kb)} kernel instances and {len(both - ka - kb)} device functions compared, "
          f"{differing} differing lines, {len(one_side)} on one side only, {len(ta + tb)} defined twice")
    return 1 if differing or one_side or ta or tb else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
