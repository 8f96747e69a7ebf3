"""Compare the plain (non-periodic) kNN kernels of two device-assembly builds of csrc/knn.hip, ignoring symbol names,
block labels and comments: knn_kernel (every DP / KP / TQ / EXACT_D instance), knn_merge_kernel, the plan kernel and
the matrix-core filter kernels.  Instances with a RadPeriod or KnnQuerySet argument (the periodic sweep, the two-set
build) are skipped; an empty trailing
pack mangles differently but must compile to the same code.  Exit 1 if any instruction differs or an instance is missing.

    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -DNDEBUG --cuda-device-only -S \
          deepmetv2_amd/csrc/knn.hip -o new.s          (and the same on the other tree -> old.s)
    python tools/knn_isa_diff.py old.s new.s"""
import difflib
import re
import sys


def funcs(path):
    out, name = {}, None
    for ln in open(path).read().split("\n"):
        m = re.match(r"^(_Z\S+):\s*(;.*)?$", ln)
        if m:
            name = m.group(1)
            out[name] = []
            continue
        if name and (ln.startswith("\t.section") or re.match(r"^\s*\.Lfunc_end", ln)):
            name = None
            continue
        if name is not None:
            out[name].append(ln)
    return out


def key(sym):
    """(kernel name, template arguments) of a plain kNN kernel instance, None for anything else."""
    m = re.search(r"\d+(knn_[a-z0-9_]*?kernel)", sym)
    if not m or "RadPeriod" in sym or "KnnQuerySet" in sym:
        return None
    return m.group(1), ",".join(re.findall(r"L[ib](\d+)E", sym))   # the integer / bool template arguments


def norm(lines):
    return [re.sub(r"\s*;.*$", "", re.sub(r"\.LBB\d+_\d+", "LBB", ln)) for ln in lines]


def main(old, new):
    a, b = funcs(old), funcs(new)
    A = {key(k): k for k in a if key(k)}
    Bm = {key(k): k for k in b if key(k)}
    bad = 0
    for k in sorted(A):
        if k not in Bm:
            print(f"{k[0]}<{k[1]}>: missing in {new}")
            bad += 1
            continue
        d = [ln for ln in difflib.unified_diff(norm(a[A[k]]), norm(b[Bm[k]]), lineterm="", n=0)
             if not ln.startswith(("@@", "---", "+++"))]
        print(f"{k[0]}<{k[1]}>: {len(a[A[k]])} lines, {len(d)} differing")
        bad += len(d)
    print(f"{len(A)} plain instances compared, {bad} differing lines")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
