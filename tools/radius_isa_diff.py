"""Compare the plain (non-periodic) radius kernels of two device-assembly builds of csrc/knn.hip, ignoring symbol names,
block labels and comments.  Exit 1 if any instruction differs.

    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -DNDEBUG --cuda-device-only -S \
          deepmetv2_amd/csrc/knn.hip -o new.s          (and the same on the other tree -> old.s)
    python tools/radius_isa_diff.py old.s new.s"""
import re, sys, difflib
def funcs(path):
    out, name = {}, None
    for ln in open(path).read().split("\n"):
        m = re.match(r"^(_Z\S+):\s*(;.*)?$", ln)
        if m: name = m.group(1); out[name] = []; continue
        if name and (ln.startswith("\t.section") or re.match(r"^\s*\.Lfunc_end", ln)): name = None; continue
        if name is not None: out[name].append(ln)
    return out
def key(sym):   # kernel name + DP, plain instances only
    m = re.search(r"(radius_\w*kernel)(?:ILi(\d+)E)?", sym)
    return None if "RadPeriod" in sym or "KnnQuerySet" in sym else (m.group(1), m.group(2))
norm = lambda L: [re.sub(r"\s*;.*$", "", re.sub(r"\.LBB\d+_\d+", "LBB", l)) for l in L]
a, b = funcs(sys.argv[1]), funcs(sys.argv[2])
A = {key(k): k for k in a if "radius" in k and key(k)}
Bm = {key(k): k for k in b if "radius" in k and key(k)}
bad = 0
for k in sorted(A):
    d = [l for l in difflib.unified_diff(norm(a[A[k]]), norm(b[Bm[k]]), lineterm="", n=0) if not l.startswith(("@@", "---", "+++"))]
    print(f"{k[0]}<{k[1]}>: {len(a[A[k]])} lines, {len(d)} differing"); bad += len(d)
sys.exit(1 if bad else 0)
