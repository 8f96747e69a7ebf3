"""Condensation clustering stated twice on the host (include/dmet.h, "Condensation clustering"), and the cases of
tests/test_condense_host.py and tests/test_gpu_condense.py.

  sequential   the rule as written: walk the candidates by descending canonical beta, a still-unassigned one becomes the
               next condensation point and takes every still-unassigned node within t_d.
  recursive    the characterisation over an O(n^2) matrix of distances: a candidate is a point iff no point with a higher
               key lies within t_d of it; a node's point is the highest-key point within t_d of it.

Distances are rule R1's fp32 chain, acc = fmaf(a, a, acc) over the coordinates in order.  The fused step is formed in
float64: a * a is exact there (24 x 24 bits), the sum is rounded to float64 and then to float32.  That double rounding can
differ from fmaf only when the float64 sum falls on a float32 tie; every case here keeps its distances exact (lattices) or
far from t_d^2 (the line), so neither that nor the rounding of t_d^2 = fl32(t_d) * fl32(t_d) can matter.

Random cases live on the lattice k / 8 with t_d = 0.3: every d^2 is a multiple of 1/64, and fl32(0.3)^2 = 0.0900000036
lies strictly between 5/64 and 6/64.
"""
import types

import numpy as np

T_D = 0.3           # with the k / 8 lattice
T_BETA = 0.25       # with beta in sixteenths
F32 = np.float32


def td2_of(t_d) -> np.float32:
    t = F32(t_d)
    return F32(t * t)


def chain_d2(x: np.ndarray, p: int) -> np.ndarray:
    """d2(j, p) for every row j of x [n, D] fp32: the R1 chain."""
    acc = np.zeros(x.shape[0], dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(x.shape[1]):
            a = (x[:, c] - x[p, c]).astype(F32)
            acc = (a.astype(np.float64) * a.astype(np.float64) + acc.astype(np.float64)).astype(F32)
    return acc


def candidate_order(beta: np.ndarray, t_beta) -> np.ndarray:
    """The candidates (beta > t_beta in fp32, strictly: no NaN) by descending canonical beta (-0.0 = +0.0), ties to the
    lower index."""
    beta = beta.astype(F32)
    with np.errstate(invalid="ignore"):
        cand = np.flatnonzero(beta > F32(t_beta))
    key = beta[cand] + F32(0.0)                 # -0.0 + 0.0 = +0.0
    return cand[np.lexsort((cand, -key.astype(np.float64)))]


def sequential_event(beta, x, t_beta, t_d):
    """(local[n], assoc[n] event-local, points) of one event by the rule as written."""
    n = beta.shape[0]
    x = x.astype(F32)                           # [n, D], as _case leaves it
    td2 = td2_of(t_d)
    local = np.full(n, -1, dtype=np.int64)
    assoc = np.full(n, -1, dtype=np.int64)
    points = []
    for c in candidate_order(beta, t_beta):
        if local[c] >= 0:
            continue
        with np.errstate(invalid="ignore"):
            take = (local < 0) & (chain_d2(x, c) < td2)
        take[c] = True
        local[take] = len(points)
        assoc[take] = c
        points.append(int(c))
    return local, assoc, points


def recursive_event(beta, x, t_beta, t_d):
    """The same three by the characterisation, over the full matrix of chain distances."""
    n = beta.shape[0]
    x = x.astype(F32)                           # [n, D], as _case leaves it
    td2 = td2_of(t_d)
    d2 = np.stack([chain_d2(x, p) for p in range(n)]) if n else np.zeros((0, 0), dtype=F32)   # d2[p, j]
    with np.errstate(invalid="ignore"):
        near = d2 < td2
    order = candidate_order(beta, t_beta)
    points = []
    for c in order:                             # higher keys first: their verdicts are known
        if not any(near[p, c] for p in points):
            points.append(int(c))
    local = np.full(n, -1, dtype=np.int64)
    assoc = np.full(n, -1, dtype=np.int64)
    for j in range(n):
        for q, p in enumerate(points):          # points are in descending key order
            if p == j or near[p, j]:
                local[j], assoc[j] = q, p
                break
    return local, assoc, points


def over_batch(event_fn, case):
    """An event function over the events of a case: a namespace with labels (numbered over the batch), local, assoc (global
    ids), points, points_batch, counts -- all int64."""
    beta, x, sizes = case.beta, case.x, case.sizes
    ptr = ptr_of(sizes)
    labels, local, assoc, points, pbatch, counts = [], [], [], [], [], []
    first = 0
    for b in range(len(sizes)):
        lo, hi = int(ptr[b]), int(ptr[b + 1])
        loc, asc, pts = event_fn(beta[lo:hi], x[lo:hi], case.t_beta, case.t_d)
        local.append(loc)
        labels.append(np.where(loc >= 0, loc + first, loc))
        assoc.append(np.where(asc >= 0, asc + lo, asc))
        points += [lo + p for p in pts]
        pbatch += [b] * len(pts)
        counts.append(len(pts))
        first += len(pts)
    cat = lambda parts: np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, dtype=np.int64)   # noqa: E731
    return types.SimpleNamespace(labels=cat(labels), local=cat(local), assoc=cat(assoc),
                                 points=np.asarray(points, dtype=np.int64), points_batch=np.asarray(pbatch, dtype=np.int64),
                                 counts=np.asarray(counts, dtype=np.int64))


def sequential(case):
    return over_batch(sequential_event, case)


def recursive(case):
    return over_batch(recursive_event, case)


def ptr_of(sizes) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.int64)


def _case(name, beta, x, sizes, t_beta=T_BETA, t_d=T_D):
    beta = np.ascontiguousarray(beta, dtype=F32)
    x = np.ascontiguousarray(x, dtype=F32).reshape(beta.shape[0], -1)
    assert sum(sizes) == beta.shape[0]
    return types.SimpleNamespace(name=name, beta=beta, x=x, sizes=list(sizes), t_beta=t_beta, t_d=t_d, N=beta.shape[0],
                                 D=x.shape[1])


# ---- the cases ------------------------------------------------------------------------------------------------------------
def _lattice(rng, n, D, extent):
    """n points on the k / 8 lattice with k in [0, extent), beta in sixteenths 0 .. 1: heavy ties in both."""
    return rng.integers(0, 17, n).astype(F32) / F32(16), rng.integers(0, extent, (n, D)).astype(F32) / F32(8)


RAGGED_SIZES = (0, 1, 63, 64, 65, 130, 300)
RAGGED_EXTENT = {1: 60, 2: 10, 3: 5, 8: 2}      # lattice extent per D: events with tens of points and with noise


def ragged(D: int):
    """Event sizes round the window and the wavefront, on the lattice."""
    rng = np.random.default_rng(100 + D)
    parts = [_lattice(rng, n, D, RAGGED_EXTENT[D]) for n in RAGGED_SIZES]
    return _case(f"ragged_d{D}", np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), RAGGED_SIZES)


def random_batch():
    """40 events of 1 .. 200 nodes in D = 2, among them one without a candidate, one with one node that is a point, and
    wide ones with more than 64 points."""
    rng = np.random.default_rng(7)
    sizes, betas, xs = [], [], []
    for e in range(40):
        n = int(rng.integers(1, 201))
        extent = 12
        if e == 3:
            n = 1
        if e in (10, 20, 30):
            n, extent = 200, 64                 # sparse: most candidates are points of their own
        beta, x = _lattice(rng, n, 2, extent)
        if e == 3:
            beta[:] = 0.75
        if e == 5:
            beta = np.minimum(beta, F32(T_BETA))        # none above the threshold: beta == t_beta is no candidate
        sizes.append(n)
        betas.append(beta)
        xs.append(x)
    return _case("random", np.concatenate(betas), np.concatenate(xs), sizes)


def line(descending: bool, n: int = 200):
    """n points on a line at spacing 0.6 t_d, beta strictly monotonic: a dead entry must not suppress the next one."""
    t_d = 1.0
    x = (np.arange(n, dtype=np.float64) * 0.6 * t_d).astype(F32)
    beta = (0.5 + np.arange(n, dtype=np.float64) / (4 * n)).astype(F32)
    beta = beta[::-1].copy() if descending else beta
    assert np.all(np.diff(beta) != 0)
    return _case("line_desc" if descending else "line_asc", beta, x, [n], t_beta=0.1, t_d=t_d)


WINDOW_COUNTS = (63, 64, 65, 128, 129)


def window_edge(count: int, coincident: bool):
    """`count` candidates, mutually farther than t_d or all on one spot, with distinct beta in shuffled order, between
    20 non-candidates that sit on candidates' spots; a second event of three nodes follows."""
    rng = np.random.default_rng(1000 + count + (500 if coincident else 0))
    n = count + 20
    is_cand = np.zeros(n, dtype=bool)
    is_cand[rng.permutation(n)[:count]] = True
    cand = np.flatnonzero(is_cand)
    beta = np.zeros(n, dtype=F32)
    beta[cand] = (F32(0.5) + rng.permutation(count).astype(F32) / F32(512))
    x = np.zeros((n, 2), dtype=F32)
    if not coincident:
        spot = np.stack([np.arange(count) % 16, np.arange(count) // 16], axis=1).astype(F32)   # spacing 1 > t_d
        x[cand] = spot
        x[~is_cand] = spot[rng.integers(0, count, n - count)]
    tail_beta, tail_x = np.array([0.5, 0.0, 0.75], dtype=F32), np.array([[0, 0], [0, 0], [9, 9]], dtype=F32)
    return _case(f"window_{count}_{'same' if coincident else 'apart'}", np.concatenate([beta, tail_beta]),
                 np.concatenate([x, tail_x]), [n, 3])


def radius_edge(t_d):
    """A 6 x 6 integer lattice, every node a candidate: with t_d = 1 a neighbour sits at d2 == t_d2 and is not taken."""
    g = np.stack(np.meshgrid(np.arange(6), np.arange(6), indexing="ij"), axis=-1).reshape(-1, 2).astype(F32)
    beta = (F32(0.5) + np.random.default_rng(5).permutation(36).astype(F32) / F32(128))
    return _case("radius_edge_at" if t_d == 1.0 else "radius_edge_above", beta, g, [36], t_beta=0.1, t_d=t_d)


def specials():
    """name -> (case, the labels it must give), worked by hand; one event each."""
    nan, inf = F32(np.nan), F32(np.inf)
    out = {}
    # constant beta: index order decides -- 0 takes 1, then 2 takes 3
    out["constant_beta"] = (_case("constant_beta", [0.5] * 4, [0.0, 0.125, 0.375, 0.5], [4]), [0, 0, 1, 1])
    # beta == t_beta exactly is no candidate: node 0 is collected by node 1, node 2 is far and noise
    out["at_threshold"] = (_case("at_threshold", [0.25, 0.5, 0.25], [0.0, 0.125, 5.0], [3]), [0, 0, -1])
    # a NaN beta is no candidate (node 0, 2) but node 0 is still collected; node 2 is far: noise
    out["nan_beta"] = (_case("nan_beta", [nan, 0.5, nan], [0.0, 0.125, 5.0], [3]), [0, 0, -1])
    # +inf ranks first: node 2 is point 0 and takes 1; node 0 is out of its reach
    out["inf_beta"] = (_case("inf_beta", [0.875, 0.5, inf], [0.0, 0.25, 0.5], [3]), [1, 0, 0])
    # -0.0 and +0.0 tie (t_beta = -1): the lower index first whichever sign it holds
    out["signed_zeros"] = (_case("signed_zeros", [0.0, -0.0, -0.0, 0.0], [0.0, 1.0, 1.125, 0.125], [4], t_beta=-1.0),
                           [0, 1, 1, 0])
    # a candidate with a NaN coordinate is a point of itself alone; it ranks first here and collects nobody
    out["nan_coordinate"] = (_case("nan_coordinate", [0.875, 0.5, 0.125], [[0.0, nan], [0.0, 0.0], [0.0, 0.125]], [3]),
                             [0, 1, 1])
    return out


def inconsistent_ranking():
    """Three events on the lattice; the test replaces one ranking entry of the middle event by ids outside it."""
    rng = np.random.default_rng(11)
    sizes = (70, 90, 80)
    parts = [_lattice(rng, n, 2, 10) for n in sizes]
    return _case("inconsistent", np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), sizes)
