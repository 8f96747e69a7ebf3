"""References and cases of the components / DBSCAN operators (deepmetv2_amd/components.py, csrc/components.hip;
include/dmet.h, "Components and DBSCAN").  numpy, scipy and sklearn on the host, no torch device.

Three statements of the same rules:
  * scipy: scipy.sparse.csgraph.connected_components (weak), every label replaced by the smallest id of its component;
  * loops: a plain union-find and the DBSCAN rule of the header in Python loops, with the events, masks and the entries
    that join nothing;
  * sklearn: sklearn.cluster.DBSCAN(eps=1.0, metric='precomputed') on a sparse matrix holding 0.5 at every entry, which
    hands sklearn exactly our entry set (sklearn adds the diagonal itself: a sample always counts itself).
tests/test_components_host.py holds them to each other on every case; tests/test_gpu_components.py holds the kernel to
them.  Everything is integer: equality, no tolerance."""
import math
import warnings

import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components as scipy_cc
from sklearn.cluster import DBSCAN

RAGGED_SIZES = [0, 1, 2, 63, 64, 65, 300, 1]
TABLE_WIDTHS = (1, 3, 16, 17, 64)
MIN_SAMPLES = (1, 2, 5, 17)


def ptr_of(sizes) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.int64)


def batch_of(sizes) -> np.ndarray:
    return np.repeat(np.arange(len(sizes), dtype=np.int64), np.asarray(sizes, dtype=np.int64))


class Graph:
    """Entries (tgt[e], src[e]) in the caller's order over the events `sizes`; row i = the entries with target i."""

    def __init__(self, name, sizes, tgt, src):
        self.name, self.sizes = name, list(sizes)
        self.tgt, self.src = np.asarray(tgt, dtype=np.int64), np.asarray(src, dtype=np.int64)
        self.N = int(sum(sizes))

    @property
    def edge_index(self) -> np.ndarray:
        """int64 [2, E], row 0 = source, row 1 = target (source_to_target)."""
        return np.stack([self.src, self.tgt])

    def rows(self) -> list:
        """Row i: the sources of the entries with target i, in the caller's order."""
        out = [[] for _ in range(self.N)]
        for t, s in zip(self.tgt.tolist(), self.src.tolist()):
            out[t].append(s)
        return out

    def grouped(self):
        """(rowptr[N + 1] int32, src[E] int32, tgt[E] int32, perm[E] int64): the stable grouping by target."""
        perm = np.argsort(self.tgt, kind="stable")
        rowptr = np.concatenate([[0], np.cumsum(np.bincount(self.tgt, minlength=self.N))]).astype(np.int32)
        return rowptr, self.src[perm].astype(np.int32), self.tgt[perm].astype(np.int32), perm

    def table(self, width: int, rng=None):
        """nbr[N, width] int32, -1 = empty.  rng None: every row packed to the left; else the entries of a row keep their
        order and the empty slots are dealt among them at random."""
        nbr = np.full((self.N, width), -1, dtype=np.int32)
        for i, r in enumerate(self.rows()):
            assert len(r) <= width, (self.name, i, len(r), width)
            slots = np.arange(len(r)) if rng is None else np.sort(rng.permutation(width)[:len(r)])
            nbr[i, slots] = r
        return nbr

    def counts(self) -> np.ndarray:
        return np.bincount(self.tgt, minlength=self.N).astype(np.int32)


# ---- the rules ------------------------------------------------------------------------------------------------------------------
def _joinable(t, s, ptr, N):
    """0: both ends in one event; 1: an end outside [0, N); 2: ends in two events."""
    if not (0 <= t < N and 0 <= s < N):
        return 1
    ev = np.searchsorted(ptr, [t, s], side="right")
    return 0 if ev[0] == ev[1] else 2


def cc_loops(N, tgt, src, ptr, edge_keep=None, node_keep=None):
    """(labels[N] int64, [entries outside the range, entries across two events]): a union-find in plain loops."""
    parent = list(range(N))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    bad = [0, 0]
    for e, (t, s) in enumerate(zip(np.asarray(tgt).tolist(), np.asarray(src).tolist())):
        kind = _joinable(t, s, ptr, N)
        if kind:
            bad[kind - 1] += 1
            continue
        if edge_keep is not None and not edge_keep[e]:
            continue
        if node_keep is not None and not (node_keep[t] and node_keep[s]):
            continue
        a, b = find(t), find(s)
        if a != b:
            parent[max(a, b)] = min(a, b)
    labels = np.array([find(i) for i in range(N)], dtype=np.int64)
    if node_keep is not None:
        labels[~np.asarray(node_keep, dtype=bool)] = -1
    return labels, bad


def cc_scipy(N, tgt, src) -> np.ndarray:
    """scipy's weak components of the entries (all of them in range), canonical: the smallest id of every component."""
    if N == 0:
        return np.zeros(0, dtype=np.int64)
    m = sp.coo_matrix((np.ones(len(tgt)), (np.asarray(tgt), np.asarray(src))), shape=(N, N)).tocsr()
    _n, lab = scipy_cc(m, directed=True, connection="weak")
    first = np.full(lab.max() + 1, N, dtype=np.int64)
    np.minimum.at(first, lab, np.arange(N))
    return first[lab]


def dbscan_loops(g: Graph, min_samples: int, count_self: bool):
    """(labels[N] int64 numbered over the batch, core[N] bool, clusters per event): the rule of the header in loops."""
    N, ptr, rows = g.N, ptr_of(g.sizes), g.rows()
    core = np.array([len(r) + (1 if count_self else 0) >= min_samples for r in rows], dtype=bool).reshape(N)
    keep = np.array([core[t] and core[s] for t, s in zip(g.tgt.tolist(), g.src.tolist())], dtype=bool)
    root, _bad = cc_loops(N, g.tgt, g.src, ptr, edge_keep=keep)
    labels = np.full(N, -1, dtype=np.int64)
    for i in range(N):
        if core[i]:
            labels[i] = root[i]
        else:
            near = [root[j] for j in rows[i] if core[j]]
            labels[i] = min(near) if near else -1
    roots = np.unique(root[core]) if core.any() else np.zeros(0, dtype=np.int64)
    number = {int(r): c for c, r in enumerate(roots)}
    labels = np.array([number[int(v)] if v >= 0 else -1 for v in labels], dtype=np.int64)
    per_event = [int(((roots >= ptr[b]) & (roots < ptr[b + 1])).sum()) for b in range(len(g.sizes))]
    return labels, core, per_event


def dbscan_sklearn_event(g: Graph, b: int, min_samples: int, count_self: bool):
    """(labels[n_b], core[n_b] bool) of sklearn on event b's entries.  sklearn counts a sample itself whatever the matrix
    holds, so a graph whose rows list themselves goes with count_self=False and one whose rows do not with True."""
    ptr = ptr_of(g.sizes)
    lo, n = int(ptr[b]), g.sizes[b]
    if n == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=bool)
    sel = (g.tgt >= lo) & (g.tgt < lo + n)
    t, s = g.tgt[sel] - lo, g.src[sel] - lo
    off = t != s                    # the diagonal is sklearn's own
    m = sp.coo_matrix((np.full(int(off.sum()), 0.5), (t[off], s[off])), shape=(n, n)).tocsr()
    assert m.data.size == 0 or m.data.max() == 0.5, "a duplicate entry: sklearn would add the two values up"
    has_self = np.bincount(t[~off], minlength=n) > 0
    assert not has_self.any() if count_self else has_self.all(), "rows list themselves exactly when count_self is False"
    with warnings.catch_warnings():                 # sklearn sorts the rows by value itself, and says so
        warnings.simplefilter("ignore")
        fit = DBSCAN(eps=1.0, min_samples=min_samples, metric="precomputed").fit(m)
    core = np.zeros(n, dtype=bool)
    core[fit.core_sample_indices_] = True
    return fit.labels_.astype(np.int64), core


def largest_loops(labels: np.ndarray, sizes, num_components: int) -> np.ndarray:
    """The bool mask of the num_components largest components of every event, size ties to the smaller root."""
    keep = np.zeros(len(labels), dtype=bool)
    ptr = ptr_of(sizes)
    for b in range(len(sizes)):
        ev = labels[ptr[b]:ptr[b + 1]]
        roots, count = np.unique(ev, return_counts=True)
        order = sorted(zip((-count).tolist(), roots.tolist()))[:num_components]
        keep[ptr[b]:ptr[b + 1]] = np.isin(ev, [r for _c, r in order])
    return keep


# ---- connected-components cases ---------------------------------------------------------------------------------------------------
def ragged(cut_last: bool = False) -> Graph:
    """The ragged batch [0, 1, 2, 63, 64, 65, 300, 1].  cut_last: without the last entry of the 64-node event, which joins
    its two 32-node paths (then two components of equal size)."""
    rng = np.random.default_rng(5)
    ptr = ptr_of(RAGGED_SIZES)
    tgt, src = [], []

    def add(b, t, s):
        tgt.append(int(ptr[b]) + int(t))
        src.append(int(ptr[b]) + int(s))

    add(1, 0, 0)                                            # the one-node event: a self entry
    # event 2 (two nodes): no entry at all
    pairs = rng.integers(0, 63, size=(40, 2))               # event 3: one direction only, duplicates, self entries
    for t, s in pairs:
        add(3, t, s)
    for t, s in pairs[:5]:
        add(3, t, s)
    for i in (4, 9, 60):
        add(3, i, i)
    for i in list(range(0, 31)) + list(range(32, 63)):      # event 4: two paths, each entry listed one way round
        add(4, i + 1, i)
    if not cut_last:
        add(4, 63, 5)                                       # ... joined by the event's last entry
    pairs = rng.integers(0, 50, size=(50, 2))               # event 5: both directions; nodes 50 .. 64 stay isolated
    for t, s in pairs:
        add(5, t, s)
        add(5, s, t)
    hub = 7                                                 # event 6: a hub whose row holds all 300 nodes, itself included
    for i in range(300):
        add(6, hub, i)
    for i in range(0, 300, 3):                              # ... a third of them list it back
        if i != hub:
            add(6, i, hub)
    # event 7 (one node): isolated
    return Graph("ragged_cut" if cut_last else "ragged", RAGGED_SIZES, tgt, src)


def bit_reversed_path(bits: int = 12) -> Graph:
    """One event, a path through all 2^bits nodes whose ids are bit-reversed along the path: neighbours on the path are far
    apart in id, and min-label propagation would need a round per node."""
    n = 1 << bits
    order = np.array([int(format(i, f"0{bits}b")[::-1], 2) for i in range(n)], dtype=np.int64)
    return Graph(f"path{n}", [n], order[1:], order[:-1])


def width_graph(width: int) -> Graph:
    """A random graph over the ragged batch whose rows hold at most `width` entries (rows of every length 0 .. width
    occur), entries inside their event, duplicates and self entries allowed."""
    rng = np.random.default_rng(100 + width)
    ptr = ptr_of(RAGGED_SIZES)
    tgt, src = [], []
    for b, n in enumerate(RAGGED_SIZES):
        for i in range(n):
            # sparse enough that an event stays in several components
            c = int(rng.integers(0, width + 1)) if rng.random() < min(1.0, 1.5 / max(width, 1)) or i % 29 == 0 else 0
            if n > 1 and i == n - 1:
                c = width                                   # the event's last row is full: its last slot is the last entry
            for s in rng.integers(0, n, size=c):
                tgt.append(int(ptr[b]) + i)
                src.append(int(ptr[b]) + int(s))
    return Graph(f"width{width}", RAGGED_SIZES, tgt, src)


def cc_graphs() -> list:
    return [ragged(), ragged(cut_last=True), bit_reversed_path()] + [width_graph(w) for w in TABLE_WIDTHS]


def bad_entry_graphs() -> list:
    """(graph, [entries outside the range, entries across events]): the ragged batch plus entries that join nothing.  The
    targets stay in range (a row exists for them); the sources do not."""
    base = ragged()
    ptr = ptr_of(RAGGED_SIZES)
    out = []
    lo3, lo4, lo6 = int(ptr[3]), int(ptr[4]), int(ptr[6])
    for name, extra, bad in (
            ("range", [(lo3 + 1, base.N), (lo6 + 299, -2), (lo4 + 3, base.N + 7)], [3, 0]),
            ("cross", [(lo3 + 1, lo4 + 1), (lo6 + 5, lo3 + 5)], [0, 2])):
        t = np.concatenate([base.tgt, [e[0] for e in extra]])
        s = np.concatenate([base.src, [e[1] for e in extra]])
        out.append((Graph("ragged_" + name, RAGGED_SIZES, t, s), bad))
    return out


def masks(g: Graph):
    """(edge_keep[E] bool in the caller's order, node_keep[N] bool), fixed and about half / three quarters True."""
    rng = np.random.default_rng(9)
    return rng.random(len(g.tgt)) < 0.5, rng.random(g.N) < 0.75


# ---- DBSCAN-over-a-graph cases -------------------------------------------------------------------------------------------------
DBSCAN_SIZES = [13, 9, 20, 0, 80, 1]


def dbscan_graph_case(with_self: bool) -> Graph:
    """A symmetric graph without duplicate entries; with_self: every row lists its own node (count_self=False), else no
    row does (count_self=True).
      event 0: two 6-cliques (0 .. 5, 7 .. 12) and node 6 between them, adjacent to 5 and 7: a border node of two clusters
               at min_samples = 5;
      event 1: two pairs and five isolated nodes: noise only from min_samples = 3 on;
      event 2: a 20-clique: one cluster at every min_samples up to 20;
      event 3: no node; event 4: 80 points in the plane joined within a radius; event 5: one node."""
    ptr = ptr_of(DBSCAN_SIZES)
    und = set()

    def link(b, i, j):
        if i != j:
            und.add((int(ptr[b]) + min(i, j), int(ptr[b]) + max(i, j)))

    for base in (0, 7):
        for i in range(6):
            for j in range(i + 1, 6):
                link(0, base + i, base + j)
    link(0, 6, 5)
    link(0, 6, 7)
    link(1, 0, 1)
    link(1, 4, 5)
    for i in range(20):
        for j in range(i + 1, 20):
            link(2, i, j)
    rng = np.random.default_rng(17)
    xy = rng.random((80, 2))
    d2 = ((xy[:, None, :] - xy[None, :, :]) ** 2).sum(-1)
    for i, j in zip(*np.nonzero(d2 < 0.16 ** 2)):
        link(4, int(i), int(j))
    tgt, src = [], []
    for a, b in sorted(und):
        tgt += [a, b]
        src += [b, a]
    if with_self:
        N = int(ptr[-1])
        tgt += list(range(N))
        src += list(range(N))
    order = np.random.default_rng(3).permutation(len(tgt))         # the caller's order is no particular order
    return Graph("dbscan_self" if with_self else "dbscan_noself", DBSCAN_SIZES, np.array(tgt)[order], np.array(src)[order])


# ---- DBSCAN over positions ------------------------------------------------------------------------------------------------------
class Points:
    """pos[N, D] float64 on the lattice of multiples of 1/8, eps = sqrt(m + 0.5) / 8: every squared distance is a multiple
    of 1/64 and none is eps^2, so neither the rounding of a distance nor `<` against `<=` can matter."""

    def __init__(self, name, sizes, pos, m, min_samples, max_num_neighbors, overflows=False):
        self.name, self.sizes, self.pos, self.m = name, list(sizes), np.asarray(pos, dtype=np.float64), m
        self.eps = math.sqrt(m + 0.5) / 8
        self.min_samples, self.max_num_neighbors, self.overflows = min_samples, max_num_neighbors, overflows

    def neighbour_counts(self) -> np.ndarray:
        """Points within eps of every point, itself included, inside its event (exact integer arithmetic)."""
        q = np.rint(self.pos * 8).astype(np.int64)
        ptr = ptr_of(self.sizes)
        out = np.zeros(len(q), dtype=np.int64)
        for b in range(len(self.sizes)):
            e = q[ptr[b]:ptr[b + 1]]
            d2 = ((e[:, None, :] - e[None, :, :]) ** 2).sum(-1)
            out[ptr[b]:ptr[b + 1]] = (2 * d2 < 2 * self.m + 1).sum(1)
        return out

    def sklearn_event(self, b: int):
        ptr = ptr_of(self.sizes)
        e = self.pos[ptr[b]:ptr[b + 1]]
        if len(e) == 0:
            return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=bool)
        fit = DBSCAN(eps=self.eps, min_samples=self.min_samples).fit(e)
        core = np.zeros(len(e), dtype=bool)
        core[fit.core_sample_indices_] = True
        return fit.labels_.astype(np.int64), core


def _lattice(rng, n, D, side):
    return rng.integers(0, side, size=(n, D)) / 8.0


def point_cases() -> list:
    rng = np.random.default_rng(23)
    out = []
    sizes = [70, 1, 0, 130]
    out.append(Points("plane", sizes, _lattice(rng, sum(sizes), 2, 12), 4, 5, 64))
    sizes = [90, 150]
    out.append(Points("space", sizes, _lattice(rng, sum(sizes), 3, 8), 2, 4, 64))
    # eight points on one spot, far from the rest: their rows hold exactly max_num_neighbors = 8 hits, one slot stays free
    far = _lattice(rng, 40, 2, 16) + 4.0
    out.append(Points("exactly_full", [48], np.concatenate([np.zeros((8, 2)), far]), 4, 5, 8))
    # nine on one spot: more than max_num_neighbors within eps, the rows fill every slot
    out.append(Points("overflow", [49], np.concatenate([np.zeros((9, 2)), far]), 4, 5, 8, overflows=True))
    return out


def periodic_case():
    """(x[N, 2] float32 (eta, phi), sizes, eps, min_samples, period): points on both sides of the phi seam; the reference
    is the rule run on the graph of tests/radius_periodic_reference.py."""
    rng = np.random.default_rng(31)
    sizes = [120, 60]
    N = sum(sizes)
    eta = rng.normal(0.0, 0.6, N)
    phi = np.where(rng.random(N) < 0.7, math.pi - np.abs(rng.normal(0.0, 0.25, N)), rng.uniform(-math.pi, math.pi, N))
    phi = np.where(rng.random(N) < 0.5, phi, -phi)
    x = np.stack([eta, phi], 1).astype(np.float32)
    x[:, 1] = np.clip(x[:, 1], -np.float32(3.1415925), np.float32(3.1415925))
    return x, sizes, 0.2, 5, [None, 2 * math.pi]
