"""TEST INFRASTRUCTURE for tests/test_gpu_softmax_nonfinite.py, tests/test_gpu_aggregate_nonfinite.py and
tests/test_nonfinite_contract_host.py: the cases and helpers that hold the fused aggregations to the non-finite contract of
include/dmet.h ("Non-finite values in the fused aggregations") and DESIGN.md.

ENTRIES names every aggregation entry of deepmetv2_amd/_native.py and the lanes it is held to here, or says why not.

Softmax lanes.  A row is written as a list of (mark, count): D a dead source (score -inf), L a live one, P a score of +inf,
N a NaN score, E an empty slot, S (self_loops only) a written entry i -> i.  c is the chunk length of the kernels: 16 at
(H, C) = (2, 8), 32 at (1, 40).  One graph of 150 nodes holds the rows of several cases, each at a target of its own, and a
background row of three live sources at every other node; the "finite" graph holds the cases whose reference is finite, the
"nan" graph those whose row is NaN, so that on the finite graph every reference gradient of GAT v1 is finite and the
backward comparison discriminates.  Nodes 0..69 are dead sources, 70 carries +inf, 71 NaN, 72..149 are live.  The special
value sits in the operand the score is formed from, so the float64 reference sees the same scores:
    attention   k[j, :, 0] with q[:, :, 0] = 1 (v stays finite)
    gat_v1      s_src[j]
    gat_v2      xl[j, :, 0] with att[:, 0] > 0 and slope 0.2 (channel 0 of out is 0 * -inf = NaN in kernel and reference)
Finite elements are held to the operators' own bars (attention_reference.assert_output_bar / assert_grad_bar); an output
row's bar is formed from the finite values of the entries that carry weight (weight_bar).
"""
from __future__ import annotations

import math

import numpy as np
import torch

import attention_reference as ar
import gat_reference as gr

INF, NAN = float("inf"), float("nan")

# entry of _native.py -> the lanes held here, or why none
ENTRIES = {
    "attention_fwd": "softmax lanes and the value sums: tests/test_gpu_softmax_nonfinite.py",
    "gat_fwd": "softmax lanes and the value sums, both modes, self loops: tests/test_gpu_softmax_nonfinite.py",
    "multi_aggr_fwd": "sum, max / min and clamp lanes, locality: tests/test_gpu_aggregate_nonfinite.py",
    "interpolate_fwd": "sum and clamp lanes, locality: tests/test_gpu_aggregate_nonfinite.py",
    "weighted_sum_fwd": "sum lanes, locality: tests/test_gpu_aggregate_nonfinite.py",
    "gravnet_fwd": "the mean half as a sum lane, the max half as a max lane, locality: tests/test_gpu_aggregate_nonfinite.py",
    "pointnet_fwd": "its out as a max lane, locality: tests/test_gpu_aggregate_nonfinite.py",
}


# ---- comparison helpers -----------------------------------------------------------------------------------------------------
def same_nonfinite(got, ref, what=""):
    """Equal NaN masks, and where the reference is +-inf the same infinity (tests/test_gpu_segment_reduce.py)."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.equal(got.isnan(), ref.isnan()), (what, "NaN masks differ", int(got.isnan().sum()), int(ref.isnan().sum()))
    inf = ref.isinf()
    assert torch.equal(got.isinf(), inf) and torch.equal(got[inf], ref[inf]), (what, "infinities differ")


def finite_pair(got, ref):
    """(got, ref) in float64 with 0 in both where the reference is not finite: what a bar is applied to after
    same_nonfinite has held the rest."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    ok = ref.isfinite()
    return torch.where(ok, got, torch.zeros_like(got)), torch.where(ok, ref, torch.zeros_like(ref))


def check_output(got, ref, bar, what=""):
    same_nonfinite(got, ref, what)
    assert bool(bar.isfinite().all()), (what, "bar")
    ar.assert_output_bar(*finite_pair(got, ref), bar, what)


def check_grad(got, ref, what=""):
    """same_nonfinite, then assert_grad_bar over the finite elements (max|ref| over those)."""
    same_nonfinite(got, ref, what)
    ok = ref.detach().cpu().isfinite()
    scale = float(ref.detach().cpu()[ok].abs().max()) if bool(ok.any()) else 0.0
    assert math.isfinite(scale), what
    ar.assert_grad_bar(got.detach().cpu()[ok], ref.detach().cpu()[ok], what)


def weight_bar(values, tgt, src, alpha, num_targets):
    """bar[i] = the largest finite |values_j| over the entries of row i whose reference weight is above 0 in any head."""
    v = values.detach().double().flatten(1)
    vinf = torch.where(v.isfinite(), v.abs(), torch.zeros_like(v)).amax(1)
    carries = (torch.nan_to_num(alpha.detach().double(), nan=0.0) > 0).any(-1)
    return torch.zeros(num_targets, dtype=torch.float64).scatter_reduce(0, tgt[carries], vinf[src[carries]], "amax",
                                                                       include_self=True)


# ---- max / min under the house rule -----------------------------------------------------------------------------------------
def _nan_skipping(values, valid, sign):
    """values[..., k] float64, valid[..., k] bool -> (value, position): the max (sign +1) or min (-1) over the valid
    candidates that are numbers, +-inf included, at its lowest position; NaN and -1 where a row has valid candidates and
    all are NaN; 0 and -1 where it has none (R3)."""
    values = values.double()
    num = valid & ~values.isnan()
    key = torch.where(num, sign * values, torch.full_like(values, -INF))
    best = key.amax(-1, keepdim=True)
    hit = num & (key == best)
    k = values.shape[-1]
    slots = torch.arange(k).expand_as(values)
    pos = torch.where(hit, slots, torch.full_like(slots, k)).amin(-1)
    any_num, any_valid = num.any(-1), valid.any(-1)
    val = torch.where(any_num, sign * best.squeeze(-1), torch.full_like(best.squeeze(-1), NAN))
    val = torch.where(any_valid, val, torch.zeros_like(val))
    return val, torch.where(any_num, pos, torch.full_like(pos, -1))


def nan_skipping_max(values, valid):
    return _nan_skipping(values, valid, 1.0)


def nan_skipping_min(values, valid):
    return _nan_skipping(values, valid, -1.0)


# ---- softmax placement cases ------------------------------------------------------------------------------------------------
NODES = 150
DEAD = list(range(0, 70))
POS_NODE, NAN_NODE = 70, 71
LIVE = list(range(72, NODES))
CHUNKS = {16: (2, 8), 32: (1, 40)}      # chunk length -> (H, C)
TABLE_K = {16: 40, 32: 64}
SLOPE = 0.2
OPS = ("attention", "gat_v1", "gat_v2")


def softmax_rows(c):
    """case -> (row as [(mark, count)], "finite" | "nan", self_loops).  S11 at c = 32 and k = 64: a run of c empty slots and
    a run of c dead entries leave no slot for a live one, so the second run is one shorter and one live entry follows."""
    k = TABLE_K[c]
    rest = k - 2 * c
    rows = {
        "S1": ([("D", c), ("L", 1)], "finite", False),
        "S2": ([("D", c), ("L", 5)], "finite", False),
        "S3": ([("D", 2 * c), ("L", 3)], "finite", False),
        "S4": ([("L", c), ("D", c), ("L", 2)], "finite", False),
        "S5": ([("L", 3), ("D", c - 3), ("D", c)], "finite", False),
        "S6": ([("D", c - 1), ("L", 1), ("D", c + 2)], "finite", False),
        "S7": ([("D", 2 * c + 1)], "nan", False),
        "S8": ([("N", 1), ("D", c - 1), ("L", 4)], "nan", False),
        "S9": ([("L", c), ("P", 1)], "nan", False),
        "S10": ([("L", c), ("N", 1)], "nan", False),
        "S11 empty, dead, live": ([("E", c), ("D", c if rest else c - 1), ("L", rest or 1)], "finite", False),
        "S11 dead, empty, live": ([("D", c), ("E", c if rest else c - 1), ("L", rest or 1)], "finite", False),
        "S12 dead row, live self": ([("D", c)], "finite", True),
        "S12 written self among the dead": ([("D", c // 2), ("S", 1), ("D", c - c // 2)], "finite", True),
        "S12 dead row, dead self": ([("D", c)], "nan", True),
    }
    return rows


def softmax_graph(c, which, self_loops=False):
    """The graph of the cases of one kind: dict(rows={target: [ids, -1 = empty]}, target={case: target}, k=table width).
    Every case sits at a live target of its own (the dead-self case at dead node 69) and draws distinct sources in the
    written order; every other node lists three live sources."""
    rows, target = {}, {}
    cases = [(n, r) for n, (r, w, s) in softmax_rows(c).items() if w == which and s == self_loops]
    for at, (name, row) in enumerate(cases):
        t = DEAD[69] if name.endswith("dead self") else LIVE[at]
        d, l, ids = 0, 0, []
        for mark, count in row:
            for _ in range(count):
                if mark == "D":
                    ids.append(DEAD[d]); d += 1
                elif mark == "L":
                    ids.append(LIVE[20 + (at * 5 + l) % (len(LIVE) - 20)]); l += 1
                else:
                    ids.append({"P": POS_NODE, "N": NAN_NODE, "E": -1, "S": t}[mark])
        assert d <= 69
        rows[t], target[name] = ids, t
    for t in range(NODES):
        if t not in rows:
            rows[t] = [LIVE[(7 * t + r * 11) % len(LIVE)] for r in range(3)]
            if self_loops:      # a written self loop would be skipped: keep the background rows three entries long
                rows[t] = [j if j != t else LIVE[(j - LIVE[0] + 1) % len(LIVE)] for j in rows[t]]
    return dict(rows=rows, target=target, k=TABLE_K[c], c=c, self_loops=self_loops)


def list_form(graph):
    """(tgt, src) int64 of the valid entries, rows in target order, entries in the written order."""
    tgt = [t for t in sorted(graph["rows"]) for j in graph["rows"][t] if j >= 0]
    src = [j for t in sorted(graph["rows"]) for j in graph["rows"][t] if j >= 0]
    return torch.tensor(tgt, dtype=torch.int64), torch.tensor(src, dtype=torch.int64)


def table_form(graph):
    """(nbr[NODES, k] int32, the cases whose row fits k): a longer row is left empty, -1 pads the others at the end."""
    k = graph["k"]
    nbr = torch.full((NODES, k), -1, dtype=torch.int32)
    for t, ids in graph["rows"].items():
        if len(ids) <= k:
            nbr[t, :len(ids)] = torch.tensor(ids, dtype=torch.int32)
    fits = [n for n, t in graph["target"].items() if len(graph["rows"][t]) <= k]
    return nbr, fits


def softmax_inputs(op, c, all_live=False, self_loops=False, seed=0):
    """fp32 CPU operands of `op` in the order its aggregate takes them.  all_live: the control, no special value.
    self_loops: every node is an entry of its own row, so only the dead nodes carry a special value."""
    H, C = CHUNKS[c]
    g = torch.Generator().manual_seed(900 + 10 * c + seed)
    special = [] if all_live else [(DEAD, -INF)] if self_loops else [(DEAD, -INF), ([POS_NODE], INF), ([NAN_NODE], NAN)]
    if op == "attention":
        q, k, v = ar.qkv(NODES, NODES, H, C, seed=900 + c)
        q[:, :, 0] = 1.0
        for nodes, val in special:
            k[nodes, :, 0] = val
        return q, k, v
    if op == "gat_v1":
        xl = torch.randn(NODES, H, C, generator=g)
        s_src, s_dst = torch.randn(NODES, H, generator=g), torch.randn(NODES, H, generator=g)
        for nodes, val in special:
            s_src[nodes] = val
        return xl, s_src, s_dst
    assert op == "gat_v2"
    xl = torch.randn(NODES, H, C, generator=g)
    xr = 0.5 * torch.randn(NODES, H, C, generator=g)
    att = torch.randn(H, C, generator=g) / math.sqrt(C)
    att[:, 0] = 0.25 + att[:, 0].abs()
    for nodes, val in special:
        xl[nodes, :, 0] = val
    return xl, xr, att


def softmax_scores(op, ins, tgt, src):
    if op == "attention":
        q, k, _v = ins
        return (q[tgt] * k[src]).sum(-1) / math.sqrt(q.shape[2])
    if op == "gat_v1":
        _xl, s_src, s_dst = ins
        return torch.nn.functional.leaky_relu(s_src[src] + s_dst[tgt], SLOPE)
    xl, xr, att = ins
    return (torch.nn.functional.leaky_relu(xl[src] + xr[tgt], SLOPE) * att.reshape(1, *xl.shape[1:])).sum(-1)


def softmax_reference(op, ins, tgt, src, self_loops=False, num_targets=NODES):
    """The operator's float64 reference as it is over the entries: dict(out, alpha (written entries kept under self_loops,
    then the self entries), lse, bar, tgt, src (the entries it ran over)).  ins: float64 leaves (requires_grad or not)."""
    if self_loops:
        tgt, src = gr.with_self_loops(tgt, src, num_targets)
    if op == "attention":
        out, alpha, _bar = ar.attention(*ins, tgt, src)
        values = ins[2]
    else:
        out, alpha, _bar = gr.run(gr.V1 if op == "gat_v1" else gr.V2, *ins, tgt, src, SLOPE)
        values = ins[0]
    with torch.no_grad():
        score = softmax_scores(op, [t.detach() for t in ins], tgt, src)
        H = score.shape[1]
        m = torch.full((num_targets, H), -INF, dtype=score.dtype).scatter_reduce(0, tgt.view(-1, 1).expand(-1, H), score,
                                                                                "amax", include_self=True)
        l = torch.zeros((num_targets, H), dtype=score.dtype).index_add(0, tgt, torch.exp(score - m[tgt]))
        lse = m + torch.log(l)
        lse[torch.bincount(tgt, minlength=num_targets) == 0] = 0.0      # a row without an entry (R3)
        bar = weight_bar(values, tgt, src, alpha, num_targets)
    return dict(out=out, alpha=alpha, lse=lse, bar=bar, tgt=tgt, src=src)


# ---- the chunked running softmax in fp32, three forms ----------------------------------------------------------------------
def row_scores(row, seed=0):
    """(score[n], valid[n], value[n]) float32 of a written row: L a seeded normal, D -inf, P +inf, N NaN; E invalid."""
    rng = np.random.default_rng(seed)
    marks = [m for m, count in row for _ in range(count)]
    s = rng.standard_normal(len(marks)).astype(np.float32)
    for t, m in enumerate(marks):
        if m in "DPN":
            s[t] = {"D": -np.inf, "P": np.inf, "N": np.nan}[m]
    return s, np.array([m != "E" for m in marks]), rng.standard_normal(len(marks)).astype(np.float32)


def chunked_softmax(score, valid, value, c, form):
    """(out, lse, alpha[n]) float32 of the kernels' recurrence over chunks of c entries with one value channel.
    form "parent": rescale by expf(m - m_new) once a valid entry was seen, p = expf(s - m_new) for every valid entry;
    "restart": the parent's, with the state set to zero at a chunk that starts while m == -inf; "contract": a score of
    -inf weighs exactly 0, the state is multiplied by 0 while m == -inf, and a row that ends with m == -inf is NaN."""
    f = np.float32
    m, l, acc, cnt = f(-np.inf), f(0), f(0), 0
    with np.errstate(all="ignore"):
        for base in range(0, len(score), c):
            s, ok, v = score[base:base + c], valid[base:base + c], value[base:base + c]
            if not ok.any():
                continue
            m_new = np.fmax(m, np.fmax.reduce(np.where(ok, s, f(-np.inf))))       # fmaxf drops a NaN
            if form == "restart" and m == -np.inf:
                l, acc, cnt = f(0), f(0), 0
            if form == "contract":
                scale = f(0) if m == -np.inf else np.exp(m - m_new)
                p = np.where(ok & (s != -np.inf), np.exp(s - m_new), f(0)).astype(f)
            else:
                scale = f(0) if cnt == 0 else np.exp(m - m_new)
                p = np.where(ok, np.exp(s - m_new), f(0)).astype(f)
            m, l, acc = m_new, f(l * scale), f(acc * scale)
            for e in np.flatnonzero(ok):
                l, acc, cnt = f(l + p[e]), f(acc + p[e] * v[e]), cnt + 1
        if cnt == 0:
            return f(0), f(0), np.zeros(len(score), f)
        if form == "contract" and m == -np.inf:
            l = f(np.nan)
        return f(acc / l), f(m + np.log(l)), np.where(valid, np.exp(score - m) / l, f(0)).astype(f)


def softmax_f64(score, valid, value):
    """torch.softmax of the valid scores in float64: (out, lse, alpha[n])."""
    s = torch.from_numpy(score.astype(np.float64))[torch.from_numpy(valid)]
    if s.numel() == 0:
        return 0.0, 0.0, np.zeros(len(score))
    a = torch.softmax(s, 0)
    alpha = np.zeros(len(score))
    alpha[valid] = a.numpy()
    lse = float(torch.logsumexp(s, 0)) if bool(a.isfinite().all()) else NAN
    return float((a * torch.from_numpy(value.astype(np.float64))[torch.from_numpy(valid)]).sum()), lse, alpha


# ---- max / min, clamp and locality cases ------------------------------------------------------------------------------------
# One event of 48 nodes and hand-built tables of width 8 (one chunk) and 40 (more than one chunk at every group width up to
# 32).  Source J is poisoned in one feature.  J is listed by the rows LISTING (J and 7 or 39 distinct companions out of the
# nodes 0..39) and by ALL_J, whose every slot holds J; the nodes 40..47 never share a row with J; a few other rows end in
# empty slots and row 47 is empty.  `rotate` rolls the rows of LISTING so that J stands in a given slot.
AGG_N = 48
J = 5
FEATURE = 1              # the poisoned feature (PointNet: input feature)
LISTING = (2, 9, 17, 33, 41)
ALL_J = 20
WIDTHS = (8, 40)
PLACEMENTS = {8: (0, 1, 7), 40: (0, 1, 15, 16, 31, 32, 39)}       # slot 0, 1, c-1, c (c = 16, 32) and k-1
POISONS = {"nan": NAN, "+inf": INF, "-inf": -INF}
AGG_OPS = ("gravnet", "pna", "pointnet", "interpolate", "weighted_sum")
PNA_AGGRS = ("sum", "mean", "min", "max", "var", "std")
# widths from the operators' smallest existing cases that still have a channel beside the poisoned one
GRAVNET_SP = (3, 22)                                      # tests/test_gpu_gravnet.py "two slot chunks on 16 lanes"
POINTNET = dict(F=3, D=2, H1=12, H2=16, act="elu", act2=False)     # tests/pointnet_cases.py "options elu act2=False bias=True"
FEATURES = 5                                              # pna, interpolate, weighted sum: the tests' odd width


def agg_table(k, seed=0):
    """(nbr[48, k] int32, dist[48, k] fp32): see above.  dist is 1e10 in an empty slot, as knn_table leaves it."""
    g = torch.Generator().manual_seed(700 + k + seed)
    companions = [n for n in range(40) if n != J]
    nbr = torch.full((AGG_N, k), -1, dtype=torch.int32)
    for i in range(AGG_N):
        if i == ALL_J:
            nbr[i] = J
        elif i in LISTING:
            pick = [companions[p] for p in torch.randperm(39, generator=g)[:k - 1].tolist()] + [J]
            nbr[i] = torch.tensor(pick, dtype=torch.int32)[torch.randperm(k, generator=g)]
        elif i != AGG_N - 1:
            rest = companions + list(range(40, AGG_N))
            nbr[i] = torch.tensor([rest[p] for p in torch.randperm(47, generator=g)[:k].tolist()], dtype=torch.int32)
            if i % 6 == 1:
                nbr[i, k - 3:] = -1
    dist = 0.05 + torch.rand(AGG_N, k, generator=g)
    dist[nbr < 0] = 1e10
    return nbr, dist


def rotate(nbr, dist, slot):
    """(nbr, dist, shift[48]) with the rows of LISTING rolled so that J stands in `slot`: entry t moves to (t + shift) % k."""
    nbr, dist = nbr.clone(), dist.clone()
    k = nbr.shape[1]
    shift = torch.zeros(AGG_N, dtype=torch.int64)
    for i in LISTING:
        at = (nbr[i] == J).nonzero().flatten()
        assert at.numel() == 1
        shift[i] = (slot - int(at)) % k
        nbr[i], dist[i] = nbr[i].roll(int(shift[i])), dist[i].roll(int(shift[i]))
    return nbr, dist, shift


def agg_masks(nbr):
    """(rows listing J, sources sharing a row with J (J included), nodes that as a source share no row with J and as a
    target do not list it) as bool [48], from the table."""
    lists = (nbr == J).any(1)
    shares = torch.zeros(AGG_N, dtype=torch.bool)
    ids = nbr[lists].flatten().long()
    shares[ids[ids >= 0]] = True
    apart = ~shares & ~lists
    for m in (lists, shares, apart):
        assert 0 < int(m.sum()) < AGG_N
    return lists, shares, apart


# seeds at which no two candidates of a max lane are close enough for the winner to depend on fp32 rounding: the top two
# GravNet messages of every (row, channel) differ by more than 1e-3 of the larger (a message carries a few ulp of its own
# size: expf, and 10 d times the rounding of d), and the PointNet reference has no fragile element; the host test asserts both
AGG_SEED = {"gravnet": 2, "pointnet": 1}


def agg_inputs(op, poison=None, seed=None):
    """fp32 CPU inputs of `op` as a dict; poison: None (the clean run) or a value written to feature FEATURE of source J."""
    g = torch.Generator().manual_seed(800 + AGG_OPS.index(op) + (AGG_SEED.get(op, 0) if seed is None else seed))
    if op == "gravnet":
        S, P = GRAVNET_SP
        d = dict(h=torch.randn(AGG_N, P, generator=g), s=0.3 * torch.randn(AGG_N, S, generator=g))
        key = "h"
    elif op == "pointnet":
        c = POINTNET
        d = dict(x=torch.randn(AGG_N, c["F"], generator=g), pos=torch.randn(AGG_N, c["D"], generator=g),
                 W1=torch.randn(c["H1"], c["F"] + c["D"], generator=g) / (c["F"] + c["D"]) ** 0.5,
                 b1=0.5 * torch.randn(c["H1"], generator=g), W2=torch.randn(c["H2"], c["H1"], generator=g) / c["H1"] ** 0.5,
                 b2=0.5 * torch.randn(c["H2"], generator=g))
        key = "x"
    else:
        d = dict(x=torch.randn(AGG_N, FEATURES, generator=g))
        key = "x"
    if poison is not None:
        d[key] = d[key].clone()
        d[key][J, FEATURE] = poison
    return d


def agg_reference(op, d, nbr, dist=None, w=None):
    """The operator's float64 reference as it is, over the table: a dict of float64 lanes (and int64 winners).
    gravnet: mean, max, arg (slot, 255 none), bar;  pna: the six statistics, argmin, argmax (positions), bounds;
    pointnet: out, win (slot, -1 none), scale;  interpolate: out, wsum, bar;  weighted_sum: out, bound."""
    import gravnet_reference as gvr
    import interpolate_reference as ir
    import pna_reference as pr
    import pointnet_reference as pnr
    import weighted_sum_reference as wr
    k = nbr.shape[1]
    if op == "gravnet":
        h, s = d["h"].double(), d["s"].double()
        out, _bar, _msg, valid, own = gvr.aggregate(h, s, nbr)
        P = h.shape[1]
        hinf = torch.where(h.isfinite(), h.abs(), torch.zeros_like(h)).amax(1)          # the bar of the finite values
        bar = torch.where(valid, hinf[nbr.long().clamp(min=0)], torch.zeros((), dtype=torch.float64)).sum(1)
        return dict(mean=out[:, :P], max=out[:, P:], arg=torch.where(own >= k, torch.full_like(own, 255), own), bar=bar)
    if op == "pna":
        pos = pr.positions_of_table(nbr, AGG_N)
        ref = pr.stats(d["x"], *pos, AGG_N)
        ref["bounds"] = pr.bounds(ref)
        return ref
    if op == "pointnet":
        c = POINTNET
        entries = pnr.entries_from_table(nbr, AGG_N, None, False)
        r = pnr.Reference(d["x"], d["pos"], d["pos"], d["W1"], d["b1"], d["W2"], d["b2"], c["act"], c["act2"], entries, AGG_N)
        fin = r.out[r.out.isfinite()]
        return dict(out=r.out, win=r.win, scale=float(fin.abs().max()), fragile=r.fragile, ref=r)
    if op == "interpolate":
        out, _bar, wsum, valid = ir.interpolate(d["x"].double(), nbr, dist)
        x = d["x"].double()
        r, _W, _valid, j = ir.weights(nbr, dist, AGG_N)
        fin = torch.where(x.isfinite(), x.abs(), torch.zeros_like(x))[j] * valid.unsqueeze(-1)
        bar = (torch.nan_to_num(r, nan=0.0).unsqueeze(-1) * fin).sum(1)
        return dict(out=out, wsum=wsum, bar=bar)
    assert op == "weighted_sum"
    pos = wr.positions_of_table(nbr, AGG_N)
    out, count, bound = wr.forward(d["x"], w, *pos, AGG_N)
    return dict(out=out, count=count, bound=bound)
