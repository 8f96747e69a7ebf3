"""The cases of tests/test_gpu_pointnet.py, their inputs and the seed search: shared with tests/test_pointnet_host.py, which
shows on a brute-force float64 graph that every case finds a seed without fragile elements.

A case: sources per event `src`, targets per event `dst` (None: one node set), widths F, D, H1, H2, the graph
(`graph`: 'knn' k / 'radius' r over max slots / 'list' in-degrees), act, act2, bias, self loops.  Inputs are drawn on the
CPU from torch.Generator(seed), the same numbers on every machine."""
import torch

import pointnet_reference as pr

TRIES = 32

CASES = {
    "smallest": dict(src=[1], dst=None, F=0, D=1, H1=1, H2=16, graph=("knn", 1), act="relu", act2=False, self_loop=True),
    "no features": dict(src=[20, 9], dst=None, F=0, D=3, H1=8, H2=16, graph=("knn", 4), act="relu", act2=False,
                        self_loop=True),
    "set abstraction": dict(src=[40, 7], dst=[10, 2], F=13, D=3, H1=64, H2=128, graph=("knn", 16), act="relu", act2=False,
                            self_loop=False),
    "empty events": dict(src=[5, 0, 9], dst=[3, 4, 0], F=6, D=3, H1=16, H2=32, graph=("knn", 3), act="relu", act2=True,
                         self_loop=False),
    "limits": dict(src=[6], dst=[5], F=128, D=8, H1=128, H2=128, graph=("knn", 64), act="elu", act2=True, self_loop=False),
    # in-degrees one below, at and one above the 16-entry tile, a hub over more than two tiles, empty and short rows; 24
    # targets are six workgroups of four wavefronts
    "tile edges": dict(src=[50], dst=[24], F=5, D=2, H1=20, H2=32,
                       graph=("list", [15, 16, 17, 40, 0, 1, 33, 2] + [3, 0, 5, 16] * 4), act="relu", act2=False,
                       self_loop=False),
    "radius": dict(src=[30, 12], dst=[8, 5], F=4, D=2, H1=16, H2=16, graph=("radius", 1.0, 12), act="elu", act2=False,
                   self_loop=False),
    "one set": dict(src=[25, 8], dst=None, F=7, D=3, H1=24, H2=32, graph=("knn", 5), act="elu", act2=True, self_loop=True),
}
for _a in ("relu", "elu"):
    for _a2 in (False, True):
        for _b in (True, False):
            CASES[f"options {_a} act2={_a2} bias={_b}"] = dict(src=[14, 6], dst=[5, 3], F=3, D=2, H1=12, H2=16,
                                                               graph=("knn", 4), act=_a, act2=_a2, bias=_b, self_loop=False)


def sizes(case):
    c = CASES[case]
    return sum(c["src"]), sum(c["src"] if c["dst"] is None else c["dst"])


def batch_of(counts):
    return torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts, dtype=torch.int64))


def make_inputs(case, seed):
    """CPU fp32: dict(x or None, pos_src, pos_dst (pos_src itself for one set), W1, b1, W2, b2, batch_src, batch_dst)."""
    c = CASES[case]
    g = torch.Generator().manual_seed(1000 * seed + len(case))
    Ns, Nt = sizes(case)
    F, D, H1, H2 = c["F"], c["D"], c["H1"], c["H2"]
    x = torch.randn(Ns, F, generator=g) if F else None
    pos_src = torch.randn(Ns, D, generator=g)
    pos_dst = pos_src if c["dst"] is None else torch.randn(Nt, D, generator=g)
    W1 = torch.randn(H1, F + D, generator=g) / (F + D) ** 0.5
    W2 = torch.randn(H2, H1, generator=g) / H1 ** 0.5
    bias = c.get("bias", True)
    b1 = torch.randn(H1, generator=g) * 0.5 if bias else None
    b2 = torch.randn(H2, generator=g) * 0.5 if bias else None
    out = dict(x=x, pos_src=pos_src, pos_dst=pos_dst, W1=W1, b1=b1, W2=W2, b2=b2, batch_src=batch_of(c["src"]),
               batch_dst=batch_of(c["src"] if c["dst"] is None else c["dst"]))
    if c["graph"][0] == "list":
        deg = c["graph"][1]
        assert len(deg) == Nt
        tgt = torch.repeat_interleave(torch.arange(Nt), torch.tensor(deg))
        # distinct sources inside a row: the same source twice is an exact tie of two entries
        src = torch.cat([torch.randperm(Ns, generator=g)[:n] for n in deg])
        out["edge_index"] = torch.stack([src, tgt])
    return out


def brute_entries(case, inp):
    """The case's graph built on the CPU in float64 (kNN: the k nearest sources of the target's event, ties to the lower
    index, the target itself excluded with self loops; radius: the first `max` sources within r, ascending id)."""
    c = CASES[case]
    Ns, Nt = sizes(case)
    kind = c["graph"][0]
    if kind == "list":
        ei = inp["edge_index"]
        return pr.entries_from_list(ei[0], ei[1], Nt, c["self_loop"])
    ps, pd = inp["pos_src"].double(), inp["pos_dst"].double()
    d2 = ((pd.unsqueeze(1) - ps.unsqueeze(0)) ** 2).sum(-1)
    same = inp["batch_dst"].view(-1, 1) == inp["batch_src"].view(1, -1)
    width = c["graph"][1] if kind == "knn" else c["graph"][2]
    nbr = torch.full((Nt, width), -1, dtype=torch.int64)
    for i in range(Nt):
        cand = same[i].nonzero().view(-1)
        if kind == "knn":
            order = torch.sort(d2[i, cand], stable=True).indices[:width]
            pick = cand[order]
        else:
            pick = cand[d2[i, cand] < c["graph"][1] ** 2][:width]
        nbr[i, :pick.numel()] = pick
    return pr.entries_from_table(nbr, Ns, None, c["self_loop"])


def reference(case, inp, entries):
    c = CASES[case]
    _Ns, Nt = sizes(case)
    return pr.Reference(inp["x"], inp["pos_src"], inp["pos_dst"], inp["W1"], inp["b1"], inp["W2"], inp["b2"], c["act"],
                        c["act2"], entries, Nt)


def find_seed(case, entries_of):
    """(seed, inputs, entries, reference) of the first of TRIES deterministic seeds whose reference has no fragile
    element over entries_of(inputs); raises AssertionError when none is clear."""
    counts = []
    for seed in range(TRIES):
        inp = make_inputs(case, seed)
        entries = entries_of(inp)
        ref = reference(case, inp, entries)
        if ref.fragile == 0:
            return seed, inp, entries, ref
        counts.append(ref.fragile)
    raise AssertionError(f"{case}: no seed of {TRIES} without fragile elements (counts {counts})")
