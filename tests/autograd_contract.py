"""TEST INFRASTRUCTURE for tests/test_gpu_autograd_contract.py and tests/test_autograd_contract_host.py: one table over every
`torch.autograd.Function` of deepmetv2_amd/, and the seven properties each of them is held to beyond its first backward.

CASES maps the qualified name of a Function ("scatter._SegmentSumRows") to builders.  A builder takes the device and returns
a `Case`: the differentiable leaves (made on the CPU from a fixed seed), a `forward` that reaches the Function through the
public operator, one incoming gradient per output, float64 reference gradients and the gradient bar.  Nothing here touches a
device before a builder runs, so the module imports without one (the completeness test reads CASES on the host).

Shapes: one ragged batch of events of 0, 1, 33 and 130 nodes; tables of width 3 and 16 with short rows (the one-node
event) and an empty row; edge lists made from a table's entries and shuffled, so that they arrive ungrouped.  Widths: the
smallest multiple of 4 the operator takes, and 5 where it takes any width.

The properties (check_*), on a Case:
    P1 reference        the first backward meets `reference` at `bar`
    P2 repeat           backward twice on one graph: the same bits, and no operand changed (leaves, outputs, g, saved
                        tensors, every tensor reachable from the graph object, its cached reverse index included)
    P3 layouts          g as an expanded, a transposed, a narrowed and a 4-byte-offset view, x as a column slice and a
                        4-byte-offset view: the bits of the run on fresh contiguous copies
    P4 subsets          every single leaf and every all-but-one set: the bits of the all-requested run
    P5 double backward  create_graph=True raises (naming double backward / once_differentiable) or differentiates correctly
    P6 scaled           g * 2**12 and g * 2**-12: the first run's gradients times the factor, bit for bit
    P7 in place         an output or a leaf's alias written after forward: autograd's error, or the unmodified run's bits

Bars.  A case's bar is its operator's own, cited where it is set: a `Pair` (rtol, atol factor, floor) where the operator's GPU
test holds its gradients to one pair, or `Bounds`, a function giving a bound per element (0: exact equality), where that
test derives one from the inputs -- the bounds of tests/test_gpu_segment_reduce.py (restated in segment_reference.py),
weighted_sum_reference.grad_x / grad_w, pna_reference.grad_bound, select_reference.select_rows_bwd, and for the event
normalisations four times the error of the same formula in fp32 torch on the CPU (tests/test_gpu_event_norm.py).  A backward
that only gathers or copies g (segment sum / max / min, pair pooling, the gather of select_rows) is held to exact equality;
the mean's is compared with g / count formed in fp32, as segment_reference._segment_mean_bwd forms it.  Two bars are not an
operator's own, because the suite has none for these gradients alone (tests/test_gpu_parity.py compares them inside whole
steps): _MetLoss and _MetLossFromWeights are held to bounds derived from the roundings of their kernels (MET,
_from_weights_bound).
"""
from __future__ import annotations

import math
from collections import namedtuple
from types import SimpleNamespace

import torch

from per_node_reference import misaligned

F_ = torch.nn.functional

SIZES = (0, 1, 33, 130)
N = sum(SIZES)
B = len(SIZES)

U = 2.0 ** -24

# rtol, atol = factor * max(max|ref|, floor), where the pair is from
Pair = namedtuple("Pair", "rtol factor floor source")
AGG = Pair(1e-4, 1e-4, 0.0, "tests/attention_reference.py assert_grad_bar (test_gpu_attention, _gat, _gravnet, _interpolate, "
           "_edgeconv_linear_sum, _pointnet; test_gpu_edge_mlp_f32 as 1e-4 of the gradient scale)")
NODE = Pair(1e-4, 1e-5, 1.0, "tests/per_node_reference.py bar('grad')")
NODE_GX = Pair(1e-4, 2e-5, 1.0, "tests/per_node_reference.py bar('g_x')")
XY = Pair(1e-5, 1e-5, 0.0, "tests/test_gpu_edgeconv_xy.py")
R6 = Pair(0.0, 2e-2, 0.0, "tests/test_gpu_edge_mlp_bf16.py (rule R6)")


class Bounds:
    """fn(leaves64, g64, refs) -> one bound per gradient: a tensor of the gradient's shape or a number; 0 is exact equality."""

    def __init__(self, fn, source):
        self.fn, self.source = fn, source


def exact(source):
    return Bounds(lambda leaves, g, refs: [0.0] * len(refs), source)


# ---- the case ------------------------------------------------------------------------------------------------------------------
def Case(inputs, forward, g, reference, bar, rows=(), graph=None, layout_bits=True, layout_citation=None, formula=None):
    """inputs: the leaves (device tensors, no grad).  forward(*leaves) -> the differentiable outputs (a tensor or a tuple).
    g: one gradient per output.  reference(leaves64, g64) -> float64 CPU gradients.  bar: a Pair or a Bounds.  rows: the indices of the leaves P3 hands over in other
    layouts (the per-row feature tensors, not the parameters).  graph: the graph object(s) whose tensors P2 watches.
    layout_bits=False needs layout_citation.  formula(*leaves64) -> outputs: only for a Function that differentiates twice."""
    if not layout_bits and not layout_citation:
        raise ValueError("layout_bits=False needs the citation of the kernel header that documents the other summation order")
    return SimpleNamespace(inputs=list(inputs), forward=forward, g=list(g), reference=reference, bar=bar, rows=tuple(rows),
                           graph=graph, layout_bits=layout_bits, layout_citation=layout_citation, formula=formula)


def autograd_reference(formula):
    """reference(leaves64, g64) by float64 autograd of a plain-torch formula of the operation."""
    def reference(leaves64, g64):
        ls = [t.detach().clone().requires_grad_(True) for t in leaves64]
        outs = formula(*ls)
        outs = outs if isinstance(outs, (tuple, list)) else (outs,)
        grads = torch.autograd.grad(outs, ls, g64, allow_unused=True)
        return [torch.zeros_like(t) if gr is None else gr for t, gr in zip(ls, grads)]
    return reference


# ---- running a case ------------------------------------------------------------------------------------------------------------
def _tuple(outs):
    return tuple(outs) if isinstance(outs, (tuple, list)) else (outs,)


def fresh(t):
    """A new contiguous (and aligned) tensor with t's values."""
    return t.detach().clone(memory_format=torch.contiguous_format)


def forward(case, leaves=None, need=None, wrap=None):
    """(leaves as autograd leaves, outputs).  leaves: tensors handed over as they are (their layout is kept); need: which of
    them require a gradient; wrap(i, leaf) -> what the operator gets in place of leaf i."""
    leaves = [fresh(t) for t in case.inputs] if leaves is None else leaves
    need = [True] * len(leaves) if need is None else need
    ls = [t.detach().requires_grad_(bool(n)) for t, n in zip(leaves, need)]
    args = [wrap(i, t) for i, t in enumerate(ls)] if wrap is not None else ls
    return ls, _tuple(case.forward(*args)), args


def run(case, leaves=None, g=None, need=None):
    """The gradients of one forward and backward, None where `need` is False."""
    g = [fresh(t) for t in case.g] if g is None else g
    ls, outs, _ = forward(case, leaves, need)
    wanted = [t for t in ls if t.requires_grad]
    grads = iter(torch.autograd.grad(outs, wanted, g, allow_unused=True))
    return [next(grads) if t.requires_grad else None for t in ls]


def same_bits(a, b, what):
    assert (a is None) == (b is None), f"{what}: one is None"
    if a is None:
        return
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {a.dtype}{tuple(a.shape)} against {b.dtype}{tuple(b.shape)}"
    a, b = a.detach().contiguous(), b.detach().contiguous()
    if a.is_floating_point():       # compare the bits: -0.0 is not 0.0 here and a NaN equals itself
        a, b = a.view(torch.int32 if a.element_size() == 4 else torch.int64 if a.element_size() == 8 else torch.int16), \
               b.view(torch.int32 if b.element_size() == 4 else torch.int64 if b.element_size() == 8 else torch.int16)
    if not torch.equal(a, b):
        bad = (a.reshape(-1) != b.reshape(-1)).nonzero().view(-1)
        raise AssertionError(f"{what}: {bad.numel()} of {a.numel()} elements differ, first at flat index {int(bad[0])}")


def all_same_bits(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        same_bits(a, b, f"{what}: gradient {i}")


def close(got, ref, bar, what):
    assert got is not None, f"{what}: no gradient"
    ref = ref.detach().double().cpu()
    top = float(ref.abs().max()) if ref.numel() else 0.0
    atol = bar.factor * max(top, bar.floor, 1e-30)
    torch.testing.assert_close(got.detach().double().cpu(), ref, rtol=bar.rtol, atol=atol, msg=lambda m: f"{what}: {m}")


def hold(case, got, g, what):
    """The gradients `got` of a run with the incoming gradients `g` against the case's reference at the case's bar."""
    leaves64 = [t.detach().double().cpu() for t in case.inputs]
    g64 = [t.detach().double().cpu() for t in g]
    refs = case.reference(leaves64, g64)
    assert len(got) == len(refs)
    if isinstance(case.bar, Pair):
        for i, (a, b) in enumerate(zip(got, refs)):
            close(a, b, case.bar, f"{what}: gradient {i}")
        return
    for i, (a, b, bound) in enumerate(zip(got, refs, case.bar.fn(leaves64, g64, refs))):
        assert a is not None, f"{what}: gradient {i}: none"
        err = (a.detach().double().cpu() - b.double()).abs()
        over = err > (bound if torch.is_tensor(bound) else float(bound))
        if bool(over.any()):
            at = int(over.reshape(-1).nonzero()[0])
            lim = float(bound.expand_as(err).reshape(-1)[at]) if torch.is_tensor(bound) else float(bound)
            raise AssertionError(f"{what}: gradient {i}: {int(over.sum())} of {err.numel()} elements beyond the bound, first at "
                                 f"flat index {at}: error {float(err.reshape(-1)[at]):.3e}, bound {lim:.3e}")


def reference_of(case, g=None):
    g = case.g if g is None else g
    return case.reference([t.detach().double().cpu() for t in case.inputs], [t.detach().double().cpu() for t in g])


def reachable(obj, depth=3):
    """{path: tensor} of every tensor an object holds, through attributes, slots, tuples, lists and dicts."""
    found = {}

    def walk(o, path, d):
        if torch.is_tensor(o):
            found[path] = o
        elif d > 0 and isinstance(o, (tuple, list)):
            for i, v in enumerate(o):
                walk(v, f"{path}[{i}]", d - 1)
        elif d > 0 and isinstance(o, dict):
            for k, v in o.items():
                walk(v, f"{path}[{k!r}]", d - 1)
        elif d > 0 and hasattr(o, "__dict__") and not isinstance(o, (type, torch.nn.Module)) and not callable(o):
            for k, v in vars(o).items():
                walk(v, f"{path}.{k}", d - 1)
    walk(obj, "graph", depth)
    return found


def graph_nodes(outs):
    """Every autograd node reachable from the outputs."""
    seen, stack = [], [o.grad_fn for o in outs if o.grad_fn is not None]
    while stack:
        fn = stack.pop()
        if fn is None or any(fn is f for f in seen):
            continue
        seen.append(fn)
        stack.extend(nxt for nxt, _ in fn.next_functions)
    return seen


def check_reaches(case, qualname):
    """The case runs the Function it is filed under (and no quiet fall-back to another route): its node is in the graph."""
    want = qualname.rsplit(".", 1)[1] + "Backward"
    names = [type(fn).__name__ for fn in graph_nodes(forward(case)[1])]
    assert want in names, f"{qualname}: no {want} node among {sorted(set(names))}"


# ---- P1 ------------------------------------------------------------------------------------------------------------------------
def check_reference(case):
    got = run(case)
    hold(case, got, case.g, "P1")
    return got


# ---- P2 ------------------------------------------------------------------------------------------------------------------------
def _watched(case, ls, outs, g):
    w = {f"leaf {i}": t for i, t in enumerate(ls)}
    w.update({f"output {i}": t for i, t in enumerate(outs)})
    w.update({f"g {i}": t for i, t in enumerate(g)})
    for i, fn in enumerate(graph_nodes(outs)):
        if not hasattr(fn, "needs_input_grad"):      # not a custom Function's node
            continue
        for j, t in enumerate(getattr(fn, "saved_tensors", ()) or ()):
            if torch.is_tensor(t):
                w[f"{type(fn).__name__} saved {j}"] = t
        # what the Function keeps as ctx attributes: its table or edge list, with the indices the backward caches on it
        w.update({f"{type(fn).__name__} ctx {k}": t for k, t in reachable(dict(vars(fn))).items()})
    if case.graph is not None:
        w.update(reachable(case.graph))
    return w


def check_repeat(case):
    g = [fresh(t) for t in case.g]
    ls, outs, _ = forward(case)
    before = {k: (t, t.detach().clone()) for k, t in _watched(case, ls, outs, g).items()}
    first = torch.autograd.grad(outs, ls, g, retain_graph=True, allow_unused=True)
    middle = {k: (t, t.detach().clone()) for k, t in _watched(case, ls, outs, g).items()}     # with what backward cached
    second = torch.autograd.grad(outs, ls, g, retain_graph=True, allow_unused=True)
    all_same_bits(second, first, "P2: the second backward")
    for name, snap in (("before the first backward", before), ("after the first backward", middle)):
        for k, (t, copy) in snap.items():
            same_bits(t, copy, f"P2: {k} changed (against its copy from {name})")


# ---- P3 ------------------------------------------------------------------------------------------------------------------------
def expanded(t):
    """t's first row in every row, as a stride-0 view (what .sum().backward() hands over)."""
    return t[:1].expand(t.shape) if t.dim() >= 1 and t.shape[0] > 1 else t


def transposed(t):
    """t's values in transposed storage: a non-contiguous view."""
    return t.transpose(0, -1).contiguous().transpose(0, -1) if t.dim() >= 2 else t


def narrowed(t):
    """t as a narrow() of a taller buffer (what torch.cat(...).backward() hands over)."""
    if t.dim() < 1 or t.shape[0] < 1:
        return t
    pad = torch.full_like(t[:1], 7.0)
    return torch.cat([pad, t, pad]).narrow(0, 1, t.shape[0])


def offset(t):
    """t as a contiguous view one float into a larger buffer."""
    return misaligned(t, 4) if t.numel() else t


def column_slice(t):
    """t as a column slice of a wider tensor."""
    if t.dim() < 1:
        return t
    if t.dim() == 1:
        wide = torch.full((t.shape[0], 3), 7.0, dtype=t.dtype, device=t.device)
        wide[:, 1] = t
        return wide[:, 1]
    wide = torch.full(tuple(t.shape[:-1]) + (t.shape[-1] + 2,), 7.0, dtype=t.dtype, device=t.device)
    wide[..., 1:-1] = t
    return wide[..., 1:-1]


G_LAYOUTS = (("transposed", transposed), ("narrowed", narrowed), ("offset", offset))
X_LAYOUTS = (("column slice", column_slice), ("offset", offset))


def check_layouts(case):
    def held(got, want, g, what):
        if case.layout_bits:
            all_same_bits(got, want, what)
        else:
            hold(case, got, g, what)

    def attempt(what, **kw):
        try:
            return run(case, **kw)
        except RuntimeError as e:
            raise AssertionError(f"P3: {what}: the operator refused the layout: {e}") from e

    base = run(case)
    g_rows = [fresh(expanded(t)) for t in case.g]
    held(attempt("expanded g", g=[expanded(t) for t in g_rows]), run(case, g=g_rows), g_rows, "P3: expanded g")
    for name, form in G_LAYOUTS:
        g = [form(fresh(t)) for t in case.g]
        for a, b in zip(g, case.g):
            assert torch.equal(a, b)
        held(attempt(f"{name} g", g=g), base, case.g, f"P3: {name} g")
    for name, form in X_LAYOUTS:
        if not case.rows:
            break
        leaves = [form(fresh(t)) if i in case.rows else fresh(t) for i, t in enumerate(case.inputs)]
        for a, b in zip(leaves, case.inputs):
            assert torch.equal(a, b)
        held(attempt(f"{name} x", leaves=leaves), base, case.g, f"P3: {name} x")


# ---- P4 ------------------------------------------------------------------------------------------------------------------------
def subsets(n):
    """Every single leaf and every all-but-one set of n leaves, as tuples of flags, each once, the full set left out."""
    sets = []
    for i in range(n):
        for s in (tuple(j == i for j in range(n)), tuple(j != i for j in range(n))):
            if any(s) and not all(s) and s not in sets:
                sets.append(s)
    return sets


def check_subsets(case):
    base = run(case)
    for need in subsets(len(case.inputs)):
        got = run(case, need=list(need))
        for i, n in enumerate(need):
            if n:
                same_bits(got[i], base[i], f"P4: gradient {i} with {need} requested")
            else:
                assert got[i] is None


# ---- P5 ------------------------------------------------------------------------------------------------------------------------
def check_double_backward(case):
    """-> "raises" or "differentiates"."""
    g = [fresh(t).requires_grad_(True) for t in case.g]
    ls, outs, _ = forward(case)
    try:
        grads = torch.autograd.grad(outs, ls, g, create_graph=True, allow_unused=True)
        for i, gr in enumerate(grads):
            assert gr is not None and gr.requires_grad, \
                f"P5: gradient {i} came back from create_graph=True without a grad_fn: a second derivative would silently " \
                f"treat it as a constant"
        total = sum((gr * torch.linspace(0.5, 1.5, gr.numel(), device=gr.device).view(gr.shape)).sum() for gr in grads)
        # backward(), as a gradient penalty inside a loss runs it: torch.autograd.grad(total, leaves) prunes a node none of
        # whose inputs it was asked about, once_differentiable's error node among them, and answers None
        total.backward()
        second = [t.grad for t in ls + g]
    except RuntimeError as e:
        msg = str(e).lower()
        assert "double backward" in msg or "once_differentiable" in msg, f"P5: a RuntimeError that names neither: {e}"
        return "raises"
    assert case.formula is not None, "P5: the second derivative came back and the case has no float64 formula to hold it to"
    assert isinstance(case.bar, Pair), "P5: a Function that differentiates twice needs a Pair to hold its second derivative to"
    l64 = [t.detach().double().cpu().requires_grad_(True) for t in case.inputs]
    g64 = [t.detach().double().cpu().requires_grad_(True) for t in case.g]
    r1 = torch.autograd.grad(_tuple(case.formula(*l64)), l64, g64, create_graph=True, allow_unused=True)
    rt = sum((gr * torch.linspace(0.5, 1.5, gr.numel(), dtype=torch.float64).view(gr.shape)).sum() for gr in r1)
    r2 = torch.autograd.grad(rt, l64 + g64, allow_unused=True)
    for i, (a, b) in enumerate(zip(second, r2)):
        b = torch.zeros_like((l64 + g64)[i]) if b is None else b
        a = torch.zeros_like((ls + g)[i]) if a is None else a
        close(a, b, case.bar, f"P5: second derivative {i}")
    return "differentiates"


# ---- P6 ------------------------------------------------------------------------------------------------------------------------
def check_scaled(case):
    base = run(case)
    for factor in (2.0 ** 12, 2.0 ** -12):
        got = run(case, g=[fresh(t) * factor for t in case.g])
        all_same_bits(got, [b * factor for b in base], f"P6: g * {factor}")


# ---- P7 ------------------------------------------------------------------------------------------------------------------------
def _backward_after(case, write, what, base):
    """Forward on clones of the leaves, write(outs, clones) in place, backward: autograd's error, or the bits of `base`."""
    ls, outs, args = forward(case, wrap=lambda i, t: t.clone())
    try:
        write(outs, args)
    except RuntimeError as e:       # e.g. an output that is a view made inside the Function's forward
        raise AssertionError(f"P7: {what}: the write itself is refused: {e}") from e
    try:
        got = torch.autograd.grad(outs, ls, [fresh(t) for t in case.g], allow_unused=True)
    except RuntimeError as e:
        assert "modified by an inplace operation" in str(e), f"P7: {what}: a RuntimeError that is not autograd's: {e}"
        return "raises"
    all_same_bits(got, base, f"P7: {what}: neither autograd's error nor the unmodified run")
    return "same bits"


def check_inplace(case):
    base = run(case)
    n_out = len(forward(case)[1])
    for j in range(n_out):
        # the version alone, the way a user's in-place op on the result bumps it
        _backward_after(case, lambda outs, args, j=j: outs[j].mul_(1.0), f"output {j} .mul_(1.0)", base)
        # and new values through an alias: a backward that reads a stashed output now reads something else
        _backward_after(case, lambda outs, args, j=j: outs[j].detach().mul_(0.5), f"output {j} rewritten", base)
    for i in range(len(case.inputs)):
        _backward_after(case, lambda outs, args, i=i: args[i].detach().mul_(0.5), f"leaf {i} rewritten", base)


PROPERTIES = {"P1": check_reference, "P2": check_repeat, "P3": check_layouts, "P4": check_subsets,
              "P5": check_double_backward, "P6": check_scaled, "P7": check_inplace}


# =================================================================================================================================
# the shared shapes
# =================================================================================================================================
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(seed, *shape, scale=1.0):
    return torch.randn(*shape, generator=_gen(seed)) * scale


def ptr_host():
    return torch.tensor([0] + list(torch.tensor(SIZES).cumsum(0)), dtype=torch.int64)


def batch_host():
    return torch.repeat_interleave(torch.arange(B), torch.tensor(SIZES))


def table_host(k, seed, num_src=None, empty_row=True):
    """nbr [N, k] int32: row i lists min(k, n) distinct random nodes of i's own event (so the one-node event has a short
    row), -1 behind them; one row of the last event is empty and one is cut to a single entry.  num_src: the candidates are
    another set of that many nodes per event instead (bipartite), laid out like the rows."""
    g = _gen(seed)
    ptr = ptr_host().tolist()
    nbr = torch.full((N, k), -1, dtype=torch.int32)
    for b in range(B):
        lo, hi = ptr[b], ptr[b + 1]
        for i in range(lo, hi):
            m = min(k, hi - lo)
            nbr[i, :m] = (torch.randperm(hi - lo, generator=g)[:m] + lo).to(torch.int32)
    if empty_row:
        nbr[N - 7] = -1
    nbr[N - 9, 1:] = -1
    return nbr


def entries(nbr):
    """(tgt, src) int64 of a table's valid slots in position order."""
    i, t = (nbr >= 0).nonzero(as_tuple=True)
    return i, nbr[i, t].long()


def make_table(dev, k, seed, dist=False, empty_row=True):
    from deepmetv2_amd.graph import NeighborTable
    nbr = table_host(k, seed, empty_row=empty_row)
    d = None
    if dist:
        d = torch.rand(N, k, generator=_gen(seed + 1)) + 0.05
        d[nbr < 0] = 1e10
        d = d.to(dev)
    return NeighborTable(nbr.to(dev), ptr_host().to(dev), dense=False, dist=d, max_nodes=max(SIZES)), nbr


def make_bipartite(dev, k, seed, dist=False):
    """Queries: the N nodes; candidates: a second set with the same events (so the same ids are in range)."""
    from deepmetv2_amd.graph import BipartiteTable
    nbr = table_host(k, seed)
    d = None
    if dist:
        d = torch.rand(N, k, generator=_gen(seed + 1)) + 0.05
        d[nbr < 0] = 1e10
        d = d.to(dev)
    p = ptr_host().to(dev)
    return BipartiteTable(nbr.to(dev), p, p, N, dist=d), nbr


def shuffled_edge_index(k, seed):
    """int64 [2, E] (row 0 the sources, row 1 the targets) of a table's entries in a shuffled, so ungrouped, order."""
    tgt, src = entries(table_host(k, seed))
    order = torch.randperm(tgt.numel(), generator=_gen(seed + 2))
    return torch.stack([src[order], tgt[order]])


def make_edge_list(dev, k, seed):
    """(EdgeList on the device from an ungrouped edge index, tgt, src of its grouped order on the host)."""
    from deepmetv2_amd.graph import edge_list_from_edge_index
    el = edge_list_from_edge_index(shuffled_edge_index(k, seed).to(dev), N, "source_to_target")
    assert el.perm is not None      # it did arrive ungrouped
    return el, el.tgt.cpu().long(), el.src.cpu().long()


def plant(mod, **tensors):
    """Put plain tensors (autograd leaves or their clones) where a module keeps its parameters."""
    for name, t in tensors.items():
        mod._parameters.pop(name, None)
        mod.__dict__.pop(name, None)
        object.__setattr__(mod, name, t)
    return mod


def _rows_sum(vals, idx, n):
    return torch.zeros((n,) + tuple(vals.shape[1:]), dtype=vals.dtype).index_add(0, idx, vals)


def _rows_ext(vals, idx, n, how):
    """Per-row max / min over dim 0, 0 for a row without an entry."""
    ix = idx.view(-1, *([1] * (vals.dim() - 1))).expand_as(vals)
    return torch.zeros((n,) + tuple(vals.shape[1:]), dtype=vals.dtype).scatter_reduce(0, ix, vals, how, include_self=False)


def _counts(idx, n):
    return torch.zeros(n, dtype=torch.float64).index_add(0, idx, torch.ones(idx.numel(), dtype=torch.float64))


# =================================================================================================================================
# scatter.py
# =================================================================================================================================
def _scatter_index(grouped):
    idx = batch_host()
    if not grouped:
        idx = idx[torch.randperm(N, generator=_gen(5))]
    return idx


def _grouping(idx):
    """(perm, rowptr): entry perm[e] of the caller's order is entry e of the grouped order (a stable sort, as the operator's)."""
    import segment_reference as sr
    perm = torch.sort(idx, stable=True).indices
    return perm, sr.lengths_rowptr(torch.bincount(idx, minlength=B).tolist())


def _grouped_formula(ref, per_entry):
    """A formula over the caller's rows from a segment_reference function of grouped rows and their rowptr."""
    def formula(s, idx):
        perm, rowptr = _grouping(idx)
        out = ref(s[perm], rowptr)
        return torch.zeros_like(out).index_copy(0, perm, out) if per_entry else out
    return formula


def _mean_reference(idx):
    """g / count formed in fp32 and gathered, as segment_reference._segment_mean_bwd forms it: exact."""
    def reference(leaves64, g64):
        import segment_reference as sr
        perm, rowptr = _grouping(idx)
        grouped = sr._segment_mean_bwd(g64[0].float(), rowptr, idx.numel())
        return [torch.zeros_like(grouped).index_copy(0, perm, grouped).double()]
    return reference


def _softmax_bounds(kind, idx):
    """The bounds of tests/test_gpu_segment_reduce.py (test_softmax_backward, test_log_softmax_backward,
    test_logsumexp_backward), in the caller's order."""
    def fn(leaves64, g64, refs):
        import segment_reference as sr
        perm, rowptr = _grouping(idx)
        src, g = leaves64[0][perm], g64[0]
        n_of = rowptr.long().diff()[sr.row_ids(rowptr)].double().view(-1, 1)
        if kind == "softmax":
            y, gg = sr.softmax_ref(src, rowptr), g[perm]
            bound = sr.softmax_bwd_bound(src, gg, rowptr, n_of)
        elif kind == "log_softmax":
            bound = sr.log_softmax_bwd_bound(src, g[perm], rowptr, n_of, refs[0][perm])
        else:
            bound = sr.logsumexp_bwd_bound(src, rowptr, n_of, refs[0][perm])
        return [torch.zeros_like(bound).index_copy(0, perm, bound)]
    return Bounds(fn, "tests/test_gpu_segment_reduce.py (segment_reference.*_bwd_bound)")


GATHER = "a gather of g (tests/test_gpu_segment_reduce.py holds segment_max_bwd and _segment_mean_bwd to the same bits)"


def _scatter_case(fn_name, formula, F, grouped, seed, kwargs=None, pick=None, bar=None, reference=None):
    def build(dev):
        import deepmetv2_amd as dm
        idx = _scatter_index(grouped)
        idx_d = idx.to(dev)
        fn = getattr(dm.scatter, fn_name)

        def fwd(src):
            out = fn(src, idx_d, dim=0, dim_size=B, **(kwargs or {}))
            return out[0] if pick else out
        x = _randn(seed, N, F)
        out_rows = N if fn_name in ("scatter_softmax", "scatter_log_softmax") else B
        ref = reference(idx) if reference is not None else autograd_reference(lambda s: formula(s, idx))
        return Case([x.to(dev)], fwd, [_randn(seed + 1, out_rows, F).to(dev)], ref,
                    bar(idx) if callable(bar) else bar, rows=(0,))
    return build


def _sr(name):
    def ref(*a):
        import segment_reference as sr
        return getattr(sr, name)(*a)
    return ref


def _min64(s, rowptr):
    import segment_reference as sr
    return _rows_ext(s, sr.row_ids(rowptr), rowptr.numel() - 1, "amin")


def _sum1d(dev):
    import deepmetv2_amd as dm
    idx = batch_host()
    idx_d = idx.to(dev)
    return Case([_randn(11, N).to(dev)], lambda s: dm.scatter_add(s, idx_d, dim=0, dim_size=B), [_randn(12, B).to(dev)],
                autograd_reference(lambda s: _rows_sum(s, idx, B)), exact(GATHER), rows=(0,))


def _met_inputs(dev):
    x = _randn(21, N, 8)
    return x, x.to(dev), ptr_host().to(dev)


def _met64(w, x):
    b = batch_host()
    return torch.stack([_rows_sum(w * x[:, 0].double(), b, B), _rows_sum(w * x[:, 1].double(), b, B)], 1)


def _met_mag(x, gmet):
    """[N] |g0 px_i| + |g1 py_i|, the magnitude the roundings of g_w[i] = g0 px_i + g1 py_i are relative to."""
    b = batch_host()
    return (gmet[b, 0] * x[:, 0].double()).abs() + (gmet[b, 1] * x[:, 1].double()).abs()


MET = ("derived here (tests/test_gpu_parity.py compares these gradients inside whole steps only): g_w[i] = g0 px_i + g1 py_i is two products and an "
       "add, each relative to at most |g0 px| + |g1 py|, and one more rounding is kept spare for second-order terms, as the "
       "derived bounds of tests/test_gpu_segment_reduce.py do")


def _met_reduce(dev):
    import deepmetv2_amd as dm
    x, xd, ptr = _met_inputs(dev)
    return Case([torch.rand(N, generator=_gen(22)).to(dev)], lambda w: dm.scatter.met_reduce(w, xd, ptr=ptr),
                [_randn(23, B, 2).to(dev)], autograd_reference(lambda w: _met64(w, x)),
                Bounds(lambda leaves, g, refs: [1e-6 + 1e-6 * refs[0].abs()],
                       "tests/test_gpu_parity.py test_met_reduce_and_scatter_add: rtol 1e-6, atol 1e-6"), rows=(0,))


def _loss64(met, truth):
    return 0.5 * ((met + truth.double()) ** 2).sum(1).mean()


def _met_loss(dev):
    import deepmetv2_amd as dm
    truth = _randn(24, B, 2)
    td = truth.to(dev)
    return Case([_randn(25, B, 2).to(dev)], lambda met: dm.scatter.met_loss(met, td), [torch.tensor(1.5).to(dev)],
                autograd_reference(lambda met: _loss64(met, truth)),
                Bounds(lambda leaves, g, refs: [4 * U * refs[0].abs()],
                       "derived here: g = ((met + truth) * (1 / B)) * g_loss is three roundings relative to the result, one spare"),
                rows=(0,))


def _from_weights_bound(x, truth):
    """g = (met + truth) g_loss / B carries the forward's met, an fp32 sum of n_b terms, (n_b + 2) u sum_i |w_i x_i| (the
    bound of a sum in any order), and four roundings of its own (add, 1 / B, g_loss, the kernel's scale); then g_w as in MET."""
    def fn(leaves, g, refs):
        w, b = leaves[0], batch_host()
        n = _counts(b, B).view(-1, 1)
        mag_met = torch.stack([_rows_sum((w * x[:, 0].double()).abs(), b, B), _rows_sum((w * x[:, 1].double()).abs(), b, B)], 1)
        gmet = (_met64(w, x) + truth.double()[:, :2]) * g[0] / B
        d_g = ((n + 2) * U * mag_met * g[0].abs() / B + 5 * U * gmet.abs())
        xa = x[:, :2].double().abs()
        return [(d_g[b] * xa).sum(1) + 4 * U * _met_mag(x, gmet)]
    return fn


def _met_loss_from_weights(dev):
    import deepmetv2_amd as dm
    x, xd, ptr = _met_inputs(dev)
    truth = _randn(24, B, 2)
    td = truth.to(dev)
    return Case([torch.rand(N, generator=_gen(22)).to(dev)],
                lambda w: dm.scatter.met_loss_from_weights(w, xd, td, ptr=ptr), [torch.tensor(1.5).to(dev)],
                autograd_reference(lambda w: _loss64(_met64(w, x), truth)), Bounds(_from_weights_bound(x, truth), MET),
                rows=(0,))


# =================================================================================================================================
# dense.py
# =================================================================================================================================
def _linear(F):
    def build(dev):
        from deepmetv2_amd import dense
        ins = [_randn(31, N, F), _randn(32, 6, F, scale=0.5), _randn(33, 6)]
        return Case([t.to(dev) for t in ins], dense.linear, [_randn(34, N, 6).to(dev)],
                    autograd_reference(F_.linear), NODE, rows=(0,))
    return build


def _embedding(F):
    def build(dev):
        from deepmetv2_amd import dense
        index = torch.randint(0, 7, (N,), generator=_gen(35))
        idx_d = index.to(dev)
        return Case([_randn(36, 7, F).to(dev)], lambda w: dense.embedding(idx_d, w), [_randn(37, N, F).to(dev)],
                    autograd_reference(lambda w: w[index]), NODE)
    return build


def _encode(dev):
    import per_node_reference as pn
    from deepmetv2_amd import dense
    x_cont, x_cat, g_h = pn.encoder_inputs(N, 33)
    xc, xk = x_cont.to(dev), x_cat.to(dev)

    def reference(leaves64, g64):
        _h, leaves = pn.encoder_ref(x_cont, x_cat, leaves64, g64[0])
        return [t.grad for t in leaves]
    return Case([p.to(dev) for p in pn.encoder_params()], lambda *ps: dense.encode(xc, xk, *ps), [g_h.to(dev)], reference, NODE)


def _bn64(x, res, w, b):
    y = F_.batch_norm(x, None, None, w, b, True, 0.1, 1e-5)
    return y + res


def _batch_norm(dev):
    import per_node_reference as pn
    from deepmetv2_amd import dense
    H = 4
    x, r, g_y = pn.bn_rows(N, H, 41)
    st = pn.bn_state(H, 42)
    bn = pn.bn_module(st).to(dev)

    def fwd(x_, r_, w, b):
        return dense.batch_norm(x_, plant(bn, weight=w, bias=b), residual=r_)
    return Case([x.to(dev), r.to(dev), st["weight"].to(dev), st["bias"].to(dev)], fwd, [g_y.to(dev)],
                autograd_reference(_bn64), NODE_GX, rows=(0, 1))


def _encode_bn(dev):
    import per_node_reference as pn
    from deepmetv2_amd import dense
    x_cont, x_cat, g_h = pn.encoder_inputs(N, 33)
    xc, xk = x_cont.to(dev), x_cat.to(dev)
    st = pn.bn_state(32, 43)
    bn = pn.bn_module(st).to(dev)

    def fwd(w, b, *ps):
        return dense.encode_bn(xc, xk, plant(bn, weight=w, bias=b), None, *ps)

    def reference(leaves64, g64):
        state = dict(st, weight=leaves64[0], bias=leaves64[1])
        _y, leaves, ref = pn.encode_bn_ref(x_cont, x_cat, leaves64[2:], state, g64[0])
        return [ref.weight.grad, ref.bias.grad] + [t.grad for t in leaves]
    return Case([st["weight"].to(dev), st["bias"].to(dev)] + [p.to(dev) for p in pn.encoder_params()], fwd, [g_h.to(dev)],
                reference, NODE)


def _head(dev):
    import per_node_reference as pn
    from deepmetv2_amd import dense
    emb, g_out = pn.head_inputs(N, 44)

    def reference(leaves64, g64):
        _o, leaves = pn.head_ref(*leaves64, g_out=g64[0])
        return [t.grad for t in leaves]
    return Case([emb.to(dev)] + [p.to(dev) for p in pn.head_params()], dense.head, [g_out.to(dev)], reference, NODE, rows=(0,))


# =================================================================================================================================
# conv.py
# =================================================================================================================================
def _edge_feat64(x_dst, x_src, tgt, src):
    return torch.cat([x_dst[tgt], x_src[src] - x_dst[tgt]], 1)


def _aggr64(msg, tgt, n, aggr):
    if aggr == "max":
        return _rows_ext(msg, tgt, n, "amax")
    s = _rows_sum(msg, tgt, n)
    return s / _counts(tgt, n).clamp(min=1).view(-1, 1) if aggr == "mean" else s


def _edgeconv_linear(aggr, over):
    """EdgeConv(Linear(64, 32), aggr) over a k = 16 table ("table") or an ungrouped edge index ("list")."""
    def build(dev):
        import deepmetv2_amd as dm
        lin = torch.nn.Linear(64, 32)
        conv = dm.EdgeConv(lin, aggr=aggr)
        if over == "table":
            graph, nbr = make_table(dev, 16, 51)
            tgt, src = entries(nbr)
            how = graph
        else:
            ei = shuffled_edge_index(16, 51)
            tgt, src = ei[1], ei[0]
            how = ei.to(dev)
            graph = None

        def fwd(x, W, b):
            plant(lin, weight=W, bias=b)
            return conv(x, how)

        def formula(x, W, b):
            return _aggr64(F_.linear(_edge_feat64(x, x, tgt, src), W, b), tgt, N, aggr)
        ins = [_randn(52, N, 32), _randn(53, 32, 64, scale=0.2), _randn(54, 32, scale=0.2)]
        bar = AGG       # _EdgeConvLinearSum: tests/test_gpu_edgeconv_linear_sum.py
        if aggr == "max":
            bar = Bounds(lambda leaves, g, refs: [1e-4 * r.abs() + 1e-5 * max(float(r.abs().max()), 1.0 if i == 0 else 0.0)
                                                  for i, r in enumerate(refs)],
                         "tests/test_gpu_parity.py fused EdgeConv: rtol 1e-4, atol 1e-5 max(1, max|ref|) for g_x, "
                         "1e-5 max|ref| for g_W and g_b")
        return Case([t.to(dev) for t in ins], fwd, [_randn(55, N, 32).to(dev)], autograd_reference(formula), bar, rows=(0,),
                    graph=graph)
    return build


def _mlp64(feat, W1, b1, W2, b2):
    return F_.linear(F_.elu(F_.linear(feat, W1, b1)), W2, b2)


def _edge_mlp(route, aggr, F, over="list"):
    """EdgeConv(Sequential(Linear(2F, 16), ELU, Linear(16, 32)), aggr): the fused route `route` over an ungrouped edge index,
    or ("table", bf16) csrc/edgemlp.hip over a k = 16 table."""
    def build(dev):
        import deepmetv2_amd as dm
        l1, l2 = torch.nn.Linear(2 * F, 16), torch.nn.Linear(16, 32)
        conv = dm.EdgeConv(torch.nn.Sequential(l1, torch.nn.ELU(), l2), aggr=aggr)
        conv.compute_dtype = {"f32": None, "bf16": torch.bfloat16, "f16": torch.float16}[route]
        if over == "table":
            graph, nbr = make_table(dev, 16, 56, empty_row=False)
            tgt, src = entries(nbr)
            how = graph
        else:
            ei = shuffled_edge_index(3, 56)
            tgt, src = ei[1], ei[0]
            how, graph = ei.to(dev), None

        def fwd(x, W1, b1, W2, b2):
            plant(l1, weight=W1, bias=b1)
            plant(l2, weight=W2, bias=b2)
            return conv(x, how)

        def formula(x, W1, b1, W2, b2):
            return _aggr64(_mlp64(_edge_feat64(x, x, tgt, src), W1, b1, W2, b2), tgt, N, aggr)
        ins = [_randn(57, N, F), _randn(58, 16, 2 * F, scale=0.3), _randn(59, 16, scale=0.3), _randn(60, 32, 16, scale=0.3),
               _randn(61, 32, scale=0.3)]
        bar = AGG if route == "f32" or over == "table" else R6
        return Case([t.to(dev) for t in ins], fwd, [_randn(62, N, 32).to(dev)], autograd_reference(formula), bar, rows=(0,),
                    graph=graph)
    return build


def _edge_features(dev):
    """The generic route: an nn no fused route takes (Linear - Tanh), max over an ungrouped edge index."""
    import deepmetv2_amd as dm
    F = 4
    lin = torch.nn.Linear(2 * F, 6)
    conv = dm.EdgeConv(torch.nn.Sequential(lin, torch.nn.Tanh()), aggr="max")
    ei = shuffled_edge_index(3, 63)
    tgt, src = ei[1], ei[0]
    eid = ei.to(dev)

    def fwd(x, W, b):
        plant(lin, weight=W, bias=b)
        return conv(x, eid)

    def formula(x, W, b):
        return _aggr64(torch.tanh(F_.linear(_edge_feat64(x, x, tgt, src), W, b)), tgt, N, "max")
    ins = [_randn(64, N, F), _randn(65, 6, 2 * F, scale=0.5), _randn(66, 6, scale=0.5)]
    return Case([t.to(dev) for t in ins], fwd, [_randn(67, N, 6).to(dev)], autograd_reference(formula), XY, rows=(0,))


def _edge_features_xy(F):
    def build(dev):
        import deepmetv2_amd as dm
        lin = torch.nn.Linear(2 * F, 6)
        conv = dm.EdgeConv(torch.nn.Sequential(lin, torch.nn.Tanh()), aggr="add")
        ei = shuffled_edge_index(3, 68)
        tgt, src = ei[1], ei[0]
        eid = ei.to(dev)

        def fwd(x_src, x_dst, W, b):
            plant(lin, weight=W, bias=b)
            return conv((x_src, x_dst), eid)

        def formula(x_src, x_dst, W, b):
            return _aggr64(torch.tanh(F_.linear(_edge_feat64(x_dst, x_src, tgt, src), W, b)), tgt, N, "add")
        ins = [_randn(69, N, F), _randn(70, N, F), _randn(71, 6, 2 * F, scale=0.5), _randn(72, 6, scale=0.5)]
        return Case([t.to(dev) for t in ins], fwd, [_randn(73, N, 6).to(dev)], autograd_reference(formula), XY, rows=(0, 1))
    return build


# =================================================================================================================================
# event_norm.py
# =================================================================================================================================
def fp32_composition(formula, source="tests/test_gpu_event_norm.py (_layer_check: tol = 4 * base)"):
    """Per gradient, four times the largest error of the same formula differentiated by fp32 torch on the CPU."""
    def fn(leaves64, g64, refs):
        got = autograd_reference(formula)([t.float() for t in leaves64], [t.float() for t in g64])
        return [4 * float((a.double() - b).abs().max()) if b.numel() else 0.0 for a, b in zip(got, refs)]
    return Bounds(fn, source)


def _event_rowptr():
    return ptr_host().int()


def _moments64(x):
    b = batch_host()
    n = _counts(b, B).clamp(min=1).view(-1, 1).to(x.dtype)       # (x.dtype: the same formula serves as the fp32 composition)
    mean = _rows_sum(x, b, B) / n
    var = _rows_sum((x - mean[b]) ** 2, b, B) / n
    return mean, var


def _event_moments(F):
    def build(dev):
        import event_norm_reference as er
        from deepmetv2_amd import event_norm
        ptr = ptr_host().to(dev)
        return Case([_randn(81, N, F).to(dev)], lambda x: event_norm.event_moments(x, ptr=ptr)[:2],
                    [_randn(82, B, F).to(dev), _randn(83, B, F).to(dev)],
                    lambda leaves, g: [er.moments_grad(leaves[0], g[0], g[1], _event_rowptr())], fp32_composition(_moments64),
                    rows=(0,))
    return build


def _normalize64(mode, eps=1e-5):
    def formula(x, alpha, w, bias):
        b = batch_host()
        mean, var = _moments64(x)
        if mode == "channel":
            A = mean * alpha
            q = var + (mean - A) ** 2
        elif mode == "graph":
            A = mean.mean(1, keepdim=True).expand_as(mean)
            q = (var + (mean - A) ** 2).mean(1, keepdim=True).expand_as(mean)
        else:
            A = mean
            q = var.sum(1, keepdim=True).expand_as(mean)
        r = 1.0 / torch.sqrt(q + eps)
        return (x - A[b]) * (r[b] * w) + bias
    return formula


def _event_normalize(mode, F):
    def build(dev):
        from deepmetv2_amd import event_norm
        ptr = ptr_host().to(dev)
        ins = [_randn(84, N, F), torch.rand(F, generator=_gen(85)) + 0.5, torch.rand(F, generator=_gen(86)) + 0.5, _randn(87, F)]
        import event_norm_reference as er
        f64 = _normalize64(mode)
        rp = _event_rowptr()
        if mode == "channel":
            fwd = lambda x, a, w, b: event_norm.event_normalize(x, ptr=ptr, mean_scale=a, weight=w, bias=b)     # noqa: E731
            ref = lambda l, g: list(er.normalize_grads(l[0], g[0], rp, l[1], l[2], l[3], 1e-5, mode))           # noqa: E731
            return Case([t.to(dev) for t in ins], fwd, [_randn(88, N, F).to(dev)], ref, fp32_composition(f64), rows=(0,))
        ins = [ins[0], ins[2], ins[3]]
        fwd = lambda x, w, b: event_norm.event_normalize(x, ptr=ptr, weight=w, bias=b, mode=mode)                # noqa: E731

        def ref(l, g):
            gx, _ga, gw, gb = er.normalize_grads(l[0], g[0], rp, torch.ones_like(l[1]), l[1], l[2], 1e-5, mode)
            return [gx, gw, gb]
        return Case([t.to(dev) for t in ins], fwd, [_randn(88, N, F).to(dev)], ref,
                    fp32_composition(lambda x, w, b: f64(x, 1.0, w, b)), rows=(0,))
    return build


def _event_affine(F):
    """InstanceNorm in evaluation mode with running statistics: shift = running_mean, k1 = weight / sqrt(running_var + eps),
    k0 = bias."""
    def build(dev):
        from deepmetv2_amd import event_norm
        mod = event_norm.InstanceNorm(F, affine=True, track_running_stats=True).eval()
        rm, rv = _randn(89, F), torch.rand(F, generator=_gen(90)) + 0.5
        mod.running_mean.copy_(rm)
        mod.running_var.copy_(rv)
        mod = mod.to(dev)
        batch = batch_host().to(dev)

        def fwd(x, w, b):
            return plant(mod, weight=w, bias=b)(x, batch, batch_size=B)

        def formula(x, w, b):
            return (x - rm.to(x.dtype)) * (w / torch.sqrt(rv.to(x.dtype) + mod.eps)) + b
        ins = [_randn(91, N, F), torch.rand(F, generator=_gen(92)) + 0.5, _randn(93, F)]
        return Case([t.to(dev) for t in ins], fwd, [_randn(94, N, F).to(dev)], autograd_reference(formula),
                    fp32_composition(formula), rows=(0,))
    return build


def _center(F):
    def build(dev):
        from deepmetv2_amd import event_norm
        mod = event_norm.MeanSubtractionNorm()
        batch = batch_host().to(dev)
        f64 = lambda x: x - _moments64(x)[0][batch_host()]                                                       # noqa: E731
        return Case([_randn(95, N, F).to(dev)], lambda x: mod(x, batch, batch_size=B), [_randn(96, N, F).to(dev)],
                    autograd_reference(f64), fp32_composition(f64), rows=(0,))
    return build


# =================================================================================================================================
# select.py, pool.py
# =================================================================================================================================
def _select_rows(F):
    def build(dev):
        import select_reference as sr
        from deepmetv2_amd import select
        score = _randn(101, N)
        perm, node_map = select.topk(score.to(dev), 0.5, ptr=ptr_host().to(dev), return_map=True)
        p = perm.cpu()
        ins = [_randn(102, N, F), _randn(103, N)]
        nm = node_map.cpu()

        def reference(leaves, g):
            # gx: one fp32 product per element, exact; gs: the float64 row sum
            gx32, _gs, _abs = sr.select_rows_bwd(g[0].float(), leaves[0].float(), leaves[1].float(), nm)
            _gx, gs, _abs = sr.select_rows_bwd(g[0], leaves[0], leaves[1], nm)
            return [gx32.double(), gs]

        def bounds(leaves, g, refs):
            return [0.0, sr.gamma(F) * sr.select_rows_bwd(g[0], leaves[0], leaves[1], nm)[2]]
        return Case([t.to(dev) for t in ins], lambda x, s: select.select_rows(x, s, perm, node_map),
                    [_randn(104, p.numel(), F).to(dev)], reference,
                    Bounds(bounds, "tests/test_gpu_select.py test_select_rows_and_its_backward: gx the same bits, gs gamma(F) sum|g x|"),
                    rows=(0, 1))
    return build


def _pair_pool(mode, F):
    def build(dev):
        import deepmetv2_amd as dm
        ei = shuffled_edge_index(3, 105)
        ei = ei[:, ei[0] != ei[1]]
        ei = torch.cat([ei, ei.flip(0)], 1).to(dev)
        batch = batch_host().to(dev)
        cluster = dm.graclus(ei, num_nodes=N, batch=batch, seed=7)
        uniq, inv = torch.unique(cluster.cpu(), return_inverse=True)
        C = uniq.numel()
        assert C < N                    # some pairs were matched
        pool = dm.max_pool_x if mode == "max" else dm.avg_pool_x

        def formula(x):
            if mode == "max":
                return _rows_ext(x, inv, C, "amax")
            return _rows_sum(x, inv, C) / _counts(inv, C).view(-1, 1)
        return Case([_randn(106, N, F).to(dev)], lambda x: pool(cluster, x, batch)[0], [_randn(107, C, F).to(dev)],
                    autograd_reference(formula),
                    exact("tests/pool_reference.py pool_pairs_bwd: a copy to the winner, or g times 1/2 or 1"), rows=(0,))
    return build


# =================================================================================================================================
# the aggregations over a table or an edge list: pna, propagate, gat, attention, gravnet, pointnet, interpolate
# =================================================================================================================================
def _graph_of(dev, over, k, seed, dist=False):
    """(graph object, tgt, src) for over = "table" / "bipartite" / "list"."""
    if over == "list":
        return make_edge_list(dev, k, seed)
    graph, nbr = (make_table if over == "table" else make_bipartite)(dev, k, seed, dist)
    tgt, src = entries(nbr)
    return graph, tgt, src


PNA_AGGRS = ("sum", "mean", "min", "max", "var", "std")


def _positions(graph):
    """(tgt, src, valid) over the positions of a graph, as pna_reference and weighted_sum_reference take them."""
    import pna_reference as pr
    from deepmetv2_amd.graph import EdgeList
    if isinstance(graph, EdgeList):
        return pr.positions_of_list(graph.src, graph.rowptr, N)
    return pr.positions_of_table(graph.nbr, N)


def _multi_aggregate(over, k, F):
    def build(dev):
        import pna_reference as pr
        from deepmetv2_amd import pna
        graph, _tgt, _src = _graph_of(dev, over, k, 111)
        pos = _positions(graph)

        def parts(leaves, g):
            ref = pr.stats(leaves[0], *pos, N)
            assert pr.clamp_is_clear(ref)
            return ref, pr.layout(g[0], PNA_AGGRS, 1)
        return Case([_randn(112, N, F).to(dev)], lambda x: pna.multi_aggregate(x, graph, PNA_AGGRS)[0],
                    [_randn(113, N, len(PNA_AGGRS), F).to(dev)],
                    lambda leaves, g: [pr.grad(leaves[0], *pos, *parts(leaves, g))[0]],
                    Bounds(lambda leaves, g, refs: [pr.grad_bound(leaves[0], *pos, *parts(leaves, g))],
                           "tests/pna_reference.py grad_bound"), rows=(0,), graph=graph)
    return build


def _weighted_sum(over, k, F):
    def build(dev):
        import weighted_sum_reference as ws
        from deepmetv2_amd import propagate
        graph, tgt, _src = _graph_of(dev, over, k, 114)
        pos = _positions(graph)
        w = _randn(115, tgt.numel()) if over == "list" else _randn(115, N, k)

        def both(leaves, g):
            g_x, _n, b_x = ws.grad_x(g[0], leaves[1], *pos, N)
            g_w, b_w = ws.grad_w(g[0], leaves[0], *pos)
            return [g_x, g_w.view(w.shape)], [b_x, b_w.view(w.shape)]
        return Case([_randn(116, N, F).to(dev), w.to(dev)], lambda x, w_: propagate.weighted_aggregate(x, graph, w_),
                    [_randn(117, N, F).to(dev)], lambda leaves, g: both(leaves, g)[0],
                    Bounds(lambda leaves, g, refs: both(leaves, g)[1], "tests/weighted_sum_reference.py grad_x, grad_w"),
                    rows=(0,), graph=graph)
    return build


def _attention(over, k, C):
    def build(dev):
        import attention_reference as ar
        from deepmetv2_amd import attention
        graph, tgt, src = _graph_of(dev, over, k, 121)
        H = 2
        ins = [_randn(122, N, H, C), _randn(123, N, H, C), _randn(124, N, H, C)]
        return Case([t.to(dev) for t in ins], lambda q, k_, v: attention.attention_aggregate(q, k_, v, graph),
                    [_randn(125, N, H, C).to(dev)], autograd_reference(lambda q, k_, v: ar.attention(q, k_, v, tgt, src)[0]),
                    AGG, rows=(0, 1, 2), graph=graph)
    return build


def _gat(mode, over, k, C):
    def build(dev):
        import gat_reference as gr
        from deepmetv2_amd import gat
        graph, tgt, src = _graph_of(dev, over, k, 126)
        H = 2
        if mode == "v2":
            ins = [_randn(127, N, H, C), _randn(128, N, H, C), _randn(129, H, C)]
            fwd = lambda xl, xr, att: gat.gat_aggregate(xl, xr, att, graph)                         # noqa: E731
            f64 = lambda xl, xr, att: gr.gatv2(xl, xr, att, tgt, src, 0.2)[0]                       # noqa: E731
            rows = (0, 1)
        else:
            ins = [_randn(127, N, H, C), _randn(128, N, H), _randn(129, N, H)]
            fwd = lambda xl, a, b: gat.gat_v1_aggregate(xl, a, b, graph)                            # noqa: E731
            f64 = lambda xl, a, b: gr.gatv1(xl, a, b, tgt, src, 0.2)[0]                             # noqa: E731
            rows = (0, 1, 2)
        return Case([t.to(dev) for t in ins], fwd, [_randn(130, N, H, C).to(dev)], autograd_reference(f64), AGG, rows=rows,
                    graph=graph)
    return build


def _gravnet(over, k, P):
    def build(dev):
        import gravnet_reference as gv
        from deepmetv2_amd import gravnet
        graph, _tgt, _src = _graph_of(dev, over, k, 131)
        nbr = graph.nbr.cpu()
        S = 4 if P % 4 == 0 else 5
        ins = [_randn(132, N, P), _randn(133, N, S, scale=0.3)]
        if over == "table":
            fwd = lambda h, s: gravnet.gravnet_aggregate(h, s, graph)                               # noqa: E731
            f64 = lambda h, s: gv.aggregate(h, s, nbr)[0]                                           # noqa: E731
            rows = (0, 1)
        else:
            ins.append(_randn(134, N, S, scale=0.3))
            fwd = lambda h, s, sd: gravnet.gravnet_aggregate(h, s, graph, sd)                       # noqa: E731
            f64 = lambda h, s, sd: gv.aggregate(h, s, nbr, sd)[0]                                   # noqa: E731
            rows = (0, 1, 2)
        return Case([t.to(dev) for t in ins], fwd, [_randn(135, N, 2 * P).to(dev)], autograd_reference(f64), AGG, rows=rows,
                    graph=graph)
    return build


def _pointnet(over, k, F):
    """Two node sets (bipartite table / list): seven differentiable inputs, the seven-way `want` of the backward; one set
    (table): pos on both sides."""
    def build(dev):
        from deepmetv2_amd import pointnet
        graph, tgt, src = _graph_of(dev, over, k, 141)
        D, H1, H2 = 3, 8, 16
        l1, l2 = torch.nn.Linear(F + D, H1), torch.nn.Linear(H1, H2)
        params = [_randn(142, H1, F + D, scale=0.4), _randn(143, H1, scale=0.4), _randn(144, H2, H1, scale=0.4),
                  _randn(145, H2, scale=0.4)]
        x, ps, pd = _randn(146, N, F), _randn(147, N, D), _randn(148, N, D)

        def mods(W1, b1, W2, b2):
            return plant(l1, weight=W1, bias=b1), plant(l2, weight=W2, bias=b2)

        def f64(x_, ps_, pd_, W1, b1, W2, b2):
            feat = torch.cat([x_[src], ps_[src] - pd_[tgt]], 1)
            return _rows_ext(F_.linear(F_.relu(F_.linear(feat, W1, b1)), W2, b2), tgt, N, "amax")
        if over == "table":
            fwd = lambda x_, p_, *w: pointnet.pointnet_aggregate(x_, p_, p_, graph, *mods(*w))      # noqa: E731
            return Case([t.to(dev) for t in [x, ps] + params], fwd, [_randn(149, N, H2).to(dev)],
                        autograd_reference(lambda x_, p_, *w: f64(x_, p_, p_, *w)), AGG, rows=(0, 1), graph=graph)
        fwd = lambda x_, ps_, pd_, *w: pointnet.pointnet_aggregate(x_, ps_, pd_, graph, *mods(*w))  # noqa: E731
        return Case([t.to(dev) for t in [x, ps, pd] + params], fwd, [_randn(149, N, H2).to(dev)], autograd_reference(f64), AGG,
                    rows=(0, 1, 2), graph=graph)
    return build


def _interpolate(over, k, F):
    def build(dev):
        import interpolate_reference as ir
        from deepmetv2_amd import interpolate
        graph, _tgt, _src = _graph_of(dev, over, k, 151, dist=True)
        nbr, dist = graph.nbr.cpu(), graph.dist.cpu()
        return Case([_randn(152, N, F).to(dev)], lambda x: interpolate.interpolate_aggregate(x, graph),
                    [_randn(153, N, F).to(dev)], autograd_reference(lambda x: ir.interpolate(x, nbr, dist)[0]), AGG, rows=(0,),
                    graph=graph)
    return build


# =================================================================================================================================
# the table
# =================================================================================================================================
def _both(make, *args):
    """The builders at width 4 and at the odd width 5."""
    return [make(*args, 4), make(*args, 5)]


CASES = {
    "scatter._SegmentSum1D": [_sum1d],
    "scatter._SegmentSumRows": [_scatter_case("scatter_add", lambda s, i: _rows_sum(s, i, B), 4, False, 201, bar=exact(GATHER)),
                                _scatter_case("scatter_add", lambda s, i: _rows_sum(s, i, B), 5, True, 202, bar=exact(GATHER))],
    "scatter._SegmentMaxRows": [_scatter_case("scatter_max", lambda s, i: _rows_ext(s, i, B, "amax"), 4, True, 203, pick=True,
                                              bar=exact(GATHER)),
                                _scatter_case("scatter_max", lambda s, i: _rows_ext(s, i, B, "amax"), 5, False, 204, pick=True,
                                              bar=exact(GATHER))],
    "scatter._SegmentMeanRows": [_scatter_case("scatter_mean", None, 4, False, 205, bar=exact(GATHER), reference=_mean_reference),
                                 _scatter_case("scatter_mean", None, 5, True, 206, bar=exact(GATHER), reference=_mean_reference)],
    "scatter._SegmentMinRows": [_scatter_case("scatter_min", _grouped_formula(_min64, False), 4, True, 207, pick=True,
                                              bar=exact(GATHER)),
                                _scatter_case("scatter_min", _grouped_formula(_min64, False), 5, False, 208, pick=True,
                                              bar=exact(GATHER))],
    "scatter._SegmentSoftmaxRows": [_scatter_case("scatter_softmax", _grouped_formula(_sr("softmax_ref"), True), 4, False, 209,
                                                  bar=lambda idx: _softmax_bounds("softmax", idx)),
                                    _scatter_case("scatter_log_softmax", _grouped_formula(_sr("log_softmax_ref"), True), 5, True,
                                                  210, bar=lambda idx: _softmax_bounds("log_softmax", idx))],
    "scatter._SegmentLogSumExpRows": [_scatter_case("scatter_logsumexp", _grouped_formula(_sr("logsumexp_ref"), False), 4, True,
                                                    211, bar=lambda idx: _softmax_bounds("logsumexp", idx)),
                                      _scatter_case("scatter_logsumexp", _grouped_formula(_sr("logsumexp_ref"), False), 5, False,
                                                    212, bar=lambda idx: _softmax_bounds("logsumexp", idx))],
    "scatter._MetReduce": [_met_reduce],
    "scatter._MetLoss": [_met_loss],
    "scatter._MetLossFromWeights": [_met_loss_from_weights],
    "dense._Linear": [_linear(4), _linear(5)],
    "dense._Embedding": [_embedding(4), _embedding(5)],
    "dense._Encode": [_encode],
    "dense._BatchNorm": [_batch_norm],
    "dense._EncodeBN": [_encode_bn],
    "dense._Head": [_head],
    "conv._EdgeConvLinearMax": [_edgeconv_linear("max", "table")],
    "conv._EdgeConvLinearSum": [_edgeconv_linear("add", "table"), _edgeconv_linear("mean", "list")],
    "conv._EdgeMLP2Bf16": [_edge_mlp("bf16", "max", 32, "table")],
    "conv._EdgeMLP2F32": [_edge_mlp("f32", "max", 4), _edge_mlp("f32", "mean", 5)],
    "conv._EdgeMLP2Bf16Edges": [_edge_mlp("bf16", "add", 4), _edge_mlp("bf16", "mean", 5)],
    "conv._EdgeMLP2F16Edges": [_edge_mlp("f16", "mean", 4), _edge_mlp("f16", "add", 5)],
    "conv._EdgeFeatures": [_edge_features],
    "conv._EdgeFeaturesXY": [_edge_features_xy(4), _edge_features_xy(5)],
    "event_norm._EventMoments": [_event_moments(4), _event_moments(5)],
    "event_norm._EventNormalize": [_event_normalize("channel", 4), _event_normalize("graph", 5), _event_normalize("pair", 4)],
    "event_norm._EventAffine": [_event_affine(4), _event_affine(5)],
    "event_norm._Center": [_center(4), _center(5)],
    "select._SelectRows": [_select_rows(4), _select_rows(5)],
    "pool._PairPool": [_pair_pool("max", 4), _pair_pool("mean", 5)],
    "pna._MultiAggregate": [_multi_aggregate("table", 3, 4), _multi_aggregate("list", 16, 5),
                            _multi_aggregate("table", 16, 4)],
    "propagate._WeightedSum": [_weighted_sum("table", 3, 4), _weighted_sum("list", 16, 5), _weighted_sum("table", 16, 4)],
    "gat._GatAggregate": [_gat("v2", "table", 3, 4), _gat("v1", "list", 16, 5), _gat("v2", "bipartite", 16, 4)],
    "attention._AttentionAggregate": [_attention("table", 3, 4), _attention("list", 16, 5), _attention("bipartite", 16, 4)],
    "gravnet._GravNetAggregate": [_gravnet("table", 3, 4), _gravnet("bipartite", 16, 5)],
    "pointnet._PointNetAggregate": [_pointnet("bipartite", 3, 4), _pointnet("list", 16, 5), _pointnet("table", 16, 4)],
    "interpolate._InterpolateAggregate": [_interpolate("bipartite", 3, 4), _interpolate("table", 16, 5)],
}
