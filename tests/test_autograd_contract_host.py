"""The autograd contract on the host: the table of tests/autograd_contract.py covers every torch.autograd.Function of
deepmetv2_amd/ (an ast walk; there is no exemption list), and the seven property functions catch what they are for -- one
small pure-torch Function on the CPU breaks each of P2 to P7 and nothing else, and one keeps all of them."""
import ast
import os

import pytest
import torch
from torch.autograd.function import once_differentiable

import autograd_contract as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deepmetv2_amd")


# ---- completeness ------------------------------------------------------------------------------------------------------------
def _names_function(base) -> bool:
    return (isinstance(base, ast.Attribute) and base.attr == "Function") or (isinstance(base, ast.Name) and base.id == "Function")


def function_classes(source: str, module: str):
    """The qualified names of a module's autograd Functions: every class one of whose bases names `Function`, and every
    module-level NAME = factory(..., "NAME", ...) whose factory returns type(name, (... Function ...), ...)."""
    tree = ast.parse(source)
    found = {f"{module}.{n.name}" for n in ast.walk(tree) if isinstance(n, ast.ClassDef) and any(map(_names_function, n.bases))}
    factories = set()
    for fn in (n for n in tree.body if isinstance(n, ast.FunctionDef)):
        for call in (n for n in ast.walk(fn) if isinstance(n, ast.Call)):
            if isinstance(call.func, ast.Name) and call.func.id == "type" and len(call.args) == 3 \
                    and isinstance(call.args[1], ast.Tuple) and any(map(_names_function, call.args[1].elts)):
                factories.add(fn.name)
    for n in tree.body:
        if isinstance(n, ast.Assign) and isinstance(n.value, ast.Call) and isinstance(n.value.func, ast.Name) \
                and n.value.func.id in factories and len(n.targets) == 1 and isinstance(n.targets[0], ast.Name):
            found.add(f"{module}.{n.targets[0].id}")
    return found


def _package_functions():
    found = set()
    for name in sorted(os.listdir(PKG)):
        if name.endswith(".py"):
            with open(os.path.join(PKG, name)) as f:
                found |= function_classes(f.read(), name[:-3])
    return found


def test_the_walk_finds_the_classes_and_the_factory_made_routes():
    found = _package_functions()
    assert {"conv._EdgeMLP2F32", "conv._EdgeMLP2Bf16Edges", "conv._EdgeMLP2F16Edges", "conv._EdgeMLP2Bf16",
            "scatter._MetLossFromWeights", "dense._EncodeBN", "pool._PairPool", "interpolate._InterpolateAggregate"} <= found
    assert len(found) >= 37


def test_every_function_has_a_case():
    found = _package_functions()
    missing = sorted(found - set(ac.CASES))
    assert not missing, f"autograd Functions without a case in tests/autograd_contract.py CASES: {missing}"
    stale = sorted(set(ac.CASES) - found)
    assert not stale, f"CASES keys that are no autograd Function of the package: {stale}"
    assert all(len(ac.CASES[n]) >= 1 and all(callable(b) for b in ac.CASES[n]) for n in found)


def test_a_function_added_without_a_case_is_reported():
    src = ("import torch\nfrom torch.autograd import Function\n\n\nclass _New(torch.autograd.Function):\n    pass\n\n\n"
           "class _Bare(Function):\n    pass\n\n\nclass _Not(torch.nn.Module):\n    pass\n\n\n"
           "def _make(name):\n    return type(name, (torch.autograd.Function,), {})\n\n\n_Made = _make('_Made')\n")
    assert function_classes(src, "brand_new") == {"brand_new._New", "brand_new._Bare", "brand_new._Made"}
    assert not function_classes(src, "brand_new") & set(ac.CASES)


def unguarded_backwards(source: str, module: str):
    """The Functions of a module whose backward carries no double-backward guard.  A class: its `backward` is decorated
    `once_differentiable`, or its first statement after a docstring is a call of `no_double_backward`.  A factory that makes
    Functions with type(...): the `backward` it hands over is wrapped, once_differentiable(backward)."""
    tree = ast.parse(source)
    bare = []
    for cls in (n for n in ast.walk(tree) if isinstance(n, ast.ClassDef) and any(map(_names_function, n.bases))):
        for fn in (n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "backward"):
            decorated = any(isinstance(d, ast.Name) and d.id == "once_differentiable" for d in fn.decorator_list)
            body = fn.body[1:] if isinstance(fn.body[0], ast.Expr) and isinstance(fn.body[0].value, ast.Constant) \
                and isinstance(fn.body[0].value.value, str) else fn.body
            first = body[0] if body else None
            guarded = isinstance(first, ast.Expr) and isinstance(first.value, ast.Call) \
                and isinstance(first.value.func, ast.Attribute) and first.value.func.attr == "no_double_backward"
            if not (decorated or guarded):
                bare.append(f"{module}.{cls.name}")
    for fn in (n for n in tree.body if isinstance(n, ast.FunctionDef)):
        makes = [c for c in ast.walk(fn) if isinstance(c, ast.Call) and isinstance(c.func, ast.Name) and c.func.id == "type"
                 and len(c.args) == 3 and isinstance(c.args[1], ast.Tuple) and any(map(_names_function, c.args[1].elts))]
        if makes and not any(isinstance(c, ast.Call) and isinstance(c.func, ast.Name) and c.func.id == "once_differentiable"
                             and len(c.args) == 1 and isinstance(c.args[0], ast.Name) and c.args[0].id == "backward"
                             for m in makes for c in ast.walk(m)):
            bare.append(f"{module}.{fn.name}")
    return bare


def test_every_function_of_the_package_is_guarded():
    """Read from the source, so that a new Function cannot join without a guard (P5 then sees it raise on the GPU)."""
    bare = []
    for name in sorted(os.listdir(PKG)):
        if name.endswith(".py"):
            with open(os.path.join(PKG, name)) as f:
                bare += unguarded_backwards(f.read(), name[:-3])
    assert not bare, f"backward without a double-backward guard: {bare}"


def test_the_guard_walk_reads_docstrings_and_factories():
    head = "import torch\nfrom torch.autograd.function import once_differentiable\n\n\n"
    doc = head + ("class _A(torch.autograd.Function):\n    @staticmethod\n    def backward(ctx, g):\n        \"\"\"doc\"\"\"\n"
                  "        _native.no_double_backward('_A')\n        return g\n")
    assert unguarded_backwards(doc, "m") == []
    assert unguarded_backwards(doc.replace("        _native.no_double_backward('_A')\n", ""), "m") == ["m._A"]
    made = head + ("def _make(name):\n    def backward(ctx, g):\n        return g\n"
                   "    return type(name, (torch.autograd.Function,), {'backward': staticmethod(WRAP)})\n")
    assert unguarded_backwards(made.replace("WRAP", "once_differentiable(backward)"), "m") == []
    assert unguarded_backwards(made.replace("WRAP", "backward"), "m") == ["m._make"]


def test_the_guard_raises_only_under_grad_mode():
    from deepmetv2_amd import _native
    with torch.no_grad():
        _native.no_double_backward("_Toy")
    with torch.enable_grad(), pytest.raises(RuntimeError, match="double backward"):
        _native.no_double_backward("_Toy")


# ---- the harness catches what it is for --------------------------------------------------------------------------------------
class _Clean(torch.autograd.Function):
    """out = a * exp(b): saves what it reads, honours needs_input_grad without changing a rounding, once differentiable."""

    @staticmethod
    def forward(ctx, a, b):
        out = a * torch.exp(b)
        ctx.save_for_backward(a, b, out)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        a, b, out = ctx.saved_tensors
        return (g * torch.exp(b) if ctx.needs_input_grad[0] else None, g * out if ctx.needs_input_grad[1] else None)


class _ScalesGInPlace(_Clean):
    """P2: writes into the gradient it was handed (a stride-0 gradient cannot be written, so that one it leaves alone)."""

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        res = _Clean.backward(ctx, g)
        if 0 not in g.stride():
            g.mul_(2.0)
        return res


class _WritesSavedOutput(_Clean):
    """P2: uses its saved output as scratch."""

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        res = _Clean.backward(ctx, g)
        ctx.saved_tensors[2].data.add_(1.0)
        return res


class _SubsetRounding(_Clean):
    """P4: another kernel when the neighbour's gradient is not needed, with another rounding."""

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        a, b, out = ctx.saved_tensors
        if ctx.needs_input_grad[1]:
            ga = g * torch.exp(b)
        else:
            ga = (g.double() * torch.exp(b.double()) * (1.0 + 2.0 ** -22)).float()
        return ga if ctx.needs_input_grad[0] else None, g * out if ctx.needs_input_grad[1] else None


class _AssumesContiguity(_Clean):
    """P3: reads g's storage from its offset as if it were contiguous, the way a kernel handed g.data_ptr() does."""

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        flat = torch.as_strided(g, (g.numel(),), (1,), g.storage_offset())
        return _Clean.backward(ctx, flat.view(g.shape))


class _SilentDoubleBackward(_Clean):
    """P5: no guard, and a backward whose result carries no graph."""

    @staticmethod
    def backward(ctx, g):
        a, b, out = ctx.saved_tensors
        with torch.no_grad():
            return g * torch.exp(b), g * out


class _NotHomogeneous(_Clean):
    """P6: an epsilon added to the gradient."""

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        ga, gb = _Clean.backward(ctx, g)
        return (None if ga is None else ga + 1e-30), gb


class _StashesOutput(torch.autograd.Function):
    """P7: keeps its output in a ctx attribute, where autograd's version check does not see it."""

    @staticmethod
    def forward(ctx, a, b):
        out = a * torch.exp(b)
        ctx.save_for_backward(a, b)
        ctx.out = out
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        return g * torch.exp(b), g * ctx.out


TOYS = {"clean": (_Clean, None), "scales g in place": (_ScalesGInPlace, "P2"), "writes its saved output": (_WritesSavedOutput, "P2"),
        "subset rounding": (_SubsetRounding, "P4"), "assumes contiguity": (_AssumesContiguity, "P3"),
        "silent double backward": (_SilentDoubleBackward, "P5"), "not homogeneous": (_NotHomogeneous, "P6"),
        "stashes its output": (_StashesOutput, "P7")}


def _toy_case(fn):
    gen = torch.Generator().manual_seed(3)
    a, b = torch.randn(6, 4, generator=gen), torch.randn(6, 4, generator=gen) * 0.5
    g = torch.randn(6, 4, generator=gen)
    g[:, 2] = 0.0       # zeros in the gradient: where an added epsilon is not rounded away
    return ac.Case([a, b], fn.apply, [g], ac.autograd_reference(lambda a_, b_: a_ * torch.exp(b_)), ac.AGG, rows=(0, 1))


@pytest.mark.parametrize("prop", sorted(ac.PROPERTIES))
@pytest.mark.parametrize("toy", sorted(TOYS))
def test_each_toy_is_caught_by_its_own_property_alone(toy, prop):
    fn, breaks = TOYS[toy]
    case = _toy_case(fn)
    if prop == breaks:
        with pytest.raises(AssertionError, match=prop):
            ac.PROPERTIES[prop](case)
    else:
        res = ac.PROPERTIES[prop](case)
        if prop == "P5":
            assert res == "raises"


def test_a_function_that_differentiates_twice_is_held_to_the_formula():
    """P5's other branch: plain torch operators differentiate twice; a wrong formula is caught."""
    gen = torch.Generator().manual_seed(4)
    a, b, g = (torch.randn(5, 3, generator=gen) for _ in range(3))
    good = lambda a_, b_: a_ * torch.exp(b_)                      # noqa: E731
    case = ac.Case([a, b], good, [g], ac.autograd_reference(good), ac.AGG, formula=good)
    assert ac.check_double_backward(case) == "differentiates"
    case.formula = lambda a_, b_: a_ * torch.exp(1.01 * b_)
    with pytest.raises(AssertionError, match="P5"):
        ac.check_double_backward(case)
    case.formula = None
    with pytest.raises(AssertionError, match="no float64 formula"):
        ac.check_double_backward(case)


def test_layout_exception_needs_a_citation():
    with pytest.raises(ValueError, match="citation"):
        ac.Case([], None, [], None, ac.AGG, layout_bits=False)
    assert not any(s == (True,) * n for n in (1, 2, 5) for s in ac.subsets(n))
    assert ac.subsets(1) == [] and len(ac.subsets(2)) == 2 and len(ac.subsets(9)) == 18


def test_the_layouts_are_what_they_say():
    t = torch.arange(24.0).view(6, 4)
    e = ac.expanded(t)
    assert e.stride(0) == 0 and torch.equal(e, t[:1].expand(6, 4))
    tr = ac.transposed(t)
    assert not tr.is_contiguous() and torch.equal(tr, t)
    na = ac.narrowed(t)
    assert na.storage_offset() == 4 and torch.equal(na, t)
    off = ac.offset(t)
    assert off.is_contiguous() and off.data_ptr() % 16 == 4 and torch.equal(off, t)
    cs = ac.column_slice(t)
    assert not cs.is_contiguous() and cs.stride(0) == 6 and torch.equal(cs, t)
    v = ac.column_slice(torch.arange(5.0))
    assert v.stride(0) == 3 and torch.equal(v, torch.arange(5.0))
