"""The poisoned-allocation mechanism (tests/poisoned_alloc.py) on the CPU, and coverage of deepmetv2_amd/_native.py by the
case table of tests/test_gpu_poisoned_buffers.py: every public wrapper that allocates with an uninitialised allocator,
directly or through a helper, has a case.  There is no exemption list."""
import ast
import os

import pytest
import torch

import poisoned_alloc as pa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deepmetv2_amd")
ALLOCATORS = {"empty", "empty_like", "empty_strided", "new_empty"}


# ---- the mechanism ------------------------------------------------------------------------------------------------------
def _toy_partial(n):
    from deepmetv2_amd import _native
    out = _native.torch.empty((n,), dtype=torch.float32)
    idx = _native.torch.empty((n,), dtype=torch.int32)
    out[: n // 2] = 1.0         # the second half is left as allocated
    idx[:] = 7
    return out, idx


def _toy_full(n):
    from deepmetv2_amd import _native
    out = _native.torch.empty((n,), dtype=torch.float32)
    ws = _native._ws(64, torch.device("cpu"))
    ws.zero_()
    out[:] = ws[:n].float() + 2.0
    return out, ws


def test_partial_writer_differs_between_patterns():
    got = pa.run_both(lambda: _toy_partial(10))
    bad = pa.differing(got["ones"][0], got["zeros_huge"][0])
    assert bad.tolist() == [5, 6, 7, 8, 9]
    assert pa.differing(got["ones"][1], got["zeros_huge"][1]).numel() == 0
    keep = torch.arange(10) < 5
    assert pa.differing(got["ones"][0], got["zeros_huge"][0], keep).numel() == 0


def test_full_writer_does_not_differ():
    got = pa.run_both(lambda: _toy_full(10))
    for a, b in zip(got["ones"], got["zeros_huge"]):
        assert pa.differing(a, b).numel() == 0


def test_patterns_read_as_documented():
    from deepmetv2_amd import _native
    with pa.poisoned("ones") as p:
        f = [_native.torch.empty((3,), dtype=d) for d in (torch.float32, torch.bfloat16, torch.float16)]
        i = [_native.torch.empty((3,), dtype=d) for d in (torch.int16, torch.int32, torch.int64)]
        u = _native.torch.empty((3,), dtype=torch.uint8)
        like = _native.torch.empty_like(f[0])
        assert isinstance(u, _native.torch.Tensor)
    assert p.count == 8 and p.elements == 24
    assert all(bool(t.isnan().all()) for t in f + [like])
    assert all(bool((t == -1).all()) for t in i)
    assert bool((u == 255).all())
    with pa.poisoned("zeros_huge") as p:
        f = [_native.torch.empty((3,), dtype=d) for d in (torch.float32, torch.bfloat16, torch.float16)]
        i = [_native.torch.empty((3,), dtype=d) for d in (torch.int16, torch.int32, torch.int64, torch.uint8)]
        ws = _native._ws(5, torch.device("cpu"))
    assert p.count == 8
    assert bool((f[0] == pa.HUGE).all()) and bool(f[0].isfinite().all())
    assert all(bool((t.float() > 6e4).all()) and bool(t.isfinite().all()) for t in f)     # fp16: 65504, its largest
    assert all(bool((t == 0).all()) for t in i) and bool((ws == 0).all()) and ws.numel() == 16
    with pytest.raises(ValueError):
        with pa.poisoned("big_index"):
            pass


def test_run_both_rejects_a_case_that_poisons_nothing():
    with pytest.raises(AssertionError, match="no allocation was poisoned"):
        pa.run_both(lambda: torch.zeros(3))


def test_global_is_restored_after_an_exception():
    from deepmetv2_amd import _native
    real = _native.torch
    assert real is torch
    with pytest.raises(KeyError):
        with pa.poisoned("ones"):
            assert _native.torch is not torch
            raise KeyError("inside")
    assert _native.torch is real
    with pa.poisoned("zeros_huge"):
        pass
    assert _native.torch is real


# ---- coverage by construction -------------------------------------------------------------------------------------------
def _calls(node):
    """Names a function body calls: ('attr', name) for x.name(...), ('name', name) for name(...)."""
    out = set()
    for n in ast.walk(node):
        if isinstance(n, ast.Call):
            if isinstance(n.func, ast.Attribute):
                out.add(("attr", n.func.attr))
            elif isinstance(n.func, ast.Name):
                out.add(("name", n.func.id))
    return out


def allocating_wrappers(source: str):
    """(public names that allocate uninitialised memory, all allocating top-level functions) of a module's source:
    top-level functions whose body calls an uninitialised allocator, or, transitively, a top-level function that does;
    plus the module-level names bound to such a function through a call that takes it as an argument (NAME = f(impl, ...):
    _native's _bind_route)."""
    tree = ast.parse(source)
    funcs = {n.name: _calls(n) for n in tree.body if isinstance(n, ast.FunctionDef)}
    alloc = {name for name, calls in funcs.items() if any(kind == "attr" and c in ALLOCATORS for kind, c in calls)}
    grew = True
    while grew:
        grew = False
        for name, calls in funcs.items():
            if name not in alloc and any(kind == "name" and c in alloc for kind, c in calls):
                alloc.add(name)
                grew = True
    public = {n for n in alloc if not n.startswith("_")}
    for n in tree.body:
        if isinstance(n, ast.Assign) and isinstance(n.value, ast.Call) and len(n.targets) == 1 \
                and isinstance(n.targets[0], ast.Name) and not n.targets[0].id.startswith("_"):
            if any(isinstance(a, ast.Name) and a.id in alloc for a in n.value.args):
                public.add(n.targets[0].id)
    return public, alloc


def _native_source():
    with open(os.path.join(PKG, "_native.py")) as f:
        return f.read()


def test_the_walk_finds_the_helpers_and_the_bound_routes():
    public, alloc = allocating_wrappers(_native_source())
    assert {"_ws", "_pq_tables", "_knn_run", "_radius_build", "_knn", "_edge_mlp_fwd", "_edge_mlp_bwd", "_xty_wide"} <= alloc
    assert {"knn", "knn_xy", "radius", "radius_periodic", "xty_wide_ones", "edge_mlp_fwd_f16", "edge_mlp_bwd_bf16", "fps",
            "bn_knn_local_dense", "table_rowptr"} <= public
    assert "edge_mlp_f32_supported" not in public and "finalize_flush" not in public


def test_every_allocating_wrapper_has_a_case():
    from test_gpu_poisoned_buffers import CASES
    public, _ = allocating_wrappers(_native_source())
    missing = sorted(public - set(CASES))
    assert not missing, f"_native wrappers that allocate uninitialised memory without a case in CASES: {missing}"
    stale = sorted(n for n in CASES if n not in public)
    assert not stale, f"CASES keys that are no allocating wrapper of _native: {stale}"
    assert all(len(CASES[n]) >= 1 for n in public)


def test_a_wrapper_added_without_a_case_is_reported():
    from test_gpu_poisoned_buffers import CASES
    src = _native_source() + ("\n\ndef brand_new_op(x):\n    ws = _ws(64, x.device)\n    return ws\n"
                              "\n\ndef brand_new_like(x):\n    return torch.empty_like(x)\n")
    public, _ = allocating_wrappers(src)
    assert {"brand_new_op", "brand_new_like"} <= public - set(CASES)


# ---- the rest of the package ----------------------------------------------------------------------------------------------
# the uninitialised allocations outside _native.py, by (module, enclosing function): zero-size, or wholly overwritten by a
# permutation scatter on the same line
OTHER_SITES = {
    ("_softmax_conv.py", "_with_alpha"): 1,  # empty_like(alpha).index_copy_(0, perm, alpha): perm is a permutation
    ("attention.py", "forward"): 1,        # out.new_empty(0) (no alpha)
    ("cluster.py", "fps"): 1,              # torch.empty(0): N == 0 or B == 0
    ("pool.py", "forward"): 1,             # torch.empty(0): no pooled batch asked for
    ("pool.py", "__init__"): 1,            # empty_like(rank).scatter_(0, order, rank): order is a permutation
}


def _sites(path):
    """[(enclosing function name, the call node)] of every uninitialised allocation in a file."""
    with open(path) as f:
        tree = ast.parse(f.read())
    found = []

    def walk(node, fn):
        for child in ast.iter_child_nodes(node):
            name = child.name if isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef)) else fn
            if isinstance(child, ast.Call) and isinstance(child.func, ast.Attribute) and child.func.attr in ALLOCATORS:
                found.append((fn, child))
            walk(child, name)
    walk(tree, None)
    return found


def test_no_other_module_allocates_uninitialised_memory():
    seen = {}
    for name in sorted(os.listdir(PKG)):
        if not name.endswith(".py") or name == "_native.py":
            continue
        for fn, call in _sites(os.path.join(PKG, name)):
            seen[(name, fn)] = seen.get((name, fn), 0) + 1
    assert seen == OTHER_SITES, f"uninitialised allocations outside _native.py changed: {seen}"
    assert sum(OTHER_SITES.values()) == 5
