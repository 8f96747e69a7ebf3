"""Condensation clustering without a GPU: the two host statements of tests/condense_reference.py agree on every case, every
case meets the condition it is for, the operators refuse what they must before any device work, and include/dmet.h
names what deepmetv2_amd/_lib.py binds."""
import ctypes
import os
import re
import shutil

import numpy as np
import pytest
import torch

import condense_reference as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _all_cases():
    cases = [cr.ragged(D) for D in (1, 2, 3, 8)] + [cr.random_batch(), cr.line(True), cr.line(False),
                                                    cr.radius_edge(1.0), cr.radius_edge(float(np.nextafter(np.float32(1), np.float32(2)))),
                                                    cr.inconsistent_ranking()]
    cases += [cr.window_edge(c, same) for c in cr.WINDOW_COUNTS for same in (False, True)]
    cases += [case for case, _want in cr.specials().values()]
    return cases


@pytest.fixture(scope="module")
def results():
    """name -> (case, sequential, recursive): computed once."""
    return {c.name: (c, cr.sequential(c), cr.recursive(c)) for c in _all_cases()}


def test_the_two_statements_agree_on_every_case(results):
    assert len(results) == len(_all_cases())            # distinct names
    for name, (case, seq, rec) in results.items():
        for field in ("labels", "local", "assoc", "points", "points_batch", "counts"):
            a, b = getattr(seq, field), getattr(rec, field)
            assert a.dtype == np.int64 and np.array_equal(a, b), (name, field)
        keep = seq.labels >= 0
        assert np.array_equal(seq.points[seq.labels[keep]], seq.assoc[keep]), name
        assert np.array_equal(seq.assoc >= 0, keep) and np.array_equal(seq.assoc[seq.points], seq.points), name
        assert seq.counts.sum() == len(seq.points) and len(seq.counts) == len(case.sizes), name


def test_the_lattice_keeps_roundings_out():
    td2 = cr.td2_of(cr.T_D)
    assert np.float32(5 / 64) < td2 < np.float32(6 / 64)
    rng = np.random.default_rng(0)
    x = rng.integers(0, 64, (200, 8)).astype(np.float32) / np.float32(8)
    d2 = cr.chain_d2(x, 17)
    exact = ((x.astype(np.float64) - x[17].astype(np.float64)) ** 2).sum(1)
    assert np.array_equal(d2.astype(np.float64), exact)              # exact multiples of 1/64: no rounding anywhere
    assert np.array_equal(d2 * 64, np.round(d2 * 64))
    # d2(a, b) and d2(b, a) are the same bits
    assert all(cr.chain_d2(x, p)[q] == cr.chain_d2(x, q)[p] for p, q in ((0, 5), (17, 3), (100, 199)))


def test_ragged_cases_meet_their_conditions(results):
    for D in (1, 2, 3, 8):
        case, seq, _rec = results[f"ragged_d{D}"]
        assert tuple(case.sizes) == (0, 1, 63, 64, 65, 130, 300) and case.D == D
        assert seq.counts[0] == 0 and seq.counts.max() > 1
        assert 0 < (seq.labels < 0).mean() < 1, D
        # the walk meets assigned candidates: some candidate is no point
        with np.errstate(invalid="ignore"):
            assert (case.beta > np.float32(case.t_beta)).sum() > len(seq.points)
    assert results["ragged_d1"][1].counts.max() > 1 and results["ragged_d2"][1].counts.max() > 10


def test_random_batch_meets_its_conditions(results):
    case, seq, _rec = results["random"]
    assert len(case.sizes) == 40 and min(case.sizes) >= 1 and max(case.sizes) <= 200
    ptr = cr.ptr_of(case.sizes)
    with np.errstate(invalid="ignore"):
        ncand = np.array([(case.beta[ptr[b]:ptr[b + 1]] > np.float32(case.t_beta)).sum() for b in range(40)])
    assert (ncand == 0).sum() >= 1 and np.all(seq.counts[ncand == 0] == 0)      # an event with no candidate
    assert (seq.counts == 1).sum() >= 1                                          # exactly one condensation point
    assert (seq.counts > 64).sum() >= 2                                          # more than one window of points
    noise = (seq.labels < 0).mean()
    assert 0 < noise < 1
    assert len(np.unique(case.beta)) <= 17                                       # heavy ties


def test_line_points_are_every_other_position(results):
    for name, descending in (("line_desc", True), ("line_asc", False)):
        case, seq, _rec = results[name]
        n = case.N
        assert n == 200 > 3 * 64 - 1                    # the entries cross three windows
        pos = np.arange(n)
        if descending:
            want_points = pos[::2]
            want_assoc = pos - pos % 2                  # an odd position belongs to its left neighbour
        else:
            want_points = pos[::-1][::2]                # 199, 197, ...
            want_assoc = pos + (1 - pos % 2)            # an even position belongs to its right neighbour
        assert np.array_equal(seq.points, want_points), name
        assert np.array_equal(seq.assoc, want_assoc), name
        # "no higher-key candidate within t_d" would leave one point only: every entry but the first has such a one
        assert len(seq.points) == 100


def test_window_edges_meet_their_conditions(results):
    for count in cr.WINDOW_COUNTS:
        case, seq, _rec = results[f"window_{count}_apart"]
        with np.errstate(invalid="ignore"):
            cand = np.flatnonzero(case.beta[:case.sizes[0]] > np.float32(case.t_beta))
        assert len(cand) == count and seq.counts.tolist() == [count, 2]
        rank = np.empty(count, dtype=np.int64)
        rank[np.argsort(-case.beta[cand], kind="stable")] = np.arange(count)
        assert np.array_equal(seq.labels[cand], rank)                   # every candidate a point: labels equal ranks
        assert np.all(seq.labels[:case.sizes[0]] >= 0)                  # the others sit on a candidate's spot
        case, seq, _rec = results[f"window_{count}_same"]
        assert seq.counts.tolist() == [1, 2] and np.all(seq.labels[:case.sizes[0]] == 0)
        assert seq.labels[case.sizes[0]:].tolist() == [2, 2, 1]         # 0.75 at (9, 9) ranks before 0.5 at (0, 0)


def test_specials_give_the_hand_worked_labels(results):
    for name, (case, want) in cr.specials().items():
        assert results[name][1].labels.tolist() == want, name
        assert results[name][2].labels.tolist() == want, name


def test_radius_edge_is_strict(results):
    _case, strict, _rec = results["radius_edge_at"]
    assert strict.counts.tolist() == [36] and np.array_equal(strict.assoc, np.arange(36))   # d2 == t_d2: not collected
    case, wider, _rec = results["radius_edge_above"]
    assert np.float32(case.t_d) > 1 and wider.counts[0] < 36 and np.all(wider.labels >= 0)


# ---- the operators' refusals, on CPU tensors ----------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ("condensation_cluster", "condensation_points"))
def test_python_errors_before_any_native_call(monkeypatch, op):
    import deepmetv2_amd as dm
    from deepmetv2_amd import _native

    def never(*a, **k):
        raise AssertionError("_native was reached")
    monkeypatch.setattr(_native, "_condense", never)
    monkeypatch.setattr(_native, "_topk", never)
    f = getattr(dm, op)
    beta, x = torch.rand(10), torch.rand(10, 3)
    for bad in (float("nan"), float("inf"), True, "0.1", None, 1e39):
        with pytest.raises(ValueError, match="t_beta"):
            f(beta, x, t_beta=bad)
    for bad in (0.0, -0.5, float("nan"), float("inf"), True, False, "0.8", None, 1e39, 1e-50):
        with pytest.raises(ValueError, match="t_d"):
            f(beta, x, t_d=bad)
    with pytest.raises(TypeError, match="beta must be a float32, bfloat16 or float16"):
        f(beta.double(), x)
    with pytest.raises(TypeError, match="x must be a float32, bfloat16 or float16"):
        f(beta, x.double())
    with pytest.raises(TypeError, match="beta must be"):
        f(beta.long(), x)
    with pytest.raises(ValueError, match=r"beta must be \[N\] or \[N, 1\]"):
        f(torch.rand(10, 2), x)
    with pytest.raises(ValueError, match=r"beta must be \[N\] or \[N, 1\]"):
        f(torch.rand(2, 5, 1), x)
    with pytest.raises(ValueError, match="x must be"):
        f(beta, torch.rand(9, 3))
    with pytest.raises(ValueError, match="x must be"):
        f(beta, torch.rand(10, 3, 1))
    with pytest.raises(ValueError, match="D = 9"):
        f(beta, torch.rand(10, 9))
    with pytest.raises(ValueError, match="D = 0"):
        f(beta, torch.rand(10, 0))
    with pytest.raises(ValueError, match="batch must be"):
        f(beta, x, torch.zeros(9, dtype=torch.long))
    with pytest.raises(ValueError, match="batch must be"):
        f(beta, x, torch.zeros(10, 1, dtype=torch.long))
    with pytest.raises(TypeError, match="ptr must be a 1-D int64"):
        f(beta, x, ptr=torch.tensor([0, 10], dtype=torch.int32))
    with pytest.raises(TypeError, match="ptr must be a 1-D int64"):
        f(beta, x, ptr=[0, 10])
    # what passes every check reaches the device requirement, still before any native call: [N, 1] beta, [N] x, bf16
    for ok in ((beta[:, None], x), (beta, x[:, 0]), (beta.bfloat16(), x.half())):
        with pytest.raises(RuntimeError, match="non-GPU tensor"):
            f(*ok)


# ---- the C entry and its text -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from deepmetv2_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
            pytest.skip("libdmet_hip.so not built and no hipcc here")
        build.build_hip()
    return _lib.load()


def _call(lib, *, beta=None, x=None, order=None, ptr=None, B=1, N=10, D=3, t_beta=0.1, t_d=0.8, local=None, assoc=None,
          ncl=None, flags=None, lds_nodes=0, ws=None, ws_bytes=0):
    return lib.dmet_condense_f32(beta, x, order, ptr, B, N, D, t_beta, t_d, local, assoc, ncl, flags, lds_nodes, ws, ws_bytes,
                                 None)


def test_condense_argument_validation(lib):
    """Every check fails before any device work: NULL pointers all the way."""
    for kw, word in ((dict(N=-1), b"N=-1"), (dict(B=-2), b"B=-2"), (dict(D=0), b"D=0"), (dict(D=9), b"D=9"),
                     (dict(t_beta=float("nan")), b"t_beta"), (dict(t_beta=float("inf")), b"t_beta"),
                     (dict(t_d=0.0), b"t_d"), (dict(t_d=-1.0), b"t_d"), (dict(t_d=float("nan")), b"t_d"),
                     (dict(t_d=float("inf")), b"t_d"), (dict(lds_nodes=-1), b"lds_nodes=-1"), (dict(), b"flags is NULL")):
        assert _call(lib, **kw) == -22 and word in lib.dmet_last_error(), kw
    assert lib.dmet_condense_workspace_bytes(0) == 0 and lib.dmet_condense_workspace_bytes(-3) == 0
    sizes = [lib.dmet_condense_workspace_bytes(n) for n in (1, 2, 1000, 16384, 16385, 10 ** 6, 2 ** 31 - 1)]
    assert sizes == [4 * n for n in (1, 2, 1000, 16384, 16385, 10 ** 6, 2 ** 31 - 1)]


def _prototype(text: str, name: str):
    m = re.search(r"\b" + name + r"\(([^;]*)\);", text)
    assert m, name
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    return [(p.rsplit(" ", 1)[0].strip() + ("*" if p.rsplit(" ", 1)[1].startswith("*") else ""),
             p.rsplit(" ", 1)[1].lstrip("*")) for p in params]


def test_the_header_names_what_the_loader_binds():
    from deepmetv2_amd import _lib, _native
    text = open(os.path.join(ROOT, "include", "dmet.h")).read()
    start = text.index("/* ---- Condensation clustering")
    section = text[start:]
    comment = section[:section.index("*/")]
    ctype = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "size_t": ctypes.c_size_t,
             "dmet_stream_t": ctypes.c_void_p}
    for name in ("dmet_condense_workspace_bytes", "dmet_condense_f32"):
        proto = _prototype(section, name)
        res, args = _lib.SIGNATURES[name]
        assert len(proto) == len(args), name
        for (ty, pname), arg in zip(proto, args):
            want = ctypes.c_void_p if ty.endswith("*") else ctype[ty]
            assert arg is want, (name, pname, ty)
            if pname != "stream":
                assert re.search(r"\b" + pname + r"\b", comment), (name, pname)     # the text states every parameter
    assert _lib.SIGNATURES["dmet_condense_workspace_bytes"][0] is ctypes.c_size_t
    assert f"#define DMET_CONDENSE_LDS_NODES {_native.CONDENSE_LDS_NODES} " in text
    assert f"#define DMET_CONDENSE_WINDOW {_native.CONDENSE_WINDOW} " in text
    assert f"#define DMET_CONDENSE_MAX_DIM {_native.CONDENSE_MAX_DIM}\n" in text
    assert "Unwritten regions: none" in comment
    # the wrapper passes what the entry takes, in its order
    import inspect
    assert list(inspect.signature(_native._condense).parameters) == ["beta", "x", "order", "ptr", "t_beta", "t_d", "lds_nodes"]
