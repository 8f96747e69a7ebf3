"""Graph coarsening without a GPU: the CPU restatement of the graclus contract (tests/pool_reference.py), argument
validation of the new C entries (include/dmet.h "Graph coarsening"), and the Python-level errors."""
import os
import shutil

import numpy as np
import pytest
import torch

import pool_reference as ref


def _sym_random_graph(sizes, deg, seed):
    rng = np.random.default_rng(seed)
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rows, cols = [], []
    for b, n in enumerate(sizes):
        lo = ptr[b]
        if n < 2:
            continue
        for i in range(n):
            for j in rng.choice(n, size=min(deg, n), replace=False):
                rows += [lo + i, lo + j]
                cols += [lo + j, lo + i]
    return np.array([rows, cols], dtype=np.int64), ptr


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("max_rounds", [0, 1, 2])
def test_reference_matching_is_valid_and_maximal(weighted, max_rounds):
    ei, ptr = _sym_random_graph([1, 2, 17, 60, 0, 130], 4, seed=3 + max_rounds)
    N = int(ptr[-1])
    w = np.random.default_rng(7).random(ei.shape[1]).astype(np.float32) if weighted else None
    rowptr, col, ws = ref.to_csr(ei, N, w)
    cluster, partner, rounds = ref.graclus(rowptr, col, ws, ptr, seed=12345, max_rounds=max_rounds)
    ref.check_matching(cluster, partner, ei, ptr)
    if max_rounds:
        assert rounds.max() <= max_rounds
    leaders = cluster == np.arange(N)
    assert leaders.sum() < N          # something was matched


def test_reference_finisher_runs_with_one_round():
    """max_rounds=1 leaves nodes unmatched after the parallel round on a dense event: the finisher takes them."""
    ei, ptr = _sym_random_graph([200], 8, seed=1)
    rowptr, col, _ = ref.to_csr(ei, 200)
    c1, p1, r1 = ref.graclus(rowptr, col, None, ptr, seed=5, max_rounds=1)
    c0, p0, r0 = ref.graclus(rowptr, col, None, ptr, seed=5)
    assert r1[0] == 1 and r0[0] > 1
    ref.check_matching(c1, p1, ei, ptr)
    assert not np.array_equal(c1, c0)


def test_reference_colour_function_and_tie_rule():
    assert ref.lowbias32(0) == 0
    assert ref._best([4, 2, 9], [1.0, 1.0, 1.0]) == 4             # all equal: the first candidate
    assert ref._best([4, 2, 9], [1.0, 3.0, 3.0]) == 2             # strictly greater only
    assert ref._best([4, 2], [float("nan"), 5.0]) == 4            # IEEE compare: nothing beats a leading NaN
    assert ref._best([4, 2, 9], None) == 4
    # both colours occur, and they change between rounds
    s = 99
    k0, k1 = ref.lowbias32(s), ref.lowbias32((s + 0x9E3779B9) & ref.M32)
    c0 = [ref.is_red(u, k0) for u in range(256)]
    c1 = [ref.is_red(u, k1) for u in range(256)]
    assert 64 < sum(c0) < 192 and c0 != c1


def test_reference_self_loops_and_duplicates_are_harmless():
    ei, ptr = _sym_random_graph([40], 3, seed=4)
    loops = np.stack([np.arange(40), np.arange(40)])
    ei2 = np.concatenate([ei, loops, ei[:, :10]], axis=1)
    a = ref.graclus(*ref.to_csr(ei, 40)[:2], None, ptr, seed=8)
    b = ref.graclus(*ref.to_csr(ei2, 40)[:2], None, ptr, seed=8)
    assert np.array_equal(a[0], b[0])


# ---- the C entries: argument validation through ctypes, no GPU ---------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from deepmetv2_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
            pytest.skip("libdmet_hip.so not built and no hipcc here")
        build.build_hip()
    return _lib.load()


def test_graclus_argument_validation(lib):
    assert lib.dmet_graclus_workspace_bytes(1000) == 8000
    rc = lib.dmet_graclus_f32(None, None, None, None, 1, -1, 0, 0, None, None, None, None, 0, None)
    assert rc == -22 and b"bad sizes" in lib.dmet_last_error()
    rc = lib.dmet_graclus_f32(None, None, None, None, 1, 10, 0, -1, None, None, None, None, 0, None)
    assert rc == -22 and b"max_rounds=-1" in lib.dmet_last_error()
    rc = lib.dmet_graclus_f32(None, None, None, None, 1, 10, 0, 0, None, None, None, None, 0, None)
    assert rc == -22 and b"null pointer" in lib.dmet_last_error()
    assert lib.dmet_graclus_f32(None, None, None, None, 0, 0, 7, 0, None, None, None, None, 0, None) == 0


def test_normalized_cut_argument_validation(lib):
    assert lib.dmet_normalized_cut_workspace_bytes(10) == 40
    rc = lib.dmet_normalized_cut_2d_f32(None, None, 10, 10, None, 65, None, None, 0, None)
    assert rc == -22 and b"D=65" in lib.dmet_last_error()
    rc = lib.dmet_normalized_cut_2d_f32(None, None, 10, 10, None, 0, None, None, 0, None)
    assert rc == -22 and b"D=0" in lib.dmet_last_error()
    rc = lib.dmet_normalized_cut_f32(None, None, -1, 10, None, None, None, 0, None)
    assert rc == -22 and b"bad sizes" in lib.dmet_last_error()
    rc = lib.dmet_normalized_cut_f32(None, None, 5, 0, None, None, None, 0, None)
    assert rc == -22 and b"N=0" in lib.dmet_last_error()
    rc = lib.dmet_normalized_cut_f32(None, None, 5, 5, None, None, None, 0, None)
    assert rc == -22 and b"null pointer" in lib.dmet_last_error()
    assert lib.dmet_normalized_cut_f32(None, None, 0, 0, None, None, None, 0, None) == 0
    assert lib.dmet_normalized_cut_2d_f32(None, None, 0, 5, None, 64, None, None, 0, None) == 0


def test_pool_pairs_argument_validation(lib):
    assert lib.dmet_pool_pairs_workspace_bytes(100, 4) == 416
    rc = lib.dmet_pool_pairs_index(None, None, 1, -1, None, None, None, 0, None)
    assert rc == -22 and b"bad sizes" in lib.dmet_last_error()
    rc = lib.dmet_pool_pairs_index(None, None, 0, 5, None, None, None, 0, None)
    assert rc == -22 and b"B=0" in lib.dmet_last_error()
    rc = lib.dmet_pool_pairs_index(None, None, 2, 5, None, None, None, 0, None)
    assert rc == -22 and b"null pointer" in lib.dmet_last_error()
    assert lib.dmet_pool_pairs_index(None, None, 0, 0, None, None, None, 0, None) == 0
    rc = lib.dmet_pool_pairs_f32(None, 10, 0, None, None, None, 1, 5, None, None, None, None, None)
    assert rc == -22 and b"F=0" in lib.dmet_last_error()
    rc = lib.dmet_pool_pairs_f32(None, 10, 4, None, None, None, 1, 11, None, None, None, None, None)
    assert rc == -22 and b"C=11" in lib.dmet_last_error()
    rc = lib.dmet_pool_pairs_f32(None, 10, 4, None, None, None, 1, 5, None, None, None, None, None)
    assert rc == -22 and b"null pointer" in lib.dmet_last_error()
    assert lib.dmet_pool_pairs_f32(None, 0, 4, None, None, None, 1, 0, None, None, None, None, None) == 0
    rc = lib.dmet_pool_pairs_bwd_f32(None, None, None, None, None, 10, 4, 11, None, None)
    assert rc == -22 and b"C=11" in lib.dmet_last_error()
    rc = lib.dmet_pool_pairs_bwd_f32(None, None, None, None, None, 10, 4, 5, None, None)
    assert rc == -22 and b"null pointer" in lib.dmet_last_error()
    assert lib.dmet_pool_pairs_bwd_f32(None, None, None, None, None, 0, 4, 0, None, None) == 0


# ---- Python-level errors ---------------------------------------------------------------------------------------------
def test_python_errors_without_a_gpu():
    import deepmetv2_amd as dm
    ei = torch.tensor([[0, 1], [1, 0]])
    x = torch.randn(2, 3)
    cl = torch.tensor([0, 0])
    b = torch.zeros(2, dtype=torch.long)
    with pytest.raises(NotImplementedError):
        dm.max_pool_x(cl, x, b, size=4)
    with pytest.raises(NotImplementedError):
        dm.avg_pool_x(cl, x, b, batch_size=1, size=4)
    for call in (lambda: dm.graclus(ei), lambda: dm.normalized_cut(ei, torch.ones(2)),
                 lambda: dm.normalized_cut_2d(ei, x), lambda: dm.max_pool_x(cl, x, b), lambda: dm.avg_pool_x(cl, x, b),
                 lambda: dm.global_max_pool(x, b), lambda: dm.global_mean_pool(x, None),
                 lambda: dm.global_add_pool(x, b)):
        with pytest.raises(RuntimeError, match="non-GPU tensor"):
            call()
