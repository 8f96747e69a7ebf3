"""K1, second filter form: the exact re-rank keeps each query's sorted top-KP as 64-bit words (distance bits << 32 | id)
and inserts a candidate with one v_min_f64 + one v_max_f64 per slot, the words read as doubles (csrc/knn_key64.h), at
all three sites: the 32-feature round, the 64-feature loop and the merge of the two halves of a split item.  What can
go wrong only on the GPU: f64 subnormals flushed (a word with distance bits 0 IS a subnormal double: the self match
of every query, every duplicate row -- a flushed word loses its id), an operand quieted or canonicalised, a word at or
beyond the sentinel inserted.  Everything goes through _native.knn_local and is compared with the C oracle bit for
bit, ids and distances.

Shapes: ONE batch of events of 800, 1040 and 2600 nodes (4440 rows).  800 is the smallest second-form event, every
tile deferred; 1040 has a main sweep; 2600 runs as split items and takes the merge.  k = 16 and 20 at 32 features,
k = 16 at 64 features.

Data (seed 7):
  gaussian    randn.
  grid        randn rounded to multiples of 2^-4: the chain's arithmetic is exact, equal distances occur and the id
              decides (test_grid_has_ties counts them from the oracle: rows with a tie inside their top 16, rows with
              d_16 = d_17).
  duplicates  per event a tenth of the rows copied onto another tenth and a fiftieth copied a second time: 712 rows
              with two and 264 rows with three zero distances (test_duplicates_have_zero_runs); these lists begin with
              several words of high word 0, ordered by id alone.
  beyond      2 % of the rows scaled by 1e5..1e6 (forced candidates of every query that must never be inserted), and
              four rows each with a NaN, a +inf and a -inf feature.

Flagged queries and second attempts are deterministic for a given input: PARENT holds what the commit before this
change (861091d) returned for these inputs on an MI355X, in the same visit, and the change must return exactly those.
On the parent the grid and duplicates cases flag fewer than a tenth of the rows (PARENT below), so the re-rank, not the
exact fallback, is what these cases hold.
"""
import functools

import pytest
import torch

SIZES = (800, 1040, 2600)
CASES = ("gaussian", "grid", "duplicates", "beyond")
PARAMS = ((32, 16), (32, 20), (64, 16))
# (case, D, k) -> (flagged_queries, second_attempts) of the parent commit on one MI355X with exactly these inputs
# (the far rows of the beyond case are outside the fp16 operand range: most of its queries go to the exact kernels)
PARENT = {
    ("gaussian", 32, 16): (0, 0),
    ("gaussian", 32, 20): (0, 0),
    ("gaussian", 64, 16): (0, 0),
    ("grid", 32, 16): (0, 0),
    ("grid", 32, 20): (0, 0),
    ("grid", 64, 16): (0, 0),
    ("duplicates", 32, 16): (0, 0),
    ("duplicates", 32, 20): (0, 0),
    ("duplicates", 64, 16): (0, 0),
    ("beyond", 32, 16): (3658, 0),
    ("beyond", 32, 20): (3658, 0),
    ("beyond", 64, 16): (3651, 0),
}


def _ptr(sizes):
    return torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(sizes, dtype=torch.int64).cumsum(0)])


def _data(case, sizes, D):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(sum(sizes), D, generator=g)
    if case == "grid":
        x = torch.round(x * 16.0) / 16.0
    elif case == "duplicates":
        lo = 0
        for n in sizes:
            perm = lo + torch.randperm(n, generator=g)
            a, b = n // 10, n // 50
            x[perm[a:2 * a]] = x[perm[:a]]
            x[perm[2 * a:2 * a + b]] = x[perm[:b]]
            lo += n
    elif case == "beyond":
        N = sum(sizes)
        idx = torch.randperm(N, generator=g)
        far = idx[: N // 50]
        x[far] = x[far] * torch.empty(far.numel(), 1).uniform_(1e5, 1e6, generator=g)
        odd = idx[N // 50: N // 50 + 12]
        x[odd[0:4], 3] = float("nan")
        x[odd[4:8], 7] = float("inf")
        x[odd[8:12], 0] = float("-inf")
    return x.contiguous()


@functools.lru_cache(maxsize=None)
def _case(case, D, k):
    """(x, ptr, oracle ids, oracle distances): built once per case, read-only afterwards."""
    from oracle import ref_ops
    x, ptr = _data(case, SIZES, D), _ptr(SIZES)
    nbr_ref, dist_ref = ref_ops.knn_table(x, ptr, k)
    return x, ptr, nbr_ref, dist_ref


def _build(dev, x, ptr, k):
    from deepmetv2_amd import _native
    st = {}
    nbr, dist, _loc = _native.knn_local(x.to(dev), ptr.to(dev), k, stats=st)
    return nbr.cpu(), dist.cpu(), st


@pytest.mark.gpu
@pytest.mark.parametrize("D,k", PARAMS)
@pytest.mark.parametrize("case", CASES)
def test_rerank_keys_match_oracle(dev, monkeypatch, case, D, k):
    monkeypatch.delenv("DMET_KNN_CUT", raising=False)
    x, ptr, nbr_ref, dist_ref = _case(case, D, k)
    nbr, dist, st = _build(dev, x, ptr, k)
    print(f"{case} D={D} k={k}: {st}")
    bad = (nbr != nbr_ref).any(1).nonzero().view(-1)
    assert bad.numel() == 0, f"{bad.numel()} rows differ, first {bad[:5].tolist()}, stats {st}"
    assert torch.equal(dist, dist_ref), st
    flagged, second = PARENT[(case, D, k)]
    assert st["flagged_queries"] == flagged, st
    assert st["second_attempts"] == second, st


def test_parent_flags_leave_ties_to_the_rerank():
    """The premise of the grid and duplicates cases: on the parent fewer than a tenth of the rows went to the exact
    fallback, so the tables of those cases are the re-rank's."""
    for (case, _D, _k), (flagged, _second) in PARENT.items():
        if case in ("grid", "duplicates"):
            assert flagged < sum(SIZES) // 10, (case, flagged)
    assert sorted(PARENT) == sorted((c, D, k) for c in CASES for D, k in PARAMS)


@pytest.mark.parametrize("D", [32, 64])
def test_grid_has_ties(D):
    """From the oracle alone (no GPU): on the grid, equal distances occur inside the top 16 and across its edge."""
    from oracle import ref_ops
    x, ptr = _data("grid", SIZES, D), _ptr(SIZES)
    _nbr, dist = ref_ops.knn_table(x, ptr, 17)
    inside = int((dist[:, 1:16] == dist[:, :15]).any(1).sum())
    edge = int((dist[:, 15] == dist[:, 16]).sum())
    print(f"grid D={D}: {inside} rows with a tie inside their top 16, {edge} with d16 = d17")
    assert inside >= 100 and edge >= 10, (inside, edge)


def test_duplicates_have_zero_runs():
    """From the oracle alone: 712 rows see two zero distances, 264 see three, none more."""
    _x, _ptr_, _nbr, dist = _case("duplicates", 32, 16)
    zeros = (dist == 0.0).sum(1)
    assert [int((zeros == c).sum()) for c in (2, 3)] == [712, 264]
    assert int(zeros.max()) == 3 and int(zeros.min()) == 1
