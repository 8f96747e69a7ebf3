"""K1, second filter form: the final threshold of a first attempt is min(tk[M-1], cut) with the cut a margin above
tk[k-1], the k-th smallest tile minimum (csrc/knn_filter.h f2_cut), instead of tk[M-1] alone.  The certificate is
evaluated with the threshold that was applied, and a lane whose cut was too tight takes the second attempt.  Every case
runs three ways -- DMET_KNN_CUT unset (the default margin), "0" (no cut) and "0.0" (margin scale zero: the cut is
tk[k-1] itself, so the second attempt and the exact fallback carry the build) -- and the table is compared with the C
oracle bit for bit, ids and distances.  Events of 800 nodes (the form's lower limit; swept whole) and 2600 nodes (above
kF2SplitMinNodes = 2560: in a batch this small its tiles run as split items), 32 and 64 features, k = 16 and 20.

Second attempts at margin scale zero.  A query fails its certificate there when tk[k-1] lies within the slack of its
own k-th key, above all when its k nearest sit in k different tiles (tk[k-1] then IS the k-th key).  For k candidates
spread at random over T tiles that happens with probability prod_{i<k} (1 - i/T) ~ exp(-k (k-1) / 2T).  In the batch
above only the 800-node event can retry (split items have no second attempt) and it has T = 25 tiles: 0.8 % of its
queries at k = 16, about six, but 0.05 % at k = 20, less than one.  The gaussian case therefore also builds one event of
2000 nodes: below kF2SplitMinNodes, so swept whole, with T = 63 tiles -- 15 % of 2000 queries at k = 16, 5 % at k = 20 --
and asks for a non-zero second-attempt count there for every (D, k), with the table still the oracle's.
"""
import functools

import pytest
import torch

SIZES = (800, 2600)
CASES = ["gaussian", "ties", "negative_thresholds", "scaled_up", "scaled_down", "few_distinct_values", "forced_candidates"]
MODES = {"default": None, "off": "0", "scale0": "0.0"}


def _ptr(sizes):
    return torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(sizes, dtype=torch.int64).cumsum(0)])


@functools.lru_cache(maxsize=None)
def _case(case, D, k):
    """(x, ptr, oracle ids, oracle distances): built once per case, read-only afterwards."""
    from oracle import ref_ops
    g = torch.Generator().manual_seed(2600 + D + len(case))
    N = sum(SIZES)
    x = torch.randn(N, D, generator=g)
    if case == "ties":
        x = torch.round(x * 2.0)          # integer keys: many tile minima equal to tk[k-1] and to the cut
    elif case == "negative_thresholds":
        x = x + 3.0                       # every key negative: tk[k-1] and the cut are below zero
    elif case == "scaled_up":
        x = x * 1000.0                    # the fold's 2^14 threshold scale and its remainder term
    elif case == "scaled_down":
        x = x * 1.0e-4                    # the 2^-15 scale alone
    elif case == "few_distinct_values":
        x = x[:40][torch.arange(N) % 40]  # tk[k-1] == tk[M-1]: the cut must fall back to tau
    elif case == "forced_candidates":
        x[int(torch.randint(0, N, (1,), generator=g))] *= 3.0e4    # one row beyond the fp16 range: key -inf
    x = x.contiguous()
    ptr = _ptr(SIZES)
    nbr_ref, dist_ref = ref_ops.knn_table(x, ptr, k)
    return x, ptr, nbr_ref, dist_ref


def _build(dev, monkeypatch, mode, x, ptr, k):
    from deepmetv2_amd import _native
    if MODES[mode] is None:
        monkeypatch.delenv("DMET_KNN_CUT", raising=False)
    else:
        monkeypatch.setenv("DMET_KNN_CUT", MODES[mode])
    st = {}
    nbr, dist, _loc = _native.knn_local(x.to(dev), ptr.to(dev), k, stats=st)
    return nbr.cpu(), dist.cpu(), st


@pytest.mark.gpu
@pytest.mark.parametrize("k", [16, 20])
@pytest.mark.parametrize("D", [32, 64])
@pytest.mark.parametrize("case", CASES)
def test_knn_cut_matches_oracle(dev, monkeypatch, case, D, k):
    x, ptr, nbr_ref, dist_ref = _case(case, D, k)
    stats = {}
    for mode in MODES:
        nbr, dist, st = _build(dev, monkeypatch, mode, x, ptr, k)
        print(f"{case} D={D} k={k} {mode}: {st}")
        bad = (nbr != nbr_ref).any(1).nonzero().view(-1)
        assert bad.numel() == 0, f"{mode}: {bad.numel()} rows differ, first {bad[:5].tolist()}, stats {st}"
        assert torch.equal(dist, dist_ref), (mode, st)
        stats[mode] = st
    if case in ("gaussian", "negative_thresholds", "scaled_up", "scaled_down", "ties"):
        # the default margin must not hand more queries to the exact path than tk[M-1] alone does
        assert stats["default"]["flagged_queries"] <= stats["off"]["flagged_queries"], stats


@pytest.mark.gpu
@pytest.mark.parametrize("k", [16, 20])
@pytest.mark.parametrize("D", [32, 64])
def test_knn_cut_scale_zero_takes_second_attempts(dev, monkeypatch, D, k):
    """The safety net at work (see the module docstring): gaussian data, the batch of the other test and one whole-swept
    event of 2000 nodes, cut at tk[k-1].  Queries whose cut is too tight must retry and come back with the oracle's rows."""
    from oracle import ref_ops
    counts = []
    x0, ptr0, nbr0, dist0 = _case("gaussian", D, k)
    g = torch.Generator().manual_seed(2000 + D + k)
    x1 = torch.randn(2000, D, generator=g)
    ptr1 = _ptr((2000,))
    nbr1, dist1 = ref_ops.knn_table(x1, ptr1, k)
    for x, ptr, nbr_ref, dist_ref in ((x0, ptr0, nbr0, dist0), (x1, ptr1, nbr1, dist1)):
        nbr, dist, st = _build(dev, monkeypatch, "scale0", x, ptr, k)
        print(f"scale0 D={D} k={k} sizes={ptr.diff().tolist()}: {st}")
        assert torch.equal(nbr, nbr_ref) and torch.equal(dist, dist_ref), st
        counts.append(st["second_attempts"])
    assert counts[1] > 0, counts
