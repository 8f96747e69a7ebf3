"""K1, second filter form, 32 features: the query side of the fold MFMA -- {y0, y1, 0, 0, P1..P4} for each of the two
32-query blocks -- is built once per sweep (csrc/knn_filter.h f2_sweep) and held in registers; a tile that converts the
threshold rewrites the threshold dword of both operands from one v_permlane32_swap (f2_fold_tau), every other tile, the
revisit of the deferred tiles and the second attempt read them as they are.  A pair's operands exchanged, or an operand
left at 0 or at a stale threshold where a sweep starts (after the cut, with t_fix, for the deferred pass), hands a query
a threshold that admits fewer than k candidates: wrong rows or flagged queries, never a silent pass.  Everything goes
through _native.knn_local and is compared with the C oracle bit for bit, ids and distances.

Shapes: ONE batch of events of 1040, 1072, 1104, 1136, 1168, 1200, 2000 and 2600 nodes.  The first six have 33..38
tiles of 32 rows, i.e. main sweeps of 1..6 tiles behind the 32 deferred ones: every exit of the six-way unrolled loop.
The 2000-node event is swept whole (63 tiles), the 2600-node event runs as split items.  k = 16 and 20 at 32 features;
64 features once (the sweep's signature is shared).

Data: gaussian; gaussian + 3 (negative thresholds); "pair_asymmetric" -- gaussian rows whose index inside their event
lies in an odd 32-row block are multiplied by 4, so the two queries of every lane pair (query blocks 0 and 1 of a work
item) need thresholds that differ by more than 22 in key space (d_16 - |x|^2 is about +5..8 for the even blocks and
-53..-69 for the odd ones).

Flagged queries and second attempts are deterministic for a given input: PARENT holds what the commit before this
change returned for these inputs on an MI355X, and the change may not exceed them.
"""
import functools

import pytest
import torch

SIZES = (1040, 1072, 1104, 1136, 1168, 1200, 2000, 2600)
CASES = ("gaussian", "negative_thresholds", "pair_asymmetric")
# (case, D, k) -> (flagged_queries, second_attempts) of the parent commit (600ffad), measured on one MI355X with
# exactly these inputs before the fold operands were made persistent (gaussian + 3 has second attempts: its
# rows have squared norms of ~320, and the certificate's slack grows with the norms, see f2_slack)
PARENT = {
    ("gaussian", 32, 16): (0, 0),
    ("gaussian", 32, 20): (0, 1),
    ("negative_thresholds", 32, 16): (0, 42),
    ("negative_thresholds", 32, 20): (1, 65),
    ("pair_asymmetric", 32, 16): (0, 0),
    ("pair_asymmetric", 32, 20): (0, 0),
    ("gaussian", 64, 16): (0, 0),
}


def _ptr(sizes):
    return torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(sizes, dtype=torch.int64).cumsum(0)])


def _data(case, sizes, D):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(sum(sizes), D, generator=g)
    if case == "negative_thresholds":
        x = x + 3.0
    elif case == "pair_asymmetric":
        local = torch.cat([torch.arange(n) for n in sizes])      # index inside the event
        x = x * torch.where((local // 32) % 2 == 1, 4.0, 1.0).unsqueeze(1)
    return x.contiguous()


@functools.lru_cache(maxsize=None)
def _case(case, D, k, sizes=SIZES):
    """(x, ptr, oracle ids, oracle distances): built once per case, read-only afterwards."""
    from oracle import ref_ops
    x, ptr = _data(case, sizes, D), _ptr(sizes)
    nbr_ref, dist_ref = ref_ops.knn_table(x, ptr, k)
    return x, ptr, nbr_ref, dist_ref


def _build(dev, x, ptr, k):
    from deepmetv2_amd import _native
    st = {}
    nbr, dist, _loc = _native.knn_local(x.to(dev), ptr.to(dev), k, stats=st)
    return nbr.cpu(), dist.cpu(), st


def _check(nbr, dist, nbr_ref, dist_ref, st):
    bad = (nbr != nbr_ref).any(1).nonzero().view(-1)
    assert bad.numel() == 0, f"{bad.numel()} rows differ, first {bad[:5].tolist()}, stats {st}"
    assert torch.equal(dist, dist_ref), st


@pytest.mark.gpu
@pytest.mark.parametrize("case,D,k", sorted(PARENT))
def test_fold_operands_match_oracle(dev, monkeypatch, case, D, k):
    monkeypatch.delenv("DMET_KNN_CUT", raising=False)
    x, ptr, nbr_ref, dist_ref = _case(case, D, k)
    nbr, dist, st = _build(dev, x, ptr, k)
    print(f"{case} D={D} k={k}: {st}")
    _check(nbr, dist, nbr_ref, dist_ref, st)
    flagged, second = PARENT[(case, D, k)]
    assert st["flagged_queries"] <= flagged, st
    assert st["second_attempts"] <= second, st


def test_pair_asymmetric_thresholds_differ():
    """The premise of the pair_asymmetric case, from the oracle alone (no GPU): for every lane pair of every event --
    queries 64 i + c and 64 i + 32 + c -- the thresholds d_16 - |x|^2 of the two queries lie more than 22 apart."""
    x, ptr, _nbr, dist_ref = _case("pair_asymmetric", 32, 16)
    key = dist_ref[:, 15] - (x * x).sum(1)
    for lo, hi in zip(ptr[:-1].tolist(), ptr[1:].tolist()):
        loc = torch.arange(hi - lo)
        even = loc[(loc // 32) % 2 == 0]
        even = even[even + 32 < hi - lo]
        gap = key[lo + even] - key[lo + even + 32]
        assert float(gap.min()) > 22.0, (hi - lo, float(gap.min()))


@pytest.mark.gpu
@pytest.mark.parametrize("k", [16, 20])
def test_second_attempt_rebuilds_operands(dev, monkeypatch, k):
    """One whole-swept gaussian event of 2000 nodes with the cut at tk[k-1] itself (DMET_KNN_CUT=0.0): queries whose k
    nearest sit in k different tiles fail the certificate and sweep again against t_fix.  A second attempt that kept the
    first attempt's operands (or zeros) would return short or wrong rows, or flag its queries."""
    monkeypatch.setenv("DMET_KNN_CUT", "0.0")
    x, ptr, nbr_ref, dist_ref = _case("gaussian", 32, k, (2000,))
    nbr, dist, st = _build(dev, x, ptr, k)
    print(f"scale0 k={k}: {st}")
    assert st["second_attempts"] > 0, st
    _check(nbr, dist, nbr_ref, dist_ref, st)
