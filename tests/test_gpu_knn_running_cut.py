"""K1, second filter form: the main sweep records its hit masks against the running cut min(tk[M-1], tk[KP-1] + margin)
(csrc/knn_filter.h f2_running_tau) instead of tk[M-1] alone; the cut above the final tk[k-1] is still applied after the
sweep.  The change may only remove stray mask bits and entries: tables, flagged queries and second attempts are those of
the sweep without it, which the same library runs under DMET_KNN_RUNCUT=0.

Shapes: ONE batch of events of
   800 nodes   every tile is deferred (kF2Defer = 32 tiles): the running cut never acts
  1056 nodes   one main-sweep tile
  1100 nodes   three main-sweep tiles, the last one partial
  2000 nodes   whole sweep, 31 main-sweep tiles
  2600 nodes   above kF2SplitMinNodes = 2560: in a batch this small two split items of 41 tiles each, no second attempt
k = 16 and 20 at 32 features, k = 16 at 64 features, and k = 10 at 32 features, which runs on the <16,1> instance with
k != KP: the running cut is off there (the margin stays +inf).

Data (seed 8):
  gaussian       randn.
  large_norms    randn + 3: |x|^2 ~ 320, so the slack and with it the margin are large, and every key is negative.
  grid           randn rounded to multiples of 1/2: keys are multiples of 1/4, tile minima tie in masses -- tk[k-1] ==
                 tk[M-1] for many queries, where the cut has to fall back to tk[M-1].
  scaled_blocks  the rows of every odd 32-row block (one candidate tile) scaled by 4: tile minima that alternate between
                 two scales, thresholds that drop in steps.

Every build is compared with the C oracle bit for bit, ids and distances; the oracle's table is computed once per (case,
features) at 27 (23) columns, of which a build's k columns are a prefix (the oracle orders by (distance, id)).  The
premise that the second form, not the exact fallback, produces these tables is checked twice: from the oracle alone
(test_reference_certifies_the_data) and on the GPU (fewer than a tenth of the rows flagged with DMET_KNN_RUNCUT=0).
"""
import functools

import pytest
import torch

SIZES = (800, 1056, 1100, 2000, 2600)
CASES = ("gaussian", "large_norms", "grid", "scaled_blocks")
PARAMS = ((32, 16), (32, 20), (64, 16), (32, 10))
KMAX = {32: 20, 64: 16}
SENTINEL = 1.0e10     # kKnnSentinel: the distance of an empty slot
TIE_RUN = 8           # M - k <= 6 list slots beyond the k-th, the k-th itself, and one more
COLS = {D: kmax + TIE_RUN - 1 for D, kmax in KMAX.items()}     # columns of the oracle's table


def _ptr(sizes):
    return torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(sizes, dtype=torch.int64).cumsum(0)])


def _data(case, sizes, D):
    g = torch.Generator().manual_seed(8)
    x = torch.randn(sum(sizes), D, generator=g)
    if case == "large_norms":
        x = x + 3.0
    elif case == "grid":
        x = torch.round(x * 2.0) / 2.0
    elif case == "scaled_blocks":
        lo = 0
        for n in sizes:      # candidate tiles are 32 rows of one event
            r = torch.arange(n)
            x[lo + r[(r // 32) % 2 == 1]] *= 4.0
            lo += n
    return x.contiguous()


@functools.lru_cache(maxsize=None)
def _ref(case, D, sizes=SIZES):
    """(x, ptr, oracle ids, oracle distances) at COLS columns: built once, read-only afterwards."""
    from oracle import ref_ops
    x, ptr = _data(case, sizes, D), _ptr(sizes)
    nbr, dist = ref_ops.knn_table(x, ptr, COLS[D])
    return x, ptr, nbr, dist


def _build(dev, monkeypatch, x, ptr, k, cut, runcut):
    from deepmetv2_amd import _native
    for name, value in (("DMET_KNN_CUT", cut), ("DMET_KNN_RUNCUT", runcut)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    st = {}
    nbr, dist, _loc = _native.knn_local(x.to(dev), ptr.to(dev), k, stats=st)
    return nbr.cpu(), dist.cpu(), st


def _check(nbr, dist, nbr_ref, dist_ref, k, what, st):
    bad = (nbr != nbr_ref[:, :k]).any(1).nonzero().view(-1)
    assert bad.numel() == 0, f"{what}: {bad.numel()} rows differ, first {bad[:5].tolist()}, stats {st}"
    assert torch.equal(dist, dist_ref[:, :k]), (what, st)


@pytest.mark.parametrize("D,k", PARAMS)
@pytest.mark.parametrize("case", CASES)
def test_reference_certifies_the_data(case, D, k):
    """From the oracle alone (no GPU): every k-th distance is finite, and fewer than a tenth of the rows have a run of
    TIE_RUN equal distances from the k-th on.  (A tie of two or three at d_k is no obstacle: the re-rank orders equal
    distances by id.  A query is at risk when more candidates tie at d_k than its threshold list has slots beyond the
    k-th, M - k <= 6: their tiles then all sit at the threshold.)"""
    _x, _p, _nbr, dist = _ref(case, D)
    dk = dist[:, k - 1]
    assert bool(torch.isfinite(dk).all()) and float(dk.max()) < SENTINEL
    pairs = int((dist[:, k] == dk).sum())
    tied = int((dist[:, k - 1 + TIE_RUN - 1] == dk).sum())
    print(f"{case} D={D} k={k}: d_k in [{float(dk.min()):.4g}, {float(dk.max()):.4g}], {pairs} rows with d_k = d_(k+1), "
          f"{tied} with {TIE_RUN} equal distances from d_k on")
    assert tied < sum(SIZES) // 10, tied


@pytest.mark.gpu
@pytest.mark.parametrize("D,k", PARAMS)
@pytest.mark.parametrize("case", CASES)
def test_running_cut_keeps_tables_and_counters(dev, monkeypatch, case, D, k):
    x, ptr, nbr_ref, dist_ref = _ref(case, D)
    for cut in (None, "off"):
        stats = {}
        for runcut in (None, "0"):
            nbr, dist, st = _build(dev, monkeypatch, x, ptr, k, cut, runcut)
            print(f"{case} D={D} k={k} DMET_KNN_CUT={cut} DMET_KNN_RUNCUT={runcut}: {st}")
            _check(nbr, dist, nbr_ref, dist_ref, k, (cut, runcut), st)
            stats[runcut] = st
        assert stats[None] == stats["0"], (cut, stats)
        # the premise: these tables come from the second form, not from the exact fallback
        assert stats["0"]["flagged_queries"] < sum(SIZES) // 10, (cut, stats)


@pytest.mark.gpu
@pytest.mark.parametrize("D,k", PARAMS)
def test_running_cut_at_margin_zero_takes_second_attempts(dev, monkeypatch, D, k):
    """DMET_KNN_CUT=0.0 on one whole-swept gaussian event of 2000 nodes: the cut is tk[k-1] itself.  Queries whose k
    nearest sit in k different tiles fail their certificate and must retry, as many as without the running cut, and
    come back with the oracle's rows.  (A running cut at a margin of zero changed these counts -- at 32 features, k = 16,
    49 flagged / 616 retried queries against 20 / 649: the first attempt's k candidates then rested on stray bits -- so
    the kernel leaves it off there: see f2_running_tau.)"""
    x, ptr, nbr_ref, dist_ref = _ref("gaussian", D, (2000,))
    stats = {}
    for runcut in (None, "0"):
        nbr, dist, st = _build(dev, monkeypatch, x, ptr, k, "0.0", runcut)
        print(f"scale0 D={D} k={k} DMET_KNN_RUNCUT={runcut}: {st}")
        _check(nbr, dist, nbr_ref, dist_ref, k, runcut, st)
        stats[runcut] = st
    assert stats[None] == stats["0"], stats
    assert stats[None]["second_attempts"] > 0, stats
