"""K1, second filter form: the squared norms and the admission threshold are folded into the matrix product
(csrc/knn_filter.h f2_block / f2_tau16), so each key block comes out as |x_j|^2 - 2 x_i.x_j - tau_rep.  These cases aim at
that arithmetic -- the fixed fp16 scales of the norm terms and of the two threshold terms, the directed rounding of
tau_rep and of the tile minima, the forced rows at the norm limit -- and compare the table with the C oracle bit for
bit, on events of exactly 800 nodes (the form's lower limit) and 4500 nodes, at 32 and 64 features."""
import pytest
import torch

NORM_MAX = 65504.0 * 2.0 ** 15     # csrc/knn_filter.h kF2NormMax: a row at or beyond this squared norm is a forced candidate


def _ptr(sizes):
    return torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(sizes, dtype=torch.int64).cumsum(0)])


def _knn_vs_oracle(dev, x, sizes, k):
    from deepmetv2_amd import _native
    from oracle import ref_ops
    ptr = _ptr(sizes)
    nbr_ref, dist_ref = ref_ops.knn_table(x, ptr, k)
    st = {}
    nbr, dist, _loc = _native.knn_local(x.to(dev), ptr.to(dev), k, stats=st)
    nbr, dist = nbr.cpu(), dist.cpu()
    bad = (nbr != nbr_ref).any(1).nonzero().view(-1)
    assert bad.numel() == 0, f"{bad.numel()} rows differ, first {bad[:5].tolist()}, stats {st}"
    assert torch.equal(dist, dist_ref), st
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("D", [32, 64])
@pytest.mark.parametrize("case", ["norm_limit", "large_norms", "tiny_norms", "negative_tau", "ties_at_tau",
                                  "fp16_subnormal", "one_row_beyond_range"])
def test_knn_folded_threshold_matches_oracle(dev, case, D):
    g = torch.Generator().manual_seed(4500 + D + len(case))
    sizes = [4500, 800]
    N, k = sum(sizes), 16
    x = torch.randn(N, D, generator=g)
    if case == "norm_limit":
        # rows whose squared norm sits just below / above the fold's limit with every feature well inside fp16
        # (|v| ~ 8190 at 32 features): below, the four norm terms carry it; above, the row is a forced candidate
        idx = torch.randperm(N, generator=g)[:24]
        for i, r in enumerate(idx.tolist()):
            f = 0.999 if i % 2 == 0 else 1.001
            x[r] = torch.full((D,), (NORM_MAX * f / D) ** 0.5) * torch.sign(torch.randn(D, generator=g))
    elif case == "large_norms":
        x = x * 1000.0                # thresholds ~ -3e7: the 2^14 scale and its remainder term
    elif case == "tiny_norms":
        x = x * 1.0e-4                # thresholds ~ -3e-7: the 2^-15 scale alone
    elif case == "negative_tau":
        x = x + 3.0                   # every key negative, tau ~ -|x_i|^2
    elif case == "ties_at_tau":
        x = torch.round(x * 2.0)      # integer keys: many tile minima (and keys) exactly at the threshold
    elif case == "fp16_subnormal":
        x = x * 2.0e-6                # every feature an fp16 subnormal, squared norms ~1e-10
    elif case == "one_row_beyond_range":
        x[int(torch.randint(0, N, (1,), generator=g))] *= 3.0e4
    st = _knn_vs_oracle(dev, x.contiguous(), sizes, k)
    if case in ("large_norms", "tiny_norms", "negative_tau", "ties_at_tau", "one_row_beyond_range"):
        # the fold must certify these by itself: a range edge that sent them to the exact kernel would pass the table
        # comparison above unnoticed (one_row_beyond_range: that row as a query, plus one)
        assert st["flagged_queries"] <= 2, st
    # norm_limit: the rows beyond the limit are forced candidates of every query, which overflows most lanes' entry
    # lists -- the table is what is checked there; fp16_subnormal: the certificate cannot hold at this scale (fp16
    # subnormal steps of 6e-8 against features of 2e-6), the table is what is checked
