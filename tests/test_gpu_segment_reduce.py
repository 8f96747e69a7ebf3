"""The kernels of csrc/segment.hip on the device against the float64 references of tests/segment_reference.py.

Notation: u = 2^-24, n the length of the row an element belongs to.  Every bound below comes from the issue that asked for
these operators or is derived in the docstring of its test; none was fitted to what the kernels give.  Each test prints
the largest error / bound ratio it saw before it asserts.

Forms: the kernels take a `max_len` hint; from 1024 on a workgroup owns a row, below (0: unknown) a wavefront.  Either
form accepts every length, so every case runs under the hints 0, 1023 (wavefront) and 1024, 1025, 4500 (workgroup) and
is held to the same reference: the two forms agree within the bounds, not in bits.  Inside a form a kernel changes path
where a row stops fitting one step of its team (it is then read a second time instead of kept in registers): at 16, 32,
64 and 256 entries in the wavefront form (CL = 64, 32, 4 | 16, 1) and at 64, 256 and 1024 in the workgroup form (CL =
16, 4, 1); LENGTHS holds T - 1, T, T + 1 of each.  Widths: the channel lanes of a team
change at H = 1 | 4 | 16 | 32 | 64, so H covers both sides of each beside the issue's {1, 3, 16, 33, 64, 100}."""
import pytest
import torch

import poisoned_alloc as pa
import segment_reference as sr

pytestmark = pytest.mark.gpu

U = sr.U
TINY = 2.0 ** -126
LENGTHS = [0, 1, 2, 15, 16, 17, 0, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4500, 0, 31, 32, 33, 0]
HINTS = (0, 1023, 1024, 1025, 4500)           # T - 1, T, T + 1 for the form's threshold T = 1024, and the true maximum
WIDTHS = [1, 2, 3, 4, 5, 16, 17, 32, 33, 64, 65, 100]
_cache = {}


def _rows(lengths=LENGTHS):
    key = ("rows", tuple(lengths)) if len(lengths) < 100 else ("rows", len(lengths), sum(lengths))
    if key not in _cache:
        rowptr = sr.lengths_rowptr(lengths)
        n_of = torch.tensor(lengths, dtype=torch.float64)[sr.row_ids(rowptr)].view(-1, 1)
        _cache[key] = (rowptr, n_of, torch.tensor(lengths, dtype=torch.float64).view(-1, 1))
    return _cache[key]


def _gauss(H, scale=5.0, lengths=LENGTHS, seed=0):
    key = ("gauss", H, scale, sum(lengths), len(lengths), seed)
    if key not in _cache:
        g = torch.Generator().manual_seed(1000 * seed + H)
        _cache[key] = torch.randn(sum(lengths), H, generator=g) * scale
    return _cache[key]


def _ints(H, lengths=LENGTHS):
    g = torch.Generator().manual_seed(77 + H)
    return torch.randint(-8, 9, (sum(lengths), H), generator=g).float()


def _ratio(err, bound, what):
    r = (err / bound.clamp(min=1e-300)).max().item() if err.numel() else 0.0
    print(f"{what}: max error / bound = {r:.3f}")
    return r


def _hold(got, ref, bound, what):
    got = got.double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    finite = torch.isfinite(ref)
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), f"{what}: NaN pattern differs"
    err = torch.where(finite, (got - ref).abs(), torch.zeros_like(ref))
    inf_wrong = ~finite & ~torch.isnan(ref) & (got != ref)                                        # an infinity: the same one
    err = torch.where(inf_wrong, torch.full_like(err, float("inf")), err)
    _ratio(err, bound, what)
    bad = (err > bound).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} elements outside the bound, first at {bad[0].tolist()}"


def _same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert pa.differing(a, b).numel() == 0, f"{what}: bits differ"


# ---- mean ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", WIDTHS)
def test_mean_exact_data_forward_and_backward(dev, H):
    """Small integers: every partial sum is exact in fp32 whatever its order, so the result is the one correctly rounded
    quotient fp32(sum) / fp32(max(count, 1)), bit for bit, and the backward is coef / count in fp32."""
    from deepmetv2_amd import _native
    rowptr, n_of, n_row = _rows()
    src = _ints(H)
    cnt = n_row.clamp(min=1).float()
    total = torch.zeros(len(LENGTHS), H, dtype=torch.float64).index_add(0, sr.row_ids(rowptr), src.double())
    want = total.float() / cnt                                              # the exact sum, then one fp32 division
    coef = torch.randint(-8, 9, (len(LENGTHS), H), generator=torch.Generator().manual_seed(H)).float()
    want_g = (coef / cnt)[sr.row_ids(rowptr)]
    sd, rd, cd = src.to(dev), rowptr.to(dev), coef.to(dev)
    for hint in HINTS:
        _same_bits(_native._segment_mean(sd, rd, hint).cpu(), want, f"mean H={H} hint={hint}")
        _same_bits(_native._segment_mean_bwd(cd, rd, src.shape[0], hint).cpu(), want_g, f"mean_bwd H={H} hint={hint}")


@pytest.mark.parametrize("H", WIDTHS)
def test_mean_gaussian(dev, H):
    """|out - ref| <= gamma_n * sum|x| / n with gamma_n = n*u / (1 - n*u): n - 1 additions in any order and one division."""
    from deepmetv2_amd import _native
    rowptr, _n_of, n_row = _rows()
    src = _gauss(H, 1.0)
    ref = sr.mean_ref(src, rowptr)
    gamma = n_row * U / (1 - n_row * U)
    bound = gamma * sr.mean_ref(src.abs(), rowptr)
    for hint in HINTS:
        _hold(_native._segment_mean(src.to(dev), rowptr.to(dev), hint), ref, bound, f"mean H={H} hint={hint}")


# ---- min -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", WIDTHS)
def test_min_values_arg_and_backward(dev, H):
    """Values bit for bit (so -0.0 against +0.0 follows the position) and arg as the lowest tied position, against the
    mirror of _max_ref; ties, +-0.0 and +-inf in the data; an empty row gives 0 and arg -1 (E at the public interface); the
    backward puts g_out at arg and zero everywhere else, exactly."""
    from deepmetv2_amd import _native
    rowptr, _n_of, _n_row = _rows()
    g = torch.Generator().manual_seed(300 + H)
    E = sum(LENGTHS)
    src = torch.randint(-3, 4, (E, H), generator=g).float()
    pick = torch.randint(0, 12, (E, H), generator=g)
    src = torch.where(pick == 0, torch.full_like(src, -0.0), src)
    src = torch.where(pick == 1, torch.full_like(src, float("inf")), src)
    src = torch.where(pick == 2, torch.full_like(src, -float("inf")), src)
    src[rowptr[8]:rowptr[9]] = float("inf")                      # a whole row of +inf: its first position wins
    src[rowptr[4]:rowptr[5]] = torch.tensor([0.0, -0.0] * 8).view(-1, 1)        # +0.0 before -0.0: a tie, +0.0 wins
    want, want_arg = sr.min_ref(src, rowptr)
    want_arg = torch.where(want_arg >= E, torch.full_like(want_arg, -1), want_arg).int()
    g_out = torch.randn(len(LENGTHS), H, generator=g)
    want_g = torch.zeros(E, H)
    cols = torch.arange(H).view(1, -1).expand(len(LENGTHS), H)
    won = want_arg >= 0
    want_g[want_arg[won].long(), cols[won]] = g_out[won]
    sd, rd = src.to(dev), rowptr.to(dev)
    for hint in HINTS:
        out, arg = _native._segment_min(sd, rd, hint)
        _same_bits(out.cpu(), want, f"min H={H} hint={hint}")
        assert torch.equal(arg.cpu(), want_arg), f"min arg H={H} hint={hint}"
        _same_bits(_native.segment_max_bwd(g_out.to(dev), arg, rd, E).cpu(), want_g, f"min_bwd H={H} hint={hint}")


# ---- softmax, log_softmax, logsumexp: forward -----------------------------------------------------------------------------------
def _softmax_bound(src, rowptr, n_of):
    d, _l, _m, _ids = sr.softmax_parts(src, rowptr)
    y = sr.softmax_ref(src, rowptr)
    return y, 2 * (n_of + d.abs() + 8) * U * y + TINY


@pytest.mark.parametrize("H", WIDTHS)
def test_softmax_forward(dev, H):
    """|y - y_ref| <= 2*(n + |s - m| + 8)*u*y_ref + 2^-126 against float64, scores Gaussian * 5: (n + 8)*u for l and the
    division, |s - m|*u for the rounding of s - m inside expf, doubled for the online rescale and expf itself.  The lse
    the same launch returns is held to the logsumexp bound."""
    from deepmetv2_amd import _native
    rowptr, n_of, n_row = _rows()
    src = _gauss(H)
    y_ref, bound = _softmax_bound(src, rowptr, n_of)
    lse_ref = sr.logsumexp_ref(src, rowptr)
    lse_bound = 2 * ((n_row + 8) * U + 2 * U * lse_ref.abs())
    for hint in HINTS:
        y, lse = _native._segment_softmax_fwd(src.to(dev), rowptr.to(dev), False, hint)
        _hold(y, y_ref, bound, f"softmax H={H} hint={hint}")
        _hold(lse, lse_ref, lse_bound, f"softmax lse H={H} hint={hint}")


@pytest.mark.parametrize("H", [1, 3, 16, 33, 64, 100])
def test_softmax_shifted_scores(dev, H):
    """s + 100 and s + 1e4 stay within the bound of the unshifted reference: the maximum is subtracted.  The scores are
    multiples of 2^-10 below 64 in size, so both shifted inputs are exact in fp32 and s - m is the same number."""
    from deepmetv2_amd import _native
    rowptr, n_of, _n_row = _rows()
    src = (_gauss(H) * 1024).round().clamp(-60000, 60000) / 1024
    y_ref, bound = _softmax_bound(src, rowptr, n_of)
    for shift in (100.0, 1.0e4):
        shifted = src + shift
        assert torch.equal(shifted.double(), src.double() + shift)
        for hint in (0, 4500):
            y, _ = _native._segment_softmax_fwd(shifted.to(dev), rowptr.to(dev), False, hint)
            _hold(y, y_ref, bound, f"softmax shift={shift} H={H} hint={hint}")


@pytest.mark.parametrize("H", [1, 3, 16, 33, 64, 100])
def test_softmax_special_rows(dev, H):
    """One entry gives exactly 1.0; -inf beside finite scores exactly 0; a row of -inf alone NaN (as torch.softmax); the
    same rows through log_softmax and logsumexp."""
    from deepmetv2_amd import _native
    lengths = [1, 5, 4, 0, 70, 1100]
    rowptr = sr.lengths_rowptr(lengths)
    g = torch.Generator().manual_seed(H)
    src = torch.randn(sum(lengths), H, generator=g) * 5
    ninf = -float("inf")
    src[2], src[4] = ninf, ninf                      # row 1: two -inf beside three finite scores
    src[6:10] = ninf                                 # row 2: -inf alone
    src[10 + 7], src[10 + 69] = ninf, ninf           # row 4
    src[80 + 500:80 + 900] = ninf                    # row 5: a long stretch of -inf, every lane of a team meets some
    ref = sr.softmax_ref(src, rowptr)
    assert torch.isnan(ref[6:10]).all() and (ref[2] == 0).all()
    n_of = torch.tensor(lengths, dtype=torch.float64)[sr.row_ids(rowptr)].view(-1, 1)
    for hint in (0, 1100):
        y, lse = _native._segment_softmax_fwd(src.to(dev), rowptr.to(dev), False, hint)
        y, lse = y.cpu(), lse.cpu()
        assert (y[0] == 1.0).all()
        assert (y[[2, 4, 17, 79]] == 0).all() and (y[580:980] == 0).all()
        assert torch.isnan(y[6:10]).all()
        assert (lse[3] == 0).all() and (lse[2] == ninf).all()
        keep = torch.ones(sum(lengths), dtype=torch.bool)
        keep[6:10] = False
        # the bound's |s - m| is taken where the score is finite; a -inf entry has y_ref = 0 and must be 0 exactly
        d, _l, _m, _ids = sr.softmax_parts(src, rowptr)
        b = 2 * (n_of + torch.where(torch.isfinite(d), d.abs(), torch.zeros_like(d)) + 8) * U * ref + TINY
        _hold(y[keep], ref[keep], b[keep], f"softmax special H={H} hint={hint}")
        ly, _ = _native._segment_softmax_fwd(src.to(dev), rowptr.to(dev), True, hint)
        ly = ly.cpu()
        assert (ly[0] == 0).all() and (ly[[2, 4, 17, 79]] == ninf).all() and torch.isnan(ly[6:10]).all()
        out = _native._segment_logsumexp(src.to(dev), rowptr.to(dev), hint).cpu()
        _same_bits(out, lse, "logsumexp against the softmax launch's lse")


@pytest.mark.parametrize("H", WIDTHS)
def test_logsumexp_and_log_softmax_forward(dev, H):
    """|out - ref| <= 2*((n + 8)*u + 2*u*|ref|) for both: (n + 8)*u for logf(l), u*|ref| for the rounding of s - m (at most
    |ref| for log_softmax, since |y| = |s - m| + log l) or of m, u*|ref| for the final addition; doubled as for softmax.
    An empty row of logsumexp gives 0."""
    from deepmetv2_amd import _native
    rowptr, n_of, n_row = _rows()
    src = _gauss(H)
    lse_ref, ls_ref = sr.logsumexp_ref(src, rowptr), sr.log_softmax_ref(src, rowptr)
    empty = [i for i, n in enumerate(LENGTHS) if n == 0]
    for hint in HINTS:
        out = _native._segment_logsumexp(src.to(dev), rowptr.to(dev), hint)
        assert (out.cpu()[empty] == 0).all()
        _hold(out, lse_ref, 2 * ((n_row + 8) * U + 2 * U * lse_ref.abs()), f"logsumexp H={H} hint={hint}")
        y, _ = _native._segment_softmax_fwd(src.to(dev), rowptr.to(dev), True, hint)
        _hold(y, ls_ref, 2 * ((n_of + 8) * U + 2 * U * ls_ref.abs()), f"log_softmax H={H} hint={hint}")


# ---- softmax, log_softmax, logsumexp: backward ----------------------------------------------------------------------------------
def _row_sum(t, rowptr):
    ids = sr.row_ids(rowptr)
    return torch.zeros((rowptr.numel() - 1, t.shape[1]), dtype=t.dtype).index_add(0, ids, t)[ids]


@pytest.mark.parametrize("H", WIDTHS)
def test_softmax_backward(dev, H):
    """Against float64 autograd of the reference composition:
    |g - g_ref| <= 4*(n + |s| + 8)*u*y_ref*(|g_out| + sum_row |y*g_out|): the relative error of y (forward bound) and of
    the row sum of y*g_out (n terms of relative error that of y), times the magnitude y*(|g_out| + sum|y*g_out|) of what
    they multiply."""
    from deepmetv2_amd import _native
    rowptr, n_of, _n_row = _rows()
    src = _gauss(H)
    g = _gauss(H, 1.0, seed=1)
    s64 = src.double().requires_grad_(True)
    (sr.softmax_ref(s64, rowptr) * g.double()).sum().backward()
    y_ref = sr.softmax_ref(src, rowptr)
    bound = 4 * (n_of + src.double().abs() + 8) * U * y_ref * (g.double().abs() + _row_sum((y_ref * g.double()).abs(), rowptr))
    for hint in HINTS:
        y, _ = _native._segment_softmax_fwd(src.to(dev), rowptr.to(dev), False, hint)
        _hold(_native._segment_softmax_bwd(y, g.to(dev), rowptr.to(dev), False, hint), s64.grad, bound,
              f"softmax_bwd H={H} hint={hint}")


@pytest.mark.parametrize("H", WIDTHS)
def test_log_softmax_backward(dev, H):
    """g_s = g - p*G with p = expf(y), G = sum_row g.  The kernel reads the forward's y, off by at most the forward bound
    B = 2*((n + 8) + 2|y_ref|)*u, so p is off by (B + 2u)*p (expf: 2u); G is off by at most n*u*sum_row|g| (n - 1
    additions in any order); the product and the subtraction round once each: u*p*|G| and u*|g_s|.  With |G| <= sum|g|:
    |g_s - ref| <= u*|ref| + p*(2(n + 8) + 4|y_ref| + 2 + n + 1)*u*sum_row|g|; doubled, as the other bounds are, for the
    second-order terms:  2*u*(|ref| + p*(3n + 4|y_ref| + 19)*sum_row|g|)."""
    from deepmetv2_amd import _native
    rowptr, n_of, _n_row = _rows()
    src = _gauss(H)
    g = _gauss(H, 1.0, seed=1)
    s64 = src.double().requires_grad_(True)
    (sr.log_softmax_ref(s64, rowptr) * g.double()).sum().backward()
    y_ref = sr.log_softmax_ref(src, rowptr)
    bound = 2 * U * (s64.grad.abs() + y_ref.exp() * (3 * n_of + 4 * y_ref.abs() + 19) * _row_sum(g.double().abs(), rowptr))
    for hint in HINTS:
        y, _ = _native._segment_softmax_fwd(src.to(dev), rowptr.to(dev), True, hint)
        _hold(_native._segment_softmax_bwd(y, g.to(dev), rowptr.to(dev), True, hint), s64.grad, bound,
              f"log_softmax_bwd H={H} hint={hint}")


@pytest.mark.parametrize("H", WIDTHS)
def test_logsumexp_backward(dev, H):
    """g_s = g_out*expf(s - out) = g_out*y_ref.  The kernel reads the forward's out, off by at most the forward bound
    B = 2*((n + 8) + 2|out|)*u; s - out rounds once, |s - out|*u; expf 2u; the product u.  Relative to |ref|:
    B + (|s - out| + 3)*u <= (2n + 4|out| + |s - out| + 19)*u; doubled for the second-order terms:
    2*(2n + 4|out| + |s - out| + 19)*u*|ref|."""
    from deepmetv2_amd import _native
    rowptr, n_of, _n_row = _rows()
    src = _gauss(H)
    g_out = torch.randn(len(LENGTHS), H, generator=torch.Generator().manual_seed(5 + H))
    s64 = src.double().requires_grad_(True)
    (sr.logsumexp_ref(s64, rowptr) * g_out.double()).sum().backward()
    out_of = sr.logsumexp_ref(src, rowptr)[sr.row_ids(rowptr)]
    bound = 2 * (2 * n_of + 4 * out_of.abs() + (src.double() - out_of).abs() + 19) * U * s64.grad.abs()
    for hint in HINTS:
        out = _native._segment_logsumexp(src.to(dev), rowptr.to(dev), hint)
        _hold(_native._segment_logsumexp_bwd(src.to(dev), out, g_out.to(dev), rowptr.to(dev), hint), s64.grad, bound,
              f"logsumexp_bwd H={H} hint={hint}")


# ---- many short rows, one very long row -----------------------------------------------------------------------------------------
def _all_ops_hold(dev, src, rowptr, n_of, n_row, hints, what):
    from deepmetv2_amd import _native
    sd, rd = src.to(dev), rowptr.to(dev)
    y_ref, y_bound = _softmax_bound(src, rowptr, n_of)
    lse_ref, ls_ref, mean_ref = sr.logsumexp_ref(src, rowptr), sr.log_softmax_ref(src, rowptr), sr.mean_ref(src, rowptr)
    mn, arg = sr.min_ref(src, rowptr)
    arg = torch.where(arg >= src.shape[0], torch.full_like(arg, -1), arg).int()
    g = torch.randn(src.shape, generator=torch.Generator().manual_seed(9))
    s64 = src.double().requires_grad_(True)
    (sr.softmax_ref(s64, rowptr) * g.double()).sum().backward()
    g_bound = 4 * (n_of + src.double().abs() + 8) * U * y_ref * (g.double().abs() + _row_sum((y_ref * g.double()).abs(), rowptr))
    for hint in hints:
        y, lse = _native._segment_softmax_fwd(sd, rd, False, hint)
        _hold(y, y_ref, y_bound, f"{what} softmax hint={hint}")
        _hold(lse, lse_ref, 2 * ((n_row + 8) * U + 2 * U * lse_ref.abs()), f"{what} lse hint={hint}")
        _hold(_native._segment_softmax_bwd(y, g.to(dev), rd, False, hint), s64.grad, g_bound, f"{what} softmax_bwd hint={hint}")
        ly, _ = _native._segment_softmax_fwd(sd, rd, True, hint)
        _hold(ly, ls_ref, 2 * ((n_of + 8) * U + 2 * U * ls_ref.abs()), f"{what} log_softmax hint={hint}")
        _hold(_native._segment_mean(sd, rd, hint), mean_ref, n_row * U / (1 - n_row * U) * sr.mean_ref(src.abs(), rowptr),
              f"{what} mean hint={hint}")
        out, a = _native._segment_min(sd, rd, hint)
        _same_bits(out.cpu(), mn, f"{what} min hint={hint}")
        assert torch.equal(a.cpu(), arg), f"{what} min arg hint={hint}"


def test_ten_thousand_short_rows(dev):
    """10^4 rows of 0..3 entries at H = 3: teams far outnumber a workgroup's four, most lanes of a team are idle."""
    g = torch.Generator().manual_seed(11)
    lengths = torch.randint(0, 4, (10000,), generator=g).tolist()
    rowptr, n_of, n_row = _rows(lengths)
    _all_ops_hold(dev, _gauss(3, lengths=lengths), rowptr, n_of, n_row, (0, 3), "short rows")


def test_one_row_of_a_million(dev):
    """A 1-D src (H = 1) that is one row of 10^6 entries, between two short rows that leave it at an odd, unaligned
    position: 16-byte loads where the alignment allows, the same entries per lane where it does not."""
    lengths = [3, 10 ** 6, 2]
    rowptr, n_of, n_row = _rows(lengths)
    _all_ops_hold(dev, _gauss(1, lengths=lengths), rowptr, n_of, n_row, (0, 10 ** 6), "10^6 row")


# ---- same bits ------------------------------------------------------------------------------------------------------------------
def _every_entry(dev, H, hint):
    from deepmetv2_amd import _native
    rowptr, _n_of, _n_row = _rows()
    sd, rd = _gauss(H).to(dev), rowptr.to(dev)
    gd = _gauss(H, 1.0, seed=1).to(dev)
    go = torch.randn(len(LENGTHS), H, generator=torch.Generator().manual_seed(3)).to(dev)

    def call():
        y, lse = _native._segment_softmax_fwd(sd, rd, False, hint)
        ly, _ = _native._segment_softmax_fwd(sd, rd, True, hint)
        out = _native._segment_logsumexp(sd, rd, hint)
        mn, arg = _native._segment_min(sd, rd, hint)
        return (y, lse, ly, out, mn, arg, _native._segment_mean(sd, rd, hint),
                _native._segment_mean_bwd(go, rd, sd.shape[0], hint), _native._segment_softmax_bwd(y, gd, rd, False, hint),
                _native._segment_softmax_bwd(ly, gd, rd, True, hint), _native._segment_logsumexp_bwd(sd, out, go, rd, hint))
    return call


@pytest.mark.parametrize("H", [1, 3, 16, 33, 100])
@pytest.mark.parametrize("hint", [0, 4500])
def test_same_bits_twice_and_under_poisoned_allocations(dev, H, hint):
    call = _every_entry(dev, H, hint)
    first = [t.cpu() for t in call()]
    for i, t in enumerate(call()):
        _same_bits(t.cpu(), first[i], f"second run, output {i}")
    for pattern, got in pa.run_both(call).items():
        for i, t in enumerate(got):
            _same_bits(t, first[i], f"poison {pattern}, output {i}")


def test_public_calls_same_bits_as_their_equals(dev):
    """A grouped index and the equal segment_csr call; scatter(reduce='sum' | 'max') and scatter_add / scatter_max; softmax
    with ptr, with a registered batch vector and with a plain index; an unsorted index and its sorted rows."""
    import deepmetv2_amd as dm
    lengths = [0, 5, 17, 0, 1300, 2, 0]
    n = len(lengths)
    indptr = sr.lengths_rowptr(lengths).long().to(dev)
    idx = torch.repeat_interleave(torch.arange(n), torch.tensor(lengths)).to(dev)
    for H in (1, 5, 33):
        src = _gauss(H, lengths=lengths).to(dev)
        for reduce in ("sum", "mean", "min", "max"):
            _same_bits(dm.segment_csr(src, indptr, reduce=reduce), dm.scatter(src, idx, dim=0, dim_size=n, reduce=reduce),
                       f"segment_csr {reduce} H={H}")
        _same_bits(dm.scatter(src, idx, dim=0, dim_size=n, reduce="sum"), dm.scatter_add(src, idx, dim=0, dim_size=n), "sum")
        _same_bits(dm.scatter(src, idx, dim=0, dim_size=n, reduce="max"), dm.scatter_max(src, idx, dim=0, dim_size=n)[0], "max")
        want = dm.scatter_softmax(src, idx, dim=0, dim_size=n)
        reg = idx.clone()
        dm.register_batch(reg, indptr, n, max_nodes=1300, min_nodes=0)
        _same_bits(dm.softmax(src, reg), want, f"softmax registered / index H={H}")      # both know the longest row
        # ptr alone gives the mean length as the hint: the other form.  Both are within 2*(n + |s - m| + 8)*u*y of the
        # truth, n <= 1300, |s - m| < 90
        _hold(dm.softmax(src, ptr=indptr), want.double().cpu(), 4 * 1400 * U * want.double().cpu() + TINY, "softmax ptr / index")
        perm = torch.randperm(src.shape[0], generator=torch.Generator().manual_seed(H)).to(dev)
        for fn in (dm.scatter_softmax, dm.scatter_log_softmax):
            shuffled = fn(src[perm].contiguous(), idx[perm], dim=0, dim_size=n)
            order = idx[perm].sort(stable=True).indices
            _same_bits(shuffled[order], fn(src[perm][order].contiguous(), idx[perm][order], dim=0, dim_size=n), fn.__name__)
    s1 = _gauss(1, lengths=lengths).view(-1).to(dev)
    _same_bits(dm.scatter_softmax(s1, idx, dim_size=n), dm.scatter_softmax(s1.view(-1, 1), idx, dim=0, dim_size=n).view(-1), "1-D")
    out, arg = dm.scatter_min(s1, idx, dim_size=n)
    assert (arg[[0, 3, 6]] == s1.numel()).all() and (out[[0, 3, 6]] == 0).all()
    live = torch.tensor([1, 2, 4, 5], device=dev)
    assert torch.equal(s1[arg[live]], out[live]) and torch.equal(idx[arg[live]], live)
    # an unsorted index with ties: arg goes back through the grouping's permutation, and since the grouping is stable
    # the lowest position in the CALLER's order wins a tie
    g = torch.Generator().manual_seed(8)
    E = 3000
    ties = torch.randint(-2, 3, (E, 5), generator=g).float()
    uidx = torch.randint(0, 9, (E,), generator=g)
    uidx[uidx == 4] = 7                                            # row 4 is empty
    out, arg = dm.scatter_min(ties.to(dev), uidx.to(dev), dim=0, dim_size=10)
    order = uidx.sort(stable=True).indices
    want, want_arg = sr.min_ref(ties[order], sr.lengths_rowptr(torch.bincount(uidx, minlength=10).tolist()))
    want_arg = torch.where(want_arg < E, order[want_arg.clamp(max=E - 1)], want_arg)
    _same_bits(out.cpu(), want, "scatter_min unsorted")
    assert torch.equal(arg.cpu(), want_arg) and (arg[4] == E).all() and (arg[9] == E).all()


def test_autograd_reaches_the_kernels(dev):
    """Each public function's gradient is its backward kernel's output on the grouped rows, put back in src's order."""
    import deepmetv2_amd as dm
    lengths = [4, 0, 1200, 9]
    n, H = len(lengths), 5
    rowptr = sr.lengths_rowptr(lengths)
    idx_sorted = torch.repeat_interleave(torch.arange(n), torch.tensor(lengths))
    perm = torch.randperm(sum(lengths), generator=torch.Generator().manual_seed(1))
    idx = idx_sorted[perm]
    src = _gauss(H, lengths=lengths)
    order = idx.sort(stable=True).indices
    inv = torch.empty_like(order)
    inv[order] = torch.arange(order.numel())
    n_of = torch.tensor(lengths, dtype=torch.float64)[idx].view(-1, 1)
    ge, gr = _gauss(H, 1.0, lengths=lengths, seed=2), torch.randn(n, H, generator=torch.Generator().manual_seed(2))
    for fn, ref, coef in ((dm.scatter_softmax, sr.softmax_ref, ge), (dm.scatter_log_softmax, sr.log_softmax_ref, ge),
                          (dm.scatter_logsumexp, sr.logsumexp_ref, gr), (dm.scatter_mean, sr.mean_ref, gr)):
        per_entry = coef is ge
        s = src.to(dev).requires_grad_(True)
        (fn(s, idx.to(dev), dim=0, dim_size=n) * coef.to(dev)).sum().backward()
        s64 = src.double().requires_grad_(True)
        r = ref(s64[order], rowptr)
        ((r[inv] if per_entry else r) * coef.double()).sum().backward()
        scale = _row_sum(coef.double().abs()[order] if per_entry else coef.double().abs()[sr.row_ids(rowptr)], rowptr)[inv]
        # the per-operator bounds are held above on the kernels themselves; here: the plumbing, to 8*(n + 83)*u of the row's
        # summed |coef|.  With |s| < 32 (asserted), |out| < 40 and |s - out| < 72, each of those bounds stays below it:
        # softmax 4*(n + 40)*u*2*sum|g|; log_softmax (6n + 46)*u*sum|g| (p*|log p| < 1/2); logsumexp (4n + 502)*u*|g_out|
        assert src.abs().max() < 32
        _hold(s.grad, s64.grad, 8 * (n_of + 83) * U * scale, f"{fn.__name__} autograd")


# ---- host syncs ----------------------------------------------------------------------------------------------------------------
def test_no_host_sync(dev):
    import deepmetv2_amd as dm
    lengths = [1, 3, 0, 17, 2049]
    B, N = len(lengths), sum(lengths)
    ptr = sr.lengths_rowptr(lengths).long().to(dev)
    batch = torch.repeat_interleave(torch.arange(B), torch.tensor(lengths)).to(dev)
    dm.register_batch(batch, ptr, B, max_nodes=2049, min_nodes=0)
    torch.manual_seed(0)
    src = torch.randn(N, 4, device=dev)
    x = torch.randn(N, 8, device=dev)
    agg = dm.AttentionalAggregation(torch.nn.Linear(8, 1), torch.nn.Linear(8, 8)).to(dev)
    agg(x, batch).sum().backward()              # first use: lazy initialisation of the libraries may sync
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = dm.softmax(src, ptr=ptr)
        b = dm.softmax(src, batch)
        c = dm.softmax(src[:, 0].contiguous(), batch)
        outs = [dm.segment_csr(src, ptr, reduce=r) for r in ("sum", "mean", "min", "max")]
        out = agg(x, batch)
        out.square().sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    # a (hint: the mean length) and b (the registered longest event) take different forms, c (H = 1) another lane layout
    # than b (H = 4): equal to rounding, not in bits.  Each is within 2*(n + |s - m| + 8)*u*y of the truth, n <= 2049 and
    # |s - m| < 100 for these standard normal scores, so two of them are within 4*2200*u*y of each other
    for other, same in ((a, b), (c.view(-1, 1), b[:, :1])):
        _hold(other, same.double().cpu(), 4 * 2200 * U * same.double().cpu() + TINY, "softmax forms")
    assert all(o.shape == (B, 4) for o in outs) and out.shape == (B, 8)


# ---- AttentionalAggregation -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gate_out", [1, 8])
def test_attentional_aggregation(dev, gate_out):
    """Events of [1, 3, 0, 17, 2049] nodes, F = 8, against the float64 composition (both Linears in float64 too).

    The fp32 Linears (8 products and a bias each) are off by at most ds_i = 9u*(|Wg||x_i| + |bg|) on the scores and
    dh_i = 9u*(|Wn||x_i| + |bn|) on the values; a score error reaches alpha at most doubled.
    Output: out = sum_i alpha_i*h_i.  alpha is off by the softmax bound, 2*(n + |s - m| + 8)*u relative, the segment sum adds
    n*u and the product u, relative to sum alpha*|h|.  Doubled, as the bounds it is made of:
        |out - ref| <= 2*((3n + 2*max|s - m| + 9)*u + 2*max ds) * sum_i alpha_i*|h_i| + 2*sum_i alpha_i*dh_i.
    Parameter gradients: each is a sum over all N nodes of per-node terms t_i*x_ik (bias: t_i).  For nn, t_i = alpha_i*c_b
    (c the upstream gradient): relative error that of alpha.  For gate_nn, t_i is the softmax backward, whose bound is
    4*(n + |s| + 8)*u * a_i with a_i = alpha_i*(|g_i| + sum_row alpha*|g|), g = c*h; |h| is taken as |Wn||x| + |bn|, the
    magnitude that the 9u of the Linear is relative to.  The sum over N nodes in fp32 adds N*u relative to
    sum |t_i*x_ik|, and |t_i| <= a_i; the Linears add their 9u and, through alpha, 2*max ds.
    So, with A the same sums taken over the magnitudes,
        |grad - ref| <= 2*((N + 4*(n_max + max|s| + 8) + 18)*u + 2*max ds) * A."""
    import deepmetv2_amd as dm
    lengths = [1, 3, 0, 17, 2049]
    B, N, F = len(lengths), sum(lengths), 8
    rowptr = sr.lengths_rowptr(lengths)
    ids = sr.row_ids(rowptr)
    torch.manual_seed(gate_out)
    x = torch.randn(N, F)
    coef = torch.randn(B, F)
    agg = dm.AttentionalAggregation(torch.nn.Linear(F, gate_out), torch.nn.Linear(F, F))
    ref_mod = dm.AttentionalAggregation(torch.nn.Linear(F, gate_out), torch.nn.Linear(F, F)).double()
    ref_mod.load_state_dict({k: v.double() for k, v in agg.state_dict().items()})
    s = ref_mod.gate_nn(x.double())
    h = ref_mod.nn(x.double())
    alpha = sr.softmax_ref(s, rowptr)
    ref = torch.zeros(B, F, dtype=torch.float64).index_add(0, ids, alpha * h)
    (ref * coef.double()).sum().backward()
    with torch.no_grad():
        d, _l, _m, _ = sr.softmax_parts(s, rowptr)
        n_max, smax, dmax = max(lengths), s.abs().max().item(), d.abs().max().item()
        n_row = torch.tensor(lengths, dtype=torch.float64).view(-1, 1)
        xa = x.double().abs()
        h_mag = xa @ ref_mod.nn.weight.abs().t() + ref_mod.nn.bias.abs()
        ds = (9 * U * (xa @ ref_mod.gate_nn.weight.abs().t() + ref_mod.gate_nn.bias.abs())).max().item()
        zero = torch.zeros(B, F, dtype=torch.float64)
        out_bound = 2 * ((3 * n_row + 2 * dmax + 9) * U + 2 * ds) * zero.index_add(0, ids, alpha * h.abs()) \
            + 2 * zero.index_add(0, ids, alpha * 9 * U * h_mag)
        k = 2 * ((N + 4 * (n_max + smax + 8) + 18) * U + 2 * ds)
        c_i = coef.double()[ids]
        t_nn = alpha.expand(N, F) * c_i.abs()                                        # [N, F]
        g_abs = c_i.abs() * h_mag
        a_i = alpha * (g_abs + _row_sum(alpha * g_abs, rowptr))                      # [N, F] ([N, 1] alpha broadcasts)
        t_gate = a_i.sum(1, keepdim=True) if gate_out == 1 else a_i
        bounds = {"nn.weight": k * t_nn.t() @ x.double().abs(), "nn.bias": k * t_nn.sum(0),
                  "gate_nn.weight": k * t_gate.t() @ x.double().abs(), "gate_nn.bias": k * t_gate.sum(0)}
    agg = agg.to(dev)
    batch = ids.to(dev)
    dm.register_batch(batch, rowptr.long().to(dev), B, max_nodes=n_max, min_nodes=0)
    for kw in ({"index": batch}, {"ptr": rowptr.long().to(dev)}, {"index": ids.to(dev), "dim_size": B}):
        agg.zero_grad()
        out = agg(x.to(dev), **kw)
        (out * coef.to(dev)).sum().backward()
        _hold(out.detach(), ref.detach(), out_bound, f"AttentionalAggregation out {sorted(kw)}")
        for name, p in agg.named_parameters():
            _hold(p.grad, dict(ref_mod.named_parameters())[name].grad, bounds[name], f"AttentionalAggregation {name} {sorted(kw)}")


# ---- bf16 / fp16 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_half_src_is_the_fp32_result_rounded_once(dev, dtype):
    import deepmetv2_amd as dm
    lengths = [0, 5, 17, 0, 1300, 2]
    n = len(lengths)
    ptr = sr.lengths_rowptr(lengths).long().to(dev)
    idx = torch.repeat_interleave(torch.arange(n), torch.tensor(lengths)).to(dev)
    src = _gauss(5, lengths=lengths).to(dev).to(dtype)
    for fn in (dm.scatter_mean, dm.scatter_softmax, dm.scatter_log_softmax, dm.scatter_logsumexp,
               lambda *a, **k: dm.scatter_min(*a, **k)[0]):
        got = fn(src, idx, dim=0, dim_size=n)
        assert got.dtype == dtype
        _same_bits(got, fn(src.float(), idx, dim=0, dim_size=n).to(dtype), "half")
    _same_bits(dm.softmax(src, ptr=ptr), dm.softmax(src.float(), ptr=ptr).to(dtype), "half softmax")
    _same_bits(dm.segment_csr(src, ptr, reduce="min"), dm.segment_csr(src.float(), ptr, reduce="min").to(dtype), "half csr")
