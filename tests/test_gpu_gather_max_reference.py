"""K3, out = P + max_j Q[nbr[i, j]]: every form of gather_max_launch (csrc/edgeconv.hip) and the counted / winner-id entries
against the plain CPU reference of tests/gather_max_reference.py, bit for bit (one exact maximum, one fp32 add: no tolerance).

One ragged batch is shared by all parameter sets.  Its event sizes sit on every edge of the kernels: the 32-row staging chunk,
the 256- and 512-row iteration strides of the half and the full image, 1024, the half image (2559 nodes + the -inf row fill
its 2560 rows, 2560 do not fit) and the full image (5119 / 5120), with empty events first, in the middle and last and B = 25
(the grid pads the events to a multiple of 8).  The tables are built in Python (random in-event ids plus the input classes
listed in gather_max_reference.py); no kNN build runs here.  Classes (a)-(e) are in test_*_exact, the non-finite contract
(f)-(h) in test_*_nonfinite."""
import os

import pytest
import torch

from gather_max_reference import gather_max_ref, make_inputs, winner_ids16

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 8, 31, 32, 33, 63, 64, 65, 129, 255, 256, 257, 0, 511, 512, 513, 1023, 1025, 2559, 2560, 5119, 5120, 0]
FITS = [i for i, s in enumerate(SIZES) if s <= 5119]         # "every event fits the image"
SMALL = [i for i, s in enumerate(SIZES) if s <= 2559]        # ... the half image
ALL = list(range(len(SIZES)))
KMAX = 40                                                    # counted tables: depths 0 .. 40

L2_H = (16, 32, 64, 128)                                     # the channel counts gather_max_kernel is built for

_cache = {}


def _l2_only_needs(H):
    """DMET_GATHER_MAX_FORM=l2-only sends every call to the L2 kernels, which are built for four channel counts."""
    from deepmetv2_amd import _native
    if _native.GATHER_MAX_FORM == "l2-only" and H not in L2_H:
        pytest.skip(f"DMET_GATHER_MAX_FORM=l2-only: H={H} is read by the LDS-resident kernels alone")


def _data(k, H, variant, counted):
    """The inputs and their reference for one (k, H, variant, counted), never modified.  Only the two sets that more than one
    test reads stay cached; every other set belongs to one parametrised case and is dropped with it."""
    key = (k, H, variant, counted)
    if key in _cache:
        return _cache[key]
    d = make_inputs(SIZES, k, H, variant, counted, seed=1000 * k + H)
    d["out"], d["arg"] = gather_max_ref(d["P"], d["Q"], d["nbr"], d["cnt"])
    d["variant"] = variant
    assert not bool(torch.isnan(d["out"]).any())             # torch.equal below is then a comparison of every value
    if key in ((16, 32, "finite", False), (KMAX, 32, "finite", True)):
        _cache[key] = d
    return d


class _Batch:
    """The events `which` of the shared batch as device tensors, the ids re-based; the reference rows go along."""

    def __init__(self, d, which, dev):
        ptr = d["ptr"]
        rows = torch.cat([torch.arange(int(ptr[b]), int(ptr[b + 1])) for b in which] + [torch.zeros(0, dtype=torch.int64)])
        sizes = torch.tensor([int(ptr[b + 1] - ptr[b]) for b in which])
        self.ptr_cpu = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)])
        lo = torch.repeat_interleave(self.ptr_cpu[:-1], sizes).view(-1, 1)
        local = d["local"][rows]
        self.nbr_cpu = torch.where(local >= 0, local + lo, local).to(torch.int32)
        self.N, self.H = rows.numel(), d["P"].shape[1]
        self.P, self.Q = d["P"][rows].to(dev), d["Q"][rows].to(dev)
        self.nbr, self.ptr = self.nbr_cpu.to(dev), self.ptr_cpu.to(dev)
        self.loc = local.to(torch.int16).to(dev)             # event-local uint16 ids, -1 -> 0xFFFF (ids < 32768 here)
        self.cnt = None if d["cnt"] is None else d["cnt"][rows].to(dev)
        self.local = local
        self.out, self.arg = d["out"][rows].to(dev), d["arg"][rows].to(dev)
        self._sliced = None
        # Rows on which gather_max_lds_kernel is unspecified (include/dmet.h): every candidate non-finite in the first channel
        # of a lane -- the class (g) rows of cases 1 and 3 (make_inputs: l % 16 == 13 in events of more than 13 nodes) -- when
        # the row's event lies in the kernel's LDS image.  n_row + 1 is the number of image rows the event needs.
        n_row = torch.repeat_interleave(sizes, sizes)
        l = torch.arange(self.N) - lo.view(-1)
        g = (l % 16 == 13) & (n_row > 13) if d.get("variant") in ("g1", "g3") else torch.zeros(self.N, dtype=torch.bool)
        self._g, self._need = g.to(dev), (n_row + 1).to(dev)

    def sliced(self):
        """P, Q as the slice-major [H/8, N, 8] tables of node_linear_split(..., sliced=True)"""
        if self._sliced is None:
            f = lambda t: t.view(self.N, self.H // 8, 8).permute(1, 0, 2).contiguous()
            self._sliced = f(self.P), f(self.Q)
        return self._sliced

    def check(self, got, what, image=None, part="all"):
        """image: rows of the LDS image of the launch (None: no LDS-resident kernel in it).  part "specified": every row but
        those the kernel leaves unspecified; "unspecified": those rows alone; "all": no distinction."""
        out, arg = got
        if part != "all":
            unspec = self._g & (self._need <= (image or 0))
            rows = unspec if part == "unspecified" else ~unspec
            ref_out, ref_arg = self.out[rows], self.arg[rows]
            assert torch.equal(out[rows], ref_out), f"{what}: out differs from the reference on the {part} rows"
            assert arg is None or torch.equal(arg[rows], ref_arg), f"{what}: arg differs from the reference on the {part} rows"
            return
        assert torch.equal(out, self.out), f"{what}: out differs from the reference in " \
            f"{int((out != self.out).any(1).sum())} rows, first {int((out != self.out).any(1).nonzero()[0])}"
        if arg is not None:
            assert torch.equal(arg, self.arg), f"{what}: arg differs from the reference in " \
                f"{int((arg != self.arg).any(1).sum())} rows, first {int((arg != self.arg).any(1).nonzero()[0])}"


LDS_FORMS = ("row-i32", "row-u16", "sliced-i32", "sliced-u16", "half", "mixed")


def _lds_forms(d, dev, monkeypatch, part="all", only=None):
    """Every LDS kNN form (or the one named by `only`), under both work mappings, with and without arg."""
    from deepmetv2_amd import _native
    k = d["nbr"].shape[1]
    fits, small, full = _Batch(d, FITS, dev), _Batch(d, SMALL, dev), _Batch(d, ALL, dev)
    slice_major = _native.GATHER_MAX_FORM != "l2-only"       # gather_max refuses slice-major tables under l2-only
    half_image = os.environ.get("DMET_GATHER_HALF_IMAGE") != "0"
    want = lambda form: only is None or only == form
    for balanced in ("0", "1"):
        monkeypatch.setenv("DMET_GATHER_BALANCED", balanced)
        for want_arg in (True, False):
            tag = f"k={k} H={fits.H} balanced={balanced} arg={want_arg}"
            for b, name in ((fits, "every event fits"), (full, "with the 5120-node event (in-kernel L2 path)")):
                for nl in (None, b.loc):
                    ids, sfx = ("int32 ids", "i32") if nl is None else ("uint16 ids", "u16")
                    if want("row-" + sfx):
                        b.check(_native.gather_max(b.P, b.Q, b.nbr, b.ptr, want_arg, lds=True, nbr_local=nl),
                                f"LDS row-major, {ids}, {name}, {tag}", 5120, part)
                    if slice_major and want("sliced-" + sfx):
                        Ps, Qs = b.sliced()
                        b.check(_native.gather_max(Ps, Qs, b.nbr, b.ptr, want_arg, lds=True, nbr_local=nl, sliced=True),
                                f"LDS slice-major, {ids}, {name}, {tag}", 5120, part)
            if slice_major and want("half"):
                for b, hint in ((small, 2559), (full, 500)):
                    Ps, Qs = b.sliced()
                    b.check(_native.gather_max(Ps, Qs, b.nbr, b.ptr, want_arg, lds=True, nbr_local=b.loc, sliced=True,
                                               max_nodes=hint), f"half image, max_nodes={hint}, {tag}",
                            2560 if half_image else 5120, part)
            # away from H = 32 and k in {8, 16, 32} the mixed entry is the L2 kernel alone
            mixed_lds = full.H == 32 and k in (8, 16, 32)
            for nl in (None, full.loc) if full.H in L2_H and want("mixed") else ():
                full.check(_native.gather_max(full.P, full.Q, full.nbr, full.ptr, want_arg, nbr_local=nl, mixed=True),
                           f"mixed, {'int32' if nl is None else 'uint16'} ids, {tag}", 5120 if mixed_lds else None, part)
    monkeypatch.delenv("DMET_GATHER_BALANCED")


def _l2_forms(d, dev):
    """The L2 kernels (generic by H, deep for H = 32 and k in {8, 16, 32}), with cnt when the data has one."""
    from deepmetv2_amd import _native
    b = _Batch(d, ALL, dev)
    for want_arg in (True, False):
        b.check(_native.gather_max(b.P, b.Q, b.nbr, b.ptr, want_arg, cnt=b.cnt, lds=False),
                f"L2, k={b.nbr.shape[1]} H={b.H} cnt={b.cnt is not None} arg={want_arg}")


def _rows16(b, stride):
    """The uint16 rows of radius(..., local=True): slots < cnt hold event-local ids (0xFFFF = none), the rest of the last
    started chunk of 8 holds 0xFFFF; what lies beyond is unwritten there -- here a valid id, which must not be read."""
    N, k = b.local.shape
    rows = torch.zeros(N, stride, dtype=torch.int64)
    rows[:, :k] = torch.where(b.local >= 0, b.local, torch.full_like(b.local, 0xFFFF))
    slot = torch.arange(stride).view(1, -1)
    c = b.cnt.cpu().long().view(-1, 1)
    rows = torch.where((slot >= c) & (slot < (c + 7) // 8 * 8), torch.full_like(rows, 0xFFFF), rows)
    return torch.where(rows >= 0x8000, rows - 0x10000, rows).to(torch.int16)


def _counted_forms(d, dev):
    """The counted LDS kernel (slots, winner ids out of the int32 table, winner ids out of uint16 rows) and the counted L2
    kernel; the 5120-node event takes the kernels' own L2 path."""
    from deepmetv2_amd import _native
    b = _Batch(d, ALL, dev)
    H, kmax = b.H, b.nbr.shape[1]
    argj_ref = winner_ids16(b.arg, b.nbr_cpu, b.ptr_cpu).to(dev)
    order = _native.table_order_by_count(b.cnt, b.ptr)
    rows16 = _rows16(b, (kmax + 7) // 8 * 8).to(dev)
    lds = _native.GATHER_MAX_FORM != "l2-only"
    for want_arg in (True, False):
        if H in L2_H:
            b.check(_native.gather_max(b.P, b.Q, b.nbr, b.ptr, want_arg, cnt=b.cnt, lds=False), f"counted L2, H={H} arg={want_arg}")
        for sliced in ((False, True) if lds else (False,)):
            P, Q = b.sliced() if sliced else (b.P, b.Q)
            tag = f"H={H} sliced={sliced} arg={want_arg}"
            b.check(_native.gather_max(P, Q, b.nbr, b.ptr, want_arg, cnt=b.cnt, lds=True, sliced=sliced), f"counted LDS, {tag}")
            for od in (order, None):
                tag_o = f"{tag} order={od is not None}"
                if want_arg:
                    out, argj = _native.gather_max_counted_j16(P, Q, b.nbr, b.cnt, od, b.ptr, sliced)
                    b.check((out, None), f"counted j16, {tag_o}")
                    assert torch.equal(argj.long() & 0xFFFF, argj_ref), f"counted j16, {tag_o}: winner ids"
                out, argj = _native.gather_max_local_j16(P, Q, rows16, b.cnt, od, b.ptr, kmax, sliced, want_arg=want_arg)
                b.check((out, None), f"local j16, {tag_o}")
                assert (argj is None) == (not want_arg)
                if want_arg:
                    assert torch.equal(argj.long() & 0xFFFF, argj_ref), f"local j16, {tag_o}: winner ids"


LDS_SHAPES = [(k, H) for k in (8, 16, 20, 32) for H in (8, 16, 24, 32, 64)]
L2_SHAPES = [(k, H) for H in L2_H for k in (1, 3, 5, 20, 33)] + [(k, 32) for k in (8, 16, 32)]
# the non-finite contract on one shape per code path: the register form (k <= 16) and the compare chain (k = 20 with its odd
# tail, k = 32), one, three and eight slices; the generic L2 kernel at each H and the deep one
LDS_NONFINITE = [(8, 32), (16, 32), (20, 24), (32, 32), (16, 8), (20, 64)]
L2_NONFINITE = [(5, 16), (16, 32), (20, 64), (3, 128), (33, 32)]
NONFINITE = ["fh", "g1", "g2", "g3"]


@pytest.mark.parametrize("k,H", LDS_SHAPES)
def test_lds_forms_exact(dev, monkeypatch, k, H):
    _l2_only_needs(H)
    _lds_forms(_data(k, H, "finite", False), dev, monkeypatch)


@pytest.mark.parametrize("counted", [False, True])
@pytest.mark.parametrize("k,H", L2_SHAPES)
def test_l2_forms_exact(dev, k, H, counted):
    _l2_forms(_data(k, H, "finite", counted), dev)


@pytest.mark.parametrize("H", [8, 32, 64])
def test_counted_forms_exact(dev, H):
    _l2_only_needs(H)
    _counted_forms(_data(KMAX, H, "finite", True), dev)


@pytest.mark.parametrize("variant", NONFINITE)
@pytest.mark.parametrize("k,H", LDS_NONFINITE)
def test_lds_forms_nonfinite(dev, monkeypatch, k, H, variant):
    """(f) -inf and NaN among finite candidates never win; (g) a row whose candidates are all -inf or NaN in some channels
    still HAS neighbours (R3 goes by the ids): out = P + (-inf) and arg = 255 there, the other channels as usual -- case 1:
    the channels c % 4 == 0 (the first channel of a lane), 2: the others, 3: all; (h) an empty row gives 0 whatever P holds."""
    _l2_only_needs(H)
    # every row of every form but the rows that gather_max_lds_kernel leaves unspecified (cases 1 and 3, events in its LDS
    # image): those are test_lds_image_rows_without_a_finite_candidate
    _lds_forms(_data(k, H, variant, False), dev, monkeypatch, part="specified")


UNSPECIFIED = ("gather_max_lds_kernel: the result is unspecified where every candidate of a channel is non-finite "
               "(include/dmet.h); for the events in its LDS image it decides R3 by the values of a lane's first channel")


@pytest.mark.xfail(strict=True, reason=UNSPECIFIED)
@pytest.mark.parametrize("form", LDS_FORMS)
@pytest.mark.parametrize("variant", ["g1", "g3"])
@pytest.mark.parametrize("k", [16, 32])
def test_lds_image_rows_without_a_finite_candidate(dev, monkeypatch, k, variant, form):
    """Class (g), cases 1 and 3, on the rows of events that the LDS kernel keeps in its image, one form at a time: the
    reference has -inf / 255 in the channels without a finite candidate and P + max in the others; the kernel, which takes a
    finite maximum in a lane's first channel for "has a neighbour", answers 0 / 255 in the lane's four channels (measured:
    case 1, 0 where the reference has -inf in one channel and P + max in three; case 3, 0 where it has -inf everywhere; case 2
    agrees).  Both ways tried of deciding it from the ids cost the hot kernel more than the parent's run-to-run spread --
    +1.9 us and +1.3 us on 33.7 us at 64 x 4500 nodes, k = 16, spread 0.5 us (profiles/NOTES.md, "K3 empty-row rule")."""
    from deepmetv2_amd import _native
    if _native.GATHER_MAX_FORM != "auto" or os.environ.get("DMET_GATHER_HALF_IMAGE") == "0":
        pytest.skip("a diagnostic switch is set: the expected failure belongs to the default route of each form")
    _lds_forms(_data(k, 32, variant, False), dev, monkeypatch, part="unspecified", only=form)


@pytest.mark.parametrize("variant", NONFINITE)
@pytest.mark.parametrize("k,H", L2_NONFINITE)
def test_l2_forms_nonfinite(dev, k, H, variant):
    _l2_forms(_data(k, H, variant, False), dev)
    _l2_forms(_data(k, H, variant, True), dev)


@pytest.mark.parametrize("variant", NONFINITE)
def test_counted_forms_nonfinite(dev, variant):
    _counted_forms(_data(KMAX, 32, variant, True), dev)


def test_routes_are_the_kernels_named(dev, monkeypatch):
    """What `_native` names as the kernel for the main routes of the calls above (the comparisons themselves hold under every
    switch).  The note does not tell the half image from the full one, nor the in-kernel L2 path: those are reached by
    construction -- a max_nodes hint of at most 2559 with uint16 ids, an event of 5120 nodes -- as in the neighbouring tests."""
    from deepmetv2_amd import _native
    if os.environ.get("DMET_GATHER_MAX_FORM") == "l2-only":
        pytest.skip("DMET_GATHER_MAX_FORM=l2-only: the LDS-resident forms named here are switched off")
    monkeypatch.setattr(_native, "GATHER_MAX_FORM", "auto")
    monkeypatch.delenv("DMET_GATHER_HALF_IMAGE", raising=False)
    b = _Batch(_data(16, 32, "finite", False), SMALL, dev)
    Ps, Qs = b.sliced()

    def ran(text, *args, **kw):
        _native.gather_max(*args, **kw)
        assert text in _native.last_gather_kernel, _native.last_gather_kernel

    ran("from L2", b.P, b.Q, b.nbr, b.ptr, True, lds=False)
    ran("row-major P/Q, int32 ids", b.P, b.Q, b.nbr, b.ptr, True, lds=True)
    ran("row-major P/Q, uint16 ids", b.P, b.Q, b.nbr, b.ptr, True, lds=True, nbr_local=b.loc)
    ran("slice-major P/Q, int32 ids", Ps, Qs, b.nbr, b.ptr, True, lds=True, sliced=True)
    ran("slice-major P/Q, uint16 event-local ids", Ps, Qs, b.nbr, b.ptr, True, lds=True, nbr_local=b.loc, sliced=True, max_nodes=2559)
    ran("chosen per event", b.P, b.Q, b.nbr, b.ptr, True, mixed=True)
    c = _Batch(_data(KMAX, 32, "finite", True), SMALL, dev)
    ran("counted rows (radius table; gathers from L2)", c.P, c.Q, c.nbr, c.ptr, True, cnt=c.cnt, lds=False)
    ran("counted rows (radius table; Q slice resident in LDS)", c.P, c.Q, c.nbr, c.ptr, True, cnt=c.cnt, lds=True)


@pytest.mark.parametrize("k", [8, 16, 32])
def test_fused_kernel_goes_by_the_ids(dev, k):
    """edgeconv_fused_lds_kernel forms its Q slice on the matrix cores, so its values are held to the reference at the
    tolerance of the whole-layer comparisons (1e-3 of the largest finite output); what is exact is the rule: a row whose
    candidates all overflow to -inf in the first channel of a lane has neighbours -- -inf and arg 255 there, the other
    channels finite with a winner -- and a row of holes gives 0 and 255."""
    from deepmetv2_amd import _native
    H = 32
    sizes = [0, 300, 5119, 5120, 77]
    g = torch.Generator().manual_seed(7 + k)
    N = sum(sizes)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(sizes).cumsum(0)])
    lo = torch.repeat_interleave(ptr[:-1], torch.tensor(sizes))
    l = torch.arange(N) - lo
    n = torch.repeat_interleave(torch.tensor(sizes), torch.tensor(sizes))
    x = torch.randn(N, H, generator=g)
    W = torch.randn(H, 2 * H, generator=g) / 8
    b = torch.randn(H, generator=g)
    big = l % 16 == 13                     # nodes whose Q overflows to -inf in the channels c % 4 == 0, and there alone
    x[:, 0] = torch.where(big, torch.full((), 3e38), x[:, 0])
    W[:, H] = torch.where(torch.arange(H) % 4 == 0, torch.full((), -8.0), torch.zeros(()))      # -8 * 3e38 overflows fp32
    W[:, 0] = W[:, H]                      # (W1 - W2)[:, 0] = 0: P stays finite in every row
    local = (torch.rand(N, k, generator=g) * n.view(-1, 1)).long().clamp(max=n.view(-1, 1) - 1)
    pool = (16 * (torch.rand(N, k, generator=g) * ((n.view(-1, 1) - 14) // 16 + 1)).long() + 13).clamp(max=n.view(-1, 1) - 1)
    case1 = (l % 16 == 3).view(-1, 1)      # rows that see the overflowing nodes alone, half of them behind a hole in slot 0
    local = torch.where(case1, pool, local)
    local = torch.where(case1 & (l % 32 == 3).view(-1, 1) & (torch.arange(k).view(1, -1) == 0), -1, local)
    # empty rows; those of the overflowing nodes among them (in the 5120-node event the kernel evaluates every edge directly,
    # W.[x_i || x_j - x_i], which for such an x_i is inf - inf where the split form is finite: not what is under test)
    local = torch.where(((l % 16 == 5) | big).view(-1, 1), -1, local)
    nbr = torch.where(local >= 0, local + lo.view(-1, 1), local).to(torch.int32)
    xd = x.double()
    Pr = (xd @ (W[:, :H] - W[:, H:]).double().T + b.double()).float()
    Qr = (xd @ W[:, H:].double().T).float()
    assert bool(torch.isfinite(Pr).all()) and bool(torch.isneginf(Qr[big][:, ::4]).all()) and bool(torch.isfinite(Qr[~big]).all())
    out_ref, arg_ref = gather_max_ref(Pr, Qr, nbr)
    rows = case1.view(-1)
    assert bool(torch.isneginf(out_ref[rows][:, ::4]).all()) and bool((arg_ref[rows][:, 1] != 255).all())
    tol = 1e-3 * float(out_ref[torch.isfinite(out_ref)].abs().max())
    for want_arg in (True, False):
        out, arg = _native.edgeconv_fused_lds(x.to(dev), W.to(dev), b.to(dev), nbr.to(dev), ptr.to(dev), want_arg)
        out = out.cpu()
        fin = torch.isfinite(out_ref)
        assert torch.equal(torch.isneginf(out), torch.isneginf(out_ref)) and torch.equal(torch.isfinite(out), fin)
        assert float((out[fin] - out_ref[fin]).abs().max()) <= tol
        assert bool((out[(nbr < 0).all(1)] == 0).all())
        if want_arg:
            arg = arg.cpu()
            assert torch.equal(arg == 255, arg_ref == 255)
            # a winner other than the reference's must be a candidate within the tolerance of the maximum
            won = torch.gather(Qr[nbr.long().clamp(min=0)], 1, arg.long().clamp(max=k - 1).unsqueeze(1)).squeeze(1)
            best = out_ref - Pr
            ok = (arg == arg_ref) | ((arg != 255) & ((won - best).abs() <= tol))
            assert bool(ok.all())
