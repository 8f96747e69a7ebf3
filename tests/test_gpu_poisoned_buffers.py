"""Every wrapper of deepmetv2_amd/_native.py that allocates uninitialised memory, one at a time, with that memory filled
before the kernels see it (tests/poisoned_alloc.py).

CASES maps a wrapper's name to its builders.  A builder takes the device and returns a Case: `call()` runs the wrapper on
inputs built OUTSIDE the poisoned block, `check(outs)` holds the result of the `ones` run to the reference that already
pins the operator (imported from the existing reference modules and tests; a copied bar cites its test), `masks` names
the regions include/dmet.h declares unwritten.  test_case runs call() under both patterns and requires every returned
tensor to be bitwise equal between the two runs outside the masks: the design is fixed summation order and integer
atomics only, so any difference is memory the call left as it was allocated, or read before writing it.

The table is importable without a GPU (tests/test_poisoned_alloc_host.py checks it against an ast walk of _native.py);
nothing touches a device before a builder runs.  To add a case for a new wrapper: write a builder, decorate it with
@case("<wrapper name>", "<label>"), return Case(call, check) -- the host test fails until every allocating wrapper has one."""
import copy
import functools
import os

import numpy as np
import pytest
import torch

import poisoned_alloc as pa

pytestmark = pytest.mark.gpu

CASES = {}

FEAT_RTOL, FEAT_ATOL = 1e-5, 1e-5          # tests/test_gpu_parity.py: fp32 features
BF16_RTOL = 2e-2                            # tests/test_gpu_parity.py test_edge_mlp2_bf16_mfma (b): rule R6, of the output scale
GRAD_RTOL, GRAD_ATOL = 1e-4, 1e-5           # tests/per_node_reference.py bar("grad"): atol times max(1, max|ref|)

# a run under tools/toggle_sweep.sh: assertions about WHICH writer ran (kNN counters, carried dense layers) say nothing there
SWITCHED = sorted(k for k in os.environ if k.startswith("DMET_") and k != "DMET_NONE")


class Case:
    def __init__(self, call, check, masks=None, env=None, attrs=None, skip_if=None, canon=None, declines=None):
        self.call = call            # () -> the wrapper's result
        self.check = check          # (list of CPU tensors of the `ones` run) -> None; asserts
        self.masks = masks or {}    # output position -> bool CPU tensor, True = compared
        self.env = env or {}        # environment switches of the case (read per call by the library)
        self.attrs = attrs or {}    # module attributes of _native of the case
        self.skip_if = skip_if      # () -> reason or None
        self.declines = declines    # why the entry is expected to decline (return None) in this case: asserted, not skipped
        self.canon = canon or {}    # output position -> (CPU tensor) -> the form compared, where the header leaves an order open


def case(name, label):
    def deco(fn):
        fn.label = label
        CASES.setdefault(name, []).append(fn)
        return fn
    return deco


def _ptr_of(sizes):
    return torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(list(sizes), dtype=torch.int64).cumsum(0)])


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _close(got, ref, rtol, atol, what):
    torch.testing.assert_close(got.detach().cpu().double(), ref.detach().cpu().double(), rtol=rtol, atol=atol,
                               msg=lambda m: f"{what}: {m}")


def _feat(got, ref, what):
    _close(got, ref, FEAT_RTOL, FEAT_ATOL, what)


def _grad(got, ref, what):
    top = float(ref.abs().max()) if ref.numel() else 0.0
    _close(got, ref, GRAD_RTOL, GRAD_ATOL * max(1.0, top), what)


def _grad4(got, ref, what):
    """rtol 1e-4, atol 1e-4 max|ref|: tests/test_gpu_edgeconv_linear_sum.py, test_gpu_gravnet.py and
    attention_reference.assert_grad_bar."""
    _close(got, ref, 1e-4, 1e-4 * max(float(ref.abs().max()) if ref.numel() else 0.0, 1e-6), what)


def _bf16(got, ref, what):
    scale = float(ref.abs().max()) if ref.numel() else 1.0
    _close(got, ref, BF16_RTOL, BF16_RTOL * scale, what)


def _mask_ok(keep, cnt, width, what):
    """The condition on a mask, from the reference alone: at least half of the elements stay compared, and the table has
    both full and short rows."""
    assert float(keep.float().mean()) >= 0.5, (what, "more than half of the output is masked", float(keep.float().mean()))
    assert bool((cnt == width).any()) and bool((cnt < width).any()), (what, "needs full and short rows")


def _skip_under(switch, value, why):
    return lambda: f"{switch}={value}: {why}" if os.environ.get(switch) == value else None


# =========================================================================================================================
# kNN: knn, knn_local, knn_local_dense, bn_knn_local_dense, knn_periodic, knn_xy
# =========================================================================================================================
KNN_SMALL = (1, 3, 0, 17, 129, 64, 2)      # n < k, an empty event; D = 5 is a padded D
KNN_KINDS = {
    # kind: (sizes, D, what writes the table on the default path)
    "small32": (KNN_SMALL, 32, "queries"),      # its duplicated rows leave 1 .. 8 uncertified queries: the per-query fallback
    "small5": (KNN_SMALL, 5, "exact"),          # 5 features: the exact kernel alone, whatever the switch
    "first": ((600, 37), 32, "filter"),          # both events below DMET_F2_MIN_NODES: first filter form + its tail re-rank
    "f2f1": ((900, 37), 32, "filter"),           # the 900-node event takes the second form, the 37-node one the first
    "d64": ((2300, 150), 64, "filter64"),        # 64-feature records; the 150-node event is the exact kernel's
    "identical": ((600, 37), 32, "tiles"),       # first form, nothing certifies: flagged-tile fallback, the exact kernel writes
    "identical2": ((900,), 32, "second"),        # second form, nothing certifies: its second sweep of the event writes
    "outliers": ((900,), 32, "second"),          # three rows of huge norm: a few queries take the second sweep
}


@functools.lru_cache(maxsize=None)
def _knn_data(kind, k):
    """(x, ptr, nbr_ref, dist_ref) on the CPU, shared and never modified."""
    from oracle import ref_ops
    from test_gpu_parity import _ragged
    sizes, D, _w = KNN_KINDS[kind]
    x, _batch, ptr = _ragged(list(sizes), D, seed=4000 + D + k, dup=kind.startswith("small"))
    if kind.startswith("identical"):
        x = torch.ones_like(x) * 0.37
    elif kind == "outliers":
        x[100] *= 300.0
        x[517] *= 300.0
        x[803] *= 300.0
    nbr, dist = ref_ops.knn_table(x, ptr, k)
    return x, ptr, nbr, dist


def _knn_writer(kind, st, exact):
    """The counters say that the intended writer ran (the way tests/test_gpu_parity.py reads them)."""
    if SWITCHED or not st:
        return
    if exact:
        assert st["flagged_queries"] == 0, st               # test_knn_oversized_event_goes_to_exact_kernel: nothing is flagged
        return
    writer = KNN_KINDS[kind][2]
    if writer == "exact":
        assert st["flagged_queries"] == 0 and st["second_attempt_queries"] == 0, st
    elif writer == "filter64":
        assert st["flagged_tiles"] < st["tiles"], st        # 64-feature records: the second form kept tiles of its own
    elif writer == "filter":
        assert st["flagged_tiles"] < st["tiles"], st        # the matrix-core path kept tiles of its own
    elif writer == "tiles":
        assert st["flagged_tiles"] > 0 and st["flagged_queries"] > 8 * st["flagged_tiles"], st
    elif writer == "queries":
        assert 1 <= st["flagged_queries"] <= 8, st           # at most kRequeryMax in any tile: the per-query fallback
    elif writer == "second":
        assert st["second_attempt_queries"] >= 1 and st["flagged_queries"] == 0, st


def _knn_case(entry, kind, k, exact):
    def build(dev):
        from deepmetv2_amd import _native
        from test_gpu_parity import _check_local_table
        x, ptr, nbr_ref, dist_ref = _knn_data(kind, k)
        xd, pd = x.to(dev), ptr.to(dev)
        seen = []

        def call():
            st = {}
            if entry == "knn":
                out = _native.knn(xd, pd, k, stats=st)
            else:
                out = _native.knn_local(xd, pd, k, stats=st)
            seen.append(dict(st))
            return out

        def check(outs):
            assert torch.equal(outs[0], nbr_ref) and torch.equal(outs[1], dist_ref), (entry, kind, k, seen)
            if entry == "knn_local":
                _check_local_table(outs[0], outs[2], ptr)
            assert seen[0] == seen[1], ("the counters of the build differ between the patterns", seen)
            _knn_writer(kind, seen[0], exact)
        return Case(call, check, env={"DMET_KNN_PATH": "exact"} if exact else None)
    build.label = f"{kind}-k{k}" + ("-exact" if exact else "")
    return build


KNN_LOCAL_SHAPES = [("small32", 16), ("small5", 3), ("first", 16), ("f2f1", 8), ("f2f1", 16), ("f2f1", 20), ("d64", 20),
                    ("identical", 16), ("identical2", 16), ("outliers", 16)]
CASES["knn_local"] = [_knn_case("knn_local", kind, k, exact) for kind, k in KNN_LOCAL_SHAPES for exact in (False, True)]
CASES["knn"] = [_knn_case("knn", kind, k, exact) for kind, k in KNN_LOCAL_SHAPES for exact in (False, True)]


def _dense_ref(x, W, b):
    """(P, Q) = (x (W1 - W2)^T + b, x W2^T) in float64."""
    x, W = x.detach().cpu().double(), W.detach().cpu().double()
    H = W.shape[1] // 2
    P = x @ (W[:, :H] - W[:, H:]).T
    if b is not None:
        P = P + b.detach().cpu().double()
    return P, x @ W[:, H:].T


def _rows_of(t, sliced):
    """A [H/8, N, 8] slice-major table back as [N, H]."""
    return t.permute(1, 0, 2).reshape(t.shape[1], -1) if sliced is True else t


def _check_pq(P, Q, x, W, b, sliced, what):
    Pr, Qr = _dense_ref(x, W, b)
    if sliced == "bf16":
        assert Q.dtype == torch.bfloat16
        _bf16(P, Pr, what + " P")
        _bf16(Q.float(), Qr, what + " Q")
    else:
        _feat(_rows_of(P, sliced), Pr, what + " P")
        _feat(_rows_of(Q, sliced), Qr, what + " Q")


def _dense_wb(seed):
    g = _gen(seed)
    return torch.randn(32, 64, generator=g) / 8, torch.randn(32, generator=g)


def _knn_dense_case(kind, k, sliced, exact=False):
    def build(dev):
        from deepmetv2_amd import _native
        from test_gpu_parity import _check_local_table
        x, ptr, nbr_ref, dist_ref = _knn_data(kind, k)
        W, b = _dense_wb(7)
        xd, pd, Wd, bd = x.to(dev), ptr.to(dev), W.to(dev), b.to(dev)
        seen = []

        def call():
            st = {}
            nbr, dist, loc, pq = _native.knn_local_dense(xd, pd, k, Wd, bd, sliced, stats=st)
            seen.append(dict(st))
            return nbr, dist, loc, (None if pq is None else pq[:2])

        def check(outs):
            assert torch.equal(outs[0], nbr_ref) and torch.equal(outs[1], dist_ref), (kind, k, seen)
            _check_local_table(outs[0], outs[2], ptr)
            assert seen[0] == seen[1], seen
            if len(outs) == 5:
                _check_pq(outs[3], outs[4], x, W, b, sliced, f"knn_local_dense {kind} sliced={sliced}")
            elif not SWITCHED and not exact and KNN_KINDS[kind][1] == 32:
                raise AssertionError("the default build at 32 features did not carry the dense layer")
            _knn_writer(kind, seen[0], exact)
        return Case(call, check, env={"DMET_KNN_PATH": "exact"} if exact else None)
    build.label = f"{kind}-k{k}-sliced{sliced}" + ("-exact" if exact else "")
    return build


CASES["knn_local_dense"] = ([_knn_dense_case("small32", 16, s) for s in (False, True, "bf16")]
                            + [_knn_dense_case("f2f1", 16, s) for s in (False, True, "bf16")]
                            + [_knn_dense_case("small5", 3, False), _knn_dense_case("f2f1", 16, True, exact=True),
                               _knn_dense_case("small32", 16, False, exact=True), _knn_dense_case("first", 16, True),
                               _knn_dense_case("identical", 16, True), _knn_dense_case("identical2", 16, "bf16"),
                               _knn_dense_case("outliers", 16, False)])


def _bn_operands(N, H, seed, with_res=True):
    """raw, residual, gamma, beta, mean, invstd (float32 CPU; the statistics are the batch's own, formed in float64)."""
    import per_node_reference as pn
    raw, res, _g = pn.bn_rows(N, H, seed)
    st = pn.bn_state(H, seed + 1)
    r64 = raw.double()
    mean = r64.mean(0)
    invstd = 1.0 / torch.sqrt(r64.var(0, unbiased=False) + 1e-5)
    return raw, (res if with_res else None), st["weight"], st["bias"], mean.float(), invstd.float()


def _bn_affine_ref(raw, res, gamma, beta, mean, invstd):
    y = (raw.double() - mean.double()) * (gamma.double() * invstd.double()) + beta.double()
    return y if res is None else y + res.double()


def _bn_knn_case(kind, k, dense, with_res, exact=False):
    def build(dev):
        import per_node_reference as pn
        from deepmetv2_amd import _native
        from oracle import ref_ops
        from test_gpu_parity import _check_local_table
        sizes, D, _w = KNN_KINDS[kind]
        ptr = _ptr_of(sizes)
        ops = _bn_operands(int(ptr[-1]), 32, 900 + k, with_res)
        if kind.startswith("identical"):
            # every row the same: raw == mean exactly, so y = beta in every row and nothing certifies (the fallback writers)
            raw = torch.full_like(ops[0], 0.37)
            ops = (raw, None, ops[2], ops[3], raw[0].clone(), ops[5])
        W, b = _dense_wb(9)
        dops = [None if t is None else t.to(dev) for t in ops]
        pd, Wd, bd = ptr.to(dev), W.to(dev), b.to(dev)

        def call():
            out = _native.bn_knn_local_dense(*dops, pd, k, dense=(Wd, bd, dense) if dense is not None else None)
            if out is None:
                return None
            y, nbr, dist, loc, pq = out
            return y, nbr, dist, loc, (None if pq is None else pq[:2])

        def check(outs):
            y = outs[0]
            pn.close(y, _bn_affine_ref(*ops), "bn_y", "bn_knn_local_dense y")
            nbr_ref, dist_ref = ref_ops.knn_table(y, ptr, k)         # the build is exact on the y it formed
            assert torch.equal(outs[1], nbr_ref) and torch.equal(outs[2], dist_ref), (kind, k)
            _check_local_table(outs[1], outs[3], ptr)
            if kind.startswith("identical"):
                assert bool((y == y[0]).all()), "the transform of identical rows gives identical rows"
            if len(outs) == 6:
                _check_pq(outs[4], outs[5], y, W, b, dense, f"bn_knn_local_dense {kind}")
            elif dense is not None and not SWITCHED:
                raise AssertionError("the default build did not carry the dense layer")
        if exact:       # deepmetv2_amd/_native.py: "None when nothing was launched (the build would not take the matrix-core path)"
            return Case(call, check, env={"DMET_KNN_PATH": "exact"},
                        declines="DMET_KNN_PATH=exact leaves the matrix-core path, whose prep launch carries the transform")
        return Case(call, check)
    build.label = f"{kind}-k{k}-dense{dense}-res{with_res}" + ("-exact" if exact else "")
    return build


CASES["bn_knn_local_dense"] = [_bn_knn_case("small32", 16, None, True), _bn_knn_case("small32", 16, True, False),
                               _bn_knn_case("f2f1", 16, False, True), _bn_knn_case("f2f1", 20, "bf16", False),
                               _bn_knn_case("identical", 16, True, False), _bn_knn_case("identical2", 16, None, False),
                               _bn_knn_case("first", 8, False, True), _bn_knn_case("f2f1", 16, True, True, exact=True)]


def _periodic_points(sizes, D, seed, side=2.0):
    rng = np.random.default_rng(seed)
    return ((rng.random((sum(sizes), D), dtype=np.float32) - np.float32(0.5)) * np.float32(side)).astype(np.float32)


def _knn_periodic_case(sizes, D, k, which, want_local):
    def build(dev):
        import knn_periodic_reference as kp
        from deepmetv2_amd import _native
        x = _periodic_points(sizes, D, 60 + D + k)
        ptr = _ptr_of(sizes)
        period = [0.0] * D
        period[which] = 2.0
        nbr_ref, dist_ref, loc_ref = kp.knn_table(x, ptr.numpy(), k, period)
        xd, pd = torch.from_numpy(x).to(dev), ptr.to(dev)

        def call():
            return _native.knn_periodic(xd, pd, k, period, want_local)

        def check(outs):
            assert torch.equal(outs[0], torch.from_numpy(nbr_ref)) and torch.equal(outs[1], torch.from_numpy(dist_ref))
            if want_local:
                assert torch.equal(outs[2].long() & 0xFFFF, torch.from_numpy(loc_ref.astype(np.int64)))
        return Case(call, check)
    build.label = f"{'-'.join(map(str, sizes))}-D{D}-k{k}-wrap{which}-local{want_local}"
    return build


CASES["knn_periodic"] = [_knn_periodic_case(KNN_SMALL, 5, 3, 4, True), _knn_periodic_case(KNN_SMALL, 2, 16, 1, True),
                         _knn_periodic_case((300, 37), 2, 20, 0, False)]

XY_X = (63, 0, 1, 65, 130)         # candidates per event (tests/test_gpu_radius_entries.py SIZES)
XY_Y = (5, 3, 0, 70, 64)           # queries per event (QSIZES): queries without candidates, candidates without queries


def _knn_xy_case(D, k, periodic):
    def build(dev):
        import knn_xy_reference as xy
        from deepmetv2_amd import _native
        x, y = _periodic_points(XY_X, D, 70 + D), _periodic_points(XY_Y, D, 80 + D)
        px, py = _ptr_of(XY_X), _ptr_of(XY_Y)
        period = None
        if periodic:
            period = [0.0] * D
            period[D - 1] = 2.0
        nbr_ref, dist_ref = xy.knn_table(x, px.numpy(), y, py.numpy(), k, period)
        ops = [torch.from_numpy(x).to(dev), px.to(dev), torch.from_numpy(y).to(dev), py.to(dev)]

        def call():
            return _native.knn_xy(*ops, k, period)

        def check(outs):
            assert torch.equal(outs[0], torch.from_numpy(nbr_ref)) and torch.equal(outs[1], torch.from_numpy(dist_ref))
        return Case(call, check)
    build.label = f"D{D}-k{k}-periodic{periodic}"
    return build


CASES["knn_xy"] = [_knn_xy_case(5, 3, False), _knn_xy_case(2, 16, True), _knn_xy_case(32, 16, False)]


# =========================================================================================================================
# radius: radius, radius_periodic, radius_xy -- the data of tests/test_gpu_radius_entries.py
# =========================================================================================================================
def _radius_masks(nbr_ref, cnt_ref, ptr, m, pad, outs_layout, what):
    """Masks of a radius result.  include/dmet.h: "fill == 0: they [slots >= cnt[i]] are left unwritten (the counted
    form)"; nbr16: "slots cnt[i] .. roundup8(cnt[i]) - 1 hold 0xFFFF, the rest of the row is unwritten"."""
    from test_gpu_radius_periodic import _expected_rows16
    masks = {}
    cnt = torch.from_numpy(cnt_ref)
    for pos, name in enumerate(outs_layout):
        if name == "nbr" and not pad:
            keep = torch.arange(m).view(1, -1) < cnt.view(-1, 1)
            _mask_ok(keep, cnt, m, what + " nbr")
            masks[pos] = keep
        if name == "rows16":
            stride = (m + 7) // 8 * 8
            _loc, written = _expected_rows16(torch.from_numpy(nbr_ref), cnt, ptr, stride)
            _mask_ok(written, cnt, m, what + " rows16")
            masks[pos] = written
    return masks


def _radius_check(outs, layout, nbr_ref, cnt_ref, ptr, pad, what):
    from test_gpu_radius_periodic import _expected_rows16
    want_nbr, want_cnt = torch.from_numpy(nbr_ref), torch.from_numpy(cnt_ref)
    got = dict(zip(layout, outs))
    assert torch.equal(got["cnt"], want_cnt), what
    if "nbr" in got:
        keep = torch.arange(want_nbr.shape[1]).view(1, -1) < want_cnt.view(-1, 1)
        assert torch.equal(got["nbr"][keep], want_nbr[keep]), what
        if pad:
            assert torch.equal(got["nbr"], want_nbr), what
    if "rows16" in got:
        loc, written = _expected_rows16(want_nbr, want_cnt, ptr, got["rows16"].shape[1])
        assert torch.equal(got["rows16"][written], loc[written]), what


def _radius_case(D, m, skip_self, pad, local, int32_rows, kind, form):
    def build(dev):
        import radius_periodic_reference as rp
        import test_gpu_radius_entries as re_
        from deepmetv2_amd import _native
        N = sum(re_.SIZES)
        x = re_._points(D, N, 100 + D)
        ptr = _ptr_of(re_.SIZES)
        period = None if kind == "none" else re_._period(D, kind)
        r = re_.R            # caps 3 and 9 bind in the 130-node event, other rows stay short
        form_ = "sweep" if _native.RADIUS_FORM == "sweep" else form        # DMET_RADIUS=sweep keeps the all-pairs form
        nbr_ref, cnt_ref = rp.radius_table(x, ptr.numpy(), r, m, period, skip_self=skip_self)
        assert int((cnt_ref == 0).sum()) >= (1 if skip_self else 0)          # a node without a neighbour (the one-node event)
        windowed = form_ != "sweep" and (period is None or period[0] == 0.0)
        layout = ([] if (local and windowed and not int32_rows and not pad) else ["nbr"]) + ["cnt"] + (
            ["rows16"] if local and windowed else [])
        what = f"radius D={D} m={m} skip={skip_self} pad={pad} local={local} i32={int32_rows} {kind} {form}"
        masks = _radius_masks(nbr_ref, cnt_ref, ptr, m, pad, layout, what)
        xd, pd = torch.from_numpy(x).to(dev), ptr.to(dev)

        def call():
            if kind == "none":
                return _native.radius(xd, pd, r, m, skip_self, pad, local, int32_rows)
            return _native.radius_periodic(xd, pd, r, m, period, skip_self, pad, local, int32_rows)

        def check(outs):
            assert len(outs) == len(layout), (what, len(outs), layout)
            _radius_check(outs, layout, nbr_ref, cnt_ref, ptr, pad, what)
        return Case(call, check, masks, attrs={"RADIUS_FORM": form_})
    build.label = f"D{D}-m{m}-skip{int(skip_self)}-pad{int(pad)}-local{int(local)}-i32{int(int32_rows)}-{kind}-{form}"
    return build


CASES["radius"] = [_radius_case(2, m, skip, pad, local, i32, "none", form)
                   for m, skip, pad, local, i32, form in [
                       (3, False, True, False, True, "windowed"), (3, True, False, False, True, "windowed"),
                       (9, False, False, True, True, "windowed"), (9, True, True, True, True, "windowed"),
                       (9, False, False, True, False, "windowed"), (3, False, False, True, False, "windowed"),
                       (9, True, True, False, True, "sweep"), (9, False, False, False, True, "sweep"),
                       (3, True, False, True, True, "sweep")]] + [
                   _radius_case(5, 9, False, False, True, True, "none", "windowed"),
                   _radius_case(8, 3, True, True, True, True, "none", "windowed")]
CASES["radius_periodic"] = [_radius_case(2, m, skip, pad, local, True, kind, "windowed")
                            for m, skip, pad, local, kind in [
                                (9, False, False, True, "last"), (3, True, True, True, "last"), (9, True, False, False, "first"),
                                (3, False, True, False, "first")]] + [
                            _radius_case(3, 9, False, False, False, True, "last", "sweep")]


def _radius_xy_case(D, m, pad, periodic):
    def build(dev):
        import knn_xy_reference as xy
        import test_gpu_radius_entries as re_
        from deepmetv2_amd import _native
        x, y = re_._points(D, sum(re_.SIZES), 100 + D), re_._points(D, sum(re_.QSIZES), 200 + D)
        px, py = _ptr_of(re_.SIZES), _ptr_of(re_.QSIZES)
        period = re_._period(D, "last") if periodic else None
        nbr_ref, cnt_ref = xy.radius_table(x, px.numpy(), y, py.numpy(), re_.R, m, period)
        assert bool((cnt_ref == 0).any())
        what = f"radius_xy D={D} m={m} pad={pad} periodic={periodic}"
        masks = _radius_masks(nbr_ref, cnt_ref, py, m, pad, ["nbr", "cnt"], what)
        ops = [torch.from_numpy(x).to(dev), px.to(dev), torch.from_numpy(y).to(dev), py.to(dev)]

        def call():
            return _native.radius_xy(*ops, re_.R, m, period, pad)

        def check(outs):
            _radius_check(outs, ["nbr", "cnt"], nbr_ref, cnt_ref, py, pad, what)
        return Case(call, check, masks)
    build.label = f"D{D}-m{m}-pad{int(pad)}-periodic{int(periodic)}"
    return build


CASES["radius_xy"] = [_radius_xy_case(2, 3, False, False), _radius_xy_case(2, 9, True, True),
                      _radius_xy_case(5, 3, False, True), _radius_xy_case(8, 9, True, False)]


# =========================================================================================================================
# gather-max and gather-sum forms, their backwards, the fused EdgeConv, table -> edge list, reverse index
# =========================================================================================================================
GM_SIZES = (1, 3, 0, 17, 129, 33, 257)     # short events, an empty one, N = 33 and 257: the last tile of each is partial


GM_UNUSED = (3, 300)        # two nodes (of the 3- and the 257-node event) that are taken out of every row: nobody's neighbour


@functools.lru_cache(maxsize=None)
def _gm_data(k, H, counted):
    """tests/gather_max_reference.py inputs (rows with -1 holes, empty rows, duplicated ids; counted: cnt in 0 .. k with
    zero-count rows) and their exact reference.  The nodes GM_UNUSED are removed from every row (their slots become
    holes): sources no target points to, for the backward kernels."""
    from gather_max_reference import gather_max_ref, make_inputs
    d = make_inputs(list(GM_SIZES), k, H, "finite", counted, seed=77 + k + H)
    gone = torch.isin(d["nbr"].long(), torch.tensor(GM_UNUSED))
    d["nbr"] = d["nbr"].masked_fill(gone, -1)
    d["local"] = d["local"].masked_fill(gone, -1)
    d["out"], d["arg"] = gather_max_ref(d["P"], d["Q"], d["nbr"], d["cnt"])
    d["variant"] = "finite"
    assert bool((d["arg"] == 255).all(1).any()) and not bool(torch.isnan(d["out"]).any())
    return d


def _gm_batch(k, H, counted, dev):
    from test_gpu_gather_max_reference import _Batch
    d = _gm_data(k, H, counted)
    return d, _Batch(d, list(range(len(GM_SIZES))), dev)


_NEEDS_LDS = _skip_under("DMET_GATHER_MAX_FORM", "l2-only", "gather_max refuses slice-major tables: they are read by the "
                         "LDS-resident kernels alone")
GM_FORMS = {
    # form: (counted, keyword arguments by name of the batch attribute)
    "l2": (False, dict(lds=False)),
    "row-i32": (False, dict(lds=True)),
    "row-u16": (False, dict(lds=True, nbr_local="loc")),
    "sliced-i32": (False, dict(lds=True, sliced=True)),
    "sliced-u16": (False, dict(lds=True, sliced=True, nbr_local="loc")),
    "half": (False, dict(lds=True, sliced=True, nbr_local="loc", max_nodes=257)),
    "mixed": (False, dict(mixed=True, nbr_local="loc")),
    "counted-l2": (True, dict(cnt="cnt", lds=False)),
    "counted-lds": (True, dict(cnt="cnt", lds=True)),
    "counted-lds-sliced": (True, dict(cnt="cnt", lds=True, sliced=True)),
}


def _gather_max_case(form, k, H, want_arg=True):
    counted, kw = GM_FORMS[form]

    def build(dev):
        from deepmetv2_amd import _native
        d, b = _gm_batch(k, H, counted, dev)
        kwargs = {n: (getattr(b, v) if isinstance(v, str) else v) for n, v in kw.items()}
        P, Q = b.sliced() if kw.get("sliced") else (b.P, b.Q)

        def call():
            return _native.gather_max(P, Q, b.nbr, b.ptr, want_arg, **kwargs)

        def check(outs):
            assert torch.equal(outs[0], d["out"]), f"gather_max {form}: out differs from the reference"
            if want_arg:
                assert torch.equal(outs[1], d["arg"]), f"gather_max {form}: arg differs from the reference"
        skip = _NEEDS_LDS if kw.get("sliced") else (_skip_under(
            "DMET_GATHER_MAX_FORM", "l2-only", f"H={H} is read by the LDS-resident kernels alone") if H not in (16, 32, 64, 128)
            else None)
        return Case(call, check, skip_if=skip)
    build.label = f"{form}-k{k}-H{H}-arg{int(want_arg)}"
    return build


CASES["gather_max"] = ([_gather_max_case(f, 16, 32) for f in GM_FORMS] + [_gather_max_case("row-u16", 20, 32),
                       _gather_max_case("sliced-u16", 8, 64), _gather_max_case("l2", 5, 16),
                       _gather_max_case("row-i32", 16, 32, want_arg=False), _gather_max_case("counted-lds", 20, 24)])


def _counted_j16_case(local, sliced, ordered, want_arg=True):
    def build(dev):
        from deepmetv2_amd import _native
        from gather_max_reference import winner_ids16
        from test_gpu_gather_max_reference import _rows16
        k, H = 20, 32
        d, b = _gm_batch(k, H, True, dev)
        argj_ref = winner_ids16(d["arg"], b.nbr_cpu, b.ptr_cpu)
        order = _native.table_order_by_count(b.cnt, b.ptr) if ordered else None
        rows16 = _rows16(b, (k + 7) // 8 * 8).to(dev)
        P, Q = b.sliced() if sliced else (b.P, b.Q)

        def call():
            if local:
                return _native.gather_max_local_j16(P, Q, rows16, b.cnt, order, b.ptr, k, sliced, want_arg=want_arg)
            return _native.gather_max_counted_j16(P, Q, b.nbr, b.cnt, order, b.ptr, sliced)

        def check(outs):
            assert torch.equal(outs[0], d["out"])
            if want_arg:
                assert torch.equal(outs[1].long() & 0xFFFF, argj_ref)
        return Case(call, check, skip_if=_NEEDS_LDS if sliced else None)
    build.label = f"sliced{int(sliced)}-order{int(ordered)}-arg{int(want_arg)}"
    return build


CASES["gather_max_counted_j16"] = [_counted_j16_case(False, s, o) for s, o in ((False, True), (True, True), (True, False))]
CASES["gather_max_local_j16"] = [_counted_j16_case(True, s, o, a) for s, o, a in
                                 ((False, True, True), (True, True, True), (True, False, True), (True, True, False))]


@case("table_order_by_count", "counted-k20")
def _order_by_count(dev):
    from deepmetv2_amd import _native
    d, b = _gm_batch(20, 32, True, dev)

    def check(outs):
        # include/dmet.h: per event, the local node indices grouped by slot count; tests/fake_native.py: deepest rows first,
        # any order inside a group -- so: a permutation of every event whose counts do not increase
        order, cnt, ptr = outs[0].long(), d["cnt"].long(), d["ptr"]
        for e in range(len(GM_SIZES)):
            lo, hi = int(ptr[e]), int(ptr[e + 1])
            assert sorted(order[lo:hi].tolist()) == list(range(hi - lo))
            c = cnt[lo:hi][order[lo:hi]]
            assert bool((c[1:] <= c[:-1]).all())

    def canon(order):
        # include/dmet.h, dmet_table_order_by_count: "The order inside a group of equal count is unspecified and may differ
        # between runs" (LDS counting sort with integer atomics): compared are the counts along the order and each group's
        # members, ascending
        cnt, ptr, o = d["cnt"].long(), d["ptr"], order.long()
        parts = []
        for e in range(len(GM_SIZES)):
            lo, hi = int(ptr[e]), int(ptr[e + 1])
            oe = o[lo:hi].clamp(0, max(hi - lo - 1, 0))
            c = cnt[lo:hi][oe]
            parts += [c, oe[np.lexsort((oe.numpy(), -c.numpy()))]]
        return torch.cat(parts)
    return Case(lambda: _native.table_order_by_count(b.cnt, b.ptr), check, canon={0: canon})


def _gout(N, H, seed):
    return torch.randn(N, H, generator=_gen(seed))


def _gather_bwd_case(entry, sliced, hint):
    def build(dev):
        import fake_native
        from deepmetv2_amd import _native
        from gather_max_reference import winner_ids16
        k, H = 16, 32
        d, b = _gm_batch(k, H, False, dev)
        N = d["P"].shape[0]
        g = _gout(N, H, 5)
        gd, arg = g.to(dev), d["arg"].to(dev)
        ref = fake_native.gather_max_bwd_lds(g.double(), d["arg"], b.nbr_cpu, b.ptr_cpu)      # a source nobody picks: row 0
        assert bool((ref == 0).all(1).any())
        if entry == "gather_max_bwd":
            rev_ptr, rev_pos = _native.reverse_index(b.nbr.view(-1), N)
            call = lambda: _native.gather_max_bwd(gd, arg, rev_ptr, rev_pos, k)
        elif entry == "gather_max_bwd_lds":
            call = lambda: _native.gather_max_bwd_lds(gd, arg, b.nbr, b.ptr, nbr_local=b.loc, max_nodes=hint, sliced=sliced)
        else:
            j = winner_ids16(d["arg"], b.nbr_cpu, b.ptr_cpu)
            argj = torch.where(j >= 0x8000, j - 0x10000, j).to(torch.int16).to(dev)
            call = lambda: _native.gather_max_bwd_j16(gd, argj, b.ptr, max_nodes=hint, sliced=sliced)

        def check(outs):
            gq = outs[0].permute(1, 0, 2).reshape(N, H) if sliced else outs[0]
            # each gQ element adds at most k fp32 terms in a fixed order: the float64 sum at the fp32 feature bar
            _feat(gq, ref, entry)
            assert bool((gq[(ref == 0).all(1)] == 0).all()), "the gradient row of a source nobody picks must be 0"
        return Case(call, check)
    build.label = f"sliced{int(sliced)}-hint{hint}"
    return build


CASES["gather_max_bwd"] = [_gather_bwd_case("gather_max_bwd", False, None)]
CASES["gather_max_bwd_lds"] = [_gather_bwd_case("gather_max_bwd_lds", s, h) for s, h in ((False, None), (True, 257), (False, 129))]
CASES["gather_max_bwd_j16"] = [_gather_bwd_case("gather_max_bwd_j16", s, h) for s, h in ((False, None), (True, 257), (False, 129))]


def _x32(N, seed, H=32):
    return torch.randn(N, H, generator=_gen(seed))


def _nls_case(entry, N, sliced=False, with_bias=True, Hin=32, Hout=32):
    def build(dev):
        from deepmetv2_amd import _native
        g = _gen(10 + N)
        x = torch.randn(N, Hin, generator=g)
        W = torch.randn(Hout, 2 * Hin, generator=g) / 8
        b = torch.randn(Hout, generator=g) if with_bias else None
        xd, Wd, bd = x.to(dev), W.to(dev), None if b is None else b.to(dev)
        if entry == "node_linear_split":
            return Case(lambda: _native.node_linear_split(xd, Wd, bd, sliced),
                        lambda outs: _check_pq(outs[0], outs[1], x, W, b, sliced, entry))
        return Case(lambda: _native.node_linear_split_bf16(xd, Wd, bd),
                    lambda outs: _check_pq(outs[0], outs[1], x, W, b, "bf16", entry))
    build.label = f"N{N}-sliced{int(bool(sliced))}-bias{int(with_bias)}-{Hin}to{Hout}"
    return build


CASES["node_linear_split"] = [_nls_case("node_linear_split", N, s) for N in (1, 33, 257) for s in (False, True)] + [
    _nls_case("node_linear_split", 129, False, False, 64, 64)]
CASES["node_linear_split_bf16"] = [_nls_case("node_linear_split_bf16", N) for N in (1, 33, 257)]


def _bn_nls_case(N, sliced, with_res):
    def build(dev):
        import per_node_reference as pn
        from deepmetv2_amd import _native
        ops = _bn_operands(N, 32, 300 + N, with_res)
        W, b = _dense_wb(11)
        dops = [None if t is None else t.to(dev) for t in ops]
        Wd, bd = W.to(dev), b.to(dev)

        def check(outs):
            pn.close(outs[0], _bn_affine_ref(*ops), "bn_y", "bn_node_linear_split y")
            _check_pq(outs[1], outs[2], outs[0], W, b, sliced, "bn_node_linear_split")
        return Case(lambda: _native.bn_node_linear_split(*dops, Wd, bd, sliced), check)
    build.label = f"N{N}-sliced{int(sliced)}-res{int(with_res)}"
    return build


CASES["bn_node_linear_split"] = [_bn_nls_case(N, s, r) for N, s, r in ((3, False, True), (33, True, False), (257, True, True))]


@case("gather_max_bf16q", "k16-H32")
def _gather_max_bf16q(dev):
    from deepmetv2_amd import _native
    from gather_max_reference import gather_max_ref
    d, b = _gm_batch(16, 32, False, dev)
    Qh = d["Q"].to(torch.bfloat16)
    out_ref, arg_ref = gather_max_ref(d["P"], Qh.float(), d["nbr"])       # one exact maximum of bf16 values, one fp32 add
    Qd = Qh.to(dev)

    def check(outs):
        assert torch.equal(outs[0], out_ref) and torch.equal(outs[1], arg_ref)
    return Case(lambda: _native.gather_max_bf16q(b.P, Qd, b.nbr, True), check)


def _fused_lds_case(k, want_arg):
    def build(dev):
        from deepmetv2_amd import _native
        from gather_max_reference import gather_max_ref
        d, b = _gm_batch(k, 32, False, dev)
        N = d["P"].shape[0]
        x = _x32(N, 21)
        W, bias = _dense_wb(13)
        xd, Wd, bd = x.to(dev), W.to(dev), bias.to(dev)
        Pr, Qr = _dense_ref(x, W, bias)
        ref, _arg = gather_max_ref(Pr.float(), Qr.float(), d["nbr"])
        any_nbr = (d["nbr"] >= 0).any(1)

        def check(outs):
            # tests/test_gpu_gather_max_reference.py test_fused_kernel_goes_by_the_ids: the kernel forms its Q slice on the
            # matrix cores, so values are held to the fp32 feature bar; the rows without a neighbour are exact zeros
            _feat(outs[0], ref, "edgeconv_fused_lds")
            assert bool((outs[0][~any_nbr] == 0).all())
            if want_arg:
                assert bool((outs[1][~any_nbr] == 255).all()) and bool((outs[1][any_nbr] < k).all())
        return Case(lambda: _native.edgeconv_fused_lds(xd, Wd, bd, b.nbr, b.ptr, want_arg), check)
    build.label = f"k{k}-arg{int(want_arg)}"
    return build


CASES["edgeconv_fused_lds"] = [_fused_lds_case(16, True), _fused_lds_case(8, False)]


def _linear_bwd_case(N, arg_kind, gq_sliced, with_add, want_bias=True):
    def build(dev):
        import fake_native
        from deepmetv2_amd import _native
        g = _gen(30 + N)
        x, g_out, gQ = (torch.randn(N, 32, generator=g) for _ in range(3))
        W = torch.randn(32, 64, generator=g) / 8
        g_add = torch.randn(N, 32, generator=g) if with_add else None
        arg = None
        if arg_kind == "u8":
            arg = torch.randint(0, 16, (N, 32), generator=g).to(torch.uint8)
            arg[::3] = 255
        elif arg_kind == "j16":
            arg = torch.randint(0, max(N, 1), (N, 32), generator=g).to(torch.int16)
            arg[::3] = -1
        gq_in = gQ.view(N, 8, 4).permute(1, 0, 2).contiguous() if gq_sliced else gQ
        ref = fake_native.edgeconv_linear_bwd(x.double(), W.double(), g_out.double(), arg, gQ.double(), want_bias,
                                              None if g_add is None else g_add.double())
        ops = [x.to(dev), W.to(dev), g_out.to(dev), None if arg is None else arg.to(dev), gq_in.to(dev)]
        gad = None if g_add is None else g_add.to(dev)

        def check(outs):
            for got, want, name in zip(outs, [r for r in ref if r is not None], ("gx", "gW", "gb")):
                _grad(got, want, f"edgeconv_linear_bwd {name}")
        return Case(lambda: _native.edgeconv_linear_bwd(*ops, want_bias=want_bias, g_add=gad, gq_sliced=gq_sliced), check)
    build.label = f"N{N}-{arg_kind}-sliced{int(gq_sliced)}-add{int(with_add)}-bias{int(want_bias)}"
    return build


CASES["edgeconv_linear_bwd"] = [_linear_bwd_case(33, "u8", False, False), _linear_bwd_case(257, "u8", True, True),
                                _linear_bwd_case(257, "j16", False, True), _linear_bwd_case(129, "j16", True, False, False),
                                _linear_bwd_case(1, "none", False, False)]


def _sum_tables(dev, counted):
    """(d, b, nbr as the wrapper reads it, rowptr / src of the same graph on the CPU)."""
    d, b = _gm_batch(20 if counted else 16, 32, counted, dev)
    d = dict(d)
    d["Q"] = torch.randn(d["Q"].shape, generator=_gen(12))       # the sums take finite values (the max tables hold +inf)
    b.Q = d["Q"].to(dev)
    nbr = b.nbr_cpu.clone()
    k = nbr.shape[1]
    if counted:
        nbr = torch.where(torch.arange(k).view(1, -1) < d["cnt"].view(-1, 1).long(), nbr, torch.full_like(nbr, -1))
    return d, b, nbr


def _gather_sum_ref(P, Q, nbr, mean):
    P, Q = P.double(), Q.double()
    valid = nbr >= 0
    deg = valid.sum(1)
    s = (Q[nbr.long().clamp(min=0)] * valid.unsqueeze(-1)).sum(1)
    has = (deg > 0).view(-1, 1)
    out = torch.where(has, P + s / deg.clamp(min=1).view(-1, 1), torch.zeros_like(P)) if mean else \
        torch.where(has, deg.view(-1, 1) * P + s, torch.zeros_like(P))
    return out, deg.to(torch.int32)


def _gather_sum_case(form, counted, mean):
    def build(dev):
        from deepmetv2_amd import _native
        d, b, nbr = _sum_tables(dev, counted)
        out_ref, deg_ref = _gather_sum_ref(d["P"], d["Q"], nbr, mean)
        assert bool((deg_ref == 0).any())
        valid_ = nbr >= 0
        msg = (d["P"].double().unsqueeze(1) + d["Q"].double()[nbr.long().clamp(min=0)]).abs().amax(-1)
        bar = (msg * valid_).sum(1)
        if form == "table":
            call = lambda: _native.gather_sum_table(b.P, b.Q, b.nbr, b.cnt, mean)
        else:
            valid = nbr >= 0
            rowptr = torch.cat([torch.zeros(1, dtype=torch.int32), valid.sum(1).cumsum(0).to(torch.int32)]).to(dev)
            src = nbr[valid].contiguous().to(dev)
            call = lambda: _native.gather_sum_csr(b.P, b.Q, rowptr, src, mean)

        def check(outs):
            # tests/test_gpu_edgeconv_linear_sum.py _check: per row |err| <= 1e-5 sum_e |message|_inf + 1e-6
            err = (outs[0].double() - out_ref).abs().amax(1)
            lim = 1e-5 * bar + 1e-6
            assert bool((err <= lim).all()), (f"gather_sum_{form}", float((err - lim).max()))
            assert torch.equal(outs[1], deg_ref)
        return Case(call, check)
    build.label = f"counted{int(counted)}-mean{int(mean)}"
    return build


CASES["gather_sum_table"] = [_gather_sum_case("table", c, m) for c, m in ((False, False), (True, True), (True, False))]
CASES["gather_sum_csr"] = [_gather_sum_case("csr", c, m) for c, m in ((False, True), (True, False))]


def _gather_sum_bwd_case(form, mean):
    def build(dev):
        from deepmetv2_amd import _native
        d, b, nbr = _sum_tables(dev, False)
        N, k = nbr.shape
        g = _gout(N, 32, 8)
        valid = nbr >= 0
        deg = valid.sum(1)
        g64 = g.double()
        has = (deg > 0).view(-1, 1)
        gP = torch.where(has, g64 if mean else deg.view(-1, 1) * g64, torch.zeros_like(g64))
        s = g64 / deg.clamp(min=1).view(-1, 1) if mean else g64
        i, t = valid.nonzero(as_tuple=True)
        gQ = torch.zeros_like(g64).index_add_(0, nbr[i, t].long(), s[i])
        assert bool((gQ == 0).all(1).any())
        gd, degd = g.to(dev), deg.to(torch.int32).to(dev)
        if form == "table":
            rev_ptr, rev_idx = _native.reverse_index(b.nbr.view(-1), N)
            call = lambda: _native.gather_sum_bwd(gd, degd, rev_ptr, rev_idx, None, k, mean)
        else:
            src, tgt = nbr[valid].contiguous().to(dev), i.to(torch.int32).to(dev)
            rev_ptr, rev_idx = _native.reverse_index(src, N)
            call = lambda: _native.gather_sum_bwd(gd, degd, rev_ptr, rev_idx, tgt, 0, mean)

        def check(outs):
            _grad4(outs[0], gP, "gather_sum_bwd gP")
            _grad4(outs[1], gQ, "gather_sum_bwd gQ")
            assert bool((outs[1][(gQ == 0).all(1)] == 0).all()) and bool((outs[0][deg == 0] == 0).all())
        return Case(call, check)
    build.label = f"{form}-mean{int(mean)}"
    return build


CASES["gather_sum_bwd"] = [_gather_sum_bwd_case(f, m) for f, m in (("table", False), ("table", True), ("csr", True))]


def _reverse_index_case(kind):
    def build(dev):
        import fake_native
        from deepmetv2_amd import _native
        if kind == "table":            # a kNN table with -1 slots: keys outside [0, num_keys) sort last and are not indexed
            d, b = _gm_batch(16, 32, False, dev)
            keys, num = b.nbr_cpu.reshape(-1).contiguous(), d["P"].shape[0]
        elif kind == "dense":
            keys, num = torch.randint(0, 40, (1000,), generator=_gen(3)).to(torch.int32), 64      # keys 40 .. 63 never occur
        else:
            keys, num = torch.zeros(0, dtype=torch.int32), 5
        ptr_ref, pos_ref = fake_native.reverse_index(keys, num)
        M, n_idx = keys.numel(), int(ptr_ref[-1])
        kd = keys.to(dev)
        # every position 0 .. M-1 is sorted, the unindexed ones last: all of rev_pos[M] is written; M == 0: the wrapper's one zero element

        def check(outs):
            assert torch.equal(outs[0], ptr_ref) and outs[1].numel() == max(M, 1)
            assert M or int(outs[1][0]) == 0
            assert torch.equal(outs[1][:n_idx], pos_ref[:n_idx])
            if kind == "table":        # the -1 slots behind the indexed positions, in position order (a stable sort)
                assert torch.equal(outs[1], pos_ref)
        return Case(lambda: _native.reverse_index(kd, num), check)
    build.label = kind
    return build


CASES["reverse_index"] = [_reverse_index_case(k) for k in ("table", "dense", "empty")]


def _table_case(entry, counted, **kw):
    def build(dev):
        import fake_native
        from deepmetv2_amd import _native
        d, b = _gm_batch(20 if counted else 16, 32, counted, dev)
        rowptr = fake_native.table_rowptr(b.nbr_cpu, d["cnt"])
        E = int(rowptr[-1])
        if entry == "table_rowptr":
            return Case(lambda: _native.table_rowptr(b.nbr, b.cnt), lambda outs: _same(outs[0], rowptr, entry))
        ref = fake_native.table_edges(b.nbr_cpu, d["cnt"], rowptr, E, kw["swap"], kw["i64"], kw["i32"])
        rp = rowptr.to(dev)

        def check(outs):
            for got, want in zip(outs, [r for r in ref if r is not None]):
                _same(got, want, entry)
        return Case(lambda: _native.table_edges(b.nbr, b.cnt, rp, E, kw["swap"], kw["i64"], kw["i32"]), check)
    build.label = f"counted{int(counted)}" + "".join(f"-{n}{int(v)}" for n, v in kw.items())
    return build


def _same(got, want, what):
    assert got.dtype == want.dtype and torch.equal(got, want), what


CASES["table_rowptr"] = [_table_case("table_rowptr", False), _table_case("table_rowptr", True)]
CASES["table_edges"] = [_table_case("table_edges", False, swap=False, i64=True, i32=False),
                        _table_case("table_edges", True, swap=True, i64=True, i32=True),
                        _table_case("table_edges", True, swap=False, i64=False, i32=True)]


# =========================================================================================================================
# edge MLP: the three routes over a grouped edge list (forward state and every gradient), and the table form on bf16
# =========================================================================================================================
EMLP_N, EMLP_W = 129, (16, 32, 32)         # (Hin, H1, H2) of tests/test_gpu_edge_mlp_routes.py: supported by all three routes
EMLP_TOL = {"f32": 1e-4, "bf16": 2e-2, "f16": 2e-2}    # include/dmet.h: "within 1e-4 of the output and gradient scales" /
#                                                        "within rtol 2e-2 of the output and gradient scales ... (R6)"


@functools.lru_cache(maxsize=None)
def _emlp_graph():
    """Grouped by target, N = 129: node 0 isolated at both ends, node 9 without in-edges, node 7 a one-edge row, node 11 a
    70-edge row (across the 64-edge tile).  (rowptr, src, tgt, srcptr, srcperm) int32 on the CPU."""
    import fake_native
    g = _gen(3)
    deg = torch.randint(1, 9, (EMLP_N,), generator=g)
    deg[0], deg[9], deg[7], deg[11] = 0, 0, 1, 70
    tgt = torch.repeat_interleave(torch.arange(EMLP_N), deg)
    src = torch.randint(1, EMLP_N, (tgt.numel(),), generator=g)
    src[0] = 9
    rowptr = torch.cat([torch.zeros(1, dtype=torch.int64), deg.cumsum(0)]).to(torch.int32)
    srcptr, srcperm = fake_native.reverse_index(src.to(torch.int32), EMLP_N)
    return rowptr, src.to(torch.int32), tgt.to(torch.int32), srcptr, srcperm


def _emlp_parts(nn):
    mods = list(nn)
    bn = mods.pop() if isinstance(mods[-1], torch.nn.BatchNorm1d) else None
    return mods[0], mods[2], len(mods) == 4, bn


def _bn_running_ref(nn, x, ei):
    """(running_mean, running_var) after ONE training-mode forward of nn's trailing BatchNorm over the edge messages,
    in float64 (unbiased variance, torch's rule)."""
    import copy
    nn64 = copy.deepcopy(nn).double()
    bn = nn64[-1]
    x64 = x.double()
    with torch.no_grad():
        m = nn64[:-1](torch.cat([x64[ei[1]], x64[ei[0]] - x64[ei[1]]], 1))
        mean, var = m.mean(0), m.var(0, unbiased=True)
        return ((1 - bn.momentum) * bn.running_mean + bn.momentum * mean,
                (1 - bn.momentum) * bn.running_var + bn.momentum * var)


def _scale_close(got, ref, tol, scale, what):
    err = float((got.double() - ref.double()).abs().max()) if ref.numel() else 0.0
    assert bool(torch.isfinite(got).all()) and err <= tol * max(scale, 1e-6), (what, err, tol * max(scale, 1e-6))


def _emlp_fwd_args(dev, nn, x, bn_mode, aggr):
    rowptr, src, tgt, _sp, _pm = _emlp_graph()
    l1, l2, act2, bn = _emlp_parts(nn)
    t = lambda v: None if v is None else v.detach().to(dev)
    head = [t(x), t(rowptr), t(src), t(tgt), t(l1.weight), t(l1.bias), t(l2.weight), t(l2.bias), act2, aggr, bn_mode]
    return head + ([t(bn.weight), t(bn.bias), bn.eps, bn.momentum] if bn is not None else [None, None, 1e-5, 0.1])


def _emlp_fwd_case(route, aggr, bn_kind):
    def build(dev):
        from deepmetv2_amd import _native
        from edge_mlp_reference import max64, ref64
        from test_gpu_edge_mlp_f32 import _mlp
        Hin, H1, H2 = EMLP_W
        nn = _mlp(Hin, H1, H2, bn=bn_kind, neg_gamma=bn_kind is not None, seed=2)
        bn = _emlp_parts(nn)[3]
        mode = 0 if bn is None else (1 if bn.training else 2)
        x = torch.randn(EMLP_N, Hin, generator=_gen(1))
        rowptr, src, tgt, _sp, _pm = _emlp_graph()
        ei = torch.stack([src.long(), tgt.long()])
        has_in = (rowptr[1:] > rowptr[:-1])
        args = _emlp_fwd_args(dev, nn, x, mode, aggr)
        fwd = getattr(_native, f"edge_mlp_fwd_{route}")

        def call():
            stats = [None, None, None] if bn is None else [bn.running_mean.clone().to(dev), bn.running_var.clone().to(dev),
                                                           torch.zeros((), dtype=torch.int64, device=dev)]
            out, state = fwd(*args, *stats)
            return out, state, stats

        ref_nn = copy.deepcopy(nn)
        if aggr == "max":
            ref_out = max64(ref_nn, x, ei, "source_to_target")
            ref_out = torch.where(has_in.view(-1, 1), ref_out, torch.zeros_like(ref_out))
        else:
            ref_out = ref64(ref_nn, x, ei, aggr, "source_to_target", torch.zeros(EMLP_N, H2))[0]
        masks = {}
        if aggr == "max":
            # include/dmet.h, dmet_edge_mlp_fwd_f32: "win[2 N H2] int32 (max only: ... defined only for nodes with in-edges)"
            masks[3] = has_in.view(1, -1, 1).expand(2 if mode else 1, EMLP_N, H2)
        # include/dmet.h, dmet_edge_mlp_fwd_f32: "agg ... like win, defined only for nodes with in-edges"
        masks[2] = has_in.view(1, -1, 1).expand(2 if (aggr == "max" and mode) else 1, EMLP_N, H2)

        def check(outs):
            tol = EMLP_TOL[route]
            _scale_close(outs[0], ref_out, tol, float(ref_out.abs().max()), f"edge_mlp_fwd_{route} out")
            assert bool((outs[0][~has_in] == 0).all()), "a node without in-edges gives 0 (R3)"
            Pr, Qr = _dense_ref(x, nn[0].weight, nn[0].bias)
            _feat(outs[1], torch.cat([Pr, Qr], 1), f"edge_mlp_fwd_{route} pq")
            if mode == 1:
                rm, rv, nbt = outs[-3:]
                assert int(nbt) == 1
                # tests/test_gpu_parity.py test_edge_mlp2_bf16_with_trailing_batch_norm: running statistics of the edge messages
                rm_ref, rv_ref = _bn_running_ref(nn, x, ei)
                torch.testing.assert_close(rm.double(), rm_ref, rtol=2e-2, atol=2e-3)
                torch.testing.assert_close(rv.double(), rv_ref, rtol=3e-2, atol=2e-3)
        return Case(call, check, masks)
    build.label = f"{aggr}-bn{bn_kind}"
    return build


def _emlp_bwd_case(route, aggr, bn_kind, want_x=True):
    def build(dev):
        from deepmetv2_amd import _native
        from edge_mlp_reference import ref64
        from test_gpu_edge_mlp_f32 import _layer_scales, _mlp
        Hin, H1, H2 = EMLP_W
        nn = _mlp(Hin, H1, H2, bn=bn_kind, neg_gamma=bn_kind is not None, seed=2)
        l1, l2, act2, bn = _emlp_parts(nn)
        mode = 0 if bn is None else (1 if bn.training else 2)
        x = torch.randn(EMLP_N, Hin, generator=_gen(1))
        g = torch.randn(EMLP_N, H2, generator=_gen(5))
        rowptr, src, tgt, srcptr, srcperm = _emlp_graph()
        ei = torch.stack([src.long(), tgt.long()])
        args = _emlp_fwd_args(dev, nn, x, mode, aggr)
        stats = [None, None, None] if mode != 2 else [bn.running_mean.clone().to(dev), bn.running_var.clone().to(dev), None]
        _out, state = getattr(_native, f"edge_mlp_fwd_{route}")(*args, *stats)        # the state: built outside the block
        win = None
        if aggr == "max":
            w = state[2][0].long()
            if mode:
                w = torch.where(state[3][0] < 0, state[2][1].long(), w)
            win = torch.where((rowptr[1:] > rowptr[:-1]).view(-1, 1).to(dev), w, torch.full_like(w, -1)).cpu()
        ref_nn = copy.deepcopy(nn)
        if mode == 2:
            ref_nn.eval()
        _r_out, r_gx, r_grads = ref64(ref_nn, x, ei, aggr, "source_to_target", g, win)
        t = lambda v: v.detach().to(dev)
        bwd = getattr(_native, f"edge_mlp_bwd_{route}")

        def call():
            return bwd(t(g), t(x), t(rowptr), t(src), t(tgt), t(srcptr), t(srcperm), t(l1.weight), t(l2.weight),
                       None if l2.bias is None else t(l2.bias), act2, aggr, mode, state, want_x=want_x)

        def check(outs):
            tol = EMLP_TOL[route]
            outs = list(outs)
            if want_x:
                gx = outs.pop(0)
                _scale_close(gx, r_gx, tol, float(r_gx.abs().max()), f"edge_mlp_bwd_{route} gx")
                assert bool((gx[0] == 0).all()), "an isolated node takes no gradient"
            last = len(nn) - 1
            names = ["0.weight", "0.bias", "2.weight", "2.bias"] + ([f"{last}.weight", f"{last}.bias"] if mode else [])
            scale = _layer_scales(r_grads)
            for got, n in zip(outs, names):
                _scale_close(got, r_grads[n], tol, scale[n.rsplit(".", 1)[0]], f"edge_mlp_bwd_{route} {n}")
        return Case(call, check)
    build.label = f"{aggr}-bn{bn_kind}-x{int(want_x)}"
    return build


for _route in ("f32", "bf16", "f16"):
    CASES[f"edge_mlp_fwd_{_route}"] = [_emlp_fwd_case(_route, a, b) for a, b in
                                       (("max", None), ("max", "train"), ("add", "train"), ("mean", None), ("max", "eval"))]
    CASES[f"edge_mlp_bwd_{_route}"] = [_emlp_bwd_case(_route, a, b, wx) for a, b, wx in
                                       (("max", None, True), ("max", "train", True), ("add", "train", True),
                                        ("mean", None, False), ("max", "eval", True))]


def _emlp2_case(with_bn, aggr, training=True):
    def build(dev):
        from deepmetv2_amd import _native
        from edge_mlp_reference import max64, ref64
        from test_gpu_edge_mlp_f32 import _mlp
        H, H1, H2, k = 32, 48, 32, 16          # tests/test_gpu_parity.py test_edge_mlp2_bf16_mfma: the smallest supported shape
        assert _native.edge_mlp2_supported(H, H1, H2, k) if dev.type == "cuda" else True
        d, b = _gm_batch(k, 32, False, dev)
        N = d["P"].shape[0]
        x = torch.randn(N, H, generator=_gen(4))
        nn = _mlp(H, H1, H2, bn="train" if with_bn else None, neg_gamma=with_bn, seed=6)
        if with_bn and not training:
            nn.eval()
        l1, l2, act2, bn = _emlp_parts(nn)
        i, s = (b.nbr_cpu >= 0).nonzero(as_tuple=True)
        ei = torch.stack([b.nbr_cpu[i, s].long(), i])
        has = (b.nbr_cpu >= 0).any(1)
        ref_nn = copy.deepcopy(nn)
        if aggr == "max":
            ref = torch.where(has.view(-1, 1), max64(ref_nn, x, ei, "source_to_target"), torch.zeros(N, H2, dtype=torch.float64))
        else:
            ref = ref64(ref_nn, x, ei, "add", "source_to_target", torch.zeros(N, H2))[0]
        t = lambda v: v.detach().to(dev)
        head = [t(x), b.nbr, t(l1.weight), t(l1.bias), t(l2.weight), t(l2.bias), act2, aggr == "add"]

        def call():
            if not with_bn:
                return _native.edge_mlp2_bf16(*head)
            rm, rv = bn.running_mean.clone().to(dev), bn.running_var.clone().to(dev)
            nbt = torch.zeros((), dtype=torch.int64, device=dev)
            out = _native.edge_mlp2_bn_bf16(*head, t(bn.weight), t(bn.bias), bn.eps, bn.momentum, rm, rv, nbt, training)
            return out, rm, rv, nbt

        def check(outs):
            scale = float(ref.abs().max())
            # tests/test_gpu_parity.py: rtol 2e-2 of the output scale (R6); 3e-2 with the trailing BatchNorm
            tol = 3e-2 if with_bn else 2e-2
            _close(outs[0], ref, tol, tol * scale, "edge_mlp2" + ("_bn" if with_bn else "") + "_bf16")
            assert bool((outs[0][~has] == 0).all())
            if with_bn and training:
                assert int(outs[3]) == 1
                rm_ref, rv_ref = _bn_running_ref(nn, x, ei)
                torch.testing.assert_close(outs[1].double(), rm_ref, rtol=2e-2, atol=2e-3)
                torch.testing.assert_close(outs[2].double(), rv_ref, rtol=3e-2, atol=2e-3)
        return Case(call, check)
    build.label = f"{aggr}-train{int(training)}"
    return build


CASES["edge_mlp2_bf16"] = [_emlp2_case(False, "max"), _emlp2_case(False, "add")]
CASES["edge_mlp2_bn_bf16"] = [_emlp2_case(True, "max"), _emlp2_case(True, "add"), _emlp2_case(True, "max", training=False)]


# =========================================================================================================================
# per-node chain: encoder, head, BatchNorm and their compositions; A^T B
# =========================================================================================================================
EPS, MOMENTUM = 1e-5, 0.1


def _dev(ts, dev):
    return [None if t is None else t.to(dev) for t in ts]


def _encode_case(entry, N):
    def build(dev):
        import per_node_reference as pn
        from deepmetv2_amd import _native
        params = pn.encoder_params()
        x_cont, x_cat, g_h = pn.encoder_inputs(N, seed=pn.ENCODE_BN_SEEDS.get(N, 40 + N))
        pd_, xc, xk, gd = _dev(params, dev), x_cont.to(dev), x_cat.to(dev), g_h.to(dev)
        if entry == "encode_fwd":
            h_ref, _l = pn.encoder_ref(x_cont, x_cat, params)
            return Case(lambda: _native.encode_fwd(xc, xk, pd_), lambda outs: pn.close(outs[0], h_ref, "h", "encode_fwd"))
        if entry == "encode_bwd":
            _h, leaves = pn.encoder_ref(x_cont, x_cat, params, g_h)
            h = _native.encode_fwd(xc, xk, pd_)

            def check(outs):
                assert len(outs) == 9
                for got, leaf, name in zip(outs, leaves, pn.ENCODER_PARAM_NAMES):
                    pn.close(got, leaf.grad if leaf.grad is not None else torch.zeros_like(leaf), "grad", f"encode_bwd {name}")
            return Case(lambda: _native.encode_bwd(xc, xk, pd_, h, gd), check)
        state = pn.bn_state(32, 5)
        if N == 1:
            # torch's BatchNorm1d refuses one row in training mode, so the float64 module cannot serve.  The formula can: with
            # one row h == mean and g_y == mean_g exactly, so g_h = gamma invstd (g - mean_g - xhat mean_gx) = 0 and every
            # encoder gradient is 0; g_gamma = sum g xhat = 0 and g_beta = sum g = g_y[0]
            class ref:
                weight = type("P", (), {"grad": torch.zeros(32, dtype=torch.float64)})
                bias = type("P", (), {"grad": g_h[0].double()})
            leaves = [type("P", (), {"grad": torch.zeros_like(p, dtype=torch.float64)}) for p in params]
        else:
            _y, leaves, ref = pn.encode_bn_ref(x_cont, x_cat, params, state, g_h)
        h = _native.encode_fwd(xc, xk, pd_)
        mean, invstd = _native.bn_stats(h, EPS, MOMENTUM, None, None)
        if N == 1:      # the statistics are inputs of this entry: the one row's own, so that xhat is exactly 0
            mean, invstd = h[0].clone(), torch.full_like(mean, EPS ** -0.5)
        gamma = state["weight"].to(dev)

        def check(outs):
            assert len(outs) == 11
            for got, leaf, name in zip(outs[:9], leaves, pn.ENCODER_PARAM_NAMES):
                pn.close(got, leaf.grad, "grad", f"encode_bn_bwd {name}")
            pn.close(outs[9], ref.weight.grad, "grad", "encode_bn_bwd g_gamma")
            pn.close(outs[10], ref.bias.grad, "grad", "encode_bn_bwd g_beta")
        return Case(lambda: _native.encode_bn_bwd(xc, xk, pd_, h, gd, gamma, mean, invstd), check)
    build.label = f"N{N}"
    return build


CASES["encode_fwd"] = [_encode_case("encode_fwd", N) for N in (0, 1, 33, 257)]
CASES["encode_bwd"] = [_encode_case("encode_bwd", N) for N in (0, 1, 33, 257)]
# N = 0: the wrapper returns None before it allocates anything (nothing to poison; dense.encode_bn keeps the separate steps)
CASES["encode_bn_bwd"] = [_encode_case("encode_bn_bwd", N) for N in (1, 2, 33, 257)]


def _head_case(entry, N, with_res=True):
    def build(dev):
        import per_node_reference as pn
        from deepmetv2_amd import _native
        hp = pn.head_params()
        hpd = _dev(hp, dev)
        if entry == "bn_head_fwd":
            ops = _bn_operands(N, 32, 700 + N, with_res)
            emb_ref = _bn_affine_ref(*ops)
            out_ref, _l = pn.head_ref(emb_ref.float(), *hp)
            dops = _dev(ops, dev)

            def check(outs):
                pn.close(outs[0], emb_ref, "bn_y", "bn_head_fwd emb")
                pn.close(outs[1], out_ref, "head", "bn_head_fwd out")
            return Case(lambda: _native.bn_head_fwd(*dops, hpd), check)
        emb, g_out = pn.head_inputs(N, seed=60 + N)
        out_ref, leaves = pn.head_ref(emb, *hp, g_out)
        ed, gd = emb.to(dev), g_out.to(dev)
        if entry == "head_fwd":
            return Case(lambda: _native.head_fwd(ed, hpd), lambda outs: pn.close(outs[0], out_ref, "head", "head_fwd"))
        out = _native.head_fwd(ed, hpd)

        def check(outs):
            assert len(outs) == 5
            for got, leaf, name in zip(outs, leaves, ("g_emb", "gW1", "gb1", "gW2", "gb2")):
                pn.close(got, leaf.grad if leaf.grad is not None else torch.zeros_like(leaf), "grad", f"head_bwd {name}")
        return Case(lambda: _native.head_bwd(ed, hpd, out, gd), check)
    build.label = f"N{N}" + ("" if with_res else "-nores")
    return build


CASES["head_fwd"] = [_head_case("head_fwd", N) for N in (0, 1, 33, 257)]
CASES["head_bwd"] = [_head_case("head_bwd", N) for N in (0, 1, 33, 257)]
CASES["bn_head_fwd"] = [_head_case("bn_head_fwd", N, r) for N, r in ((0, True), (1, True), (3, True), (33, False), (257, True))]

BN_SHAPES = ((3, 8), (257, 32), (1025, 64))


def _normalised(x, mean, invstd):
    return (x.double() - mean.double()) * invstd.double()


def _bn_case(entry, N, H, training=True, with_res=True):
    def build(dev):
        import per_node_reference as pn
        from deepmetv2_amd import _native
        x, res, g_y = pn.bn_rows(N, H, seed=N + H)
        state = pn.bn_state(H, seed=N + H + 1)
        if not with_res:
            res = None
        xd, rd, gd = x.to(dev), None if res is None else res.to(dev), g_y.to(dev)
        gamma, beta = state["weight"].to(dev), state["bias"].to(dev)
        y_ref, ref, x64, _r = pn.bn_ref(x, state, training, res, g_y if entry == "bn_bwd" else None)
        # the statistics of the reference: what its own transform used
        if training:
            mean_ref = x.double().mean(0)
            inv_ref = 1.0 / torch.sqrt(x.double().var(0, unbiased=False) + EPS)
        else:
            mean_ref = state["running_mean"].double()
            inv_ref = 1.0 / torch.sqrt(state["running_var"].double() + EPS)
        xhat_ref = _normalised(x, mean_ref, inv_ref)

        def fresh():
            return (state["running_mean"].clone().to(dev), state["running_var"].clone().to(dev),
                    torch.zeros((), dtype=torch.int64, device=dev))

        def check_running(rm, rv, nbt):
            pn.close(rm, ref.running_mean, "running", f"{entry} running_mean")
            pn.close(rv, ref.running_var, "running", f"{entry} running_var")
            assert int(nbt) == (1 if training else 0)

        def check_stats(mean, invstd):
            # no test holds save_mean / save_invstd to a bar of their own: they are held through the transform they define,
            # at the bar of its output (per_node_reference BARS["bn_y"])
            pn.close(_normalised(x, mean, invstd).float(), xhat_ref, "bn_y", f"{entry} statistics")

        if entry == "bn_fwd":
            def call():
                rm, rv, nbt = fresh()
                return _native.bn_fwd(xd, rd, gamma, beta, EPS, MOMENTUM, rm, rv, training, nbt), rm, rv, nbt

            def check(outs):
                pn.close(outs[0], y_ref, "bn_y", "bn_fwd y")
                check_stats(outs[1], outs[2])
                check_running(*outs[3:])
            return Case(call, check)
        if entry == "bn_stats":
            def call():
                rm, rv, nbt = fresh()
                return _native.bn_stats(xd, EPS, MOMENTUM, rm, rv, nbt), rm, rv, nbt

            def check(outs):
                check_stats(outs[0], outs[1])
                check_running(*outs[2:])
            return Case(call, check)
        if entry == "bn_eval_stats":
            rm, rv, _n = fresh()
            return Case(lambda: _native.bn_eval_stats(rm, rv, EPS), lambda outs: check_stats(outs[0], outs[1]))
        md, idv = mean_ref.float().to(dev), inv_ref.float().to(dev)
        if entry == "bn_apply":
            y2 = _bn_affine_ref(x, res, state["weight"], state["bias"], mean_ref.float(), inv_ref.float())
            return Case(lambda: _native.bn_apply(xd, rd, gamma, beta, md, idv),
                        lambda outs: pn.close(outs[0], y2, "bn_y", "bn_apply"))

        def check(outs):
            pn.close(outs[0], x64.grad, "g_x", "bn_bwd g_x")
            pn.close(outs[1], ref.weight.grad, "grad", "bn_bwd g_gamma")
            pn.close(outs[2], ref.bias.grad, "grad", "bn_bwd g_beta")
        return Case(lambda: _native.bn_bwd(xd, gd, gamma, md, idv), check)
    build.label = f"N{N}-H{H}-train{int(training)}-res{int(with_res)}"
    return build


CASES["bn_fwd"] = [_bn_case("bn_fwd", N, H, True, N != 257) for N, H in BN_SHAPES] + [_bn_case("bn_fwd", 257, 32, False)]
CASES["bn_stats"] = [_bn_case("bn_stats", N, H) for N, H in BN_SHAPES]
CASES["bn_apply"] = [_bn_case("bn_apply", N, H, True, N != 3) for N, H in BN_SHAPES]
CASES["bn_eval_stats"] = [_bn_case("bn_eval_stats", N, H, False) for N, H in BN_SHAPES]
CASES["bn_bwd"] = [_bn_case("bn_bwd", N, H, True, False) for N, H in BN_SHAPES]

# (1, 1, 16): one row; (9, 16, 40) and (4097, 40, 16): the <1,2> and <2,1> instances of xty_partial_kernel; (1000, 64, 33):
# both widths past one tile; N = 0
XTY_SHAPES = ((1, 1, 16), (9, 16, 40), (4097, 40, 16), (1000, 64, 33), (0, 16, 24))


def _xty_case(entry, N, Ha, Hb):
    def build(dev):
        from deepmetv2_amd import _native
        g = _gen(N + Ha)
        A, Bm = torch.randn(N, Ha, generator=g), torch.randn(N, Hb, generator=g)
        Bd = Bm.to(dev)
        if entry == "xty":
            # tests/test_gpu_parity.py test_dense_weight_grad_kernels: |err| <= 1e-5 max(|A|^T |B|)
            ref = A.double().t() @ Bm.double()
            tol = 1e-5 * float((A.abs().double().t() @ Bm.abs().double()).max()) if N else 0.0
            Ad = A.to(dev)
            return Case(lambda: _native.xty(Ad, Bd),
                        lambda outs: _scale_close(outs[0], ref, 1.0, tol, "xty") if N else _same(outs[0], ref.float(), "xty"))
        if entry == "onehot_xty":
            R = min(Ha, 8)
            idx = torch.randint(0, R, (N,), generator=g)
            ref = torch.zeros(R, Hb, dtype=torch.float64).index_add_(0, idx, Bm.double())
            idd = idx.to(dev)
            return Case(lambda: _native.onehot_xty(idd, Bd, R),
                        lambda outs: _scale_close(outs[0], ref, 1e-5, max(1.0, float(ref.abs().max())), "onehot_xty"))
        ref = Bm.double().sum(0)
        tol = 1e-5 * float(Bm.abs().double().sum(0).max()) if N else 0.0
        return Case(lambda: _native.xty_wide_ones(Bd), lambda outs: _scale_close(outs[0], ref, 1.0, tol, "xty_wide_ones"))
    build.label = f"N{N}-{Ha}x{Hb}"
    return build


CASES["xty"] = [_xty_case("xty", *s) for s in XTY_SHAPES]
CASES["onehot_xty"] = [_xty_case("onehot_xty", *s) for s in XTY_SHAPES]
CASES["xty_wide_ones"] = [_xty_case("xty_wide_ones", 1000, 1, 33), _xty_case("xty_wide_ones", 4097, 1, 130),
                          _xty_case("xty_wide_ones", 1, 1, 16)]


# =========================================================================================================================
# segment, scatter and MET
# =========================================================================================================================
SEG_DEG = (0, 3, 1, 0, 0, 70, 2, 300, 5, 0)          # empty first, middle and last segments; rows across a 256-edge chunk


def _seg_case(entry, H):
    def build(dev):
        import fake_native
        from deepmetv2_amd import _native
        from test_gpu_scatter import _ints
        deg = torch.tensor(SEG_DEG * 3 + (0,))
        N, E = deg.numel(), int(deg.sum())
        rowptr = torch.cat([torch.zeros(1, dtype=torch.int64), deg.cumsum(0)]).to(torch.int32)
        g = _gen(17 + H)
        msg = _ints((E, H), g) / 8               # multiples of 1/8 in [-1, 1]: every sum is exact, many maxima tie
        g_out = _ints((N, H), g) / 8
        rp, md, gd = rowptr.to(dev), msg.to(dev), g_out.to(dev)
        empty = deg == 0
        if entry == "segment_sum":
            ref = fake_native.segment_sum(msg.double(), rowptr.long(), N).float()
            return Case(lambda: _native.segment_sum(md, rp, N), lambda outs: _same(outs[0], ref, entry))
        if entry == "segment_max":
            ref, _arg = fake_native.segment_max(msg, rowptr.long(), N)

            def check(outs):
                _same(outs[0], ref, entry)
                assert bool((outs[0][empty] == 0).all())
                a = outs[1].long()
                tgt = fake_native._tgt_of(rowptr.long(), N)
                assert bool((a[empty] < 0).all())                                     # no winner in an empty segment
                ne = ~empty
                lo, hi = rowptr[:-1].long().view(-1, 1), rowptr[1:].long().view(-1, 1)
                assert bool(((a >= lo) & (a < hi))[ne].all())
                assert torch.equal(msg.gather(0, a.clamp(min=0))[ne], ref[ne])        # the winner holds the maximum
                first = torch.full((N, H), E, dtype=torch.int64).scatter_reduce(
                    0, tgt.view(-1, 1).expand(E, H), torch.where(msg == ref[tgt], torch.arange(E).view(-1, 1).expand(E, H),
                                                                 torch.full((E, H), E)), "amin")
                assert torch.equal(a[ne], first[ne])                                  # R4: the lowest position wins ties
            return Case(lambda: _native.segment_max(md, rp, N), check)
        if entry == "segment_sum_bwd":
            ref = fake_native.segment_sum_bwd(g_out, rowptr.long(), E)
            return Case(lambda: _native.segment_sum_bwd(gd, rp, E), lambda outs: _same(outs[0], ref, entry))
        first = _native.segment_max(md, rp, N)[1]                      # the kernel's own winners (lowest position)
        ref = fake_native.segment_max_bwd(g_out, first.cpu(), rowptr.long(), E)
        return Case(lambda: _native.segment_max_bwd(gd, first, rp, E), lambda outs: _same(outs[0], ref, entry))
    build.label = f"H{H}"
    return build


for _e in ("segment_sum", "segment_max", "segment_sum_bwd", "segment_max_bwd"):
    CASES[_e] = [_seg_case(_e, H) for H in (3, 32)]


def _met_case(entry, B):
    def build(dev):
        import fake_native
        from deepmetv2_amd import _native
        from test_gpu_scatter import U, _ints, _met_data, _sum_ref
        g = _gen(500 + B)
        x, w, batch, truth = _met_data(B, g)
        if B > 1:
            sizes = torch.bincount(batch, minlength=B)
            assert sizes[0] == 0 and bool((sizes[1:-1] == 0).any())
        ptr = _ptr_of(torch.bincount(batch, minlength=B).tolist())
        if entry == "met_loss":
            met = _ints((B, 2), g, -64, 64) / 16
            r = met.double() + truth[:, :2].double()
            loss_ref, g_ref = 0.5 * (r * r).sum() / B, r / B
            md, td = met.to(dev), truth.to(dev)

            def check(outs):
                # tests/test_gpu_scatter.py test_met_reduce_and_loss: gamma = (2B + 8) u for the loss, 4 u |g| for the gradient
                assert abs(float(outs[0]) - float(loss_ref)) <= (2 * B + 8) * U * float(loss_ref)
                assert bool(((outs[1].double() - g_ref).abs() <= 4 * U * g_ref.abs()).all())
            return Case(lambda: _native.met_loss(md, td), check)
        xd, pd = x.to(dev), ptr.to(dev)
        if entry == "met_reduce":
            ref = _sum_ref(w.double().view(-1, 1) * x[:, :2].double(), batch, B).float()
            wd = w.to(dev)
            return Case(lambda: _native.met_reduce(wd, xd, pd), lambda outs: _same(outs[0], ref, entry))
        if entry == "segment_sum_1d":
            ref = fake_native.segment_sum_1d(w.double(), ptr).float()
            wd = w.to(dev)
            return Case(lambda: _native.segment_sum_1d(wd, pd), lambda outs: _same(outs[0], ref, entry))
        coef = _ints((B, 2), g)
        ref = fake_native.met_reduce_bwd(coef.double(), x.double(), ptr).float()
        cd = coef.to(dev)
        return Case(lambda: _native.met_reduce_bwd(cd, xd, pd), lambda outs: _same(outs[0], ref, entry))
    build.label = f"B{B}"
    return build


for _e in ("met_reduce", "met_reduce_bwd", "segment_sum_1d", "met_loss"):
    CASES[_e] = [_met_case(_e, B) for B in (1, 257)]


def _batch_to_ptr_case(sizes):
    def build(dev):
        from deepmetv2_amd import _native
        ptr = _ptr_of(sizes)
        batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(dev)
        return Case(lambda: _native.batch_to_ptr(batch, len(sizes)), lambda outs: _same(outs[0], ptr, "batch_to_ptr"))
    build.label = "-".join(map(str, sizes))
    return build


# leading, interior and trailing empty events; a sorted, in-range vector only (the header leaves the rest unspecified)
CASES["batch_to_ptr"] = [_batch_to_ptr_case(s) for s in ((0, 0, 5, 0, 0, 300, 1, 0), (7,), (0, 0, 0))]


def _edge_features_case(entry, H):
    def build(dev):
        import fake_native
        import knn_xy_reference as xy
        from deepmetv2_amd import _native
        rowptr, src, tgt, srcptr, srcperm = _emlp_graph()             # nodes without an edge at either end
        N, E = EMLP_N, src.numel()
        g = _gen(90 + H)
        x, x2 = torch.randn(N, H, generator=g), torch.randn(N + 5, H, generator=g)
        g_feat = torch.randn(E, 2 * H, generator=g)
        ops = _dev([rowptr, src, tgt, srcptr, srcperm], dev)
        if entry == "edge_features":            # tests/test_gpu_edgeconv_xy.py test_edge_features_kernel_bit_exact: one subtraction
            ref = fake_native.edge_features(x, src, tgt)
            xd = x.to(dev)
            return Case(lambda: _native.edge_features(xd, ops[1], ops[2]), lambda outs: _same(outs[0], ref, entry))
        if entry == "edge_features_xy":
            ref = xy.edge_features_xy(x2, x, src, tgt)
            xs, xd = x2.to(dev), x.to(dev)
            return Case(lambda: _native.edge_features_xy(xs, xd, ops[1], ops[2]), lambda outs: _same(outs[0], ref, entry))
        gd = g_feat.to(dev)
        if entry == "edge_features_bwd":
            ref = fake_native.edge_features_bwd(g_feat.double(), rowptr.long(), srcptr.long(), srcperm, N, H)

            def check(outs):
                _grad4(outs[0], ref, entry)
                assert bool((outs[0][0] == 0).all()), "a node without an edge takes no gradient"
            return Case(lambda: _native.edge_features_bwd(gd, ops[0], ops[3], ops[4], N, H), check)
        r_src, r_dst = xy.edge_features_xy_bwd(g_feat.double(), rowptr.long(), srcptr.long(), srcperm, N, N, H)

        def check(outs):
            _grad4(outs[0], r_src, entry + " g_src")
            _grad4(outs[1], r_dst, entry + " g_dst")
            assert bool((outs[0][0] == 0).all()) and bool((outs[1][0] == 0).all()) and bool((outs[1][9] == 0).all())
        return Case(lambda: _native.edge_features_xy_bwd(gd, ops[0], ops[3], ops[4], N, N, H), check)
    build.label = f"H{H}"
    return build


for _e in ("edge_features", "edge_features_bwd", "edge_features_xy", "edge_features_xy_bwd"):
    # dmet_edge_features_f32 takes multiples of 4; the others any H
    CASES[_e] = [_edge_features_case(_e, H) for H in ((4, 32) if _e == "edge_features" else (3, 32))]


# =========================================================================================================================
# GravNet and attention aggregation
# =========================================================================================================================
def _agg_table(kind):
    """(nbr [Nt, k] int32 on the CPU, Ns): "one": the gather-max table (holes, rows without a neighbour: cnt == 0 targets);
    "two": its first 200 rows as queries over all N sources (sources no target points to); "none": Nt == 0 with Ns > 0."""
    d = _gm_data(16, 32, False)
    nbr, N = d["nbr"], d["P"].shape[0]
    if kind == "two":
        return nbr[:200].contiguous(), N
    if kind == "none":
        return nbr[:0].contiguous(), N
    return nbr, N


def _gravnet_case(entry, kind, S=4, P=22):
    def build(dev):
        import gravnet_reference as gr
        from deepmetv2_amd import _native
        nbr, Ns = _agg_table(kind)
        Nt, k = nbr.shape
        g = _gen(33)
        h, s_src = torch.randn(Ns, P, generator=g), 0.3 * torch.randn(Ns, S, generator=g)
        s_tgt = s_src if kind == "one" else 0.3 * torch.randn(Nt, S, generator=g)
        g_out = torch.randn(Nt, 2 * P, generator=g)
        hd, ssd, nd = h.to(dev), s_src.to(dev), nbr.to(dev)
        std = ssd if kind == "one" else s_tgt.to(dev)
        h64, s64 = h.double().requires_grad_(True), s_src.double().requires_grad_(True)
        t64 = None if kind == "one" else s_tgt.double().requires_grad_(True)
        r_out, bar, msg, valid, _own = gr.aggregate(h64.detach(), s64.detach(), nbr, None if t64 is None else t64.detach())
        empty = ~valid.any(1)
        if kind == "one":
            assert bool(empty.any())
        if entry == "gravnet_fwd":
            def check(outs):
                out, arg, cnt = outs
                # tests/test_gpu_gravnet.py _check: per row |err| <= 1e-5 bar + 1e-6; empty rows exact zeros, arg 255
                lim = 1e-5 * bar + 1e-6
                err = (out.double() - r_out).abs().amax(1) if Nt else torch.zeros(0, dtype=torch.float64)
                assert bool((err <= lim).all()), ("gravnet_fwd out", float((err - lim).max()) if Nt else 0.0)
                assert bool((out[empty] == 0).all()) and bool((arg[empty] == 255).all())
                assert torch.equal(cnt, valid.sum(1).to(torch.int32))
                a = arg[~empty].long()
                assert bool((a < k).all()) and (a.numel() == 0 or bool(valid[~empty].gather(1, a).all()))
                if a.numel():
                    at = msg[~empty].gather(1, a.unsqueeze(1)).squeeze(1)
                    assert bool((r_out[~empty][:, P:] - at <= lim[~empty].unsqueeze(1)).all()), "gravnet_fwd arg"
            return Case(lambda: _native.gravnet_fwd(hd, ssd, std, nd), check)
        _o, arg, cnt = _native.gravnet_fwd(hd, ssd, std, nd)                   # the forward state: built outside the block
        rev_ptr, rev_pos = _native.reverse_index(nd.view(-1), Ns)
        gd = g_out.to(dev)
        r = gr.aggregate(h64, s64, nbr, t64, arg=arg.cpu())[0]
        r.backward(g_out.double())
        zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
        refs = [zero(h64), zero(s64) if kind != "one" else None, None]
        unused = torch.ones(Ns, dtype=torch.bool)
        unused[nbr[nbr >= 0].long()] = False

        def check(outs):
            g_h, g_ss, g_st = outs
            # tests/test_gpu_gravnet.py _check: rtol 1e-4, atol 1e-4 max|ref|
            _grad4(g_h, refs[0], "gravnet_bwd g_h")
            if kind == "one":
                _grad4(g_ss.double() + g_st.double(), zero(s64), "gravnet_bwd g_s (both roles)")
            else:
                _grad4(g_ss, refs[1], "gravnet_bwd g_s_src")
                _grad4(g_st, zero(t64), "gravnet_bwd g_s_tgt")
                assert bool(unused.any()) and bool((g_h[unused] == 0).all()) and bool((g_ss[unused] == 0).all()), \
                    "the gradient rows of a source no target points to must be 0"
            assert bool((g_st[empty] == 0).all())
        return Case(lambda: _native.gravnet_bwd(gd, hd, ssd, std, nd, rev_ptr, rev_pos, arg, cnt), check)
    build.label = f"{kind}-S{S}-P{P}"
    return build


CASES["gravnet_fwd"] = [_gravnet_case("gravnet_fwd", k_) for k_ in ("one", "two", "none")] + [
    _gravnet_case("gravnet_fwd", "one", 1, 33)]
CASES["gravnet_bwd"] = [_gravnet_case("gravnet_bwd", k_) for k_ in ("one", "two", "none")] + [
    _gravnet_case("gravnet_bwd", "two", 16, 65)]


def _attention_case(entry, kind, form, H=2, C=16):
    def build(dev):
        import attention_reference as ar
        from deepmetv2_amd import _native
        nbr, Ns = _agg_table(kind)
        Nt, k = nbr.shape
        g = _gen(44)
        q, kk, v = (torch.randn(n, H, C, generator=g) for n in (Nt, Ns, Ns))
        g_out = torch.randn(Nt, H, C, generator=g)
        tgt, src, pos = ar.table_entries(nbr, Ns)
        deg = torch.bincount(tgt, minlength=Nt)
        q64, k64, v64 = (t.double().requires_grad_(True) for t in (q, kk, v))
        r_out, r_alpha, bar = ar.attention(q64, k64, v64, tgt, src)
        qd, kd, vd = q.to(dev), kk.to(dev), v.to(dev)
        if form == "table":
            idx, rowptr, tg = nbr.to(dev), None, None
        else:
            idx = src.to(torch.int32).to(dev)
            rowptr = torch.cat([torch.zeros(1, dtype=torch.int64), deg.cumsum(0)]).to(torch.int32).to(dev)
            tg = tgt.to(torch.int32).to(dev)
        if entry == "attention_fwd":
            score = (q64[tgt] * k64[src]).sum(-1).detach() / C ** 0.5
            m = torch.full((Nt, H), float("-inf"), dtype=torch.float64).scatter_reduce(
                0, tgt.view(-1, 1).expand(-1, H), score, "amax", include_self=True)
            lse_ref = m + torch.log(torch.zeros((Nt, H), dtype=torch.float64).index_add(0, tgt, torch.exp(score - m[tgt])))
            lse_ref = torch.where(deg.view(-1, 1) > 0, lse_ref, torch.zeros_like(lse_ref))

            def check(outs):
                out, lse, alpha = outs
                ar.assert_output_bar(out, r_out.detach(), bar, "attention_fwd")
                assert bool((out[deg == 0] == 0).all()) and bool((lse[deg == 0] == 0).all())
                a = alpha.double()
                # tests/test_gpu_attention.py _check: alpha rtol 1e-4, atol 1e-6
                ref_a = r_alpha.detach()
                if form == "table" and Nt:
                    ref_a = ar.table_alpha(ref_a, pos, Nt, k).reshape(Nt * k, H)
                torch.testing.assert_close(a, ref_a, rtol=1e-4, atol=1e-6)
                # alpha = exp(score - lse): the alpha bar's rtol 1e-4 is an absolute 1e-4 on lse
                assert bool(((lse.double() - lse_ref).abs() <= 1e-4).all()), "attention_fwd lse"
            return Case(lambda: _native.attention_fwd(qd, kd, vd, idx, rowptr, want_alpha=True), check)
        out, lse, _a = _native.attention_fwd(qd, kd, vd, idx, rowptr)          # the forward state: built outside the block
        keys = nbr.to(dev).view(-1) if form == "table" else idx
        rev_ptr, rev_pos = _native.reverse_index(keys.contiguous(), Ns)
        gd = g_out.to(dev)
        r_out.backward(g_out.double())
        zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
        unused = torch.ones(Ns, dtype=torch.bool)
        unused[src] = False

        def check(outs):
            for got, ref, name in zip(outs, (zero(q64), zero(k64), zero(v64)), ("g_q", "g_k", "g_v")):
                ar.assert_grad_bar(got, ref, f"attention_bwd {name}")
            assert bool((outs[0][deg == 0] == 0).all())
            if kind != "one":
                assert bool(unused.any()) and bool((outs[1][unused] == 0).all()) and bool((outs[2][unused] == 0).all()), \
                    "the gradient rows of a source no target points to must be 0"
        return Case(lambda: _native.attention_bwd(gd, qd, kd, vd, out, lse, idx, rev_ptr, rev_pos, rowptr, tg), check)
    build.label = f"{kind}-{form}-H{H}-C{C}"
    return build


CASES["attention_fwd"] = [_attention_case("attention_fwd", k_, f) for k_, f in
                          (("one", "table"), ("two", "table"), ("two", "list"), ("none", "table"))] + [
                          _attention_case("attention_fwd", "one", "list", 1, 40)]
CASES["attention_bwd"] = [_attention_case("attention_bwd", k_, f) for k_, f in
                          (("one", "table"), ("two", "table"), ("two", "list"), ("none", "table"))] + [
                          _attention_case("attention_bwd", "one", "list", 1, 40)]


# =========================================================================================================================
# pool and fps: the edge shapes of tests/test_gpu_pool_edges.py and tests/test_gpu_fps.py
# =========================================================================================================================
def _graclus_case(weighted, max_rounds):
    def build(dev):
        import pool_reference as ref
        from deepmetv2_amd import _native
        from test_gpu_pool_edges import _csr_with_entries_to_ignore
        ptr, (rowptr, col), _clean, _keep = _csr_with_entries_to_ignore([40, 1, 0, 25, 300], seed=3)
        w = (np.random.default_rng(4).integers(0, 4, len(col)) * 0.25).astype(np.float32) if weighted else None
        c_ref, p_ref, r_ref = ref.graclus(rowptr, col, w, ptr, 9, max_rounds)
        assert (p_ref < 0).any() and (p_ref >= 0).any()           # singletons (the one-node event) and pairs
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
        ops = [t(rowptr, torch.int64), t(col, torch.int32), None if w is None else t(w, torch.float32), t(ptr, torch.int64)]

        def check(outs):
            assert torch.equal(outs[0], torch.from_numpy(c_ref)) and torch.equal(outs[1].long(), torch.from_numpy(p_ref))
            assert torch.equal(outs[2].long(), torch.from_numpy(np.asarray(r_ref)).long())
        return Case(lambda: _native.graclus(*ops, 9, max_rounds, want_rounds=True), check)
    build.label = f"w{int(weighted)}-rounds{max_rounds}"
    return build


CASES["graclus"] = [_graclus_case(w, r) for w, r in ((False, 0), (True, 0), (True, 1))]


def _ncut_case(two_d):
    def build(dev):
        from deepmetv2_amd import _native
        N = 129
        rng = np.random.default_rng(8)
        a = np.concatenate([np.arange(N), rng.integers(0, N, 300)])
        b = np.concatenate([(np.arange(N) + 1) % N, rng.integers(0, N, 300)])
        row, col = np.concatenate([a, b]), np.concatenate([b, a])           # symmetric: every degree >= 2
        x = rng.standard_normal((N, 3)).astype(np.float32)
        attr = rng.random(len(row)).astype(np.float32)
        deg = np.bincount(col, minlength=N).astype(np.float64)
        x64 = x.astype(np.float64)
        base = np.sqrt(((x64[row] - x64[col]) ** 2).sum(1)) if two_d else attr.astype(np.float64)
        want = torch.from_numpy(base * (1.0 / deg[row] + 1.0 / deg[col]))
        ei = torch.from_numpy(np.stack([row, col])).to(dev)
        xd, ad = torch.from_numpy(x).to(dev), torch.from_numpy(attr).to(dev)

        def check(outs):       # tests/test_gpu_pool_edges.py test_normalized_cut_general: four fp32 roundings, rtol 3e-7
            torch.testing.assert_close(outs[0].double(), want, rtol=3e-7, atol=0)
        return Case(lambda: _native.normalized_cut(ei, N, attr=None if two_d else ad, x=xd if two_d else None), check)
    build.label = "2d" if two_d else "attr"
    return build


CASES["normalized_cut"] = [_ncut_case(False), _ncut_case(True)]


def _pool_case(entry, share, F=8):
    def build(dev):
        import pool_reference as ref
        from deepmetv2_amd import _native
        from test_gpu_pool_edges import _matching, _same_bits
        ptr, partner, cid_ref, pp_ref = _matching("pool", share)            # singletons, unmatched nodes, an empty event
        N, C = len(partner), int(pp_ref[-1])
        rng = np.random.default_rng(100 * F + int(10 * share))
        x = ref.tie_grid(rng, (N, F))
        mx_ref, arg_ref, mean_ref, pb_ref = ref.pool_pairs(x, partner, cid_ref, ptr, C)
        pd_ = torch.from_numpy(partner).to(torch.int32).to(dev)
        ptrd, cidd, xd = torch.from_numpy(ptr).to(dev), torch.from_numpy(cid_ref).to(dev), torch.from_numpy(x).to(dev)
        if entry == "pool_pairs_index":
            def check(outs):
                assert torch.equal(outs[0], torch.from_numpy(cid_ref)) and torch.equal(outs[1], torch.from_numpy(pp_ref))
            return Case(lambda: _native.pool_pairs_index(pd_, ptrd), check)
        if entry == "pool_pairs":
            def check(outs):
                assert _same_bits(outs[0], mx_ref) and torch.equal(outs[1], torch.from_numpy(arg_ref))
                assert _same_bits(outs[2], mean_ref) and torch.equal(outs[3], torch.from_numpy(pb_ref))
            return Case(lambda: _native.pool_pairs(xd, pd_, cidd, ptrd, C, True, True, True), check)
        g_max = (rng.integers(-8, 9, (C, F)) * 0.25).astype(np.float32)
        g_mean = (rng.integers(-8, 9, (C, F)) * 0.25 + 0.125).astype(np.float32)
        want = ref.pool_pairs_bwd(g_max, arg_ref, g_mean, partner, cid_ref, F)
        gm, ga, argd = torch.from_numpy(g_max).to(dev), torch.from_numpy(g_mean).to(dev), torch.from_numpy(arg_ref).to(dev)
        return Case(lambda: _native.pool_pairs_bwd(gm, argd, ga, pd_, cidd, F, C),
                    lambda outs: _assert(_same_bits(outs[0], want), "pool_pairs_bwd"))
    build.label = f"share{share}-F{F}"
    return build


def _assert(ok, what):
    assert ok, what


for _e in ("pool_pairs_index", "pool_pairs", "pool_pairs_bwd"):
    CASES[_e] = [_pool_case(_e, 0.0, 8), _pool_case(_e, 0.5, 65), _pool_case(_e, 1.0, 3)]


def _fps_case(sizes, m, start, D):
    def build(dev):
        import fps_reference as fr
        from deepmetv2_amd import _native
        ptr = _ptr_of(sizes).numpy()
        x = np.random.default_rng(6 + D).standard_normal((sum(sizes), D)).astype(np.float32)
        m_ = np.asarray(m, dtype=np.int64)
        out_ptr = np.concatenate([[0], np.cumsum(m_)]).astype(np.int64)
        st = None if start is None else np.asarray(start, dtype=np.int64)
        want = fr.fps(x, ptr, m_, st)
        ops = [torch.from_numpy(x).to(dev), torch.from_numpy(ptr).to(dev), torch.from_numpy(out_ptr).to(dev),
               None if st is None else torch.from_numpy(st).to(dev)]

        def check(outs):
            assert np.array_equal(outs[0].numpy(), want)
        return Case(lambda: _native.fps(*ops, int(out_ptr[-1])), check)
    build.label = f"{'-'.join(map(str, sizes))}-D{D}"
    return build


# an empty event, a one-node event, m = 1, m > n with clamped starts (tests/test_gpu_fps.py); past one 1024-thread workgroup
CASES["fps"] = [_fps_case((5, 0, 1027, 1, 70, 0), (2, 0, 103, 1, 1, 0), None, 2),
                _fps_case((9, 70, 3), (14, 20, 3), (-3, 10 ** 6, 1), 3), _fps_case((130,), (65,), None, 13)]


# =========================================================================================================================
# the runner
# =========================================================================================================================
def _params():
    return [pytest.param(name, i, id=f"{name}-{b.label}") for name in CASES for i, b in enumerate(CASES[name])]


def _run_case(dev, monkeypatch, spec):
    """call() under both patterns: {pattern: CPU tensors}, or a skip when a diagnostic switch makes the entry decline."""
    from deepmetv2_amd import _native
    for k, v in spec.env.items():
        monkeypatch.setenv(k, v)
    for k, v in spec.attrs.items():
        monkeypatch.setattr(_native, k, v)
    got = pa.run_both(spec.call)
    torch.cuda.synchronize(dev)
    return got


def _compare(got, masks, what, canon=None):
    a, b = got["ones"], got["zeros_huge"]
    assert len(a) == len(b), (what, len(a), len(b))
    for pos, (x, y) in enumerate(zip(a, b)):
        if canon and pos in canon:
            x, y = canon[pos](x), canon[pos](y)
        bad = pa.differing(x, y, masks.get(pos))
        assert bad.numel() == 0, (f"{what}: output {pos} {tuple(x.shape)} {x.dtype} differs between the two patterns in "
                                  f"{bad.numel()} elements, first at flat index {int(bad[0])}: "
                                  f"{x.reshape(-1)[bad[:4]].tolist()} vs {y.reshape(-1)[bad[:4]].tolist()}")


@pytest.mark.parametrize("name,i", _params())
def test_case(dev, monkeypatch, name, i):
    spec = CASES[name][i](dev)
    reason = spec.skip_if() if spec.skip_if else None
    if reason:
        pytest.skip(reason)
    got = _run_case(dev, monkeypatch, spec)
    what = f"{name}[{CASES[name][i].label}]"
    if spec.declines:
        assert not got["ones"] and not got["zeros_huge"], f"{what} was expected to decline: {spec.declines}"
        return
    if not got["ones"] and not got["zeros_huge"]:
        if SWITCHED:
            pytest.skip(f"{what}: the entry declined under {SWITCHED}")
        raise AssertionError(f"{what}: the wrapper returned no tensor")
    _compare(got, spec.masks, what, spec.canon)
    spec.check(got["ones"])


def test_counted_radius_shows_poison_without_its_mask(dev, monkeypatch):
    """The sensitivity of the harness, on a region the header already declares unwritten: the counted radius form
    (fill == 0) compared WITHOUT its mask must differ between the patterns, and only in slots >= cnt."""
    spec = _radius_case(2, 9, False, False, False, True, "none", "windowed")(dev)
    got = _run_case(dev, monkeypatch, spec)
    nbr_a, nbr_b = got["ones"][0], got["zeros_huge"][0]
    bad = pa.differing(nbr_a, nbr_b)
    keep = spec.masks[0]
    assert bad.numel() > 0, "poison did not reach the device, or the comparison does not see it"
    assert not bool(keep.reshape(-1)[bad].any()), "a slot below cnt differs"
    unwritten = (~keep).reshape(-1).nonzero().view(-1)
    assert torch.equal(bad, unwritten), "every slot >= cnt keeps what the allocation held: -1 under ones, 0 under zeros_huge"
    assert bool((nbr_a.reshape(-1)[unwritten] == -1).all()) and bool((nbr_b.reshape(-1)[unwritten] == 0).all())
