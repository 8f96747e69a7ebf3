"""K3: the two forms of gather_max_launch (csrc/edgeconv.hip) that no other test reaches by name -- the mixed form
(dmet_gather_max_mixed_f32: an LDS launch that skips the events beyond its image, then an L2 launch for those) and the
half-image form (dmet_gather_max_lds_sliced_cap_f32 with a max_nodes hint) -- bit for bit against the plain routes."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _events(sizes, k, dev, seed):
    from deepmetv2_amd import _native
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(sum(sizes), 32, generator=g).to(dev)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(sizes).cumsum(0)]).to(dev)
    nbr, _, loc = _native.knn_local(x, ptr, k)
    return x, ptr, nbr, loc, g


def _same(a, b):
    return torch.equal(a[0], b[0]) and (a[1] is None) == (b[1] is None) and (a[1] is None or torch.equal(a[1], b[1]))


def test_mixed_form_matches_l2_form(dev, monkeypatch):
    """5200 nodes do not fit the 5119-row image, so both launches of the mixed form do work; the empty event covers the
    skip logic of both."""
    from deepmetv2_amd import _native
    monkeypatch.setattr(_native, "GATHER_MAX_FORM", "auto")     # gather_max offers the mixed form under its default only
    x, ptr, nbr, loc, g = _events([300, 0, 5200, 77], 16, dev, seed=31)
    P = torch.randn(x.shape[0], 32, generator=g).to(dev)
    Q = torch.randn(x.shape[0], 32, generator=g).to(dev)
    for want_arg in (True, False):
        ref = _native.gather_max(P, Q, nbr, ptr, want_arg, lds=False)
        assert "gather_max_mlp_kernel (row gathers from L2" in _native.last_gather_kernel
        for nl in (loc, None):
            got = _native.gather_max(P, Q, nbr, ptr, want_arg, nbr_local=nl, mixed=True)
            assert "chosen per event" in _native.last_gather_kernel
            assert _same(got, ref)


@pytest.mark.parametrize("k", [8, 20])
def test_half_image_form_matches_full_image(dev, monkeypatch, k):
    """2559 nodes + the -inf row are exactly the 2560 rows of the half image; a hint that is too small (500) sends the
    larger events through the kernel's own L2 path: slower, never wrong.  The hinted calls must give the bits of the call
    without a hint, of the same calls with the half image switched off (DMET_GATHER_HALF_IMAGE=0, read per call: with the
    switch at its default the hinted calls are the half-image form) and of the L2 kernels on the row-major tables."""
    from deepmetv2_amd import _native
    monkeypatch.setattr(_native, "GATHER_MAX_FORM", "auto")     # slice-major tables are refused under l2-only
    monkeypatch.delenv("DMET_GATHER_HALF_IMAGE", raising=False)
    x, ptr, nbr, loc, g = _events([2559, 1, 0, 900], k, dev, seed=41 + k)
    W = (torch.randn(32, 64, generator=g) * 0.2).to(dev)
    Pr, Qr = _native.node_linear_split(x, W, None)
    P, Q = _native.node_linear_split(x, W, None, sliced=True)

    def sliced(want_arg, hint):
        return _native.gather_max(P, Q, nbr, ptr, want_arg, lds=True, nbr_local=loc, sliced=True, max_nodes=hint)

    for want_arg in (True, False):
        l2 = _native.gather_max(Pr, Qr, nbr, ptr, want_arg, lds=False)
        assert "from L2" in _native.last_gather_kernel
        assert _same(sliced(want_arg, None), l2)
        half = {hint: sliced(want_arg, hint) for hint in (2559, 500)}
        monkeypatch.setenv("DMET_GATHER_HALF_IMAGE", "0")
        full = {hint: sliced(want_arg, hint) for hint in (2559, 500)}
        monkeypatch.delenv("DMET_GATHER_HALF_IMAGE")
        for hint in (2559, 500):
            assert _same(half[hint], l2) and _same(full[hint], l2)
