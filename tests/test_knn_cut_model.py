"""tools/knn_cut_model.py, the CPU model of the second kNN filter form's sweep (no GPU): what the comment at
f2_running_tau (csrc/knn_filter.h) argues, checked on the model.  With the main sweep's masks taken against the running
cut min(tk[M-1], tk[k-1] + margin) instead of tk[M-1] alone
  * the final threshold of every query is the same number,
  * no candidate whose key is below the final threshold is removed (the certificate's premise),
  * the candidates that reach the re-rank are a subset of those that reached it before, and no query overflows that did
    not overflow before.
8 events x 512 queries each on gaussian and on 12-cluster data, 4500 nodes, k = 16."""
import importlib.util
import os

import numpy as np
import pytest

_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "knn_cut_model.py")


def _model():
    spec = importlib.util.spec_from_file_location("knn_cut_model", _PATH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("case", ["gaussian", "clustered"])
def test_running_cut_removes_only_strays(case):
    m = _model()
    fewer = 0
    for seed in range(8):
        x = m.make_event(case, 4500, seed)
        off = m.sweep(x, 512, 16, runcut=False)
        on = m.sweep(x, 512, 16, runcut=True)
        assert np.array_equal(on["tau"], off["tau"]), seed
        assert not (on["overflow"] & ~off["overflow"]).any(), seed
        live = ~on["overflow"]
        below = on["keys"] < on["tau"][:, None]
        assert not (below & ~on["kept"])[live].any(), seed
        both = live & ~off["overflow"]
        assert not (on["kept"] & ~off["kept"])[both].any(), seed
        fewer += int(off["kept"][both].sum() - on["kept"][both].sum())
    print(f"{case}: the running cut removed {fewer} stray candidates of 8 x 512 queries")
    assert fewer > 0     # the model's running cut does act at this size


def test_cut_margin_grows_with_the_kth_minimum():
    """The step of the argument that rests on f2_cut: its margin above tk[k-1] does not shrink as tk[k-1] grows by more
    than the 1 % pad covers -- over the keys and norms the sweeps see (|x|^2 from 1 to 1000, tk[k-1] + |x|^2 from 0 up)."""
    m = _model()
    for nx in (1.0, 32.0, 320.0, 1000.0):
        tkk = np.linspace(-nx, -nx + 400.0, 4001)
        margin = m.cut(tkk, nx) - tkk
        assert (margin > 0).all()
        # the margin taken at any larger tk[k-1], padded, covers the margin at every smaller one
        assert (np.minimum.accumulate((margin * 1.01)[::-1])[::-1] >= margin).all(), nx
