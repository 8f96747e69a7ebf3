"""The argument checks of the EdgeConv(Linear, max) gather entries and of their LDS-scatter backward entries: all of them
run before any HIP call (no GPU needed), through one launch path each (gather_max_launch, gather_max_bwd_launch), and a
rejection names the entry that was called."""
import os
import re
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FORWARD = ["dmet_gather_max_f32", "dmet_gather_max_counted_f32", "dmet_gather_max_lds_f32", "dmet_gather_max_lds16_f32",
           "dmet_gather_max_mixed_f32", "dmet_gather_max_lds_sliced_f32", "dmet_gather_max_lds_sliced_cap_f32",
           "dmet_gather_max_counted_lds_f32", "dmet_gather_max_counted_lds_j16_f32", "dmet_gather_max_local_j16_f32"]
# the entries that promise an LDS-resident form (H must be a multiple of the 8-channel slice)
FORWARD_LDS = [n for n in FORWARD if n not in ("dmet_gather_max_f32", "dmet_gather_max_counted_f32")]
BACKWARD = ["dmet_gather_max_bwd_lds_f32", "dmet_gather_max_bwd_lds16_f32", "dmet_gather_max_bwd_lds16_cap_f32",
            "dmet_gather_max_bwd_j16_f32", "dmet_gather_max_bwd_j16_cap_f32", "dmet_gather_max_bwd_sliced_f32",
            "dmet_gather_max_bwd_j16_sliced_f32"]


@pytest.fixture(scope="module")
def lib():
    from deepmetv2_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
            pytest.skip("libdmet_hip.so not built and no hipcc here")
        build.build_hip()
    return _lib.load()


def _parameters(name):
    """The parameter names of `name` as include/dmet.h declares it."""
    text = open(os.path.join(ROOT, "include", "dmet.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    params = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
    return [re.search(r"(\w+)\s*$", p).group(1) for p in params.split(",")]


def _call(lib, name, **sizes):
    """`name` with null pointers, a null stream and zero sizes except those given (k also sets kmax)."""
    sizes.setdefault("kmax", sizes.get("k", 0))
    sizes.setdefault("stride16", (sizes["kmax"] + 7) // 8 * 8)
    return getattr(lib, name)(*[sizes.get(p) for p in _parameters(name)]), lib.dmet_last_error()


def test_the_lists_are_the_header_s(lib):
    from deepmetv2_amd import _lib
    gather = {n for n in _lib.SIGNATURES if n.startswith("dmet_gather_max_")}
    assert set(FORWARD + BACKWARD) == gather - {"dmet_gather_max_bf16q", "dmet_gather_max_bwd_f32"}
    assert len(FORWARD) == 10 and len(BACKWARD) == 7
    for name in FORWARD + BACKWARD:
        params = _parameters(name)
        assert {"N", "H"} <= set(params) and len(params) == len(_lib.SIGNATURES[name][1])


@pytest.mark.parametrize("name", FORWARD + BACKWARD)
def test_empty_problem_is_a_no_op(lib, name):
    rc, _ = _call(lib, name, N=0, B=0, k=16, H=32, max_nodes=0, pq_sliced=0)
    assert rc == 0


@pytest.mark.parametrize("name", FORWARD + BACKWARD)
def test_null_pointers_are_rejected(lib, name):
    rc, err = _call(lib, name, N=10, B=1, k=16, H=32, max_nodes=0, pq_sliced=0)
    assert rc == -22 and err.startswith(name.encode() + b":") and b"null pointer" in err


@pytest.mark.parametrize("name", FORWARD)
def test_forward_rejects_k_300(lib, name):
    rc, err = _call(lib, name, N=10, B=1, k=300, H=32, max_nodes=0, pq_sliced=0)
    assert rc == -22 and err.startswith(name.encode() + b":") and b"300" in err


@pytest.mark.parametrize("name", FORWARD_LDS)
def test_lds_family_rejects_H_12(lib, name):
    rc, err = _call(lib, name, N=10, B=1, k=16, H=12, max_nodes=0, pq_sliced=0)
    assert rc == -22 and err.startswith(name.encode() + b":")
    # the mixed entry takes the L2 form outside H = 32: it meets the null pointers first (and, given pointers, refuses
    # H = 12 as the L2 form does)
    assert (b"null pointer" if name == "dmet_gather_max_mixed_f32" else b"H=12") in err


def test_uint16_rows_need_a_stride(lib):
    """dmet_gather_max_local_j16_f32: rows of stride16 >= kmax ids, a multiple of 8 -- checked before anything else, also
    for an empty problem."""
    name = "dmet_gather_max_local_j16_f32"
    for N in (0, 10):
        for stride16 in (0, 8, 20):
            rc, err = _call(lib, name, N=N, B=1, k=16, H=32, pq_sliced=0, stride16=stride16)
            assert rc == -22 and err.startswith(name.encode() + b":") and b"stride16=%d" % stride16 in err


@pytest.mark.parametrize("name", BACKWARD)
def test_backward_rejects_H_64(lib, name):
    rc, err = _call(lib, name, N=10, B=1, k=16, H=64, max_nodes=0, pq_sliced=0)
    assert rc == -22 and err.startswith(name.encode() + b":") and b"H=64" in err
