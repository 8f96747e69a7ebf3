"""Every torch.autograd.Function of deepmetv2_amd/ held to one contract beyond its first backward: the table of
tests/autograd_contract.py (one or more cases per Function, reached through the public operator) against the seven
properties defined there -- P1 reference, P2 repeat, P3 layouts, P4 subsets, P5 double backward, P6 scaled gradients,
P7 in-place writes after forward.  One test per case and property, so that a failure names both.  Before any
property runs, the case must reach the Function it is filed under (a node of its name in the graph), so that a route's quiet
fall-back to another one cannot leave a key untested."""
import pytest
import torch

import autograd_contract as ac

pytestmark = pytest.mark.gpu

_IDS = [(name, i) for name in sorted(ac.CASES) for i in range(len(ac.CASES[name]))]
_BUILT = {}


def _case(dev, name, i):
    """One build per case: the inputs, the graph and the reference's operands are shared by the seven properties, which
    clone what they hand to the operator and leave the case unchanged."""
    if (name, i) not in _BUILT:
        with torch.no_grad():
            _BUILT[(name, i)] = ac.CASES[name][i](dev)
    return _BUILT[(name, i)]


@pytest.mark.parametrize("prop", sorted(ac.PROPERTIES))
@pytest.mark.parametrize("name,i", _IDS, ids=[f"{n}-{i}" for n, i in _IDS])
def test_contract(dev, name, i, prop):
    try:
        case = _case(dev, name, i)
        before = [t.clone() for t in case.inputs + case.g]
        res = ac.PROPERTIES[prop](case)
    except (RuntimeError, AssertionError) as e:
        if "hip error" in str(e).lower() or "illegal memory access" in str(e).lower():
            pytest.exit(f"{name}[{i}] {prop}: the device reported a fault; nothing more is started on it: {e}", returncode=3)
        raise
    if prop == "P1":
        ac.check_reaches(case, name)
    if prop == "P5":
        print(f"{name}[{i}] P5: {res}")
    for a, b in zip(case.inputs + case.g, before):
        assert torch.equal(a, b), "the property changed the case it was given"
