"""Steps over changing ragged batches on the CPU: the sequences (a) and (b) of tests/test_gpu_changing_batches.py at tiny
sizes, with deepmetv2_amd._native replaced by the oracle-backed stand-in of tests/fake_native.py (the convention of
tests/test_host_logic.py).  Every step of a run on long-lived objects must have the bits of the same step run alone
(tests/changing_batches.py): this holds the registries and the autograd wiring to the contract the GPU tests hold the
whole package to.  The side-stream future of (b) needs a device and is only in the GPU module."""
import pytest
import torch

import changing_batches as cb
from fake_native import install

CPU = torch.device("cpu")


@pytest.fixture(autouse=True)
def _fake(monkeypatch):
    from deepmetv2_amd import _native
    install(monkeypatch)
    monkeypatch.setattr(_native, "DEFER_FINALIZE", False)      # the deferral queues inside the HIP library


def test_dynamic_sequence_equals_every_step_alone():
    make = cb.net_rig(CPU, "dynamic")
    records = cb.run_sequence(make(), cb.HOST_DYNAMIC)
    assert len({tuple(r[3][1][1].reshape(-1).tolist()) for r in records[:-1]}) == len(records) - 1   # the losses do change
    cb.check_alone(make, records, "host dynamic")


@pytest.mark.parametrize("graph", ["table", "edge_index"])
def test_static_sequence_equals_every_step_alone(graph):
    make = cb.net_rig(CPU, "static")
    records = cb.run_sequence(make(), cb.with_graph(cb.HOST_STATIC, graph))
    cb.check_alone(make, records, f"host static {graph}")


def test_registries_hold_no_dead_entry_after_a_sequence():
    import gc
    make = cb.net_rig(CPU, "static")
    lengths = []
    for n in (4, 8):
        rig, stage = make(), {}
        cb.run_sequence(rig, cb.with_graph(cb.HOST_STATIC[:n], "edge_index"), stage)
        del rig
        stage.clear()
        gc.collect()
        regs = cb.registries()
        assert {name: cb.dead_entries(r) for name, r in regs.items()} == {name: [] for name in regs}
        lengths.append({name: len(r) for name, r in regs.items()})
    assert lengths[0] == lengths[1]
