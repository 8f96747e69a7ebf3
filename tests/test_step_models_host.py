"""The premises of tests/test_gpu_step_models.py, on the CPU: the float64 reference of every case of tests/step_models.py
is a reference worth comparing with (its own fp32 run sits five orders of magnitude below the differences the GPU tests
look for, no gradient is trivially zero, frozen parameters get none), and a shared layer's gradient really is a sum
whose parts are far from it -- so a step that handed autograd one part, or an unwritten one, cannot pass by rounding."""
import pytest
import torch

import step_models as sm


@pytest.mark.parametrize("name", list(sm.CASES))
def test_fp32_reference_agrees_with_float64(name):
    """The reference run in fp32 is within 1e-5 of the gradient scale of the float64 run (measured: 3.2e-7 to 9.3e-7 over
    the cases, depths 1 to 9 and the shared ones included), and within 1e-5 of the loss."""
    loss, grads, gscale = sm.reference(name)
    state = sm.build_model(name).state_dict()
    loss32, grads32, _ = sm.reference_from(name, state, dtype=torch.float32)
    worst = 0.0
    for n, g in grads.items():
        assert (g is None) == (grads32[n] is None), n
        if g is not None:
            worst = max(worst, float((grads32[n].double() - g).abs().max()) / gscale)
    print(f"{name}: fp32 against float64, worst gradient error / gscale = {worst:.3g}, gscale = {gscale:.4g}, "
          f"loss {float(loss32):.8g} against {float(loss):.8g}")
    assert worst <= 1e-5
    assert abs(float(loss32) - float(loss)) <= 1e-5 * abs(float(loss))


@pytest.mark.parametrize("name", list(sm.CASES))
def test_reference_gradients_are_there(name):
    """No trainable parameter's reference gradient is identically zero (or non-finite); a frozen one has none."""
    _loss, grads, gscale = sm.reference(name)
    assert gscale > 0
    model = sm.build_model(name)
    trainable = {n: p.requires_grad for n, p in model.named_parameters()}
    assert list(trainable) == list(grads)           # same names in the same order on both sides
    for n, g in grads.items():
        if trainable[n]:
            assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, n
        else:
            assert g is None, n
    frozen = [n for n, t in trainable.items() if not t]
    assert bool(frozen) == (name in sm.FROZEN_CASES)
    if name in sm.FROZEN_CASES:
        case = sm.CASES[name]
        assert frozen == [n for n in trainable if case.frozen(n[len("graphnet."):])]


@pytest.mark.parametrize("name", sm.SHARED_CASES)
def test_a_single_use_is_far_from_the_shared_gradient(name):
    """Each single use's weight gradient differs from the summed one by at least 0.3 of the gradient scale, the largest
    absolute gradient of the whole model (measured: 0.38 and 0.42 for the two uses of shared2, 0.62, 0.65 and 0.74 for
    the three of shared3), while the uses do add up to it."""
    _loss, grads, gscale = sm.reference(name)
    tied = sm.build_ref(name, sm.build_model(name).state_dict())
    _l, parts = sm.ref_step(sm.untie(tied))
    depth = sm.CASES[name].depth
    key = "graphnet.conv_continuous.{}.0.nn.0.weight"
    total = grads[key.format(0)]
    uses = [parts[key.format(i)] for i in range(depth)]
    assert float((sum(uses) - total).abs().max()) <= 1e-12 * gscale
    for i, g in enumerate(uses):
        away = float((g - total).abs().max()) / gscale
        print(f"{name}: use {i} alone is {away:.3g} of the gradient scale away from the sum")
        assert away >= 0.3


def test_case_table_names_what_it_says():
    c = sm.CASES
    assert sorted(v.depth for k, v in c.items() if k.startswith("depth")) == [1, 3, 6, 7, 9]
    assert [c[n].depth for n in sm.SHARED_CASES] == [2, 3]
    assert sm.FROZEN_CASES == ["frozen_head", "frozen_encoder", "frozen_conv0", "frozen_conv_bias", "head_only"]
    shared = sm.build_model("shared3").graphnet.conv_continuous
    assert all(b is shared[0] for b in shared)
    # the counts a plain model of depth d leaves for the flush: head + d + encoder, eight at the most
    assert [sm.expected_pending(f"depth{d}") for d in (1, 3, 6, 7, 9)] == [3, 5, 8, 8, 8]
    bn = sm.build_ref("bn_eval", sm.build_model("bn_eval").state_dict())
    sm.settle_bn_eval(bn, sm.ref_forward)
    assert bn.training and not any(m.training for m in sm.bn_layers(bn))
