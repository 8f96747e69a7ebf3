"""TEST INFRASTRUCTURE for tests/test_gpu_step_models.py and tests/test_step_models_host.py: a table of models that leave
the one shape every other test of the training step runs (`Net`: hidden 32, two convolutions, every parameter trainable
and used once), each built twice -- as deepmetv2_amd.model.GraphMETNetwork behind Net's sigmoid and as
oracle.ref_model.RefGraphMETNetwork in float64 -- with the state copied across, and the float64 loss and gradients of one
step on one ragged batch.

The step defers its weight-gradient sums (deepmetv2_amd._native.finalize_defer_begin): the gradients that
edgeconv_linear_bwd, encode_bwd / encode_bn_bwd and head_bwd hand to autograd are unwritten until the flush.  That is safe
only while nothing reads, adds or frees them before the flush, and a model with a frozen parameter (autograd drops its
gradient inside the pass), a layer applied twice (autograd adds its two gradients inside the pass) or more than six
convolutions (the library's queue holds eight sums) leaves what `Net` exercises.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import torch

SIZES = [300, 37, 520]
SEED = 21
K = 16
RADIUS = 0.4
QUEUE = 8           # kDeferMax of csrc/finalize.hip

# depth, hidden: GraphMETNetwork(conv_depth, hidden_dim).  shared: conv_continuous[i] = conv_continuous[0] for every i.
# frozen: a predicate over the parameter names of the GraphMETNetwork, or None.  bn_eval: every BatchNorm1d in eval mode
# under a model in training mode, its running statistics first moved off (0, 1) by one training forward.
Case = namedtuple("Case", "depth hidden shared frozen bn_eval", defaults=(2, 32, False, None, False))

_ENCODER = ("embed_", "encode_all.", "bn_all.")


def _is_conv_bias(name: str) -> bool:
    return name.startswith("conv_continuous.") and name.endswith(".0.nn.0.bias")


CASES = {
    "depth1": Case(depth=1),
    "depth3": Case(depth=3),
    "depth6": Case(depth=6),            # head + 6 + encoder: a full queue
    "depth7": Case(depth=7),            # the encoder's sums, pushed last, find the queue full
    "depth9": Case(depth=9),            # ... and so do two convolutions before it
    "shared2": Case(depth=2, shared=True),
    "shared3": Case(depth=3, shared=True),
    "frozen_head": Case(frozen=lambda n: n.startswith("output.")),
    "frozen_encoder": Case(frozen=lambda n: n.startswith(_ENCODER)),
    "frozen_conv0": Case(frozen=lambda n: n.startswith("conv_continuous.0.0.nn.0.")),
    "frozen_conv_bias": Case(frozen=_is_conv_bias),
    "head_only": Case(frozen=lambda n: not n.startswith("output.")),
    "bn_eval": Case(bn_eval=True),
    "hidden16": Case(hidden=16),
    "hidden64": Case(hidden=64),
}
FROZEN_CASES = [n for n, c in CASES.items() if c.frozen is not None]
SHARED_CASES = [n for n, c in CASES.items() if c.shared]


def expected_pending(name: str, fused_encoder: bool = True) -> int:
    """Sums still queued when train_step reaches its flush, deferral on (DESIGN.md, K5 "Weight-gradient sums").

    In the order of the backward pass: the head queues one (fused route only), every convolution whose backward runs
    one (hidden 32 only), the encoder one (fused route only; it runs last), up to the queue's eight; a call that finds
    the queue full sums at once.  A frozen parameter changes nothing as long as its layer's backward runs (the layer's
    input or another of its parameters wants a gradient): the sums are formed into memory the deferral keeps.  Behind
    a wholly frozen front (`head_only`, `frozen_encoder`) autograd never calls the frozen layers' backward.  The second
    backward call of a shared layer forms what is queued so far and its own sums at once, and so does every further
    one: of a shared model only the encoder's sums are left for the flush."""
    c = CASES[name]
    if c.hidden != 32:
        return 0                        # layer-by-layer encoder and head, addmm weight gradients: nothing to queue
    fused = 1 if fused_encoder else 0
    if c.shared:
        return fused
    if name == "head_only":
        return fused
    convs = c.depth
    enc = 0 if name == "frozen_encoder" else fused
    return min(QUEUE, fused + convs + enc)


# ---- the two models ------------------------------------------------------------------------------------------------------
class _Sigmoid(torch.nn.Module):
    """model.Net's wiring around any GraphMETNetwork (same state_dict prefix, `graphnet.`)."""

    def __init__(self, graphnet):
        super().__init__()
        self.graphnet = graphnet

    def forward(self, x_cont, x_cat, edge_index, batch):
        return self.graphnet(x_cont, x_cat, edge_index, batch, apply_sigmoid=True)


class _RefSigmoid(torch.nn.Module):
    def __init__(self, graphnet):
        super().__init__()
        self.graphnet = graphnet

    def forward(self, x_cont, x_cat, edge_index, batch):
        return self.graphnet(x_cont, x_cat, edge_index, batch).sigmoid()


def _wire(net, case: Case):
    if case.shared:
        for i in range(1, len(net.conv_continuous)):
            net.conv_continuous[i] = net.conv_continuous[0]
    return net


def _freeze(model, case: Case) -> None:
    if case.frozen is not None:
        hit = 0
        for n, p in model.graphnet.named_parameters():
            if case.frozen(n):
                p.requires_grad_(False)
                hit += 1
        assert hit, "the case freezes nothing"


def bn_layers(model):
    return [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm1d)]


def build_model(name: str, graph: str = "static"):
    """The package's model of case `name` on the CPU, in training mode, frozen as the case says (bn_eval: see
    settle_bn_eval -- it needs a forward on the model's device)."""
    from deepmetv2_amd.model import GraphMETNetwork
    case = CASES[name]
    torch.manual_seed(SEED)
    net = GraphMETNetwork(8, 3, output_dim=1, hidden_dim=case.hidden, conv_depth=case.depth, graph=graph, k=K)
    model = _Sigmoid(_wire(net, case)).train()
    _freeze(model, case)
    return model


def build_ref(name: str, state, graph: str = "static", dtype=torch.float64):
    """The oracle's model of case `name` with the parameters and buffers of `state` (a state_dict of build_model's)."""
    from oracle.ref_model import RefGraphMETNetwork
    case = CASES[name]
    net = RefGraphMETNetwork(8, 3, 1, case.hidden, case.depth, graph=graph, k=K)
    ref = _RefSigmoid(_wire(net, case))
    ref.load_state_dict({k: v.detach().cpu() for k, v in state.items()})
    ref = ref.to(dtype).train()
    _freeze(ref, case)
    return ref


def untie(ref):
    """A copy of a shared-weight reference whose blocks own equal but separate parameters: block i's gradient is then the
    gradient of the i-th USE of the shared layer alone."""
    import copy
    out = copy.deepcopy(ref)
    blocks = out.graphnet.conv_continuous
    for i in range(1, len(blocks)):
        blocks[i] = copy.deepcopy(blocks[0])
    return out


def settle_bn_eval(model, forward) -> None:
    """bn_eval: one training forward (`forward(model)`) moves every running statistic off (0, 1), then every
    BatchNorm1d goes to eval mode under a model that stays in training mode."""
    with torch.no_grad():
        forward(model)
    for bn in bn_layers(model):
        assert float(bn.running_mean.abs().max()) > 0 and int(bn.num_batches_tracked) == 1
        bn.eval()
    assert model.training


# ---- the batch and its static graph --------------------------------------------------------------------------------------
def host_batch(seed: int = SEED):
    from deepmetv2_amd import synth
    return synth.make_events(SIZES, seed=seed)


def etaphi_of(x):
    return torch.stack([x[:, 3], torch.atan2(x[:, 1], x[:, 0])], 1)


@functools.lru_cache(maxsize=None)
def host_graph():
    """(x, y, batch, ptr, etaphi, edge_index) on the CPU: radius 0.4 in (eta, phi) with self loops, by the oracle."""
    from oracle import ref_ops
    x, y, batch, ptr = host_batch()
    etaphi = etaphi_of(x)
    ei = ref_ops.radius_graph(etaphi, RADIUS, batch, loop=True, max_num_neighbors=255)
    return x, y, batch, ptr, etaphi, ei


def ref_forward(ref, dtype=torch.float64):
    from deepmetv2_amd.model import split_features
    x, _y, batch, _ptr, _e, ei = host_graph()
    x_cont, x_cat = split_features(x)
    return ref(x_cont.to(dtype), x_cat, ei, batch)


def ref_step(ref, dtype=torch.float64):
    """(loss, {name: gradient or None}) of one forward / loss / backward of `ref` on the batch."""
    from oracle import ref_ops
    x, y, batch = host_graph()[:3]
    for p in ref.parameters():
        p.grad = None
    loss = ref_ops.loss_fn(ref_forward(ref, dtype), x.to(dtype), y.to(dtype), batch)
    loss.backward()
    return loss.detach(), {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in ref.named_parameters()}


def gscale_of(grads) -> float:
    return max(float(g.abs().max()) for g in grads.values() if g is not None)


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """(loss, grads, gscale) in float64 for case `name` from the state build_model gives it; computed once, read-only."""
    return reference_from(name, build_model(name).state_dict())


def reference_from(name: str, state, dtype=torch.float64):
    """... from any state of the case's model as build_model leaves it (bn_eval: before its training forward -- the
    reference runs its own, as the model under test does)."""
    ref = build_ref(name, state, dtype=dtype)
    if CASES[name].bn_eval:
        settle_bn_eval(ref, lambda m: ref_forward(m, dtype))
    loss, grads = ref_step(ref, dtype)
    return loss, grads, gscale_of(grads)
