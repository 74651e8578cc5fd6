"""The layer that carries the kernels' gradients into a training loop: the C++ autograd bridge (csrc/torch_bridge.cpp) and
the captured training step (gvp_hip/graphed.py).  Each test pins one contract a training run relies on and that no
kernel-level comparison sees:

  A. a parameter leaf with a second producer in the same backward (an L2 term, a stock op on an encoder weight) gets the
     SUM of both gradients from a plain `loss.backward()`, with and without a gradient already in place;
  B. a backward pass that fails after an encoder's node has run leaves a graph kept with retain_graph=True intact;
  C. GraphedTrainStep refuses heads that are not row-wise (BatchNorm on batch statistics, pair parallelism) before it
     builds anything, and runs BatchNorm in eval mode like the eager step;
  D. what the staging launch is given is checked on the host: a tensor on the CPU, a wrong count or a wrong trailing
     dimension is a ValueError, never an address handed to a kernel (an interceptor on the library handle proves it);
  E. `run` replaces p.grad: nothing stale survives, nothing is accumulated.

Bounds: those of tests/test_hip_models.py -- `same()` of the leaf test (2e-5 of the wanted gradient's maximum + 1e-6 of the
step's largest gradient: the backward's float atomics differ in the last bits from run to run, analytically-zero
gradients are pure noise) and the three of test_graphed_train_step_equals_eager."""
import json
import os

import pytest
import torch

import davis_synth as ds
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
mse = torch.nn.functional.mse_loss


def _to(d, dev=DEV):
    return {k: (tuple(t.to(dev) for t in v) if isinstance(v, tuple) else v.to(dev)) for k, v in d.items()}


def _bridge():
    from gvp_hip import _lib
    bridge = _lib.bridge()
    if bridge is None:
        pytest.skip("C++ bridge not in use")
    return bridge


def _joint(pretrained=None, seed=None, **joint_kwargs):
    from models.joint_gnn import JointGNN
    kw = json.load(open(os.path.join(GOLDEN, "model_kwargs.json")))
    if seed is not None:
        torch.manual_seed(seed)
    model = JointGNN(protein_gnn_kwargs=kw["protein_gnn_kwargs"], molecule_gnn_kwargs=kw["molecule_gnn_kwargs"],
                     **dict(kw["joint_gnn_kwargs"], **joint_kwargs))
    if pretrained is not None:
        model.load_state_dict(pretrained, strict=True)
    return model.to(DEV).eval()                            # eval: no dropout, two runs see the same numbers


def _pairs(B, seed, lengths=None):
    """(pdata, mdata, target) on the device, the dicts with `ptr`"""
    p, m = ds.pair_batch(B, seed, lengths=lengths)
    pd, md = _to(ds.to_torch(p)), _to(ds.to_torch(m))
    pd["ptr"], md["ptr"] = torch.as_tensor(p.ptr).to(DEV), torch.as_tensor(m.ptr).to(DEV)
    target = torch.randn(B, 1, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
    return pd, md, target


def _eager_step(model, params, pd, md, target):
    """(loss, pred, gradients) of the eager step, detached; its autograd graph is gone when this returns (a capture
    refuses to start while one built on another stream is alive)"""
    pred, _ = model(pd, md)
    loss = mse(pred, target)
    grads = torch.autograd.grad(loss, params, allow_unused=True)
    return loss.detach().clone(), pred.detach().clone(), grads


def _assert_equals_eager(got_loss, got_pred, params, eager):
    """the three bounds of tests/test_hip_models.py::test_graphed_train_step_equals_eager"""
    loss, pred, ref = eager
    torch.cuda.synchronize()
    assert float((got_loss - loss).abs()) <= 1e-5 * float(loss.abs())
    assert float((got_pred - pred).abs().max()) <= 1e-5 * float(pred.abs().max())
    scale = max(float(g.abs().max()) for g in ref if g is not None)
    for q, g in zip(params, ref):
        if g is None:
            assert q.grad is None
            continue
        assert q.grad is not None
        assert float((q.grad - g).abs().max()) <= 2e-5 * float(g.abs().max()) + 2e-7 * scale


@pytest.fixture(scope="module")
def golden_model(pretrained):
    return _joint(pretrained)


# ===================================================================================== A. shared leaves
@pytest.fixture(scope="module")
def leaves(golden_model):
    """The model of the leaf test, its batch, and the stock-path gradients `g` of the MSE loss alone (computed once)."""
    bridge = _bridge()
    model = golden_model
    pd, md, target = _pairs(6, 21)
    named = [(n, q) for n, q in model.named_parameters() if q.numel() and n.startswith(("protein_gnn", "molecule_gnn"))]
    params = [q for _, q in named]
    was = bridge.set_exact_leaves(True)
    try:
        model.zero_grad(set_to_none=True)
        pred, _ = model(pd, md)
        mse(pred, target).backward()
        g = [q.grad.detach().clone() for q in params]
    finally:
        bridge.set_exact_leaves(was)
        model.zero_grad(set_to_none=True)
    gscale = max(float(t.abs().max()) for t in g)
    gen = torch.Generator(device=DEV).manual_seed(77)
    # the second producer's contribution is as large as the gradient itself: dropping it cannot hide inside a tolerance
    w = [torch.randn(q.shape, device=DEV, generator=gen) * gscale for q in params]
    h = [torch.randn(q.shape, device=DEV, generator=gen) * gscale for q in params]      # a gradient already in place (d)
    return dict(bridge=bridge, model=model, pd=pd, md=md, target=target, names=[n for n, _ in named], params=params, g=g,
                gscale=gscale, w=w, h=h)


@pytest.mark.parametrize("shape", ["a_every_encoder_parameter", "b_one_encoder", "c_stock_op_on_a_weight", "d_on_an_existing_grad"])
def test_leaf_with_a_second_producer_gets_both_gradients(leaves, shape):
    """LeafScatter writes p.grad itself and takes its edge to the leaf's AccumulateGrad node out of the backward.  If
    another node of the same backward feeds that accumulator, the engine waits for two gradients, sees one, and drops the
    other without an error: p.grad then holds the encoder's part only.  Expected here, analytically: g_i + w_i wherever the
    loss has the extra term (p_i * w_i).sum(), g_i elsewhere (+ the gradient already in place in d)."""
    L = leaves
    bridge, model, params, names, g, w, gscale = L["bridge"], L["model"], L["params"], L["names"], L["g"], L["w"], L["gscale"]
    protein = [n.startswith("protein_gnn") for n in names]
    k_stock = next(i for i, n in enumerate(names) if n.startswith("molecule_gnn") and params[i].dim() == 2)

    def loss_of():
        pred, _ = model(L["pd"], L["md"])
        if shape == "b_one_encoder":
            return mse(pred, L["target"]) + sum((q * wi).sum() for q, wi, pr in zip(params, w, protein) if pr)
        if shape == "c_stock_op_on_a_weight":          # one drug-encoder weight is also read by stock ops inside the model's graph
            q = params[k_stock]
            return mse(pred + 0 * q.sum(), L["target"]) + (q * w[k_stock]).sum()
        return mse(pred, L["target"]) + sum((q * wi).sum() for q, wi in zip(params, w))

    def extra(i):
        if shape == "b_one_encoder":
            return protein[i]
        if shape == "c_stock_op_on_a_weight":
            return i == k_stock
        return True
    want = [g[i] + w[i] if extra(i) else g[i] for i in range(len(params))]
    if shape == "d_on_an_existing_grad":
        want = [t + hi for t, hi in zip(want, L["h"])]
    # encoders none of whose leaves has a second producer keep the fast path
    fast = {"a_every_encoder_parameter": 0, "b_one_encoder": 1, "c_stock_op_on_a_weight": 1, "d_on_an_existing_grad": 0}[shape]

    def same(x, y):
        return float((x - y).abs().max()) <= 2e-5 * float(y.abs().max()) + 1e-6 * gscale

    def run():
        model.zero_grad(set_to_none=True)
        if shape == "d_on_an_existing_grad":
            for q, hi in zip(params, L["h"]):
                q.grad = hi.clone()
        loss_of().backward()
        return [q.grad.detach().clone() for q in params]

    was = bridge.set_exact_leaves(False)
    try:
        n0 = bridge.fast_leaf_passes()
        got = run()
        assert bridge.fast_leaf_passes() == n0 + fast
        bridge.set_exact_leaves(True)
        stock = run()
    finally:
        bridge.set_exact_leaves(was)
        model.zero_grad(set_to_none=True)
    for a, s, b, name in zip(got, stock, want, names):
        assert same(s, b), f"stock path: {name}"
        assert same(a, b), f"default path: {name}"
        assert same(a, s), f"default path against the stock path: {name}"


# ===================================================================================== B. a failed backward
class _FailsWhileArmed(torch.autograd.Function):
    armed = False

    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        if _FailsWhileArmed.armed:
            raise RuntimeError("injected failure in a node behind the encoder")
        return g


def _find_node(fn, name, seen=None):
    seen = set() if seen is None else seen
    if fn is None or fn in seen:
        return None
    seen.add(fn)
    if fn.name() == name:
        return fn
    for nxt, _ in fn.next_functions:
        hit = _find_node(nxt, name, seen)
        if hit is not None:
            return hit
    return None


def test_failed_backward_leaves_a_retained_graph_intact(protein_params):
    """The node behind the encoder (it produces x_s) raises in the first backward, after the encoder's node has written
    p.grad and taken its leaf edges out of that pass.  The engine does not run end-of-backward callbacks of a failed pass:
    the node has to put the edges back itself, or the retained graph has lost its leaves for good."""
    from models.protein_gnn import SelectableProteinModelWrapper
    bridge = _bridge()
    kw = json.load(open(os.path.join(GOLDEN, "model_kwargs.json")))["protein_gnn_kwargs"]
    kw = {k: (tuple(v) if k in ("in_channels", "edge_dim", "hidden_channels", "edge_hidden_channels") else v) for k, v in kw.items()}
    enc = SelectableProteinModelWrapper(**kw)
    enc.load_state_dict({"gnn_model." + k: v for k, v in protein_params.items()})
    enc.to(DEV).eval()
    params = [q for q in enc.parameters() if q.numel()]
    d = _to(ds.to_torch(ds.pair_batch(4, 3, lengths=[40, 55, 33, 70])[0]))
    g_out = torch.randn(d["x"][0].shape[0], 64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))

    def loss_of(x_s):
        return (enc(**dict(d, x=(x_s, d["x"][1]))) * g_out).sum()

    was = bridge.set_exact_leaves(True)
    try:
        ref = torch.autograd.grad(loss_of(d["x"][0]), params)
    finally:
        bridge.set_exact_leaves(was)
    gscale = max(float(t.abs().max()) for t in ref)

    def same(x, y):
        return float((x - y).abs().max()) <= 2e-5 * float(y.abs().max()) + 1e-6 * gscale

    was = bridge.set_exact_leaves(False)
    try:
        enc.zero_grad(set_to_none=True)
        x0 = d["x"][0].clone().requires_grad_(True)
        loss = loss_of(_FailsWhileArmed.apply(x0))
        n0 = bridge.fast_leaf_passes()
        _FailsWhileArmed.armed = True
        with pytest.raises(RuntimeError, match="injected failure"):
            loss.backward(retain_graph=True)
        _FailsWhileArmed.armed = False
        assert bridge.fast_leaf_passes() == n0 + 1          # the encoder's node had run, on the fast path, when the pass failed
        node = _find_node(loss.grad_fn, "CasterGvpLbaEncoderBackward")
        assert node is not None
        valid = sum(fn is not None for fn, _ in node.next_functions[:len(params)])
        del node
        assert valid == len(params)                         # every leaf edge is back
        enc.zero_grad(set_to_none=True)
        for a, b in zip(torch.autograd.grad(loss, params, retain_graph=True), ref):
            assert same(a, b)
        loss.backward()
        for q, b in zip(params, ref):
            assert q.grad is not None and same(q.grad, b)
        assert x0.grad is not None
    finally:
        _FailsWhileArmed.armed = False
        bridge.set_exact_leaves(was)


# ===================================================================================== C. row-wise heads only
def _batch_norm_model():
    model = _joint(seed=5, out_lin_norm_type="batch")
    norms = [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm1d)]
    assert norms
    gen = torch.Generator(device=DEV).manual_seed(6)
    with torch.no_grad():                                   # away from (0, 1): the norm is not the identity in eval mode
        for m in norms:
            m.running_mean.add_(0.1 * torch.randn(m.running_mean.shape, device=DEV, generator=gen))
            m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, device=DEV, generator=gen))
    return model


def test_batch_norm_is_refused_in_training_mode_and_captured_in_eval_mode():
    """With out_lin_norm_type="batch" in training mode the padding pair of the captured step would enter the batch
    statistics and the warm-up passes would advance the running statistics: refused, with every buffer untouched and no
    bucket built.  In eval mode the norm uses the running statistics, row by row: the captured step equals the eager one
    at the first run of a bucket and at a replay."""
    from gvp_hip.graphed import GraphedTrainStep
    _bridge()
    model = _batch_norm_model()
    params = [q for q in model.parameters() if q.numel()]
    pd, md, target = _pairs(4, 11, lengths=[40, 55, 33, 70])
    before = {k: v.detach().clone() for k, v in model.named_buffers()}
    assert any(k.endswith("num_batches_tracked") for k in before)

    def buffers_untouched():
        now = dict(model.named_buffers())
        return now.keys() == before.keys() and all(torch.equal(now[k], before[k]) for k in before)

    model.train()
    with pytest.raises(RuntimeError, match="BatchNorm"):
        GraphedTrainStep(model, mse)
    model.eval()
    runner = GraphedTrainStep(model, mse)
    model.train()                                           # the mode changes after the construction
    with pytest.raises(RuntimeError, match="BatchNorm"):
        runner.run(pd, md, target)
    assert len(runner.buckets) == 0 and buffers_untouched()
    model.eval()
    eager = _eager_step(model, params, pd, md, target)
    model.zero_grad(set_to_none=True)
    for _ in range(2):                                      # the capture, then a replay
        loss, pred = runner.run(pd, md, target)
        _assert_equals_eager(loss, pred, params, eager)
    assert len(runner.buckets) == 1 and sum(b.steps for b in runner.buckets.values()) == 2
    assert buffers_untouched() and not model.training


def test_pair_parallel_models_are_refused_with_and_without_an_optimizer(golden_model):
    from gvp_hip.graphed import GraphedTrainStep
    from gvp_hip.optim import FusedAdam
    _bridge()
    model = golden_model
    pd, md, target = _pairs(4, 11, lengths=[40, 55, 33, 70])
    built_before = GraphedTrainStep(model, mse)
    assert model._pair_parallel is False
    model._pair_parallel = True                             # what enable_pair_parallel() sets; no process group is needed
    try:
        with pytest.raises(RuntimeError, match="enable_pair_parallel"):
            GraphedTrainStep(model, mse)
        with pytest.raises(RuntimeError, match="enable_pair_parallel"):
            GraphedTrainStep(model, mse, optimizer=FusedAdam(model.parameters(), lr=1e-4))
        with pytest.raises(RuntimeError, match="enable_pair_parallel"):
            built_before.run(pd, md, target)
        assert len(built_before.buckets) == 0
    finally:
        model._pair_parallel = False


# ===================================================================================== D. staged inputs
class _NoStaging:
    """The library handle with cgvp_stage_buffers taken out: a refusal that is missing fails the test on the host, and no
    address of a refused batch can reach the kernel."""

    def __init__(self, real):
        self._real, self.calls = real, 0

    def __getattr__(self, name):
        return getattr(self._real, name)

    def cgvp_stage_buffers(self, *args):
        self.calls += 1
        raise AssertionError("a batch that must be refused on the host reached the staging launch")


def _refused(monkeypatch, runner, cases, run):
    from gvp_hip import graphed
    proxy = _NoStaging(graphed._lib.lib())
    buckets = len(runner.buckets)
    with monkeypatch.context() as mp:
        mp.setattr(graphed._lib, "lib", lambda: proxy)
        for what, args in cases.items():
            with pytest.raises(ValueError):
                run(*args)
            assert len(runner.buckets) == buckets and proxy.calls == 0, what
    assert graphed._lib.lib() is not proxy


def test_graphed_train_step_checks_its_sources_on_the_host(golden_model, monkeypatch):
    from gvp_hip.graphed import GraphedTrainStep
    _bridge()
    model = golden_model
    params = [q for q in model.parameters() if q.numel()]
    pd, md, target = _pairs(4, 11, lengths=[40, 55, 33, 70])
    B = 4
    cpu = lambda t: t.cpu()
    longer = lambda t: torch.cat([t, t[-1:]])
    cases = {
        "target on the CPU": (pd, md, cpu(target)),
        "protein ptr on the CPU": (dict(pd, ptr=cpu(pd["ptr"])), md, target),
        "drug ptr on the CPU": (pd, dict(md, ptr=cpu(md["ptr"])), target),
        "drug features on the CPU": (pd, dict(md, x=cpu(md["x"])), target),
        "protein vector features on the CPU": (dict(pd, x=(pd["x"][0], cpu(pd["x"][1]))), md, target),
        "protein edge_index on the CPU": (dict(pd, edge_index=cpu(pd["edge_index"])), md, target),
        "drug ptr of B + 2 entries": (pd, dict(md, ptr=longer(md["ptr"])), target),
        "protein ptr of B + 2 entries": (dict(pd, ptr=longer(pd["ptr"])), md, target),
        "target of B - 1 rows": (pd, md, target[:B - 1]),
        "target of B + 1 rows": (pd, md, longer(target)),
    }
    runner = GraphedTrainStep(model, mse)
    _refused(monkeypatch, runner, cases, runner.run)
    assert len(runner.buckets) == 0
    # the same runner, a good batch: the first run of its bucket and a replay equal the eager step
    eager = _eager_step(model, params, pd, md, target)
    model.zero_grad(set_to_none=True)
    for _ in range(2):
        loss, pred = runner.run(pd, md, target)
        _assert_equals_eager(loss, pred, params, eager)
    assert len(runner.buckets) == 1
    # against the bucket that now exists: the same refusals, and features whose trailing dimensions are not the bucket's
    wider = lambda t: torch.cat([t, t[:, :1]], dim=1)
    cases.update({
        "protein scalar features one column wider": (dict(pd, x=(wider(pd["x"][0]), pd["x"][1])), md, target),
        "drug edge features one column wider": (pd, dict(md, eattr=wider(md["eattr"])), target),
        "target with a second column": (pd, md, wider(target)),
    })
    _refused(monkeypatch, runner, cases, runner.run)
    loss, pred = runner.run(pd, md, target)
    _assert_equals_eager(loss, pred, params, eager)


def test_graphed_encoder_step_checks_its_sources_on_the_host(golden_model, monkeypatch):
    from gvp_hip.graphed import GraphedEncoderStep
    model = golden_model
    pd, md, _ = _pairs(4, 11, lengths=[40, 55, 33, 70])
    pd, md = {k: v for k, v in pd.items() if k != "ptr"}, {k: v for k, v in md.items() if k != "ptr"}
    gen = torch.Generator(device=DEV).manual_seed(4)
    g_res = torch.randn(pd["x"][0].shape[0], 64, device=DEV, generator=gen)
    g_atm = torch.randn(md["x"].shape[0], 64, device=DEV, generator=gen)
    runner = GraphedEncoderStep(model.protein_gnn, model.molecule_gnn)
    cases = {
        "g_res on the CPU": (pd, md, g_res.cpu(), g_atm),
        "g_atm on the CPU": (pd, md, g_res, g_atm.cpu()),
        "g_res one row short": (pd, md, g_res[:-1], g_atm),
        "g_atm one row long": (pd, md, g_res, torch.cat([g_atm, g_atm[-1:]])),
        "g_res of another width": (pd, md, g_res[:, :32], g_atm),
        "drug node types on the CPU": (pd, dict(md, ntypes=md["ntypes"].cpu()), g_res, g_atm),
    }
    _refused(monkeypatch, runner, cases, runner.run)
    assert len(runner.buckets) == 0


# ===================================================================================== E. published gradients
def test_run_replaces_gradients_and_clears_those_of_unused_parameters(pretrained):
    from gvp_hip.graphed import GraphedTrainStep
    _bridge()
    model = _joint(pretrained)
    model.register_parameter("never_used", torch.nn.Parameter(torch.zeros(3, device=DEV)))
    params = [q for q in model.parameters() if q.numel()]
    unused = model.never_used
    pd, md, target = _pairs(4, 11, lengths=[40, 55, 33, 70])
    target2 = target.flip(0) * 1.5 + 0.25
    # an eager step leaves its gradients behind (and somebody gave the unused parameter one)
    pred, _ = model(pd, md)
    mse(pred, target2).backward()
    del pred
    unused.grad = torch.ones_like(unused)
    assert all(q.grad is not None and float(q.grad.abs().max()) > 0 for q in params)
    eager = _eager_step(model, params, pd, md, target)
    eager2 = _eager_step(model, params, pd, md, target2)
    assert [g is None for g in eager[2]] == [q is unused for q in params]
    runner = GraphedTrainStep(model, mse)
    loss, pred = runner.run(pd, md, target)
    assert unused.grad is None                              # not the stale one, which an optimizer would apply at every step
    _assert_equals_eager(loss, pred, params, eager)         # this step's gradient alone, not stale + this step's
    loss, pred = runner.run(pd, md, target2)                # the same bucket again: that step's gradient
    _assert_equals_eager(loss, pred, params, eager2)
    assert unused.grad is None and len(runner.buckets) == 1
