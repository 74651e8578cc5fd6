"""The GINE drug encoder at hidden and output widths 16, 32 and 64 (csrc/gine_quad_tile.h: GineShapesShipped +
GineShapesWide, 15 layer shapes (cin, c, c); quad::src_sum rows of 32 / 64; models/molecule_gnn.py).

Checker: oracle/gvp_oracle.py::molecule_gine_forward / gine_conv (PyG's published GINEConv / MLP formulas restated,
width-generic) with autograd on the CPU, compared the way tests/test_gine_depth4.py::_compare does, at the project's drug
bars: output rel_err < 2e-5, every gradient < 2e-4 of the tensor's own maximum (DRUG_FWD_TOL, DRUG_GRAD_TOL).

ONE small batch serves every case: drugs of 1, 2, 15, 16, 17 and 33 atoms (tile edges of the 16-atom tile, a one-atom
graph) and a hand-built graph of 120 atoms holding an atom with 70 + 1 incoming edges (its tile needs two 64-edge
chunks), an atom with no incoming edge at all and an atom whose only edge is its self loop: 204 atoms, 13 tiles.
Before the widths were compiled every GPU case here ended in the unsupported-dims error."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import davis_synth as ds
from conftest import GOLDEN, REPO, rel_err
from oracle import gvp_oracle as O

DEV = "cuda:0"
DRUG_FWD_TOL, DRUG_GRAD_TOL = 2e-5, 2e-4            # test_gine_depth4.py::_compare, test_gine_edge_grad.py
P_DROP = 0.2
SIZES = (1, 2, 15, 16, 17, 33)
HUB_N, HUB_IN = 120, 70                             # the hand-built graph: atoms, edges into its atom 0 (+ the self loop)
WIDTHS = (16, 32, 64)
STACKS3 = [(h, o) for h in WIDTHS for o in WIDTHS]  # 52 -> h -> h -> o: every first, middle and last layer shape
# every supported width list a test below runs (the CPU workspace test walks them)
WIDTH_LISTS = ([[52, h, h, o] for h, o in STACKS3] + [[52, 32, 32], [52, 64, 64], [52, 32], [52, 64, 64, 64]])


# ------------------------------------------------------------------------------------------------ the batch
def _hub_graph(rng):
    """drug_graph's atoms and bonds with: atom 0 the target of an edge from each of atoms 3 .. 3 + HUB_IN - 1 (bond
    features made the way davis_synth makes its own), atom 1 without any incoming edge (self loop included), atom 2
    with its self loop only; the edge list shuffled."""
    g = ds.drug_graph(rng, n_atoms=HUB_N)
    ei, e_s, et = g["edge_index"], g["e_s"], g["etypes"]
    keep = ~((ei[1] == 1) | ((ei[1] == 2) & (ei[0] != 2)) | ((ei[1] == 0) & (ei[0] != 0)))
    ei, e_s, et = ei[:, keep], e_s[keep], et[keep]
    src = np.arange(3, 3 + HUB_IN)
    feat = np.zeros((HUB_IN, 9), np.float32)
    feat[np.arange(HUB_IN), rng.integers(0, 7, size=HUB_IN)] = 1.0
    feat[:, 7:] = rng.integers(0, 2, size=(HUB_IN, 2))
    ei = np.concatenate([ei, np.stack([src, np.zeros_like(src)])], 1)
    e_s, et = np.concatenate([e_s, feat]), np.concatenate([et, rng.integers(1, 5, size=HUB_IN)])
    perm = rng.permutation(ei.shape[1])
    return dict(g, edge_index=np.ascontiguousarray(ei[:, perm]), e_s=e_s[perm], etypes=et[perm].astype(np.int64))


_BATCH = []


def _batch():
    """-> (the batch's tensors on the CPU, index of the hub graph's atom 0)"""
    if not _BATCH:
        rng = np.random.default_rng(20261)
        graphs = [ds.drug_graph(rng, n_atoms=n) for n in SIZES] + [_hub_graph(rng)]
        gb = ds.collate(graphs)
        _BATCH.append((ds.to_torch(gb), int(gb.ptr[len(SIZES)])))
    return _BATCH[0]


def test_the_batch_is_what_the_cases_need():
    d, h0 = _batch()
    N, ei = d["x"].shape[0], d["edge_index"].numpy()
    deg = np.bincount(ei[1], minlength=N)
    assert N == sum(SIZES) + HUB_N == 204 and N % 16 == 12 and d["eattr"].shape[1] == 9
    assert deg[h0] == HUB_IN + 1 >= 65 and deg[h0 + 1] == 0                 # two chunks for the hub's tile; no edge at all
    assert deg[h0 + 2] == 1 and ((ei[1] == h0 + 2) & (ei[0] == h0 + 2)).sum() == 1      # the self loop alone
    assert (ei[0] == h0 + 1).sum() >= 1                                     # ... but atom 1 still sends messages
    assert (np.diff(ei[1]) < 0).any()                                       # not sorted by target


# ------------------------------------------------------------------------------------------------ model, GPU pass, oracle
def _model(hidden, out, num_convs=3, seed=0, **kw):
    from models.molecule_gnn import SelectableMoleculeModelWrapper
    base = json.load(open(os.path.join(GOLDEN, "model_kwargs.json")))["molecule_gnn_kwargs"]
    torch.manual_seed(1000 + 100 * seed + hidden + out // 16)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")             # (num_convs = 1 warns that hidden_channels is unused, as the reference does)
        m = SelectableMoleculeModelWrapper(**dict(base, num_convs=num_convs, hidden_channels=hidden, out_channels=out,
                                                  dropout_rate=P_DROP, **kw))
    with torch.no_grad():                           # eps = 0 at initialisation would leave d/d eps untested as a multiplier
        for l, conv in enumerate(m.gnn_model.conv_list):
            conv.eps.fill_(0.05 * (l + 1))
    assert m.gnn_model._widths == [52] + [hidden] * (num_convs - 1) + [out]
    return m


def _upstream(n, width, seed=1):
    return torch.randn(n, width, generator=torch.Generator().manual_seed(seed))


def _grads(model):
    g = model.gnn_model
    if getattr(g, "_fused", False):
        return {k: v for k, v in g._leaf.views(g.arena.grad)}
    return {k: p.grad for k, p in g.named_parameters()}


def _gpu_pass(model, d, r):
    """forward + backward on the GPU -> dict(out, gx, ge, grads, masks of the training pass or None)"""
    from gvp_hip import autograd_ops, ops
    model.zero_grad(set_to_none=True)
    gx, ge = d["x"].to(DEV).requires_grad_(), d["eattr"].to(DEV).requires_grad_()
    out = model(gx, d["edge_index"].to(DEV), d["ntypes"].to(DEV), d["etypes"].to(DEV), eattr=ge)
    masks = None
    if model.training:                              # {seed, offset} of this pass: read before anything else runs
        sd = autograd_ops.last_seed("gine")
        masks = [ops.dropout_masks(sd, P_DROP, l, 1, gx.shape[0], w)[0].cpu()
                 for l, w in enumerate(model.gnn_model._widths[1:-1])]
    (out * r.to(DEV)).sum().backward()
    return dict(out=out.detach().cpu(), gx=gx.grad.cpu(), ge=ge.grad.cpu(),
                grads={k: v.detach().cpu() for k, v in _grads(model).items()}, masks=masks)


def _oracle(state, d, r, num_convs, masks=None, dtype=torch.float32):
    P = {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in state.items()}
    x, e = d["x"].to(dtype).clone().requires_grad_(), d["eattr"].to(dtype).clone().requires_grad_()
    ref = O.molecule_gine_forward(P, x, d["edge_index"], d["ntypes"], d["etypes"], e, num_convs=num_convs,
                                  masks=None if masks is None else [m.to(dtype) for m in masks])
    (ref * r.to(dtype)).sum().backward()
    return dict(out=ref.detach(), gx=x.grad, ge=e.grad, grads={k: v.grad for k, v in P.items()})


def _assert_matches(got, ref, what):
    figs = {"out": rel_err(got["out"], ref["out"]), "d x": rel_err(got["gx"], ref["gx"]),
            "d eattr": rel_err(got["ge"], ref["ge"])}
    assert set(got["grads"]) == set(ref["grads"]), what
    for k in ref["grads"]:
        assert got["grads"][k] is not None, (what, k)
        figs[k] = rel_err(got["grads"][k], ref["grads"][k])
    print(what, {k: f"{v:.1e}" for k, v in figs.items()})
    assert figs.pop("out") < DRUG_FWD_TOL, what
    bad = {k: v for k, v in figs.items() if not v < DRUG_GRAD_TOL}
    assert not bad, (what, bad)


def _state(model):
    return {k: v.detach().cpu().clone() for k, v in model.gnn_model.state_dict().items()}


# ------------------------------------------------------------------------------------------------ GPU: all 15 shapes
@pytest.mark.gpu
@pytest.mark.parametrize("hidden,out,route", [(h, o, "bridge") for h, o in STACKS3] + [(32, 64, "ops"), (64, 32, "fused")])
def test_every_layer_shape_forward_and_all_gradients(monkeypatch, hidden, out, route):
    """52 -> h -> h -> o, eval mode: output, the 21 weight gradients, d x and d eattr.  route: the C++ eager bridge; the
    torch.library ops (what CGVP_BRIDGE=0 and torch.compile run: the bridge taken away); fuse_parameters() (one leaf)."""
    from gvp_hip import autograd_ops
    d, _ = _batch()
    model = _model(hidden, out)
    state = _state(model)
    model = model.to(DEV).eval()
    if route == "ops":
        monkeypatch.setattr(autograd_ops, "_eager_bridge", lambda: None)
    if route == "fused":
        model.gnn_model.fuse_parameters()
        assert [n for n, _ in model.gnn_model.named_parameters()] == ["arena"]
    r = _upstream(d["x"].shape[0], out)
    got = _gpu_pass(model, d, r)
    assert got["out"].shape == (d["x"].shape[0], out) and len(got["grads"]) == 21
    _assert_matches(got, _oracle(state, d, r, 3), (hidden, out, route))


@pytest.mark.gpu
@pytest.mark.parametrize("hidden", [32, 64])
def test_embedding_atom_types_first_layer_without_type_columns(hidden):
    """nn.Embedding atom types of width 11 (nt = 0: the first layer runs as a plain 52-wide layer), 2 layers; every
    gradient incl. the table's."""
    d, _ = _batch()
    model = _model(hidden, hidden, num_convs=2, ntype_emb_dim=11)
    state = _state(model)
    assert "ntype_embedding.weight" in state
    model = model.to(DEV).eval()
    r = _upstream(d["x"].shape[0], hidden)
    got = _gpu_pass(model, d, r)
    assert len(got["grads"]) == 15 and float(got["grads"]["ntype_embedding.weight"].abs().max()) > 0
    _assert_matches(got, _oracle(state, d, r, 2), ("embedding", hidden))


@pytest.mark.gpu
def test_single_conv_with_out_channels_32():
    d, _ = _batch()
    model = _model(16, 32, num_convs=1)
    state = _state(model)
    model = model.to(DEV).eval()
    r = _upstream(d["x"].shape[0], 32)
    _assert_matches(_gpu_pass(model, d, r), _oracle(state, d, r, 1), "52 -> 32")


@pytest.mark.gpu
@pytest.mark.parametrize("hidden", [32, 64])
def test_training_step_with_in_kernel_dropout(hidden):
    """Training mode, 3 layers: the two inter-layer dropouts are drawn inside the forward kernels and regenerated inside
    the backward kernels; the oracle runs with the factors the kernels drew (exported as
    test_gine_depth4.py::test_gine44_training_step_with_in_kernel_dropout does)."""
    d, _ = _batch()
    model = _model(hidden, hidden)
    state = _state(model)
    model = model.to(DEV).train()
    r = _upstream(d["x"].shape[0], hidden, seed=2)
    got = _gpu_pass(model, d, r)
    assert len(got["masks"]) == 2 and not torch.equal(got["masks"][0], got["masks"][1])
    for m in got["masks"]:
        assert m.shape == (d["x"].shape[0], hidden)
        assert set(np.unique(m.numpy()).round(4)) <= {0.0, 1.25} and 0.1 < float((m == 0).float().mean()) < 0.3
    ref = _oracle(state, d, r, 3, masks=got["masks"])
    _assert_matches(got, ref, ("train", hidden))
    with torch.no_grad():
        ev = model.eval()(d["x"].to(DEV), d["edge_index"].to(DEV), d["ntypes"].to(DEV), d["etypes"].to(DEV),
                          eattr=d["eattr"].to(DEV))
    assert rel_err(ev, ref["out"]) > 1e-2                   # dropout really was applied


class _Deterministic:
    def __enter__(self):
        self.was = torch.are_deterministic_algorithms_enabled()
        torch.use_deterministic_algorithms(True)

    def __exit__(self, *a):
        torch.use_deterministic_algorithms(self.was)


@pytest.mark.gpu
@pytest.mark.parametrize("c", [32, 64])
def test_deterministic_mode(c):
    """h = o = c under torch.use_deterministic_algorithms: two backward passes bitwise equal (d x through quad::src_sum
    rows of width c), within 1e-5 relative L2 of the default mode with the global-scale floor of
    tests/test_deterministic.py::_assert_default_close, and at the oracle bars."""
    d, _ = _batch()
    model = _model(c, c)
    state = _state(model)
    model = model.to(DEV).eval()
    r = _upstream(d["x"].shape[0], c)
    with _Deterministic():
        runs = [_gpu_pass(model, d, r) for _ in range(2)]
    flat = lambda g: dict(g["grads"], **{"in.x": g["gx"], "in.eattr": g["ge"]})
    a, b = flat(runs[0]), flat(runs[1])
    assert torch.equal(runs[0]["out"], runs[1]["out"])
    for k in a:
        assert torch.equal(a[k], b[k]), k
    default = _gpu_pass(model, d, r)
    gd = flat(default)
    assert torch.equal(default["out"], runs[0]["out"])      # the forward is the same launches either way
    scale = max(float(v.abs().max()) for k, v in gd.items() if not k.startswith("in."))
    for k in a:
        err = float((a[k] - gd[k]).double().norm()) / (float(gd[k].double().norm()) + 1e-6 * scale)
        assert err < 1e-5, (k, err)
    _assert_matches(runs[0], _oracle(state, d, r, 3), ("deterministic", c))


# ------------------------------------------------------------------------------------------------ GPU: fine-grained entry points
SENT = 12345.5


def _guarded(n, dev=DEV):
    """n floats between two sentinel blocks of 64: (the whole buffer, the view to hand out)"""
    buf = torch.full((n + 128,), SENT, dtype=torch.float32, device=dev)
    return buf, buf[64:64 + n]


def _intact(buf, n):
    return bool((buf[:64] == SENT).all()) and bool((buf[64 + n:] == SENT).all())


@pytest.mark.gpu
@pytest.mark.parametrize("cin,nt", [(52, 11), (64, 0)])
def test_recompute_path_of_the_fine_grained_entry_points(cin, nt):
    """cgvp_gine_conv_fwd + cgvp_gine_conv_bwd on their own at (52,64,64) and (64,64,64): no forward workspace, so the
    backward recomputes its aggregates (the !SAVED instantiations, occupancy 1 with AGPRs).  One-layer oracle evaluation;
    the workspace is cgvp_gine_bwd_workspace_floats() floats, sentinels stand behind it and around every output."""
    from gvp_hip import _lib, ops
    L = _lib.lib()
    d, _ = _batch()
    N, E, c = d["x"].shape[0], d["edge_index"].shape[1], 64
    gen = torch.Generator().manual_seed(64 + cin)
    x = d["x"] if nt else torch.randn(N, cin, generator=gen)
    lin = lambda o, i: (torch.randn(o, i, generator=gen) / i ** 0.5, 0.1 * torch.randn(o, generator=gen))
    (we, be), (w0, b0), (w1, b1) = lin(cin, 14), lin(c, cin), lin(c, c)
    P = {"eps": torch.tensor([0.07]), "lin.weight": we, "lin.bias": be, "nn.lins.0.weight": w0, "nn.lins.0.bias": b0,
         "nn.lins.1.weight": w1, "nn.lins.1.bias": b1}
    r = _upstream(N, c, seed=3)
    # oracle: one GINEConv + activation
    Pr = {k: v.clone().requires_grad_() for k, v in P.items()}
    xr = x.clone().requires_grad_()
    xin = torch.cat([torch.nn.functional.one_hot(d["ntypes"], 11).float(), xr], -1) if nt else xr
    ea = torch.cat([torch.nn.functional.one_hot(d["etypes"], 5).float(), d["eattr"]], -1)
    ref = O._act("leaky_relu")(O.gine_conv(Pr, "", xin, d["edge_index"], ea))
    (ref * r).sum().backward()
    # GPU
    csr = ops.build_csr(d["edge_index"].to(DEV), N)
    w = {k: P[n].to(DEV).contiguous() for k, n in (("eps", "eps"), ("we", "lin.weight"), ("be", "lin.bias"),
                                                   ("w0", "nn.lins.0.weight"), ("b0", "nn.lins.0.bias"),
                                                   ("w1", "nn.lins.1.weight"), ("b1", "nn.lins.1.bias"))}
    gw = _lib.GineW(**{k: v.data_ptr() for k, v in w.items()})
    xd, ead, etd = x.to(DEV).contiguous(), d["eattr"].to(DEV).contiguous(), d["etypes"].to(DEV)
    ntd = d["ntypes"].to(DEV) if nt else None
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    tables = (p(csr.rowptr), p(csr.eperm), p(csr.esrc), p(csr.edst))
    out_buf, out = _guarded(N * c)
    rc = L.cgvp_gine_conv_fwd(p(xd), p(ntd), nt, p(ead), p(etd), 5, 9, *tables, N, E, cin, c, c, C.byref(gw), 0.01, None,
                              None, 0, p(out), st)
    assert rc == 0
    nws = int(L.cgvp_gine_bwd_workspace_floats())
    n_layer = 1 + c * cin + c + c * c + c + cin * 14 + cin
    assert nws >= 256 * n_layer                            # 256 slab rows of the largest compiled layer, which this is
    ws_buf, ws = _guarded(nws)
    gx_buf, gx = _guarded(N * (cin - nt))
    gl_buf, gl = _guarded(n_layer)
    gl.zero_()                                             # the fine-grained reduce ADDS into grad_layer
    g_out = r.to(DEV).contiguous()
    rc = L.cgvp_gine_conv_bwd(p(xd), p(ntd), nt, p(ead), p(etd), 5, 9, *tables, N, E, cin, c, c, C.byref(gw), 0.01, None,
                              None, p(g_out), p(gx), p(gl), p(ws), 256, st)
    assert rc == 0
    torch.cuda.synchronize()
    assert _intact(out_buf, N * c) and _intact(ws_buf, nws) and _intact(gx_buf, N * (cin - nt)) and _intact(gl_buf, n_layer)
    assert rel_err(out.view(N, c), ref) < DRUG_FWD_TOL
    assert rel_err(gx.view(N, cin - nt), xr.grad) < DRUG_GRAD_TOL
    off = 0
    for k in ("eps", "nn.lins.0.weight", "nn.lins.0.bias", "nn.lins.1.weight", "nn.lins.1.bias", "lin.weight", "lin.bias"):
        n = P[k].numel()
        assert rel_err(gl[off:off + n].view(P[k].shape), Pr[k].grad) < DRUG_GRAD_TOL, k
        off += n
    assert off == n_layer


# ------------------------------------------------------------------------------------------------ GPU: multi-trip loops
def _child_main(out_path):
    """Runs in the child (CGVP_GINE_FWD_WGS=1 is read once per process): 52 -> 64 -> 64 -> 64 with ONE workgroup per
    launch -- 8 forward waves and 2 backward waves walk the 13 tiles."""
    from gvp_hip import autograd_ops
    assert os.environ.get("CGVP_GINE_FWD_WGS") == "1"
    autograd_ops.GINE_BWD_WORKGROUPS = 1
    d, _ = _batch()
    model = _model(64, 64)
    res = {"state." + k: v.numpy() for k, v in _state(model).items()}
    got = _gpu_pass(model.to(DEV).eval(), d, _upstream(d["x"].shape[0], 64))
    torch.cuda.synchronize()
    res.update(out=got["out"].numpy(), gx=got["gx"].numpy(), ge=got["ge"].numpy())
    res.update({"g." + k: v.numpy() for k, v in got["grads"].items()})
    np.savez(out_path, **res)


_CHILD = r"""
import os, sys
sys.path.insert(0, {pkg!r}); sys.path.insert(0, {repo!r}); sys.path.insert(0, os.path.join({repo!r}, "tests"))
import test_gine_widths as W
W._child_main(sys.argv[1])
print("ok")
"""


@pytest.mark.gpu
def test_multi_trip_loops_at_two_waves_per_workgroup(tmp_path):
    """(52,64,64) and (64,64,64) have 2 waves per backward workgroup: with one workgroup each wave walks 6 or 7 tiles
    (the read-add-write into an already filled AccPriv block at MH = MO = 4), and the forward's 8 waves a second one."""
    d, _ = _batch()
    tiles = -(-d["x"].shape[0] // 16)
    assert tiles == 13 and -(-tiles // 2) == 7 and -(-tiles // 8) == 2
    out = tmp_path / "multi_trip.npz"
    env = dict(os.environ, CGVP_GINE_FWD_WGS="1")
    code = _CHILD.format(pkg=os.path.join(REPO, "caster-dta_amd"), repo=REPO)
    res = subprocess.run([sys.executable, "-c", code, str(out)], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip().endswith("ok"), res.stderr[-3000:]
    z = dict(np.load(out))
    T = torch.from_numpy
    state = {k[len("state."):]: T(v) for k, v in z.items() if k.startswith("state.")}
    got = dict(out=T(z["out"]), gx=T(z["gx"]), ge=T(z["ge"]), grads={k[2:]: T(v) for k, v in z.items() if k.startswith("g.")})
    _assert_matches(got, _oracle(state, d, _upstream(d["x"].shape[0], 64), 3), "multi-trip")


# ------------------------------------------------------------------------------------------------ GPU: the whole model
@pytest.mark.gpu
def test_joint_model_with_a_32_wide_drug_encoder_eager_and_captured(monkeypatch):
    """JointGNN with drug hidden_channels = out_channels = 32 and four heads: the atom side is 64 wide beside a residue
    side of 128 -- head dims 16 / 32, both on the varlen kernels.  One eager training step and one GraphedTrainStep step
    on the same batch agree in loss and in every gradient (bounds of
    tests/test_hip_models.py::test_graphed_train_step_equals_eager); no dense attention runs."""
    from gvp_hip import _lib
    from gvp_hip.graphed import GraphedTrainStep
    from models.joint_gnn import JointGNN
    import models.joint_gnn as J
    kw = json.load(open(os.path.join(GOLDEN, "model_kwargs.json")))
    torch.manual_seed(32)
    model = JointGNN(protein_gnn_kwargs=kw["protein_gnn_kwargs"],
                     molecule_gnn_kwargs=dict(kw["molecule_gnn_kwargs"], hidden_channels=32, out_channels=32),
                     **dict(kw["joint_gnn_kwargs"], n_attention_heads=4))
    model.to(DEV).eval()                                   # no dropout: the two runs see the same numbers
    assert model.molecule_gnn.gnn_model._widths == [52, 32, 32]
    layer = model.cross_attn_module.cross_attn_layers[0]
    assert sorted((layer.embed1_to_2.head_dim, layer.embed2_to_1.head_dim)) == [16, 32]
    assert model.cross_attn_module.varlen_supported(torch.empty(1, 128, device=DEV))
    dense = []
    real_dense, real_mha = J.to_dense_batch, torch.nn.MultiheadAttention.forward
    monkeypatch.setattr(J, "to_dense_batch", lambda *a, **k: dense.append("to_dense_batch") or real_dense(*a, **k))
    monkeypatch.setattr(torch.nn.MultiheadAttention, "forward", lambda *a, **k: dense.append("mha") or real_mha(*a, **k))
    to = lambda d: {k: (tuple(t.to(DEV) for t in v) if isinstance(v, tuple) else v.to(DEV)) for k, v in d.items()}
    pb, mb = ds.pair_batch(4, 1, lengths=[60, 45, 80, 33])
    pd, md = to(ds.to_torch(pb)), to(ds.to_torch(mb))
    pd["ptr"], md["ptr"] = torch.as_tensor(pb.ptr).to(DEV), torch.as_tensor(mb.ptr).to(DEV)
    target = torch.randn(4, 1, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    params = [q for q in model.parameters() if q.numel()]
    pred, _ = model(pd, md)
    loss = torch.nn.functional.mse_loss(pred, target)
    ref = [g.clone() for g in torch.autograd.grad(loss, params)]
    pred, loss = pred.detach().clone(), loss.detach().clone()
    model.zero_grad(set_to_none=True)
    assert np.isfinite(float(loss)) and all(bool(torch.isfinite(g).all()) for g in ref)
    if _lib.bridge() is None:              # (CGVP_BRIDGE=0 runs of the suite) the capture-safety check lives in the bridge
        with pytest.raises(RuntimeError, match="bridge"):
            GraphedTrainStep(model, torch.nn.functional.mse_loss)
        assert not dense
        return
    runner = GraphedTrainStep(model, torch.nn.functional.mse_loss)
    gl, gp = runner.run(pd, md, target)
    torch.cuda.synchronize()
    assert not dense, dense
    assert float((gl - loss).abs()) <= 1e-5 * float(loss.abs())
    assert float((gp - pred).abs().max()) <= 1e-5 * float(pred.abs().max())
    scale = max(float(g.abs().max()) for g in ref)
    for q, g in zip(params, ref):
        assert q.grad is not None
        assert float((q.grad - g).abs().max()) <= 2e-5 * float(g.abs().max()) + 2e-7 * scale


# ------------------------------------------------------------------------------------------------ still refused
@pytest.mark.gpu
@pytest.mark.parametrize("hidden,out", [(48, 64), (8, 64), (128, 64), (16, 128)])
def test_other_widths_raise_at_the_first_forward(hidden, out):
    """The model names the supported set; the C pass refuses the configuration before its first launch: the output, the
    workspace and the CSR counters are as they were."""
    from gvp_hip import _lib, autograd_ops, ops
    d, _ = _batch()
    dd = {k: v.to(DEV) for k, v in d.items()}
    model = _model(hidden, out).to(DEV)
    for mode in (model.train(), model.eval()):
        with pytest.raises(NotImplementedError, match=r"\(16, 32, 64\)"):
            mode(dd["x"], dd["edge_index"], dd["ntypes"], dd["etypes"], eattr=dd["eattr"])
    # the C call of a training pass
    L = _lib.lib()
    widths = [52, hidden, hidden, out]
    N, E = d["x"].shape[0], d["edge_index"].shape[1]
    cfg = autograd_ops._gine_cfg(widths, 11, 5, 9, 0.01)
    params = autograd_ops.gine_params(model.gnn_model)
    warr, keep = autograd_ops._gine_weights(params, 3)
    nbytes = autograd_ops.gine_fwd_ws_bytes(N, E, widths, True)
    ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=DEV)
    out_buf, o = _guarded(N * out)
    o.fill_(SENT)
    batch = autograd_ops._batch(_lib.GineBatch, (dd["x"], dd["ntypes"]), (dd["eattr"], dd["etypes"]), dd["edge_index"], [], N, E)
    counters = ops.csr_counters(torch.device(DEV), N)
    before = counters.clone()
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = L.cgvp_gine_forward_pass(C.byref(cfg), warr, C.byref(batch), 0.0, None, None, p(counters), p(ws), 1, 0, p(o),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == -2                                          # CGVP_ERR_UNSUPPORTED_DIMS
    assert bool((out_buf == SENT).all()) and bool((ws == 0xA5).all()) and torch.equal(counters, before)


# ------------------------------------------------------------------------------------------------ CPU
def test_workspace_formula_matches_the_library_for_every_width_list():
    from gvp_hip import _lib, autograd_ops
    for widths in WIDTH_LISTS:
        cfg = autograd_ops._gine_cfg(widths, 11, 5, 9, 0.01)
        for N, E in ((0, 0), (1, 0), (204, 700), (2560, 8200)):
            for save in (True, False):
                w = _lib.GineFwdWs()
                assert _lib.lib().cgvp_gine_fwd_workspace(C.byref(cfg), N, E, 1 if save else 0, C.byref(w)) == 0
                assert autograd_ops.gine_fwd_ws_bytes(N, E, widths, save) == int(w.total), (widths, N, E, save)
                assert autograd_ops.gine_fwd_ws_bytes(N, E, widths, save, True) == int(w.saved), (widths, N, E, save)


def test_backward_workspace_covers_the_largest_compiled_layer():
    """cgvp_gine_bwd_workspace_floats(): 256 slab rows of the (64,64,64) layer; the passes size their slabs by the
    configuration: the shipped stacks keep their bytes, a 64-wide stack gets rows of its own length."""
    from gvp_hip import _lib, autograd_ops
    L = _lib.lib()
    floats = lambda cin, c: 1 + c * cin + c + c * c + c + cin * 14 + cin
    assert int(L.cgvp_gine_bwd_workspace_floats()) == 256 * floats(64, 64) == 256 * max(
        floats(cin, c) for cin in (16, 32, 52, 64) for c in WIDTHS)
    up = lambda v: (v + 255) // 256 * 256
    for widths, row in (([52, 16, 64], floats(16, 64)), ([52, 16, 16, 16, 64], floats(16, 64)), ([52, 16, 16], floats(16, 64)),
                        ([52, 64, 64, 64], floats(64, 64)), ([52, 64], floats(52, 64))):
        cfg = autograd_ops._gine_cfg(widths, 11, 5, 9, 0.01)
        nl, N = len(widths) - 1, 300
        want = up(nl * 256 * row * 4) + (nl - 1) * up(N * max([0] + widths[1:-1]) * 4)
        assert int(L.cgvp_gine_bwd_workspace_bytes(C.byref(cfg), N, 900)) == want or _lib.DETERMINISTIC_ENV, widths


@pytest.mark.parametrize("widths", [[52, 32, 32, 64], [52, 64, 64, 16], [52, 32]])
def test_fake_kernels_give_the_real_shapes(widths):
    from torch._subclasses.fake_tensor import FakeTensorMode
    from gvp_hip import autograd_ops
    nl, N, E = len(widths) - 1, 204, 700
    n_par = sum(1 + c * a + c + c * c + c + a * 14 + a for a, c in zip(widths[:-1], widths[1:]))
    with FakeTensorMode():
        f = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device="cuda")
        args = ([f(n_par)], f(N, 41), f(N, dt=torch.long), f(E, 9), f(E, dt=torch.long), f(2, E, dt=torch.long), [])
        out, ws, masks = torch.ops.caster_gvp.gine_encoder(*args, widths, 11, 5, 0.01, 0.2, True)
        assert out.shape == (N, widths[-1]) and out.dtype == torch.float32 and len(masks) == nl - 1
        assert ws.shape == (autograd_ops.gine_fwd_ws_bytes(N, E, widths, True, saved_only=True),) and ws.dtype == torch.uint8
        out0, ws0, masks0 = torch.ops.caster_gvp.gine_encoder(*args, widths, 11, 5, 0.01, 0.0, False)
        assert out0.shape == (N, widths[-1]) and ws0.numel() == 0 and masks0 == []
        g = torch.ops.caster_gvp.gine_encoder_backward(out, *args, ws, masks, widths, 11, 5, 0.01, 0.2, True, 0)
        assert [tuple(t.shape) for t in g] == [(n_par,), (N, 41)]
        g = torch.ops.caster_gvp.gine_encoder_backward_eattr(out, *args, ws, masks, widths, 11, 5, 0.01, 0.2, True, True, 24)
        assert [tuple(t.shape) for t in g] == [(n_par,), (N, 41), (E, 9)]


def test_the_model_names_the_supported_set_without_a_gpu():
    """The width check comes before the device check: the message names the set on any machine."""
    from models import molecule_gnn
    assert molecule_gnn.GINE_WIDTHS == WIDTHS and "16, 32 or 64" in molecule_gnn.HomoMoleculeGNN_GINE.__doc__
    d, _ = _batch()
    model = _model(48, 64)
    with pytest.raises(NotImplementedError, match=r"\(16, 32, 64\).*\[52, 48, 48, 64\]"):
        model(d["x"], d["edge_index"], d["ntypes"], d["etypes"], eattr=d["eattr"])
    with pytest.raises(RuntimeError, match="MI355X only"):            # a supported width goes on to the device check
        _model(32, 64)(d["x"], d["edge_index"], d["ntypes"], d["etypes"], eattr=d["eattr"])
