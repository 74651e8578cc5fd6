"""Gradients w.r.t. the raw BOND FEATURES from the drug encoder's backward (C ABI v31, cgvp_gine_backward_pass_eattr):

    d eattr[e][k] = sum_layers sum_c dm_l[e][c] * lin_l.weight[c][NET + k]

computed in the edge phase of gine_quad_bwd_kernel (one transposed MFMA chain per 16-edge tile) and returned in the
caller's edge order on every host path: the C++ eager bridge, the torch.library ops (CGVP_BRIDGE=0, torch.compile),
both backward modes, the recompute form of the kernel, and through JointGNN.

Checker: oracle/gvp_oracle.py::molecule_gine_forward on the CPU with eattr.clone().requires_grad_() -- plain torch, so
autograd gives the reference d eattr.  The drug side's parity is UNPINNED against PyG (see test_gine_depth4.py).  Bounds:
the project's gradient bar of test_gine_depth4.py::_compare (rel_err < 2e-4, forward 2e-5); the whole model takes the
bound of test_attention.py::test_joint_model_all_gradients_vs_oracle.

CPU part: the sibling custom op's schema and fake kernel, the new C symbol's host-side argument checks."""
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
TOL_OUT, TOL_G = 2e-5, 2e-4            # test_gine_depth4.py::_compare


def _to(d, dev=DEV):
    return {k: (tuple(t.to(dev) for t in v) if isinstance(v, tuple) else v.to(dev)) for k, v in d.items()}


def _mol(num_convs, seed=44, **extra):
    """The golden drug encoder (52 -> 16 -> 64) or its 4-layer form (52 -> 16 -> 16 -> 16 -> 64), seeded default
    initialisation, eps non-zero as test_gine_depth4.py::_mol44 sets it."""
    from models.molecule_gnn import SelectableMoleculeModelWrapper
    kw = json.load(open(os.path.join(GOLDEN, "model_kwargs.json")))["molecule_gnn_kwargs"]
    torch.manual_seed(seed)
    m = SelectableMoleculeModelWrapper(**dict(kw, num_convs=num_convs, **extra))
    with torch.no_grad():
        for l, conv in enumerate(m.gnn_model.conv_list):
            conv.eps.fill_(0.05 * (l + 1))
    assert m.gnn_model._widths == [52] + [16] * (num_convs - 1) + [64]
    return m.to(DEV)


def _dense_hubs():
    """> 64 incoming edges per 16-atom tile, isolated atoms, permuted edge order (eperm is not the identity): the graph
    of test_gine44_forward_and_all_gradients[dense_hubs]."""
    base = ds.to_torch(ds.drug_batch(5, 7))
    gen = torch.Generator().manual_seed(5)
    n = base["x"].shape[0] - 3
    deg = torch.randint(8, 13, (n,), generator=gen)
    deg[torch.randperm(n, generator=gen)[:4]] = 0
    dst = torch.repeat_interleave(torch.arange(n), deg)
    src = torch.randint(0, n, (int(deg.sum()),), generator=gen)
    perm = torch.randperm(dst.numel(), generator=gen)
    ei = torch.stack([src, dst])[:, perm].contiguous()
    return dict(x=base["x"][:n].clone(), ntypes=base["ntypes"][:n].clone(), edge_index=ei,
                etypes=torch.randint(0, 5, (ei.shape[1],), generator=gen),
                eattr=torch.randn(ei.shape[1], base["eattr"].shape[1], generator=gen))


def _case(name):
    if name == "ragged":
        return ds.to_torch(ds.drug_batch(7, 3))
    if name == "c5_32_drugs":
        return ds.to_torch(ds.drug_batch(32, 23))
    return _dense_hubs()


def _oracle(model, d, r, num_convs, masks=None):
    """-> (reference output, P with .grad, d x, d eattr) from oracle autograd on the CPU."""
    P = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in model.gnn_model.state_dict().items()}
    xr, er = d["x"].clone().requires_grad_(), d["eattr"].clone().requires_grad_()
    ref = O.molecule_gine_forward(P, xr, d["edge_index"], d["ntypes"], d["etypes"], er, num_convs=num_convs, masks=masks)
    (ref * r).sum().backward()
    assert er.grad.shape == d["eattr"].shape
    assert bool((er.grad.abs().amax(0) > 0).all()), "a bond-feature column without gradient: the check would be vacuous"
    return ref, P, xr.grad, er.grad


def _run(model, d, seed=1):
    """Forward + backward on the GPU with x and eattr requiring grad -> (out, gx, ge, r)."""
    dd = _to(d)
    gx, ge = dd["x"].clone().requires_grad_(), dd["eattr"].clone().requires_grad_()
    out = model(gx, dd["edge_index"], dd["ntypes"], dd["etypes"], eattr=ge)
    r = torch.randn(out.shape, generator=torch.Generator().manual_seed(seed))
    (out * r.to(DEV)).sum().backward()
    return out, gx, ge, r


def _check_all(model, d, out, gx, ge, r, num_convs, masks=None):
    ref, P, gx_ref, ge_ref = _oracle(model, d, r, num_convs, masks)
    print(f"out {rel_err(out, ref):.2e}  d eattr {rel_err(ge.grad, ge_ref):.2e}  d x {rel_err(gx.grad, gx_ref):.2e}")
    assert rel_err(out, ref) < TOL_OUT
    assert ge.grad is not None and ge.grad.shape == d["eattr"].shape and ge.grad.dtype == torch.float32
    assert rel_err(ge.grad, ge_ref) < TOL_G
    assert rel_err(gx.grad, gx_ref) < TOL_G                     # asking for d eattr disturbs nothing else
    for name, p in model.gnn_model.named_parameters():
        assert p.grad is not None, name
        assert rel_err(p.grad, P[name].grad) < TOL_G, name
    return ref


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["ragged", "c5_32_drugs", "dense_hubs"])
@pytest.mark.parametrize("num_convs", [2, 4])
def test_bond_feature_gradients_eval(num_convs, case):
    """Eval mode, 2- and 4-layer encoders: d eattr, and in the same backward d x and every parameter gradient.  The
    dense-hub graph has a permuted edge order: its rows prove the gradient lands at the ORIGINAL edge ids."""
    model = _mol(num_convs).eval()
    d = _case(case)
    if case == "dense_hubs":
        assert not torch.equal(torch.argsort(d["edge_index"][1], stable=True), torch.arange(d["edge_index"].shape[1]))
    out, gx, ge, r = _run(model, d)
    _check_all(model, d, out, gx, ge, r, num_convs)


@pytest.mark.gpu
@pytest.mark.parametrize("n_drugs,seed", [(6, 13), (32, 29)])
def test_bond_feature_gradients_training_dropout(n_drugs, seed):
    """Training mode, 4 layers: the three inter-layer dropouts drawn inside the kernels; the oracle runs with the factors
    exported through ops.dropout_masks (as test_gine44_training_step_with_in_kernel_dropout)."""
    from gvp_hip import autograd_ops, ops
    model = _mol(4).train()
    d = ds.to_torch(ds.drug_batch(n_drugs, seed))
    dd = _to(d)
    gx, ge = dd["x"].clone().requires_grad_(), dd["eattr"].clone().requires_grad_()
    out = model(gx, dd["edge_index"], dd["ntypes"], dd["etypes"], eattr=ge)
    sd = autograd_ops.last_seed("gine")
    masks = [ops.dropout_masks(sd, 0.2, l, 1, d["x"].shape[0], 16)[0].cpu() for l in range(3)]
    assert all(0.1 < float((m == 0).float().mean()) < 0.3 for m in masks)
    r = torch.randn(out.shape, generator=torch.Generator().manual_seed(2))
    (out * r.to(DEV)).sum().backward()
    _check_all(model, d, out, gx, ge, r, 4, masks=masks)


@pytest.mark.gpu
@pytest.mark.parametrize("nt_emb,et_emb", [(None, 4), (11, None), (11, 3)])
def test_bond_feature_gradients_embedding_type_encoders(nt_emb, et_emb):
    """nn.Embedding bond types: the kernels see the equivalent one-hot weight, whose feature columns are lin.weight[:, D:]
    unchanged.  nn.Embedding atom types of width 11: the first layer runs as a plain 52-wide layer (nt = 0 shape)."""
    model = _mol(2, seed=7, ntype_emb_dim=nt_emb, etype_emb_dim=et_emb).eval()
    keys = set(model.gnn_model.state_dict())
    assert ("ntype_embedding.weight" in keys) == (nt_emb is not None) and ("etype_embedding.weight" in keys) == (et_emb is not None)
    d = ds.to_torch(ds.drug_batch(9, 5))
    out, gx, ge, r = _run(model, d)
    _check_all(model, d, out, gx, ge, r, 2)


_PATHS = r"""
import json, os, sys
sys.path.insert(0, {pkg!r}); sys.path.insert(0, {repo!r})
import numpy as np, torch
import davis_synth as ds
from gvp_hip import _lib, autograd_ops
from models.molecule_gnn import SelectableMoleculeModelWrapper
way, out_path = sys.argv[1], sys.argv[2]
assert (_lib.bridge() is None) == (os.environ.get("CGVP_BRIDGE") == "0")
dev = "cuda:0"
kw = json.load(open(os.path.join({gold!r}, "model_kwargs.json")))["molecule_gnn_kwargs"]
torch.manual_seed(44)
model = SelectableMoleculeModelWrapper(**dict(kw, num_convs=4))
with torch.no_grad():
    for l, conv in enumerate(model.gnn_model.conv_list):
        conv.eps.fill_(0.05 * (l + 1))
model = model.to(dev).eval()
fwd = torch.compile(model, dynamic=True) if way == "compile" else model
d = {{k: v.to(dev) for k, v in ds.to_torch(ds.drug_batch(7, 3)).items()}}
r = torch.randn(d["x"].shape[0], 64, generator=torch.Generator().manual_seed(1)).to(dev)
res = {{"state." + k: v.detach().cpu().numpy() for k, v in model.gnn_model.state_dict().items()}}

def run(x, e):
    return fwd(x, d["edge_index"], d["ntypes"], d["etypes"], eattr=e)

# 1. plain backward(): parameters, x and eattr
x, e = d["x"].clone().requires_grad_(), d["eattr"].clone().requires_grad_()
out = run(x, e)
(out * r).sum().backward()
res["out"] = out.detach().cpu().numpy()
res["backward"] = e.grad.cpu().numpy()
res["backward.gx"] = x.grad.cpu().numpy()
for n, p in model.gnn_model.named_parameters():
    res["backward.param." + n] = p.grad.cpu().numpy()
# 2. backward(inputs=[eattr]) and retain_graph=True called twice (.grad accumulates: twice the gradient).  A compiled
#    backward cannot be retained (AOTAutograd donates its buffers and says so): there the second call is a second forward.
e = d["eattr"].clone().requires_grad_()
out = run(d["x"], e)
loss = (out * r).sum()
loss.backward(inputs=[e], retain_graph=way != "compile")
res["inputs"] = e.grad.clone().cpu().numpy()
if way == "compile":
    loss = (run(d["x"], e) * r).sum()
loss.backward(inputs=[e])
res["twice"] = e.grad.cpu().numpy()
# 3. torch.autograd.grad w.r.t. eattr alone, no parameter requiring grad
for p in model.parameters():
    p.requires_grad_(False)
e = d["eattr"].clone().requires_grad_()
out = run(d["x"], e)
(g,) = torch.autograd.grad((out * r).sum(), [e])
assert e.grad is None
res["grad_alone"] = g.cpu().numpy()
torch.cuda.synchronize()
np.savez(out_path, **res)
print("ok")
"""


def _child(code, args, env, timeout=600):
    """A fresh child process (the bridge / recompute switches are read once per process), one at a time, under its own
    time limit."""
    res = subprocess.run([sys.executable, "-c", code, *args], env=env, capture_output=True, text=True, timeout=timeout)
    assert res.returncode == 0 and res.stdout.strip().endswith("ok"), (res.returncode, res.stderr[-3000:])


def _paths_reference():
    model = _mol(4).eval()
    d = ds.to_torch(ds.drug_batch(7, 3))
    r = torch.randn(d["x"].shape[0], 64, generator=torch.Generator().manual_seed(1))
    return model, d, r


@pytest.mark.gpu
def test_every_host_path_gives_the_same_bond_feature_gradient(tmp_path):
    """The eager C++ bridge, the torch.library ops (CGVP_BRIDGE=0) and torch.compile(model, dynamic=True), each in a
    fresh process; in each: backward(), backward(inputs=[eattr]) with retain_graph=True then once more (compiled: a
    second forward instead, torch does not retain a compiled backward), and torch.autograd.grad(.., [eattr]) with no
    parameter requiring grad.  Every one against the oracle at the gradient bar;
    the paths against each other at the same bar (the default mode sums the lower layers' g_out with atomics, so the
    numbers are not bitwise equal across runs)."""
    code = _PATHS.format(pkg=os.path.join(REPO, "caster-dta_amd"), repo=REPO, gold=GOLDEN)
    got = {}
    for way, bridge in (("eager", "1"), ("eager", "0"), ("compile", "1")):
        out = tmp_path / f"{way}{bridge}.npz"
        _child(code, [way, str(out)], dict(os.environ, CGVP_BRIDGE=bridge))
        got[(way, bridge)] = dict(np.load(out))
    model, d, r = _paths_reference()
    first = got[("eager", "1")]
    for k, v in model.gnn_model.state_dict().items():               # the children built the same model
        assert np.array_equal(first["state." + k], v.cpu().numpy()), k
    ref, P, gx_ref, ge_ref = _oracle(model, d, r, 4)
    for key, z in got.items():
        assert rel_err(z["out"], ref) < TOL_OUT, key
        for leg in ("backward", "inputs", "grad_alone"):
            print(key, leg, f"{rel_err(z[leg], ge_ref):.2e}")
            assert z[leg].shape == tuple(ge_ref.shape) and rel_err(z[leg], ge_ref) < TOL_G, (key, leg)
            assert rel_err(z[leg], first["backward"]) < TOL_G, (key, leg)
        assert rel_err(z["twice"], 2 * ge_ref) < TOL_G, key
        assert rel_err(z["backward.gx"], gx_ref) < TOL_G, key
        for name in P:
            assert rel_err(z["backward.param." + name], P[name].grad) < TOL_G, (key, name)


@pytest.mark.gpu
def test_bond_feature_gradients_deterministic_mode():
    """torch.use_deterministic_algorithms(True): the STORE instantiation; two identical backward calls give bitwise equal
    d eattr (and d x), within the same bound of the oracle."""
    model = _mol(4).eval()
    d = _dense_hubs()
    torch.use_deterministic_algorithms(True)
    try:
        runs = [_run(model, d) for _ in range(2)]
        torch.cuda.synchronize()
    finally:
        torch.use_deterministic_algorithms(False)
    (out, gx, ge, r), (_, gx2, ge2, _) = runs
    assert torch.equal(ge.grad, ge2.grad) and torch.equal(gx.grad, gx2.grad)
    for p in model.parameters():
        p.grad = p.grad / 2                                     # two backward calls accumulated
    _check_all(model, d, out, gx, ge, r, 4)


_RECOMPUTE = r"""
import json, os, sys
sys.path.insert(0, {pkg!r}); sys.path.insert(0, {repo!r})
import numpy as np, torch
import davis_synth as ds
sys.path.insert(0, os.path.join({repo!r}, "tests"))
import test_gine_edge_grad as T
assert os.environ.get("CGVP_GINE_RECOMPUTE") == "1"
res = {{}}
for num_convs in (2, 4):
    model = T._mol(num_convs).eval()
    d = T._dense_hubs()
    out, gx, ge, r = T._run(model, d)
    res[f"{{num_convs}}.out"] = out.detach().cpu().numpy()
    res[f"{{num_convs}}.ge"] = ge.grad.cpu().numpy()
    res[f"{{num_convs}}.gx"] = gx.grad.cpu().numpy()
    for n, p in model.gnn_model.named_parameters():
        res[f"{{num_convs}}.param." + n] = p.grad.cpu().numpy()
torch.cuda.synchronize()
np.savez(sys.argv[1], **res)
print("ok")
"""


@pytest.mark.gpu
def test_bond_feature_gradients_recompute_kernel(tmp_path):
    """CGVP_GINE_RECOMPUTE=1 (read once per process: a child): the !SAVED instantiation recomputes the messages and
    holds dm the same way.  Dense hubs: tiles of more than one 64-edge chunk reload their registers in phase C."""
    code = _RECOMPUTE.format(pkg=os.path.join(REPO, "caster-dta_amd"), repo=REPO)
    out = tmp_path / "recompute.npz"
    _child(code, [str(out)], dict(os.environ, CGVP_GINE_RECOMPUTE="1"))
    z = dict(np.load(out))
    d = _dense_hubs()
    for num_convs in (2, 4):
        model = _mol(num_convs).eval()
        r = torch.randn(d["x"].shape[0], 64, generator=torch.Generator().manual_seed(1))
        ref, P, gx_ref, ge_ref = _oracle(model, d, r, num_convs)
        print(num_convs, f"d eattr {rel_err(z[f'{num_convs}.ge'], ge_ref):.2e}")
        assert rel_err(z[f"{num_convs}.out"], ref) < TOL_OUT
        assert rel_err(z[f"{num_convs}.ge"], ge_ref) < TOL_G
        assert rel_err(z[f"{num_convs}.gx"], gx_ref) < TOL_G
        for name in P:
            assert rel_err(z[f"{num_convs}.param.{name}"], P[name].grad) < TOL_G, name


@pytest.mark.gpu
def test_molecules_without_bonds():
    """No bonds at all: an empty gradient of the right shape, no launch error."""
    model = _mol(2).eval()
    base = ds.to_torch(ds.drug_batch(3, 2))
    d = dict(x=base["x"], ntypes=base["ntypes"], edge_index=torch.zeros(2, 0, dtype=torch.long),
             etypes=torch.zeros(0, dtype=torch.long), eattr=torch.zeros(0, 9))
    dd = _to(d)
    ge = dd["eattr"].clone().requires_grad_()
    out = model(dd["x"], dd["edge_index"], dd["ntypes"], dd["etypes"], eattr=ge)
    out.sum().backward()
    torch.cuda.synchronize()
    assert ge.grad is not None and ge.grad.shape == (0, 9)
    ref = O.molecule_gine_forward({k: v.detach().cpu() for k, v in model.gnn_model.state_dict().items()}, d["x"],
                                  d["edge_index"], d["ntypes"], d["etypes"], d["eattr"], num_convs=2)
    assert rel_err(out, ref) < TOL_OUT


_ROUTE = r"""
import os, sys
sys.path.insert(0, {pkg!r}); sys.path.insert(0, {repo!r}); sys.path.insert(0, os.path.join({repo!r}, "tests"))
import torch
import davis_synth as ds
from gvp_hip import _lib, autograd_ops
import test_gine_edge_grad as T
assert _lib.bridge() is None
calls = {{"plain": 0, "eattr": 0}}
real = autograd_ops.gine_backward
def counted(*a, need_eattr=None, **k):
    calls["plain" if need_eattr is None else "eattr"] += 1
    return real(*a, need_eattr=need_eattr, **k)
autograd_ops.gine_backward = counted
model = T._mol(2).eval()
dd = T._to(ds.to_torch(ds.drug_batch(4, 9)))
gx = dd["x"].clone().requires_grad_()
out = model(gx, dd["edge_index"], dd["ntypes"], dd["etypes"], eattr=dd["eattr"])
out.sum().backward()
assert calls == {{"plain": 1, "eattr": 0}}, calls            # eattr does not require grad: today's op, today's C call
assert gx.grad is not None
ge = dd["eattr"].clone().requires_grad_()
out = model(dd["x"], dd["edge_index"], dd["ntypes"], dd["etypes"], eattr=ge)
out.sum().backward()
assert calls == {{"plain": 1, "eattr": 1}}, calls
assert ge.grad is not None
torch.cuda.synchronize()
print("ok")
"""


@pytest.mark.gpu
def test_without_bond_feature_gradient_the_route_is_unchanged():
    """eattr without requires_grad beside an x that requires it: caster_gvp::gine_encoder_backward, not the sibling op
    (custom-op path, CGVP_BRIDGE=0, counted at the function both ops call); on the bridge the node allocates no d eattr."""
    code = _ROUTE.format(pkg=os.path.join(REPO, "caster-dta_amd"), repo=REPO)
    _child(code, [], dict(os.environ, CGVP_BRIDGE="0"))
    model = _mol(2).eval()
    dd = _to(ds.to_torch(ds.drug_batch(4, 9)))
    gx = dd["x"].clone().requires_grad_()
    out = model(gx, dd["edge_index"], dd["ntypes"], dd["etypes"], eattr=dd["eattr"])
    out.sum().backward()
    assert gx.grad is not None and dd["eattr"].grad is None


@pytest.mark.gpu
def test_joint_model_bond_feature_gradient_vs_oracle(pretrained):
    """JointGNN, built and loaded as test_attention.py::test_joint_model_all_gradients_vs_oracle: the drug graph's eattr
    requires grad, (y * r).sum().backward() fills its .grad; reference: oracle.joint_forward autograd on the CPU.  Bound:
    that test's, max|err| <= 5e-4 max|want| + 2e-6 scale (scale: the largest parameter-gradient magnitude of the
    reference) -- looser than the encoder-alone bar because the head's dense-vs-varlen formulations sit in between."""
    from models.joint_gnn import JointGNN
    kw = json.load(open(os.path.join(GOLDEN, "model_kwargs.json")))
    model = JointGNN(protein_gnn_kwargs=kw["protein_gnn_kwargs"], molecule_gnn_kwargs=kw["molecule_gnn_kwargs"],
                     **kw["joint_gnn_kwargs"])
    model.load_state_dict(pretrained, strict=True)
    model = model.to(DEV).eval()
    p, m = ds.pair_batch(5, 21, lengths=[40, 75, 33, 120, 64])
    pd, md = ds.to_torch(p), ds.to_torch(m)
    dp, dm = _to(pd), _to(md)
    dp["ptr"], dm["ptr"] = torch.as_tensor(p.ptr).to(DEV), torch.as_tensor(m.ptr).to(DEV)
    dm["eattr"] = dm["eattr"].clone().requires_grad_()
    y, _ = model(dp, dm)
    P = {k: v.clone().requires_grad_(v.numel() > 0) for k, v in pretrained.items()}
    md = dict(md, eattr=md["eattr"].clone().requires_grad_())
    ref = O.joint_forward(P, pd, md)
    assert rel_err(y, ref) < 1e-4
    r = torch.randn(5, 1, generator=torch.Generator().manual_seed(2))
    (y * r.to(DEV)).sum().backward()
    (ref * r).sum().backward()
    scale = max(float(v.grad.abs().max()) for v in P.values() if v.grad is not None)
    want, got = md["eattr"].grad, dm["eattr"].grad
    assert got is not None and got.shape == want.shape
    assert bool((want.abs().amax(0) > 0).all())
    err = float((got.cpu() - want).abs().max())
    print(f"joint d eattr: err {err:.3e}, max|want| {float(want.abs().max()):.3e}, scale {scale:.3e}")
    assert err <= 5e-4 * float(want.abs().max()) + 2e-6 * scale, (err, float(want.abs().max()), scale)
    for name, q in model.named_parameters():                    # and the parameters are what they were
        if q.numel():
            w = P[name].grad
            assert float((q.grad.cpu() - w).abs().max()) <= 5e-4 * float(w.abs().max()) + 2e-6 * scale, name


# ------------------------------------------------------------------------------------------------ CPU
def test_sibling_op_is_registered_with_a_fake_kernel(molecule_params):
    from torch._subclasses.fake_tensor import FakeTensorMode
    from gvp_hip import autograd_ops  # noqa: F401  (registers the ops)
    schema = str(torch.ops.caster_gvp.gine_encoder_backward_eattr.default._schema)
    assert "Tensor[] params" in schema and "bool need_eattr" in schema and schema.rstrip().endswith("(Tensor, Tensor, Tensor)")
    with FakeTensorMode():
        f = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device="cuda")
        keys = ("eps", "nn.lins.0.weight", "nn.lins.0.bias", "nn.lins.1.weight", "nn.lins.1.bias", "lin.weight", "lin.bias")
        mparams = [f(*molecule_params[f"conv_list.{l}.{k}"].shape) for l in range(2) for k in keys]
        Na, Ea = 40, 130
        margs = (mparams, f(Na, 41), f(Na, dt=torch.int64), f(Ea, 9), f(Ea, dt=torch.int64), f(2, Ea, dt=torch.int64), [],
                 [52, 16, 64], 11, 5, 0.01)
        out, mws, mk = torch.ops.caster_gvp.gine_encoder(*margs, 0.2, True)
        op = torch.ops.caster_gvp.gine_encoder_backward_eattr
        gflat, gx, ge = op(f(Na, 64), *margs[:7], mws, mk, [52, 16, 64], 11, 5, 0.01, 0.2, True, True, 0)
        assert gflat.shape == (7390,) and gx.shape == (Na, 41) and ge.shape == (Ea, 9) and ge.dtype == torch.float32
        gflat, gx, ge = op(f(Na, 64), *margs[:7], mws, mk, [52, 16, 64], 11, 5, 0.01, 0.2, False, False, 0)
        assert gflat.shape == (7390,) and gx.numel() == 0 and ge.numel() == 0


def test_new_entry_point_is_exported_and_checks_its_arguments():
    """cgvp_gine_backward_pass_eattr: exported, and with g_eattr = NULL it answers bad arguments exactly as
    cgvp_gine_backward_pass_ex does (host-side checks: no kernel is started, no GPU needed)."""
    from gvp_hip import _lib, autograd_ops
    L = _lib.lib()
    assert "cgvp_gine_backward_pass_eattr" in _lib.exported_symbols() and hasattr(L, "cgvp_gine_backward_pass_eattr")
    assert _lib.ABI_VERSION == 31 and L.cgvp_abi_version() == 31
    header = open(os.path.join(REPO, "include", "caster_gvp.h")).read()
    assert "cgvp_gine_backward_pass_eattr(" in header
    cfg = autograd_ops._gine_cfg([52, 16, 64], 11, 5, 9, 0.01)
    bad = autograd_ops._gine_cfg([52, 16, 64], 11, 5, 9, 0.01)
    bad.num_layers = 0
    w = (_lib.GineW * 2)()
    batch = _lib.GineBatch()
    batch.num_nodes, batch.num_edges = 5, 4
    null, p256, odd = C.c_void_p(0), C.c_void_p(0x1000), C.c_void_p(0x1010)
    cases = [
        (None, w, batch, null, null, null),                     # no configuration
        (C.byref(cfg), w, batch, null, null, null),             # no workspaces
        (C.byref(cfg), w, batch, odd, p256, p256),              # misaligned forward workspace
        (C.byref(cfg), w, batch, p256, odd, p256),              # misaligned backward workspace
        (C.byref(cfg), w, batch, p256, p256, null),             # no grad_flat
        (C.byref(bad), w, batch, p256, p256, p256),             # bad configuration
    ]
    for flags in (0, _lib.BWD_DETERMINISTIC):
        for cfg_p, w_, b_, fws, bws, gflat in cases:
            rc_ex = L.cgvp_gine_backward_pass_ex(cfg_p, w_, C.byref(b_), 0.0, null, fws, null, bws, gflat, null, 0, flags, null)
            rc_new = L.cgvp_gine_backward_pass_eattr(cfg_p, w_, C.byref(b_), 0.0, null, fws, null, bws, gflat, null, null, 0,
                                                     flags, null)
            assert rc_ex != 0 and rc_new == rc_ex, (flags, rc_ex, rc_new)
