"""The deterministic mode of the backward passes (torch.use_deterministic_algorithms(True) / CGVP_DETERMINISTIC=1):
no float atomics in any kernel the mode launches, bitwise equal gradients run to run, the same math as the default
mode, and torch's rule -- deterministic or raise -- where a path has no deterministic form."""
import copy
import ctypes as C
import glob
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import davis_synth as ds
from conftest import GOLDEN, REPO, rel_err
from gvp_hip import _lib, graphed
from test_hip_backward import DEV, T, _check_grads, _encoder, _to

OBJ = os.path.join(REPO, "caster-dta_amd", "lib", "_obj")
FLOAT_ATOMIC = re.compile(r"\b(global|flat|buffer)_atomic_(add_f32|pk_add_\w+)\b")
CMPSWAP = re.compile(r"\b(global|flat|buffer)_atomic_cmpswap")


def _kernels(stem):
    """{mangled kernel name: its instruction lines} from the build's gfx950 assembly of one translation unit."""
    path = glob.glob(os.path.join(OBJ, stem + "-hip-amdgcn-amd-amdhsa-gfx950.s"))
    assert path, f"no assembly of {stem} (build() keeps it under lib/_obj)"
    out, cur = {}, None
    for line in open(path[0]):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            out[cur] = []
        elif cur and line.startswith("\t"):
            out[cur].append(line)
        if line.startswith("\t.size\t") or line.startswith(".Lfunc_end"):
            cur = None
    return out


def _one(kernels, *parts):
    names = [k for k in kernels if all(p in k for p in parts)]
    assert len(names) == 1, (parts, names)
    return kernels[names[0]]


def _clean(lines):
    return not any(FLOAT_ATOMIC.search(l) or CMPSWAP.search(l) for l in lines)


# ----------------------------------------------------------------------------------------------------- CPU: ISA
def test_isa_of_the_deterministic_kernels_has_no_float_atomics():
    bwd = _kernels("gvp_quad_bwd_kernels")
    # conv_bwd2_kernel<NTE, ST, TN = 1, 8 waves, STORE = true>: fp32 and bf16 storage, both edge one-hot widths
    for st in ("Ef", "EN2gq5bf16sE"):
        for nte in ("ILi0", "ILi1"):
            k = _one(bwd, "conv_bwd2_kernel" + nte + st, "Li1ELi8ELb1E")
            assert _clean(k), ("conv_bwd2 STORE", nte, st)
    for w in (16, 28, 41, 52):
        assert _clean(_one(bwd, f"src_sum_kernelILi{w}E")), w
    assert _clean(_one(bwd, "reduce_segments_kernelILb0E"))
    assert _clean(_one(bwd, "reduce_segments_rows_kernelILb0E"))
    gine = _kernels("gine_quad_kernels")
    stores = [k for k in gine if "gine_quad_bwd_kernel" in k and k.endswith("Lb1ELb1EEEvNS_9GineQArgsE")]
    assert len(stores) == 4                      # every compiled layer shape, SAVED + STORE
    for k in stores:
        assert _clean(gine[k]), k
    # control: the default instantiation still adds d h[src] with float atomics -- the grep reads the right code
    default = _one(bwd, "conv_bwd2_kernelILi0EfLi1ELi8ELb0E")
    assert any("global_atomic_add_f32" in l for l in default)
    src = _kernels("graph_index_kernels")
    for name in ("src_count_kernel", "src_fill_kernel", "src_rank_kernel"):
        assert _clean(_one(src, name)), name


# ----------------------------------------------------------------------------------------------------- CPU: ABI
def test_workspace_queries_of_the_mode():
    """Host-only calls: in the mode the queries leave room for the stored rows and the source-order index; with flags 0
    they return exactly what the plain queries return."""
    from gvp_hip import autograd_ops, ops
    L = _lib.lib()
    dims = ops.make_dims(storage=ops.F32, node_in_s=17, node_in_v=3, edge_in_s=32, edge_in_v=1, hidden_s=16, hidden_v=4,
                         edge_hidden_s=32, edge_hidden_v=1, out_s=64)
    layout = ops.lba_layout(dims, 20, 1, 2)
    for N, E in ((19200, 57000), (300, 0), (1, 1)):
        plain = L.cgvp_lba_bwd_workspace_bytes(C.byref(dims), C.byref(layout), N, E)
        assert plain > 0
        assert L.cgvp_lba_bwd_workspace_bytes_ex(C.byref(dims), C.byref(layout), N, E, 0) == plain or _lib.DETERMINISTIC_ENV
        det = L.cgvp_lba_bwd_workspace_bytes_ex(C.byref(dims), C.byref(layout), N, E, _lib.BWD_DETERMINISTIC)
        assert det >= plain + E * 28 * 4 + (N + 1 + E) * 4, (N, E)
    cfg = autograd_ops._gine_cfg([52, 16, 16], 11, 5, 9, 0.0)
    for N, E in ((2600, 5600), (40, 0)):
        plain = L.cgvp_gine_bwd_workspace_bytes(C.byref(cfg), N, E)
        assert plain > 0
        assert L.cgvp_gine_bwd_workspace_bytes_ex(C.byref(cfg), N, E, 0) == plain or _lib.DETERMINISTIC_ENV
        det = L.cgvp_gine_bwd_workspace_bytes_ex(C.byref(cfg), N, E, _lib.BWD_DETERMINISTIC)
        assert det >= plain + E * 41 * 4 + N * 41 * 4 + (N + 1 + E) * 4, (N, E)
    assert L.cgvp_deterministic_forced() == (1 if _lib.DETERMINISTIC_ENV else 0)


# ----------------------------------------------------------------------------------------------------- CPU: mode
def test_mode_follows_torch_flag_and_graph_buckets_carry_it():
    was = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(False)
        assert _lib.deterministic_mode() == _lib.DETERMINISTIC_ENV
        assert _lib.bwd_flags() == (_lib.BWD_DETERMINISTIC if _lib.DETERMINISTIC_ENV else 0)
        off = graphed.mode_key((1, 2, 3, 4), torch.float32)
        torch.use_deterministic_algorithms(True)
        assert _lib.deterministic_mode() and _lib.bwd_flags() == _lib.BWD_DETERMINISTIC
        on = graphed.mode_key((1, 2, 3, 4), torch.float32)
        assert on != off or _lib.DETERMINISTIC_ENV
    finally:
        torch.use_deterministic_algorithms(was)


def test_warn_only_runs_a_path_without_deterministic_form_with_a_warning():
    """torch.use_deterministic_algorithms(True, warn_only=True): a backward without a deterministic form (its entry point
    returns ERR_NONDETERMINISTIC before launching anything) warns and runs in the default mode; with the plain flag it
    raises."""
    calls = []

    def fn(flags):
        calls.append(flags)
        return _lib.ERR_NONDETERMINISTIC if flags else 0
    was, wo = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    try:
        torch.use_deterministic_algorithms(True, warn_only=True)
        if not _lib.DETERMINISTIC_ENV:
            with pytest.warns(UserWarning, match="does not have a deterministic implementation"):
                assert _lib.call_bwd(fn, _lib.bwd_flags(), "x") == 0
            assert calls == [1, 0]
        torch.use_deterministic_algorithms(True)
        with pytest.raises(RuntimeError, match="does not have a deterministic implementation"):
            _lib.check(_lib.call_bwd(fn, _lib.bwd_flags(), "x"), "x")
    finally:
        torch.use_deterministic_algorithms(was, warn_only=wo)
    L = _lib.lib()
    assert L.cgvp_conv_bwd_det_floats(19200, 57000) >= 57000 * 28
    assert L.cgvp_src_index_work_ints(19200, 57000) >= 19201 + 57000


def test_environment_switch_forces_the_mode_and_refuses_the_plain_passes():
    code = ("import ctypes as C, sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from gvp_hip import _lib\n"
            "L = _lib.lib()\n"
            "assert _lib.DETERMINISTIC_ENV and _lib.deterministic_mode() and _lib.bwd_flags() == 1\n"
            "assert L.cgvp_deterministic_forced() == 1\n"
            "rc = L.cgvp_lba_backward_pass(None, None, None, 0, 0.0, None, None, None, None, None, None, None, None, None, None)\n"
            "assert rc == _lib.ERR_NONDETERMINISTIC, rc\n"
            "try:\n"
            "    _lib.check(rc, 'cgvp_lba_backward_pass')\n"
            "except RuntimeError as e:\n"
            "    assert 'does not have a deterministic implementation' in str(e)\n"
            "else:\n"
            "    raise AssertionError('no error')\n"
            "print('ok')\n") % (os.path.join(REPO, "caster-dta_amd"), REPO)
    env = dict(os.environ, CGVP_DETERMINISTIC="1")
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip().endswith("ok"), res.stderr[-2000:]


# ----------------------------------------------------------------------------------------------------- GPU
class _Deterministic:
    def __enter__(self):
        self.was = torch.are_deterministic_algorithms_enabled()
        torch.use_deterministic_algorithms(True)

    def __exit__(self, *a):
        torch.use_deterministic_algorithms(self.was)


def _rng_snapshot():
    """torch's CUDA generator and the encoders' persistent dropout generator states ({seed, offset} on the device, advanced
    by every training pass), so that every run of a test draws the same dropout masks (_rng_restore)."""
    from gvp_hip import autograd_ops
    torch.cuda.manual_seed(1234)
    states = {k: autograd_ops.rng_state(k, torch.device(DEV)) for k in ("lba", "gine")}
    return states, {k: v.clone() for k, v in states.items()}, torch.cuda.get_rng_state()


def _rng_restore(snap):
    states, saved, cuda = snap
    torch.cuda.set_rng_state(cuda)
    for k, v in states.items():
        v.copy_(saved[k])


def _assert_bitwise(runs):
    out0, g0 = runs[0]
    for out, g in runs[1:]:
        assert torch.equal(out, out0)
        assert g.keys() == g0.keys()
        for k in g0:
            assert g[k] is not None and torch.equal(g[k], g0[k]), k


def _assert_default_close(g0, gd, loose=("gvp_edge.",)):
    """The mode reorders sums, nothing else: relative L2 per tensor within 1e-5 (5e-2 for the cancelling edge-embedding
    block: gvp_edge, or W_e of the stand-alone stacks),
    with the floor tied to the global gradient scale that every run-to-run comparison of the default mode needs
    (analytically-zero gradients such as gvp_edge's gate weights, ~1e-8, are rounding noise)."""
    scale = max(float(v.abs().max()) for k, v in gd.items() if not k.startswith("in."))
    for k in g0:
        tol = 5e-2 if loose and k.startswith(loose) else 1e-5
        err = float((g0[k] - gd[k]).double().norm()) / (float(gd[k].double().norm()) + 1e-6 * scale)
        assert err < tol, (k, err)


def _lba_run(model, d, r, snap, det=True):
    """fwd + bwd of a COPY of `model` from the generator state `snap`, train mode; returns (out, grads)."""
    m = copy.deepcopy(model).train()
    _rng_restore(snap)
    xs, xv = d["x"][0].clone().requires_grad_(), d["x"][1].clone().requires_grad_()
    es, ev = d["eattr"][0].clone().requires_grad_(), d["eattr"][1].clone().requires_grad_()
    with (_Deterministic() if det else torch.enable_grad()):
        out = m((xs, xv), d["edge_index"], d["ntypes"], d["etypes"], eattr=(es, ev))
        (out * r).sum().backward()
    g = {n: p.grad.clone() for n, p in m.gnn_model.named_parameters() if p.numel()}
    g.update({"in.x_s": xs.grad, "in.x_v": xv.grad, "in.e_s": es.grad, "in.e_v": ev.grad})
    return out.detach(), g


def _check_bitwise_and_default(model, d):
    snap = _rng_snapshot()
    r = torch.randn(_lba_run(model, d, 1.0, snap, det=False)[0].shape, generator=torch.Generator().manual_seed(7)).to(DEV)
    runs = [_lba_run(model, d, r, snap) for _ in range(3)]
    _assert_bitwise(runs)
    outd, gd = _lba_run(model, d, r, snap, det=False)
    assert torch.equal(outd, runs[0][0])         # the forward is the same launches either way
    _assert_default_close(runs[0][1], gd)


@pytest.mark.gpu
def test_lba_davis_b64_bitwise(protein_params):
    pb, _ = ds.pair_batch(64, 0, length=300, thresh=4.0, thresh_type="dist")
    _check_bitwise_and_default(_encoder(protein_params), _to(ds.to_torch(pb)))


@pytest.mark.gpu
def test_lba_long_graph_bitwise(protein_params):
    pb, _ = ds.pair_batch(4, 1, length=1200, thresh=4.0, thresh_type="dist")
    _check_bitwise_and_default(_encoder(protein_params), _to(ds.to_torch(pb)))


@pytest.mark.gpu
def test_lba_bf16_four_layers_bitwise():
    """CASTER-DTA(4,4) with bf16 activation storage (config 5's encoder)."""
    pb, _ = ds.pair_batch(16, 2, length=300, thresh=4.0, thresh_type="dist")
    d = _to(ds.to_torch(pb))
    d = dict(d, x=tuple(t.bfloat16() for t in d["x"]), eattr=tuple(t.bfloat16() for t in d["eattr"]))
    _check_bitwise_and_default(_encoder(num_convs=4, seed=0), d)


@pytest.mark.gpu
def test_lba_golden_under_the_mode(lba_small, protein_params):
    """The reference's own gradients hold in the mode at the existing tolerances."""
    g = lba_small
    model = _encoder(protein_params).eval()
    with _Deterministic():
        xs, xv = T(g["x_s"]).to(DEV).requires_grad_(), T(g["x_v"]).to(DEV).requires_grad_()
        out = model((xs, xv), T(g["edge_index"]).to(DEV), T(g["ntypes"]).to(DEV), T(g["etypes"]).to(DEV),
                    eattr=(T(g["e_s"]).to(DEV), T(g["e_v"]).to(DEV)), batch=T(g["batch"]).to(DEV))
        (out * T(g["r"]).to(DEV)).sum().backward()
    ref = {k[2:]: T(v) for k, v in g.items() if k.startswith("g_")}
    assert _check_grads(model, ref) >= 60
    assert rel_err(xs.grad, g["gin_x_s"]) < 2e-4
    assert rel_err(xv.grad, g["gin_x_v"]) < 2e-4


@pytest.mark.gpu
def test_lba_sparse_edge_feature_gradients_golden_under_the_mode(lba_sparse, protein_params):
    """lba_sparse (the fused layers) with the raw edge-feature gradients, against the reference's autograd, in the mode;
    a second call in the mode gives the same input gradients bitwise."""
    g = lba_sparse
    model = _encoder(protein_params).eval()
    res = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        with _Deterministic():
            xs, xv = T(g["x_s"]).to(DEV).requires_grad_(), T(g["x_v"]).to(DEV).requires_grad_()
            es, ev = T(g["e_s"]).to(DEV).requires_grad_(), T(g["e_v"]).to(DEV).requires_grad_()
            out = model((xs, xv), T(g["edge_index"]).to(DEV), T(g["ntypes"]).to(DEV), T(g["etypes"]).to(DEV),
                        eattr=(es, ev), batch=T(g["batch"]).to(DEV))
            (out * T(g["r"]).to(DEV)).sum().backward()
        res.append((es.grad, ev.grad, xs.grad, xv.grad))
    assert rel_err(es.grad, g["gin_e_s"]) < 2e-4 and rel_err(ev.grad, g["gin_e_v"]) < 2e-4
    assert rel_err(xs.grad, g["gin_x_s"]) < 2e-4 and rel_err(xv.grad, g["gin_x_v"]) < 2e-4
    ref = {k[2:]: T(v) for k, v in g.items() if k.startswith("g_")}
    assert _check_grads(model, ref) >= 60
    for a_, b_ in zip(*res):
        assert torch.equal(a_, b_)


@pytest.mark.gpu
@pytest.mark.parametrize("num_convs", [2, 4])
def test_gine_bitwise_with_input_gradient(molecule_params, num_convs):
    from models.molecule_gnn import SelectableMoleculeModelWrapper
    from oracle import gvp_oracle as O
    kw = json.load(open(os.path.join(GOLDEN, "model_kwargs.json")))["molecule_gnn_kwargs"]
    kw = dict(kw, num_convs=num_convs)
    torch.manual_seed(0)
    model = SelectableMoleculeModelWrapper(**kw)
    if num_convs == 2:
        model.load_state_dict({"gnn_model." + k: v for k, v in molecule_params.items()})
    model = model.to(DEV)
    d = _to(ds.to_torch(ds.drug_batch(64, 3)))
    snap = _rng_snapshot()

    def run(det):
        m = copy.deepcopy(model).train()
        _rng_restore(snap)
        gx = d["x"].clone().requires_grad_()
        ctx = _Deterministic() if det else torch.enable_grad()
        with ctx:
            out = m(gx, d["edge_index"], d["ntypes"], d["etypes"], eattr=d["eattr"])
            r = torch.randn(out.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
            (out * r).sum().backward()
        g = {n: p.grad.clone() for n, p in m.gnn_model.named_parameters()}
        g["in.x"] = gx.grad
        return out.detach(), g
    runs = [run(True) for _ in range(3)]
    for out, g in runs[1:]:
        assert torch.equal(out, runs[0][0])
        for k in runs[0][1]:
            assert torch.equal(g[k], runs[0][1][k]), k
    _, gd = run(False)
    for k, v in runs[0][1].items():
        assert rel_err(v, gd[k]) < 1e-5, (k, rel_err(v, gd[k]))
    if num_convs == 2:                           # the oracle, at the existing tolerance
        dc = ds.to_torch(ds.drug_batch(64, 3))
        P = {k: v.clone().requires_grad_(True) for k, v in molecule_params.items()}
        x = dc["x"].clone().requires_grad_()
        m = copy.deepcopy(model).eval()
        gx = d["x"].clone().requires_grad_()
        with _Deterministic():
            out = m(gx, d["edge_index"], d["ntypes"], d["etypes"], eattr=d["eattr"])
            r = torch.randn(out.shape, generator=torch.Generator().manual_seed(1))
            (out * r.to(DEV)).sum().backward()
        ref = O.molecule_gine_forward(P, x, dc["edge_index"], dc["ntypes"], dc["etypes"], dc["eattr"])
        (ref * r).sum().backward()
        for name, p in m.gnn_model.named_parameters():
            assert rel_err(p.grad, P[name].grad) < 2e-4, name
        assert rel_err(gx.grad, x.grad) < 2e-4


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["pocketminer", "cpdmodel", "cpdmodel_k"])
def test_standalone_gvp_stacks_bitwise_and_golden_in_the_mode(name):
    """The stand-alone GVPConvLayer stacks (PocketMiner; CPD with its autoregressive decoder at the default folded edge
    width 52, and at 32) through conv_layer_ops in the mode: three runs bitwise equal, the reference's own outputs and
    gradients at the tolerance of test_gvp_stacks.py, and the default mode's gradients to 1e-5."""
    import test_gvp_stacks as S
    from conftest import load_npz
    gold = load_npz("gvp_stacks.npz")
    model = S._model(name, gold).to(DEV)
    inp = S._inputs(gold, DEV)
    r = T(gold[f"{name}_r"]).to(DEV)

    def run(det):
        m = copy.deepcopy(model)
        with (_Deterministic() if det else torch.enable_grad()):
            out = m(**inp)
            (out * r).sum().backward()
        return m, out.detach(), {n: p.grad.clone() for n, p in m.named_parameters() if p.numel() and p.grad is not None}
    runs = [run(True) for _ in range(3)]
    _assert_bitwise([(o, g) for _, o, g in runs])
    m0, out0, g0 = runs[0]
    assert rel_err(out0, gold[f"{name}_out"]) < 2e-5
    assert S._check_grads(m0, gold, name)[0] >= 60
    _, _, gd = run(False)
    _assert_default_close(g0, gd, loose=("gnn_model.W_e.",))    # W_e: the stacks' edge embedding (gvp_edge's role)


_HEAD_RNG_FN = "_head_rng_state"      # the head's fused dropout sites: their persistent {seed, offset}
_JOINT = r"""
import copy, json, os, sys
sys.path.insert(0, {pkg!r}); sys.path.insert(0, {repo!r})
import numpy as np, torch
import davis_synth as ds
from gvp_hip import _lib, autograd_ops, head_ops
from models.joint_gnn import JointGNN
way, out_path = sys.argv[1], sys.argv[2]
assert (_lib.bridge() is None) == (os.environ.get("CGVP_BRIDGE") == "0")
dev = torch.device("cuda:0")
gold = {gold!r}
kw = json.load(open(os.path.join(gold, "model_kwargs.json")))
state = {{k: torch.from_numpy(v) for k, v in np.load(os.path.join(gold, "pretrained_state.npz")).items()}}
model = JointGNN(protein_gnn_kwargs=kw["protein_gnn_kwargs"], molecule_gnn_kwargs=kw["molecule_gnn_kwargs"],
                 **kw["joint_gnn_kwargs"])
model.load_state_dict(state, strict=True)
model = model.to(dev).train()
p, m = ds.pair_batch(6, 2, lengths=[120, 80, 95, 130, 60, 101])
to = lambda d: {{k: (tuple(t.to(dev) for t in v) if isinstance(v, tuple) else v.to(dev)) for k, v in d.items()}}
pd, md = to(ds.to_torch(p)), to(ds.to_torch(m))
pd["ptr"], md["ptr"] = torch.as_tensor(p.ptr).to(dev), torch.as_tensor(m.ptr).to(dev)
target = torch.linspace(-1, 1, 6, device=dev).unsqueeze(-1)
torch.cuda.manual_seed(1234)
states = {{k: autograd_ops.rng_state(k, dev) for k in ("lba", "gine")}}
states["head"] = head_ops.{headfn}(dev)
saved = {{k: v.clone() for k, v in states.items()}}
cuda = torch.cuda.get_rng_state()
torch.use_deterministic_algorithms(True)
assert _lib.bwd_flags() == _lib.BWD_DETERMINISTIC
res = {{}}
for run in range(3):
    mm = copy.deepcopy(model)
    torch.cuda.set_rng_state(cuda)
    for k, v in states.items():
        v.copy_(saved[k])
    if way == "graphed":
        from gvp_hip.graphed import GraphedTrainStep
        step = GraphedTrainStep(mm, torch.nn.functional.mse_loss)
        loss, pred = step.run(pd, md, target)
    else:
        pred, _ = mm(pd, md)
        loss = torch.nn.functional.mse_loss(pred, target)
        loss.backward()
    torch.cuda.synchronize()
    res[f"{{run}}.loss"] = loss.detach().float().cpu().numpy().reshape(1)
    res[f"{{run}}.pred"] = pred.detach().float().cpu().numpy()
    for n, q in mm.named_parameters():
        if q.grad is not None:
            res[f"{{run}}.grad.{{n}}"] = q.grad.detach().cpu().numpy()
np.savez(out_path, **res)
print("ok")
"""


@pytest.mark.gpu
@pytest.mark.parametrize("way,bridge", [("eager", "1"), ("eager", "0"), ("graphed", "1")])
def test_joint_training_step_bitwise(tmp_path, way, bridge):
    """A whole JointGNN training step (train mode, dropout on, MSE loss, backward through the head and both encoders)
    under torch.use_deterministic_algorithms(True), three ways: eager through the C++ bridge, through the torch.library
    ops (bridge off), and replayed by GraphedTrainStep.  Three runs from the same state: loss, predictions and every
    gradient bitwise equal.  (A fresh process per way: the bridge switch is read once per process.)"""
    code = _JOINT.format(pkg=os.path.join(REPO, "caster-dta_amd"), repo=REPO, gold=GOLDEN, headfn=_HEAD_RNG_FN)
    out = tmp_path / "res.npz"
    env = dict(os.environ, CGVP_BRIDGE=bridge)
    res = subprocess.run([sys.executable, "-c", code, way, str(out)], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and res.stdout.strip().endswith("ok"), res.stderr[-3000:]
    z = dict(np.load(out))
    keys = sorted(k[2:] for k in z if k.startswith("0."))
    assert "loss" in keys and "pred" in keys and sum(k.startswith("grad.") for k in keys) > 100
    for run in (1, 2):
        assert sorted(k[2:] for k in z if k.startswith(f"{run}.")) == keys
        for k in keys:
            assert np.array_equal(z[f"{run}.{k}"], z[f"0.{k}"]), (run, k)


@pytest.mark.gpu
def test_bench_dump_outputs_bitwise_in_the_mode(tmp_path):
    args = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--epoch", "off", "--no-cpu-baseline"]
    env = dict(os.environ, CGVP_DETERMINISTIC="1")
    arrays = []
    for tag in ("a", "b"):
        res = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *args, "--dump-outputs", str(tmp_path / tag)],
                             capture_output=True, text=True, timeout=600, env=env)
        assert res.returncode == 0, res.stderr[-3000:]
        arrays.append({p.name[:-4]: np.load(p) for p in sorted((tmp_path / tag).iterdir())})
    a, b = arrays
    assert sorted(a) == sorted(b) and any(k.startswith("grad.protein_gnn.") for k in a)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
