"""The launch-dispatch branches that environment switches select, each in a fresh child process (the switches are read
once per process): CGVP_CONV_BWD=1|2 (the two A/B conv backward kernels), CGVP_BWD_STORE_ONCE=0 (read-add-write slab
accumulation at every size), CGVP_SPLIT_HEAD_BWD=1 (head backward in a launch of its own), CGVP_BRIDGE=0 (the
torch.library host path) and the default.

Every child runs the protein encoder forward + backward -- two conv layers, eval mode (dropout off), aggr 'sum' and
'mean', fp32 and bf16 storage -- on the two small golden batches of test_hip_backward.py (lba_small: two-launch layers,
lba_sparse: fused layers, a node count that is no multiple of 16) and writes the output, every parameter gradient and
the node-feature gradients (fp32: the edge-feature gradients too) to an .npz.

Checker: the CPU oracle (oracle/gvp_oracle.py, autograd), computed once per module.  fp32: the metric and bound of
test_hip_backward.py::_check_grads (2e-4 of the tensor's own maximum + the floor tied to the global gradient scale),
outputs 2e-5, input gradients rel_err < 2e-4.  bf16: the emulating oracle and the bounds of test_bf16_storage.py
(outputs 1e-2, every gradient tensor 2e-2 in L2 with its absolute floor).  The variants are NOT compared with each
other: they sum in different orders."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, load_npz, rel_err
from oracle import gvp_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = torch.from_numpy
BATCHES, AGGRS, STORAGES = ("lba_small", "lba_sparse"), ("sum", "mean"), ("f32", "bf16")
SETTINGS = [{}, {"CGVP_CONV_BWD": "1"}, {"CGVP_CONV_BWD": "2"}, {"CGVP_BWD_STORE_ONCE": "0"},
            {"CGVP_SPLIT_HEAD_BWD": "1"}, {"CGVP_BRIDGE": "0"}]
SWITCHES = sorted({k for s in SETTINGS for k in s})
FWD_TOL_BF16, GRAD_TOL_BF16 = 1e-2, 2e-2            # test_bf16_storage.py


def _state():
    pfx = "protein_gnn.gnn_model."
    return {k[len(pfx):]: T(v) for k, v in load_npz("pretrained_state.npz").items() if k.startswith(pfx)}


def _inputs(batch, storage):
    """The golden batch's tensors on the CPU; bf16 storage: the features rounded to bf16 (widened again, for the oracle)."""
    g = load_npz(batch + ".npz")
    c = (lambda a: T(a).to(torch.bfloat16).float()) if storage == "bf16" else T
    return dict(x=(c(g["x_s"]), c(g["x_v"])), eattr=(c(g["e_s"]), c(g["e_v"])), edge_index=T(g["edge_index"]),
                ntypes=T(g["ntypes"]), etypes=T(g["etypes"]), r=T(g["r"]))


def _child_main(out_path):
    """Runs in the child: every (batch, aggr, storage) case on the GPU -> one .npz."""
    from test_hip_backward import _encoder
    state, res = _state(), {}
    for batch in BATCHES:
        for aggr in AGGRS:
            for storage in STORAGES:
                d = _inputs(batch, storage)
                model = _encoder(state, 2, aggr, dropout=0.0).eval()
                dt = torch.bfloat16 if storage == "bf16" else torch.float32
                leaf = lambda t, grad: t.to(DEV).to(dt).requires_grad_(grad)
                xs, xv = leaf(d["x"][0], True), leaf(d["x"][1], True)
                es, ev = leaf(d["eattr"][0], storage == "f32"), leaf(d["eattr"][1], storage == "f32")
                out = model((xs, xv), d["edge_index"].to(DEV), d["ntypes"].to(DEV), d["etypes"].to(DEV), eattr=(es, ev))
                assert out.dtype == dt
                (out.float() * d["r"].to(DEV)).sum().backward()
                key = f"{batch}.{aggr}.{storage}."
                res[key + "out"] = out.detach().float().cpu().numpy()
                res[key + "gin.x_s"], res[key + "gin.x_v"] = xs.grad.float().cpu().numpy(), xv.grad.float().cpu().numpy()
                if storage == "f32":
                    res[key + "gin.e_s"], res[key + "gin.e_v"] = es.grad.cpu().numpy(), ev.grad.cpu().numpy()
                for name, p in model.gnn_model.named_parameters():
                    if p.numel():
                        assert p.grad.dtype == torch.float32
                        res[key + "g." + name] = p.grad.cpu().numpy()
    torch.cuda.synchronize()
    np.savez(out_path, **res)


_CHILD = r"""
import os, sys
sys.path.insert(0, {pkg!r}); sys.path.insert(0, {repo!r}); sys.path.insert(0, os.path.join({repo!r}, "tests"))
from gvp_hip import _lib
import test_launch_variants as V
assert os.environ.get("CGVP_BRIDGE") != "0" or _lib.bridge() is None
V._child_main(sys.argv[1])
print("ok")
"""


@pytest.fixture(scope="module")
def oracle_refs():
    """(batch, aggr, storage) -> output, parameter gradients and input gradients of the CPU oracle; computed once."""
    state, refs = _state(), {}
    for batch in BATCHES:
        for aggr in AGGRS:
            for storage in STORAGES:
                d = _inputs(batch, storage)
                P = {k: v.clone().requires_grad_(v.numel() > 0) for k, v in state.items()}
                x = tuple(t.clone().requires_grad_() for t in d["x"])
                e = tuple(t.clone().requires_grad_() for t in d["eattr"])
                if storage == "bf16":
                    with O.emulate_gemm_dtype(torch.bfloat16):
                        ref = O.protein_lba_forward(P, x, d["edge_index"], d["ntypes"], d["etypes"], e, num_convs=2,
                                                    aggr=aggr, store_dtype=torch.bfloat16)
                        (ref * d["r"]).sum().backward()
                else:
                    ref = O.protein_lba_forward(P, x, d["edge_index"], d["ntypes"], d["etypes"], e, num_convs=2, aggr=aggr)
                    (ref * d["r"]).sum().backward()
                refs[(batch, aggr, storage)] = dict(
                    out=ref.detach(), g={k: v.grad for k, v in P.items() if v.numel()},
                    gin={"x_s": x[0].grad, "x_v": x[1].grad, "e_s": e[0].grad, "e_v": e[1].grad})
    return refs


def _figures_f32(z, key, ref):
    """-> [(what, error, bound)]: outputs 2e-5; weight gradients as test_hip_backward.py::_check_grads; inputs 2e-4."""
    figs = [(key + "out", rel_err(z[key + "out"], ref["out"]), 2e-5)]
    scale = max(float(v.abs().max()) for v in ref["g"].values())
    for name, want in ref["g"].items():
        err = float((T(z[key + "g." + name]) - want).abs().max())
        figs.append((key + "g." + name, err, 2e-4 * float(want.abs().max()) + 2e-6 * scale))
    for name, want in ref["gin"].items():
        figs.append((key + "gin." + name, rel_err(z[key + "gin." + name], want), 2e-4))
    return figs


def _figures_bf16(z, key, ref):
    """-> [(what, error, bound)] as test_bf16_storage.py::test_bf16_forward_backward_vs_oracle states them."""
    figs = [(key + "out", rel_err(z[key + "out"], ref["out"]), FWD_TOL_BF16)]
    scale = max(float(v.abs().max()) for v in ref["g"].values())
    for name, want in ref["g"].items():
        err = (float((T(z[key + "g." + name]) - want).norm()) - 2e-3 * scale) / max(float(want.norm()), 1e-30)
        figs.append((key + "g." + name, err, GRAD_TOL_BF16))
    for name in ("x_s", "x_v"):
        want = ref["gin"][name]
        figs.append((key + "gin." + name, float((T(z[key + "gin." + name]) - want).norm() / want.norm()), GRAD_TOL_BF16))
    return figs


_child_failed = []          # a child that crashed or ran out of time: no further child is started in this session


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "-".join(f"{k}={v}" for k, v in s.items()) or "default")
def test_launch_variant_matches_the_oracle(setting, oracle_refs, tmp_path):
    if _child_failed:
        pytest.fail(f"not started: the child for {_child_failed[0]} failed before")
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(setting)
    out = tmp_path / "variant.npz"
    code = _CHILD.format(pkg=os.path.join(REPO, "caster-dta_amd"), repo=REPO)
    try:
        res = subprocess.run([sys.executable, "-c", code, str(out)], env=env, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        _child_failed.append(setting)
        raise
    if not (res.returncode == 0 and res.stdout.strip().endswith("ok")):
        _child_failed.append(setting)
        pytest.fail(f"child failed: {res.returncode}\n{res.stderr[-3000:]}")
    z = dict(np.load(out))
    bad = []
    for (batch, aggr, storage), ref in oracle_refs.items():
        key = f"{batch}.{aggr}.{storage}."
        figs = (_figures_f32 if storage == "f32" else _figures_bf16)(z, key, ref)
        what, err, bound = max(figs, key=lambda f: f[1] / f[2])
        print(f"{setting or 'default'} {key} closest to its bound: {what} {err:.2e} (bound {bound:.2e})")
        bad += [f for f in figs if not f[1] <= f[2]]
    assert not bad, bad
