"""The persistent tile loops of the encoder kernels beyond their first trip, at small shapes.

Every tile kernel of the backward chain is a fixed grid of workgroups whose waves walk 16-row tiles in a loop; at the
suite's usual sizes every wave has at most one tile, so the second trip -- the read-add-write into a wave's already
filled LDS block (AccPriv), the carry of a target's partial sum across a wave's iterations, a wave whose whole edge range
lies inside one target, waves with an empty range -- never runs.  The launch knobs (read once per process) shrink the
grids until ~400 nodes are several trips: CGVP_BWD_GRID, CGVP_CONV_FWD_WAVES, CGVP_GINE_FWD_WGS, combined with
CGVP_CONV_BWD, CGVP_SPLIT_HEAD_BWD, CGVP_GINE_RECOMPUTE and autograd_ops.GINE_BWD_WORKGROUPS.

Each setting of SETTINGS runs in a fresh child process that runs every case on the GPU and writes one .npz (the
pattern, and the `_child_failed` rule, of test_launch_variants.py).  Checker: the CPU oracle (oracle/gvp_oracle.py,
autograd), computed once per module; training-mode cases run the oracle with the dropout factors the child exported.
Bounds, none of them new: fp32 outputs rel_err < 2e-5, weight gradients as test_hip_backward.py::_check_grads, input
and edge-feature gradients rel_err < 2e-4; bf16 as test_bf16_storage.py (outputs 1e-2, gradients 2e-2 in L2 with the
2e-3 * scale floor); the drug encoder as test_gine_depth4.py / test_gine_edge_grad.py (2e-5, 2e-4).  More trips only
reorder sums of the same terms over at most 25 tiles.

The CPU tests at the bottom restate the host's launch formulas and assert that every (case, setting) is in the regime
it is here for -- and that the default setting is NOT -- so a change of the workgroup shapes or caps says that the
shapes need revisiting; and that every environment name used is one the library reads."""
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
from conftest import GOLDEN, REPO, load_npz, rel_err
from oracle import gvp_oracle as O

DEV = "cuda:0"
T = torch.from_numpy
FWD_TOL, GRAD_TOL, IN_TOL = 2e-5, 2e-4, 2e-4        # test_hip_backward.py
FWD_TOL_BF16, GRAD_TOL_BF16 = 1e-2, 2e-2            # test_bf16_storage.py
DRUG_FWD_TOL, DRUG_GRAD_TOL = 2e-5, 2e-4            # test_gine_depth4.py::_compare, test_gine_edge_grad.py
P_DROP = 0.2

# id -> (environment, autograd_ops.GINE_BWD_WORKGROUPS, runs the drug cases, runs the deterministic variants)
SETTINGS = {
    "default": ({}, 0, True, True),
    "grid1": ({"CGVP_BWD_GRID": "1", "CGVP_CONV_FWD_WAVES": "4", "CGVP_GINE_FWD_WGS": "1"}, 1, True, True),
    "grid3": ({"CGVP_BWD_GRID": "3", "CGVP_CONV_FWD_WAVES": "8", "CGVP_GINE_FWD_WGS": "2"}, 3, True, True),
    # the A/B kernels have no deterministic form (test_deterministic.py checks that they say so)
    "grid1-ab": ({"CGVP_BWD_GRID": "1", "CGVP_CONV_BWD": "2", "CGVP_SPLIT_HEAD_BWD": "1", "CGVP_GINE_RECOMPUTE": "1"},
                 1, True, False),
    "grid1-r3": ({"CGVP_BWD_GRID": "1", "CGVP_CONV_BWD": "1"}, 0, False, False),
}
SWITCHES = sorted({k for env, *_ in SETTINGS.values() for k in env} | {"CGVP_BWD_STORE_ONCE", "CGVP_DETERMINISTIC"})
PROTEIN_CASES = {"sparse": "sum", "knn": "mean", "hub": "sum"}         # case -> aggr
BF16_CASES = ("sparse", "knn")
HUB, HUB_LOST = 100, (0, 30, 31, 390)       # the hub node; the nodes that lose every incoming edge (0: a one-node graph)


# ------------------------------------------------------------------------------------------------ cases
def _hub_edges(gb):
    """The `sparse` batch's edge tables with node HUB made a hub of its graph -- an edge from every node of the graph
    and one to each -- and HUB_LOST left without incoming edges (self loops included).  The added edges stand behind
    the original ones (the edge list is then no longer sorted by source); their features are made the way davis_synth
    makes its own, from a seeded distance and direction."""
    g = int(np.searchsorted(gb.ptr, HUB, side="right") - 1)
    nodes = np.arange(gb.ptr[g], gb.ptr[g + 1])
    have = set(map(tuple, gb.edge_index.T.tolist()))
    new = [(int(j), HUB) for j in nodes if (int(j), HUB) not in have] + \
          [(HUB, int(j)) for j in nodes if (HUB, int(j)) not in have]
    new = np.asarray(new, dtype=np.int64).T
    rng = np.random.default_rng(1009)
    dist = rng.uniform(4.0, ds.RBF_MAX, size=new.shape[1])
    mu = np.linspace(0.0, ds.RBF_MAX, ds.RBF_COUNT)
    rbf = np.exp(-np.square((dist[:, None] - mu[None, :]) / (ds.RBF_MAX / ds.RBF_COUNT)))
    e_s = np.concatenate([rbf, ds._pos_encoding((new[1] - new[0]).astype(np.float64))], -1).astype(np.float32)
    e_v = ds._unit(rng.normal(size=(new.shape[1], 3)))[:, None, :].astype(np.float32)
    ei = np.concatenate([gb.edge_index, new], 1)
    e_s, e_v = np.concatenate([gb.e_s, e_s]), np.concatenate([gb.e_v, e_v])
    keep = ~np.isin(ei[1], HUB_LOST)
    return ei[:, keep], e_s[keep], e_v[keep], np.zeros(int(keep.sum()), np.int64)


_CASES = {}


def _case(name):
    """-> the case's tensors on the CPU, fp32: x (x_s, x_v), eattr (e_s, e_v), edge_index, ntypes, etypes (protein) or
    x, eattr, edge_index, ntypes, etypes (drug); r, the upstream gradient, is drawn by _upstream."""
    if name not in _CASES:
        if name == "drug":
            d = ds.to_torch(ds.drug_batch(12, 5))
        elif name == "knn":
            d = ds.to_torch(ds.protein_batch(2, 42, lengths=[200, 195], thresh=12, thresh_type="num"))
        else:
            gb = ds.protein_batch(3, 41, lengths=[1, 200, 190])
            d = ds.to_torch(gb)
            if name == "hub":
                ei, e_s, e_v, et = _hub_edges(gb)
                d = dict(d, edge_index=T(np.ascontiguousarray(ei)), eattr=(T(e_s), T(e_v)), etypes=T(et))
        _CASES[name] = d
    return _CASES[name]


def _upstream(name, variant):
    """The upstream gradient of (case, variant): the same seeded draw in the child and in the parent."""
    n = (_case(name)["x"] if name == "drug" else _case(name)["x"][0]).shape[0]
    seed = 100 * sorted(list(PROTEIN_CASES) + ["drug"]).index(name) + ("f32", "bf16", "train").index(variant)
    return torch.randn(n, 64, generator=torch.Generator().manual_seed(seed))


def _bf(d):
    """bf16 storage: the features rounded to bf16, widened again (the child narrows them back without loss)."""
    c = lambda t: t.to(torch.bfloat16).float()
    return dict(d, x=tuple(c(t) for t in d["x"]), eattr=tuple(c(t) for t in d["eattr"]))


def _protein_state():
    pfx = "protein_gnn.gnn_model."
    return {k[len(pfx):]: T(v) for k, v in load_npz("pretrained_state.npz").items() if k.startswith(pfx)}


def _drug_model():
    """The four-layer drug encoder of test_gine_depth4.py::_mol44 (52 -> 16 -> 16 -> 16 -> 64: every compiled layer
    shape), seeded default initialisation, eps non-zero; on the CPU."""
    from models.molecule_gnn import SelectableMoleculeModelWrapper
    kw = json.load(open(os.path.join(GOLDEN, "model_kwargs.json")))["molecule_gnn_kwargs"]
    torch.manual_seed(44)
    m = SelectableMoleculeModelWrapper(**dict(kw, num_convs=4))
    with torch.no_grad():
        for l, conv in enumerate(m.gnn_model.conv_list):
            conv.eps.fill_(0.05 * (l + 1))
    assert m.gnn_model._widths == [52, 16, 16, 16, 64] and float(m.gnn_model.dropout_rate) == P_DROP
    return m


# ------------------------------------------------------------------------------------------------ the child
class _Deterministic:
    def __enter__(self):
        self.was = torch.are_deterministic_algorithms_enabled()
        torch.use_deterministic_algorithms(True)

    def __exit__(self, *a):
        torch.use_deterministic_algorithms(self.was)


def _protein_pass(model, d, r, dt, res, key, edge_grad=True):
    """One forward + backward on the GPU; output, every parameter gradient and the input gradients -> res[key + ..]."""
    model.zero_grad(set_to_none=True)
    leaf = lambda t, grad: t.to(DEV).to(dt).requires_grad_(grad)
    xs, xv = leaf(d["x"][0], True), leaf(d["x"][1], True)
    es, ev = leaf(d["eattr"][0], edge_grad), leaf(d["eattr"][1], edge_grad)
    out = model((xs, xv), d["edge_index"].to(DEV), d["ntypes"].to(DEV), d["etypes"].to(DEV), eattr=(es, ev))
    assert out.dtype == dt
    if model.training:                        # {seed, offset} of this pass: read before anything else runs
        from gvp_hip import autograd_ops, ops
        seed = autograd_ops.last_seed("lba")
        res[key + "masks"] = ops.dropout_masks(seed, P_DROP, 0, 4, xs.shape[0], 20).cpu().numpy()
    (out.float() * r.to(DEV)).sum().backward()
    res[key + "out"] = out.detach().float().cpu().numpy()
    res[key + "gin.x_s"], res[key + "gin.x_v"] = xs.grad.float().cpu().numpy(), xv.grad.float().cpu().numpy()
    if edge_grad:
        res[key + "gin.e_s"], res[key + "gin.e_v"] = es.grad.float().cpu().numpy(), ev.grad.float().cpu().numpy()
    for name, p in model.gnn_model.named_parameters():
        if p.numel():
            assert p.grad.dtype == torch.float32
            res[key + "g." + name] = p.grad.cpu().numpy()


def _drug_pass(model, d, r, res, key):
    model.zero_grad(set_to_none=True)
    gx, ge = d["x"].to(DEV).requires_grad_(), d["eattr"].to(DEV).requires_grad_()
    out = model(gx, d["edge_index"].to(DEV), d["ntypes"].to(DEV), d["etypes"].to(DEV), eattr=ge)
    if model.training:
        from gvp_hip import autograd_ops, ops
        seed = autograd_ops.last_seed("gine")
        res[key + "masks"] = np.stack([ops.dropout_masks(seed, P_DROP, l, 1, gx.shape[0], 16)[0].cpu().numpy()
                                       for l in range(3)])
    (out * r.to(DEV)).sum().backward()
    res[key + "out"] = out.detach().cpu().numpy()
    res[key + "gin.x"], res[key + "gin.eattr"] = gx.grad.cpu().numpy(), ge.grad.cpu().numpy()
    for name, p in model.gnn_model.named_parameters():
        res[key + "g." + name] = p.grad.cpu().numpy()


def _child_main(setting, out_path):
    """Runs in the child: every case and variant of `setting` on the GPU -> one .npz."""
    from gvp_hip import autograd_ops
    from test_hip_backward import _encoder
    env, gine_wgs, with_drug, with_det = SETTINGS[setting]
    assert all(os.environ.get(k) == v for k, v in env.items()) and not any(k in os.environ for k in SWITCHES if k not in env)
    autograd_ops.GINE_BWD_WORKGROUPS = gine_wgs
    state, res = _protein_state(), {}
    for case, aggr in PROTEIN_CASES.items():
        d = _case(case)
        model = _encoder(state, 2, aggr, dropout=0.0).eval()
        _protein_pass(model, d, _upstream(case, "f32"), torch.float32, res, f"{case}.f32.")
        if with_det:
            for run in ("det", "det2"):
                with _Deterministic():
                    _protein_pass(model, d, _upstream(case, "f32"), torch.float32, res, f"{case}.{run}.")
        if case in BF16_CASES:                  # (no edge-feature gradient: the bf16 bounds of the suite name none)
            _protein_pass(model, _bf(d), _upstream(case, "bf16"), torch.bfloat16, res, f"{case}.bf16.", edge_grad=False)
    model = _encoder(state, 2, "sum", dropout=P_DROP).train()
    _protein_pass(model, _case("sparse"), _upstream("sparse", "train"), torch.float32, res, "sparse.train.")
    if with_drug:
        d = _case("drug")
        mol = _drug_model().to(DEV).eval()
        for k, v in mol.gnn_model.state_dict().items():
            res["drug.state." + k] = v.cpu().numpy()
        _drug_pass(mol, d, _upstream("drug", "f32"), res, "drug.f32.")
        if with_det:
            for run in ("det", "det2"):
                with _Deterministic():
                    _drug_pass(mol, d, _upstream("drug", "f32"), res, f"drug.{run}.")
        _drug_pass(mol.train(), d, _upstream("drug", "train"), res, "drug.train.")
    torch.cuda.synchronize()
    np.savez(out_path, **res)


_CHILD = r"""
import os, sys
sys.path.insert(0, {pkg!r}); sys.path.insert(0, {repo!r}); sys.path.insert(0, os.path.join({repo!r}, "tests"))
import test_persistent_loops as L
L._child_main(sys.argv[1], sys.argv[2])
print("ok")
"""

_child_failed = []          # a child that crashed or ran out of time: no further child is started in this session
_results = {}               # setting -> the child's arrays (a setting runs once per session)


def _run_child(setting, tmp_dir):
    if setting in _results:
        return _results[setting]
    if _child_failed:
        pytest.fail(f"not started: the child for {_child_failed[0]} failed before")
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(SETTINGS[setting][0])
    out = tmp_dir / f"{setting}.npz"
    code = _CHILD.format(pkg=os.path.join(REPO, "caster-dta_amd"), repo=REPO)
    try:
        res = subprocess.run([sys.executable, "-c", code, setting, str(out)], env=env, capture_output=True, text=True,
                             timeout=300)
    except subprocess.TimeoutExpired:
        _child_failed.append(setting)
        raise
    if not (res.returncode == 0 and res.stdout.strip().endswith("ok")):
        _child_failed.append(setting)
        pytest.fail(f"child failed: {res.returncode}\n{res.stderr[-3000:]}")
    _results[setting] = dict(np.load(out))
    return _results[setting]


@pytest.fixture(scope="module")
def child_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("persistent_loops")


# ------------------------------------------------------------------------------------------------ the oracle
def _protein_oracle(d, aggr, r, bf16=False, masks=None):
    P = {k: v.clone().requires_grad_(v.numel() > 0) for k, v in _protein_state().items()}
    x = tuple(t.clone().requires_grad_() for t in d["x"])
    e = tuple(t.clone().requires_grad_() for t in d["eattr"])
    kw = dict(num_convs=2, aggr=aggr)
    if masks is not None:
        kw["masks"] = [(masks[0], masks[1]), (masks[2], masks[3])]
    if bf16:
        with O.emulate_gemm_dtype(torch.bfloat16):
            ref = O.protein_lba_forward(P, x, d["edge_index"], d["ntypes"], d["etypes"], e, store_dtype=torch.bfloat16, **kw)
            (ref * r).sum().backward()
    else:
        ref = O.protein_lba_forward(P, x, d["edge_index"], d["ntypes"], d["etypes"], e, **kw)
        (ref * r).sum().backward()
    return dict(out=ref.detach(), g={k: v.grad for k, v in P.items() if v.numel()},
                gin={"x_s": x[0].grad, "x_v": x[1].grad, "e_s": e[0].grad, "e_v": e[1].grad})


def _drug_oracle(r, masks=None):
    d = _case("drug")
    P = {k: v.detach().clone().requires_grad_(True) for k, v in _drug_model().gnn_model.state_dict().items()}
    x, e = d["x"].clone().requires_grad_(), d["eattr"].clone().requires_grad_()
    ref = O.molecule_gine_forward(P, x, d["edge_index"], d["ntypes"], d["etypes"], e, num_convs=4, masks=masks)
    (ref * r).sum().backward()
    assert bool((e.grad.abs().amax(0) > 0).all()), "a bond-feature column without gradient: the check would be vacuous"
    return dict(out=ref.detach(), g={k: v.grad for k, v in P.items()}, gin={"x": x.grad, "eattr": e.grad},
                state={k: v.detach() for k, v in P.items()})


@pytest.fixture(scope="module")
def oracle_refs():
    """(case, 'f32' | 'bf16') -> output, parameter gradients and input gradients of the CPU oracle, eval mode; computed
    once and left unchanged.  (The training-mode references depend on each child's exported masks: _train_ref.)"""
    refs = {}
    for case, aggr in PROTEIN_CASES.items():
        refs[(case, "f32")] = _protein_oracle(_case(case), aggr, _upstream(case, "f32"))
        if case in BF16_CASES:
            refs[(case, "bf16")] = _protein_oracle(_bf(_case(case)), aggr, _upstream(case, "bf16"), bf16=True)
    refs[("drug", "f32")] = _drug_oracle(_upstream("drug", "f32"))
    return refs


def _masks_ok(m):
    """exported dropout factors: 0 or 1 / (1 - p), drop rate near p -- dropout really was applied"""
    assert set(np.unique(m).round(4)) == {0.0, round(1 / (1 - P_DROP), 4)}
    assert abs(float((m == 0).mean()) - P_DROP) < 0.05
    return T(m)


# ------------------------------------------------------------------------------------------------ the bounds
def _figures_f32(z, key, ref):
    """-> [(what, error, bound, strict)]: outputs 2e-5; weight gradients as test_hip_backward.py::_check_grads (<=);
    node- and edge-feature gradients 2e-4."""
    figs = [(key + "out", rel_err(z[key + "out"], ref["out"]), FWD_TOL, True)]
    scale = max(float(v.abs().max()) for v in ref["g"].values())
    for name, want in ref["g"].items():
        err = float((T(z[key + "g." + name]) - want).abs().max())
        figs.append((key + "g." + name, err, GRAD_TOL * float(want.abs().max()) + 2e-6 * scale, False))
    for name, want in ref["gin"].items():
        figs.append((key + "gin." + name, rel_err(z[key + "gin." + name], want), IN_TOL, True))
    return figs


def _figures_bf16(z, key, ref):
    """-> [(what, error, bound, strict)] as test_bf16_storage.py::test_bf16_forward_backward_vs_oracle states them."""
    figs = [(key + "out", rel_err(z[key + "out"], ref["out"]), FWD_TOL_BF16, True)]
    scale = max(float(v.abs().max()) for v in ref["g"].values())
    for name, want in ref["g"].items():
        err = (float((T(z[key + "g." + name]) - want).norm()) - 2e-3 * scale) / max(float(want.norm()), 1e-30)
        figs.append((key + "g." + name, err, GRAD_TOL_BF16, False))
    for name in ("x_s", "x_v"):
        want = ref["gin"][name]
        figs.append((key + "gin." + name, float((T(z[key + "gin." + name]) - want).norm() / want.norm()), GRAD_TOL_BF16, True))
    return figs


def _figures_drug(z, key, ref):
    """-> [(what, error, bound, strict)] as test_gine_edge_grad.py::_check_all: output 2e-5, everything else 2e-4."""
    figs = [(key + "out", rel_err(z[key + "out"], ref["out"]), DRUG_FWD_TOL, True)]
    for name, want in ref["g"].items():
        figs.append((key + "g." + name, rel_err(z[key + "g." + name], want), DRUG_GRAD_TOL, True))
    for name, want in ref["gin"].items():
        assert z[key + "gin." + name].shape == tuple(want.shape)
        figs.append((key + "gin." + name, rel_err(z[key + "gin." + name], want), DRUG_GRAD_TOL, True))
    return figs


def _judge(setting, key, figs, bad):
    for kind, sel in (("output", [f for f in figs if f[0] == key + "out"]), ("gradient", [f for f in figs if f[0] != key + "out"])):
        what, err, bound, _ = max(sel, key=lambda f: f[1] / f[2])
        print(f"{setting} {key} {kind} closest to its bound: {what} {err:.2e} (bound {bound:.2e})")
    bad += [f[:3] for f in figs if not (f[1] < f[2] if f[3] else f[1] <= f[2])]


def _same_bits(z, a, b):
    keys = sorted(k[len(a):] for k in z if k.startswith(a))
    assert keys and keys == sorted(k[len(b):] for k in z if k.startswith(b))
    return [k for k in keys if not np.array_equal(z[a + k], z[b + k])]


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_multi_trip_loops_match_the_oracle(setting, oracle_refs, child_dir):
    z = _run_child(setting, child_dir)
    _, _, with_drug, with_det = SETTINGS[setting]
    bad = []
    for case, aggr in PROTEIN_CASES.items():
        ref = oracle_refs[(case, "f32")]
        _judge(setting, f"{case}.f32.", _figures_f32(z, f"{case}.f32.", ref), bad)
        if with_det:
            assert not _same_bits(z, f"{case}.det.", f"{case}.det2."), "deterministic mode: two runs differ"
            for run in ("det", "det2"):
                _judge(setting, f"{case}.{run}.", _figures_f32(z, f"{case}.{run}.", ref), bad)
        if case in BF16_CASES:
            _judge(setting, f"{case}.bf16.", _figures_bf16(z, f"{case}.bf16.", oracle_refs[(case, "bf16")]), bad)
    # training mode: the oracle applies the factors the kernels drew (exported for the pass's seed); a row of a wave's
    # second tile must have been keyed by its global node index, like every other row
    masks = _masks_ok(z["sparse.train.masks"])
    ref = _protein_oracle(_case("sparse"), "sum", _upstream("sparse", "train"), masks=masks)
    assert rel_err(ref["out"], oracle_refs[("sparse", "f32")]["out"]) > 1e-2
    _judge(setting, "sparse.train.", _figures_f32(z, "sparse.train.", ref), bad)
    if with_drug:
        ref = oracle_refs[("drug", "f32")]
        for k, v in ref["state"].items():                           # the child built the same model
            assert np.array_equal(z["drug.state." + k], v.numpy()), k
        _judge(setting, "drug.f32.", _figures_drug(z, "drug.f32.", ref), bad)
        if with_det:
            assert not _same_bits(z, "drug.det.", "drug.det2."), "deterministic mode: two runs differ"
            for run in ("det", "det2"):
                _judge(setting, f"drug.{run}.", _figures_drug(z, f"drug.{run}.", ref), bad)
        masks = _masks_ok(z["drug.train.masks"])
        tref = _drug_oracle(_upstream("drug", "train"), masks=list(masks))
        _judge(setting, "drug.train.", _figures_drug(z, "drug.train.", tref), bad)
    else:
        assert not any(k.startswith("drug.") for k in z)
    assert not bad, bad


@pytest.mark.gpu
def test_the_grid_knob_took_effect(oracle_refs, child_dir):
    """Deterministic mode repeats bitwise within a setting, so a difference between two settings is the launch shape's:
    with one workgroup the weight gradients of `sparse` are summed over another partition into waves than with the
    default grid, and must differ from it in at least one bit (both agree with the oracle: the test above).  Children
    that ignored their environment would be five default runs."""
    base, one = _run_child("default", child_dir), _run_child("grid1", child_dir)
    for z in (base, one):
        assert not _same_bits(z, "sparse.det.", "sparse.det2.")
    names = [k for k in base if k.startswith("sparse.det.g.")]
    assert len(names) >= 60
    assert any(not np.array_equal(base[k], one[k]) for k in names)


# ------------------------------------------------------------------------------------------------ CPU: regimes
TILE, BW_WPB, BW_MAX_GRID, GF_WPB, GINE_BWD_DEFAULT_GRID = 16, 8, 240, 8, 16
C2_SHAPES = {3: (1, 8), 2: (2, 4)}          # CGVP_CONV_BWD -> (TN tiles in lockstep, waves per workgroup) of conv_bwd2_kernel


def _ceil(a, b):
    return -(-a // b)


def _bwd_grid_cap(units, forced):
    """gvp_quad_bwd_kernels.hip::bwd_grid_cap"""
    if forced:
        return forced
    small = BW_MAX_GRID - 8
    return small if units <= small * BW_WPB else BW_MAX_GRID


def _node_stage(N, forced):
    """node_bwd / node_head_bwd / head_bwd / embed_bwd: -> (tiles, waves, most tiles of one wave, ONE)."""
    tiles = _ceil(N, TILE)
    G = max(1, min(tiles, _bwd_grid_cap(tiles, forced)))
    return tiles, G * BW_WPB, _ceil(tiles, G * BW_WPB), tiles <= G * BW_WPB


def _conv_bwd2(E, forced, version=3):
    """conv_bwd2_impl + the kernel's ranges: -> (iters, waves, ipw, chunk = positions of one wave's range)."""
    tn, wpb = C2_SHAPES[version]
    iters = _ceil(E, tn * TILE)
    G = max(1, min(_ceil(iters, wpb), _bwd_grid_cap((_ceil(E, TILE) + 1) // 2, forced)))
    waves = G * wpb
    ipw = _ceil(iters, waves)
    return iters, waves, ipw, ipw * tn * TILE


def _conv_bwd_r3(N, E, forced):
    """conv_bwd + conv_bwd_impl (the round-3 kernel: target groups round-robin): -> most groups of one wave."""
    deg = max(1, _ceil(E, N))
    npw = min(64, max(1, (2 * TILE - 2) // deg))
    groups = _ceil(N, npw)
    G = max(1, min(_ceil(groups, BW_WPB), _bwd_grid_cap(groups, forced)))
    return _ceil(groups, G * BW_WPB)


def _edge_bwd(E, forced):
    """edge_bwd_impl: two workgroups per CU -> most tiles of one wave."""
    tiles = _ceil(E, TILE)
    G = max(1, min(tiles, 2 * _bwd_grid_cap((tiles + 1) // 2, forced)))
    return _ceil(tiles, G * BW_WPB)


def _gine(N, fwd_cap, bwd_cap, wpb):
    """launch_fwd / launch_bwd of gine_quad_kernels.hip: -> most tiles of one wave (forward, backward).  The backward's
    waves per workgroup depend on the layer shape (what one CU's LDS holds, 8 at the most)."""
    tiles = _ceil(N, TILE)
    gf = max(1, min(_ceil(tiles, GF_WPB), fwd_cap or 1024))
    gb = max(1, min(_ceil(tiles, wpb), bwd_cap or GINE_BWD_DEFAULT_GRID))
    return _ceil(tiles, gf * GF_WPB), _ceil(tiles, gb * wpb)


def _sizes(case):
    d = _case(case)
    ei = d["edge_index"].numpy()
    N = (d["x"] if case == "drug" else d["x"][0]).shape[0]
    return N, ei.shape[1], np.bincount(ei[1], minlength=N)


def test_the_cases_are_what_the_regimes_need():
    N, E, deg = _sizes("sparse")
    assert (N, E) == (391, 1167) and N % TILE == 7 and E % TILE == 15 and E <= 4 * N          # fused layers
    N, E, deg = _sizes("knn")
    assert (N, E) == (395, 4740) and N % TILE and E % TILE and E > 4 * N                       # two-launch layers
    N, E, deg = _sizes("hub")
    assert N == 391 and E % TILE and E <= 4 * N and deg[HUB] >= 199 and all(deg[n] == 0 for n in HUB_LOST)
    ei = _case("hub")["edge_index"].numpy()
    assert (np.diff(ei[0]) < 0).any() and len(set(map(tuple, ei.T.tolist()))) == E            # unsorted, no duplicates
    assert int((ei[0] == HUB).sum()) >= 199 - 2
    N, E, deg = _sizes("drug")
    assert (N, E) == (488, 1514) and N % TILE == 8


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_every_setting_is_in_its_regime(setting):
    """The host formulas restated (16 rows per tile, 8 waves per backward workgroup, 8 / 4 waves for the conv backward's
    TN = 1 / TN = 2 shapes): which trips every (case, setting) runs."""
    env, gine_bwd, with_drug, with_det = SETTINGS[setting]
    forced = int(env.get("CGVP_BWD_GRID", 0))
    version = int(env.get("CGVP_CONV_BWD", 3))
    multi = forced > 0
    for case in PROTEIN_CASES:
        N, E, deg = _sizes(case)
        rowptr = np.concatenate([[0], np.cumsum(deg)])
        tiles, waves, trips, one = _node_stage(N, forced)
        assert N % TILE                                                             # a ragged last tile
        assert (trips > 1) == multi and one == (not multi), (case, tiles, waves, trips)
        assert (_edge_bwd(E, forced) > 1) == multi
        if forced == 1:
            assert trips == 4 and tiles - 3 * waves == 1                            # wave 0: four trips, the others three
        if forced == 3:
            assert tiles == waves + 1 and trips == 2                                # ONE wave with a second tile
        if version == 1:
            assert _conv_bwd_r3(N, E, forced) > 1
            continue
        for v in sorted({version, 3} if with_det else {version}):                   # deterministic mode: the default kernel's STORE form
            iters, cwaves, ipw, chunk = _conv_bwd2(E, forced, v)
            assert (ipw > 1) == multi, (case, iters, cwaves, ipw)
            assert E % (C2_SHAPES[v][0] * TILE)                                     # a ragged last iteration
            spans = [int(_ceil(rowptr[n + 1], chunk) - rowptr[n] // chunk) for n in range(N) if deg[n]]
            if multi:
                assert max(spans) >= 2                                              # a target carried across a range border
            if multi and case == "hub":
                # owned NODES (an even split over the waves): a range of several nodes with and without incoming edges
                own = _ceil(N, cwaves)
                assert own > 1 and any(0 < np.count_nonzero(deg[n0:n0 + own] == 0) < len(deg[n0:n0 + own])
                                       for n0 in range(0, N, own))
            if case != "hub":
                assert deg.min() >= 1
            if forced == 3 and case == "sparse":
                assert (iters, ipw) == (73, 4) and _ceil(iters, ipw) < cwaves       # the last waves own an empty range
            if forced == 3 and case == "hub" and v == 3:
                # >= 3 ranges: a wave whose whole range lies inside the hub, two boundary slots for src_sum_kernel
                assert chunk == 80 and max(spans) >= 3 and spans[[n for n in range(N) if deg[n]].index(HUB)] >= 3
            if forced == 1 and case == "sparse" and v == 3:
                assert ipw == 10
    if with_drug:
        N, E, deg = _sizes("drug")
        assert N % TILE
        fwd_cap = int(env.get("CGVP_GINE_FWD_WGS", 0))
        # the backward's waves per workgroup (GineQ::WPB: what one CU's LDS holds): 8 for the 16-wide layers, 5 for the
        # last one (16 -> 64 -> 64)
        trips = [_gine(N, fwd_cap, gine_bwd, wpb) for wpb in (8, 5)]
        if multi:
            assert all(b > 1 and (f > 1) == (fwd_cap > 0) for f, b in trips), trips
            if setting == "grid1":
                assert trips == [(4, 4), (4, 7)]
            if setting == "grid3":
                assert trips == [(2, 2), (2, 3)]
        else:
            assert trips == [(1, 1), (1, 1)] and _gine(N, 0, 0, 2) == (1, 1)       # (any shape with two waves or more)


def test_every_knob_is_one_the_library_reads():
    """Each environment name used above is a getenv("...") literal of the library's sources: a renamed knob fails here
    and does not turn the children into default runs."""
    read = set()
    for path in glob.glob(os.path.join(REPO, "caster-dta_amd", "csrc", "*")):
        read |= set(re.findall(r'getenv\("(\w+)"\)', open(path, errors="replace").read()))
    used = {k for env, *_ in SETTINGS.values() for k in env}
    assert used == {"CGVP_BWD_GRID", "CGVP_CONV_FWD_WAVES", "CGVP_GINE_FWD_WGS", "CGVP_CONV_BWD", "CGVP_SPLIT_HEAD_BWD",
                    "CGVP_GINE_RECOMPUTE"}
    assert used <= read, used - read
    from gvp_hip import autograd_ops
    assert autograd_ops.GINE_BWD_WORKGROUPS == 0
    assert re.search(r"\bGINE_BWD_WORKGROUPS\)", open(autograd_ops.__file__).read())      # forwarded to the passes
