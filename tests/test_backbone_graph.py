"""Backbone atoms -> protein graph on the device (csrc/structure_kernels.hip, include/caster_gvp_structure.h,
gvp_hip.structure.protein_graphs).

PINNED by tests/golden/backbone_graphs.npz: what the reference's own `compute_residue_node_features`,
`compute_residue_edge_features` (utils/create_protein_features.py:12, :201) and `construct_graph`
(utils/create_graphs.py:6) give for the float64 up-cast of float32 backbones (recipe: tests/golden/
make_backbone_golden.py).  The float64 NumPy restatement below is itself checked against that fixture on the CPU and
then serves where the fixture holds no case (the tie at the k-th neighbour, the end-to-end graph, the timing tool).

Tolerances.  Edge lists are compared EXACTLY: the recipe and `test_fixture_keeps_clear_of_every_threshold` assert that
no pair lies within 1e-4 A of a radius and no k-th / (k+1)-th neighbour distances are closer than 1e-4 A, while the
device compares fp64 squared distances of the same fp32 inputs (relative error ~1e-16).  Node features are computed in
fp64 on the device and rounded once to fp32 (6e-8 on [-1, 1] values); the edge features keep the 2e-6 absolute bound
tests/test_edge_featurise.py states for cgvp_edge_featurise.  2e-6 absolute is asserted for all four tensors, and the
fixture's exact zeros (chain ends, zero directions, sin of the padded angles) must be exact zeros.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import davis_synth as ds
from conftest import GOLDEN, REPO, load_npz, rel_err

DEV = "cuda:0"
CASES = ("helixish", "tiny1", "tiny2", "short37", "coincident", "knn30", "knn_short", "noself", "all_types")
OLD_CASES = {"radius4": (4.0, "dist"), "coincident": (6.0, "dist"), "box_far_in_sequence": (4.5, "dist"), "knn12": (12, "num")}
NEW_SYMBOLS = ("cgvp_structure_version", "cgvp_node_featurise", "cgvp_radius_graph_count", "cgvp_knn_graph_select",
               "cgvp_graph_fill")
TOL = 2e-6


# ---------------------------------------------------------------------------------------------------------------------
# float64 NumPy restatement of utils/create_protein_features.py:27-92, :225-331 and utils/create_graphs.py:29,44-45
def _unit(v):
    n = np.linalg.norm(v, axis=-1, keepdims=True)
    return np.divide(v, n, out=np.zeros_like(v), where=n != 0)


def numpy_node_features(coords, types, props):
    c = coords.astype(np.float64)
    L = c.shape[0]
    chain = c[:, :3].reshape(-1, 3)                                        # N, CA, C, N, CA, C, ...
    step = _unit(chain[1:] - chain[:-1])
    u0, u1, u2 = step[2:], step[1:-1], step[:-2]
    n1, n2 = _unit(np.cross(u1, u0)), _unit(np.cross(u2, u1))
    ang = np.arccos(np.clip((n1 * n2).sum(-1), -1.0, 1.0)) * np.sign((n1 * u2).sum(-1))
    ang = np.pad(ang, [1, 2]).reshape(-1, 3)                               # first phi, last psi / omega: angle 0
    ca = c[:, 1]
    fwd = _unit(ca[1:] - ca[:-1])
    x_v0 = np.pad(fwd, [(0, 1), (0, 0)])
    x_v1 = np.pad(-fwd, [(1, 0), (0, 0)])
    dn, dc = _unit(c[:, 0] - ca), _unit(c[:, 2] - ca)
    side = -_unit(dn + dc) * np.sqrt(1 / 3) - _unit(np.cross(dc, dn)) * np.sqrt(2 / 3)
    x_s = np.concatenate([np.cos(ang), np.sin(ang), props.astype(np.float64)[types].reshape(L, -1)], axis=-1)
    return x_s, np.stack([x_v0, x_v1, side], axis=1)


def numpy_edge_list(ca, thresh, kind, self_loops=True):
    ca = ca.astype(np.float64)
    L = ca.shape[0]
    d = np.linalg.norm(ca[:, None] - ca[None], axis=-1)
    if not self_loops:
        d[np.arange(L), np.arange(L)] = np.nan                             # :279-282; NaN sorts last, compares false
    if kind == "dist":
        with np.errstate(invalid="ignore"):
            keep = d <= thresh
    else:
        keep = np.zeros((L, L), dtype=bool)
        keep[np.arange(L)[:, None], np.argsort(d, axis=-1, kind="stable")[:, :int(thresh)]] = True
        keep &= ~np.isnan(d)
    src, dst = np.nonzero(keep)                                            # row-major: the reference's COO order
    return np.stack([src, dst]).astype(np.int64)


def numpy_edge_features(ca, seq, ei):
    i, j = ei[0], ei[1]
    diff = ca[i].astype(np.float64) - ca[j].astype(np.float64)
    d = np.linalg.norm(diff, axis=-1)
    rbf = np.exp(-np.square((d[:, None] - np.linspace(0.0, 20.0, 16)[None, :]) / (20.0 / 16)))
    freqs = np.exp(2 * np.arange(8) * -(np.log(10000.0) / 8))
    ang = (seq[j] - seq[i]).astype(np.float64)[:, None] * freqs
    return np.concatenate([rbf, np.cos(ang), np.sin(ang)], -1), _unit(diff)[:, None, :]


def numpy_protein_graph(coords, types, props, thresh, kind, self_loops=True):
    """One graph, float64: (x_s, x_v, edge_index, e_s, e_v)."""
    x_s, x_v = numpy_node_features(coords, types, props)
    ei = numpy_edge_list(coords[:, 1], thresh, kind, self_loops)
    e_s, e_v = numpy_edge_features(coords[:, 1], np.arange(coords.shape[0]), ei)
    return x_s, x_v, ei, e_s, e_v


def threshold_gap(ca, thresh, kind):
    ca = ca.astype(np.float64)
    d = np.linalg.norm(ca[:, None] - ca[None], axis=-1)
    if kind == "dist":
        return float(np.abs(d - thresh).min())
    k = int(thresh)
    if d.shape[0] <= k:
        return float("inf")
    s = np.sort(d, axis=-1)
    return float((s[:, k] - s[:, k - 1]).min())


@pytest.fixture(scope="module")
def gold():
    return load_npz("backbone_graphs.npz")


def case_of(g, name):
    return (g[f"{name}_coords"], g[f"{name}_types"], float(g[f"{name}_thresh"]), str(g[f"{name}_kind"]),
            bool(g[f"{name}_self_loops"]))


# ---------------------------------------------------------------------------------------------------------------------
# CPU
def test_numpy_restatement_matches_reference_fixture(gold):
    for name in CASES:
        coords, types, thresh, kind, loops = case_of(gold, name)
        assert coords.dtype == np.float32 and coords.shape[1:] == (4, 3)
        x_s, x_v, ei, e_s, e_v = numpy_protein_graph(coords, types, gold["aa_props"], thresh, kind, loops)
        assert np.array_equal(ei, gold[f"{name}_edge_index"]), name
        for mine, key in ((x_s, "x_s"), (x_v, "x_v"), (e_s, "e_s"), (e_v, "e_v")):
            want = gold[f"{name}_{key}"]
            assert mine.shape == want.shape and float(np.abs(mine - want).max()) < 1e-6, (name, key)   # fixture is float32
    assert gold["aa_props"].shape == (21, 11) and set(gold["all_types_types"].tolist()) == set(range(21))
    # what the cases are there for
    assert gold["tiny1_x_s"][0, :6].tolist() == [1, 1, 1, 0, 0, 0] and not gold["tiny1_x_v"][0, :2].any()
    assert gold["knn30_edge_index"].shape[1] == 200 * 30 and gold["knn_short_edge_index"].shape[1] == 20 * 20
    ei = gold["noself_edge_index"]
    assert (ei[0] != ei[1]).all()
    co = gold["coincident_coords"]
    assert (co[3, 0] == co[3, 1]).all() and (co[11, 1] == co[10, 1]).all() and (co[21, 0] == co[20, 2]).all()


def test_fixture_keeps_clear_of_every_threshold(gold):
    """No pair within 1e-4 A of a radius, no k-th / (k+1)-th neighbour distances closer than 1e-4 A -- in the new
    fixture and in the four edge_feats.npz cases the GPU tests build edge lists for."""
    for name in CASES:
        coords, _, thresh, kind, _ = case_of(gold, name)
        assert threshold_gap(coords[:, 1], thresh, kind) > 1e-4, name
    old = load_npz("edge_feats.npz")
    for name, (thresh, kind) in OLD_CASES.items():
        ca = old[f"{name}_ca"]
        assert threshold_gap(ca, thresh, kind) > 1e-4, name
        assert np.array_equal(numpy_edge_list(ca, thresh, kind), old[f"{name}_edge_index"]), name


def test_structure_entry_points_have_a_header_and_a_version_of_their_own():
    from gvp_hip import _lib, structure
    handle = C.CDLL(_lib.LIB_PATH)
    main_header = open(os.path.join(REPO, "include", "caster_gvp.h")).read()
    header = open(os.path.join(REPO, "include", "caster_gvp_structure.h")).read()
    assert set(structure.exported_symbols()) == set(NEW_SYMBOLS)
    for name in NEW_SYMBOLS:
        assert hasattr(handle, name), name
        assert name + "(" in header and name not in main_header and name not in _lib.exported_symbols()
    assert structure.lib().cgvp_structure_version() == 1 == structure.STRUCTURE_VERSION
    assert "#define CGVP_STRUCTURE_VERSION 1" in header
    assert _lib.ABI_VERSION == 31 and _lib.lib().cgvp_abi_version() == 31
    from gvp_hip import ops
    assert ops.protein_graphs is structure.protein_graphs


def test_entry_points_check_their_arguments_on_the_host():
    """Every bad-argument case is answered with CGVP_ERR_BAD_ARG before any launch: no GPU is needed (or touched)."""
    from gvp_hip import structure
    L = structure.lib()
    BAD = -1
    null, p = C.c_void_p(0), C.c_void_p(0x1000)         # never dereferenced: the checks run on the host
    node = lambda coords=p, types=p, ptr=p, props=p, n=8, b=1, t=21, pr=11, x_s=p, x_v=p: \
        L.cgvp_node_featurise(coords, types, ptr, props, n, b, t, pr, x_s, x_v, null, null, null)
    for kw in (dict(coords=null), dict(types=null), dict(ptr=null), dict(props=null), dict(x_s=null), dict(x_v=null),
               dict(n=-1), dict(b=-1), dict(b=0), dict(t=-1), dict(t=0), dict(pr=-1)):
        assert node(**kw) == BAD, kw
    assert node(n=0) == 0                                # an empty batch is not an error (and launches nothing)
    count = lambda ca=p, ptr=p, n=8, b=1, r=4.0, deg=p: L.cgvp_radius_graph_count(ca, ptr, n, b, r, 1, deg, null)
    for kw in (dict(ca=null), dict(ptr=null), dict(deg=null), dict(n=-1), dict(b=-1), dict(b=0), dict(r=-1.0),
               dict(r=float("nan")), dict(r=float("inf"))):
        assert count(**kw) == BAD, kw
    assert count(n=0) == 0
    select = lambda ca=p, ptr=p, n=8, b=1, k=30, td=p, tj=p, deg=p: L.cgvp_knn_graph_select(ca, ptr, n, b, k, 1, td, tj, deg, null)
    for kw in (dict(ca=null), dict(ptr=null), dict(td=null), dict(tj=null), dict(deg=null), dict(n=-1), dict(b=-1),
               dict(b=0), dict(k=0), dict(k=-3), dict(k=65), dict(k=65, n=0)):
        assert select(**kw) == BAD, kw
    assert select(n=0) == 0
    fill = lambda ca=p, ptr=p, n=8, b=1, r=4.0, td=null, tj=null, rs=p, e=16, ei=p: \
        L.cgvp_graph_fill(ca, ptr, n, b, r, td, tj, 1, rs, e, ei, null)
    for kw in (dict(ca=null), dict(ptr=null), dict(rs=null), dict(ei=null), dict(n=-1), dict(b=-1), dict(b=0), dict(e=-1),
               dict(r=-1.0), dict(r=float("nan")), dict(td=p), dict(tj=p)):
        assert fill(**kw) == BAD, kw
    assert fill(n=0) == 0 and fill(e=0) == 0


def test_protein_graphs_refuses_what_it_does_not_build():
    from gvp_hip import ops
    coords, types = torch.zeros(5, 4, 3), torch.zeros(5, dtype=torch.int64)
    ptr, props = torch.tensor([0, 5]), torch.zeros(21, 11)
    with pytest.raises(ValueError, match="thresh_type"):
        ops.protein_graphs(coords, types, ptr, props, edge_thresh=0.1, thresh_type="prop")
    with pytest.raises(ValueError, match="edge_thresh"):
        ops.protein_graphs(coords, types, ptr, props, edge_thresh=None)
    for k in (65, 0, 2.5):
        with pytest.raises(ValueError, match="edge_thresh"):
            ops.protein_graphs(coords, types, ptr, props, edge_thresh=k, thresh_type="num")
    with pytest.raises(ValueError, match="add_residue_posenc"):
        ops.protein_graphs(coords, types, ptr, props, add_residue_posenc=True)
    for kind, thresh in (("dist", 4.0), ("num", 30)):
        with pytest.raises(RuntimeError, match="MI355X only"):
            ops.protein_graphs(coords, types, ptr, props, edge_thresh=thresh, thresh_type=kind)


# ---------------------------------------------------------------------------------------------------------------------
# GPU
def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def build(coords_list, types_list, props, thresh, kind, loops=True, **kw):
    from gvp_hip import ops
    ptr = np.cumsum([0] + [c.shape[0] for c in coords_list]).astype(np.int64)
    out = ops.protein_graphs(T(np.concatenate(coords_list)), T(np.concatenate(types_list)), T(ptr), T(props),
                             edge_thresh=thresh, thresh_type=kind, keep_self_loops=loops, **kw)
    torch.cuda.synchronize()
    return out


def close(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, what
    err = float(np.abs(got.astype(np.float64) - want).max()) if want.size else 0.0
    print(f"{what}: max abs err {err:.3e}")
    assert err < TOL, what
    assert not got[want == 0].any(), f"{what}: the reference's exact zeros"


def check_against(out, x_s, x_v, ei, e_s, e_v, what):
    assert out["edge_index"].dtype == torch.int64 and torch.equal(out["edge_index"].cpu(), torch.from_numpy(ei)), what
    close(out["x"][0], x_s, what + " x_s"); close(out["x"][1], x_v, what + " x_v")
    close(out["eattr"][0], e_s, what + " e_s"); close(out["eattr"][1], e_v, what + " e_v")
    E = ei.shape[1]
    assert out["etypes"].dtype == torch.int64 and out["etypes"].shape == (E,) and not out["etypes"].any()
    assert out["eattr"][1].shape == (E, 1, 3)
    assert not any(t.requires_grad for t in (*out["x"], *out["eattr"]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(OLD_CASES))
def test_edge_lists_of_the_existing_fixture(name):
    """C-alphas of tests/golden/edge_feats.npz in an otherwise zero backbone: the built list is the reference's, its
    features are the fixture's and bitwise what ops.edge_features gives on the same list."""
    from gvp_hip import ops
    g = load_npz("edge_feats.npz")
    ca, (thresh, kind) = g[f"{name}_ca"], OLD_CASES[name]
    coords = np.zeros((ca.shape[0], 4, 3), np.float32)
    coords[:, 1] = ca
    out = build([coords], [np.zeros(ca.shape[0], np.int64)], np.zeros((1, 0), np.float32), thresh, kind)
    assert torch.equal(out["edge_index"].cpu(), torch.from_numpy(g[f"{name}_edge_index"]))
    assert out["x"][0].shape == (ca.shape[0], 6)                             # P = 0: the angle columns alone
    close(out["eattr"][0], g[f"{name}_e_s"], name + " e_s")
    close(out["eattr"][1], g[f"{name}_e_v"], name + " e_v")
    e_s, e_v = ops.edge_features(T(ca), torch.arange(ca.shape[0], device=DEV), out["edge_index"])
    assert torch.equal(e_s, out["eattr"][0]) and torch.equal(e_v, out["eattr"][1])


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_every_fixture_case_on_its_own(gold, name):
    coords, types, thresh, kind, loops = case_of(gold, name)
    out = build([coords], [types], gold["aa_props"], thresh, kind, loops)
    check_against(out, *(gold[f"{name}_{k}"] for k in ("x_s", "x_v", "edge_index", "e_s", "e_v")), name)
    L = coords.shape[0]
    assert out["batch"].cpu().tolist() == [0] * L and out["ptr"].cpu().tolist() == [0, L]
    assert torch.equal(out["ntypes"].cpu(), torch.from_numpy(types))
    if kind == "num":                                                        # the path without a host read gives the same
        again = build([coords], [types], gold["aa_props"], thresh, kind, loops, num_edges=gold[f"{name}_edge_index"].shape[1])
        assert torch.equal(again["edge_index"], out["edge_index"]) and torch.equal(again["eattr"][0], out["eattr"][0])


@pytest.mark.gpu
def test_four_graph_batch(gold):
    """tiny1 | helixish | tiny2 | short37 in one call == the per-graph fixtures concatenated with node offsets."""
    names = ("tiny1", "helixish", "tiny2", "short37")
    out = build([gold[f"{n}_coords"] for n in names], [gold[f"{n}_types"] for n in names], gold["aa_props"], 4.0, "dist")
    lens = [gold[f"{n}_coords"].shape[0] for n in names]
    ptr = np.cumsum([0] + lens)
    cat = lambda k, ax=0: np.concatenate([gold[f"{n}_{k}"] for n in names], axis=ax)
    ei = np.concatenate([gold[f"{n}_edge_index"] + off for n, off in zip(names, ptr[:-1])], axis=1)
    check_against(out, cat("x_s"), cat("x_v"), ei, cat("e_s"), cat("e_v"), "batch")
    batch = out["batch"].cpu().numpy()
    assert np.array_equal(batch, np.repeat(np.arange(4), lens)) and out["ptr"].cpu().tolist() == ptr.tolist()
    got = out["edge_index"].cpu().numpy()
    assert np.array_equal(batch[got[0]], batch[got[1]])                      # no edge crosses a graph
    x_s = out["x"][0].cpu().numpy()
    for b in range(4):                                                       # no dihedral crosses a boundary
        assert x_s[ptr[b], [0, 3]].tolist() == [1.0, 0.0] and x_s[ptr[b + 1] - 1, [1, 2, 4, 5]].tolist() == [1.0, 1.0, 0.0, 0.0]


@pytest.mark.gpu
def test_knn_tie_goes_to_the_lower_index(gold):
    """Two exactly coincident candidates at the k-th boundary: np.argsort(kind='stable') keeps the lower j."""
    rng = np.random.default_rng(5)
    coords = (rng.normal(size=(10, 4, 3)) * 0.3).astype(np.float32)
    coords[:, 1] = 50.0 + 10.0 * np.arange(10)[:, None]                      # far apart on a line ...
    coords[0, 1] = (0.0, 0.0, 0.0)
    coords[1, 1] = (1.0, 0.0, 0.0)
    coords[4, 1] = coords[7, 1] = (0.0, 2.0, 0.0)                            # ... but for a tie for source 0's 3rd neighbour
    types = np.zeros(10, np.int64)
    for loops, k, want in ((True, 3, [0, 1, 4]), (False, 2, [1, 4])):
        out = build([coords], [types], gold["aa_props"], k, "num", loops)
        ei = out["edge_index"].cpu().numpy()
        assert ei[1][ei[0] == 0].tolist() == want
        assert np.array_equal(ei, numpy_edge_list(coords[:, 1], k, "num", loops))
    # and a batch of kNN graphs, one of them shorter than k, without self loops: degrees min(k, L_b - 1)
    names = ("knn_short", "tiny1", "short37")
    cs, ts = [gold[f"{n}_coords"] for n in names], [gold[f"{n}_types"] for n in names]
    out = build(cs, ts, gold["aa_props"], 30, "num", False)
    offs = np.cumsum([0] + [c.shape[0] for c in cs])
    want = np.concatenate([numpy_edge_list(c[:, 1], 30, "num", False) + o for c, o in zip(cs, offs[:-1])], axis=1)
    assert want.shape[1] == 20 * 19 + 0 + 37 * 30 and np.array_equal(out["edge_index"].cpu().numpy(), want)


@pytest.mark.gpu
def test_malformed_offsets_and_types_are_clamped(gold):
    """A ptr whose last entry exceeds N and residue types outside the table: the call returns well-formed tensors."""
    from gvp_hip import ops
    coords, types = gold["helixish_coords"][:50], gold["helixish_types"][:50].copy()
    types[7], types[9] = 25, -3
    for kind, thresh in (("dist", 4.0), ("num", 5)):
        out = ops.protein_graphs(T(coords), T(types), T(np.array([0, 20, 70])), T(gold["aa_props"]), edge_thresh=thresh,
                                 thresh_type=kind)
        torch.cuda.synchronize()
        E = out["edge_index"].shape[1]
        assert out["x"][0].shape == (50, 17) and out["x"][1].shape == (50, 3, 3) and out["eattr"][0].shape == (E, 32)
        assert all(bool(torch.isfinite(t).all()) for t in (*out["x"], *out["eattr"]))
        assert E > 0 and int(out["edge_index"].min()) >= 0 and int(out["edge_index"].max()) < 50
        assert int(out["batch"].min()) >= 0 and int(out["batch"].max()) <= 1


def _synthetic_backbone(ca, rng):
    out = np.zeros((ca.shape[0], 4, 3))
    out[:, 1] = ca
    for atom in (0, 2, 3):
        d = rng.normal(size=ca.shape)
        out[:, atom] = ca + 1.4 * d / np.linalg.norm(d, axis=-1, keepdims=True)
    return out.astype(np.float32)


@pytest.mark.gpu
def test_built_graph_feeds_the_encoder_and_the_joint_model(gold, protein_params, pretrained):
    """coordinates -> device graph -> encoder == the same graph computed in float64 and stored as float32 -> encoder."""
    from models.joint_gnn import JointGNN
    from models.protein_gnn import SelectableProteinModelWrapper
    kwargs = json.load(open(os.path.join(GOLDEN, "model_kwargs.json")))
    kw = dict(kwargs["protein_gnn_kwargs"])
    for k in ("in_channels", "edge_dim", "hidden_channels", "edge_hidden_channels"):
        kw[k] = tuple(kw[k])
    model = SelectableProteinModelWrapper(**kw)
    model.load_state_dict({"gnn_model." + k: v for k, v in protein_params.items()})
    model = model.to(DEV).eval()
    rng = np.random.default_rng(2)
    coords = _synthetic_backbone(ds.ca_trace(90, rng), rng)
    types = rng.integers(0, 20, size=90).astype(np.int64)
    props = gold["aa_props"]
    x_s, x_v, ei, e_s, e_v = numpy_protein_graph(coords, types, props, 4.0, "dist")
    out = build([coords], [types], props, 4.0, "dist")
    assert torch.equal(out["edge_index"].cpu(), torch.from_numpy(ei))
    f = lambda a: T(a.astype(np.float32))
    with torch.no_grad():
        a = model((f(x_s), f(x_v)), T(ei), T(types), torch.zeros(ei.shape[1], dtype=torch.int64, device=DEV),
                  eattr=(f(e_s), f(e_v)))
        b = model(**{k: v for k, v in out.items() if k != "ptr"})
    err = rel_err(b, a)
    print(f"encoder on the built graph vs on the stored float64 graph: rel err {err:.3e}")
    assert err < 2e-5

    joint = JointGNN(protein_gnn_kwargs=kwargs["protein_gnn_kwargs"], molecule_gnn_kwargs=kwargs["molecule_gnn_kwargs"],
                     **kwargs["joint_gnn_kwargs"])
    joint.load_state_dict(pretrained, strict=True)
    joint = joint.to(DEV).eval()
    pair = build([coords[:30], coords[40:60]], [types[:30], types[40:60]], props, 4.0, "dist")
    assert "ptr" in pair and pair["ptr"].tolist() == [0, 30, 50]
    md = ds.to_torch(ds.drug_batch(2, 0))
    md = {k: (tuple(t.to(DEV) for t in v) if isinstance(v, tuple) else v.to(DEV)) for k, v in md.items()}
    with torch.no_grad():
        y, _ = joint(pair, md)
    assert y.shape[0] == 2 and bool(torch.isfinite(y).all())
