#!/usr/bin/env python3
"""Generate tests/golden/backbone_graphs.npz from the reference's own protein featuriser.

Like make_golden.py (whose stand-ins for `ipdb` / `torch_geometric.data.Data` and whose by-path davis_synth loader
it reuses) this runs ONLY where a checkout of the upstream CASTER-DTA repository is at hand ($CASTER_DTA_REFERENCE);
the test-suite reads the .npz alone.  Nothing from the reference is copied: the fixture holds coordinates, residue
types and the numbers the reference computes from them.

What is driven, unmodified: utils/create_protein_features.py `compute_residue_node_features(coords, types,
vectorize_features=True, add_esm2_embeds=False, add_residue_posenc=False, include_aa_props=True)`,
`compute_residue_edge_features(coords, types, thresh, kind, keep_self_loops, True)` and utils/create_graphs.py
`construct_graph`.  They are fed the float64 up-cast of float32 coordinates, so the stored truth is the float64
result of exactly the float32 inputs csrc/structure_kernels.hip sees.

Per case `<name>_{coords,types,x_s,x_v,edge_index,e_s,e_v,thresh,kind,self_loops}`; `aa_props` [21, 11] is read off
the reference's own x_s[:, 6:17] rows of the `all_types` case.  The recipe asserts (and prints) that no residue pair
lies within 1e-4 A of a radius threshold and that no kNN row has its k-th and (k+1)-th distances closer than 1e-4 A:
exact edge-set equality is then a fair condition for an fp64 comparison on the device.

`--out-dir DIR --check` regenerates into DIR and compares bit for bit with the committed fixture.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (stand-ins, davis_synth by path, REF; never puts caster-dta_amd on sys.path)

NAME = "backbone_graphs.npz"
GAP = 1e-4
NUM_TYPES = 21           # 20 amino acids + 'X' (utils/protein_definitions.py:4-30)


def backbone(L, rng):
    """[L, 4, 3] float32: CA from davis_synth.ca_trace, N / C / O at seeded random offsets of 1.3-1.5 A from it."""
    ca = mg.ds.ca_trace(L, rng)
    out = np.zeros((L, 4, 3))
    out[:, 1] = ca
    for atom in (0, 2, 3):
        d = rng.normal(size=(L, 3))
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        out[:, atom] = ca + d * rng.uniform(1.3, 1.5, size=(L, 1))
    return out.astype(np.float32)


def cases():
    rng = np.random.default_rng(2024)
    types = lambda L: rng.integers(0, NUM_TYPES, size=L).astype(np.int64)
    out = {}
    out["helixish"] = (backbone(130, rng), types(130), 4.0, "dist", True)
    out["tiny1"] = (backbone(1, rng), types(1), 4.0, "dist", True)
    out["tiny2"] = (backbone(2, rng), types(2), 4.0, "dist", True)
    out["short37"] = (backbone(37, rng), types(37), 4.0, "dist", True)
    co = backbone(40, rng)
    co[3, 0] = co[3, 1]                  # N == CA
    co[11, 1] = co[10, 1]                # CA_i == CA_{i+1}
    co[21, 0] = co[20, 2]                # C_i == N_{i+1}
    co[30, 1] = co[28, 1]                # coincident C-alphas two apart (a zero direction off the chain)
    out["coincident"] = (co, types(40), 6.0, "dist", True)
    # a trace of its own: the shared stream gave a 30th / 31st neighbour 3e-5 A apart, below the gap asserted in main()
    out["knn30"] = (backbone(200, np.random.default_rng(2042)), types(200), 30, "num", True)
    out["knn_short"] = (backbone(20, rng), types(20), 30, "num", True)
    out["noself"] = (backbone(61, rng), types(61), 4.0, "dist", False)
    every = np.concatenate([rng.permutation(NUM_TYPES), rng.permutation(NUM_TYPES)]).astype(np.int64)
    out["all_types"] = (backbone(every.shape[0], rng), every, 4.0, "dist", True)
    return out


def threshold_gap(ca, thresh, kind):
    """Distance (A) between the threshold and the nearest pair distance that could flip an edge."""
    ca = ca.astype(np.float64)
    d = np.linalg.norm(ca[:, None] - ca[None], axis=-1)
    if kind == "dist":
        return float(np.abs(d - thresh).min())
    k = int(thresh)
    if d.shape[0] <= k:
        return float("inf")
    s = np.sort(d, axis=-1)
    return float((s[:, k] - s[:, k - 1]).min())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=HERE)
    ap.add_argument("--check", action="store_true", help="compare the regenerated file bit for bit with the committed one")
    args = ap.parse_args()
    REF = mg.REF
    if REF is None or not os.path.isdir(os.path.join(REF, "utils")):
        ap.error("set CASTER_DTA_REFERENCE to a checkout of the upstream CASTER-DTA repository")
    if args.check and os.path.abspath(args.out_dir) == HERE:
        ap.error("--check compares against the committed fixture: give --out-dir another directory")
    mg.install_standins()
    assert not any(os.path.abspath(p or ".").startswith(os.path.join(mg.REPO, "caster-dta_amd")) for p in sys.path), \
        "caster-dta_amd must not be importable here"
    sys.path.insert(0, REF)
    import utils.create_protein_features as cpf          # reference, unmodified
    import utils.create_graphs as cg
    for mod in (cpf, cg):
        assert os.path.abspath(mod.__file__).startswith(REF + "/"), mod.__file__

    arrays = {}
    for name, (coords, types, thresh, kind, self_loops) in cases().items():
        assert coords.dtype == np.float32
        n = coords.shape[0]
        c64 = coords.astype(np.float64)
        nodes = cpf.compute_residue_node_features(c64, types, vectorize_features=True, add_esm2_embeds=False,
                                                  add_residue_posenc=False, include_aa_props=True)
        edges = cpf.compute_residue_edge_features(c64, types, thresh, kind, self_loops, True)
        g = cg.construct_graph(nodes, edges, types, np.zeros((n, n), np.int64))
        gap = threshold_gap(coords[:, 1], thresh, kind)
        assert gap > GAP, (name, gap)
        arrays.update({f"{name}_coords": coords, f"{name}_types": types, f"{name}_x_s": mg.np_(g.x[0]),
                       f"{name}_x_v": mg.np_(g.x[1]), f"{name}_edge_index": mg.np_(g.edge_index),
                       f"{name}_e_s": mg.np_(g.edge_attr[0]), f"{name}_e_v": mg.np_(g.edge_attr[1]),
                       f"{name}_thresh": np.float64(thresh), f"{name}_kind": np.array(kind),
                       f"{name}_self_loops": np.bool_(self_loops)})
        print(f"backbone {name}: L {n} E {g.edge_index.shape[1]} {kind} {thresh} self_loops {self_loops} "
              f"gap to the threshold {gap:.3g} A")
    co = arrays["coincident_coords"]
    assert (co[3, 0] == co[3, 1]).all() and (co[11, 1] == co[10, 1]).all() and (co[21, 0] == co[20, 2]).all()
    types, x_s = arrays["all_types_types"], arrays["all_types_x_s"]
    assert set(types.tolist()) == set(range(NUM_TYPES))
    props = np.stack([x_s[np.nonzero(types == t)[0][0], 6:17] for t in range(NUM_TYPES)])
    assert (x_s[:, 6:17] == props[types]).all()
    arrays["aa_props"] = props
    os.makedirs(args.out_dir, exist_ok=True)
    np.savez_compressed(os.path.join(args.out_dir, NAME), **arrays)
    print("wrote", NAME, os.path.getsize(os.path.join(args.out_dir, NAME)), "bytes")
    if args.check:
        new, old = np.load(os.path.join(args.out_dir, NAME)), np.load(os.path.join(HERE, NAME))
        same = set(new.files) == set(old.files) and all(
            new[k].dtype == old[k].dtype and new[k].shape == old[k].shape and new[k].tobytes() == old[k].tobytes()
            for k in old.files)
        print("check:", "the regenerated fixture matches bit for bit" if same else "DIFFERENT")
        if not same:
            sys.exit(1)


if __name__ == "__main__":
    main()
