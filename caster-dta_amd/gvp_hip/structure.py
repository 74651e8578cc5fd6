"""Backbone coordinates -> the protein graph dict the encoders take, built on the device.

ctypes binding of include/caster_gvp_structure.h (csrc/structure_kernels.hip), a header and a version of its own
beside the main C ABI: the entry points live in the same libcaster_gvp.so, the signature table below is this
module's.  `protein_graphs` replaces the reference's per-protein CPU featuriser
(utils/create_protein_features.py:12-357 + utils/create_graphs.py:29,44-45) for `thresh_type` 'dist' and 'num'.
"""
from __future__ import annotations

import ctypes as C
import functools

import torch

from . import _lib
from ._lib import _on_gpu, _ptr, _stream

STRUCTURE_VERSION = 1    # CGVP_STRUCTURE_VERSION
KNN_MAX = 64             # CGVP_KNN_MAX

_P, _I64, _I32, _F64 = C.c_void_p, C.c_int64, C.c_int32, C.c_double
_SIGNATURES = {
    "cgvp_structure_version": (C.c_int, []),
    "cgvp_node_featurise": (C.c_int, [_P, _P, _P, _P, _I64, _I64, _I32, _I32, _P, _P, _P, _P, _P]),
    "cgvp_radius_graph_count": (C.c_int, [_P, _P, _I64, _I64, _F64, _I32, _P, _P]),
    "cgvp_knn_graph_select": (C.c_int, [_P, _P, _I64, _I64, _I32, _I32, _P, _P, _P, _P]),
    "cgvp_graph_fill": (C.c_int, [_P, _P, _I64, _I64, _F64, _P, _P, _I32, _P, _I64, _P, _P]),
}


def exported_symbols():
    """Names include/caster_gvp_structure.h declares."""
    return tuple(_SIGNATURES)


@functools.lru_cache(maxsize=None)
def lib():
    """libcaster_gvp.so (the handle of `_lib.lib()`) with the structure entry points typed (once)."""
    return _lib.bind(_lib.lib(), _SIGNATURES, "cgvp_structure_version", STRUCTURE_VERSION, "structure version")


def _checked(t, name, dtypes, what):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name}: expected a tensor ({what})")
    _on_gpu(t, name)
    if t.dtype not in dtypes:
        raise ValueError(f"{name}: expected {what}, got dtype {t.dtype}")
    return t.detach().contiguous()


def protein_graphs(coords, residue_types, ptr, props, *, edge_thresh=4.0, thresh_type="dist", keep_self_loops=True,
                   add_residue_posenc=False, num_edges=None):
    """The batched protein graph of the reference's featuriser, from backbone atoms.

    coords [N, 4, 3] fp32 (N, CA, C, O per residue, Angstrom), residue_types [N] int64, ptr [B + 1] int64 (graph b
    owns rows ptr[b] .. ptr[b+1]), props [T, P] fp32 (per-type property rows; the reference's table has P = 11) ->

        {"x": (x_s [N, 6 + P], x_v [N, 3, 3]), "edge_index": int64 [2, E], "ntypes": residue_types,
         "etypes": zeros int64 [E], "eattr": (e_s [E, 32], e_v [E, 1, 3]), "batch": int64 [N], "ptr": ptr}

    which `JointGNN.forward` takes as `protein_graph_data` (and the protein wrapper without "ptr").  Edges are those of
    `thresh_type` 'dist' (|CA_i - CA_j| <= edge_thresh) or 'num' (the edge_thresh <= 64 nearest residues of the same
    graph, ties to the lower index), in the reference's row-major order.  Nothing crosses a graph.  The reference's
    other modes ('prop', dense graphs, residue positional encodings) raise ValueError.

    Host synchronisation: the number of edges sizes the outputs, so it is read back ONCE per call (after the count
    launch on the 'dist' path).  On the 'num' path E = sum_b L_b * min(k, L_b) (L_b - 1 without self loops) depends on
    the graph lengths alone: pass it as `num_edges` and the call makes no host read at all.  (`num_edges` is trusted;
    positions a wrong value leaves uncovered stay zero, nothing is written out of bounds.)

    No autograd through coordinates: the outputs do not require grad.
    """
    if thresh_type not in ("dist", "num"):
        raise ValueError(f"thresh_type {thresh_type!r}: only 'dist' and 'num' are built on the device")
    if edge_thresh is None:
        raise ValueError("edge_thresh=None (dense graphs) is not built on the device")
    if add_residue_posenc:
        raise ValueError("add_residue_posenc: 33-wide node inputs are not built on the device")
    if thresh_type == "num":
        k = int(edge_thresh)
        if k != edge_thresh or not 1 <= k <= KNN_MAX:
            raise ValueError(f"thresh_type='num' needs an integer 1 <= edge_thresh <= {KNN_MAX}, got {edge_thresh!r}")
    else:
        radius = float(edge_thresh)
        if not 0.0 <= radius < float("inf"):
            raise ValueError(f"thresh_type='dist' needs a finite edge_thresh >= 0, got {edge_thresh!r}")
    coords = _checked(coords, "coords", (torch.float32,), "float32 [N, 4, 3]")
    types = _checked(residue_types, "residue_types", (torch.int64,), "int64 [N]")
    ptr_c = _checked(ptr, "ptr", (torch.int64,), "int64 [B + 1]")
    props = _checked(props, "props", (torch.float32,), "float32 [T, P]")
    if coords.dim() != 3 or tuple(coords.shape[1:]) != (4, 3):
        raise ValueError(f"coords: expected [N, 4, 3] (N, CA, C, O), got {tuple(coords.shape)}")
    N = int(coords.shape[0])
    if types.dim() != 1 or types.shape[0] != N:
        raise ValueError(f"residue_types: expected [{N}], got {tuple(types.shape)}")
    if ptr_c.dim() != 1 or ptr_c.shape[0] < 2:
        raise ValueError(f"ptr: expected [B + 1] with B >= 1, got {tuple(ptr_c.shape)}")
    if props.dim() != 2 or (props.shape[1] > 0 and props.shape[0] < 1):
        raise ValueError(f"props: expected [T, P], got {tuple(props.shape)}")
    if num_edges is not None and int(num_edges) < 0:
        raise ValueError("num_edges must be >= 0")
    B, T, P = int(ptr_c.shape[0]) - 1, int(props.shape[0]), int(props.shape[1])
    dev, L = coords.device, lib()
    new = lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype, device=dev)
    x_s, x_v = new(N, 6 + P), new(N, 3, 3)
    batch, seq = new(N, dtype=torch.int64), new(N, dtype=torch.int64)
    deg = new(N, dtype=torch.int64)
    ca = coords[:, 1, :].contiguous()
    self_loops = 1 if keep_self_loops else 0
    with torch.cuda.device(dev):
        st = _stream()
        _lib.check(L.cgvp_node_featurise(_ptr(coords), _ptr(types), _ptr(ptr_c), _ptr(props), N, B, T, P, _ptr(x_s),
                                         _ptr(x_v), _ptr(batch), _ptr(seq), st), "cgvp_node_featurise")
        if thresh_type == "dist":
            tau_d2 = tau_j = None
            _lib.check(L.cgvp_radius_graph_count(_ptr(ca), _ptr(ptr_c), N, B, radius, self_loops, _ptr(deg), st),
                       "cgvp_radius_graph_count")
        else:
            radius = 0.0
            tau_d2, tau_j = new(N, dtype=torch.float64), new(N, dtype=torch.int64)
            _lib.check(L.cgvp_knn_graph_select(_ptr(ca), _ptr(ptr_c), N, B, k, self_loops, _ptr(tau_d2), _ptr(tau_j),
                                               _ptr(deg), st), "cgvp_knn_graph_select")
        ends = torch.cumsum(deg, 0)
        rowstart = ends - deg                                      # exclusive scan
        if num_edges is None:
            E = int(ends[-1]) if N else 0                          # the one host read
            edge_index = new(2, E, dtype=torch.int64)
        else:
            E = int(num_edges)
            edge_index = torch.zeros(2, E, dtype=torch.int64, device=dev)
        _lib.check(L.cgvp_graph_fill(_ptr(ca), _ptr(ptr_c), N, B, radius, _ptr(tau_d2), _ptr(tau_j), self_loops,
                                     _ptr(rowstart), E, _ptr(edge_index), st), "cgvp_graph_fill")
        e_s, e_v = new(E, 32), new(E, 1, 3)
        _lib.check(L.cgvp_edge_featurise(_ptr(ca), _ptr(seq), _ptr(edge_index), N, E, _ptr(e_s), _ptr(e_v), st),
                   "cgvp_edge_featurise")
    return {"x": (x_s, x_v), "edge_index": edge_index, "ntypes": residue_types,
            "etypes": torch.zeros(E, dtype=torch.int64, device=dev), "eattr": (e_s, e_v), "batch": batch, "ptr": ptr}
