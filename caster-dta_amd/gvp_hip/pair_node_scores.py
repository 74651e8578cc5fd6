"""Per-node attention scores of a LIST OF PAIRS drawn from a few unique graphs:
`caster_gvp::cross_attention_pairs_node_scores`.

ctypes binding of include/caster_gvp_pairscore.h (csrc/attn_pairs_score_kernels.hip), a header and a version of its own
beside the main C ABI: the entry point lives in the same libcaster_gvp.so, the signature table below is this module's.

`caster_gvp::cross_attention_node_scores` ties pair b to rows ptr[b] .. ptr[b+1] of its queries, keys and lse alike; to
use it on a pair list the projected rows of every unique graph would have to be copied once per pair.  Here the queries
and keys stay where `caster_gvp::cross_attention_pairs` read them -- every unique graph once -- and the pairing is that
op's index tables; only the log-sum-exp it saved and the four outputs are per pair, at the offsets `plan_pairs` lays
out.  One launch for both directions, no host read, no synchronisation.  Inference only: no autograd.
`JointGNN.score_pairs_with_node_attention` is the caller.
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import Tuple

import torch
from torch import Tensor

from . import _lib, attention_ops, attention_scores
from ._lib import _stream
from .pair_scoring import _table

PAIR_SCORE_VERSION = 1   # CGVP_PAIR_SCORE_VERSION


class PairScoreProblem(C.Structure):
    """cgvp_attn_pairs_score_problem (one direction of the cross attention over a pair list)."""
    _fields_ = [("q", C.c_void_p), ("k", C.c_void_p), ("lse", C.c_void_p), ("q_ptr", C.c_void_p), ("k_ptr", C.c_void_p),
                ("num_q_graphs", C.c_int64), ("num_k_graphs", C.c_int64), ("num_q", C.c_int64), ("num_k", C.c_int64),
                ("q_graph", C.c_void_p), ("k_graph", C.c_void_p), ("qout_ptr", C.c_void_p), ("num_qout", C.c_int64),
                ("kout_ptr", C.c_void_p), ("num_kout", C.c_int64), ("out_mean", C.c_void_p), ("out_max", C.c_void_p)]


_P, _I64, _I32 = C.c_void_p, C.c_int64, C.c_int32
_SIGNATURES = {
    "cgvp_pair_score_version": (C.c_int, []),
    "cgvp_attn_node_scores_pairs": (C.c_int, [C.POINTER(PairScoreProblem), _I32, _I64, _I32, _I32, C.c_float, _P]),
}


def exported_symbols():
    """Names include/caster_gvp_pairscore.h declares."""
    return tuple(_SIGNATURES)


@functools.lru_cache(maxsize=None)
def lib():
    """libcaster_gvp.so (the handle of `_lib.lib()`) with the pair-score entry point typed (once)."""
    return _lib.bind(_lib.lib(), _SIGNATURES, "cgvp_pair_score_version", PAIR_SCORE_VERSION, "pair-score version")


def _shapes(q1, q2, heads):
    """-> ((width, head_dim) of direction 0, of direction 1); NotImplementedError for a head count or a width the kernel
    is not compiled for.  The op and its fake kernel both start here, so a trace refuses what a call refuses."""
    if not 1 <= heads <= attention_scores.MAX_HEADS:
        raise NotImplementedError(f"the pair-score kernel is compiled for 1..{attention_scores.MAX_HEADS} heads, got {heads}")
    return attention_scores._width(q1, "q1", heads), attention_scores._width(q2, "q2", heads)


@torch.library.custom_op("caster_gvp::cross_attention_pairs_node_scores", mutates_args=(), device_types="cuda")
def cross_attention_pairs_node_scores_op(q1: Tensor, k1: Tensor, lse1: Tensor, q2: Tensor, k2: Tensor, lse2: Tensor,
                                         ptr1: Tensor, ptr2: Tensor, g1: Tensor, g2: Tensor, optr1: Tensor,
                                         optr2: Tensor, heads: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """-> (atom_mean [rows2], atom_max [rows2], residue_mean [rows1], residue_max [rows1]), fp32, with
    rows1 = lse1.shape[0] and rows2 = lse2.shape[0] (host-known: nothing is read back).

    Operand order and meaning are those of `caster_gvp::cross_attention_node_scores`, the tables those of
    `caster_gvp::cross_attention_pairs`.  Direction 0: the queries of pair b are the rows ptr1[g1[b]] .. of q1 (the
    residues of protein g1[b]) with the lse rows optr1[b] .. of lse1, its keys the rows ptr2[g2[b]] .. of k1 (the atoms
    of molecule g2[b]); it writes entries optr2[b] .. optr2[b+1] of atom_mean / atom_max -- the mean / max over the
    pair's residues of every atom's head-averaged weight.  Direction 1 is the mirror image: queries q2 with lse2 at
    optr2, keys k2, outputs residue_mean / residue_max at optr1.  q1 / k2 hold the unique proteins' rows, q2 / k1 the
    unique molecules'; lse1 / lse2 are what `caster_gvp::cross_attention_pairs_lse` returned for the same tables.

    A node whose pair has no node on the other side gets 0.  The kernel writes every entry below optr[-1]; entries
    behind optr2[-1] / optr1[-1] (when lse2 / lse1 have more rows than the pairs cover) are NOT written.  The tables
    are not checked on the device: take them from `plan_pairs`.

    head_dim = width // heads is 16, 32 or 64 per direction ((q1, k1) share a width, (q2, k2) another) and a width is
    at most 128: NotImplementedError for anything else, and for heads outside 1..8.  One launch when the widths agree,
    else one per direction."""
    (E1, hd1), (E2, hd2) = _shapes(q1, q2, heads)
    rows = attention_scores._rows
    q1, k1, q2, k2 = rows(q1, "q1", E1), rows(k1, "k1", E1), rows(q2, "q2", E2), rows(k2, "k2", E2)
    lse1, lse2 = rows(lse1, "lse1", heads), rows(lse2, "lse2", heads)
    if not (q1.shape[0] == k2.shape[0] and q2.shape[0] == k1.shape[0]):
        raise ValueError("row counts of the protein-side (q1, k2) / molecule-side (q2, k1) tensors disagree")
    ptr1, ptr2, g1 = _table(ptr1, "ptr1"), _table(ptr2, "ptr2"), _table(g1, "g1")
    if ptr1.numel() < 1 or ptr2.numel() < 1:
        raise ValueError("ptr1 / ptr2 must be [num_graphs + 1]")
    B = int(g1.numel())
    g2, optr1, optr2 = _table(g2, "g2", B), _table(optr1, "optr1", B + 1), _table(optr2, "optr2", B + 1)
    dev = q1.device
    rows1, rows2 = int(lse1.shape[0]), int(lse2.shape[0])
    f32 = dict(dtype=torch.float32, device=dev)
    atom_mean, atom_max = torch.empty(rows2, **f32), torch.empty(rows2, **f32)
    res_mean, res_max = torch.empty(rows1, **f32), torch.empty(rows1, **f32)
    P = (PairScoreProblem * 2)()
    a = attention_ops._addr
    for p, (q, k, lse, qp, kp, qg, kg, qo, ko, mean, mx) in zip(
            P, ((q1, k1, lse1, ptr1, ptr2, g1, g2, optr1, optr2, atom_mean, atom_max),
                (q2, k2, lse2, ptr2, ptr1, g2, g1, optr2, optr1, res_mean, res_max))):
        p.q, p.k, p.lse, p.q_ptr, p.k_ptr = a(q), a(k), a(lse), qp.data_ptr(), kp.data_ptr()
        p.num_q_graphs, p.num_k_graphs, p.num_q, p.num_k = qp.numel() - 1, kp.numel() - 1, int(q.shape[0]), int(k.shape[0])
        # an empty table still needs an address: the entry point refuses NULL tables before it looks at num_pairs
        p.q_graph, p.k_graph = qg.data_ptr() or qp.data_ptr(), kg.data_ptr() or kp.data_ptr()
        p.qout_ptr, p.num_qout, p.kout_ptr, p.num_kout = qo.data_ptr(), int(lse.shape[0]), ko.data_ptr(), int(mean.shape[0])
        p.out_mean, p.out_max = a(mean), a(mx)
    fn = lib().cgvp_attn_node_scores_pairs
    with torch.cuda.device(dev):
        for first, n, hd, scale in attention_ops.launch_plan((hd1, hd2)):
            _lib.check(fn(C.pointer(P[first]), n, B, heads, hd, scale, _stream()), "cgvp_attn_node_scores_pairs")
    return atom_mean, atom_max, res_mean, res_max


@cross_attention_pairs_node_scores_op.register_fake
def _(q1, k1, lse1, q2, k2, lse2, ptr1, ptr2, g1, g2, optr1, optr2, heads):
    _shapes(q1, q2, heads)
    f = lambda t: t.new_empty((t.shape[0],), dtype=torch.float32)
    return f(lse2), f(lse2), f(lse1), f(lse1)


torch.library.register_autocast("caster_gvp::cross_attention_pairs_node_scores", "cuda", torch.float32)
