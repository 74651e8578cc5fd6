"""Per-node attention scores of the varlen cross attention: `caster_gvp::cross_attention_node_scores`, `per_pair`.

ctypes binding of include/caster_gvp_attnscore.h (csrc/attn_score_kernels.hip), a header and a version of its own beside
the main C ABI: the entry points live in the same libcaster_gvp.so, the signature table below is this module's.
The reference's evaluation keeps four vectors of every pair's attention weights (inference/evaluation.py:54-66, 97-102:
the head-averaged weight matrices cut to the pair's lengths, then the column mean and the column max of each):

    molecule_attention / max_molecule_attention    one value per atom, reduced over the residue queries
    protein_attention  / max_protein_attention     one value per residue, reduced over the atom queries

The op computes all four from the compact rows and the log-sum-exp `caster_gvp::cross_attention` saved, in one launch:
no dense [B, Rmax, Amax] weights, no host read of the longest pair, no synchronisation -- it can be captured.
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import List, Tuple

import torch
from torch import Tensor

from . import _lib, attention_ops
from ._lib import _on_gpu, _stream

ATTN_SCORE_VERSION = 1   # CGVP_ATTN_SCORE_VERSION
MAX_HEADS = 8            # CGVP_ATTN_SCORE_MAX_HEADS
HEAD_DIM = 16
MAX_WIDTH = MAX_HEADS * HEAD_DIM   # the kernel keeps the keys of all heads in registers: heads * head_dim <= 128


class ScoreProblem(C.Structure):
    """cgvp_attn_score_problem (one direction of the cross attention)."""
    _fields_ = [("q", C.c_void_p), ("k", C.c_void_p), ("lse", C.c_void_p), ("q_ptr", C.c_void_p), ("k_ptr", C.c_void_p),
                ("num_q", C.c_int64), ("num_k", C.c_int64), ("out_mean", C.c_void_p), ("out_max", C.c_void_p)]


_P, _I64, _I32 = C.c_void_p, C.c_int64, C.c_int32
_SIGNATURES = {
    "cgvp_attn_score_version": (C.c_int, []),
    "cgvp_attn_node_scores": (C.c_int, [C.POINTER(ScoreProblem), _I32, _I64, _I32, C.c_float, _P]),
}


def exported_symbols():
    """Names include/caster_gvp_attnscore.h declares."""
    return tuple(_SIGNATURES)


@functools.lru_cache(maxsize=None)
def lib():
    """libcaster_gvp.so (the handle of `_lib.lib()`) with the attention-score entry points typed (once)."""
    return _lib.bind(_lib.lib(), _SIGNATURES, "cgvp_attn_score_version", ATTN_SCORE_VERSION, "attention-score version")


# include/caster_gvp_attnhd.h: the same kernel with the head width as an argument (the other entry points of that
# header are typed in gvp_hip.attention_ops, on the same handle)
_HD_SIGNATURES = {
    "cgvp_attn_node_scores_hd": (C.c_int, [C.POINTER(ScoreProblem), _I32, _I64, _I32, _I32, C.c_float, _P]),
}


@functools.lru_cache(maxsize=None)
def hd_lib():
    return _lib.bind(attention_ops.hd_lib(), _HD_SIGNATURES)


def _rows(t, name, width):
    _on_gpu(t, name)
    if t.dim() != 2 or t.shape[1] != width:
        raise NotImplementedError(f"{name}: expected [rows, {width}] (the width of its direction's queries / the head "
                                  f"count), got {tuple(t.shape)}")
    return t.detach().to(torch.float32).contiguous()


def _width(q, name, heads):
    """heads * head_dim of a direction's queries, head_dim in {16, 32, 64} and the width at most MAX_WIDTH."""
    _on_gpu(q, name)
    hd = attention_ops.head_dim_of(q, name, heads)
    if heads * hd > MAX_WIDTH:
        raise NotImplementedError(f"{name}: the attention-score kernel is compiled for embed widths up to {MAX_WIDTH} "
                                  f"(heads * head_dim), got {heads} x {hd}; reduce caster_gvp::cross_attention_weights")
    return heads * hd, hd


@torch.library.custom_op("caster_gvp::cross_attention_node_scores", mutates_args=(), device_types="cuda")
def cross_attention_node_scores_op(q_r: Tensor, k_a: Tensor, lse_r: Tensor, q_a: Tensor, k_r: Tensor, lse_a: Tensor,
                                   rptr: Tensor, aptr: Tensor, heads: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """-> (atom_mean [Na], atom_max [Na], residue_mean [N], residue_max [N]), fp32.

    Direction 0: residue queries q_r [N, E] with lse_r [N, heads] on atom keys k_a [Na, E] -- the mean / max over a
    pair's residues of every atom's head-averaged weight (the reference's molecule_attention / max_molecule_attention).
    Direction 1: atom queries q_a, lse_a on residue keys k_r (protein_attention / max_protein_attention).  The
    operands and the lse are those of `caster_gvp::cross_attention`; rptr / aptr [B + 1] delimit the pairs.  A node
    whose pair has no node on the other side gets 0; rptr[-1] / aptr[-1] must be the row counts (rows behind them are
    not written).  No host read, no synchronisation.

    head_dim = width // heads is 16, 32 or 64 per direction ((q_r, k_a) share a width, (q_a, k_r) another) and a width
    is at most 128: NotImplementedError for anything else (the model then reduces the dense weights)."""
    if not 1 <= heads <= MAX_HEADS:
        raise NotImplementedError(f"the attention-score kernel is compiled for 1..{MAX_HEADS} heads, got {heads}")
    (E_r, hd_r), (E_a, hd_a) = _width(q_r, "q_r", heads), _width(q_a, "q_a", heads)
    q_r, k_a = _rows(q_r, "q_r", E_r), _rows(k_a, "k_a", E_r)
    q_a, k_r = _rows(q_a, "q_a", E_a), _rows(k_r, "k_r", E_a)
    lse_r, lse_a = _rows(lse_r, "lse_r", heads), _rows(lse_a, "lse_a", heads)
    attention_ops._check_rows(q_r, k_r, lse_r, q_a, k_a, lse_a, rptr, aptr)
    rptr, aptr = attention_ops._i64c(rptr, "rptr"), attention_ops._i64c(aptr, "aptr")
    N, Na = int(q_r.shape[0]), int(q_a.shape[0])
    dev, B = q_r.device, int(rptr.numel()) - 1
    # every key row of a pair is written by the kernel: with ptr[-1] == the row count (what PyG batches deliver, and what
    # caster_gvp::cross_attention assumes for its own outputs) nothing stays undefined and nothing needs a fill
    f32 = dict(dtype=torch.float32, device=dev)
    atom_mean, atom_max = torch.empty(Na, **f32), torch.empty(Na, **f32)
    res_mean, res_max = torch.empty(N, **f32), torch.empty(N, **f32)
    P = (ScoreProblem * 2)()
    v = attention_ops._addr
    for p, (q, k, lse, qp, kp, mean, mx) in zip(P, ((q_r, k_a, lse_r, rptr, aptr, atom_mean, atom_max),
                                                     (q_a, k_r, lse_a, aptr, rptr, res_mean, res_max))):
        p.q, p.k, p.lse, p.q_ptr, p.k_ptr = v(q), v(k), v(lse), qp.data_ptr(), kp.data_ptr()
        p.num_q, p.num_k, p.out_mean, p.out_max = int(q.shape[0]), int(k.shape[0]), v(mean), v(mx)
    fn = hd_lib().cgvp_attn_node_scores_hd
    with torch.cuda.device(dev):
        for first, n, hd, scale in attention_ops.launch_plan((hd_r, hd_a)):
            _lib.check(fn(C.pointer(P[first]), n, B, heads, hd, scale, _stream()), "cgvp_attn_node_scores_hd")
    return atom_mean, atom_max, res_mean, res_max


@cross_attention_node_scores_op.register_fake
def _(q_r, k_a, lse_r, q_a, k_r, lse_a, rptr, aptr, heads):
    f = lambda t: t.new_empty((t.shape[0],), dtype=torch.float32)
    return f(k_a), f(k_a), f(k_r), f(k_r)


torch.library.register_autocast("caster_gvp::cross_attention_node_scores", "cuda", torch.float32)


def per_pair(values: Tensor, ptr: Tensor) -> List[Tensor]:
    """The per-pair views of a compact per-node vector (the reference's list-of-arrays columns): ONE host read of `ptr`."""
    edges = ptr.tolist()
    return [values[lo:hi] for lo, hi in zip(edges[:-1], edges[1:])]
