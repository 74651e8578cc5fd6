"""TRAINING on a list of pairs drawn from a few unique proteins and molecules: `plan_pair_training`,
`caster_gvp::cross_attention_pairs_train`, `caster_gvp::expand_rows_train` and their backward ops.

ctypes binding of include/caster_gvp_pairtrain.h (csrc/attn_pairs_bwd_kernels.hip), a header and a version of its own
beside the main C ABI and beside caster_gvp_attnpairs.h: the entry points live in the same libcaster_gvp.so, the
signature table below is this module's.

`gvp_hip.pair_scoring` computes a pair list with every unique graph encoded once, for inference: its ops refuse
gradients.  The ops here are the same forward (bitwise: the same entry points) under autograd.  The gradient of a unique
row is the sum over all the pairs that reference its graph; it is an ORDERED sum (per-pair partial gradients written
with plain stores, then `cgvp_reduce_rows` over the inverse tables of the pair list, in ascending pair order), never a
scatter of float atomics: two runs give bitwise equal gradients, with or without
torch.use_deterministic_algorithms.  Both ops work on the stream of the call and keep nothing between calls (the
workspace is a tensor of the call), so they can be captured into a HIP graph.  `JointGNN.forward_pairs` is the caller.
"""
from __future__ import annotations

import ctypes as C
import functools
from collections import namedtuple
from typing import Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib, attention_ops, pair_scoring
from ._lib import _on_gpu, _stream
from .pair_scoring import _table

PAIR_TRAIN_VERSION = 1   # CGVP_PAIR_TRAIN_VERSION


class PairsBwdProblem(C.Structure):
    """cgvp_attn_pairs_bwd_problem (one direction of the cross attention over a pair list, for its backward)."""
    _fields_ = [("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("q_ptr", C.c_void_p), ("k_ptr", C.c_void_p),
                ("num_q_graphs", C.c_int64), ("num_k_graphs", C.c_int64), ("num_q", C.c_int64), ("num_k", C.c_int64),
                ("q_graph", C.c_void_p), ("k_graph", C.c_void_p), ("out_ptr", C.c_void_p), ("num_out", C.c_int64),
                ("out", C.c_void_p), ("lse", C.c_void_p), ("g_out", C.c_void_p), ("kout_ptr", C.c_void_p),
                ("num_kout", C.c_int64), ("q_inv_ptr", C.c_void_p), ("q_inv_pairs", C.c_void_p), ("k_inv_ptr", C.c_void_p),
                ("k_inv_pairs", C.c_void_p), ("g_q", C.c_void_p), ("g_k", C.c_void_p), ("g_v", C.c_void_p)]


_P, _I64, _I32 = C.c_void_p, C.c_int64, C.c_int32
_SIGNATURES = {
    "cgvp_pair_train_version": (C.c_int, []),
    "cgvp_attn_bwd_pairs_floats": (C.c_int64, [C.POINTER(PairsBwdProblem), _I32, _I32, _I32]),
    "cgvp_attn_bwd_pairs": (C.c_int, [C.POINTER(PairsBwdProblem), _I32, _I64, _I32, _I32, C.c_float, _P, _I64, _P]),
    "cgvp_reduce_rows": (C.c_int, [_P, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _I32, _P, _P]),
}


def exported_symbols():
    """Names include/caster_gvp_pairtrain.h declares."""
    return tuple(_SIGNATURES)


@functools.lru_cache(maxsize=None)
def lib():
    """libcaster_gvp.so (the handle of `_lib.lib()`) with the pair-training entry points typed (once)."""
    return _lib.bind(_lib.lib(), _SIGNATURES, "cgvp_pair_train_version", PAIR_TRAIN_VERSION, "pair-training version")


# ------------------------------------------------------------------------------------------------ planner (host only)
# All K pairs as ONE chunk (the fields of pair_scoring.PairChunk without start / stop) and, for each side, the inverse of
# the pair list: the pairs that reference graph g are inv_pairs[inv_ptr[g] .. inv_ptr[g+1]-1], in ascending pair index.
# numpy int64 throughout.
TABLES = ("g1", "g2", "optr1", "optr2", "inv1_ptr", "inv1_pairs", "inv2_ptr", "inv2_pairs")


class PairTrainPlan(namedtuple("PairTrainPlan", ["g1", "g2", "optr1", "optr2", "rows1", "rows2", "inv1_ptr", "inv1_pairs",
                                                 "inv2_ptr", "inv2_pairs"])):
    """The host tables of one training step (fields above).  `on(device)` is their device copy, made ONCE per plan and
    device: a plan that is part of a prepared batch brings its tables along like the batch's `ptr`, and a step that
    takes it makes no copy -- a host-to-device copy from pageable memory waits for the stream's earlier work."""

    def on(self, device):
        cache = self.__dict__.setdefault("_device_tables", {})
        key = str(torch.device(device))
        if key not in cache:
            cache[key] = upload(self, device)
        return cache[key]


def _inverse(g, num_graphs):
    counts = np.bincount(g, minlength=num_graphs).astype(np.int64)
    return (np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(counts)]),
            np.argsort(g, kind="stable").astype(np.int64))


def plan_pair_training(len1, len2, pairs):
    """The tables of one training step over a pair list -> PairTrainPlan.

    `len1` [P] / `len2` [D]: rows of every unique protein / molecule.  `pairs` [K, 2] of (protein, molecule) indices, or
    None for the full cross product in protein-major order.  No chunking: a training step holds all its pairs at once.
    Validation is `pair_scoring.plan_pairs`': IndexError for an index outside 0 .. P-1 / 0 .. D-1 (the kernels cannot
    check their device tables, this is where they are checked), TypeError for pairs that are not integers.  K = 0 is
    legal (every table of pairs is empty, every inverse range too)."""
    len1, len2 = np.asarray(len1, dtype=np.int64).reshape(-1), np.asarray(len2, dtype=np.int64).reshape(-1)
    chunks = pair_scoring.plan_pairs(len1, len2, pairs, 1 << 62)
    if chunks:
        (c,) = chunks
        g1, g2, optr1, optr2, rows1, rows2 = c.g1, c.g2, c.optr1, c.optr2, c.rows1, c.rows2
    else:
        g1 = g2 = np.zeros(0, dtype=np.int64)
        optr1 = optr2 = np.zeros(1, dtype=np.int64)
        rows1 = rows2 = 0
    inv1_ptr, inv1_pairs = _inverse(g1, len1.shape[0])
    inv2_ptr, inv2_pairs = _inverse(g2, len2.shape[0])
    return PairTrainPlan(g1, g2, optr1, optr2, rows1, rows2, inv1_ptr, inv1_pairs, inv2_ptr, inv2_pairs)


def upload(plan, device):
    """The eight tables of a plan on `device` -> dict name -> int64 tensor: ONE copy (slices of an int64 vector keep the
    8-byte alignment the entry points ask for)."""
    arrays = [getattr(plan, n) for n in TABLES]
    packed = torch.from_numpy(np.concatenate(arrays)).to(device)
    return dict(zip(TABLES, packed.split([int(a.shape[0]) for a in arrays])))


# ------------------------------------------------------------------------------------------------ attention
def _tables(ptr1, ptr2, g1, g2, optr1, optr2, inv1_ptr, inv1_pairs, inv2_ptr, inv2_pairs):
    ptr1, ptr2, g1 = _table(ptr1, "ptr1"), _table(ptr2, "ptr2"), _table(g1, "g1")
    if ptr1.numel() < 1 or ptr2.numel() < 1:
        raise ValueError("ptr1 / ptr2 must be [num_graphs + 1]")
    B = int(g1.numel())
    return (ptr1, ptr2, g1, _table(g2, "g2", B), _table(optr1, "optr1", B + 1), _table(optr2, "optr2", B + 1),
            _table(inv1_ptr, "inv1_ptr", ptr1.numel()), _table(inv1_pairs, "inv1_pairs", B),
            _table(inv2_ptr, "inv2_ptr", ptr2.numel()), _table(inv2_pairs, "inv2_pairs", B))


@torch.library.custom_op("caster_gvp::cross_attention_pairs_train", mutates_args=(), device_types="cuda")
def cross_attention_pairs_train_op(q1: Tensor, k1: Tensor, v1: Tensor, q2: Tensor, k2: Tensor, v2: Tensor, ptr1: Tensor,
                                   ptr2: Tensor, g1: Tensor, g2: Tensor, optr1: Tensor, optr2: Tensor, inv1_ptr: Tensor,
                                   inv1_pairs: Tensor, inv2_ptr: Tensor, inv2_pairs: Tensor, heads: int, rows1: int,
                                   rows2: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """`caster_gvp::cross_attention_pairs_lse` with an autograd formula: -> (o1 [rows1, E1], o2 [rows2, E2], lse1
    [rows1, heads], lse2 [rows2, heads]); the forward IS cgvp_attn_fwd_pairs, so o1 / o2 are bitwise those of
    `cross_attention_pairs`.  (The log-sum-exp are outputs because the backward needs them saved; they carry no
    gradient.  `cross_attention_pairs_train` below returns (o1, o2).)  The inverse tables (`plan_pair_training`) are
    used by the backward alone.  rows1 / rows2 are required: nothing is read back."""
    if rows1 < 0 or rows2 < 0:
        raise ValueError("cross_attention_pairs_train: rows1 / rows2 are required (PairTrainPlan.rows1 / .rows2)")
    _tables(ptr1, ptr2, g1, g2, optr1, optr2, inv1_ptr, inv1_pairs, inv2_ptr, inv2_pairs)
    return pair_scoring._run(q1, k1, v1, q2, k2, v2, ptr1, ptr2, g1, g2, optr1, optr2, heads, rows1, rows2, True)


@cross_attention_pairs_train_op.register_fake
def _(q1, k1, v1, q2, k2, v2, ptr1, ptr2, g1, g2, optr1, optr2, inv1_ptr, inv1_pairs, inv2_ptr, inv2_pairs, heads, rows1, rows2):
    f = lambda t, *s: t.new_empty(s, dtype=torch.float32)
    return f(q1, rows1, q1.shape[1]), f(q2, rows2, q2.shape[1]), f(q1, rows1, heads), f(q2, rows2, heads)


@torch.library.custom_op("caster_gvp::cross_attention_pairs_backward", mutates_args=(), device_types="cuda")
def cross_attention_pairs_backward_op(g_o1: Tensor, g_o2: Tensor, q1: Tensor, k1: Tensor, v1: Tensor, q2: Tensor, k2: Tensor,
                                      v2: Tensor, o1: Tensor, o2: Tensor, lse1: Tensor, lse2: Tensor, ptr1: Tensor,
                                      ptr2: Tensor, g1: Tensor, g2: Tensor, optr1: Tensor, optr2: Tensor, inv1_ptr: Tensor,
                                      inv1_pairs: Tensor, inv2_ptr: Tensor, inv2_pairs: Tensor,
                                      heads: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """-> (g_q1, g_k1, g_v1, g_q2, g_k2, g_v2), gradients of the UNIQUE rows (cgvp_attn_bwd_pairs: per-pair partials, then
    the ordered sum over each graph's pairs; no atomics).  Every row of a graph no pair references is zero, written by the
    kernels.  The ptr tables cover every row (ptr[-1] == rows, as a collated batch has it): rows behind ptr[-1] belong to
    no graph and are not written."""
    hds = pair_scoring._widths(q1, k1, v1, q2, k2, v2, heads)
    ts = [attention_ops._f32(t, "attention operand") for t in (q1, k1, v1, q2, k2, v2)]
    g_o1, g_o2, o1, o2 = (attention_ops._f32(t, "attention gradient") for t in (g_o1, g_o2, o1, o2))
    lse1, lse2 = attention_ops._f32(lse1, "lse"), attention_ops._f32(lse2, "lse")
    (ptr1, ptr2, g1, g2, optr1, optr2, inv1_ptr, inv1_pairs, inv2_ptr, inv2_pairs) = _tables(
        ptr1, ptr2, g1, g2, optr1, optr2, inv1_ptr, inv1_pairs, inv2_ptr, inv2_pairs)
    B, rows1, rows2 = int(g1.numel()), int(o1.shape[0]), int(o2.shape[0])
    if g_o1.shape != o1.shape or g_o2.shape != o2.shape or lse1.shape != (rows1, heads) or lse2.shape != (rows2, heads):
        raise ValueError("cross_attention_pairs_backward: g_o / o / lse shapes disagree")
    dev = ts[0].device
    grads = [torch.empty_like(t) for t in ts]                # g_q1, g_k1, g_v1, g_q2, g_k2, g_v2
    P = (PairsBwdProblem * 2)()
    a = attention_ops._addr
    sides = ((ts[0], ts[1], ts[2], ptr1, ptr2, g1, g2, optr1, optr2, o1, lse1, g_o1, inv1_ptr, inv1_pairs, inv2_ptr, inv2_pairs, 0),
             (ts[3], ts[4], ts[5], ptr2, ptr1, g2, g1, optr2, optr1, o2, lse2, g_o2, inv2_ptr, inv2_pairs, inv1_ptr, inv1_pairs, 3))
    for p, (q, k, v, qp, kp, qg, kg, op, kop, o, lse, g_o, qip, qii, kip, kii, at) in zip(P, sides):
        p.q, p.k, p.v, p.q_ptr, p.k_ptr = a(q), a(k), a(v), qp.data_ptr(), kp.data_ptr()
        p.num_q_graphs, p.num_k_graphs, p.num_q, p.num_k = qp.numel() - 1, kp.numel() - 1, int(q.shape[0]), int(k.shape[0])
        # an empty table still needs an address: the entry point refuses NULL tables before it looks at num_pairs
        p.q_graph, p.k_graph = qg.data_ptr() or qp.data_ptr(), kg.data_ptr() or kp.data_ptr()
        p.out_ptr, p.kout_ptr, p.num_out, p.num_kout = op.data_ptr(), kop.data_ptr(), int(o.shape[0]), rows1 + rows2 - int(o.shape[0])
        p.out, p.lse, p.g_out = a(o), a(lse), a(g_o)
        p.q_inv_ptr, p.q_inv_pairs = qip.data_ptr(), qii.data_ptr() or qip.data_ptr()
        p.k_inv_ptr, p.k_inv_pairs = kip.data_ptr(), kii.data_ptr() or kip.data_ptr()
        p.g_q, p.g_k, p.g_v = a(grads[at]), a(grads[at + 1]), a(grads[at + 2])
    L = lib()
    with torch.cuda.device(dev):
        for first, n, hd, scale in attention_ops.launch_plan(hds):
            need = L.cgvp_attn_bwd_pairs_floats(C.pointer(P[first]), n, heads, hd)
            if need < 0:
                _lib.check(int(need), "cgvp_attn_bwd_pairs_floats")
            ws = torch.empty(max(int(need), 4), dtype=torch.float32, device=dev)     # the call's own: nothing persists
            _lib.check(L.cgvp_attn_bwd_pairs(C.pointer(P[first]), n, B, heads, hd, scale, ws.data_ptr(), ws.numel(), _stream()),
                       "cgvp_attn_bwd_pairs")
    return tuple(grads)


@cross_attention_pairs_backward_op.register_fake
def _(g_o1, g_o2, q1, k1, v1, q2, k2, v2, *rest):
    return tuple(t.new_empty(t.shape, dtype=torch.float32) for t in (q1, k1, v1, q2, k2, v2))


def _attn_setup(ctx, inputs, output):
    ctx.heads = inputs[16]
    ctx.set_materialize_grads(False)          # the log-sum-exp outputs never carry a gradient: no zero fills for them
    ctx.save_for_backward(*inputs[:6], *output, *inputs[6:16])


def _attn_backward(ctx, g_o1, g_o2, g_lse1, g_lse2):
    saved = ctx.saved_tensors                 # q1, k1, v1, q2, k2, v2, o1, o2, lse1, lse2, the ten tables
    if g_o1 is None and g_o2 is None:
        return (None,) * 19
    g_o1 = torch.zeros_like(saved[6]) if g_o1 is None else g_o1
    g_o2 = torch.zeros_like(saved[7]) if g_o2 is None else g_o2
    grads = torch.ops.caster_gvp.cross_attention_pairs_backward(g_o1.contiguous(), g_o2.contiguous(), *saved, ctx.heads)
    return (*grads, *(None,) * 13)


torch.library.register_autograd("caster_gvp::cross_attention_pairs_train", _attn_backward, setup_context=_attn_setup)
torch.library.register_autocast("caster_gvp::cross_attention_pairs_train", "cuda", torch.float32)


def cross_attention_pairs_train(q1, k1, v1, q2, k2, v2, ptr1, ptr2, g1, g2, optr1, optr2, inv1_ptr, inv1_pairs, inv2_ptr,
                                inv2_pairs, heads, rows1, rows2):
    """`caster_gvp::cross_attention_pairs_train` -> (o1 [rows1, E1], o2 [rows2, E2]), differentiable in the six operands.
    Tables and row totals from `plan_pair_training` (`upload`)."""
    return torch.ops.caster_gvp.cross_attention_pairs_train(q1, k1, v1, q2, k2, v2, ptr1, ptr2, g1, g2, optr1, optr2, inv1_ptr,
                                                            inv1_pairs, inv2_ptr, inv2_pairs, heads, rows1, rows2)[:2]


# ------------------------------------------------------------------------------------------------ row copy
@torch.library.custom_op("caster_gvp::expand_rows_train", mutates_args=(), device_types="cuda")
def expand_rows_train_op(src: Tensor, src_ptr: Tensor, g: Tensor, optr: Tensor, inv_ptr: Tensor, inv_pairs: Tensor,
                         num_out: int) -> Tuple[Tensor, Tensor]:
    """`caster_gvp::expand_rows` with an autograd formula: -> (rows [num_out, W], batch [num_out] int64).  The backward is
    cgvp_reduce_rows over (inv_ptr, inv_pairs), the inverse of `g` (`plan_pair_training`)."""
    _table(inv_ptr, "inv_ptr", src_ptr.numel())
    _table(inv_pairs, "inv_pairs", g.numel())
    return pair_scoring._expand(src, src_ptr, g, optr, num_out)


@expand_rows_train_op.register_fake
def _(src, src_ptr, g, optr, inv_ptr, inv_pairs, num_out):
    return src.new_empty((num_out, src.shape[1]), dtype=torch.float32), src.new_empty((num_out,), dtype=torch.int64)


@torch.library.custom_op("caster_gvp::expand_rows_backward", mutates_args=(), device_types="cuda")
def expand_rows_backward_op(g_rows: Tensor, src_ptr: Tensor, optr: Tensor, inv_ptr: Tensor, inv_pairs: Tensor,
                            num_src: int) -> Tensor:
    """-> g_src [num_src, W]: g_src[src_ptr[g] + r] = the sum of g_rows[optr[b] + r] over the pairs b of graph g, in
    ascending b (cgvp_reduce_rows; no atomics).  Rows of a graph no pair references are zero, written by the kernel; rows
    behind src_ptr[-1] belong to no graph and are not written."""
    _on_gpu(g_rows, "g_rows")
    if g_rows.dim() != 2 or g_rows.shape[1] < 4 or g_rows.shape[1] % 4:
        raise NotImplementedError(f"g_rows: expected [rows, W] with W a multiple of 4, got {tuple(g_rows.shape)}")
    g_rows = attention_ops._f32(g_rows, "g_rows")
    src_ptr, inv_pairs = _table(src_ptr, "src_ptr"), _table(inv_pairs, "inv_pairs")
    B = int(inv_pairs.numel())
    optr, inv_ptr = _table(optr, "optr", B + 1), _table(inv_ptr, "inv_ptr", src_ptr.numel())
    if num_src < 0 or src_ptr.numel() < 1:
        raise ValueError("expand_rows_backward: negative num_src or an empty src_ptr")
    dev = g_rows.device
    g_src = torch.empty(num_src, g_rows.shape[1], dtype=torch.float32, device=dev)
    a = attention_ops._addr
    with torch.cuda.device(dev):
        _lib.check(lib().cgvp_reduce_rows(a(g_rows), optr.data_ptr(), inv_ptr.data_ptr(), inv_pairs.data_ptr() or inv_ptr.data_ptr(),
                                          src_ptr.data_ptr(), src_ptr.numel() - 1, B, int(g_rows.shape[0]), num_src,
                                          int(g_rows.shape[1]), a(g_src), _stream()), "cgvp_reduce_rows")
    return g_src


@expand_rows_backward_op.register_fake
def _(g_rows, src_ptr, optr, inv_ptr, inv_pairs, num_src):
    return g_rows.new_empty((num_src, g_rows.shape[1]), dtype=torch.float32)


def _expand_setup(ctx, inputs, output):
    ctx.num_src = inputs[0].shape[0]
    ctx.set_materialize_grads(False)
    ctx.save_for_backward(inputs[1], inputs[3], inputs[4], inputs[5])


def _expand_backward(ctx, g_rows, g_batch):
    if g_rows is None:
        return (None,) * 7
    src_ptr, optr, inv_ptr, inv_pairs = ctx.saved_tensors
    g_src = torch.ops.caster_gvp.expand_rows_backward(g_rows.contiguous(), src_ptr, optr, inv_ptr, inv_pairs, ctx.num_src)
    return (g_src,) + (None,) * 6


torch.library.register_autograd("caster_gvp::expand_rows_train", _expand_backward, setup_context=_expand_setup)
torch.library.register_autocast("caster_gvp::expand_rows_train", "cuda", torch.float32)


def expand_rows_train(src, src_ptr, g, optr, inv_ptr, inv_pairs, num_out):
    """`caster_gvp::expand_rows_train` -> (rows, batch), differentiable in `src`."""
    return torch.ops.caster_gvp.expand_rows_train(src, src_ptr, g, optr, inv_ptr, inv_pairs, num_out)
