"""Varlen residue <-> atom cross attention as `torch.library` custom ops.

`caster_gvp::cross_attention` is the part of the two nn.MultiheadAttention modules of CrossAttentionModule
(joint_gnn.py:321-409) that lies between their input and output projections, for BOTH directions in one launch, on
compact row arrays with ptr offsets (no to_dense_batch padding, no key-padding masks, no score tensor in HBM):

    o_r[q] = softmax_k(q_r[q] . k_a[k] / sqrt(head_dim)) v_a[k]      residues attend to the atoms of their pair
    o_a[q] = softmax_k(q_a[q] . k_r[k] / sqrt(head_dim)) v_r[k]      atoms attend to the residues of their pair

head_dim = width // heads is 16, 32 or 64 (include/caster_gvp_attnhd.h), per direction: (q_r, k_a, v_a) have one width
and (q_a, k_r, v_r) another.  Equal widths go in one launch, unequal ones in one launch each on the same stream.
The projections themselves stay plain library GEMMs (F.linear on [N, E] rows).  Registered with fake kernels,
autograd (the backward is the op `cross_attention_backward`: two launches, no atomics) and an autocast rule (fp32),
like the encoders.  `cross_attention_weights` produces nn.MultiheadAttention's head-averaged weights in the
reference's dense [B, Lq_max, Lk_max] layout for inference (inference/evaluation.py:43-66).
"""
from __future__ import annotations

import ctypes as C
import functools
import math
from typing import Tuple

import torch
from torch import Tensor

from . import _lib
from .ops import _f32, _ptr, _stream

HEAD_DIM = 16                # the shipped module: embed 128, 8 heads
HEAD_DIMS = (16, 32, 64)     # what the kernels are compiled for

# include/caster_gvp_attnhd.h: every attention entry point with the head width as an argument -- a header, a version
# and a signature table of their own, bound on the handle of `_lib.lib()`.  (cgvp_attn_node_scores_hd takes the problem
# struct of gvp_hip.attention_scores, which types it there.)
ATTN_HD_VERSION = 1          # CGVP_ATTN_HD_VERSION
_HD_ARGS = [C.POINTER(_lib.AttnProblem), C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_float]
_HD_SIGNATURES = {
    "cgvp_attn_hd_version": (C.c_int, []),
    "cgvp_attn_fwd_hd": (C.c_int, _HD_ARGS + [C.POINTER(_lib.Rng), C.c_void_p]),
    "cgvp_attn_bwd_hd": (C.c_int, _HD_ARGS + [C.POINTER(_lib.Rng), C.c_void_p]),
    "cgvp_attn_weights_hd": (C.c_int, _HD_ARGS + [C.c_void_p]),
}


def hd_exported_symbols():
    """Names include/caster_gvp_attnhd.h declares."""
    return tuple(_HD_SIGNATURES) + ("cgvp_attn_node_scores_hd",)


@functools.lru_cache(maxsize=None)
def hd_lib():
    """libcaster_gvp.so (the handle of `_lib.lib()`) with the head-width entry points typed (once)."""
    return _lib.bind(_lib.lib(), _HD_SIGNATURES, "cgvp_attn_hd_version", ATTN_HD_VERSION, "attention head-width version")


def _i64c(t, name):
    if not t.is_cuda:
        raise RuntimeError(f"{name}: caster-dta_amd runs on MI355X only (got a {t.device} tensor)")
    return t.to(torch.int64).contiguous()


def _problems(q_r, k_a, v_a, q_a, k_r, v_r, rptr, aptr):
    P = (_lib.AttnProblem * 2)()
    for p, (q, k, v, qp, kp) in zip(P, ((q_r, k_a, v_a, rptr, aptr), (q_a, k_r, v_r, aptr, rptr))):
        p.q, p.k, p.v = q.data_ptr(), k.data_ptr(), v.data_ptr()
        p.q_ptr, p.k_ptr = qp.data_ptr(), kp.data_ptr()
        p.num_q, p.num_k = int(q.shape[0]), int(k.shape[0])
    return P


def head_dim_of(t, name, heads):
    """width // heads of a [rows, width] operand; NotImplementedError unless it is one of HEAD_DIMS."""
    hd, rest = divmod(int(t.shape[1]), heads) if t.dim() == 2 and heads >= 1 else (0, 1)
    if rest or hd not in HEAD_DIMS:
        raise NotImplementedError(f"{name}: the attention kernels are compiled for head_dim 16, 32 and 64 "
                                  f"(embed = heads * head_dim), got {tuple(t.shape)} with {heads} heads")
    return hd


def _check_rows(r0, r1, r2, a0, a1, a2, rptr, aptr):
    """What every attention op asks of its row counts: the three residue-side tensors agree, the three atom-side tensors
    agree, and rptr / aptr are both [num_pairs + 1].  (gvp_hip.attention_scores uses it too.)"""
    if not (r0.shape[0] == r1.shape[0] == r2.shape[0] and a0.shape[0] == a1.shape[0] == a2.shape[0]):
        raise ValueError("row counts of the residue / atom tensors disagree")
    if rptr.shape != aptr.shape or rptr.dim() != 1 or rptr.numel() < 1:
        raise ValueError("rptr / aptr must both be [num_pairs + 1]")


def _check(q_r, k_a, v_a, q_a, k_r, v_r, rptr, aptr, heads):
    """The width rule of the shipped head shape alone: every operand is [rows, 16 * heads].  No op calls it (they take
    `_check_hd`); tests/test_attention_edges.py holds it to its refusals, one of which (4 heads at width 128) is a shape
    `_check_hd` accepts."""
    E = heads * HEAD_DIM
    for name, t in (("q_r", q_r), ("k_a", k_a), ("v_a", v_a), ("q_a", q_a), ("k_r", k_r), ("v_r", v_r)):
        if t.dim() != 2 or t.shape[1] != E:
            raise NotImplementedError(f"{name}: the attention kernels are compiled for head_dim 16 "
                                      f"(embed = 16 * heads = {E}), got {tuple(t.shape)}")
    _check_rows(q_r, k_r, v_r, q_a, k_a, v_a, rptr, aptr)


def _check_hd(q_r, k_a, v_a, q_a, k_r, v_r, rptr, aptr, heads):
    """-> (head_dim of the residue-query direction, head_dim of the atom-query direction), each of HEAD_DIMS."""
    hds = []
    for (qn, q), others in ((("q_r", q_r), (("k_a", k_a), ("v_a", v_a))), (("q_a", q_a), (("k_r", k_r), ("v_r", v_r)))):
        hds.append(head_dim_of(q, qn, heads))
        for name, t in others:
            if t.dim() != 2 or t.shape[1] != q.shape[1]:
                raise NotImplementedError(f"{name}: keys and values have the width of their queries "
                                          f"({qn}: {q.shape[1]} = {heads} heads x head_dim {hds[-1]}), got {tuple(t.shape)}")
    _check_rows(q_r, k_r, v_r, q_a, k_a, v_a, rptr, aptr)
    return tuple(hds)


def launch_plan(hds):
    """(first problem, number of problems, head_dim, scale = 1 / sqrt(head_dim)) of every launch of an entry point of
    caster_gvp_attnhd.h on both directions: ONE launch with two problems when their head dims agree, else one launch with
    one problem each, on the same stream."""
    if hds[0] == hds[1]:
        return ((0, 2, hds[0], 1.0 / math.sqrt(hds[0])),)
    return ((0, 1, hds[0], 1.0 / math.sqrt(hds[0])), (1, 1, hds[1], 1.0 / math.sqrt(hds[1])))


def _launch(name, P, B, heads, hds, R=None):
    fn = getattr(hd_lib(), name)
    for first, n, hd, scale in launch_plan(hds):
        args = [C.pointer(P[first]), n, B, heads, hd, scale]
        if name != "cgvp_attn_weights_hd":
            args.append(None if R is None else C.pointer(R[first]))
        _lib.check(fn(*args, _stream()), name)


def _addr(t):
    return _ptr(t).value or 0


# ------------------------------------------------------------------------------------------------ attention dropout
# include/caster_gvp_attndrop.h: the same kernels with nn.MultiheadAttention's training-mode dropout on the softmax
# probabilities, factors regenerated in the kernels from the step's {seed, offset} pair -- a header, a version and a
# signature table of their own, bound on the handle of `_lib.lib()`.  The ops below go through the _hd entry points,
# where a NULL generator is "no dropout": `cross_attention` and `cross_attention_dropout` share one body, the second
# with the trailing arguments `drop` = (pair, site_r, site_a, p_r, p_a).
ATTN_DROPOUT_VERSION = 1     # CGVP_ATTN_DROPOUT_VERSION
DROPOUT_MAX_HEADS = 128      # CGVP_ATTN_DROPOUT_MAX_HEADS

_DROP_ARGS = [C.POINTER(_lib.AttnProblem), C.c_int32, C.c_int64, C.c_int32, C.c_float, C.POINTER(_lib.Rng), C.c_void_p]
_DROP_SIGNATURES = {
    "cgvp_attn_dropout_version": (C.c_int, []),
    "cgvp_attn_fwd_dropout": (C.c_int, _DROP_ARGS),
    "cgvp_attn_bwd_dropout": (C.c_int, _DROP_ARGS),
}


def dropout_exported_symbols():
    """Names include/caster_gvp_attndrop.h declares."""
    return tuple(_DROP_SIGNATURES)


@functools.lru_cache(maxsize=None)
def dropout_lib():
    """libcaster_gvp.so (the handle of `_lib.lib()`) with the attention-dropout entry points typed (once)."""
    return _lib.bind(_lib.lib(), _DROP_SIGNATURES, "cgvp_attn_dropout_version", ATTN_DROPOUT_VERSION,
                     "attention-dropout version")


def _rngs(pair, site_r, site_a, p_r, p_a):
    if pair.dtype != torch.int64 or pair.numel() != 2 or not pair.is_cuda or not pair.is_contiguous():
        raise ValueError("pair must be the int64[2] {seed, offset} of caster_gvp::rng_next on the GPU")
    R = (_lib.Rng * 2)()
    for r, site, p in zip(R, (site_r, site_a), (p_r, p_a)):
        r.seed, r.p, r.stream = pair.data_ptr(), float(p), int(site)
    return R


def _forward(q_r, k_a, v_a, q_a, k_r, v_r, rptr, aptr, heads, *drop):
    hds = _check_hd(q_r, k_a, v_a, q_a, k_r, v_r, rptr, aptr, heads)
    ts = [_f32(t, "attention operand") for t in (q_r, k_a, v_a, q_a, k_r, v_r)]
    rptr, aptr = _i64c(rptr, "rptr"), _i64c(aptr, "aptr")
    dev = ts[0].device
    N, Na, B = int(q_r.shape[0]), int(q_a.shape[0]), int(rptr.numel()) - 1
    f32 = dict(dtype=torch.float32, device=dev)
    o_r, o_a = torch.empty(N, heads * hds[0], **f32), torch.empty(Na, heads * hds[1], **f32)
    lse_r, lse_a = torch.empty(N, heads, **f32), torch.empty(Na, heads, **f32)
    P = _problems(*ts, rptr, aptr)
    for p, o, lse in zip(P, (o_r, o_a), (lse_r, lse_a)):
        p.out, p.lse = _addr(o), _addr(lse)
    R = _rngs(*drop) if drop else None
    with torch.cuda.device(dev):
        _launch("cgvp_attn_fwd_hd", P, B, heads, hds, R)
    return o_r, o_a, lse_r, lse_a


def _backward(g_o_r, g_o_a, q_r, k_a, v_a, q_a, k_r, v_r, o_r, o_a, lse_r, lse_a, rptr, aptr, heads, *drop):
    hds = (head_dim_of(q_r, "q_r", heads), head_dim_of(q_a, "q_a", heads))      # (the forward checked the rest)
    ts = [_f32(t, "attention operand") for t in (q_r, k_a, v_a, q_a, k_r, v_r)]
    g_o_r, g_o_a, o_r, o_a = (_f32(t, "attention gradient") for t in (g_o_r, g_o_a, o_r, o_a))
    lse_r, lse_a = _f32(lse_r, "lse"), _f32(lse_a, "lse")
    rptr, aptr = _i64c(rptr, "rptr"), _i64c(aptr, "aptr")
    dev = ts[0].device
    B = int(rptr.numel()) - 1
    outs = [torch.empty_like(t) for t in ts]                 # g_q_r, g_k_a, g_v_a, g_q_a, g_k_r, g_v_r
    d_r, d_a = torch.empty_like(lse_r), torch.empty_like(lse_a)
    P = _problems(*ts, rptr, aptr)
    for i, (p, o, lse, g_o, d) in enumerate(zip(P, (o_r, o_a), (lse_r, lse_a), (g_o_r, g_o_a), (d_r, d_a))):
        p.out, p.lse, p.g_out, p.delta = _addr(o), _addr(lse), _addr(g_o), _addr(d)
        p.g_q, p.g_k, p.g_v = _addr(outs[3 * i]), _addr(outs[3 * i + 1]), _addr(outs[3 * i + 2])
    R = _rngs(*drop) if drop else None
    with torch.cuda.device(dev):
        _launch("cgvp_attn_bwd_hd", P, B, heads, hds, R)
    return tuple(outs)


def _fake_forward(q_r, k_a, v_a, q_a, k_r, v_r, rptr, aptr, heads, *drop):
    f = lambda t, *s: t.new_empty(s, dtype=torch.float32)
    return (f(q_r, q_r.shape[0], q_r.shape[1]), f(q_a, q_a.shape[0], q_a.shape[1]), f(q_r, q_r.shape[0], heads),
            f(q_a, q_a.shape[0], heads))


def _fake_backward(g_o_r, g_o_a, q_r, k_a, v_a, q_a, k_r, v_r, *rest):
    return tuple(t.new_empty(t.shape, dtype=torch.float32) for t in (q_r, k_a, v_a, q_a, k_r, v_r))


@torch.library.custom_op("caster_gvp::cross_attention", mutates_args=(), device_types="cuda")
def cross_attention_op(q_r: Tensor, k_a: Tensor, v_a: Tensor, q_a: Tensor, k_r: Tensor, v_r: Tensor, rptr: Tensor,
                       aptr: Tensor, heads: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """-> (o_r [N, E], o_a [Na, E], lse_r [N, heads], lse_a [Na, heads])."""
    return _forward(q_r, k_a, v_a, q_a, k_r, v_r, rptr, aptr, heads)


@torch.library.custom_op("caster_gvp::cross_attention_backward", mutates_args=(), device_types="cuda")
def cross_attention_backward_op(g_o_r: Tensor, g_o_a: Tensor, q_r: Tensor, k_a: Tensor, v_a: Tensor, q_a: Tensor,
                                k_r: Tensor, v_r: Tensor, o_r: Tensor, o_a: Tensor, lse_r: Tensor, lse_a: Tensor,
                                rptr: Tensor, aptr: Tensor,
                                heads: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """-> (g_q_r, g_k_a, g_v_a, g_q_a, g_k_r, g_v_r)."""
    return _backward(g_o_r, g_o_a, q_r, k_a, v_a, q_a, k_r, v_r, o_r, o_a, lse_r, lse_a, rptr, aptr, heads)


@torch.library.custom_op("caster_gvp::cross_attention_dropout", mutates_args=(), device_types="cuda")
def cross_attention_dropout_op(q_r: Tensor, k_a: Tensor, v_a: Tensor, q_a: Tensor, k_r: Tensor, v_r: Tensor, rptr: Tensor,
                               aptr: Tensor, heads: int, pair: Tensor, site_r: int, site_a: int, p_r: float,
                               p_a: float) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """`cross_attention` with dropout on the softmax probabilities (nn.MultiheadAttention in training mode):
    o = (softmax(q k^T / sqrt(head_dim)) o f) v, f in {0, 1/(1-p)} a pure function of (pair, site, head, query row, key row).
    -> (o_r, o_a, lse_r, lse_a); the lse are those of the UNdropped scores.  p_r = p_a = 0 is `cross_attention`."""
    return _forward(q_r, k_a, v_a, q_a, k_r, v_r, rptr, aptr, heads, pair, site_r, site_a, p_r, p_a)


@torch.library.custom_op("caster_gvp::cross_attention_dropout_backward", mutates_args=(), device_types="cuda")
def cross_attention_dropout_backward_op(g_o_r: Tensor, g_o_a: Tensor, q_r: Tensor, k_a: Tensor, v_a: Tensor, q_a: Tensor,
                                        k_r: Tensor, v_r: Tensor, o_r: Tensor, o_a: Tensor, lse_r: Tensor, lse_a: Tensor,
                                        rptr: Tensor, aptr: Tensor, heads: int, pair: Tensor, site_r: int, site_a: int,
                                        p_r: float, p_a: float) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """-> (g_q_r, g_k_a, g_v_a, g_q_a, g_k_r, g_v_r); `pair`, sites and p are the forward's: the factors are regenerated."""
    return _backward(g_o_r, g_o_a, q_r, k_a, v_a, q_a, k_r, v_r, o_r, o_a, lse_r, lse_a, rptr, aptr, heads,
                     pair, site_r, site_a, p_r, p_a)


def _attn_setup(ctx, inputs, output):
    """inputs: the six operands, rptr, aptr, heads[, pair, site_r, site_a, p_r, p_a]; output: (o_r, o_a, lse_r, lse_a)."""
    ctx.heads, ctx.drop = inputs[8], inputs[10:]
    ctx.set_materialize_grads(False)          # the log-sum-exp outputs never carry a gradient: no zero fills for them
    ctx.save_for_backward(*inputs[:6], *output, *inputs[6:8], *inputs[9:10])


def _attn_backward(ctx, g_o_r, g_o_a, g_lse_r, g_lse_a):
    saved = ctx.saved_tensors                 # q_r, k_a, v_a, q_a, k_r, v_r, o_r, o_a, lse_r, lse_a, rptr, aptr[, pair]
    nones = (None,) * (len(saved) - 9 + len(ctx.drop))          # rptr, aptr, heads[, pair, sites, ps]
    if g_o_r is None and g_o_a is None:
        return (None,) * 6 + nones
    g_o_r = torch.zeros_like(saved[6]) if g_o_r is None else g_o_r
    g_o_a = torch.zeros_like(saved[7]) if g_o_a is None else g_o_a
    op = torch.ops.caster_gvp.cross_attention_dropout_backward if ctx.drop else torch.ops.caster_gvp.cross_attention_backward
    grads = op(g_o_r.contiguous(), g_o_a.contiguous(), *saved[:12], ctx.heads, *saved[12:], *ctx.drop)
    # the two directions share no operand: a residue-side tensor gets its gradient from exactly one of them
    return (*grads, *nones)


cross_attention_op.register_fake(_fake_forward)
cross_attention_dropout_op.register_fake(_fake_forward)
cross_attention_backward_op.register_fake(_fake_backward)
cross_attention_dropout_backward_op.register_fake(_fake_backward)
for _name in ("caster_gvp::cross_attention", "caster_gvp::cross_attention_dropout"):
    torch.library.register_autograd(_name, _attn_backward, setup_context=_attn_setup)
    torch.library.register_autocast(_name, "cuda", torch.float32)


@torch.library.custom_op("caster_gvp::cross_attention_weights", mutates_args=(), device_types="cuda")
def cross_attention_weights_op(q_r: Tensor, k_a: Tensor, lse_r: Tensor, q_a: Tensor, k_r: Tensor, lse_a: Tensor,
                               rptr: Tensor, aptr: Tensor, heads: int, r_max: int,
                               a_max: int) -> Tuple[Tensor, Tensor]:
    """-> (w_r [B, r_max, a_max], w_a [B, a_max, r_max]): head-averaged attention weights, zero in the padding.
    A pair with more than r_max residues or a_max atoms is truncated to the layout (its kept entries unchanged)."""
    hds = _check_hd(q_r, k_a, k_a, q_a, k_r, k_r, rptr, aptr, heads)
    ts = [_f32(t, "attention operand") for t in (q_r, k_a, k_a, q_a, k_r, k_r)]
    lse_r, lse_a = _f32(lse_r, "lse"), _f32(lse_a, "lse")
    rptr, aptr = _i64c(rptr, "rptr"), _i64c(aptr, "aptr")
    dev = ts[0].device
    B = int(rptr.numel()) - 1
    w_r = torch.zeros(B, r_max, a_max, dtype=torch.float32, device=dev)
    w_a = torch.zeros(B, a_max, r_max, dtype=torch.float32, device=dev)
    if w_r.numel() == 0:                                     # no pair, or one side empty in every pair: nothing to write
        return w_r, w_a
    dummy_r, dummy_a = torch.empty(1, device=dev), torch.empty(1, device=dev)    # `out` is not written by this entry point
    P = _problems(*ts, rptr, aptr)
    P[0].out, P[0].lse, P[0].weights, P[0].weights_lq, P[0].weights_lk = _addr(dummy_r), _addr(lse_r), _addr(w_r), r_max, a_max
    P[1].out, P[1].lse, P[1].weights, P[1].weights_lq, P[1].weights_lk = _addr(dummy_a), _addr(lse_a), _addr(w_a), a_max, r_max
    with torch.cuda.device(dev):
        _launch("cgvp_attn_weights_hd", P, B, heads, hds)
    return w_r, w_a


@cross_attention_weights_op.register_fake
def _(q_r, k_a, lse_r, q_a, k_r, lse_a, rptr, aptr, heads, r_max, a_max):
    B = rptr.shape[0] - 1
    return (q_r.new_empty((B, r_max, a_max), dtype=torch.float32), q_r.new_empty((B, a_max, r_max), dtype=torch.float32))
