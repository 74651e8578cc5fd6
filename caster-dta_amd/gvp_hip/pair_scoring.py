"""Scoring a LIST OF PAIRS drawn from a few unique proteins and molecules: `caster_gvp::cross_attention_pairs`,
`caster_gvp::expand_rows`, `plan_pairs`.

ctypes binding of include/caster_gvp_attnpairs.h (csrc/attn_pairs_kernels.hip), a header and a version of its own beside
the main C ABI: the entry points live in the same libcaster_gvp.so, the signature table below is this module's.

`caster_gvp::cross_attention` ties pair b to rows ptr[b] .. ptr[b+1] on both sides, so a screen of one protein against
1,024 drugs collates -- and encodes, norms and projects -- the same protein 1,024 times.  Nothing before
softmax(Q K^T) V depends on the partner.  Here the projected rows of every unique graph are computed once and the pairing
is two index tables (g1[b]: the protein of pair b, g2[b]: its molecule); only the attention OUTPUT is per pair, at the
offsets `plan_pairs` lays out.  Inference only: no dropout, no autograd.  `JointGNN.score_pairs` is the caller.
"""
from __future__ import annotations

import ctypes as C
import functools
from collections import namedtuple
from typing import Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib, attention_ops
from ._lib import _on_gpu, _stream

ATTN_PAIRS_VERSION = 1   # CGVP_ATTN_PAIRS_VERSION


class PairsProblem(C.Structure):
    """cgvp_attn_pairs_problem (one direction of the cross attention over a pair list)."""
    _fields_ = [("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("q_ptr", C.c_void_p), ("k_ptr", C.c_void_p),
                ("num_q_graphs", C.c_int64), ("num_k_graphs", C.c_int64), ("num_q", C.c_int64), ("num_k", C.c_int64),
                ("q_graph", C.c_void_p), ("k_graph", C.c_void_p), ("out_ptr", C.c_void_p), ("num_out", C.c_int64),
                ("out", C.c_void_p), ("lse", C.c_void_p)]


_P, _I64, _I32 = C.c_void_p, C.c_int64, C.c_int32
_SIGNATURES = {
    "cgvp_attn_pairs_version": (C.c_int, []),
    "cgvp_attn_fwd_pairs": (C.c_int, [C.POINTER(PairsProblem), _I32, _I64, _I32, _I32, C.c_float, _P]),
    "cgvp_expand_rows": (C.c_int, [_P, _P, _P, _P, _I64, _I64, _I32, _P, _P, _P]),
}


def exported_symbols():
    """Names include/caster_gvp_attnpairs.h declares."""
    return tuple(_SIGNATURES)


@functools.lru_cache(maxsize=None)
def lib():
    """libcaster_gvp.so (the handle of `_lib.lib()`) with the pair-list entry points typed (once)."""
    return _lib.bind(_lib.lib(), _SIGNATURES, "cgvp_attn_pairs_version", ATTN_PAIRS_VERSION, "attention-pairs version")


# ------------------------------------------------------------------------------------------------ planner (host only)
# One chunk of a pair list: pairs start .. stop, their graphs, the offsets of their rows in the per-pair arrays of
# either side (prefix sums of the indexed lengths) and the row totals (optr1[-1], optr2[-1]).  numpy int64 throughout.
PairChunk = namedtuple("PairChunk", ["start", "stop", "g1", "g2", "optr1", "optr2", "rows1", "rows2"])


def plan_pairs(len1, len2, pairs, max_rows):
    """Cut a pair list into chunks the device works through one at a time -> [PairChunk].

    `len1` [P] / `len2` [D]: rows of every unique protein / molecule.  `pairs` [K, 2] of (protein, molecule) indices, or
    None for the full cross product in protein-major order.  A chunk is a consecutive run of pairs whose summed protein
    rows plus summed molecule rows stay <= `max_rows` (what the per-pair arrays of one chunk hold); a single pair larger
    than the budget forms a chunk of its own.  K = 0 gives no chunks.  An index outside 0 .. P-1 / 0 .. D-1 raises
    IndexError: the kernels cannot check their device tables, this is where they are checked."""
    len1, len2 = np.asarray(len1, dtype=np.int64).reshape(-1), np.asarray(len2, dtype=np.int64).reshape(-1)
    P, D = int(len1.shape[0]), int(len2.shape[0])
    if (len1 < 0).any() or (len2 < 0).any():
        raise ValueError("negative graph length")
    if pairs is None:
        g1, g2 = np.repeat(np.arange(P, dtype=np.int64), D), np.tile(np.arange(D, dtype=np.int64), P)
    else:
        pairs = np.asarray(pairs)
        if pairs.size and pairs.dtype.kind not in "iu":
            raise TypeError(f"pairs must hold integers, got {pairs.dtype}")
        pairs = pairs.astype(np.int64).reshape(-1, 2)
        g1, g2 = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
        for g, n, what in ((g1, P, "protein"), (g2, D, "molecule")):
            bad = np.nonzero((g < 0) | (g >= n))[0]
            if bad.size:
                raise IndexError(f"pair {int(bad[0])}: {what} index {int(g[bad[0]])} outside 0 .. {n - 1}")
    K = int(g1.shape[0])
    rows1, rows2 = len1[g1], len2[g2]
    cum = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(rows1 + rows2)])
    chunks, s = [], 0
    while s < K:
        # the longest run from s within the budget: the last e with cum[e] - cum[s] <= max_rows; at least one pair
        e = min(max(int(np.searchsorted(cum, cum[s] + int(max_rows), side="right")) - 1, s + 1), K)
        optr1 = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(rows1[s:e])])
        optr2 = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(rows2[s:e])])
        chunks.append(PairChunk(s, e, g1[s:e].copy(), g2[s:e].copy(), optr1, optr2, int(optr1[-1]), int(optr2[-1])))
        s = e
    return chunks


# ------------------------------------------------------------------------------------------------ ops
def _refuse_grad(name, *tensors):
    """The pair-list ops have no backward.  An input that asks for a gradient while gradients are recorded is an error,
    not a silently detached result."""
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        raise RuntimeError(f"{name} is inference only (no autograd formula): call it under torch.no_grad() or detach "
                           "its inputs")


def _table(t, name, numel=None):
    t = attention_ops._i64c(t, name)
    if t.dim() != 1 or (numel is not None and t.numel() != numel):
        raise ValueError(f"{name}: expected a 1-D int64 table" + ("" if numel is None else f" of {numel} entries")
                         + f", got {tuple(t.shape)}")
    return t


def _widths(q1, k1, v1, q2, k2, v2, heads):
    """-> (head_dim of direction 1, head_dim of direction 2): (q1, k1, v1) share one width, (q2, k2, v2) another; side 1
    (proteins) holds the rows of q1 / k2 / v2, side 2 (molecules) those of q2 / k1 / v1."""
    hds = []
    for (qn, q), others in ((("q1", q1), (("k1", k1), ("v1", v1))), (("q2", q2), (("k2", k2), ("v2", v2)))):
        _on_gpu(q, qn)
        hds.append(attention_ops.head_dim_of(q, qn, heads))
        for name, t in others:
            if t.dim() != 2 or t.shape[1] != q.shape[1]:
                raise NotImplementedError(f"{name}: keys and values have the width of their queries ({qn}: {q.shape[1]}), "
                                          f"got {tuple(t.shape)}")
    if not (q1.shape[0] == k2.shape[0] == v2.shape[0] and q2.shape[0] == k1.shape[0] == v1.shape[0]):
        raise ValueError("row counts of the protein-side (q1, k2, v2) / molecule-side (q2, k1, v1) tensors disagree")
    return tuple(hds)


def _run(q1, k1, v1, q2, k2, v2, ptr1, ptr2, g1, g2, optr1, optr2, heads, rows1, rows2, want_lse):
    hds = _widths(q1, k1, v1, q2, k2, v2, heads)
    ts = [attention_ops._f32(t, "attention operand") for t in (q1, k1, v1, q2, k2, v2)]
    ptr1, ptr2, g1 = _table(ptr1, "ptr1"), _table(ptr2, "ptr2"), _table(g1, "g1")
    if ptr1.numel() < 1 or ptr2.numel() < 1:
        raise ValueError("ptr1 / ptr2 must be [num_graphs + 1]")
    B = int(g1.numel())
    g2, optr1, optr2 = _table(g2, "g2", B), _table(optr1, "optr1", B + 1), _table(optr2, "optr2", B + 1)
    dev = ts[0].device
    if rows1 < 0 or rows2 < 0:           # not given: read the totals back (ONE synchronisation; plan_pairs knows them)
        rows1, rows2 = (int(x) for x in torch.stack([optr1[-1], optr2[-1]]).tolist())
    f32 = dict(dtype=torch.float32, device=dev)
    o1, o2 = torch.empty(rows1, heads * hds[0], **f32), torch.empty(rows2, heads * hds[1], **f32)
    lse1 = torch.empty(rows1 if want_lse else 0, heads, **f32)
    lse2 = torch.empty(rows2 if want_lse else 0, heads, **f32)
    P = (PairsProblem * 2)()
    a = attention_ops._addr
    for p, (q, k, v, qp, kp, qg, kg, op, o, lse) in zip(P, ((ts[0], ts[1], ts[2], ptr1, ptr2, g1, g2, optr1, o1, lse1),
                                                            (ts[3], ts[4], ts[5], ptr2, ptr1, g2, g1, optr2, o2, lse2))):
        p.q, p.k, p.v, p.q_ptr, p.k_ptr = a(q), a(k), a(v), qp.data_ptr(), kp.data_ptr()
        p.num_q_graphs, p.num_k_graphs, p.num_q, p.num_k = qp.numel() - 1, kp.numel() - 1, int(q.shape[0]), int(k.shape[0])
        # an empty table still needs an address: the entry point refuses NULL tables before it looks at num_pairs
        p.q_graph, p.k_graph, p.out_ptr = qg.data_ptr() or qp.data_ptr(), kg.data_ptr() or kp.data_ptr(), op.data_ptr()
        p.num_out, p.out, p.lse = int(o.shape[0]), a(o), a(lse)
    fn = lib().cgvp_attn_fwd_pairs
    with torch.cuda.device(dev):
        for first, n, hd, scale in attention_ops.launch_plan(hds):
            _lib.check(fn(C.pointer(P[first]), n, B, heads, hd, scale, _stream()), "cgvp_attn_fwd_pairs")
    return o1, o2, lse1, lse2


@torch.library.custom_op("caster_gvp::cross_attention_pairs", mutates_args=(), device_types="cuda")
def cross_attention_pairs_op(q1: Tensor, k1: Tensor, v1: Tensor, q2: Tensor, k2: Tensor, v2: Tensor, ptr1: Tensor,
                             ptr2: Tensor, g1: Tensor, g2: Tensor, optr1: Tensor, optr2: Tensor, heads: int,
                             rows1: int = -1, rows2: int = -1) -> Tuple[Tensor, Tensor]:
    """-> (o1 [rows1, E1], o2 [rows2, E2]).

    Direction 1: the queries of pair b are the rows ptr1[g1[b]] .. of q1 (the residues of protein g1[b]), its keys /
    values the rows ptr2[g2[b]] .. of k1 / v1 (the atoms of molecule g2[b]); it writes rows optr1[b] .. optr1[b+1] of o1.
    Direction 2 is the mirror image: queries q2 (atoms of g2[b]), keys / values k2 / v2 (residues of g1[b]), output at
    optr2.  (q1, k1, v1) share one width, (q2, k2, v2) another, head_dim = width // heads in {16, 32, 64}: one launch
    when the widths agree, else one per direction.  rows1 / rows2 are optr1[-1] / optr2[-1] as the host knows them
    (`plan_pairs`): with them nothing is read back; left at -1 the op reads the two totals from the device (one
    synchronisation).  The tables are not checked on the device: take them from `plan_pairs`."""
    return _run(q1, k1, v1, q2, k2, v2, ptr1, ptr2, g1, g2, optr1, optr2, heads, rows1, rows2, False)[:2]


@torch.library.custom_op("caster_gvp::cross_attention_pairs_lse", mutates_args=(), device_types="cuda")
def cross_attention_pairs_lse_op(q1: Tensor, k1: Tensor, v1: Tensor, q2: Tensor, k2: Tensor, v2: Tensor, ptr1: Tensor,
                                 ptr2: Tensor, g1: Tensor, g2: Tensor, optr1: Tensor, optr2: Tensor, heads: int,
                                 rows1: int = -1, rows2: int = -1) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """`cross_attention_pairs` that also returns the log-sum-exp: -> (o1, o2, lse1 [rows1, heads], lse2 [rows2, heads])."""
    return _run(q1, k1, v1, q2, k2, v2, ptr1, ptr2, g1, g2, optr1, optr2, heads, rows1, rows2, True)


def _fake_pairs(q1, k1, v1, q2, k2, v2, ptr1, ptr2, g1, g2, optr1, optr2, heads, rows1, rows2):
    if rows1 < 0 or rows2 < 0:
        raise RuntimeError("caster_gvp::cross_attention_pairs: pass rows1 / rows2 to trace the op (the totals are data)")
    f = lambda t, *s: t.new_empty(s, dtype=torch.float32)
    return f(q1, rows1, q1.shape[1]), f(q2, rows2, q2.shape[1])


@cross_attention_pairs_op.register_fake
def _(q1, k1, v1, q2, k2, v2, ptr1, ptr2, g1, g2, optr1, optr2, heads, rows1=-1, rows2=-1):
    return _fake_pairs(q1, k1, v1, q2, k2, v2, ptr1, ptr2, g1, g2, optr1, optr2, heads, rows1, rows2)


@cross_attention_pairs_lse_op.register_fake
def _(q1, k1, v1, q2, k2, v2, ptr1, ptr2, g1, g2, optr1, optr2, heads, rows1=-1, rows2=-1):
    o1, o2 = _fake_pairs(q1, k1, v1, q2, k2, v2, ptr1, ptr2, g1, g2, optr1, optr2, heads, rows1, rows2)
    return o1, o2, q1.new_empty((rows1, heads), dtype=torch.float32), q2.new_empty((rows2, heads), dtype=torch.float32)


@torch.library.custom_op("caster_gvp::expand_rows", mutates_args=(), device_types="cuda")
def expand_rows_op(src: Tensor, src_ptr: Tensor, g: Tensor, optr: Tensor, num_out: int) -> Tuple[Tensor, Tensor]:
    """-> (rows [num_out, W] with rows[optr[b] + r] = src[src_ptr[g[b]] + r], batch [num_out] int64 with
    batch[optr[b] + r] = b).  W is a multiple of 4; num_out is optr[-1] as the host knows it (`plan_pairs`)."""
    return _expand(src, src_ptr, g, optr, num_out)


def _expand(src, src_ptr, g, optr, num_out):
    _on_gpu(src, "src")
    if src.dim() != 2 or src.shape[1] < 4 or src.shape[1] % 4:
        raise NotImplementedError(f"src: expected [rows, W] with W a multiple of 4, got {tuple(src.shape)}")
    src = attention_ops._f32(src, "src")
    src_ptr, g = _table(src_ptr, "src_ptr"), _table(g, "g")
    B = int(g.numel())
    optr = _table(optr, "optr", B + 1)
    if num_out < 0 or src_ptr.numel() < 1:
        raise ValueError("expand_rows: negative num_out or an empty src_ptr")
    dev = src.device
    rows = torch.empty(num_out, src.shape[1], dtype=torch.float32, device=dev)
    batch = torch.empty(num_out, dtype=torch.int64, device=dev)
    a = attention_ops._addr
    with torch.cuda.device(dev):
        _lib.check(lib().cgvp_expand_rows(a(src), src_ptr.data_ptr(), g.data_ptr() or src_ptr.data_ptr(), optr.data_ptr(), B,
                                          num_out, int(src.shape[1]), a(rows), a(batch), _stream()), "cgvp_expand_rows")
    return rows, batch


@expand_rows_op.register_fake
def _(src, src_ptr, g, optr, num_out):
    return src.new_empty((num_out, src.shape[1]), dtype=torch.float32), src.new_empty((num_out,), dtype=torch.int64)


for _name in ("caster_gvp::cross_attention_pairs", "caster_gvp::cross_attention_pairs_lse", "caster_gvp::expand_rows"):
    torch.library.register_autocast(_name, "cuda", torch.float32)


def cross_attention_pairs(q1, k1, v1, q2, k2, v2, ptr1, ptr2, g1, g2, optr1, optr2, heads, rows1=-1, rows2=-1, lse=False):
    """`caster_gvp::cross_attention_pairs` (with `lse=True`: `caster_gvp::cross_attention_pairs_lse`) behind the check the
    ops themselves cannot make: an input that requires grad while gradients are recorded raises."""
    _refuse_grad("caster_gvp::cross_attention_pairs", q1, k1, v1, q2, k2, v2)
    op = torch.ops.caster_gvp.cross_attention_pairs_lse if lse else torch.ops.caster_gvp.cross_attention_pairs
    return op(q1, k1, v1, q2, k2, v2, ptr1, ptr2, g1, g2, optr1, optr2, heads, rows1, rows2)


def expand_rows(src, src_ptr, g, optr, num_out):
    """`caster_gvp::expand_rows` behind the same check."""
    _refuse_grad("caster_gvp::expand_rows", src)
    return torch.ops.caster_gvp.expand_rows(src, src_ptr, g, optr, num_out)
