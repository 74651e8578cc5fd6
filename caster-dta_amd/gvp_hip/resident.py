"""Batches collated ON THE DEVICE from a resident set of unique graphs: `ResidentGraphs`, `CollatePlan`, `ResidentPairs`.

ctypes binding of include/caster_gvp_resident.h (csrc/resident_kernels.hip), a header and a version of its own beside the
main C ABI: the entry points live in the same libcaster_gvp.so, the signature table below is this module's.

A CASTER-DTA dataset is a few hundred unique graphs reused across tens of thousands of pairs (Davis: 442 proteins x 68
drugs, 30,056 pairs).  `ResidentGraphs` keeps one side's unique graphs on the device, each field concatenated once;
`plan(ids)` is host arithmetic over the graphs' node and edge counts plus ONE upload of a packed int64 table;
`collate(plan)` is ONE launch that assembles the batch -- bitwise what `davis_synth.collate` of the same graphs and an
upload give -- with no host read, no further upload and no synchronisation, on the stream of the call.  Nothing is kept
between calls, so with `out=` buffers and a ready plan the call can be captured into a HIP graph, and overwriting
`plan.table` in place with the table of another plan of the same (B, N, E) replays the other batch.
"""
from __future__ import annotations

import ctypes as C
import functools
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._lib import _stream

RESIDENT_VERSION = 1     # CGVP_RESIDENT_VERSION
MAX_ITEMS = 16           # CGVP_COLLATE_MAX_ITEMS
NODE_ROWS, EDGE_ROWS, ENDPOINTS, BATCH = 0, 1, 2, 3      # CGVP_COLLATE_*


class CollateItem(C.Structure):
    """cgvp_collate_item: one tensor of the batch and the resident tensor it is assembled from."""
    _fields_ = [("dst", C.c_void_p), ("src", C.c_void_p), ("row_bytes", C.c_int32), ("kind", C.c_int32)]


_P, _I64, _I32 = C.c_void_p, C.c_int64, C.c_int32
_SIGNATURES = {
    "cgvp_resident_version": (C.c_int, []),
    "cgvp_collate_graphs": (C.c_int, [C.POINTER(CollateItem), _I32, _P, _P, _P, _P, _P, _I64, _I64, _I64, _I32, _P]),
}


def exported_symbols():
    """Names include/caster_gvp_resident.h declares."""
    return tuple(_SIGNATURES)


@functools.lru_cache(maxsize=None)
def lib():
    """libcaster_gvp.so (the handle of `_lib.lib()`) with the resident-collate entry points typed (once)."""
    return _lib.bind(_lib.lib(), _SIGNATURES, "cgvp_resident_version", RESIDENT_VERSION, "resident version")


# ------------------------------------------------------------------------------------------------ host tables
def _index_array(ids, limit, what):
    """`ids` as a flat int64 array: TypeError for anything but integers, IndexError outside 0 .. limit-1."""
    if torch.is_tensor(ids):
        ids = ids.detach().cpu().numpy()
    a = np.asarray(ids)
    if a.size == 0:
        return np.zeros(0, dtype=np.int64)
    if a.dtype.kind not in "iu":
        raise TypeError(f"{what} must be integers, got {a.dtype}")
    a = a.reshape(-1).astype(np.int64)
    if a.min() < 0 or a.max() >= limit:
        bad = a[(a < 0) | (a >= limit)][0]
        raise IndexError(f"{what}: index {int(bad)} is outside 0 .. {limit - 1}")
    return a


def _offsets(counts):
    return np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(counts, dtype=np.int64)])


def plan_tables(node_off, edge_off, ids):
    """The host half of `ResidentGraphs.plan`, from a store's offsets alone -> (sel [B], dst_node_off [B+1],
    dst_edge_off [B+1]), numpy int64."""
    node_off, edge_off = np.asarray(node_off, dtype=np.int64), np.asarray(edge_off, dtype=np.int64)
    sel = _index_array(ids, node_off.shape[0] - 1, "graph ids")
    return sel, _offsets(np.diff(node_off)[sel]), _offsets(np.diff(edge_off)[sel])


class CollatePlan(namedtuple("CollatePlan", ["sel", "node_off", "edge_off", "N", "E", "B", "table"])):
    """One batch of a store: `sel` [B] the unique graph of every position, `node_off` / `edge_off` [B+1] the positions'
    row offsets in the batch (numpy int64, host), the totals `N`, `E`, `B` (ints) and `table`, ONE packed int64 tensor on
    the store's device = sel | node_off | edge_off (slices of an int64 vector keep the 8-byte alignment the entry point
    asks for).  `ptr` of the batch is a slice of it."""

    @property
    def ptr(self):
        return self.table[self.B:2 * self.B + 1]


# ------------------------------------------------------------------------------------------------ one side's store
_FLOAT_FIELDS, _INT_FIELDS = ("x_s", "x_v", "e_s", "e_v"), ("ntypes", "etypes", "edge_index")
_NODE_FIELDS = ("x_s", "x_v", "ntypes")


def _row_bytes(t):
    return int(np.prod(t.shape[1:], dtype=np.int64)) * t.element_size()


def _field(g, name, i):
    a = g[name]
    if a is None:
        return None
    t = a.detach().cpu() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    want = torch.float32 if name in _FLOAT_FIELDS else torch.int64
    if t.dtype != want:
        raise NotImplementedError(f"graph {i}: {name} is {t.dtype}; a resident store holds {want} "
                                  f"{'features' if want.is_floating_point else 'indices'} only")
    return t


class ResidentGraphs:
    """One side of a dataset on the device.  `graphs`: per-graph dicts in the layout of `davis_synth.protein_graph` /
    `drug_graph` (x_s, x_v or None, edge_index with LOCAL node ids, e_s, e_v or None, ntypes, etypes; numpy arrays or
    torch tensors).  Built once: every field is concatenated over the graphs and moved to `device`; `node_off` /
    `edge_off` [len + 1] are kept on the host (numpy int64) and on the device.  fp32 features and int64 indices only."""

    def __init__(self, graphs, device):
        graphs = list(graphs)
        if not graphs:
            raise ValueError("ResidentGraphs: no graphs")
        self.device = torch.device(device)
        cols = {n: [_field(g, n, i) for i, g in enumerate(graphs)] for n in _FLOAT_FIELDS + _INT_FIELDS}
        self.vector = cols["x_v"][0] is not None
        for n in ("x_v", "e_v"):
            if any((t is not None) != self.vector for t in cols[n]):
                raise ValueError(f"ResidentGraphs: {n} must be given for every graph or for none")
        for i, g in enumerate(graphs):
            n, e = cols["x_s"][i].shape[0], cols["edge_index"][i].shape[1]
            if cols["edge_index"][i].dim() != 2 or cols["edge_index"][i].shape[0] != 2:
                raise ValueError(f"graph {i}: edge_index must be [2, E]")
            for name in _FLOAT_FIELDS + ("ntypes", "etypes"):
                t = cols[name][i]
                if t is not None and t.shape[0] != (n if name in _NODE_FIELDS else e):
                    raise ValueError(f"graph {i}: {name} has {t.shape[0]} rows, expected {n if name in _NODE_FIELDS else e}")
            if e and n and (int(cols["edge_index"][i].min()) < 0 or int(cols["edge_index"][i].max()) >= n):
                raise ValueError(f"graph {i}: edge_index leaves its {n} nodes (ids must be local)")
            if e and not n:
                raise ValueError(f"graph {i}: edges without nodes")
        self.node_off = _offsets([t.shape[0] for t in cols["x_s"]])
        self.edge_off = _offsets([t.shape[1] for t in cols["edge_index"]])
        names = [n for n in _FLOAT_FIELDS + ("ntypes", "etypes") if self.vector or n not in ("x_v", "e_v")]
        host = {n: torch.cat(cols[n], dim=0).contiguous() for n in names}
        host["edge_index"] = torch.cat(cols["edge_index"], dim=1).contiguous()
        for n, t in host.items():
            row = 8 if n == "edge_index" else _row_bytes(t)
            if row < 4 or row % 4:
                raise NotImplementedError(f"ResidentGraphs: a row of {n} has {row} bytes, not a multiple of 4")
        self.tensors = {n: t.to(self.device) for n, t in host.items()}
        # one upload: node_off | edge_off
        self.offsets = torch.from_numpy(np.concatenate([self.node_off, self.edge_off])).to(self.device)
        self.device = self.offsets.device          # "cuda" -> the device the tensors landed on

    def __len__(self):
        return int(self.node_off.shape[0] - 1)

    def num_nodes(self, i):
        return int(self.node_off[i + 1] - self.node_off[i])

    def num_edges(self, i):
        return int(self.edge_off[i + 1] - self.edge_off[i])

    @property
    def nbytes(self):
        """Bytes the store holds on the device (features, indices and the two offset tables)."""
        return int(sum(t.numel() * t.element_size() for t in self.tensors.values())
                   + self.offsets.numel() * self.offsets.element_size())

    # -------------------------------------------------------------------------------------------- plan
    def plan(self, ids):
        """The batch of unique graphs `ids` (a sequence or integer array, in batch order, repeats allowed) ->
        CollatePlan.  Host arithmetic and ONE upload.  IndexError for an index outside 0 .. len-1, TypeError for
        non-integers, both before anything is uploaded.  An empty `ids` is legal (B = 0, ptr = [0])."""
        sel, node_off, edge_off = plan_tables(self.node_off, self.edge_off, ids)
        table = torch.from_numpy(np.concatenate([sel, node_off, edge_off])).to(self.device)
        plan = CollatePlan(sel, node_off, edge_off, int(node_off[-1]), int(edge_off[-1]), int(sel.shape[0]), table)
        plan.__dict__["_store"] = self             # collate takes the plans of its own store only
        return plan

    # -------------------------------------------------------------------------------------------- collate
    def _layout(self):
        """(key of the batch dict, slot in a tuple or None, resident tensor, kind) of every copied tensor."""
        T = self.tensors
        if self.vector:
            feats = [("x", 0, T["x_s"], NODE_ROWS), ("x", 1, T["x_v"], NODE_ROWS),
                     ("eattr", 0, T["e_s"], EDGE_ROWS), ("eattr", 1, T["e_v"], EDGE_ROWS)]
        else:
            feats = [("x", None, T["x_s"], NODE_ROWS), ("eattr", None, T["e_s"], EDGE_ROWS)]
        return feats + [("ntypes", None, T["ntypes"], NODE_ROWS), ("etypes", None, T["etypes"], EDGE_ROWS)]

    def _checked(self, t, what, like, rows, lead=None):
        """`t` of an `out` dict against the resident tensor `like` ([rows, ...]; `lead`: edge_index, [2, rows])."""
        if not torch.is_tensor(t):
            raise ValueError(f"out[{what}] is not a tensor")
        if t.device != like.device:
            raise ValueError(f"out[{what}] is on {t.device}, the store is on {like.device}")
        if t.dtype != like.dtype:
            raise ValueError(f"out[{what}] is {t.dtype}, expected {like.dtype}")
        if lead is not None:
            if t.dim() != 2 or t.shape[0] != lead:
                raise ValueError(f"out[{what}] must be [{lead}, rows], got {tuple(t.shape)}")
            if t.shape[1] > 1 and t.stride(1) != 1:
                raise ValueError(f"out[{what}]: each of its {lead} rows must be contiguous")
            have = t.shape[1]
        else:
            if t.dim() != like.dim() or tuple(t.shape[1:]) != tuple(like.shape[1:]):
                raise ValueError(f"out[{what}] must be [rows{''.join(f', {s}' for s in like.shape[1:])}], got {tuple(t.shape)}")
            if not t.is_contiguous():
                raise ValueError(f"out[{what}] is not contiguous")
            have = t.shape[0]
        if have < rows:
            raise ValueError(f"out[{what}] has {have} rows, the batch needs {rows}")
        return t

    def collate(self, plan, out=None, max_blocks=0):
        """The batch of `plan` -> {"x", "edge_index", "ntypes", "etypes", "eattr", "batch", "ptr"}: what
        `davis_synth.to_torch(davis_synth.collate([...]))` returns, plus `ptr` (a slice of `plan.table`); `x` and `eattr`
        are tuples when the graphs carry vector features.  One launch on the current stream.

        Without `out` every tensor is a fresh allocation of exactly the batch's size.  With `out`, a dict of the same
        structure (no `ptr`) whose tensors have at least the batch's rows, the launch writes into them and views of the
        first N / E rows are returned; rows behind them are not touched.  `out["edge_index"]` is [2, rows >= E] with
        contiguous rows (a column slice of a larger allocation is fine; the returned view is then `[:, :E]` of it).
        ValueError, before the launch: a tensor on another device, of another dtype, with other trailing dimensions, not
        contiguous, or with too few rows.  `max_blocks` caps the grid (0: the default)."""
        if not isinstance(plan, CollatePlan):
            raise TypeError("collate takes a CollatePlan (ResidentGraphs.plan)")
        _lib._on_gpu(self.offsets, "ResidentGraphs.collate")
        if plan.__dict__.get("_store") is not self:    # another store's graphs have other sizes: the kernel would read astray
            raise ValueError("collate: the plan was not made by this store's plan()")
        N, E, B = plan.N, plan.E, plan.B
        layout, T = self._layout(), self.tensors
        if out is None:
            new = lambda like, rows: torch.empty((rows,) + tuple(like.shape[1:]), dtype=like.dtype, device=self.device)
            got = {(k, s): new(src, N if kind == NODE_ROWS else E) for k, s, src, kind in layout}
            ei = torch.empty((2, E), dtype=torch.int64, device=self.device)
            batch = torch.empty((N,), dtype=torch.int64, device=self.device)
        else:
            got = {}
            for k, s, src, kind in layout:
                if k not in out or (s is not None and (not isinstance(out[k], (tuple, list)) or len(out[k]) != 2)):
                    raise ValueError(f"out[{k!r}] is missing or not a pair of tensors")
                got[(k, s)] = self._checked(out[k] if s is None else out[k][s], k if s is None else f"{k}[{s}]", src,
                                            N if kind == NODE_ROWS else E)
            for k in ("edge_index", "batch"):
                if k not in out:
                    raise ValueError(f"out[{k!r}] is missing")
            ei = self._checked(out["edge_index"], "edge_index", T["edge_index"], E, lead=2)
            batch = self._checked(out["batch"], "batch", T["ntypes"], N)
        items = (CollateItem * MAX_ITEMS)()
        n = 0
        for k, s, src, kind in layout:
            dst = got[(k, s)]
            items[n] = CollateItem(dst.data_ptr(), src.data_ptr(), int(np.prod(src.shape[1:], dtype=np.int64)) * src.element_size(), kind)
            n += 1
        for row in range(2):
            items[n] = CollateItem(ei[row].data_ptr() if ei.shape[1] else 0, T["edge_index"][row].data_ptr() if E else 0, 8, ENDPOINTS)
            n += 1
        items[n] = CollateItem(batch.data_ptr(), 0, 8, BATCH)
        n += 1
        tab, off = plan.table, self.offsets
        base, step = tab.data_ptr(), 8
        G = len(self)
        with torch.cuda.device(self.device):
            _lib.check(lib().cgvp_collate_graphs(items, n, base, base + step * B, base + step * (2 * B + 1), off.data_ptr(),
                                                 off.data_ptr() + step * (G + 1), B, N, E, int(max_blocks), _stream()),
                       "cgvp_collate_graphs")
        view = lambda t, rows: t if t.shape[0] == rows else t[:rows]
        res = {}
        for k in ("x", "eattr"):
            res[k] = ((view(got[(k, 0)], N if k == "x" else E), view(got[(k, 1)], N if k == "x" else E)) if self.vector
                      else view(got[(k, None)], N if k == "x" else E))
        res["edge_index"] = ei if ei.shape[1] == E else ei[:, :E]
        res["ntypes"], res["etypes"] = view(got[("ntypes", None)], N), view(got[("etypes", None)], E)
        res["batch"], res["ptr"] = view(batch, N), plan.ptr
        return {k: res[k] for k in ("x", "edge_index", "ntypes", "etypes", "eattr", "batch", "ptr")}


# ------------------------------------------------------------------------------------------------ both sides and the pairs
class ResidentPairs:
    """A pair dataset over two stores: `proteins` and `molecules` (ResidentGraphs on one device), `pair_index` [K, 2] of
    (protein, molecule) indices (kept on the host) and the targets `y` [K, ...] (kept on the device)."""

    def __init__(self, proteins, molecules, pair_index, y):
        if proteins.device != molecules.device:
            raise ValueError("ResidentPairs: the two stores are on different devices")
        self.proteins, self.molecules, self.device = proteins, molecules, proteins.device
        pi = pair_index.detach().cpu().numpy() if torch.is_tensor(pair_index) else np.asarray(pair_index)
        if pi.size and pi.dtype.kind not in "iu":
            raise TypeError(f"pair_index must be integers, got {pi.dtype}")
        pi = pi.reshape(-1, 2).astype(np.int64)
        _index_array(pi[:, 0], len(proteins), "pair_index[:, 0]")
        _index_array(pi[:, 1], len(molecules), "pair_index[:, 1]")
        self.pair_index = pi
        y = y if torch.is_tensor(y) else torch.from_numpy(np.ascontiguousarray(y))
        if y.shape[0] != pi.shape[0]:
            raise ValueError(f"y has {y.shape[0]} rows for {pi.shape[0]} pairs")
        self.y = y.to(self.device)

    def __len__(self):
        return int(self.pair_index.shape[0])

    def batch(self, pair_ids):
        """The collated batch of those pairs, one graph per pair on each side, as the reference's collator yields it
        -> (pdata, mdata, y_batch).  Two collate launches and one index_select of `y`."""
        ids = _index_array(pair_ids, len(self), "pair ids")
        pplan, mplan = self.proteins.plan(self.pair_index[ids, 0]), self.molecules.plan(self.pair_index[ids, 1])
        rows = torch.from_numpy(ids).to(self.device)
        return self.proteins.collate(pplan), self.molecules.collate(mplan), self.y.index_select(0, rows)

    def block(self, protein_ids, molecule_ids, pairs=None):
        """Each unique graph once -> (pdata, mdata, plan): the batches of `protein_ids` and `molecule_ids` and the
        `gvp_hip.pair_training.PairTrainPlan` of `pairs` ([K, 2] indices INTO the two id lists; None = the full cross
        product, protein-major), planned from the host lengths.  Goes straight into `model.forward_pairs(pdata, mdata,
        plan)` with no host read (`model.score_pairs(pdata, mdata, pairs)` takes the pair list itself)."""
        from .pair_training import plan_pair_training
        pplan, mplan = self.proteins.plan(protein_ids), self.molecules.plan(molecule_ids)
        plan = plan_pair_training(np.diff(pplan.node_off), np.diff(mplan.node_off), pairs)
        return self.proteins.collate(pplan), self.molecules.collate(mplan), plan

    def batches(self, max_num=None, batch_size=None, shuffle=True, generator=None, max_bsize=None):
        """One epoch as lists of pair ids; every pair appears once.  Either `batch_size` pairs a batch, or an edge
        budget: pairs are taken in order while the batch's protein plus molecule edges stay within `max_num`; a pair that
        would exceed it starts the next batch, and a single pair larger than the budget is a batch of its own.
        `max_bsize` also closes a batch at that many pairs.  Host only; `shuffle` draws the order from `generator` (a
        torch.Generator)."""
        if (max_num is None) == (batch_size is None):
            raise ValueError("batches: give either max_num (an edge budget) or batch_size")
        limit = batch_size if batch_size is not None else max_num
        if int(limit) <= 0 or (max_bsize is not None and int(max_bsize) <= 0):
            raise ValueError("batches: max_num / batch_size / max_bsize must be positive")
        K = len(self)
        order = torch.randperm(K, generator=generator).tolist() if shuffle else list(range(K))
        if batch_size is not None:
            size = int(batch_size) if max_bsize is None else min(int(batch_size), int(max_bsize))
            for at in range(0, K, size):
                yield order[at:at + size]
            return
        cost = (np.diff(self.proteins.edge_off)[self.pair_index[:, 0]] + np.diff(self.molecules.edge_off)[self.pair_index[:, 1]])
        current, used = [], 0
        for i in order:
            c = int(cost[i])
            if current and (used + c > max_num or (max_bsize is not None and len(current) >= max_bsize)):
                yield current
                current, used = [], 0
            current.append(i)
            used += c
        if current:
            yield current
