"""Shape-bucketed HIP-graph replay of an encoder training step for loops that feed a DIFFERENT batch every step.

The reference's loop (train_model.py:548-587) draws a new batch -- new N, E, edge_index -- every step.  Launched
eagerly, a step of both encoders costs ~0.6 ms of host time (PyTorch's autograd engine alone spends ~0.3 ms on the 74
parameter leaves) for ~0.25 ms of device work.  A captured step replays in one host call, but a HIP graph freezes its
shapes.  `GraphedEncoderStep` keeps one captured step per SHAPE BUCKET:

  * sizes (residues, protein edges, atoms, drug edges) are rounded up to the next multiple of 1/8 of their power of two
    (at most 12.5 % padding), a bucket = the four rounded sizes;
  * each bucket owns static input buffers; a step copies the batch into them with ONE launch (cgvp_stage_buffers) and
    replays the bucket's graph;
  * padding is inert by construction: padded residues / atoms are isolated nodes (their upstream gradient rows are zero,
    and every backward stage is linear in its upstream gradient), padded edges carry endpoint -1 and are dropped by the
    CSR build inside the captured step (tests/test_hip_random_graphs.py covers out-of-range endpoints); dropout is keyed
    by (seed, offset, layer, row, channel), so the real rows draw the same factors as in an unpadded eager step.

The outputs (embeddings of the real rows, every weight gradient) are the graph's static tensors: consume them (optimizer
step, all-reduce) before the next `run` of the same bucket.  The inputs are staged copies, so a captured step returns no
input gradients (d x, d eattr: the eager nn.Module path does).  Opt-in: the nn.Module API is untouched.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import os

import torch

from . import _lib, ops


def mode_key(key, sdt):
    """Dictionary key of a bucket: its sizes, the storage dtype and the deterministic mode of the backward passes
    (torch.use_deterministic_algorithms / CGVP_DETERMINISTIC), so a graph captured in one mode is never replayed in the
    other."""
    return (key, sdt, _lib.deterministic_mode())


def bucket_size(n):
    """n rounded up to a multiple of 2^(floor(log2 n) - 3): at most 12.5 % larger, 8 buckets per octave."""
    n = int(n)
    if n <= 64:
        return 64
    q = 1 << max(n.bit_length() - 4, 0)
    return (n + q - 1) // q * q


class _Bucket:
    """Static inputs of one shape bucket -- the protein and drug dicts padded to (N, E) and (Na, Ea) rows, edge_index
    filled with -1 -- and its captured step (`graph`, outputs `out`, replay count `steps`)."""

    def __init__(self, dev, N, E, Na, Ea, pdata, mdata, sdt):
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
        ni = pdata["x"][0].shape[1], pdata["x"][1].shape[1], pdata["eattr"][0].shape[1], pdata["eattr"][1].shape[1]
        self.p = dict(x=(z(N, ni[0], dt=sdt), z(N, ni[1], 3, dt=sdt)), edge_index=torch.full((2, E), -1, dtype=torch.int64, device=dev),
                      ntypes=z(N, dt=torch.int64), etypes=z(E, dt=torch.int64),
                      eattr=(z(E, ni[2], dt=sdt), z(E, ni[3], 3, dt=sdt)))
        self.m = dict(x=z(Na, mdata["x"].shape[1]), edge_index=torch.full((2, Ea), -1, dtype=torch.int64, device=dev),
                      ntypes=z(Na, dt=torch.int64), etypes=z(Ea, dt=torch.int64), eattr=z(Ea, mdata["eattr"].shape[1]))
        self.graph, self.out, self.steps = None, None, 0


# The ten feature tensors of a batch: (dict, field, index in a tuple field or None, which of the bucket's four sizes
# (residues, protein edges, atoms, drug edges) is its row capacity, its name in messages)
_FEATURES = tuple((side, field, i, size, f"{'pdata' if side == 'p' else 'mdata'}[{field!r}]" + ("" if i is None else f"[{i}]"))
                  for side, field, i, size in (("p", "x", 0, 0), ("p", "x", 1, 0), ("p", "ntypes", None, 0), ("p", "etypes", None, 1),
                                               ("p", "eattr", 0, 1), ("p", "eattr", 1, 1), ("m", "x", None, 2),
                                               ("m", "ntypes", None, 2), ("m", "etypes", None, 3), ("m", "eattr", None, 3)))


def _field(d, field, i):
    return d[field] if i is None else d[field][i]


class _BucketedGraphs:
    """Capture-or-replay core of both steps.  A subclass supplies `_new_bucket`, `_pairs` (its staging pairs after the ten
    feature tensors), `_exact` (name, source and required shape of each of those), `_step` and `_capture_mode` (the
    context of a bucket's creation, warm-up and capture)."""

    def _check_batch(self, key, b, pdata, mdata, *extra):
        """The staging launch gets raw addresses and byte counts: a source on the host or on another GPU would be a device
        read of a foreign address, a source larger than its static buffer a write past its end.  So everything `_stage`
        will be given is checked here, on the host, before a bucket is created, staged or captured: ValueError.  `b` is
        the batch's bucket, or None when this batch is about to create it (its trailing dimensions are then the
        batch's own)."""
        dev = self.device

        def foreign(name, t):
            if not isinstance(t, torch.Tensor):
                return ValueError(f"{name}: expected a tensor, got {type(t).__name__}")
            return ValueError(f"{name} is on {t.device}, the captured step's buffers are on {dev}: move the batch to the "
                              "model's device first (.to(device, non_blocking=True))")
        for side, field, i, size, name in _FEATURES:
            src = _field(pdata if side == "p" else mdata, field, i)
            if not isinstance(src, torch.Tensor) or src.device != dev:
                raise foreign(name, src)
            if src.dim() < 1 or src.shape[0] > key[size]:
                raise ValueError(f"{name} has shape {tuple(src.shape)}: more than the {key[size]} rows of the batch's bucket")
            if b is not None and src.shape[1:] != _field(getattr(b, side), field, i).shape[1:]:
                raise ValueError(f"{name} has shape {tuple(src.shape)}, the captured step was built for rows of shape "
                                 f"{tuple(_field(getattr(b, side), field, i).shape[1:])}")
        for name, src, size in (("pdata['edge_index']", pdata["edge_index"], 1), ("mdata['edge_index']", mdata["edge_index"], 3)):
            if not isinstance(src, torch.Tensor) or src.device != dev:
                raise foreign(name, src)
            if src.dim() != 2 or src.shape[0] != 2 or src.shape[1] > key[size]:
                raise ValueError(f"{name} has shape {tuple(src.shape)}: expected [2, E] with E <= {key[size]}, the batch's bucket")
        for name, src, shape in self._exact(key, b, pdata, mdata, *extra):
            if not isinstance(src, torch.Tensor) or src.device != dev:
                raise foreign(name, src)
            if src.numel() != math.prod(shape) or (src.dim() and src.shape[0] != shape[0]):
                raise ValueError(f"{name} has shape {tuple(src.shape)}, the captured step expects {tuple(shape)}")

    def _stage(self, b, pdata, mdata, extra):
        """ONE launch copies the batch into b's static buffers; returns the sources that must outlive the copy.  (The
        sources have passed `_check_batch`.)"""
        pairs = [(_field(getattr(b, side), field, i), _field(pdata if side == "p" else mdata, field, i))
                 for side, field, i, _, _ in _FEATURES] + extra
        items = (_lib.StageItem * _lib.MAX_STAGE)()
        keep, k = [], 0
        for dst, src in pairs:
            if src.dtype != dst.dtype or not src.is_contiguous():
                src = src.to(dst.dtype).contiguous()
                keep.append(src)
            items[k] = _lib.StageItem(dst.data_ptr(), src.data_ptr() if src.numel() else 0, src.numel() * src.element_size(),
                                      dst.numel() * dst.element_size(), 0)
            k += 1
        for dst, src in ((b.p["edge_index"], pdata["edge_index"]), (b.m["edge_index"], mdata["edge_index"])):
            src = src.contiguous()
            keep.append(src)
            E, Ecap = src.shape[1], dst.shape[1]
            for row in range(2):                                      # each row of [2, E] lands in its row of [2, Ecap], tail = -1
                items[k] = _lib.StageItem(dst[row].data_ptr(), src[row].data_ptr() if E else 0, E * 8, Ecap * 8, 0xFFFFFFFF)
                k += 1
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().cgvp_stage_buffers(items, k, C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                       "cgvp_stage_buffers")
        return keep

    def _replay(self, key, pdata, mdata, *extra):
        """Stage the batch and replay its bucket's graph (captured at the first visit); returns the bucket."""
        sdt = torch.bfloat16 if pdata["x"][0].dtype == torch.bfloat16 else torch.float32
        b = self.buckets.get(mode_key(key, sdt))
        self._check_batch(key, b, pdata, mdata, *extra)
        if b is not None and b.graph is not None:
            # steady state: stage + replay on the caller's stream (a graph replays on whatever stream it is launched on;
            # no cross-stream dependency, which costs ~10 us of idle device per hop)
            keep = self._stage(b, pdata, mdata, self._pairs(b, pdata, mdata, *extra))
            b.graph.replay()
            b.steps += 1
            del keep                                         # same stream: the allocator's stream ordering covers the reuse
            return b
        caller = torch.cuda.current_stream()
        self.stream.wait_stream(caller)
        with torch.cuda.stream(self.stream), self._capture_mode():
            if b is None:
                b = self.buckets[mode_key(key, sdt)] = self._new_bucket(key, sdt, pdata, mdata, *extra)
            keep = self._stage(b, pdata, mdata, self._pairs(b, pdata, mdata, *extra))
            old = ops.CSR_CACHE_ENABLED
            ops.CSR_CACHE_ENABLED = False                    # the captured step rebuilds its CSR tables from the staged edge_index
            try:
                for _ in range(2):                           # warm-up on the capture stream (generator state, counters exist)
                    self._step(b)
                torch.cuda.current_stream().synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=self.stream, pool=self.pool):
                    b.out = self._step(b)
                if self.pool is None:
                    self.pool = g.pool()                     # every bucket's graph shares one memory pool
                b.graph = g
            finally:
                ops.CSR_CACHE_ENABLED = old
            b.graph.replay()
            b.steps += 1
        caller.wait_stream(self.stream)
        for t in keep:
            t.record_stream(self.stream)
        return b


class GraphedEncoderStep(_BucketedGraphs):
    """step = forward of both encoders + backward with every weight gradient, protein chain on the launch stream, drug
    chain on a side stream (what bench.py times).  `run(pdata, mdata, g_res, g_atm)` -> (residues [N, 64],
    atoms [Na, 64], protein grads, drug grads) -- views of static tensors of the batch's bucket."""

    def __init__(self, protein_gnn, molecule_gnn, train=True, quantum=bucket_size):
        self.prot, self.mol = protein_gnn, molecule_gnn
        self.pp = [p for p in protein_gnn.parameters() if p.numel()]
        self.mp = [p for p in molecule_gnn.parameters() if p.numel()]
        self.device = self.pp[0].device
        self.out_res = protein_gnn.out_channels[0] if isinstance(protein_gnn.out_channels, (tuple, list)) else protein_gnn.out_channels
        self.out_atm = molecule_gnn.out_channels
        self.train, self.quantum = train, quantum
        self.buckets = {}
        self.stream = torch.cuda.Stream(device=self.device)          # capture + replay stream (its CSR counters persist)
        self.side = torch.cuda.Stream(device=self.device)
        self.pool = None

    def _new_bucket(self, key, sdt, pdata, mdata, g_res, g_atm):
        N, E, Na, Ea = key
        b = _Bucket(self.device, N, E, Na, Ea, pdata, mdata, sdt)
        b.g_res = torch.zeros(N, self.out_res, dtype=sdt, device=self.device)
        b.g_atm = torch.zeros(Na, self.out_atm, dtype=torch.float32, device=self.device)
        return b

    def _pairs(self, b, pdata, mdata, g_res, g_atm):
        return [(b.g_res, g_res), (b.g_atm, g_atm)] if self.train else []

    def _exact(self, key, b, pdata, mdata, g_res, g_atm):
        if not self.train:
            return []
        return [("g_res", g_res, (pdata["x"][0].shape[0], self.out_res)), ("g_atm", g_atm, (mdata["x"].shape[0], self.out_atm))]

    def _capture_mode(self):
        return torch.set_grad_enabled(self.train)

    def _step(self, b):
        main_s = torch.cuda.current_stream()
        self.side.wait_stream(main_s)
        res = self.prot(**b.p)
        with torch.cuda.stream(self.side):
            atm = self.mol(**b.m)
        if not self.train:
            main_s.wait_stream(self.side)
            return res, atm, (), ()
        gp = torch.autograd.grad([res], self.pp, [b.g_res])
        with torch.cuda.stream(self.side):
            gd = torch.autograd.grad([atm], self.mp, [b.g_atm])
        main_s.wait_stream(self.side)
        return res, atm, gp, gd

    def run(self, pdata, mdata, g_res=None, g_atm=None):
        N, E = pdata["x"][0].shape[0], pdata["edge_index"].shape[1]
        Na, Ea = mdata["x"].shape[0], mdata["edge_index"].shape[1]
        key = (self.quantum(N), self.quantum(E), self.quantum(Na), self.quantum(Ea))
        res, atm, gp, gd = self._replay(key, pdata, mdata, g_res, g_atm).out
        return res[:N], atm[:Na], gp, gd


def _check_no_foreign_graph(params):
    """Observed on this ROCm / PyTorch build (tools/debug_graphed.py, 15 runs): capturing the WHOLE-MODEL backward while an
    autograd graph of an earlier eager step on another stream is still alive (its `pred` / `loss` held somewhere) ends in
    a segmentation fault inside hipStreamEndCapture, every time; with that graph dropped, or no eager step before, never.
    What such a graph keeps alive are the leaves' AccumulateGrad nodes, which remember the stream they were created under
    (csrc/torch_bridge.cpp, stale_grad_accumulators); the engine synchronises gradient hand-offs with that stream.  The
    encoder-only captures of GraphedEncoderStep never showed it.  Refuse with a message instead of crashing."""
    br = _lib.bridge()                     # (GraphedTrainStep refuses to exist without it)
    n = int(br.stale_grad_accumulators(list(params)))
    if n:
        raise RuntimeError(
            f"{n} parameters are still referenced by an autograd graph that was built on another stream (an output or loss "
            "of an earlier eager step is alive): capturing a backward pass now would pull that stream into the capture. "
            "Drop those tensors first (`del loss, pred`), or run the eager step after the captured one.")


class GraphedTrainStep(_BucketedGraphs):
    """The WHOLE JointGNN training step -- forward of both encoders and the head, loss, backward with all 764k gradients --
    replayed from shape-bucketed HIP graphs, for the loop of train_model.py:548-587 that feeds a different batch every step:

        step = GraphedTrainStep(model, torch.nn.functional.mse_loss)        # optional: scaler=GradScaler, autocast=dtype
        for pdata, mdata, y in loader:            # the dicts carry 'ptr' (PyG Batch objects do)
            loss, pred = step.run(pdata, mdata, y)                           # p.grad of every parameter is set
            optimizer.step()

    `run` REPLACES every trainable parameter's .grad by this step's gradient: nothing is accumulated into a gradient that
    is already there (unlike `loss.backward()`; no `zero_grad()` is needed between steps), and a parameter the step does
    not use gets .grad = None, so a stale gradient of an earlier eager step is never applied again.

    With `optimizer=` a gvp_hip.optim.FusedAdam over `model.parameters()`, the update (unscale, clip, Adam, and the
    scaler's update when `scaler` is given: train_model.py:578-587) is part of the captured step: `run` still returns
    (loss, pred) and publishes p.grad, and the caller calls neither `optimizer.step()` nor `scaler.update()`.  The optimizer
    state is shared by all buckets, only the gradient addresses are per bucket; the warm-up passes of a capture run the
    update dry.  The learning rate is read from `param_groups[0]["lr"]` at every `run`; the other hyperparameters are those
    of the construction.

    Row-wise heads only.  The step runs the head on B + 1 rows (below), and a capture runs it three times.  So a model
    whose head mixes rows is refused with a RuntimeError, at construction and at `run`, before any bucket exists:
    BatchNorm on batch statistics (out_lin_norm_type="batch" in training mode; in eval mode it normalises by the running
    statistics, row by row, and is captured like any other head), and `enable_pair_parallel()` with or without
    `optimizer=` (the gather would carry the padding pair, and the all-reduce sits between backward and update).

    The batch must be on the model's device: `run` raises ValueError for a tensor that is on the host or another GPU
    (`y` straight from a loader), for `ptr` or `target` that do not hold B + 1 / B entries, and for a feature tensor whose
    trailing dimensions differ from the bucket's -- before anything is staged.

    With `meter=` a gvp_hip.metrics.RegressionMeter on the model's device, every `run` appends its B predictions and
    targets to the meter inside the captured step (the warm-up passes of a capture add nothing, the padding pair is never
    recorded): `meter.compute()` at the end of an epoch replaces the reference's `.item()` per step (train_model.py:609-636).

    One launch stages the batch into the bucket's padded static buffers, one replay runs the step.  Padding: padded
    residues / atoms are isolated nodes that belong to an extra (B+1)-th pair whose prediction the loss never reads, so
    every real pair's numbers and every gradient equal those of the eager step on the unpadded batch (padded rows have
    zero upstream gradient; tests/test_hip_models.py::test_graphed_train_step_equals_eager).  The gradients are the graph's
    static tensors: consume them (optimizer step) before the next `run` of the same bucket."""

    def __init__(self, model, loss_fn, scaler=None, autocast=None, quantum=bucket_size, optimizer=None, meter=None):
        if _lib.bridge() is None:
            # the capture-safety check below (_check_no_foreign_graph) lives in the C++ bridge: without it a forgotten eager
            # `loss` / `pred` turns the next capture into a segmentation fault inside hipStreamEndCapture
            raise RuntimeError("GraphedTrainStep needs the C++ eager bridge (lib/caster_gvp_torch.so, built by "
                               "__graft_entry__.build(); CGVP_BRIDGE=0 / CGVP_LIB_PATH turn it off)")
        self.model, self.loss_fn, self.scaler, self.autocast, self.quantum = model, loss_fn, scaler, autocast, quantum
        self.params = [p for p in model.parameters() if p.numel() and p.requires_grad]
        self.device = self.params[0].device
        self.buckets = {}
        self.stream = torch.cuda.Stream(device=self.device)          # capture + replay stream
        self.pool = None
        self.optimizer = optimizer
        if optimizer is not None:
            from .optim import FusedAdam
            if not isinstance(optimizer, FusedAdam):
                raise TypeError(f"GraphedTrainStep(optimizer=...) captures a gvp_hip.optim.FusedAdam, not a {type(optimizer).__name__}: "
                                "step any other optimizer after `run`, from the published p.grad")
            slot = {id(p): i for i, p in enumerate(optimizer.param_groups[0]["params"])}
            if any(id(p) not in slot for p in self.params):
                raise ValueError("GraphedTrainStep(optimizer=...): the optimizer must hold every trainable parameter of the model "
                                 "(FusedAdam(model.parameters(), ...))")
            self._opt_slots, self._opt_key = [slot[id(p)] for p in self.params], optimizer.hyper_key()
        self.meter = meter
        if meter is not None:
            from .metrics import RegressionMeter
            if not isinstance(meter, RegressionMeter):
                raise TypeError(f"GraphedTrainStep(meter=...) captures a gvp_hip.metrics.RegressionMeter, not a {type(meter).__name__}")
            if meter.device != self.device:
                raise ValueError(f"GraphedTrainStep(meter=...): the meter lives on {meter.device}, the model on {self.device}")
        self._batch_norms = [(n, m) for n, m in model.named_modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
        self._check_row_wise()

    def _check_row_wise(self):
        """The captured step runs the head on B + 1 rows (the padding pair) and twice more to warm up: refuse what is not
        row-wise.  At construction and at every `run` (a mode can change in between), before a bucket exists."""
        if getattr(self.model, "_pair_parallel", False):
            raise RuntimeError("GraphedTrainStep cannot be combined with enable_pair_parallel(): the captured step carries a "
                               "padding pair that the gather would send to every rank as one of the local pairs"
                               + ("" if self.optimizer is None else ", and the gradient all-reduce belongs between the "
                                  "backward pass and the captured update"))
        for name, mod in self._batch_norms:
            if mod.training or mod.running_mean is None:
                raise RuntimeError(f"GraphedTrainStep cannot run BatchNorm on batch statistics ({name or 'the model'}, "
                                   "out_lin_norm_type='batch' in training mode): the padding pair of the captured step would "
                                   "enter the mean and variance of every real pair, and the warm-up passes of a capture would "
                                   "advance the running statistics.  Use the eager step, out_lin_norm_type='layer', or "
                                   "model.eval() (running statistics are row-wise)")

    def _new_bucket(self, key, sdt, pdata, mdata, target):
        N, E, Na, Ea, B = key
        dev = self.device
        b = _Bucket(dev, N, E, Na, Ea, pdata, mdata, sdt)
        # B real pairs + ONE padding pair that owns every padded residue / atom (never empty: the sizes are rounded up from
        # n + 1), so that the head's per-pair pooling and attention see B + 1 well-formed pairs and the loss reads the first B
        b.p["ptr"] = torch.full((B + 2,), N, dtype=torch.int64, device=dev)
        b.m["ptr"] = torch.full((B + 2,), Na, dtype=torch.int64, device=dev)
        b.target = torch.zeros((B,) + tuple(target.shape[1:]), dtype=target.dtype, device=dev)
        b.rows_p, b.rows_m = torch.arange(N, device=dev), torch.arange(Na, device=dev)
        return b

    def _pairs(self, b, pdata, mdata, target):
        return [(b.target, target), (b.p["ptr"][:-1], pdata["ptr"]), (b.m["ptr"][:-1], mdata["ptr"])]   # (the last offset stays the padded size)

    def _exact(self, key, b, pdata, mdata, target):
        B = key[4]
        rest = tuple(b.target.shape[1:]) if b is not None else tuple(target.shape[1:]) if isinstance(target, torch.Tensor) else ()
        return [("target", target, (B,) + rest), ("pdata['ptr']", pdata["ptr"], (B + 1,)), ("mdata['ptr']", mdata["ptr"], (B + 1,))]

    @contextlib.contextmanager
    def _capture_mode(self):
        was_training = self.model.training
        with torch.enable_grad():
            _check_no_foreign_graph(self.params)     # before the bucket is created or staged
            yield
        self.model.train(was_training)

    def _step(self, b):
        B = len(b.target)                               # real pairs
        ctx = torch.autocast("cuda", dtype=self.autocast) if self.autocast is not None else contextlib.nullcontext()
        # pair index of every row from the staged offsets (no host sync): rows behind the last real one -> the padding pair B
        pd = dict(b.p, batch=self._pair_of_rows(b.p["ptr"], b.rows_p))
        md = dict(b.m, batch=self._pair_of_rows(b.m["ptr"], b.rows_m))
        aw = getattr(self.model, "attention_weights", None)
        if aw is not None:
            self.model.attention_weights = "never"      # (the padded weight tensors need a host-side maximum: not capturable)
        try:
            with ctx:
                pred, _ = self.model(pd, md)
                loss = self.loss_fn(pred[:B], b.target)
        finally:
            if aw is not None:
                self.model.attention_weights = aw
        out = self.scaler.scale(loss) if self.scaler is not None else loss
        grads = torch.autograd.grad(out, self.params, allow_unused=True)
        if self.optimizer is not None:
            # the update on the captured gradients; the two warm-up passes of a capture (_replay) only compute the norm,
            # otherwise the first batch of every bucket would be applied three times
            full = [None] * len(self.optimizer.param_groups[0]["params"])
            for i, g in zip(self._opt_slots, grads):
                full[i] = g
            self.optimizer.apply(full, scaler=self.scaler, dry=not torch.cuda.is_current_stream_capturing())
        if self.meter is not None:
            # the B real predictions and targets of this step (never the padding pair); dry in the warm-up passes, as above
            self.meter.update(pred[:B].detach(), b.target, dry=not torch.cuda.is_current_stream_capturing())
        return loss.detach(), pred[:B].detach(), grads

    @staticmethod
    def _pair_of_rows(ptr, rows):
        """pair index of every row = number of pair END offsets <= row (plain compare + sum: capturable, no host sync)"""
        if os.environ.get("CGVP_GRAPHED_BATCH") == "searchsorted":
            return torch.searchsorted(ptr[1:].contiguous(), rows, right=True)
        return (rows.unsqueeze(1) >= ptr[1:].unsqueeze(0)).sum(dim=1)

    def _publish(self, b):
        loss, pred, grads = b.out
        for p, g in zip(self.params, grads):        # (g None: a parameter the step does not use loses a stale gradient)
            if p.grad is not g:
                p.grad = g
        return loss, pred

    def run(self, pdata, mdata, target):
        if "ptr" not in pdata or "ptr" not in mdata:
            raise ValueError("GraphedTrainStep needs the graph offsets 'ptr' in both dicts (PyG Batch objects carry them)")
        N, E = pdata["x"][0].shape[0], pdata["edge_index"].shape[1]
        Na, Ea = mdata["x"].shape[0], mdata["edge_index"].shape[1]
        B = int(pdata["ptr"].numel()) - 1
        key = (self.quantum(N + 1), self.quantum(E), self.quantum(Na + 1), self.quantum(Ea), B)
        self._check_row_wise()
        if self.optimizer is not None:
            if self.optimizer.hyper_key() != self._opt_key:
                raise RuntimeError("the optimizer's betas / eps / weight decay / max_grad_norm changed since GraphedTrainStep was "
                                   "built: captured steps keep the old values (only the learning rate is read at run time)")
            self.optimizer.sync_lr()
        return self._publish(self._replay(key, pdata, mdata, target))
