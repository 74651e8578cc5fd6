"""Evaluation metrics on the device: `regression_metrics`, `concordance_index`, `RegressionMeter`.

ctypes binding of include/caster_gvp_metrics.h (csrc/metrics_kernels.hip), a header and a version of its own beside the
main C ABI: the entry points live in the same libcaster_gvp.so, the signature table below is this module's.
`regression_metrics` is the reference's test evaluation (train_model.py:759-793: MSE, RMSE, MAE, Pearson and the
concordance index, the last one a Python double loop over all pairs) as one call and one host read.
`RegressionMeter.update` appends a batch to device buffers without a host synchronisation -- it can be captured
(gvp_hip.graphed.GraphedTrainStep(meter=...)) -- so that a training or validation loop needs no `.item()` per step
(train_model.py:609-631, 645-674): `compute()["mse"]` over an epoch is its batch-size-weighted mean of the losses.
"""
from __future__ import annotations

import ctypes as C
import functools
import math

import torch

from . import _lib
from ._lib import _on_gpu, _ptr, _stream

METRICS_VERSION = 1      # CGVP_METRICS_VERSION
TILE = 256               # CGVP_METRICS_TILE
CHUNK = 1024             # CGVP_METRICS_CHUNK
MAX_ROWS = 1 << 26       # CGVP_METRICS_MAX_ROWS

_P, _I64, _I32 = C.c_void_p, C.c_int64, C.c_int32
_SIGNATURES = {
    "cgvp_metrics_version": (C.c_int, []),
    "cgvp_metrics_reset": (C.c_int, [_P, _P]),
    "cgvp_metrics_append": (C.c_int, [_P, _P, _I64, _P, _P, _I64, _P, _I32, _P]),
    "cgvp_metrics_workspace_bytes": (C.c_int64, [_I64]),
    "cgvp_metrics_compute": (C.c_int, [_P, _P, _P, _I64, _P, _P, _P, _I64, _P]),
}


def exported_symbols():
    """Names include/caster_gvp_metrics.h declares."""
    return tuple(_SIGNATURES)


@functools.lru_cache(maxsize=None)
def lib():
    """libcaster_gvp.so (the handle of `_lib.lib()`) with the metrics entry points typed (once)."""
    return _lib.bind(_lib.lib(), _SIGNATURES, "cgvp_metrics_version", METRICS_VERSION, "metrics version")


def workspace_bytes(max_rows):
    """Bytes of workspace for one compute over at most `max_rows` rows (cgvp_metrics_workspace_bytes)."""
    n = int(lib().cgvp_metrics_workspace_bytes(int(max_rows)))
    if n < 0:
        raise ValueError(f"cgvp_metrics_workspace_bytes: bad argument (code {n}); at most {MAX_ROWS} rows")
    return n


def _rows(t, name):
    """`t` as a flat contiguous float32 tensor (bf16 / fp16 / fp64 are cast by torch)."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name}: expected a tensor")
    _on_gpu(t, name)
    if not t.dtype.is_floating_point:
        raise ValueError(f"{name}: expected a floating-point tensor, got dtype {t.dtype}")
    return t.detach().reshape(-1).to(torch.float32).contiguous()


def _pair(pred, target):
    p, t = _rows(pred, "pred"), _rows(target, "target")
    if p.numel() != t.numel():
        raise ValueError(f"pred has {p.numel()} values, target {t.numel()}")
    if p.device != t.device:
        raise ValueError(f"pred is on {p.device}, target on {t.device}")
    return p, t


def _result(words):
    """The dict of a compute from its 10 host words: int64 [4] counts, then the bits of double [6] values."""
    n, concordant, tied, comparable = (int(x) for x in words[:4])
    mse, mae, pearson, ci = (float(x) for x in words[4:8].view(torch.float64))
    return {"n": n, "mse": mse, "rmse": math.sqrt(mse) if mse >= 0.0 else float("nan"), "mae": mae, "pearson": pearson,
            "ci": ci, "concordant": concordant, "tied_pred": tied, "comparable": comparable}


def regression_metrics(pred, target):
    """MSE, RMSE, MAE, Pearson correlation and concordance index of `pred` against `target`: CUDA tensors of equal
    numel and any shape (float32 is used as it is, other floating types are cast by torch) ->

        {"n", "mse", "rmse", "mae", "pearson", "ci", "concordant", "tied_pred", "comparable"}

    The moments are accumulated in float64; the concordance index is (concordant + tied_pred / 2) / comparable over all
    pairs of rows, counted exactly (include/caster_gvp_metrics.h has the definitions, the treatment of NaN and of
    n == 0 included).  One compute call and ONE host read."""
    p, t = _pair(pred, target)
    n = p.numel()
    L, dev = lib(), p.device
    out = torch.empty(10, dtype=torch.int64, device=dev)
    ws = torch.empty(workspace_bytes(n) // 8, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        rc = L.cgvp_metrics_compute(_ptr(p), _ptr(t), None, n, _ptr(out[:4]), _ptr(out[4:]), _ptr(ws), ws.numel() * 8,
                                    _stream())
    _lib.check(rc, "cgvp_metrics_compute")
    return _result(out.cpu())


def concordance_index(pred, target):
    """The concordance index alone (`regression_metrics(pred, target)["ci"]`)."""
    return regression_metrics(pred, target)["ci"]


class RegressionMeter:
    """Predictions and targets of a whole epoch (or test split) on the device, and their metrics at the end:

        meter = RegressionMeter(len(dataset), device, transform=dataset.unscale_target)
        for batch in loader:
            ...
            meter.update(pred, target)        # no host synchronisation
        stats = meter.compute()               # one host read: the dict of `regression_metrics` + "dropped"
        meter.reset()

    `update` applies `transform` (any torch function of one tensor; un-scaling is not always affine, so it stays in
    torch) to both tensors, then appends them behind a cursor that lives in device memory: it allocates nothing of its
    own, reads nothing back and can be captured.  `dry=True` launches and writes nothing (the warm-up passes of a
    capture).  Rows beyond `capacity` are not stored but counted, and `compute` refuses to report on a truncated epoch
    unless told to.  Updates must be ordered by their stream (one workgroup, no atomics)."""

    def __init__(self, capacity, device, transform=None):
        capacity = int(capacity)
        if not 0 <= capacity <= MAX_ROWS:
            raise ValueError(f"RegressionMeter: capacity must lie in [0, {MAX_ROWS}], got {capacity}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"RegressionMeter: caster-dta_amd runs on MI355X only (got device {self.device}); "
                               "there is no CPU path")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.capacity, self.transform = capacity, transform
        self._lib = lib()
        self.pred = torch.zeros(capacity, dtype=torch.float32, device=self.device)
        self.target = torch.zeros(capacity, dtype=torch.float32, device=self.device)
        # [rows stored, rows dropped | n, concordant, tied_pred, comparable | the bits of six doubles]: one host read
        self._words = torch.zeros(12, dtype=torch.int64, device=self.device)
        self.state = self._words[:2]
        self._workspace = torch.empty(workspace_bytes(capacity) // 8, dtype=torch.int64, device=self.device)

    def update(self, pred, target, dry=False):
        """Append a batch (any shape, equal numel).  No host synchronisation; capturable."""
        if self.transform is not None:
            pred, target = self.transform(pred), self.transform(target)
        p, t = _pair(pred, target)
        if p.device != self.device:
            raise ValueError(f"RegressionMeter: the batch is on {p.device}, the meter on {self.device}")
        with torch.cuda.device(self.device):
            rc = self._lib.cgvp_metrics_append(_ptr(p), _ptr(t), p.numel(), _ptr(self.pred), _ptr(self.target),
                                               self.capacity, _ptr(self.state), 1 if dry else 0, _stream())
        _lib.check(rc, "cgvp_metrics_append")

    def reset(self):
        """Forget every row (the buffers keep their bytes, the count returns to 0).  No host synchronisation."""
        with torch.cuda.device(self.device):
            rc = self._lib.cgvp_metrics_reset(_ptr(self.state), _stream())
        _lib.check(rc, "cgvp_metrics_reset")

    def compute(self, allow_dropped=False):
        """The metrics of the rows stored so far (`regression_metrics`' dict and "dropped"): one compute call that
        follows the device-side count, and ONE host read."""
        w = self._words
        with torch.cuda.device(self.device):
            rc = self._lib.cgvp_metrics_compute(_ptr(self.pred), _ptr(self.target), _ptr(self.state), self.capacity,
                                                _ptr(w[2:6]), _ptr(w[6:]), _ptr(self._workspace),
                                                self._workspace.numel() * 8, _stream())
        _lib.check(rc, "cgvp_metrics_compute")
        host = w.cpu()
        dropped = int(host[1])
        if dropped and not allow_dropped:
            raise RuntimeError(f"RegressionMeter: {dropped} rows did not fit into the capacity of {self.capacity} rows and "
                               "were dropped; size the meter for the epoch, or pass allow_dropped=True for the metrics of "
                               "the rows that were stored")
        out = _result(host[2:])
        out["dropped"] = dropped
        return out
