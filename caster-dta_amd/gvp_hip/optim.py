"""The optimizer update of a training step on the device: `FusedAdam`.

ctypes binding of include/caster_gvp_optim.h (csrc/optim_kernels.hip), a header and a version of its own beside the
main C ABI: the entry points live in the same libcaster_gvp.so, the signature table below is this module's.
`FusedAdam.step(scaler)` is the whole of the reference's train_model.py:578-587 -- `scaler.unscale_`,
`clip_grad_norm_`, `scaler.step(optimizer)`, `scaler.update()` -- as one host call that launches a norm kernel, a
scalar kernel and an update kernel per table of 80 parameter tensors, reads every changing scalar from device memory
and never synchronises: it can be captured (gvp_hip.graphed.GraphedTrainStep(optimizer=...)).
"""
from __future__ import annotations

import ctypes as C
import functools

import torch

from . import _lib
from ._lib import _on_gpu, _ptr, _stream

OPTIM_VERSION = 1        # CGVP_OPTIM_VERSION
MAX_SEGMENTS = 80        # CGVP_OPTIM_MAX_SEGMENTS (per launch; a step takes any number)
CHUNK = 4096             # CGVP_OPTIM_CHUNK


class Segment(C.Structure):
    """cgvp_optim_segment: one parameter tensor."""
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("numel", C.c_int64)]


class Hyper(C.Structure):
    """cgvp_optim_hyper: the host scalars of a step."""
    _fields_ = [("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("weight_decay", C.c_double),
                ("decoupled", C.c_int32), ("dry", C.c_int32), ("max_norm", C.c_double), ("growth_factor", C.c_double),
                ("backoff_factor", C.c_double), ("growth_interval", C.c_int32), ("reserved", C.c_int32)]


_P, _I64, _I32 = C.c_void_p, C.c_int64, C.c_int32
_SIGNATURES = {
    "cgvp_optim_version": (C.c_int, []),
    "cgvp_optim_workspace_bytes": (C.c_int64, [C.POINTER(C.c_int64), _I32]),
    "cgvp_optim_adam_step": (C.c_int, [C.POINTER(Segment), _I32, C.POINTER(Hyper), _P, _P, _P, _P, _P, _P, _P, _I64, _P]),
}


def exported_symbols():
    """Names include/caster_gvp_optim.h declares."""
    return tuple(_SIGNATURES)


@functools.lru_cache(maxsize=None)
def lib():
    """libcaster_gvp.so (the handle of `_lib.lib()`) with the optimizer entry points typed (once)."""
    return _lib.bind(_lib.lib(), _SIGNATURES, "cgvp_optim_version", OPTIM_VERSION, "optimizer version")


def workspace_bytes(numels):
    """Bytes of workspace for one step over tensors of these sizes (cgvp_optim_workspace_bytes)."""
    arr = (C.c_int64 * max(len(numels), 1))(*numels)
    n = int(lib().cgvp_optim_workspace_bytes(arr, len(numels)))
    if n < 0:
        raise ValueError(f"cgvp_optim_workspace_bytes: bad argument (code {n})")
    return n


class FusedAdam(torch.optim.Optimizer):
    """Adam (`decoupled=False`: weight decay as an L2 term) or AdamW (`decoupled=True`) with the arithmetic of
    torch.optim.Adam / AdamW(amsgrad=False, maximize=False), over ONE parameter group of fp32 parameters on one MI355X.

        opt = FusedAdam(model.parameters(), lr=1e-4, max_grad_norm=1.0)
        scaler.scale(loss).backward()
        opt.step(scaler)                      # = unscale_ + clip_grad_norm_ + scaler.step(opt) + scaler.update()

    Unlike `unscale_` / `clip_grad_norm_`, a step does NOT write gradient memory: `p.grad` keeps the raw, still scaled
    gradient.  `last_grad_norm` (of the unscaled gradients, before clipping) and `last_found_inf` are device tensors;
    reading them is the caller's synchronisation, a step makes none.  A step whose gradients hold a NaN or an Inf
    changes nothing but the loss scale.

    State: all `exp_avg` and `exp_avg_sq` live in one flat buffer, `state[p]` holds views of it and the shared `step`
    tensor, so `state_dict()` has the layout of torch.optim.Adam and checkpoints move between the two in both
    directions; `load_state_dict` copies into the buffer.  Schedulers work on `param_groups[0]["lr"]`: the value is
    copied to the device when it has changed.  The other hyperparameters are read from the group at every call, but
    are baked into a captured step.
    """

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, decoupled=False,
                 max_grad_norm=None, amsgrad=False):
        if amsgrad:
            raise ValueError("FusedAdam: amsgrad is not implemented")
        if not 0.0 <= lr:
            raise ValueError(f"FusedAdam: invalid learning rate {lr}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"FusedAdam: betas must lie in [0, 1), got {betas}")
        if not 0.0 <= eps:
            raise ValueError(f"FusedAdam: invalid eps {eps}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"FusedAdam: invalid weight_decay {weight_decay}")
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                        decoupled_weight_decay=bool(decoupled), max_grad_norm=max_grad_norm)
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise ValueError(f"FusedAdam: one parameter group only, got {len(self.param_groups)}")
        ps = self.param_groups[0]["params"]
        for i, p in enumerate(ps):
            if p.dtype != torch.float32:
                raise ValueError(f"FusedAdam: parameter {i} is {p.dtype}; only float32 parameters are updated")
            _on_gpu(p, f"FusedAdam: parameter {i}")
            if p.device != ps[0].device:
                raise ValueError(f"FusedAdam: parameter {i} is on {p.device}, parameter 0 on {ps[0].device}")
            if not p.is_contiguous():
                raise ValueError(f"FusedAdam: parameter {i} is not contiguous")
        self._lib = lib()
        dev = self.device = ps[0].device
        total = sum(p.numel() for p in ps)
        # [exp_avg of every parameter | exp_avg_sq of every parameter | lr, step, grad_norm, found_inf]
        self._flat = torch.zeros(2 * total + 4, dtype=torch.float32, device=dev)
        sc = self._flat[2 * total:]
        self._lr, self._step, self._grad_norm, self._found_inf = sc[0:1], sc[1:2], sc[2:3], sc[3:4]
        self._lr_host = None
        step = self._step.view(())
        off = 0
        for p in ps:
            n = p.numel()
            self.state[p] = {"step": step, "exp_avg": self._flat[off:off + n].view(p.shape),
                             "exp_avg_sq": self._flat[total + off:total + off + n].view(p.shape)}
            off += n
        self._workspace = torch.empty(workspace_bytes([p.numel() for p in ps]) // 8, dtype=torch.float64, device=dev)
        self._table_key, self._table, self._table_len = None, None, 0

    # ------------------------------------------------------------ reporting
    @property
    def last_grad_norm(self):
        """Global L2 norm of the unscaled gradients of the last step, before clipping (0-dim device tensor)."""
        return self._grad_norm.view(())

    @property
    def last_found_inf(self):
        """1.0 when the last step met a NaN / Inf gradient and was skipped, else 0.0 (0-dim device tensor)."""
        return self._found_inf.view(())

    # ------------------------------------------------------------ checkpoints
    def state_dict(self):
        """The layout of torch.optim.Adam: per parameter `step`, `exp_avg`, `exp_avg_sq`.  The tensors are COPIES:
        torch's `load_state_dict` keeps the tensors it is given, and an optimizer that adopted views of the flat buffer
        (or the one `step` all parameters share) would update this one's state."""
        sd = super().state_dict()
        sd["state"] = {i: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()} for i, st in sd["state"].items()}
        return sd

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """Accepts what `state_dict()` of this class or of torch.optim.Adam / AdamW over the same parameters returns.
        The values are COPIED into the flat buffer (its views stay), the group's hyperparameters are taken over."""
        groups = state_dict["param_groups"]
        if len(groups) != 1:
            raise ValueError(f"FusedAdam: one parameter group only, the checkpoint has {len(groups)}")
        saved, group = groups[0], self.param_groups[0]
        if len(saved["params"]) != len(group["params"]):
            raise ValueError(f"FusedAdam: the checkpoint's group has {len(saved['params'])} parameters, this optimizer "
                             f"{len(group['params'])}")
        if saved.get("amsgrad") or saved.get("maximize"):
            raise ValueError("FusedAdam: a checkpoint with amsgrad or maximize cannot be continued")
        state = state_dict["state"]
        steps = {float(s["step"]) for s in state.values()}
        if len(steps) > 1:
            raise ValueError(f"FusedAdam: the checkpoint's parameters are at different steps {sorted(steps)}; "
                             "one count is kept for all")
        for pid, p in zip(saved["params"], group["params"]):
            mine, theirs = self.state[p], state.get(pid)
            for key in ("exp_avg", "exp_avg_sq"):
                if theirs is None:
                    mine[key].zero_()                       # (a parameter that never had a gradient)
                elif tuple(theirs[key].shape) != tuple(p.shape):
                    raise ValueError(f"FusedAdam: {key} of parameter {pid} has shape {tuple(theirs[key].shape)}, the "
                                     f"parameter {tuple(p.shape)}")
                else:
                    mine[key].copy_(theirs[key])
        self._step.fill_(steps.pop() if steps else 0.0)
        for key, value in saved.items():
            if key != "params":
                group[key] = value
        group.setdefault("decoupled_weight_decay", False)
        group.setdefault("max_grad_norm", None)

    # ------------------------------------------------------------ the step
    def sync_lr(self):
        """Copy param_groups[0]['lr'] to the device scalar if it has changed (one small launch; not captured: call it
        before a replay, as GraphedTrainStep.run does)."""
        lr = float(self.param_groups[0]["lr"])
        if lr != self._lr_host:
            self._lr.fill_(lr)
            self._lr_host = lr

    def hyper_key(self):
        """The host scalars a launch bakes in (a captured step keeps those of its capture)."""
        g = self.param_groups[0]
        return (float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]),
                bool(g.get("decoupled_weight_decay", False)), g.get("max_grad_norm"))

    def _segments(self, grads):
        ps = self.param_groups[0]["params"]
        if len(grads) != len(ps):
            raise ValueError(f"FusedAdam: {len(grads)} gradients for {len(ps)} parameters")
        key = tuple((p.data_ptr(), g.data_ptr()) for p, g in zip(ps, grads) if g is not None)
        if key != self._table_key:
            rows = []
            for i, (p, g) in enumerate(zip(ps, grads)):
                if g is None or p.numel() == 0:
                    continue
                if not g.is_cuda or g.device != self.device or g.dtype != torch.float32 or g.shape != p.shape \
                        or not g.is_contiguous() or g.is_sparse:
                    raise ValueError(f"FusedAdam: the gradient of parameter {i} must be a dense contiguous float32 tensor "
                                     f"of shape {tuple(p.shape)} on {self.device}")
                if not p.is_contiguous():
                    raise ValueError(f"FusedAdam: parameter {i} is not contiguous")
                st = self.state[p]
                rows.append(Segment(p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                                    p.numel()))
            self._table = (Segment * max(len(rows), 1))(*rows)
            self._table_len, self._table_key = len(rows), key
        return self._table, self._table_len

    def apply(self, grads, scaler=None, dry=False):
        """One update from an explicit gradient list (`grads[i]` belongs to parameter i of the group, None = leave the
        parameter out): the capturable core of `step`.  It launches kernels on the current stream and touches nothing
        else -- no allocation, no host read, no copy of the learning rate (`sync_lr`).  `dry`: only `last_grad_norm`
        and `last_found_inf` are written."""
        table, n = self._segments(grads)
        g = self.param_groups[0]
        if g.get("amsgrad") or g.get("maximize"):
            raise ValueError("FusedAdam: amsgrad and maximize are not implemented")
        max_norm = g.get("max_grad_norm")
        hyper = Hyper(beta1=g["betas"][0], beta2=g["betas"][1], eps=g["eps"], weight_decay=g["weight_decay"],
                      decoupled=1 if g.get("decoupled_weight_decay", False) else 0, dry=1 if dry else 0,
                      max_norm=float(max_norm) if max_norm is not None else 0.0, growth_factor=2.0, backoff_factor=0.5,
                      growth_interval=2000)
        scale = tracker = None
        if scaler is not None and scaler.is_enabled():
            if scaler._scale is None:
                scaler._lazy_init_scale_growth_tracker(self.device)
            scale, tracker = scaler._scale, scaler._growth_tracker
            if scale.device != self.device or scale.dtype != torch.float32 or tracker.dtype != torch.int32:
                raise ValueError("FusedAdam: the GradScaler's scale / growth tracker must be float32 / int32 on the "
                                 "parameters' device")
            hyper.growth_factor, hyper.backoff_factor = scaler.get_growth_factor(), scaler.get_backoff_factor()
            hyper.growth_interval = scaler.get_growth_interval()
        with torch.cuda.device(self.device):
            rc = self._lib.cgvp_optim_adam_step(table, n, C.byref(hyper), _ptr(self._lr), _ptr(self._step), _ptr(scale),
                                                _ptr(tracker), _ptr(self._grad_norm), _ptr(self._found_inf),
                                                _ptr(self._workspace), self._workspace.numel() * 8, _stream())
        _lib.check(rc, "cgvp_optim_adam_step")

    def step(self, scaler=None, closure=None):
        """The update from `p.grad` of every parameter that has one, with `scaler`'s loss scale and its update when a
        torch.amp.GradScaler is given (do not call `scaler.step` / `scaler.update` as well).  No host synchronisation."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        grads = [p.grad for p in self.param_groups[0]["params"]]
        if all(g is None for g in grads):
            return loss
        self.sync_lr()
        self.apply(grads, scaler=scaler)
        return loss
