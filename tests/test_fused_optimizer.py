"""The fused optimizer update (csrc/optim_kernels.hip, include/caster_gvp_optim.h, gvp_hip.optim.FusedAdam) and its
place inside the captured training step (gvp_hip.graphed.GraphedTrainStep(optimizer=...)).

REFERENCE.  `Ref64` below restates the semantics of include/caster_gvp_optim.h in float64 NumPy.  On the CPU it is
pinned to 1e-12 against stock PyTorch in float64 -- scaler.unscale_, clip_grad_norm_, scaler.step(Adam / AdamW(foreach=
False)), scaler.update(), the order of the reference's train_model.py:578-587 -- and then serves the GPU tests.

BOUND.  The error of a float32 update is measured as  max |p - p64| / (|p64| + steps * lr)  against `Ref64`.  The
kernels may use at most 4x the error stock float32 torch.optim.Adam / AdamW(foreach=False) (after clip_grad_norm_, on
the CPU) makes on the same inputs against the same reference: the factor covers a different but equally valid order of
operations (fused multiply-adds, g * (inv * clip) in one product).  The bound is computed inside each test from the
stock run, never from the kernels.  Measured: profiles/fused_optimizer/README.md.

Segments of the kernel-level tests are views into larger buffers whose every other element is a canary; the canaries
are compared bitwise after every call.
"""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import davis_synth as ds
from conftest import GOLDEN, REPO
from gvp_hip import _lib, optim

DEV = "cuda:0"
SETTINGS = {"adam": dict(weight_decay=0.0, decoupled=False), "adam_l2": dict(weight_decay=1e-2, decoupled=False),
            "adamw": dict(weight_decay=1e-2, decoupled=True)}
LR, BETAS, EPS, STEPS = 1e-3, (0.9, 0.999), 1e-8, 6
EDGE_SIZES = (1, 3, 4, 5, 1023, 1024, 1025, 2049, 4099)
CANARY = float(np.float32(-7.25e11))          # (compared as a Python float too: exactly a float32)


# ---------------------------------------------------------------------------------------------------------------------
# float64 restatement of include/caster_gvp_optim.h
class Ref64:
    def __init__(self, params, lr=LR, betas=BETAS, eps=EPS, weight_decay=0.0, decoupled=False, max_norm=None,
                 scale=None, growth_factor=2.0, backoff_factor=0.5, growth_interval=2):
        self.p = [np.array(p, dtype=np.float64) for p in params]
        self.m = [np.zeros_like(p) for p in self.p]
        self.v = [np.zeros_like(p) for p in self.p]
        self.lr, self.betas, self.eps, self.wd, self.decoupled, self.max_norm = lr, betas, eps, weight_decay, decoupled, max_norm
        self.step, self.scale, self.tracker = 0, scale, 0
        self.growth_factor, self.backoff_factor, self.growth_interval = growth_factor, backoff_factor, growth_interval
        self.grad_norm, self.found_inf, self.clip = 0.0, False, 1.0

    def update(self, grads, dry=False):
        """grads[i] is None (parameter left out) or the raw, still scaled gradient."""
        inv = 1.0 / self.scale if self.scale is not None else 1.0
        have = [np.asarray(g, dtype=np.float64) for g in grads if g is not None]
        with np.errstate(all="ignore"):
            total = sum(float(np.sum(g * g)) for g in have)
            self.found_inf = not all(np.isfinite(g).all() for g in have)
            self.grad_norm = inv * np.sqrt(total)
        if dry:
            return
        if not self.found_inf:
            b1, b2 = self.betas
            self.clip = min(1.0, self.max_norm / (self.grad_norm + 1e-6)) if self.max_norm and self.max_norm > 0 else 1.0
            self.step += 1
            step_size = self.lr / (1.0 - b1 ** self.step)
            bc2_sqrt = np.sqrt(1.0 - b2 ** self.step)
            for i, g in enumerate(grads):
                if g is None:
                    continue
                g = np.asarray(g, dtype=np.float64) * inv * self.clip
                if self.decoupled:
                    self.p[i] *= 1.0 - self.lr * self.wd
                elif self.wd != 0:
                    g = g + self.wd * self.p[i]
                self.m[i] += (g - self.m[i]) * (1.0 - b1)
                self.v[i] = b2 * self.v[i] + (1.0 - b2) * g * g
                self.p[i] -= step_size * self.m[i] / (np.sqrt(self.v[i]) / bc2_sqrt + self.eps)
        if self.scale is not None:                                   # GradScaler.update()
            if self.found_inf:
                self.scale, self.tracker = self.scale * self.backoff_factor, 0
            else:
                self.tracker += 1
                if self.tracker >= self.growth_interval:
                    self.tracker = 0
                    if np.isfinite(np.float32(self.scale * self.growth_factor)):
                        self.scale = self.scale * self.growth_factor


def step_error(p, p64, steps, lr=LR):
    """max |p - p64| / (|p64| + steps * lr) over all tensors"""
    worst = 0.0
    for a, b in zip(p, p64):
        a = np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float64).reshape(-1)
        b = np.asarray(b, dtype=np.float64).reshape(-1)
        if a.size:
            worst = max(worst, float(np.max(np.abs(a - b) / (np.abs(b) + steps * lr))))
    return worst


def stock_cpu(params, grad_steps, dtype, weight_decay=0.0, decoupled=False, max_norm=None, scaler=None, lr=LR):
    """Stock PyTorch on the CPU in `dtype`, in the order of train_model.py:578-587.  grad_steps[k][i] is the UNSCALED
    gradient of parameter i in step k; with a scaler the loss sum(p * g) is scaled and back-propagated."""
    ps = [torch.nn.Parameter(torch.as_tensor(np.asarray(p)).to(dtype).clone()) for p in params]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls(ps, lr=lr, betas=BETAS, eps=EPS, weight_decay=weight_decay, foreach=False)
    for grads in grad_steps:
        opt.zero_grad(set_to_none=True)
        gs = [torch.as_tensor(np.asarray(g)).to(dtype) for g in grads]
        if scaler is not None:
            with np.errstate(all="ignore"):
                scaler.scale(sum((p * g).sum() for p, g in zip(ps, gs))).backward()
            scaler.unscale_(opt)
        else:
            for p, g in zip(ps, gs):
                p.grad = g.clone()
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(ps, max_norm)
        if scaler is not None:
            scaler.step(opt)
            scaler.update()
        else:
            opt.step()
    return ps, opt


def make_problem(sizes, seed, steps=STEPS, quiet_steps=(1, 4)):
    """Parameters and per-step gradients whose magnitudes span four decades (10^U(-2, 2)); the steps in `quiet_steps`
    are a million times smaller, so that a max_grad_norm of 1 clips in some steps and not in others."""
    rng = np.random.default_rng(seed)
    params = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    grad_steps = []
    for k in range(steps):
        amp = 1e-6 if k in quiet_steps else 1.0
        grad_steps.append([(rng.standard_normal(n) * 10.0 ** rng.uniform(-2, 2, n) * amp).astype(np.float32) for n in sizes])
    return params, grad_steps


# ---------------------------------------------------------------------------------------------------------------------
# CPU
def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(cgvp_[a-z0-9_]+)\s*\(", text))


def test_optimizer_entry_points_have_a_header_and_a_version_of_their_own():
    header = os.path.join(REPO, "include", "caster_gvp_optim.h")
    assert _declared(header) == set(optim.exported_symbols())
    handle = C.CDLL(_lib.LIB_PATH)
    main = open(os.path.join(REPO, "include", "caster_gvp.h")).read()
    for name in optim.exported_symbols():
        assert hasattr(handle, name), name
        assert name not in main and name not in _lib.exported_symbols(), name
    text = open(header).read()
    assert optim.lib().cgvp_optim_version() == 1 == optim.OPTIM_VERSION and "#define CGVP_OPTIM_VERSION 1" in text
    assert f"#define CGVP_OPTIM_MAX_SEGMENTS {optim.MAX_SEGMENTS}\n" in text and f"#define CGVP_OPTIM_CHUNK {optim.CHUNK}\n" in text
    assert C.sizeof(optim.Segment) == 40 and C.sizeof(optim.Hyper) == 72
    assert _lib.ABI_VERSION == 31 and _lib.lib().cgvp_abi_version() == 31
    assert "C ABI v1" not in re.sub(r"C ABI v31", "", open(os.path.join(REPO, "INTEGRATION.md")).read())


def test_entry_points_refuse_bad_arguments_on_the_host():
    """Every refusal is CGVP_ERR_BAD_ARG before any launch: no GPU is needed (or touched)."""
    L = optim.lib()
    BAD, null, p, odd = -1, 0, 0x10000, 0x10002          # never dereferenced: the checks run on the host

    def call(n=2, numel=(5, 4099), hyper=None, null_hyper=False, null_segs=False, ws=p, ws_bytes=None, **ptrs):
        names = ("param", "grad", "exp_avg", "exp_avg_sq")
        table = (optim.Segment * max(len(numel), 1))()
        for i, k in enumerate(numel):
            table[i] = optim.Segment(*[ptrs.get(f"{nm}{i}", p) for nm in names], k)
        h = optim.Hyper(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, decoupled=0, dry=0, max_norm=1.0,
                        growth_factor=2.0, backoff_factor=0.5, growth_interval=2)
        for k, v in (hyper or {}).items():
            setattr(h, k, v)
        need = 64 + 8 * sum((k + optim.CHUNK - 1) // optim.CHUNK for k in numel if k > 0)
        sc = {k: ptrs.get(k, p) for k in ("lr", "step", "grad_norm", "found_inf")}
        return L.cgvp_optim_adam_step(None if null_segs else table, n, None if null_hyper else C.byref(h), sc["lr"],
                                      sc["step"], ptrs.get("scale", null), ptrs.get("tracker", null), sc["grad_norm"],
                                      sc["found_inf"], ws, need if ws_bytes is None else ws_bytes, null)

    for name in ("param0", "grad0", "exp_avg1", "exp_avg_sq1", "lr", "step", "grad_norm", "found_inf"):
        assert call(**{name: null}) == BAD, (name, "null")
        assert call(**{name: odd}) == BAD, (name, "misaligned")
    assert call(scale=p) == BAD and call(tracker=p) == BAD                     # both or neither
    assert call(scale=odd, tracker=p) == BAD and call(scale=p, tracker=odd) == BAD
    assert call(n=-1) == BAD and call(null_segs=True) == BAD and call(null_hyper=True) == BAD
    assert call(numel=(5, -1)) == BAD
    assert call(ws=null) == BAD and call(ws=0x10004) == BAD and call(ws_bytes=64 + 8 * 2) == BAD
    for key in ("beta1", "beta2"):
        for value in (1.0, -0.1, 1.5, float("nan")):
            assert call(hyper={key: value}) == BAD, (key, value)
    assert call(hyper={"eps": -1e-8}) == BAD and call(hyper={"eps": float("nan")}) == BAD
    assert call(hyper={"growth_interval": 0}) == BAD and call(hyper={"growth_interval": -3}) == BAD
    # the size function
    sizes = (C.c_int64 * 5)(0, 1, 4096, 4097, 10000)
    assert L.cgvp_optim_workspace_bytes(sizes, 5) == 64 + 8 * (0 + 1 + 1 + 2 + 3)
    assert L.cgvp_optim_workspace_bytes(sizes, 0) == 64 and L.cgvp_optim_workspace_bytes(None, 0) == 64
    assert L.cgvp_optim_workspace_bytes(sizes, -1) == BAD and L.cgvp_optim_workspace_bytes(None, 2) == BAD
    assert L.cgvp_optim_workspace_bytes((C.c_int64 * 2)(3, -1), 2) == BAD


@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("nonfinite", [False, True])
def test_float64_restatement_equals_stock_pytorch(setting, nonfinite):
    """Ref64 against scaler.unscale_ + clip_grad_norm_ + scaler.step(Adam / AdamW) + scaler.update() in float64 on the
    CPU: parameters, moments, step, scale and growth tracker to 1e-12 relative over 6 steps (one of them non-finite)."""
    sizes = (1, 3, 17, 260)
    params, grad_steps = make_problem(sizes, seed=11)
    grad_steps = [[g.astype(np.float64) for g in gs] for gs in grad_steps]
    if nonfinite:
        grad_steps[2][3][7] = np.inf
    kw = SETTINGS[setting]
    scaler = torch.amp.GradScaler("cpu", init_scale=1024, growth_interval=2)
    ps, opt = stock_cpu(params, grad_steps, torch.float64, max_norm=1.0, scaler=scaler, **kw)
    ref = Ref64(params, max_norm=1.0, scale=1024.0, growth_interval=2, **kw)
    clips = []
    for gs in grad_steps:
        ref.update([g * ref.scale for g in gs])                      # what scaler.scale(loss).backward() leaves in p.grad
        clips.append(ref.clip)
    assert min(clips) < 1.0 and max(clips) == 1.0                    # both branches of the clip
    close = lambda a, b: np.allclose(np.asarray(a), np.asarray(b), rtol=1e-12, atol=0.0)
    for i, q in enumerate(ps):
        st = opt.state[q]
        assert close(ref.p[i], q.detach().numpy()), i
        assert close(ref.m[i], st["exp_avg"].numpy()) and close(ref.v[i], st["exp_avg_sq"].numpy()), i
        assert float(st["step"]) == ref.step == (5 if nonfinite else 6)
    assert scaler.get_scale() == ref.scale and int(scaler._growth_tracker) == ref.tracker
    assert ref.scale == (2048.0 if nonfinite else 8192.0)            # 1024 -> 2048 -> (inf: 1024) -> 2048 / 1024 * 2^3


def test_fused_adam_refuses_what_it_does_not_update():
    from gvp_hip.optim import FusedAdam
    w = lambda dtype=torch.float32: torch.nn.Parameter(torch.zeros(3, dtype=dtype))
    with pytest.raises(RuntimeError, match="MI355X only"):
        FusedAdam([w()])
    with pytest.raises(ValueError, match="float32"):
        FusedAdam([w(torch.float64)])
    with pytest.raises(ValueError, match="float32"):
        FusedAdam([w(torch.bfloat16)])
    with pytest.raises(ValueError, match="one parameter group"):
        FusedAdam([{"params": [w()]}, {"params": [w()], "lr": 1e-3}])
    with pytest.raises(ValueError, match="amsgrad"):
        FusedAdam([w()], amsgrad=True)
    with pytest.raises(ValueError, match="betas"):
        FusedAdam([w()], betas=(0.9, 1.0))
    with pytest.raises(ValueError, match="eps"):
        FusedAdam([w()], eps=-1.0)


# ---------------------------------------------------------------------------------------------------------------------
# GPU, kernel level: segments inside canary buffers
class Harness:
    """Segments of the given sizes laid into four buffers (param, grad, exp_avg, exp_avg_sq) at the given byte offsets
    from a 16-byte boundary, at least 8 canary floats on both sides of each."""

    def __init__(self, sizes, params, offsets, scale=None, lr=LR, **hyper):
        self.sizes, self.n = list(sizes), len(sizes)
        self.lib = optim.lib()
        self.bufs, self.views, self.masks = {}, {}, {}
        for kind in ("param", "grad", "exp_avg", "exp_avg_sq"):
            pos, cur = [], 8
            for i, n in enumerate(sizes):
                cur = (cur + 3) // 4 * 4 + offsets[kind][i] // 4
                pos.append(cur)
                cur += n + 8
            buf = torch.full((cur + 8,), CANARY, dtype=torch.float32, device=DEV)
            assert buf.data_ptr() % 16 == 0
            mask = torch.zeros(cur + 8, dtype=torch.bool, device=DEV)
            for at, n in zip(pos, sizes):
                mask[at:at + n] = True
            self.bufs[kind], self.masks[kind] = buf, mask
            self.views[kind] = [buf[at:at + n] for at, n in zip(pos, sizes)]
            for i, v in enumerate(self.views[kind]):
                assert v.data_ptr() % 16 == offsets[kind][i] or v.numel() == 0
                v.copy_(torch.from_numpy(np.asarray(params[i], dtype=np.float32))) if kind == "param" else v.zero_()
        # device scalars, canaries around them too: [c, lr, c, step, c, grad_norm, c, found_inf, c, scale, c]
        self.sc = torch.full((11,), CANARY, dtype=torch.float32, device=DEV)
        self.sc[1], self.sc[3], self.sc[5], self.sc[7] = lr, 0.0, -1.0, -1.0
        self.tracker = torch.tensor([-99, 0, -99], dtype=torch.int32, device=DEV)
        self.scaled = scale is not None
        if self.scaled:
            self.sc[9] = scale
        self.hyper = dict(beta1=BETAS[0], beta2=BETAS[1], eps=EPS, weight_decay=0.0, decoupled=0, dry=0, max_norm=0.0,
                          growth_factor=2.0, backoff_factor=0.5, growth_interval=2)
        self.hyper.update(hyper)
        self.table = (optim.Segment * max(self.n, 1))(*[
            optim.Segment(*[self.views[k][i].data_ptr() if sizes[i] else 0 for k in ("param", "grad", "exp_avg", "exp_avg_sq")],
                          sizes[i]) for i in range(self.n)])
        need = optim.workspace_bytes(self.sizes)
        self.ws = torch.full((need // 8 + 2,), CANARY, dtype=torch.float64, device=DEV)
        self.ws_bytes = need

    def set_grads(self, grads):
        for v, g in zip(self.views["grad"], grads):
            v.copy_(torch.from_numpy(np.asarray(g, dtype=np.float32)))

    def call(self, dry=False):
        h = optim.Hyper(**dict(self.hyper, dry=1 if dry else 0))
        at = lambda i: C.c_void_p(self.sc.data_ptr() + 4 * i)
        rc = self.lib.cgvp_optim_adam_step(
            self.table, self.n, C.byref(h), at(1), at(3), at(9) if self.scaled else None,
            C.c_void_p(self.tracker.data_ptr() + 4) if self.scaled else None, at(5), at(7),
            C.c_void_p(self.ws.data_ptr()), self.ws_bytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc
        torch.cuda.synchronize()
        self.check_canaries()

    def check_canaries(self):
        for kind, buf in self.bufs.items():
            outside = buf[~self.masks[kind]]
            assert bool((outside == CANARY).all()), f"a canary of the {kind} buffer was overwritten"
        sc = self.sc.cpu()
        assert all(float(sc[i]) == CANARY for i in ((0, 2, 4, 6, 8, 10) if self.scaled else (0, 2, 4, 6, 8, 9, 10)))
        assert self.tracker.cpu().tolist()[::2] == [-99, -99] and (self.scaled or int(self.tracker[1]) == 0)
        assert bool((self.ws[self.ws_bytes // 8:] == CANARY).all()), "the workspace was overrun"

    step = property(lambda self: float(self.sc[3]))
    grad_norm = property(lambda self: float(self.sc[5]))
    found_inf = property(lambda self: float(self.sc[7]))
    scale = property(lambda self: float(self.sc[9]))
    growth_tracker = property(lambda self: int(self.tracker[1]))

    def get(self, kind):
        return [v.cpu().numpy().copy() for v in self.views[kind]]

    def snapshot(self):
        return {k: b.clone() for k, b in self.bufs.items()} | {"sc": self.sc[[1, 3, 9]].clone(), "tr": self.tracker.clone()}

    def same_as(self, snap):
        bits = lambda t: t.view(torch.int32)
        return all(torch.equal(bits(self.bufs[k]), bits(snap[k])) for k in self.bufs) and \
            torch.equal(bits(self.sc[[1, 3, 9]]), bits(snap["sc"])) and torch.equal(self.tracker, snap["tr"])


def aligned(sizes):
    return {k: [0] * len(sizes) for k in ("param", "grad", "exp_avg", "exp_avg_sq")}


def run_against_stock(sizes, offsets, params, grad_steps, max_norm, scale=None, **kw):
    """(error of the kernels, error of stock float32 on the CPU, reference) after all steps, both against Ref64."""
    steps = len(grad_steps)
    ref = Ref64(params, max_norm=max_norm, **kw)
    h = Harness(sizes, params, offsets, scale=scale, weight_decay=kw["weight_decay"], decoupled=int(kw["decoupled"]),
                max_norm=max_norm or 0.0, growth_interval=1000)
    clips = []
    for gs in grad_steps:
        ref.update(gs)
        clips.append(ref.clip)
        h.set_grads([g * np.float32(scale) for g in gs] if scale else gs)     # (a power of two: the product is exact)
        h.call()
        assert h.found_inf == 0.0 and h.step == ref.step
        assert abs(h.grad_norm - ref.grad_norm) <= 2.0 ** -22 * ref.grad_norm
    stock, _ = stock_cpu(params, grad_steps, torch.float32, max_norm=max_norm, **kw)
    e_fused = step_error(h.get("param"), ref.p, steps)
    e_stock = step_error(stock, ref.p, steps)
    for kind, want in (("exp_avg", ref.m), ("exp_avg_sq", ref.v)):            # moments: a loose sanity bound, relative to the
        for a, b in zip(h.get(kind), want):                                   # segment's largest (g + wd * p may cancel)
            assert a.size == 0 or np.abs(a - b).max() <= 1e-5 * np.abs(b).max(), kind
    return e_fused, e_stock, clips


@pytest.mark.gpu
@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_edges_of_size_and_alignment_against_float64(setting):
    """(a) every edge size at every pair of param / grad byte offsets (0, 4, 8, 12 from a 16-byte boundary; the moments
    take two more combinations), 144 segments = two launch tables, 6 steps, clipping on (both branches) and off, and
    once with a loss scale: within 4x the error of stock float32 Adam."""
    sizes, off = [], {k: [] for k in ("param", "grad", "exp_avg", "exp_avg_sq")}
    for n in EDGE_SIZES:
        for po in (0, 4, 8, 12):
            for go in (0, 4, 8, 12):
                sizes.append(n)
                off["param"].append(po), off["grad"].append(go)
                off["exp_avg"].append((po + go) % 16), off["exp_avg_sq"].append((2 * po + go + 4) % 16)
    params, grad_steps = make_problem(sizes, seed=5)
    kw = SETTINGS[setting]
    for max_norm, scale in ((1.0, None), (None, None), (1.0, 1024.0)):
        e_fused, e_stock, clips = run_against_stock(sizes, off, params, grad_steps, max_norm, scale=scale, **kw)
        print(f"{setting} max_norm={max_norm} scale={scale}: fused {e_fused / 2.0 ** -24:.2f} x 2^-24, "
              f"stock fp32 {e_stock / 2.0 ** -24:.2f} x 2^-24")
        if max_norm:
            assert min(clips) < 1.0 and max(clips) == 1.0
        assert 0.0 < e_stock < 64 * 2.0 ** -24                       # the yardstick itself is a float32 rounding error
        assert e_fused <= 4.0 * e_stock, (setting, max_norm, scale, e_fused, e_stock)


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, optim.MAX_SEGMENTS, optim.MAX_SEGMENTS + 1, 2 * optim.MAX_SEGMENTS + 3])
def test_segment_counts_around_the_launch_cap(count):
    """(b) every segment is updated and the norm covers all of them (the clip factor depends on it), with empty
    segments in between."""
    sizes = [(1, 3, 5, 0, 17, 130)[i % 6] if count > 1 else 9 for i in range(count)]
    if count > 1:
        sizes[-1] = 7                                                 # the last segment of the last table is a real one
    rng = np.random.default_rng(count)
    off = {k: [int(o) if n else 0 for o, n in zip(rng.integers(0, 4, count) * 4, sizes)] for k in ("param", "grad", "exp_avg", "exp_avg_sq")}
    params, grad_steps = make_problem(sizes, seed=count, steps=2, quiet_steps=())
    e_fused, e_stock, clips = run_against_stock(sizes, off, params, grad_steps, 1.0, **SETTINGS["adam_l2"])
    assert max(clips) < 1.0 and e_fused <= 4.0 * e_stock, (e_fused, e_stock)
    h = Harness(sizes, params, off)                                   # unclipped: the first step moves every element by ~lr
    h.set_grads(grad_steps[0])
    h.call()
    for i, (before, after) in enumerate(zip(params, h.get("param"))):
        assert not np.any(before == after), i
    total = np.sqrt(sum(float(np.sum(g.astype(np.float64) ** 2)) for g in grad_steps[0]))
    assert abs(h.grad_norm - total) <= 2.0 ** -22 * total


@pytest.mark.gpu
def test_nonfinite_gradients_skip_the_step_and_back_off_the_scale():
    """(c) NaN, +Inf, -Inf at the first element of the first segment, the last element of the last segment and in a
    chunk tail; the next clean step applies; two clean steps double the scale; a finite 1e30 is not an overflow."""
    sizes = [5, 4099, 1025]
    off = {"param": [4, 8, 0], "grad": [12, 4, 8], "exp_avg": [0, 12, 4], "exp_avg_sq": [8, 0, 12]}
    params, grad_steps = make_problem(sizes, seed=3, steps=1, quiet_steps=())
    clean = grad_steps[0]
    h = Harness(sizes, params, off, scale=2.0 ** 20, max_norm=1.0, growth_interval=2)
    ref = Ref64(params, max_norm=1.0, scale=2.0 ** 20, growth_interval=2)
    h.set_grads(clean)
    h.call()
    ref.update(clean)
    places = ((0, 0), (2, 1024), (1, 4098), (1, 4095))       # ..., the 3-element tail of a chunk, the last lane of a full chunk
    for value in (float("nan"), float("inf"), float("-inf")):
        for seg, at in places:
            bad = [g.copy() for g in clean]
            bad[seg][at] = value
            h.tracker[1] = 1
            ref.tracker = 1
            snap, scale = h.snapshot(), h.scale
            h.set_grads(bad)
            snap["grad"] = h.bufs["grad"].clone()
            h.call()
            ref.update(bad)
            assert h.found_inf == 1.0 and h.scale == scale / 2 == ref.scale and h.growth_tracker == 0
            snap["sc"][2], snap["tr"][1] = scale / 2, 0
            assert h.same_as(snap), (value, seg, at)         # params, moments, step, lr: bitwise unchanged
            h.set_grads(clean)
            step = h.step
            h.call()
            ref.update(clean)
            assert h.found_inf == 0.0 and h.step == step + 1 == ref.step and h.growth_tracker == 1 and h.scale == scale / 2
            assert not h.same_as(snap)
    assert step_error(h.get("param"), ref.p, ref.step) < 1e-5          # the clean steps in between all applied
    h.tracker[1] = 0
    scale = h.scale
    h.call()
    assert h.scale == scale and h.growth_tracker == 1
    h.call()
    assert h.scale == 2 * scale and h.growth_tracker == 0             # growth_interval = 2
    huge = [g.copy() for g in clean]
    huge[1][77] = 1e30
    h.set_grads(huge)
    step = h.step
    h.call()
    assert h.found_inf == 0.0 and h.step == step + 1 and np.isfinite(h.grad_norm) and h.grad_norm > 1e29 / h.scale
    assert all(np.isfinite(p).all() for p in h.get("param"))


@pytest.mark.gpu
def test_dry_writes_the_norm_and_nothing_else():
    """(d)"""
    sizes = [3, 4099, 1, 1024]
    off = {"param": [4, 0, 12, 8], "grad": [8, 12, 0, 4], "exp_avg": [0, 4, 8, 12], "exp_avg_sq": [12, 8, 4, 0]}
    params, grad_steps = make_problem(sizes, seed=8, steps=2, quiet_steps=())
    h = Harness(sizes, params, off, scale=1024.0, max_norm=1.0, growth_interval=1, weight_decay=1e-2)
    h.set_grads(grad_steps[0])
    h.call()                                                          # a real step first: non-trivial moments
    h.set_grads(grad_steps[1])
    snap = h.snapshot()
    h.call(dry=True)
    assert h.same_as(snap)
    want = np.sqrt(sum(float(np.sum(g.astype(np.float64) ** 2)) for g in grad_steps[1])) / h.scale
    assert abs(h.grad_norm - want) <= 2.0 ** -22 * want and h.found_inf == 0.0
    bad = [g.copy() for g in grad_steps[1]]
    bad[3][1023] = np.inf
    h.set_grads(bad)
    snap = h.snapshot()
    h.call(dry=True)
    assert h.same_as(snap) and h.found_inf == 1.0                     # not even the scale backs off


@pytest.mark.gpu
def test_two_runs_are_bitwise_equal_at_any_alignment():
    """(e) the same values twice -> the same bits in parameters and norm; the norm does not depend on where the
    gradients lie either (every thread owns the same elements at any alignment)."""
    sizes = [4099, 5, 2049, 1023, 3]
    params, grad_steps = make_problem(sizes, seed=21, steps=3)
    offs = [{"param": [4, 0, 12, 8, 4], "grad": [8, 12, 0, 4, 0], "exp_avg": [0, 4, 8, 12, 8], "exp_avg_sq": [12, 8, 4, 0, 4]},
            aligned(sizes)]
    runs = []
    for off in (offs[0], offs[0], offs[1]):
        h = Harness(sizes, params, off, max_norm=1.0, weight_decay=1e-2)
        norms = []
        for gs in grad_steps:
            h.set_grads(gs)
            h.call()
            norms.append(np.float32(h.grad_norm).tobytes())
        runs.append((norms, [p.tobytes() for p in h.get("param")]))
    assert runs[0] == runs[1]
    assert runs[0][0] == runs[2][0]


# ---------------------------------------------------------------------------------------------------------------------
# GPU: FusedAdam
def _cuda_params(params):
    return [torch.nn.Parameter(torch.from_numpy(np.asarray(p, dtype=np.float32)).to(DEV)) for p in params]


def _feed(ps, grads):
    for p, g in zip(ps, grads):
        p.grad = torch.from_numpy(np.asarray(g, dtype=np.float32)).to(DEV).view(p.shape)


@pytest.mark.gpu
def test_checkpoints_move_between_fused_and_stock_adam():
    """(f) 3 steps with one optimizer, its state_dict loaded into the other over cloned parameters, 2 more steps: both
    continuations stay within the bound of (a); the layout is torch.optim.Adam's; loading keeps the flat buffer."""
    from gvp_hip.optim import FusedAdam
    sizes = [7, 165, 1, 4099]
    params, grad_steps = make_problem(sizes, seed=13, steps=5, quiet_steps=())
    kw = SETTINGS["adam_l2"]
    ref = Ref64(params, **kw)
    for gs in grad_steps:
        ref.update(gs)
    stock_all, _ = stock_cpu(params, grad_steps, torch.float32, **kw)
    bound = 4.0 * step_error(stock_all, ref.p, 5)
    make_stock = lambda ps: torch.optim.Adam(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=kw["weight_decay"], foreach=False)
    make_fused = lambda ps: FusedAdam(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=kw["weight_decay"])

    def run(opt, ps, steps):
        for gs in steps:
            _feed(ps, gs)
            opt.step()

    for first, second in ((make_fused, make_stock), (make_stock, make_fused)):
        a = _cuda_params(params)
        opt_a = first(a)
        run(opt_a, a, grad_steps[:3])
        sd = opt_a.state_dict()
        assert sorted(sd) == ["param_groups", "state"] and sorted(sd["state"]) == [0, 1, 2, 3]
        for i, st in sd["state"].items():
            assert sorted(st) == ["exp_avg", "exp_avg_sq", "step"] and float(st["step"]) == 3.0
            assert tuple(st["exp_avg"].shape) == tuple(st["exp_avg_sq"].shape) == (sizes[i],)
        b = _cuda_params([p.detach().cpu().numpy() for p in a])
        opt_b = second(b)
        if isinstance(opt_b, FusedAdam):
            where = [opt_b.state[q]["exp_avg"].data_ptr() for q in b]
            opt_b.load_state_dict(sd)
            assert where == [opt_b.state[q]["exp_avg"].data_ptr() for q in b]       # copied into the flat buffer
            assert float(opt_b.state[b[0]]["step"]) == 3.0
        else:
            opt_b.load_state_dict(sd)
            opt_b.param_groups[0]["foreach"] = False
        run(opt_a, a, grad_steps[3:])
        run(opt_b, b, grad_steps[3:])
        torch.cuda.synchronize()
        for name, ps in (("continued", a), ("loaded", b)):
            err = step_error(ps, ref.p, 5)
            assert err <= bound, (first.__name__, name, err, bound)
        assert float(opt_b.state[b[0]]["step"]) == 5.0


@pytest.mark.gpu
def test_learning_rate_is_read_from_the_group_every_step():
    """(g) a scheduler's write to param_groups[0]['lr'] takes effect at the next step; lr = 0 leaves the parameters
    bitwise alone while the moments move.  Bound: 100 x 2^-24 of the step metric -- two orders above the rounding of a
    float32 Adam step, five below what a missed learning-rate change costs (~0.5)."""
    from gvp_hip.optim import FusedAdam
    sizes = [5, 1030]
    params, grad_steps = make_problem(sizes, seed=17, steps=4, quiet_steps=())
    ps = _cuda_params(params)
    opt = FusedAdam(ps, lr=LR, max_grad_norm=1.0)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.5)
    ref = Ref64(params, max_norm=1.0)
    for k, lr in enumerate((LR, LR / 2, 0.0, 3e-3)):
        if k == 1:
            sched.step()
            assert opt.param_groups[0]["lr"] == LR / 2
        elif k > 1:
            opt.param_groups[0]["lr"] = lr
        ref.lr = lr
        before = [p.detach().clone() for p in ps]
        moments = [opt.state[p]["exp_avg"].clone() for p in ps]
        _feed(ps, grad_steps[k])
        opt.step()
        ref.update(grad_steps[k])
        if lr == 0.0:
            assert all(torch.equal(a.view(torch.int32), b.detach().view(torch.int32)) for a, b in zip(before, ps))
            assert all(not torch.equal(a, opt.state[p]["exp_avg"]) for a, p in zip(moments, ps))
        assert step_error(ps, ref.p, k + 1) <= 100 * 2.0 ** -24, (k, lr)
        assert abs(float(opt.last_grad_norm) - ref.grad_norm) <= 2.0 ** -22 * ref.grad_norm and float(opt.last_found_inf) == 0.0
    assert float(opt.state[ps[0]]["step"]) == 4.0
    # a parameter without a gradient is left out; one with a gradient still moves
    ps[0].grad = None
    kept = ps[0].detach().clone()
    opt.step()
    assert torch.equal(kept, ps[0].detach()) and float(opt.state[ps[0]]["step"]) == 5.0


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the captured step
def _to(d):
    return {k: (tuple(t.to(DEV) for t in v) if isinstance(v, tuple) else v.to(DEV)) for k, v in d.items()}


def _model(pretrained):
    from models.joint_gnn import JointGNN
    kw = json.load(open(os.path.join(GOLDEN, "model_kwargs.json")))
    model = JointGNN(protein_gnn_kwargs=kw["protein_gnn_kwargs"], molecule_gnn_kwargs=kw["molecule_gnn_kwargs"],
                     **kw["joint_gnn_kwargs"])
    model.load_state_dict(pretrained, strict=True)
    return model.to(DEV).eval()                                  # no dropout: the runs see the same numbers


def _batches():
    """The three six-pair batches of test_hip_models.py::test_graphed_train_step_equals_eager (two share a bucket)."""
    out = []
    for seed, lengths in ((1, [120, 80, 95, 130, 60, 101]), (2, [118, 83, 95, 128, 62, 100]), (3, [200, 150, 170, 90, 60, 210])):
        p, m = ds.pair_batch(6, seed, lengths=lengths)
        pd, md = _to(ds.to_torch(p)), _to(ds.to_torch(m))
        pd["ptr"], md["ptr"] = torch.as_tensor(p.ptr).to(DEV), torch.as_tensor(m.ptr).to(DEV)
        target = torch.randn(6, 1, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
        out.append((pd, md, target))
    return out


@pytest.mark.gpu
def test_captured_step_updates_exactly_as_the_eager_optimizer(pretrained):
    """(h) GraphedTrainStep(optimizer=FusedAdam): after every `run` the model's parameters equal, bit for bit, a shadow
    copy stepped eagerly by a second FusedAdam on clones of the published p.grad.  The step count is 1 after the first
    run -- a warm-up pass that applied its update would make it 3 -- and 3 at the end."""
    from gvp_hip.graphed import GraphedTrainStep
    from gvp_hip.optim import FusedAdam
    assert _lib.bridge() is not None
    model = _model(pretrained)
    params = list(model.parameters())
    shadow = [p.detach().clone() for p in params]
    opt = FusedAdam(params, lr=1e-3, weight_decay=1e-2, max_grad_norm=1.0)
    shadow_opt = FusedAdam(shadow, lr=1e-3, weight_decay=1e-2, max_grad_norm=1.0)
    runner = GraphedTrainStep(model, torch.nn.functional.mse_loss, optimizer=opt)
    for k, (pd, md, target) in enumerate(_batches()):
        loss, pred = runner.run(pd, md, target)
        assert loss.shape == () and pred.shape == (6, 1)
        for p, s in zip(params, shadow):
            s.grad = p.grad.clone() if p.grad is not None else None
        assert sum(p.grad is not None for p in params) >= 100
        shadow_opt.step()
        torch.cuda.synchronize()
        assert float(opt.state[params[0]]["step"]) == k + 1 == float(shadow_opt.state[shadow[0]]["step"])
        assert float(opt.last_found_inf) == 0.0
        assert torch.equal(opt.last_grad_norm.view(torch.int32), shadow_opt.last_grad_norm.view(torch.int32))
        for i, (p, s) in enumerate(zip(params, shadow)):
            assert torch.equal(p.detach().view(torch.int32), s.view(torch.int32)), (k, i)
    assert float(opt.last_grad_norm) > 0.0
    assert 1 <= len(runner.buckets) <= 3 and sum(b.steps for b in runner.buckets.values()) == 3
    moved = sum(not torch.equal(p.detach().cpu(), q) for p, q in zip(params, [pretrained[k] for k, _ in model.named_parameters()]))
    assert moved >= 100                                                # the update really ran


@pytest.mark.gpu
def test_captured_step_with_a_grad_scaler(pretrained):
    """(i) the scaler's own tensors are updated inside the captured step; an overflowing batch changes nothing but the
    scale; the forward numbers are those of the run without a scaler."""
    from gvp_hip.graphed import GraphedTrainStep
    from gvp_hip.optim import FusedAdam
    batches = _batches()
    plain = GraphedTrainStep(_model(pretrained), torch.nn.functional.mse_loss)
    loss0, pred0 = (t.clone() for t in plain.run(*batches[0]))
    model = _model(pretrained)
    params = list(model.parameters())
    opt = FusedAdam(params, lr=1e-3, max_grad_norm=1.0)
    scaler = torch.amp.GradScaler("cuda", init_scale=1024, growth_interval=2)
    runner = GraphedTrainStep(model, torch.nn.functional.mse_loss, scaler=scaler, optimizer=opt)
    loss, pred = runner.run(*batches[0])
    torch.cuda.synchronize()
    assert float((loss - loss0).abs()) <= 1e-5 * float(loss0.abs())
    assert float((pred - pred0).abs().max()) <= 1e-5 * float(pred0.abs().max())
    assert float(scaler._scale) == 1024.0 and int(scaler._growth_tracker) == 1 and float(opt.state[params[0]]["step"]) == 1.0
    runner.run(*batches[1])
    assert float(scaler._scale) == 2048.0 and int(scaler._growth_tracker) == 0 and float(opt.state[params[0]]["step"]) == 2.0
    before = [p.detach().clone() for p in params]
    moments = opt._flat.clone()
    pd, md, target = batches[2]
    target = target.clone()
    target[3, 0] = float("inf")
    runner.run(pd, md, target)
    torch.cuda.synchronize()
    assert float(opt.last_found_inf) == 1.0 and float(scaler._scale) == 1024.0 and int(scaler._growth_tracker) == 0
    assert float(opt.state[params[0]]["step"]) == 2.0
    for p, q in zip(params, before):
        assert torch.equal(p.detach().view(torch.int32), q.view(torch.int32))
    n = 2 * sum(p.numel() for p in params)
    assert torch.equal(opt._flat[:n].view(torch.int32), moments[:n].view(torch.int32))
    runner.run(*batches[2])                                            # the same bucket, clean: the step applies again
    assert float(opt.last_found_inf) == 0.0 and float(opt.state[params[0]]["step"]) == 3.0 and int(scaler._growth_tracker) == 1


@pytest.mark.gpu
def test_captured_step_refuses_other_optimizers(pretrained):
    """(j)"""
    from gvp_hip.graphed import GraphedTrainStep
    from gvp_hip.optim import FusedAdam
    model = _model(pretrained)
    with pytest.raises(TypeError, match="FusedAdam"):
        GraphedTrainStep(model, torch.nn.functional.mse_loss, optimizer=torch.optim.Adam(model.parameters(), lr=1e-3))
    with pytest.raises(ValueError, match="every trainable parameter"):
        GraphedTrainStep(model, torch.nn.functional.mse_loss, optimizer=FusedAdam(list(model.parameters())[:10]))
