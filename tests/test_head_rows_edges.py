"""The head's row-wise kernels at their launch and numeric edges: csrc/norm_kernels.hip (LayerNorm forward / backward),
csrc/linear_kernels.hip (split-row MFMA weight / bias gradient), csrc/elementwise_kernels.hip (the fused dropout sites)
and the reducer all three end in, quad::reduce_segments behind cgvp_bwd_reduce.  Fewer rows than a workgroup, second
grid-stride trips, ragged last splits, NULL gamma / beta, no rows, constant rows, a large common offset, eps = 0,
non-finite rows, exact integer data for the MFMA tile / lane mapping, the dropout mask pinned bit for bit to the g++
build of csrc/gvp_rng.h, and the host checks of every entry point."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import REPO
from gvp_hip import _lib, head_ops, ops
from gvp_hip.ops import _ptr, _stream

DEV = "cuda:0"
NAN = float("nan")
CANARY = -12345.5
F32 = np.float32


# ------------------------------------------------------------------------------------------------ host checks (no GPU)
def test_head_entry_points_check_their_arguments_on_the_host():
    """Every bad-argument case is answered with a CGVP_ERR_* code by checks that precede the launch: no GPU is needed (or
    touched) and the pointers are never dereferenced.  The accepted calls ask for zero rows where that launches nothing
    (not cgvp_layer_norm_bwd / cgvp_linear_wgrad: their rows == 0 path zero-fills the output with a kernel)."""
    L = _lib.lib()
    BAD, UNSUP, p = -1, -2, 0x1000
    nan, inf = float("nan"), float("inf")

    fwd = lambda x=p, gamma=p, beta=p, rows=8, dim=128, eps=1e-5, y=p, mean=p, rstd=p: \
        L.cgvp_layer_norm_fwd(x, gamma, beta, rows, dim, eps, y, mean, rstd, None)
    for dim in (0, 32, 96, 100, 192, 1024, -128):
        assert fwd(dim=dim) == UNSUP and fwd(dim=dim, rows=0) == UNSUP, dim
    for kw in (dict(rows=-1), dict(eps=-1e-5), dict(eps=nan), dict(eps=-inf), dict(rows=0, eps=-1.0), dict(x=0), dict(y=0),
               dict(mean=0), dict(rstd=0)):
        assert fwd(**kw) == BAD, kw
    for dim in (64, 128, 256, 512):
        assert fwd(rows=0, dim=dim) == 0 and fwd(rows=0, dim=dim, eps=0.0, x=0, y=0, mean=0, rstd=0) == 0, dim

    bwd = lambda gy=p, x=p, mean=p, rstd=p, gamma=p, rows=8, dim=128, gx=p, ws=p, out=p: \
        L.cgvp_layer_norm_bwd(gy, x, mean, rstd, gamma, rows, dim, gx, ws, out, None)
    for dim in (0, 32, 96, 1024, -64):
        assert bwd(dim=dim) == UNSUP, dim
    for kw in (dict(rows=-1), dict(out=0), dict(gy=0), dict(x=0), dict(mean=0), dict(rstd=0), dict(gx=0), dict(ws=0)):
        assert bwd(**kw) == BAD, kw

    ln_ws = L.cgvp_layer_norm_bwd_workspace_floats
    assert ln_ws(8, 96) == UNSUP and ln_ws(8, 0) == UNSUP and ln_ws(-1, 128) == BAD
    for dim in (64, 128, 256, 512):
        sizes = [ln_ws(R, dim) for R in (0, 1, 7, 8, 9, 32, 33, 255, 256, 4096, 16384, 16385, 16425, 1 << 20, 1 << 33)]
        for n in sizes:                                   # whole slab rows [d gamma | d beta], at most 512 of them
            assert n > 0 and n % (2 * dim) == 0 and n // (2 * dim) <= 512, (dim, n)
        assert sizes == sorted(sizes), (dim, sizes)

    lin = lambda x=p, gy=p, R=8, I=64, O=128, ws=p, out=p: L.cgvp_linear_wgrad(x, gy, R, I, O, ws, out, None)
    lin_ws = L.cgvp_linear_wgrad_workspace_floats
    for kw in (dict(I=0), dict(I=8), dict(I=24), dict(I=272), dict(I=-16), dict(O=0), dict(O=32), dict(O=96), dict(O=-64),
               dict(R=-1)):
        assert lin(**kw) == UNSUP, kw
        assert lin_ws(kw.get("R", 8), kw.get("I", 64), kw.get("O", 128)) == UNSUP, kw
    for kw in (dict(out=0), dict(ws=0), dict(x=0), dict(gy=0), dict(x=p + 4), dict(gy=p + 4), dict(ws=p + 4), dict(x=p + 8),
               dict(R=0, x=0, gy=0, out=0), dict(R=0, x=0, gy=0, ws=0), dict(R=0, ws=p + 4)):
        assert lin(**kw) == BAD, kw
    for I, O in ((16, 64), (64, 128), (256, 384), (144, 64)):
        sizes = [lin_ws(R, I, O) for R in (0, 1, 4, 63, 64, 65, 129, 4096, 8129, 8193, 19200, 1 << 20, 1 << 33)]
        for n in sizes:                                   # whole slab rows [d W | d b], at most 128 of them
            assert n > 0 and n % (O * I + O) == 0 and n // (O * I + O) <= 128, (I, O, n)
        assert sizes == sorted(sizes), (I, O, sizes)

    rng = lambda prob=0.25, seed=p, stream=3: C.byref(_lib.Rng(seed, prob, stream))
    sites = {
        "add": lambda a=p, rng=None, rows=8, dim=64, out=p, x=p: L.cgvp_dropout_add(a, x, rng, rows, dim, out, None),
        "scale": lambda a=p, rng=None, rows=8, dim=64, out=p: L.cgvp_dropout_scale(a, rng, rows, dim, out, None),
        "act": lambda a=p, rng=None, rows=8, dim=64, out=p, slope=0.01: L.cgvp_act_dropout_fwd(a, rng, slope, rows, dim, out, None),
        "act_bwd": lambda a=p, rng=None, rows=8, dim=64, out=p, slope=0.01, y=p:
            L.cgvp_act_dropout_bwd(a, y, rng, slope, rows, dim, out, None),
    }
    for name, f in sites.items():
        for dim in (4, 12, 60, 130):
            assert f(dim=dim) == UNSUP and f(dim=dim, rows=0) == UNSUP, (name, dim)
        for kw in (dict(dim=0), dict(dim=-8), dict(rows=-1), dict(a=0), dict(out=0), dict(a=p + 4), dict(out=p + 4),
                   dict(a=p + 8), dict(rows=0, out=p + 4), dict(rng=rng(1.0)), dict(rng=rng(1.5)), dict(rng=rng(-0.1)),
                   dict(rng=rng(nan)), dict(rng=rng(seed=p + 4)), dict(rows=0, rng=rng(1.0))):
            assert f(**kw) == BAD, (name, kw)
        assert f(rows=0) == 0 and f(rows=0, a=0, out=0) == 0 and f(rows=0, rng=rng()) == 0, name
        assert f(rows=0, rng=rng(0.0)) == 0 and f(rows=0, rng=rng(1.0, seed=0)) == 0, name    # no seed: no dropout, p unread
    assert sites["add"](x=p + 4) == BAD and sites["add"](rows=0, x=p + 4) == BAD and sites["add"](rows=0, x=0) == 0
    assert sites["act_bwd"](y=0) == BAD and sites["act_bwd"](y=p + 4) == BAD
    # the backward takes act' from the sign of the saved output, which is the sign of t only for a finite slope >= 0
    for name in ("act", "act_bwd"):
        for slope in (-0.1, -1e-30, nan, inf, -inf):
            assert sites[name](slope=slope) == BAD and sites[name](slope=slope, rows=0) == BAD, (name, slope)
        for slope in (0.0, 0.01, 1.0, 3.0):
            assert sites[name](slope=slope, rows=0) == 0, (name, slope)

    segs = (_lib.Segment * (_lib_max_segs() + 1))()
    red = lambda segs=segs, n=1, grad=p, ow=1: L.cgvp_bwd_reduce(segs, n, grad, ow, None)
    for kw in (dict(segs=None), dict(n=-1), dict(n=_lib_max_segs() + 1), dict(grad=0), dict(n=0, grad=0), dict(n=0, segs=None)):
        assert red(**kw) == BAD, kw


def _lib_max_segs():
    """CGVP_MAX_SEGS of include/caster_gvp.h"""
    import re
    text = open(os.path.join(REPO, "include", "caster_gvp.h")).read()
    return int(re.search(r"#define\s+CGVP_MAX_SEGS\s+(\d+)", text).group(1))


def test_slope_of_a_negative_leaky_relu_is_not_taken_by_the_fused_site():
    nn = torch.nn
    assert head_ops._slope(nn.ReLU()) == 0.0 and head_ops._slope(torch.relu) == 0.0
    assert head_ops._slope(nn.LeakyReLU(0.01)) == 0.01 and head_ops._slope(nn.LeakyReLU(0.0)) == 0.0
    for slope in (-0.1, -1e-30, float("nan"), float("inf"), -float("inf")):
        assert head_ops._slope(nn.LeakyReLU(slope)) is None, slope
    assert head_ops._slope(nn.GELU()) is None


# ------------------------------------------------------------------------------------------------ summation orders
def _seq_sum(a):
    """reduce_segments_rows_kernel (segment lists of at most 32 rows): s = 0; s += row r, r ascending.  a [rows, cols] fp32"""
    s = np.zeros(a.shape[1], F32)
    for r in range(a.shape[0]):
        s = s + a[r]
    return s


def _grouped_sum(a, RG=16):
    """reduce_segments_kernel (lists with a segment of more than 32 rows): row group rg takes rows rg, rg + 16, ...; four
    interleaved partial sums while four rows remain, the rest into the first; (s0 + s1) + (s2 + s3); the 16 groups in order."""
    rows, cols = a.shape
    tt = np.zeros(cols, F32)
    for rg in range(RG):
        s = [np.zeros(cols, F32) for _ in range(4)]
        r = rg
        while r + 3 * RG < rows:
            for k in range(4):
                s[k] = s[k] + a[r + k * RG]
            r += 4 * RG
        while r < rows:
            s[0] = s[0] + a[r]
            r += RG
        tt = tt + ((s[0] + s[1]) + (s[2] + s[3]))
    return tt


# ------------------------------------------------------------------------------------------------ LayerNorm
LN_EPS = 1e-5
CONSTANTS = (0.0, 1.0, -3.0, 0.1, 1.0 / 3.0, 1e-3, 1000.7, -2.5e6, 7.0, 1e-20, -65504.0)     # most are no power of two
LN_CASES = {f"{rows}x{dim}": (rows, dim, LN_EPS, "randn") for dim in (64, 128, 256, 512) for rows in (1, 7, 8, 9, 33)}
LN_CASES.update({
    # forward: ceil(32777 / 8) = 4098 workgroups > the cap of 4096 -> rows 32768.. are a second, partial trip
    "fwd_second_trip_32777x64": (32768 + 9, 64, LN_EPS, "randn"),
    # backward: ceil(16425 / 32) = 514 > the cap of 512 workgroups -> waves take 5 rows or 4 (16425 = 4 * 4096 + 41)
    "bwd_capped_uneven_16425x64": (16384 + 41, 64, LN_EPS, "randn"),
    "constant_rows_33x128": (33, 128, LN_EPS, "const"),
    "offset_1000_33x128": (33, 128, LN_EPS, "offset"),
    "eps_zero_33x128": (33, 128, 0.0, "randn"),
})
LN_OUT = ("y", "mean", "rstd", "gx", "g_gamma", "g_beta")
LN_FACTOR = 2.0          # e_ours <= max(LN_FACTOR e_stock, 2e-6 scale): the bound of test_layer_norm_kernels_vs_torch, in every case


@functools.lru_cache(maxsize=None)
def _ln_inputs(case):
    """(x, gamma, beta, d y) fp32 on the CPU, seeded; shared by the CPU and the GPU tests, never modified"""
    rows, dim, _, kind = LN_CASES[case]
    g = torch.Generator().manual_seed(1000 * dim + rows)
    x = torch.randn(rows, dim, generator=g)
    if kind == "randn":
        x = x * 2.0 + 0.5
    elif kind == "offset":
        x = x + 1000.0
    else:
        x = torch.tensor([CONSTANTS[r % len(CONSTANTS)] for r in range(rows)])[:, None].expand(rows, dim).contiguous()
    w = torch.randn(dim, generator=g) * 0.3 + 1.0
    b = torch.randn(dim, generator=g) * 0.1
    gy = torch.randn(rows, dim, generator=g)
    return x, w, b, gy


def _ln_fp64(x, w, b, eps, gy):
    """fp64 arithmetic on the fp32 inputs -> {name: tensor} of LN_OUT"""
    x, w, b, gy = x.double(), w.double(), b.double(), gy.double()
    mean = x.mean(1, keepdim=True)
    rstd = ((x - mean) ** 2).mean(1, keepdim=True).add(eps).rsqrt()
    xh = (x - mean) * rstd
    a = gy * w
    gx = rstd * (a - a.mean(1, keepdim=True) - xh * (a * xh).mean(1, keepdim=True))
    return dict(y=xh * w + b, mean=mean[:, 0], rstd=rstd[:, 0], gx=gx, g_gamma=(gy * xh).sum(0), g_beta=gy.sum(0))


@functools.lru_cache(maxsize=None)
def _ln_ref(case):
    return _ln_fp64(*_ln_inputs(case)[:3], LN_CASES[case][2], _ln_inputs(case)[3])


def _ln_stock(x, w, b, eps, gy):
    """torch's fp32 kernels on the device of the operands"""
    D = x.shape[1]
    y, mean, rstd = torch.native_layer_norm(x, [D], w, b, eps)
    gx, gw, gb = torch.ops.aten.native_layer_norm_backward(gy, x, [D], mean, rstd, w, b, [True, True, True])
    return dict(y=y, mean=mean.reshape(-1), rstd=rstd.reshape(-1), gx=gx, g_gamma=gw, g_beta=gb)


def _ln_ours(x, w, b, eps, gy):
    x, w, b, gy = (t.to(DEV) for t in (x, w, b, gy))
    y, mean, rstd = torch.ops.caster_gvp.layer_norm(x, w, b, eps)
    gx, gwb = torch.ops.caster_gvp.layer_norm_backward(gy, x, mean, rstd, w)
    torch.cuda.synchronize()
    D = x.shape[1]
    return dict(y=y, mean=mean, rstd=rstd, gx=gx, g_gamma=gwb[:D], g_beta=gwb[D:])


def _ln_within(ours, stock, ref, factor, what):
    bad = []
    for name in LN_OUT:
        f = ref[name]
        scale = float(f.abs().max()) if f.numel() else 0.0
        e_ours = float((ours[name].double().cpu() - f).abs().max()) if f.numel() else 0.0
        e_stock = float((stock[name].double().cpu() - f).abs().max()) if f.numel() else 0.0
        print(f"{what} {name}: e_ours {e_ours:.3e} e_stock {e_stock:.3e} ratio {e_ours / max(e_stock, 1e-300):.2f} scale {scale:.3e}")
        if not e_ours <= max(factor * e_stock, 2e-6 * scale):
            bad.append((name, e_ours, e_stock, scale))
    assert not bad, (what, bad)


def _fma(a, b, c):
    """fmaf on fp32 arrays: the product of two fp32 values is exact in fp64"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _wave_sum(v):
    """the 64-lane xor butterfly of wave_sum(): v [rows, 64] fp32 -> every lane's total (identical in all lanes)"""
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ off]
    return v[:, :1]


def _ln_emulation(x, w, b, eps, gy):
    """What csrc/norm_kernels.hip is documented to compute, in NumPy fp32: lane l holds columns l, 64 + l, ...; two-pass mean
    and variance (lane-serial partial sums, then the butterfly), rstd = 1 / sqrtf(var + eps), y = fmaf(xhat, gamma, beta);
    backward with that mean / rstd, d gamma / d beta per wave over its grid-stride rows, then the 8 waves of a workgroup,
    then the workgroups in quad::reduce_segments' order."""
    x, w, b, gy = (t.numpy().astype(F32) for t in (x, w, b, gy))
    rows, D = x.shape
    V, inv_d = D // 64, F32(1.0 / D)
    lanes = lambda t: t.reshape(rows, V, 64)
    xv = lanes(x)
    s = np.zeros((rows, 64), F32)
    for k in range(V):
        s = s + xv[:, k]
    mean = _wave_sum(s) * inv_d                                             # [rows, 1]
    q = np.zeros((rows, 64), F32)
    for k in range(V):
        d = xv[:, k] - mean
        q = _fma(d, d, q)
    rstd = F32(1.0) / np.sqrt(_wave_sum(q) * inv_d + F32(eps))
    xh = (x - mean) * rstd
    y = _fma(xh, w[None], b[None])
    a = gy * w[None]
    s1, s2 = np.zeros((rows, 64), F32), np.zeros((rows, 64), F32)
    for k in range(V):
        s1 = s1 + lanes(a)[:, k]
        s2 = _fma(lanes(a)[:, k], lanes(xh)[:, k], s2)
    s1, s2 = _wave_sum(s1) * inv_d, _wave_sum(s2) * inv_d
    gx = rstd * (a - s1 - xh * s2)
    G = min(512, max(1, (rows + 31) // 32))                                 # grid_for(): >= 4 rows per wave, 512 at the most
    slots = G * 8
    trips = (rows + slots - 1) // slots
    pad = lambda t: np.concatenate([t, np.zeros((trips * slots - rows, D), F32)]).reshape(trips, slots, D)
    dg, db = np.zeros((slots, D), F32), np.zeros((slots, D), F32)
    for dy_t, xh_t in zip(pad(gy), pad(xh)):
        dg, db = _fma(dy_t, xh_t, dg), db + dy_t
    out = []
    for part in (dg, db):
        part = part.reshape(G, 8, D)
        wg = np.zeros((G, D), F32)
        for ww in range(8):
            wg = wg + part[:, ww]
        out.append(_seq_sum(wg) if G <= 32 else _grouped_sum(wg))
    t = torch.from_numpy
    return dict(y=t(y), mean=t(mean[:, 0].copy()), rstd=t(rstd[:, 0].copy()), gx=t(gx), g_gamma=t(out[0]), g_beta=t(out[1]))


def test_layer_norm_bounds_are_reachable_by_the_documented_arithmetic_cpu():
    """No GPU: the fp32 arithmetic the kernels are documented to do (_ln_emulation) stays within
    max(LN_FACTOR e_stock, 2e-6 scale) of fp64 on exactly the inputs of the GPU test below, e_stock being torch's own
    fp32 kernels -- so the GPU test's cap is one the kernels can meet."""
    for case, (rows, dim, eps, kind) in LN_CASES.items():
        x, w, b, gy = _ln_inputs(case)
        _ln_within(_ln_emulation(x, w, b, eps, gy), _ln_stock(x, w, b, eps, gy), _ln_ref(case), LN_FACTOR,
                   f"emulation {case}")


def _ln_abi(x, gamma, beta, eps, gy, rows, dim, tail=64):
    """Both LayerNorm entry points through the C ABI: inputs are the leading `rows` of buffers whose tails are NaN, every
    output is NaN-prefilled and followed by `tail` canary floats.  gamma / beta may be None (NULL).  -> the LN_OUT dict"""
    L = _lib.lib()

    def lead(t, n):
        buf = torch.full((n + 8 * dim,), NAN, device=DEV)
        buf[:n] = t.to(DEV).reshape(-1)[:n]
        return buf

    def out(n):
        buf = torch.full((n + tail,), NAN, device=DEV)
        buf[n:] = CANARY
        return buf

    xb, gyb = lead(x, rows * dim), lead(gy, rows * dim)
    g = None if gamma is None else gamma.to(DEV)
    b = None if beta is None else beta.to(DEV)
    y, mean, rstd, gx, gwb = out(rows * dim), out(rows), out(rows), out(rows * dim), out(2 * dim)
    ws = out(int(L.cgvp_layer_norm_bwd_workspace_floats(rows, dim)))
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    assert L.cgvp_layer_norm_fwd(p(xb), p(g), p(b), rows, dim, eps, p(y), p(mean), p(rstd), _stream()) == 0
    mb, rb = lead(mean, rows), lead(rstd, rows)
    assert L.cgvp_layer_norm_bwd(p(gyb), p(xb), p(mb), p(rb), p(g), rows, dim, p(gx), p(ws), p(gwb), _stream()) == 0
    torch.cuda.synchronize()
    for name, buf, n in (("y", y, rows * dim), ("mean", mean, rows), ("rstd", rstd, rows), ("gx", gx, rows * dim),
                         ("gwb", gwb, 2 * dim), ("workspace", ws, ws.numel() - tail)):
        assert (buf[n:] == CANARY).all(), f"{name}: written past its end"
    return dict(y=y[:rows * dim].view(rows, dim), mean=mean[:rows], rstd=rstd[:rows], gx=gx[:rows * dim].view(rows, dim),
                g_gamma=gwb[:dim], g_beta=gwb[dim:2 * dim])


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(LN_CASES))
def test_layer_norm_edges(case):
    """y, mean, rstd, d x, d gamma, d beta of caster_gvp::layer_norm / layer_norm_backward against fp64 on the same fp32
    inputs, no further from it than twice torch's own fp32 kernels (or 2e-6 of the tensor's scale); run to run bitwise;
    and the same bits through the C ABI into NaN-prefilled outputs (every row is written, by exactly one trip of the
    grid-stride loops) with nothing written past them and no NaN read from beyond the inputs.
    Measured on an MI355X, the largest e_ours / e_stock over the 25 cases: y 1.76 (33x128), mean 1.92 (7x512), gx 1.81 (1x64),
    d beta 1.20 (9x512); above 2 only under the 2e-6 scale floor (1x64: rstd 5.93 at e_ours 2.6e-8, d gamma 2.01 at 3.3e-7).
    x = 1000 + N(0, 1): y 1.02, mean 1.05, rstd 0.01, d x 0.84, d gamma 1.58, d beta 0.36 -- the factor 2 holds there too.
    32,777 rows: 0.95 / 0.94 / 0.92 / 0.98 / 0.74 / 1.09; 16,425 rows: 0.94 / 0.95 / 0.92 / 1.16 / 1.71 / 0.81."""
    rows, dim, eps, kind = LN_CASES[case]
    x, w, b, gy = _ln_inputs(case)
    ours, again = _ln_ours(x, w, b, eps, gy), _ln_ours(x, w, b, eps, gy)
    abi = _ln_abi(x, w, b, eps, gy, rows, dim)
    for name in LN_OUT:
        assert ours[name].shape == _ln_ref(case)[name].shape, name
        assert torch.equal(ours[name], again[name]), name
        assert torch.equal(ours[name], abi[name]), name
        assert torch.isfinite(ours[name]).all(), name
    stock = _ln_stock(*(t.to(DEV) for t in (x, w, b)), eps, gy.to(DEV))
    _ln_within(ours, stock, _ln_ref(case), LN_FACTOR, case)


@pytest.mark.gpu
def test_layer_norm_of_constant_rows():
    """Rows constant at c, most c no power of two: the lane sums and the butterfly only double, so mean == c and
    x - mean == 0 exactly -> y == beta bitwise (whatever rstd is), rstd = eps ** -0.5."""
    case = "constant_rows_33x128"
    rows, dim, eps, _ = LN_CASES[case]
    x, w, b, gy = _ln_inputs(case)
    ours = _ln_ours(x, w, b, eps, gy)
    assert torch.equal(ours["mean"].cpu(), x[:, 0])
    assert torch.equal(ours["y"].cpu(), b[None].expand(rows, dim))
    ref = _ln_ref(case)
    assert float((ref["rstd"] - eps ** -0.5).abs().max()) < 1e-9 and float(ref["y"].sub(b.double()).abs().max()) == 0
    stock = _ln_stock(*(t.to(DEV) for t in (x, w, b)), eps, gy.to(DEV))
    e_ours = float((ours["rstd"].double().cpu() - eps ** -0.5).abs().max())
    e_stock = float((stock["rstd"].double().cpu() - eps ** -0.5).abs().max())
    print(f"rstd of constant rows: e_ours {e_ours:.3e} e_stock {e_stock:.3e}")
    assert e_ours <= max(2.0 * e_stock, 2e-6 * eps ** -0.5)
    assert (ours["g_gamma"] == 0).all()                                    # xhat == 0 exactly


@pytest.mark.gpu
def test_layer_norm_keeps_a_non_finite_row_to_itself():
    """Row 5 all NaN, row 6 with one +inf: every other row's y, mean, rstd and d x is bitwise what the run with finite
    values in those two rows gives.  mean is NaN / +inf, rstd NaN, y and d x NaN in the two rows; d gamma = sum d y xhat is
    NaN in every column (xhat of both rows is NaN everywhere), d beta = sum d y does not see x at all."""
    rows, dim, eps = 33, 128, LN_EPS
    x, w, b, gy = _ln_inputs("eps_zero_33x128")
    clean = _ln_ours(x, w, b, eps, gy)
    bad = x.clone()
    bad[5] = NAN
    bad[6, 77] = float("inf")
    got, again = _ln_ours(bad, w, b, eps, gy), _ln_ours(bad, w, b, eps, gy)
    others = [r for r in range(rows) if r not in (5, 6)]
    for name in ("y", "mean", "rstd", "gx"):
        assert torch.equal(got[name][others], clean[name][others]), name
        assert torch.equal(got[name].nan_to_num(nan=7.0, posinf=8.0), again[name].nan_to_num(nan=7.0, posinf=8.0)), name
    assert torch.isnan(got["mean"][5]) and float(got["mean"][6]) == float("inf")
    assert torch.isnan(got["rstd"][5:7]).all()
    assert torch.isnan(got["y"][5:7]).all() and torch.isnan(got["gx"][5:7]).all()
    assert torch.isnan(got["g_gamma"]).all()
    assert torch.equal(got["g_beta"], clean["g_beta"])


@pytest.mark.gpu
def test_layer_norm_without_rows():
    for dim in (64, 512):
        x, w, b = torch.empty(0, dim, device=DEV), torch.ones(dim, device=DEV), torch.zeros(dim, device=DEV)
        y, mean, rstd = torch.ops.caster_gvp.layer_norm(x, w, b, LN_EPS)
        assert y.shape == (0, dim) and mean.shape == (0,) and rstd.shape == (0,)
        gx, gwb = torch.ops.caster_gvp.layer_norm_backward(x, x, mean, rstd, w)
        assert gx.shape == (0, dim) and gwb.shape == (2 * dim,) and (gwb == 0).all()
        # the C ABI: d gamma / d beta are STORED zeros, nothing else is touched
        out = torch.full((2 * dim + 64,), NAN, device=DEV)
        assert _lib.lib().cgvp_layer_norm_bwd(None, None, None, None, None, 0, dim, None, None, _ptr(out), _stream()) == 0
        torch.cuda.synchronize()
        assert (out[:2 * dim] == 0).all() and torch.isnan(out[2 * dim:]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("rows,dim", [(9, 128), (33, 64), (1, 512)])
def test_layer_norm_null_gamma_and_beta_through_the_c_abi(rows, dim):
    """gamma == NULL, beta == NULL and both: bitwise gamma = 1, beta = 0 (the canary and NaN-tail checks are _ln_abi's)."""
    g = torch.Generator().manual_seed(rows + dim)
    x, gy = torch.randn(rows, dim, generator=g) * 2 + 0.5, torch.randn(rows, dim, generator=g)
    w, b = torch.randn(dim, generator=g) * 0.3 + 1.0, torch.randn(dim, generator=g) * 0.1
    one, zero = torch.ones(dim), torch.zeros(dim)
    for gamma, beta, g_full, b_full in ((None, b, one, b), (w, None, w, zero), (None, None, one, zero)):
        got = _ln_abi(x, gamma, beta, LN_EPS, gy, rows, dim)
        want = _ln_abi(x, g_full, b_full, LN_EPS, gy, rows, dim)
        for name in LN_OUT:
            assert torch.isfinite(got[name]).all() and torch.equal(got[name], want[name]), (name, gamma is None, beta is None)
    ref = _ln_fp64(x, one, zero, LN_EPS, gy)
    for name in LN_OUT:
        scale = float(ref[name].abs().max())
        assert float((got[name].double().cpu() - ref[name]).abs().max()) <= 1e-5 * max(scale, 1.0), name


# ------------------------------------------------------------------------------------------------ linear weight gradient
WG_CASES = [(R, I, O) for R in (1, 2, 3, 4, 5, 63, 64, 65, 129) for I in (16, 64) for O in (64, 128)]
WG_CASES += [
    (8129, 64, 64),     # 128 splits of 64 rows: the last one holds row 8128 alone
    (8193, 64, 64),     # the workspace is sized for 128 splits, rows_per_split = 68 launches ceil(8193 / 68) = 121
    (8129, 16, 64), (8193, 16, 64),
    (65, 64, 384),
]
WG_CASES += [(65, I, 128) for I in (80, 96, 144, 160, 256)]      # both ends of every instantiation (I <= 80 / 144 / 256)
WG_CASES += [(65, I, 64) for I in (80, 144, 256)]


def _wg_launch(R, O):
    """(splits the workspace is sized for, rows per split, splits launched): the host arithmetic of cgvp_linear_wgrad"""
    s = max(1, min(256 // (O // 64), 128, (R + 63) // 64))
    rps = ((R + s - 1) // s + 3) // 4 * 4
    return s, rps, (R + rps - 1) // rps


def test_linear_wgrad_cases_reach_the_launch_edges_they_name():
    assert _wg_launch(8129, 64) == (128, 64, 128) and 8129 - 127 * 64 == 1
    assert _wg_launch(8193, 64) == (128, 68, 121)
    assert _wg_launch(3, 64) == (1, 4, 1) and _wg_launch(129, 128) == (3, 44, 3) and _wg_launch(65, 128) == (2, 36, 2)
    L = _lib.lib()
    for R, I, O in WG_CASES:                              # the workspace holds a slab row for every split that is launched
        assert L.cgvp_linear_wgrad_workspace_floats(R, I, O) // (O * I + O) >= _wg_launch(R, O)[2], (R, I, O)
    assert L.cgvp_linear_wgrad_workspace_floats(8193, 64, 64) // (64 * 64 + 64) > _wg_launch(8193, 64)[2]


def _wg_exact_operands(R, I, O):
    """x[r] one-hot at column (7 r + 3) % I times 1..3, gy[r][o] integers in -2..2: every partial sum is an integer of
    magnitude <= 6 R < 2^24, so fp32 in any order is exact.  -> x, gy (fp32), [d W | d b] flat from int64 arithmetic"""
    r, o = torch.arange(R)[:, None], torch.arange(O)[None]
    xi = torch.zeros(R, I, dtype=torch.int64)
    xi[torch.arange(R), (7 * torch.arange(R) + 3) % I] = 1 + torch.arange(R) % 3
    gi = (5 * r + 3 * o + (r * o) % 7) % 5 - 2
    want = torch.cat([(gi.t() @ xi).reshape(-1), gi.sum(0)])
    assert 6 * R < 1 << 24 and int(gi.min()) == -2 and int(gi.max()) == 2
    return xi.float(), gi.float(), want


@pytest.mark.gpu
@pytest.mark.parametrize("R,I,O", WG_CASES)
def test_linear_wgrad_edges(R, I, O):
    """Exact: one-hot / small-integer operands must give the int64 reference bit for bit, bias included (the tile and
    lane mapping, the ragged last chunk, a last split of one row, splits the workspace holds but the launch does not
    use).  Random: Gaussian operands under the bound of test_linear_wgrad_kernel_matches_torch.  Both run to run bitwise."""
    x, gy, want = _wg_exact_operands(R, I, O)
    x, gy = x.to(DEV), gy.to(DEV)
    out = torch.ops.caster_gvp.linear_wgrad(x, gy)
    assert out.shape == (O * I + O,)
    bad = (out.cpu().long() != want).nonzero().reshape(-1).tolist()
    assert not bad, ("first wrong flat indices", bad[:8], "of", len(bad))
    assert torch.equal(out.cpu(), want.float()) and torch.equal(out, torch.ops.caster_gvp.linear_wgrad(x, gy))
    gen = torch.Generator().manual_seed(R + I + O)
    x, gy = torch.randn(R, I, generator=gen).to(DEV), torch.randn(R, O, generator=gen).to(DEV)
    out = torch.ops.caster_gvp.linear_wgrad(x, gy)
    want_w, want_b = gy.double().t() @ x.double(), gy.double().sum(0)
    e_w, e_b = float((out[:O * I].view(O, I).double() - want_w).abs().max()), float((out[O * I:].double() - want_b).abs().max())
    s_w, s_b = max(1.0, float(want_w.abs().max())), max(1.0, float(want_b.abs().max()))
    m_w, m_b = float(((gy.t() @ x).double() - want_w).abs().max()), float((gy.sum(0).double() - want_b).abs().max())
    print(f"R {R} I {I} O {O}: d W e_ours {e_w:.3e} fp32 matmul {m_w:.3e} bound {2e-6 * s_w * R ** 0.5:.3e}; "
          f"d b e_ours {e_b:.3e} fp32 sum {m_b:.3e} bound {2e-6 * s_b * R ** 0.5:.3e}")
    assert e_w <= 2e-6 * s_w * R ** 0.5 and e_b <= 2e-6 * s_b * R ** 0.5
    assert torch.equal(out, torch.ops.caster_gvp.linear_wgrad(x, gy))


@pytest.mark.gpu
@pytest.mark.parametrize("R,I,O", [(5, 16, 64), (65, 64, 128), (129, 256, 64), (8129, 64, 64)])
def test_linear_wgrad_reads_no_row_beyond_the_last(R, I, O):
    """x and gy are the first R rows of buffers whose 64-row tails are NaN (one LDS chunk: all a chunk's fetch could
    reach): the output is finite and bitwise the output from exactly-sized buffers."""
    gen = torch.Generator().manual_seed(R)
    x, gy = torch.randn(R, I, generator=gen).to(DEV), torch.randn(R, O, generator=gen).to(DEV)
    xb, gb = torch.full((R + 64, I), NAN, device=DEV), torch.full((R + 64, O), NAN, device=DEV)
    xb[:R], gb[:R] = x, gy
    out = torch.ops.caster_gvp.linear_wgrad(xb[:R], gb[:R])
    assert xb[:R].data_ptr() == xb.data_ptr() and torch.isfinite(out).all()
    assert torch.equal(out, torch.ops.caster_gvp.linear_wgrad(x, gy))


@pytest.mark.gpu
def test_linear_wgrad_keeps_a_nan_to_its_column():
    """x[r0][i0] = NaN: exactly column i0 of d W is NaN (0 * NaN included); every other element and all of d b are
    bitwise what x[r0][i0] = 0 gives."""
    R, I, O, r0, i0 = 129, 64, 128, 70, 37
    gen = torch.Generator().manual_seed(4)
    x, gy = torch.randn(R, I, generator=gen).to(DEV), torch.randn(R, O, generator=gen).to(DEV)
    gy[r0, 5] = 0.0
    x[r0, i0] = 0.0
    clean = torch.ops.caster_gvp.linear_wgrad(x, gy)
    x[r0, i0] = NAN
    got = torch.ops.caster_gvp.linear_wgrad(x, gy)
    gw, cw = got[:O * I].view(O, I), clean[:O * I].view(O, I)
    col = torch.zeros(O, I, dtype=torch.bool, device=DEV)
    col[:, i0] = True
    assert torch.equal(torch.isnan(gw), col)
    assert torch.equal(gw[~col], cw[~col]) and torch.equal(got[O * I:], clean[O * I:])
    assert torch.isfinite(clean).all()


@pytest.mark.gpu
def test_linear_wgrad_without_rows_stores_zeros():
    L = _lib.lib()
    for I, O in ((16, 64), (256, 384)):
        n = O * I + O
        out = torch.full((n + 64,), NAN, device=DEV)
        ws = torch.empty(max(1, int(L.cgvp_linear_wgrad_workspace_floats(0, I, O))), device=DEV)
        assert L.cgvp_linear_wgrad(None, None, 0, I, O, _ptr(ws), _ptr(out), _stream()) == 0
        torch.cuda.synchronize()
        assert (out[:n] == 0).all() and torch.isnan(out[n:]).all()
        assert (torch.ops.caster_gvp.linear_wgrad(torch.empty(0, I, device=DEV), torch.empty(0, O, device=DEV)) == 0).all()


# ------------------------------------------------------------------------------------------------ fused dropout sites
@pytest.fixture(scope="module")
def host_rng(tmp_path_factory):
    """csrc/gvp_rng.h compiled with g++ (tests/host_math/host_rng.cpp; pinned to the published Philox known answers in
    tests/test_host_math.py)"""
    so = str(tmp_path_factory.mktemp("host_rng") / "host_rng.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-o", so,
                           os.path.join(REPO, "tests", "host_math", "host_rng.cpp")])
    return C.CDLL(so)


def _host_mask(lib, pair, site, rows, dim, p):
    """host_dropout_mask with the {seed, offset} pair read back from the device: columns 4 b .. 4 b + 3 of a row come from
    dropout4(row, b) = half b & 1 of dropout8_raw(row, b >> 1) -- the 8-column block the head's kernels draw at once."""
    seed, offset = (int(v) & (2 ** 64 - 1) for v in pair.cpu())
    out = np.zeros((rows, dim), F32)
    lib.host_dropout_mask(C.c_ulonglong(seed), C.c_ulonglong(offset), int(site), C.c_longlong(rows), int(dim), C.c_float(p),
                          out.ctypes.data_as(C.c_void_p))
    return torch.from_numpy(out)


def _pairs(n):
    state = head_ops._head_rng_state(torch.device(DEV))
    return [torch.ops.caster_gvp.rng_next(state) for _ in range(n)]


def _grad(y, leaf, g):
    return torch.autograd.grad(y, [leaf], g)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("rows,dim", [(5, 8), (33, 24), (64, 128), (9, 512), (7, 520)])
def test_head_dropout_mask_is_the_generator_of_the_encoders(rows, dim, host_rng):
    """The factors of every fused site -- read through a = 1 / t = 1 / g = 1 -- are bitwise cgvp_dropout_masks' and the
    g++ build's of csrc/gvp_rng.h for the same {seed, offset}, stream id = site, row and 8-column block."""
    p = 0.3
    none = torch.empty(0, device=DEV)
    seen = []
    for pair in _pairs(2):
        for site in (1, 2, 37):
            want = ops.dropout_masks(pair, p, site, 1, rows, dim)[0]
            assert torch.equal(want.cpu(), _host_mask(host_rng, pair, site, rows, dim, p)), site
            vals = set(want.unique().tolist())
            assert vals <= {0.0, float(np.float32(1) / (np.float32(1) - np.float32(p)))}, vals
            ones = torch.ones(rows, dim, device=DEV, requires_grad=True)
            y_add = torch.ops.caster_gvp.dropout_add(ones, none, pair, site, p)
            y_act = torch.ops.caster_gvp.act_dropout(ones, pair, site, p, 0.01)
            got = {"dropout_add": y_add, "act_dropout": y_act,
                   "d dropout_add": _grad(y_add, ones, torch.ones_like(y_add)),
                   "d act_dropout": _grad(y_act, ones, torch.ones_like(y_act)),
                   "dropout_scale": torch.ops.caster_gvp.dropout_scale(ones.detach(), pair, site, p),
                   "dropout_add with x": torch.ops.caster_gvp.dropout_add(ones.detach(), torch.zeros(rows, dim, device=DEV), pair, site, p)}
            for name, t in got.items():
                assert torch.equal(t.detach(), want), (name, site)
            seen.append(want)
    if rows * dim >= 256:
        assert all(not torch.equal(seen[i], seen[j]) for i in range(len(seen)) for j in range(i))


def _ulp_bound(*terms):
    """2^-23 (|a| + |b| + ...): one fused or two separate fp32 roundings of a result made of these terms"""
    return 2.0 ** -23 * sum(t.abs() for t in terms)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,dim,p", [(33, 24, 0.1), (64, 128, 0.5), (7, 520, 0.25)])
def test_fused_dropout_arithmetic_vs_fp64(rows, dim, p):
    """Outputs and gradients of the four kernels against fp64 under the pinned mask f: per element within
    2^-23 (|x| + |a f|) (one fused or two separate roundings), exact zeros where f = 0, d x == g."""
    (pair,) = _pairs(1)
    site = 5
    f = ops.dropout_masks(pair, p, site, 1, rows, dim)[0]
    fd, zero = f.double(), f == 0
    assert 0 < int(zero.sum()) < rows * dim
    gen = torch.Generator().manual_seed(rows)
    a, x, g, t = (torch.randn(rows, dim, generator=gen).to(DEV) for _ in range(4))
    al, xl = a.clone().requires_grad_(), x.clone().requires_grad_()
    y = torch.ops.caster_gvp.dropout_add(al, xl, pair, site, p)
    ga, gx = torch.autograd.grad(y, [al, xl], g)
    assert ((y.double() - (x.double() + a.double() * fd)).abs() <= _ulp_bound(x.double(), a.double() * fd)).all()
    assert torch.equal(y[zero], x[zero]) and torch.equal(gx, g)
    assert ((ga.double() - g.double() * fd).abs() <= _ulp_bound(g.double() * fd)).all() and (ga[zero] == 0).all()
    assert torch.equal(torch.ops.caster_gvp.dropout_scale(g, pair, site, p), ga)
    only = torch.ops.caster_gvp.dropout_add(a, torch.empty(0, device=DEV), pair, site, p)
    assert ((only.double() - a.double() * fd).abs() <= _ulp_bound(a.double() * fd)).all() and (only[zero] == 0).all()
    for slope in (0.0, 0.01, 1.0, 2.5):
        s = float(np.float32(slope))                                     # the kernel's argument is a float
        tl = t.clone().requires_grad_()
        y = torch.ops.caster_gvp.act_dropout(tl, pair, site, p, slope)
        gt = _grad(y, tl, g)
        act = torch.where(t > 0, t.double(), t.double() * s)
        dact = torch.where(t > 0, torch.ones_like(fd), torch.full_like(fd, s))
        assert ((y.double() - act * fd).abs() <= _ulp_bound(act * fd)).all(), slope
        assert ((gt.double() - g.double() * fd * dact).abs() <= _ulp_bound(g.double() * fd * dact)).all(), slope
        assert (y[zero] == 0).all() and (gt[zero] == 0).all(), slope
    # p = 0: the identity, bitwise, whatever the pair
    assert torch.equal(torch.ops.caster_gvp.dropout_add(a, x, pair, site, 0.0), x + a)
    assert torch.equal(torch.ops.caster_gvp.dropout_scale(g, pair, site, 0.0), g)
    assert torch.equal(torch.ops.caster_gvp.act_dropout(t, pair, site, 0.0, 0.01), torch.nn.functional.leaky_relu(t, 0.01))


@pytest.mark.gpu
def test_act_dropout_at_zeros_the_smallest_normal_and_negative_values():
    """t holding +0.0, -0.0, +- the smallest normal float, negative and positive values, slopes 0 and 0.01: the forward is
    bitwise leaky_relu(t) * f of the stock ops, the gradient is autograd's (bitwise where act' is 0 or 1; within one
    rounding where it is the slope: stock rounds (g f) slope, the kernel g (f slope))."""
    rows, dim, p, site = 16, 64, 0.3, 9
    (pair,) = _pairs(1)
    f = ops.dropout_masks(pair, p, site, 1, rows, dim)[0]
    tiny = float(np.finfo(np.float32).tiny)
    special = torch.tensor([0.0, -0.0, tiny, -tiny, -1.0, 1.0, -3.5e-3, 2.5e4, -7e20, 1e-30, -1e-30, 0.5, -0.5])
    gen = torch.Generator().manual_seed(2)
    t = special[torch.randint(len(special), (rows, dim), generator=gen)].to(DEV)
    g = torch.randn(rows, dim, generator=gen).to(DEV)
    for v in (0.0, tiny, -tiny, -1.0):
        assert ((t == v) & (f > 0)).any() and ((t == v) & (f == 0)).any()
    assert (torch.signbit(t) & (t == 0)).any() and (~torch.signbit(t) & (t == 0)).any()
    for slope in (0.0, 0.01):
        tl, ts = t.clone().requires_grad_(), t.clone().requires_grad_()
        y = torch.ops.caster_gvp.act_dropout(tl, pair, site, p, slope)
        y_stock = torch.nn.functional.leaky_relu(ts, slope) * f
        gt, gt_stock = _grad(y, tl, g), _grad(y_stock, ts, g)
        assert torch.equal(y, y_stock.detach()), slope
        exact = (t > 0) | (f == 0) | torch.tensor(slope == 0.0, device=DEV)
        assert torch.equal(gt[exact], gt_stock[exact]), slope
        assert ((gt.double() - gt_stock.double()).abs() <= _ulp_bound(gt_stock.double())).all(), slope


@pytest.mark.gpu
def test_fused_dropout_second_grid_stride_trip(host_rng):
    """rows x dim / 8 = 8200 x 128 = 1,049,600 eight-column blocks > 4096 workgroups x 256 threads = 1,048,576: the last 1,024
    blocks (rows 8192..) are a second trip.  The mask is the host generator's and y = x + a f holds over the whole tensor."""
    rows, dim, p, site = 8200, 1024, 0.2, 2
    assert rows * (dim // 8) > 4096 * 256 and (rows - 8) * (dim // 8) <= 4096 * 256
    (pair,) = _pairs(1)
    ones = torch.ones(rows, dim, device=DEV)
    f = torch.ops.caster_gvp.dropout_add(ones, torch.empty(0, device=DEV), pair, site, p)
    assert torch.equal(f.cpu(), _host_mask(host_rng, pair, site, rows, dim, p))
    assert torch.equal(f, torch.ops.caster_gvp.dropout_scale(ones, pair, site, p))
    assert torch.equal(f, torch.ops.caster_gvp.act_dropout(ones, pair, site, p, 0.0))
    gen = torch.Generator(device=DEV).manual_seed(8)
    a, x = torch.randn(rows, dim, device=DEV, generator=gen), torch.randn(rows, dim, device=DEV, generator=gen)
    y = torch.ops.caster_gvp.dropout_add(a, x, pair, site, p)
    af = a.double() * f.double()
    assert ((y.double() - (x.double() + af)).abs() <= _ulp_bound(x.double(), af)).all()
    assert torch.equal(y[f == 0], x[f == 0])


@pytest.mark.gpu
@pytest.mark.parametrize("rows,dim", [(7, 520), (1, 8), (33, 24)])
def test_fused_dropout_through_the_c_abi(rows, dim):
    """Inputs are the leading rows of NaN-tailed buffers, outputs are NaN-prefilled and followed by 64 canary floats: the
    ops' bits, no NaN, the canary survives.  A NULL rng is the identity, bitwise."""
    L = _lib.lib()
    p, site, slope, n = 0.25, 4, 0.01, rows * dim
    (pair,) = _pairs(1)
    gen = torch.Generator().manual_seed(n)
    a, x, g, t = (torch.randn(rows, dim, generator=gen).to(DEV) for _ in range(4))

    def lead(src):
        buf = torch.full((n + 1024,), NAN, device=DEV)
        buf[:n] = src.reshape(-1)
        return buf

    def out():
        buf = torch.full((n + 64,), NAN, device=DEV)
        buf[n:] = CANARY
        return buf

    ptr = lambda buf: C.c_void_p(buf.data_ptr())
    y_act = torch.ops.caster_gvp.act_dropout(t, pair, site, p, slope)
    la, lx, lg, lt, ly = (lead(src) for src in (a, x, g, t, y_act))
    for rng, p_op in ((C.byref(_lib.Rng(pair.data_ptr(), p, site)), p), (None, 0.0)):
        calls = {
            "dropout_add": (lambda o: L.cgvp_dropout_add(ptr(la), ptr(lx), rng, rows, dim, ptr(o), _stream()),
                            torch.ops.caster_gvp.dropout_add(a, x, pair, site, p_op)),
            "dropout_add, no x": (lambda o: L.cgvp_dropout_add(ptr(la), None, rng, rows, dim, ptr(o), _stream()),
                                  torch.ops.caster_gvp.dropout_add(a, torch.empty(0, device=DEV), pair, site, p_op)),
            "dropout_scale": (lambda o: L.cgvp_dropout_scale(ptr(lg), rng, rows, dim, ptr(o), _stream()),
                              torch.ops.caster_gvp.dropout_scale(g, pair, site, p_op)),
            "act_dropout": (lambda o: L.cgvp_act_dropout_fwd(ptr(lt), rng, slope, rows, dim, ptr(o), _stream()),
                            torch.ops.caster_gvp.act_dropout(t, pair, site, p_op, slope)),
            "act_dropout_bwd": (lambda o: L.cgvp_act_dropout_bwd(ptr(lg), ptr(ly), rng, slope, rows, dim, ptr(o), _stream()),
                                torch.ops.caster_gvp.act_dropout_backward(g, y_act, pair, site, p_op, slope)),
        }
        for name, (call, want) in calls.items():
            o = out()
            assert call(o) == 0, name
            torch.cuda.synchronize()
            assert torch.isfinite(o[:n]).all() and torch.equal(o[:n].view(rows, dim), want), (name, rng is None)
            assert (o[n:] == CANARY).all(), name
        if rng is None:
            assert torch.equal(calls["dropout_add"][1], x + a) and torch.equal(calls["dropout_add, no x"][1], a)
            assert torch.equal(calls["dropout_scale"][1], g)
            assert torch.equal(calls["act_dropout"][1], torch.nn.functional.leaky_relu(t, slope))


@pytest.mark.gpu
def test_drop_sites_leave_a_negative_leaky_relu_slope_to_the_stock_ops():
    """nn.LeakyReLU(-0.1): y > 0 is no longer t > 0, so the fused backward (act' from the sign of the saved output) would
    return g f where autograd returns g f slope.  DropSites.act_dropout must give the stock outputs and gradients (the
    same torch generator state -> the same mask), and the op itself refuses such a slope."""
    rows, dim, p = 300, 64, 0.2
    gen = torch.Generator().manual_seed(6)
    t, g = torch.randn(rows, dim, generator=gen).to(DEV), torch.randn(rows, dim, generator=gen).to(DEV)
    drop = torch.nn.Dropout(p).train()
    for act in (torch.nn.LeakyReLU(-0.1), torch.nn.LeakyReLU(0.01)):
        sites = head_ops.DropSites(t, True, p)
        assert sites.active
        tl, ts = t.clone().requires_grad_(), t.clone().requires_grad_()
        torch.manual_seed(77)
        y = sites.act_dropout(tl, act, drop)
        torch.manual_seed(77)
        y_stock = drop(act(ts))
        gt, gt_stock = _grad(y, tl, g), _grad(y_stock, ts, g)
        if act.negative_slope < 0:
            assert sites.site == 0                                       # no fused site was taken
            assert torch.equal(y, y_stock) and torch.equal(gt, gt_stock)
            assert (y[t < 0] > 0).sum() > 1000                           # the case exists: negative t, positive output
        else:
            assert sites.site == 1 and not torch.equal(y, y_stock)      # the fused site draws its own mask
            f = ops.dropout_masks(sites.pair, p, 1, 1, rows, dim)[0]
            assert torch.equal(y, torch.nn.functional.leaky_relu(t, 0.01) * f)
    (pair,) = _pairs(1)
    with pytest.raises(ValueError, match="cgvp_act_dropout_fwd"):
        torch.ops.caster_gvp.act_dropout(t, pair, 1, p, -0.1)
    with pytest.raises(ValueError, match="cgvp_act_dropout_bwd"):
        torch.ops.caster_gvp.act_dropout_backward(g, t, pair, 1, p, -0.1)


# ------------------------------------------------------------------------------------------------ cgvp_bwd_reduce
def _reduce(specs, grad, overwrite):
    """specs: [(slab tensor [rows, stride] on the GPU, col0, len, dst)] -> rc of one cgvp_bwd_reduce over all of them"""
    segs = (_lib.Segment * max(1, len(specs)))()
    for sg, (slab, col0, ln, dst) in zip(segs, specs):
        sg.slab, sg.rows, sg.stride, sg.col0, sg.len, sg.dst = slab.data_ptr(), slab.shape[0], slab.shape[1], col0, ln, dst
    rc = _lib.lib().cgvp_bwd_reduce(segs, len(specs), _ptr(grad), overwrite, _stream())
    torch.cuda.synchronize()
    return rc


def _int_slab(rows, stride, k):
    r, c = torch.arange(rows)[:, None], torch.arange(stride)[None]
    return ((3 * r + 5 * c + (r * c) % 11 + k) % 7 - 3).float()


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [1, 2, 32, 33, 37, 240])
def test_bwd_reduce_one_segment(rows):
    """Small-integer slabs (sums exact in any order): both kernels (rows <= 32 / > 32), lengths around the 64- and
    256-column blocks, stride > col0 + len, non-zero col0 and dst; overwrite stores into a NaN-prefilled destination
    and leaves what no segment covers NaN, add mode adds to what is there."""
    for ln in (1, 63, 64, 65, 257):
        col0, dst = 3, 11
        stride = col0 + ln + 6
        slab = _int_slab(rows, stride, ln)
        slab[:, :col0], slab[:, col0 + ln:] = 1000.0, 1000.0              # a column outside [col0, col0 + len) would show
        want = slab[:, col0:col0 + ln].long().sum(0).float()
        grad = torch.full((dst + ln + 9,), NAN, device=DEV)
        assert _reduce([(slab.to(DEV), col0, ln, dst)], grad, 1) == 0
        assert torch.equal(grad[dst:dst + ln].cpu(), want), (rows, ln)
        assert torch.isnan(grad[:dst]).all() and torch.isnan(grad[dst + ln:]).all(), (rows, ln)
        base = (torch.arange(dst + ln + 9) % 13 - 6).float()
        grad = base.to(DEV)
        assert _reduce([(slab.to(DEV), col0, ln, dst)], grad, 0) == 0
        base[dst:dst + ln] += want
        assert torch.equal(grad.cpu(), base), (rows, ln)
        assert _reduce([], grad, 1) == 0 and _reduce([], grad, 0) == 0 and torch.equal(grad.cpu(), base)      # nsegs = 0


def _seg_list(rows_of, len_of, n, gaussian):
    """n segments with their own slabs, disjoint destinations with a gap of 2 between them"""
    gen = torch.Generator().manual_seed(n)
    specs, dst = [], 1
    for i in range(n):
        rows, ln, col0 = rows_of(i), len_of(i), i % 5
        stride = col0 + ln + 1 + i % 3
        slab = torch.randn(rows, stride, generator=gen) if gaussian else _int_slab(rows, stride, i)
        specs.append((slab, col0, ln, dst))
        dst += ln + 2
    return specs, dst


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["rows_kernel", "grouped_kernel", "mixed_rows_grouped_kernel"])
def test_bwd_reduce_segment_lists(which):
    """CGVP_MAX_SEGS segments of mixed length in ONE launch -- whole blocks of the grid lie beyond the short segments.
    Integer slabs: exact sums, NaN kept wherever no segment stores.  Gaussian slabs: every sum is bitwise the fp32 sum
    in the order of the kernel the list is dispatched to BY ITS LARGEST rows (<= 32: row after row; more: the
    16-group order of _grouped_sum) -- in the mixed list also the segments of 1, 2 and 32 rows, the first among them."""
    n = _lib_max_segs()
    lens = (1, 257, 63, 5, 64, 130, 65, 2)
    rows_of = {"rows_kernel": lambda i: (1, 2, 32, 7, 31)[i % 5],
               "grouped_kernel": lambda i: (33, 37, 240, 64, 100)[i % 5],
               "mixed_rows_grouped_kernel": lambda i: (2, 240, 32, 33, 1, 37)[i % 6]}[which]
    order = _seq_sum if which == "rows_kernel" else _grouped_sum
    for gaussian in (False, True):
        specs, total = _seg_list(rows_of, lambda i: lens[i % len(lens)], n, gaussian)
        assert len(specs) == 32 and (max(s[0].shape[0] for s in specs) <= 32) == (which == "rows_kernel")
        assert which != "mixed_rows_grouped_kernel" or specs[0][0].shape[0] <= 32
        dev = [(slab.to(DEV), col0, ln, dst) for slab, col0, ln, dst in specs]
        grad = torch.full((total,), NAN, device=DEV)
        assert _reduce(dev, grad, 1) == 0
        again = torch.full((total,), NAN, device=DEV)
        assert _reduce(dev, again, 1) == 0
        covered = torch.zeros(total, dtype=torch.bool)
        for i, (slab, col0, ln, dst) in enumerate(specs):
            cols = slab[:, col0:col0 + ln]
            want = torch.from_numpy(order(cols.numpy().astype(F32))) if gaussian else cols.long().sum(0).float()
            assert torch.equal(grad[dst:dst + ln].cpu(), want), (i, slab.shape[0], ln, gaussian)
            covered[dst:dst + ln] = True
        assert torch.equal(torch.isnan(grad).cpu(), ~covered)
        assert torch.equal(grad.nan_to_num(nan=3.0), again.nan_to_num(nan=3.0))
        if not gaussian:                                                   # add mode over the same list
            base = (torch.arange(total) % 9 - 4).float()
            grad = base.to(DEV)
            assert _reduce(dev, grad, 0) == 0
            for slab, col0, ln, dst in specs:
                base[dst:dst + ln] += slab[:, col0:col0 + ln].long().sum(0).float()
            assert torch.equal(grad.cpu(), base)
