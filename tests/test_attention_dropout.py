"""Attention dropout inside the varlen cross-attention kernels (csrc/attn_kernels.hip DROP instantiations,
csrc/gvp_rng.h attn_drop_*, include/caster_gvp_attndrop.h, caster_gvp::cross_attention_dropout, CrossAttentionModule /
JointGNN with attention_dropout > 0 in training mode).

REFERENCE.  The factor f[head][q][k] is recomputed on the host by the generator's own definition (gvp_rng.h compiled
with g++: tests/host_math/host_attn_dropout.cpp) from the {seed, offset} pair read back from the device.  With it
nn.MultiheadAttention's training arithmetic -- O = (softmax(Q K^T / 4) o f) V per pair and head -- is evaluated densely
in float64 on the CPU, its gradients by autograd.

BOUNDS.  rel_err < 1e-5 for outputs and < 2e-5 for gradients: what tests/test_attention.py holds the same kernels to
without dropout; the only new arithmetic is one exact-or-rounded multiply per probability.  A single wrong factor is an
error of order 1.  The host-mask drop rate is held to max(0.02, 3 / sqrt(n)) of p, the bound of
test_fused_dropout_sites_vs_stock_ops_with_the_same_mask.
"""
import ctypes as C
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import davis_synth as ds
from conftest import GOLDEN, REPO, rel_err
from gvp_hip import _lib, attention_ops, head_ops  # noqa: F401

DEV = "cuda:0"
H, E = 8, 128
RL, AL = [1, 17, 16, 33, 64, 5], [10, 1, 100, 16, 17, 0]
NAMES = ("q_r", "k_a", "v_a", "q_a", "k_r", "v_r")
U64 = (1 << 64) - 1


# ---------------------------------------------------------------------------------------------------------------------
# the host definition of the factor
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("host_attn_dropout") / "host_attn_dropout.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-o", so,
                           os.path.join(REPO, "tests", "host_math", "host_attn_dropout.cpp")])
    return C.CDLL(so)


def _factors(host, seed, offset, stream, p, q0, nq, k0, nk, heads=H, form=0):
    """[heads][nq][nk] float32: the factor of (head, global query row q0 + i, global key row k0 + j)."""
    out = np.zeros((heads, nq, nk), np.float32)
    if out.size:
        host.host_attn_dropout(C.c_ulonglong(int(seed) & U64), C.c_ulonglong(int(offset) & U64), C.c_int(stream),
                               C.c_float(p), C.c_int(heads), C.c_longlong(q0), C.c_longlong(nq), C.c_longlong(k0),
                               C.c_longlong(nk), C.c_int(form), out.ctypes.data_as(C.c_void_p))
    return out


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_host_mask_values_rate_and_purity(host, p):
    seed, offset, nq, nk = 0x1234567890ABCDEF, 99, 64, 96
    f = _factors(host, seed, offset, 3, p, 5, nq, 7, nk)
    inv = np.float32(1) / (np.float32(1) - np.float32(p))
    assert set(np.unique(f)) == {np.float32(0), inv}
    n = f.size
    assert abs(float((f == 0).mean()) - p) < max(0.02, 3 / math.sqrt(n))
    assert np.array_equal(f, _factors(host, seed, offset, 3, p, 5, nq, 7, nk))


def test_host_mask_depends_on_stream_offset_and_head(host):
    seed, offset, p = 77, 5, 0.5
    f = _factors(host, seed, offset, 3, p, 0, 64, 0, 96)
    assert (f != _factors(host, seed, offset, 4, p, 0, 64, 0, 96)).mean() > 0.2
    assert (f != _factors(host, seed, offset + 1, 3, p, 0, 64, 0, 96)).mean() > 0.2
    assert (f != _factors(host, seed + 1, offset, 3, p, 0, 64, 0, 96)).mean() > 0.2
    for h in range(1, H):
        assert (f[0] != f[h]).mean() > 0.2, h


@pytest.mark.parametrize("form", [0, 1, 2])
def test_host_mask_is_a_function_of_global_rows_not_of_tiling(host, form):
    """A block with first rows (q0, k0) is the window of a larger block; the run forms the kernels use (1: 1 x 4 key runs,
    2: 4 x 1 query runs) give the definition's (form 0) factors at every alignment of their first row."""
    seed, offset, p = 0xDEADBEEFCAFE, 1 << 33, 0.5
    big = _factors(host, seed, offset, 9, p, 3, 40, 5, 50, form=form)
    small = _factors(host, seed, offset, 9, p, 3 + 7, 13, 5 + 9, 11, form=form)
    assert np.array_equal(small, big[:, 7:20, 9:20])
    for q0 in range(4):
        for k0 in range(4):
            want = _factors(host, seed, offset, 9, p, q0 + 100, 21, k0 + 200, 22, form=0)
            assert np.array_equal(_factors(host, seed, offset, 9, p, q0 + 100, 21, k0 + 200, 22, form=form), want), (q0, k0)


# ---------------------------------------------------------------------------------------------------------------------
# CPU: fake kernels, argument checks, version
def test_fake_kernels_of_both_ops():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        f = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device="cuda")
        N, Na = 70, 9
        ops = (f(N, E), f(Na, E), f(Na, E), f(Na, E), f(N, E), f(N, E))
        ptrs = (f(3, dt=torch.long), f(3, dt=torch.long))
        pair = f(2, dt=torch.long)
        outs = torch.ops.caster_gvp.cross_attention_dropout(*ops, *ptrs, H, pair, 1, 2, 0.1, 0.5)
        assert [tuple(t.shape) for t in outs] == [(N, E), (Na, E), (N, H), (Na, H)]
        assert all(t.dtype == torch.float32 and t.device.type == "cuda" for t in outs)
        grads = torch.ops.caster_gvp.cross_attention_dropout_backward(outs[0], outs[1], *ops, *outs, *ptrs, H, pair, 1, 2,
                                                                      0.1, 0.5)
        assert [tuple(t.shape) for t in grads] == [tuple(t.shape) for t in ops]
        assert all(t.dtype == torch.float32 and t.device.type == "cuda" for t in grads)


def test_entry_points_check_their_arguments_on_the_host():
    """CGVP_ERR_BAD_ARG before any launch and before the `num_pairs == 0` return: every call asks for zero pairs, so
    nothing could launch even if a check were missing.  Pointers are never dereferenced."""
    L = attention_ops.dropout_lib()
    BAD, ptr = -1, 0x1000
    fields = [n for n, t in _lib.AttnProblem._fields_ if t is C.c_void_p and n != "weights"]

    def call(fn, nprob=2, heads=H, with_rng=True, which=1, **kw):
        P = (_lib.AttnProblem * 2)()
        for x in P:
            for n in fields:
                setattr(x, n, ptr)
            x.num_q, x.num_k = 32, 48
        R = (_lib.Rng * 2)()
        for r in R:
            r.seed, r.p, r.stream = ptr, 0.1, 3
        for n, val in kw.items():
            setattr(R[which], n, val)
        return fn(P, nprob, 0, heads, 0.25, R if with_rng else None, None)

    for fn in (L.cgvp_attn_fwd_dropout, L.cgvp_attn_bwd_dropout):
        assert call(fn) == 0 and call(fn, nprob=1) == 0 and call(fn, with_rng=False) == 0
        assert call(fn, p=0.0) == 0 and call(fn, seed=0) == 0 and call(fn, heads=attention_ops.DROPOUT_MAX_HEADS) == 0
        for which in (0, 1):
            for kw in (dict(p=1.0), dict(p=-0.25), dict(p=float("nan")), dict(p=float("inf")), dict(seed=ptr + 4),
                       dict(seed=ptr + 1)):
                assert call(fn, which=which, **kw) == BAD, (which, kw)
            assert call(fn, which=which, seed=0, p=1.0) == BAD              # p is checked even where no seed is given
        assert call(fn, nprob=3) == BAD and call(fn, nprob=0) == BAD
        assert call(fn, heads=attention_ops.DROPOUT_MAX_HEADS + 1) == BAD and call(fn, heads=0) == BAD
        assert fn(None, 2, 0, H, 0.25, None, None) == BAD


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(cgvp_[a-z0-9_]+)\s*\(", text))


def test_header_and_version_of_their_own():
    header = os.path.join(REPO, "include", "caster_gvp_attndrop.h")
    assert _declared(header) == set(attention_ops.dropout_exported_symbols())
    main = open(os.path.join(REPO, "include", "caster_gvp.h")).read()
    for name in attention_ops.dropout_exported_symbols():
        assert name not in main and name not in _lib.exported_symbols(), name
    text = open(header).read()
    assert attention_ops.dropout_lib().cgvp_attn_dropout_version() == attention_ops.ATTN_DROPOUT_VERSION
    assert f"#define CGVP_ATTN_DROPOUT_VERSION {attention_ops.ATTN_DROPOUT_VERSION}\n" in text
    assert f"#define CGVP_ATTN_DROPOUT_MAX_HEADS {attention_ops.DROPOUT_MAX_HEADS}\n" in text
    assert _lib.abi_header_digest() == _lib.ABI_HEADER_SHA256 and _lib.ABI_VERSION == 31      # the main C ABI did not move


# ---------------------------------------------------------------------------------------------------------------------
# GPU
def _ptr(lens):
    return [0] + [int(x) for x in np.cumsum(lens)]


def _operands(seed, rl=RL, al=AL):
    """(q_r, k_a, v_a, q_a, k_r, v_r) as in tests/test_attention.py::_ragged, on the CPU, and the two ptr lists."""
    g = torch.Generator().manual_seed(seed)
    N, Na = sum(rl), sum(al)
    return [torch.randn(n, E, generator=g) for n in (N, Na, Na, Na, N, N)], _ptr(rl), _ptr(al)


def _cotangents(seed=9, rl=RL, al=AL):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(sum(rl), E, generator=g), torch.randn(sum(al), E, generator=g)


def _direction64(host, q, k, v, qp, kp, pair, site, p):
    """One direction in float64: per pair and head (softmax(q k^T / 4) o f) v, f from the host definition at the pair's
    GLOBAL rows.  A pair without keys yields zero rows."""
    outs = []
    for b in range(len(qp) - 1):
        nq, nk = qp[b + 1] - qp[b], kp[b + 1] - kp[b]
        qs, ks = slice(qp[b], qp[b + 1]), slice(kp[b], kp[b + 1])
        if nq == 0:
            continue
        if nk == 0:
            outs.append(q[qs] * 0)
            continue
        qb = q[qs].view(nq, H, 16).transpose(0, 1)
        kb = k[ks].view(nk, H, 16).transpose(0, 1)
        vb = v[ks].view(nk, H, 16).transpose(0, 1)
        f = torch.from_numpy(_factors(host, pair[0], pair[1], site, p, qp[b], nq, kp[b], nk)).double()
        pr = torch.softmax(qb @ kb.transpose(1, 2) / 4.0, dim=-1) * f
        outs.append((pr @ vb).transpose(0, 1).reshape(nq, E))
    return torch.cat(outs)


def _oracle(host, ops, rptr, aptr, pair, sites, ps, g_r, g_a):
    """-> (o_r, o_a, [six input gradients of sum(o_r g_r) + sum(o_a g_a)]) in float64 on the CPU."""
    leaves = [t.detach().double().cpu().requires_grad_() for t in ops]
    o_r = _direction64(host, leaves[0], leaves[1], leaves[2], rptr, aptr, pair, sites[0], ps[0])
    o_a = _direction64(host, leaves[3], leaves[4], leaves[5], aptr, rptr, pair, sites[1], ps[1])
    ((o_r * g_r.double()).sum() + (o_a * g_a.double()).sum()).backward()
    return o_r.detach(), o_a.detach(), [t.grad for t in leaves]


def _run(ops, rptr, aptr, pair, sites, ps, g_r, g_a, op=None):
    """The op forward and backward on the GPU -> (o_r, o_a, lse_r, lse_a, [six gradients])."""
    leaves = [t.detach().clone().requires_grad_() for t in ops]
    if op is None:
        o = torch.ops.caster_gvp.cross_attention_dropout(*leaves, rptr, aptr, H, pair, sites[0], sites[1], ps[0], ps[1])
    else:
        o = op(*leaves, rptr, aptr, H)
    ((o[0] * g_r).sum() + (o[1] * g_a).sum()).backward()
    return [t.detach() for t in o] + [[t.grad for t in leaves]]


def _next_pair(state):
    return torch.ops.caster_gvp.rng_next(state)


def _on_gpu(rl=RL, al=AL):
    ops, rp, ap = _operands(5, rl, al)
    g_r, g_a = _cotangents(9, rl, al)
    return ([t.to(DEV) for t in ops], torch.tensor(rp, device=DEV), torch.tensor(ap, device=DEV), rp, ap,
            g_r.to(DEV), g_a.to(DEV))


@pytest.fixture(scope="module")
def gpu_inputs():
    return _on_gpu()


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_outputs_and_gradients_match_the_exact_mask_oracle(host, gpu_inputs, p):
    ops, rptr, aptr, rp, ap, g_r, g_a = gpu_inputs
    state = torch.tensor([0x5EED5EED5EED, 41], dtype=torch.int64, device=DEV)
    pair = _next_pair(state)
    hp = [int(x) for x in pair.cpu()]
    assert hp == [0x5EED5EED5EED, 42]
    sites, ps = (7, 8), (p, p)
    o_r, o_a, lse_r, lse_a, grads = _run(ops, rptr, aptr, pair, sites, ps, g_r, g_a)
    w_r, w_a, wg = _oracle(host, ops, rp, ap, hp, sites, ps, g_r.cpu(), g_a.cpu())
    print(f"p={p}: forward rel err {rel_err(o_r, w_r):.2e} / {rel_err(o_a, w_a):.2e}; gradients "
          + " ".join(f"{n} {rel_err(g, w):.2e}" for n, g, w in zip(NAMES, grads, wg)))
    assert rel_err(o_r, w_r) < 1e-5 and rel_err(o_a, w_a) < 1e-5
    for name, got, want in zip(NAMES, grads, wg):
        assert rel_err(got, want) < 2e-5, name
    assert float(o_r[sum(RL[:5]):].abs().max()) == 0.0                  # the pair without atoms: zero rows, zero gradients
    assert float(grads[0][sum(RL[:5]):].abs().max()) == 0.0
    # the lse is the one of the undropped scores
    _, _, l_r, l_a, _ = _run(ops, rptr, aptr, None, None, None, g_r, g_a, op=torch.ops.caster_gvp.cross_attention)
    assert torch.equal(lse_r, l_r) and torch.equal(lse_a, l_a)


@pytest.mark.gpu
@pytest.mark.parametrize("lens", [None, ([40, 37, 3], [9, 12, 21])])
def test_two_problems_with_different_p_match_the_oracle(host, gpu_inputs, lens):
    """The two directions differ in p and site.  The launches order the two problems by their loop length: with the
    issue's lengths (136 residues, 144 atoms) only the d K / d V launch swaps them, with more residues than atoms (the
    shape of real batches) the forward and d Q launches do."""
    ops, rptr, aptr, rp, ap, g_r, g_a = gpu_inputs if lens is None else _on_gpu(*lens)
    pair = _next_pair(torch.tensor([-3, 1 << 40], dtype=torch.int64, device=DEV))      # a seed with the top bit set
    hp = [int(x) for x in pair.cpu()]
    sites, ps = (1, 2), (0.5, 0.1)
    o_r, o_a, _, _, grads = _run(ops, rptr, aptr, pair, sites, ps, g_r, g_a)
    w_r, w_a, wg = _oracle(host, ops, rp, ap, hp, sites, ps, g_r.cpu(), g_a.cpu())
    assert rel_err(o_r, w_r) < 1e-5 and rel_err(o_a, w_a) < 1e-5
    for name, got, want in zip(NAMES, grads, wg):
        assert rel_err(got, want) < 2e-5, name


@pytest.mark.gpu
def test_p_zero_is_the_op_without_dropout_bitwise(gpu_inputs):
    ops, rptr, aptr, rp, ap, g_r, g_a = gpu_inputs
    pair = _next_pair(torch.tensor([11, 0], dtype=torch.int64, device=DEV))
    base = _run(ops, rptr, aptr, None, None, None, g_r, g_a, op=torch.ops.caster_gvp.cross_attention)
    zero = _run(ops, rptr, aptr, pair, (1, 2), (0.0, 0.0), g_r, g_a)
    for got, want in zip(zero[:4], base[:4]):
        assert torch.equal(got, want)
    for name, got, want in zip(NAMES, zero[4], base[4]):
        assert torch.equal(got, want), name
    half = _run(ops, rptr, aptr, pair, (1, 2), (0.5, 0.0), g_r, g_a)          # the atom direction keeps factor 1
    assert torch.equal(half[1], base[1]) and torch.equal(half[3], base[3]) and torch.equal(half[2], base[2])
    for i in (3, 4, 5):
        assert torch.equal(half[4][i], base[4][i]), NAMES[i]
    assert not torch.equal(half[0], base[0])


@pytest.mark.gpu
def test_opcheck(gpu_inputs):
    ops, rptr, aptr, rp, ap, g_r, g_a = gpu_inputs
    pair = _next_pair(torch.tensor([5, 0], dtype=torch.int64, device=DEV))
    args = tuple(t.clone().requires_grad_() for t in ops) + (rptr, aptr, H, pair, 1, 2, 0.5, 0.1)
    torch.library.opcheck(torch.ops.caster_gvp.cross_attention_dropout.default, args)


@pytest.mark.gpu
def test_same_pair_and_sites_repeat_bitwise_and_new_ones_differ(gpu_inputs):
    ops, rptr, aptr, rp, ap, g_r, g_a = gpu_inputs
    state = torch.tensor([2024, 0], dtype=torch.int64, device=DEV)
    pair = _next_pair(state)
    a = _run(ops, rptr, aptr, pair, (3, 4), (0.5, 0.5), g_r, g_a)
    b = _run(ops, rptr, aptr, pair, (3, 4), (0.5, 0.5), g_r, g_a)
    for got, want in zip(a[:4] + a[4], b[:4] + b[4]):
        assert torch.equal(got, want)                                  # no atomics anywhere
    nxt = _run(ops, rptr, aptr, _next_pair(state), (3, 4), (0.5, 0.5), g_r, g_a)
    swapped = _run(ops, rptr, aptr, pair, (4, 3), (0.5, 0.5), g_r, g_a)
    for other in (nxt, swapped):
        assert not torch.equal(other[0], a[0]) and not torch.equal(other[1], a[1])
        assert not torch.equal(other[4][0], a[4][0]) and not torch.equal(other[4][3], a[4][3])
        assert torch.equal(other[2], a[2]) and torch.equal(other[3], a[3])       # (the lse does not see the factors)


@pytest.mark.gpu
def test_forward_and_backward_replay_from_a_captured_graph_with_fresh_factors(host, gpu_inputs):
    """rng_next + the op + its backward captured in one torch.cuda.graph on a side stream after a warm-up; each replay
    advances the offset on the device, so two replays differ and each matches the oracle for the offset it left."""
    ops, rptr, aptr, rp, ap, g_r, g_a = gpu_inputs
    p, sites = 0.5, (5, 6)
    state = torch.tensor([987654321, 100], dtype=torch.int64, device=DEV)
    leaves = [t.detach().clone().requires_grad_() for t in ops]

    def step():
        pair = _next_pair(state)
        o = torch.ops.caster_gvp.cross_attention_dropout(*leaves, rptr, aptr, H, pair, sites[0], sites[1], p, p)
        grads = torch.autograd.grad([o[0], o[1]], leaves, [g_r, g_a])
        return pair, o[0], o[1], grads

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pair, o_r, o_a, grads = step()
    seen = []
    for k in range(2):
        graph.replay()
        torch.cuda.synchronize()
        hp = [int(x) for x in pair.cpu()]
        assert hp == [987654321, 102 + k]                              # (the warm-up took 101)
        w_r, w_a, wg = _oracle(host, ops, rp, ap, hp, sites, (p, p), g_r.cpu(), g_a.cpu())
        assert rel_err(o_r, w_r) < 1e-5 and rel_err(o_a, w_a) < 1e-5, k
        for name, got, want in zip(NAMES, grads, wg):
            assert rel_err(got, want) < 2e-5, (k, name)
        seen.append((o_r.clone(), o_a.clone()))
    assert not torch.equal(seen[0][0], seen[1][0]) and not torch.equal(seen[0][1], seen[1][1])


@pytest.mark.gpu
@pytest.mark.parametrize("autocast", [False, True])
def test_module_trains_on_the_varlen_path_with_attention_dropout(monkeypatch, autocast):
    """CrossAttentionModule(attn_dropout = 0.25) in training mode on compact rows: no dense fallback, fresh factors every
    forward, the same forward again after the same torch.manual_seed (the device-side state is re-seeded when the
    generator's seed CHANGES, so another seed is set in between), finite gradients for every parameter.  Under
    autocast DropSites is inactive and the layer draws a pair of its own."""
    import models.joint_gnn as J

    def no_dense(*a, **k):
        raise AssertionError("the dense fallback was taken")
    monkeypatch.setattr(J, "to_dense_batch", no_dense)
    torch.manual_seed(0)
    mod = J.CrossAttentionModule(128, 128, 8, attn_dropout=0.25).to(DEV).train()
    rl, al = [57, 120, 33], [21, 40, 17]
    g = torch.Generator().manual_seed(3)
    r, m = torch.randn(sum(rl), 128, generator=g).to(DEV), torch.randn(sum(al), 128, generator=g).to(DEV)
    rptr, aptr = torch.tensor(_ptr(rl), device=DEV), torch.tensor(_ptr(al), device=DEV)
    assert mod.varlen_supported(r)
    ctx = (lambda: torch.autocast("cuda", dtype=torch.bfloat16)) if autocast else (lambda: torch.autocast("cuda", enabled=False))

    def fwd():
        with ctx():
            e1, e2, w = mod.forward_varlen(r, m, rptr, aptr)
        assert w is None
        return e1, e2

    torch.manual_seed(100)                  # (whatever ran before: the state has now been drawn from a seed other than 101)
    fwd()
    torch.manual_seed(101)
    a1, a2 = fwd()
    b1, b2 = fwd()
    assert not torch.equal(a1, b1) and not torch.equal(a2, b2)
    torch.manual_seed(102)
    fwd()
    torch.manual_seed(101)
    c1, c2 = fwd()
    assert torch.equal(a1, c1) and torch.equal(a2, c2)
    mod.eval()
    with torch.no_grad():
        v1, v2 = fwd()
    mod.train()
    assert not torch.equal(v1.float(), a1.float()) and not torch.equal(v2.float(), a2.float())
    (c1.float().square().mean() + c2.float().square().mean()).backward()
    for name, prm in mod.named_parameters():
        assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()), name
    assert float(mod.embed1_to_2.in_proj_weight.grad.abs().max()) > 0 and float(mod.embed2_to_1.in_proj_weight.grad.abs().max()) > 0


@pytest.mark.gpu
def test_whole_model_with_attention_dropout_runs_as_a_captured_training_step(pretrained):
    """JointGNN(attention_dropout = 0.1) in training mode through GraphedTrainStep with the fused optimizer: it captures
    (the dense fallback reads lengths on the host and cannot), the losses are finite and the parameters move."""
    from gvp_hip.graphed import GraphedTrainStep
    from gvp_hip.optim import FusedAdam
    from models.joint_gnn import JointGNN
    kw = json.load(open(os.path.join(GOLDEN, "model_kwargs.json")))
    model = JointGNN(protein_gnn_kwargs=kw["protein_gnn_kwargs"], molecule_gnn_kwargs=kw["molecule_gnn_kwargs"],
                     **dict(kw["joint_gnn_kwargs"], attention_dropout=0.1))
    model.load_state_dict(pretrained, strict=True)
    model = model.to(DEV).train()
    assert model.cross_attn_module.varlen_supported(torch.empty(1, 128, device=DEV))
    to = lambda d: {k: (tuple(t.to(DEV) for t in v) if isinstance(v, tuple) else v.to(DEV)) for k, v in d.items()}
    batches = []
    for seed, lengths in ((1, [60, 45, 80, 33]), (2, [58, 47, 77, 36])):
        pb, mb = ds.pair_batch(4, seed, lengths=lengths)
        pd, md = to(ds.to_torch(pb)), to(ds.to_torch(mb))
        pd["ptr"], md["ptr"] = torch.as_tensor(pb.ptr).to(DEV), torch.as_tensor(mb.ptr).to(DEV)
        batches.append((pd, md, torch.randn(4, 1, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))))
    params = list(model.parameters())
    before = [prm.detach().clone() for prm in params]
    runner = GraphedTrainStep(model, torch.nn.functional.mse_loss, optimizer=FusedAdam(params, lr=1e-3, max_grad_norm=1.0))
    losses = []
    for pd, md, target in (batches[0], batches[1], batches[0]):
        loss, pred = runner.run(pd, md, target)
        torch.cuda.synchronize()
        assert pred.shape == (4, 1) and bool(torch.isfinite(pred).all())
        losses.append(float(loss))
    assert all(math.isfinite(x) for x in losses)
    assert losses[0] != losses[2]                                      # the same batch again: other factors, moved weights
    moved = sum(not torch.equal(prm.detach(), old) for prm, old in zip(params, before))
    assert moved >= 100
    w = model.cross_attn_module.cross_attn_layers[0].embed1_to_2.in_proj_weight
    assert not torch.equal(w.detach(), before[[id(x) for x in params].index(id(w))])
