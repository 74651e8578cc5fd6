"""The varlen cross attention at head dims 32 and 64 and with unequal side widths (csrc/attn_kernels.hip and
csrc/attn_score_kernels.hip as templates on M = head_dim / 16, include/caster_gvp_attnhd.h, the five attention ops, the C++
bridge, CrossAttentionModule.varlen_supported / forward_varlen, JointGNN(n_attention_heads=4) as a captured step).

REFERENCE.  A per-pair dense softmax in float64 on the CPU (`_dense_ref`: the one of tests/test_attention.py with the
head count and the head width as parameters), gradients by autograd; with dropout the exact-mask oracle of
tests/test_attention_dropout.py (factors from tests/host_math/host_attn_dropout.cpp, called with this test's `heads`).

BOUNDS.  rel_err < 1e-5 for outputs, weights and node scores, < 2e-5 for gradients: the bars tests/test_attention.py,
tests/test_attention_dropout.py and tests/test_attention_scores.py hold head dim 16 to.  A wider head only lengthens the
fp32 dot product of a score from 16 to 64 terms.

LENGTHS.  Those of tests/test_attention_dropout.py: a 1-row pair, exact and off-by-one tiles, a 7-tile key loop, a pair
without keys.  A configuration is (heads, head_dim of the residue-query direction, head_dim of the atom-query one).
"""
import ctypes as C
import functools
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import davis_synth as ds
from conftest import GOLDEN, REPO, rel_err
from gvp_hip import _lib, attention_ops, attention_scores, head_ops  # noqa: F401

DEV = "cuda:0"
RL, AL = [1, 17, 16, 33, 64, 5], [10, 1, 100, 16, 17, 0]
NAMES = ("q_r", "k_a", "v_a", "q_a", "k_r", "v_r")
SCORES = ("atom_mean", "atom_max", "residue_mean", "residue_max")
CONFIGS = [(4, 32, 32), (2, 64, 64), (3, 32, 32), (8, 32, 32)]
UNEQUAL = (8, 16, 32)                                      # E1 = 128, E2 = 256
U64 = (1 << 64) - 1
BAD, UNSUPPORTED = -1, -2


def _ptr(lens):
    return [0] + [int(x) for x in np.cumsum(lens)]


# ---------------------------------------------------------------------------------------------------------------------
# CPU: header, exports, version
def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(cgvp_[a-z0-9_]+)\s*\(", text))


def test_header_and_version_of_their_own():
    header = os.path.join(REPO, "include", "caster_gvp_attnhd.h")
    want = {"cgvp_attn_hd_version", "cgvp_attn_fwd_hd", "cgvp_attn_bwd_hd", "cgvp_attn_weights_hd", "cgvp_attn_node_scores_hd"}
    assert _declared(header) == want == set(attention_ops.hd_exported_symbols())
    main = open(os.path.join(REPO, "include", "caster_gvp.h")).read()
    handle = C.CDLL(_lib.LIB_PATH)
    for name in want:
        assert hasattr(handle, name), name
        assert name not in main and name not in _lib.exported_symbols(), name
    assert attention_ops.hd_lib().cgvp_attn_hd_version() == 1 == attention_ops.ATTN_HD_VERSION
    assert "#define CGVP_ATTN_HD_VERSION 1\n" in open(header).read()
    assert _lib.abi_header_digest() == _lib.ABI_HEADER_SHA256 and _lib.ABI_VERSION == 31      # the main C ABI did not move


# ---------------------------------------------------------------------------------------------------------------------
# CPU: host argument checks (zero pairs in every call but none could launch anyway: the pointers are dummies)
def _attn_call(fn, nprob=2, pairs=0, heads=8, head_dim=32, with_rng=False, which=1, **kw):
    p = 0x1000
    P = (_lib.AttnProblem * 2)()
    for x in P:
        for n, t in _lib.AttnProblem._fields_:
            if t is C.c_void_p:
                setattr(x, n, p)
        x.num_q, x.num_k, x.weights_lq, x.weights_lk = 32, 48, 32, 48
    for n, val in kw.items():
        setattr(P[which], n, val)
    args = [P, nprob, pairs, heads, head_dim, 0.25]
    if fn != "cgvp_attn_weights_hd":
        R = (_lib.Rng * 2)()
        for r in R:
            r.seed, r.p, r.stream = p, 0.1, 3
        args.append(R if with_rng else None)
    return getattr(attention_ops.hd_lib(), fn)(*args, None)


def _score_call(nprob=2, pairs=0, heads=4, head_dim=32, which=1, **kw):
    p = 0x1000
    P = (attention_scores.ScoreProblem * 2)()
    for x in P:
        for n, t in attention_scores.ScoreProblem._fields_:
            if t is C.c_void_p:
                setattr(x, n, p)
        x.num_q, x.num_k = 32, 48
    for n, val in kw.items():
        setattr(P[which], n, val)
    return attention_scores.hd_lib().cgvp_attn_node_scores_hd(P, nprob, pairs, heads, head_dim, 0.25, None)


ATTN_FNS = ("cgvp_attn_fwd_hd", "cgvp_attn_bwd_hd", "cgvp_attn_weights_hd")


def test_entry_points_check_their_arguments_on_the_host():
    for fn in ATTN_FNS:
        for hd in (16, 32, 64):
            assert _attn_call(fn, head_dim=hd) == 0 and _attn_call(fn, head_dim=hd, nprob=1) == 0, (fn, hd)   # num_pairs = 0
        for hd in (0, 8, 24, 48, 128):
            assert _attn_call(fn, head_dim=hd) == UNSUPPORTED, (fn, hd)
        for which in (0, 1):
            for kw in (dict(q=0x1004), dict(v=0x1008), dict(out=0x1001), dict(g_k=0x100c), dict(q_ptr=0), dict(num_q=-1)):
                assert _attn_call(fn, which=which, **kw) == BAD, (fn, which, kw)
        assert _attn_call(fn, nprob=0) == BAD and _attn_call(fn, nprob=3) == BAD and _attn_call(fn, heads=0) == BAD
        assert _attn_call(fn, pairs=-1) == BAD
        # 32-bit element offsets: (rows + 16) * heads * head_dim < 2^31
        for heads, hd in ((8, 32), (8, 64), (2, 64)):
            rows = (1 << 31) // (heads * hd)
            assert _attn_call(fn, heads=heads, head_dim=hd, num_q=rows - 17) == 0, (fn, heads, hd)
            assert _attn_call(fn, heads=heads, head_dim=hd, num_q=rows - 16) == BAD, (fn, heads, hd)
            assert _attn_call(fn, heads=heads, head_dim=hd, num_k=rows) == BAD, (fn, heads, hd)
    for fn in ATTN_FNS[:2]:                                   # the generator arguments, as cgvp_attn_*_dropout checks them
        assert _attn_call(fn, with_rng=True) == 0
        assert _attn_call(fn, with_rng=True, heads=129) == BAD and _attn_call(fn, heads=129) == 0
        assert _attn_call(fn, with_rng=True, head_dim=48) == UNSUPPORTED
    assert _attn_call("cgvp_attn_bwd_hd", g_out=0) == BAD and _attn_call("cgvp_attn_weights_hd", weights=0) == BAD
    # node scores: heads * head_dim <= 128
    for heads, hd in ((4, 32), (2, 64), (3, 32), (8, 16), (1, 64)):
        assert _score_call(heads=heads, head_dim=hd) == 0 and _score_call(heads=heads, head_dim=hd, nprob=1) == 0, (heads, hd)
    for hd in (0, 8, 24, 48, 128):
        assert _score_call(heads=1, head_dim=hd) == UNSUPPORTED, hd
    for heads, hd in ((8, 32), (5, 32), (3, 64), (9, 16)):
        assert _score_call(heads=heads, head_dim=hd) == UNSUPPORTED, (heads, hd)
    for which in (0, 1):
        for kw in (dict(q=0x1004), dict(k=0x1008), dict(out_mean=0x1002), dict(q_ptr=0x1004), dict(num_k=-1), dict(lse=0)):
            assert _score_call(which=which, **kw) == BAD, (which, kw)
    rows = (1 << 31) // 128
    assert _score_call(num_q=rows - 17) == 0 and _score_call(num_q=rows - 16) == BAD


# ---------------------------------------------------------------------------------------------------------------------
# CPU: fake kernels and the Python shape check
@pytest.mark.parametrize("heads,e_r,e_a", [(4, 128, 128), (2, 128, 128), (8, 256, 256), (3, 96, 96), (8, 128, 256)])
def test_fake_kernels_follow_the_shapes(heads, e_r, e_a):
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        f = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device="cuda")
        N, Na, H = 70, 9, heads
        ops = (f(N, e_r), f(Na, e_r), f(Na, e_r), f(Na, e_a), f(N, e_a), f(N, e_a))
        ptrs = (f(3, dt=torch.long), f(3, dt=torch.long))
        pair = f(2, dt=torch.long)
        shapes = lambda ts: [tuple(t.shape) for t in ts]
        for outs in (torch.ops.caster_gvp.cross_attention(*ops, *ptrs, H),
                     torch.ops.caster_gvp.cross_attention_dropout(*ops, *ptrs, H, pair, 1, 2, 0.1, 0.5)):
            assert shapes(outs) == [(N, e_r), (Na, e_a), (N, H), (Na, H)]
            assert all(t.dtype == torch.float32 and t.device.type == "cuda" for t in outs)
        for grads in (torch.ops.caster_gvp.cross_attention_backward(outs[0], outs[1], *ops, *outs, *ptrs, H),
                      torch.ops.caster_gvp.cross_attention_dropout_backward(outs[0], outs[1], *ops, *outs, *ptrs, H, pair, 1, 2,
                                                                            0.1, 0.5)):
            assert shapes(grads) == shapes(ops)
        w_r, w_a = torch.ops.caster_gvp.cross_attention_weights(ops[0], ops[1], outs[2], ops[3], ops[4], outs[3], *ptrs, H, 40, 5)
        assert w_r.shape == (2, 40, 5) and w_a.shape == (2, 5, 40)
        sc = torch.ops.caster_gvp.cross_attention_node_scores(ops[0], ops[1], outs[2], ops[3], ops[4], outs[3], *ptrs, H)
        assert shapes(sc) == [(Na,), (Na,), (N,), (N,)]


def test_python_check_names_the_supported_head_dims():
    f = lambda *s: torch.zeros(*s)
    ptr = torch.zeros(3, dtype=torch.long)
    ok = lambda e_r, e_a: dict(q_r=f(7, e_r), k_a=f(4, e_r), v_a=f(4, e_r), q_a=f(4, e_a), k_r=f(7, e_a), v_r=f(7, e_a),
                               rptr=ptr, aptr=ptr)
    assert attention_ops._check_hd(**ok(128, 128), heads=4) == (32, 32)
    assert attention_ops._check_hd(**ok(128, 128), heads=2) == (64, 64)
    assert attention_ops._check_hd(**ok(128, 256), heads=8) == (16, 32)
    with pytest.raises(NotImplementedError, match="16, 32 and 64"):
        attention_ops._check_hd(**ok(64, 64), heads=8)                    # head_dim 8
    with pytest.raises(NotImplementedError, match="16, 32 and 64"):
        attention_ops._check_hd(**ok(384, 384), heads=8)                  # head_dim 48
    with pytest.raises(NotImplementedError, match="k_a"):
        attention_ops._check_hd(**dict(ok(128, 256), k_a=f(4, 256)), heads=8)


def test_module_gate():
    """CPU rows never take the varlen path; the head-dim part of the gate is checked on the GPU below."""
    from models.joint_gnn import CrossAttentionModule
    assert not CrossAttentionModule(128, 128, 4, 0.0).varlen_supported(torch.zeros(1, 128))


# ---------------------------------------------------------------------------------------------------------------------
# the float64 reference, computed once per configuration
def _operands(cfg, seed=5):
    H, hd_r, hd_a = cfg
    g = torch.Generator().manual_seed(seed)
    N, Na = sum(RL), sum(AL)
    return [torch.randn(n, H * hd, generator=g) for n, hd in ((N, hd_r), (Na, hd_r), (Na, hd_r), (Na, hd_a), (N, hd_a), (N, hd_a))]


def _cotangents(cfg, seed=9):
    H, hd_r, hd_a = cfg
    g = torch.Generator().manual_seed(seed)
    return torch.randn(sum(RL), H * hd_r, generator=g), torch.randn(sum(AL), H * hd_a, generator=g)


def _dense_ref(q, k, v, qp, kp, H, HD, factors=None):
    """per pair, per head: (softmax(q k^T / sqrt(HD)) o f) v in the operands' dtype; also the head-averaged (undropped)
    weights per pair.  A pair without keys yields zero rows."""
    outs, ws = [], []
    for b in range(len(qp) - 1):
        nq, nk = qp[b + 1] - qp[b], kp[b + 1] - kp[b]
        qs, ks = slice(qp[b], qp[b + 1]), slice(kp[b], kp[b + 1])
        if nk == 0:
            outs.append(q[qs] * 0)
            ws.append(q.new_zeros(nq, 0))
            continue
        qb = q[qs].view(nq, H, HD).transpose(0, 1)
        kb = k[ks].view(nk, H, HD).transpose(0, 1)
        vb = v[ks].view(nk, H, HD).transpose(0, 1)
        p = torch.softmax(qb @ kb.transpose(1, 2) / HD ** 0.5, dim=-1)
        ws.append(p.detach().mean(0))
        if factors is not None:
            p = p * factors(b, nq, nk)
        outs.append((p @ vb).transpose(0, 1).reshape(nq, H * HD))
    return torch.cat(outs), ws


def _reference_of(cfg, ops, factors_r=None, factors_a=None):
    H, hd_r, hd_a = cfg
    rp, ap = _ptr(RL), _ptr(AL)
    g_r, g_a = _cotangents(cfg)
    leaves = [t.detach().double().requires_grad_() for t in ops]
    o_r, w_r = _dense_ref(leaves[0], leaves[1], leaves[2], rp, ap, H, hd_r, factors_r)
    o_a, w_a = _dense_ref(leaves[3], leaves[4], leaves[5], ap, rp, H, hd_a, factors_a)
    ((o_r * g_r.double()).sum() + (o_a * g_a.double()).sum()).backward()
    return dict(o_r=o_r.detach(), o_a=o_a.detach(), w_r=w_r, w_a=w_a, grads=[t.grad for t in leaves])


@functools.lru_cache(maxsize=None)
def _reference(cfg):
    return _reference_of(cfg, _operands(cfg))


def _gpu(cfg):
    ops = [t.to(DEV) for t in _operands(cfg)]
    g_r, g_a = (t.to(DEV) for t in _cotangents(cfg))
    return ops, torch.tensor(_ptr(RL), device=DEV), torch.tensor(_ptr(AL), device=DEV), g_r, g_a


def _run(cfg, ops, rptr, aptr, g_r, g_a, op=None, tail=()):
    leaves = [t.detach().clone().requires_grad_() for t in ops]
    o = (op or torch.ops.caster_gvp.cross_attention)(*leaves, rptr, aptr, cfg[0], *tail)
    ((o[0] * g_r).sum() + (o[1] * g_a).sum()).backward()
    return [t.detach() for t in o] + [[t.grad for t in leaves]]


def _assert_matches(got, ref, what):
    o_r, o_a, lse_r, lse_a, grads = got
    errs = [rel_err(o_r, ref["o_r"]), rel_err(o_a, ref["o_a"])] + [rel_err(g, w) for g, w in zip(grads, ref["grads"])]
    print(f"{what}: forward rel err {errs[0]:.2e} / {errs[1]:.2e}; gradients "
          + " ".join(f"{n} {e:.2e}" for n, e in zip(NAMES, errs[2:])))
    assert errs[0] < 1e-5 and errs[1] < 1e-5, what
    for name, e in zip(NAMES, errs[2:]):
        assert e < 2e-5, (what, name)
    lo = sum(RL[:5])                                        # the pair without atoms: zero rows, zero gradients, exactly
    assert float(o_r[lo:].abs().max()) == 0.0 and float(grads[0][lo:].abs().max()) == 0.0, what


# ---------------------------------------------------------------------------------------------------------------------
# GPU
@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CONFIGS + [UNEQUAL], ids=lambda c: "h%d_hd%d_%d" % c)
def test_forward_gradients_and_weights_match_the_float64_reference(cfg):
    H = cfg[0]
    ops, rptr, aptr, g_r, g_a = _gpu(cfg)
    ref = _reference(cfg)
    got = _run(cfg, ops, rptr, aptr, g_r, g_a)
    _assert_matches(got, ref, f"{cfg}")
    assert got[0].shape == (sum(RL), H * cfg[1]) and got[1].shape == (sum(AL), H * cfg[2])
    again = torch.ops.caster_gvp.cross_attention(*ops, rptr, aptr, H)
    for a, b in zip(again, got[:4]):
        assert torch.equal(a, b)                            # a second call: the same bits (no atomics anywhere)
    rmax, amax = max(RL), max(AL)
    d_r, d_a = torch.ops.caster_gvp.cross_attention_weights(ops[0], ops[1], got[2], ops[3], ops[4], got[3], rptr, aptr, H, rmax, amax)
    assert d_r.shape == (len(RL), rmax, amax) and d_a.shape == (len(RL), amax, rmax)
    worst = 0.0
    for b, (lr, la) in enumerate(zip(RL, AL)):
        if la:
            worst = max(worst, rel_err(d_r[b, :lr, :la], ref["w_r"][b]), rel_err(d_a[b, :la, :lr], ref["w_a"][b]))
        assert float(d_r[b, lr:].abs().sum()) == 0 and float(d_r[b, :, la:].abs().sum()) == 0
        assert float(d_a[b, la:].abs().sum()) == 0 and float(d_a[b, :, lr:].abs().sum()) == 0
    print(f"{cfg}: weights rel err {worst:.2e}")
    assert worst < 1e-5


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("host_attn_dropout") / "host_attn_dropout.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-o", so,
                           os.path.join(REPO, "tests", "host_math", "host_attn_dropout.cpp")])
    return C.CDLL(so)


def _factors(host, seed, offset, stream, p, q0, nq, k0, nk, heads):
    """[heads][nq][nk]: the factor of (head, global query row q0 + i, global key row k0 + j), by the generator's definition."""
    out = np.zeros((heads, nq, nk), np.float32)
    if out.size:
        host.host_attn_dropout(C.c_ulonglong(int(seed) & U64), C.c_ulonglong(int(offset) & U64), C.c_int(stream),
                               C.c_float(p), C.c_int(heads), C.c_longlong(q0), C.c_longlong(nq), C.c_longlong(k0),
                               C.c_longlong(nk), C.c_int(0), out.ctypes.data_as(C.c_void_p))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("cfg", [(4, 32, 32), (2, 64, 64)], ids=lambda c: "h%d_hd%d_%d" % c)
def test_dropout_matches_the_exact_mask_oracle(host, cfg, p):
    H = cfg[0]
    ops, rptr, aptr, g_r, g_a = _gpu(cfg)
    rp, ap = _ptr(RL), _ptr(AL)
    pair = torch.ops.caster_gvp.rng_next(torch.tensor([0x5EED5EED5EED, 41], dtype=torch.int64, device=DEV))
    hp = [int(x) for x in pair.cpu()]
    assert hp == [0x5EED5EED5EED, 42]
    sites = (7, 8)
    got = _run(cfg, ops, rptr, aptr, g_r, g_a, torch.ops.caster_gvp.cross_attention_dropout, (pair, sites[0], sites[1], p, p))
    f_r = lambda b, nq, nk: torch.from_numpy(_factors(host, hp[0], hp[1], sites[0], p, rp[b], nq, ap[b], nk, H)).double()
    f_a = lambda b, nq, nk: torch.from_numpy(_factors(host, hp[0], hp[1], sites[1], p, ap[b], nq, rp[b], nk, H)).double()
    ref = _reference_of(cfg, _operands(cfg), f_r, f_a)
    _assert_matches(got, ref, f"{cfg} p={p}")
    assert not torch.equal(got[0], _run(cfg, ops, rptr, aptr, g_r, g_a)[0])
    plain = _run(cfg, ops, rptr, aptr, g_r, g_a)
    assert torch.equal(got[2], plain[2]) and torch.equal(got[3], plain[3])       # the lse of the undropped scores, bitwise


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [(4, 32, 32), (2, 64, 64)], ids=lambda c: "h%d_hd%d_%d" % c)
def test_p_zero_is_the_op_without_dropout_bitwise(cfg):
    ops, rptr, aptr, g_r, g_a = _gpu(cfg)
    pair = torch.ops.caster_gvp.rng_next(torch.tensor([11, 0], dtype=torch.int64, device=DEV))
    base = _run(cfg, ops, rptr, aptr, g_r, g_a)
    zero = _run(cfg, ops, rptr, aptr, g_r, g_a, torch.ops.caster_gvp.cross_attention_dropout, (pair, 1, 2, 0.0, 0.0))
    for a, b in zip(zero[:4] + zero[4], base[:4] + base[4]):
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CONFIGS[:3], ids=lambda c: "h%d_hd%d_%d" % c)
def test_node_scores_match_the_reduced_float64_weights(cfg):
    H = cfg[0]
    ops, rptr, aptr, g_r, g_a = _gpu(cfg)
    ref = _reference(cfg)
    _, _, lse_r, lse_a = torch.ops.caster_gvp.cross_attention(*ops, rptr, aptr, H)
    runs = [torch.ops.caster_gvp.cross_attention_node_scores(ops[0], ops[1], lse_r, ops[3], ops[4], lse_a, rptr, aptr, H)
            for _ in range(2)]
    reduce = lambda ws, nq: (torch.cat([w.mean(0) if w.shape[0] and w.shape[1] else w.new_zeros(w.shape[1]) for w in ws]),
                             torch.cat([w.max(0).values if w.shape[0] and w.shape[1] else w.new_zeros(w.shape[1]) for w in ws]))
    # (w_a of the pair without atoms is [0 queries, 5 keys]: its residues get 0, the kernel's documented value)
    w_a = [w if w.shape[0] else w.new_zeros(0, lr) for w, lr in zip(ref["w_a"], RL)]
    want = dict(zip(SCORES, reduce(ref["w_r"], RL) + reduce(w_a, AL)))
    for name, got, again in zip(SCORES, *runs):
        assert torch.equal(got, again), name
        err = rel_err(got, want[name])
        print(f"{cfg} {name}: rel_err {err:.3e}")
        assert err < 1e-5, name


def _module_case(e1, e2, heads, seed=0):
    from models.joint_gnn import CrossAttentionModule
    torch.manual_seed(seed)
    mod = CrossAttentionModule(e1, e2, heads, 0.0, True, 2, 0.2).to(DEV).eval()
    rl, al = [57, 120, 33], [21, 40, 17]
    g = torch.Generator().manual_seed(3)
    r, m = torch.randn(sum(rl), e1, generator=g).to(DEV), torch.randn(sum(al), e2, generator=g).to(DEV)
    rb = torch.repeat_interleave(torch.arange(3), torch.tensor(rl)).to(DEV)
    mb = torch.repeat_interleave(torch.arange(3), torch.tensor(al)).to(DEV)
    return mod, rl, al, r, m, rb, mb, torch.tensor(_ptr(rl)).to(DEV), torch.tensor(_ptr(al)).to(DEV)


@pytest.mark.gpu
def test_node_scores_of_width_256_raise_from_the_op_and_come_from_the_dense_weights_in_the_module():
    from models.joint_gnn import NodeAttention, to_dense_batch
    cfg = (8, 32, 32)
    ops, rptr, aptr, g_r, g_a = _gpu(cfg)
    _, _, lse_r, lse_a = torch.ops.caster_gvp.cross_attention(*ops, rptr, aptr, 8)
    with pytest.raises(NotImplementedError, match="128"):
        torch.ops.caster_gvp.cross_attention_node_scores(ops[0], ops[1], lse_r, ops[3], ops[4], lse_a, rptr, aptr, 8)
    mod, rl, al, r, m, rb, mb, rptr, aptr = _module_case(256, 256, 8)
    scores = []
    with torch.no_grad():
        e1, e2, none = mod.forward_varlen(r, m, rptr, aptr, scores_out=scores)
        plain = mod.forward_varlen(r, m, rptr, aptr)
        dr, rmask = to_dense_batch(r, rb)
        dm, mmask = to_dense_batch(m, mb)
        _, _, (x1, x2) = mod(dr, dm, rmask, mmask)
    assert none is None and len(scores) == 1 and isinstance(scores[0], NodeAttention)
    assert torch.equal(e1, plain[0]) and torch.equal(e2, plain[1])
    x1, x2 = x1.double().cpu(), x2.double().cpu()
    pairs = list(enumerate(zip(rl, al)))
    want = dict(atom_mean=[x1[b, :lr, :la].mean(0) for b, (lr, la) in pairs],
                atom_max=[x1[b, :lr, :la].max(0).values for b, (lr, la) in pairs],
                residue_mean=[x2[b, :la, :lr].mean(0) for b, (lr, la) in pairs],
                residue_max=[x2[b, :la, :lr].max(0).values for b, (lr, la) in pairs])
    for name in SCORES:
        got = getattr(scores[0], name)
        assert got.shape == ((sum(al),) if name.startswith("atom") else (sum(rl),))
        err = rel_err(got, torch.cat(want[name]))
        print(f"{name}: rel_err {err:.3e}")
        assert err < 1e-5, name


@pytest.mark.gpu
def test_opcheck_at_head_dim_32():
    cfg = (4, 32, 32)
    ops, rptr, aptr, g_r, g_a = _gpu(cfg)
    args = tuple(t.clone().requires_grad_() for t in ops) + (rptr, aptr, 4)
    torch.library.opcheck(torch.ops.caster_gvp.cross_attention.default, args)
    pair = torch.ops.caster_gvp.rng_next(torch.tensor([5, 0], dtype=torch.int64, device=DEV))
    args = tuple(t.clone().requires_grad_() for t in ops) + (rptr, aptr, 4, pair, 1, 2, 0.5, 0.1)
    torch.library.opcheck(torch.ops.caster_gvp.cross_attention_dropout.default, args)


@pytest.mark.gpu
@pytest.mark.parametrize("e1,e2,heads", [(128, 128, 4), (256, 256, 8), (128, 256, 8)])
def test_module_varlen_equals_its_dense_forward(monkeypatch, e1, e2, heads):
    """forward_varlen (embeddings and weights) == the module's own dense forward through stock nn.MultiheadAttention, on
    the C++ bridge route and, with the bridge taken away, on the custom-op route; the two routes agree bitwise."""
    from models.joint_gnn import to_dense_batch
    mod, rl, al, r, m, rb, mb, rptr, aptr = _module_case(e1, e2, heads)
    assert mod.varlen_supported(r)
    with torch.no_grad():
        dr, rmask = to_dense_batch(r, rb)
        dm, mmask = to_dense_batch(m, mb)
        d1, d2, (x1, x2) = mod(dr, dm, rmask, mmask)
    routes = []
    for bridge in (True, False):
        if not bridge:
            monkeypatch.setattr(head_ops, "_bridge", lambda: None)
        elif head_ops._bridge() is None or not hasattr(head_ops._bridge(), "head_cross_attention"):
            pytest.skip("C++ bridge not built")            # (as test_bridge_head_ops_equal_the_custom_ops: visibly, not half a test)
        with torch.no_grad():
            e_1, e_2, (w1, w2) = mod.forward_varlen(r, m, rptr, aptr, need_weights=True)
        print(f"({e1}, {e2}, {heads}) bridge={bridge}: {rel_err(e_1, d1[rmask]):.2e} {rel_err(e_2, d2[mmask]):.2e}")
        assert rel_err(e_1, d1[rmask]) < 1e-5 and rel_err(e_2, d2[mmask]) < 1e-5
        assert w1.shape == x1.shape and w2.shape == x2.shape
        for b, (lr, la) in enumerate(zip(rl, al)):
            assert rel_err(w1[b, :lr, :la], x1[b, :lr, :la]) < 1e-5 and rel_err(w2[b, :la, :lr], x2[b, :la, :lr]) < 1e-5
        routes.append((e_1, e_2))
    assert len(routes) == 2
    assert torch.equal(routes[0][0], routes[1][0]) and torch.equal(routes[0][1], routes[1][1])


@pytest.mark.gpu
@pytest.mark.parametrize("e,heads", [(64, 8), (384, 8)])
def test_other_head_dims_stay_on_the_dense_path(e, heads):
    from models.joint_gnn import CrossAttentionModule
    mod = CrossAttentionModule(e, e, heads, 0.0).to(DEV)
    assert not mod.varlen_supported(torch.zeros(1, e, device=DEV))           # head_dim 8 and 48


@pytest.mark.gpu
def test_model_with_four_heads_runs_as_a_captured_training_step(pretrained):
    """JointGNN(n_attention_heads=4, attention_dropout=0.1): head_dim 32 at width 128.  The pretrained fixture loads
    strictly (in_proj_weight does not depend on the head count), the step captures (the dense path reads lengths on the
    host and cannot), and a replay's loss equals the eager training step's loss drawn from the same generator states
    (every dropout site of the step -- encoders, head, attention -- reads device-resident {seed, offset} states), at the
    tolerance of tests/test_hip_models.py::test_graphed_train_step_equals_eager."""
    from gvp_hip import autograd_ops
    from gvp_hip.graphed import GraphedTrainStep
    from models.joint_gnn import JointGNN
    import models.joint_gnn as J
    kw = json.load(open(os.path.join(GOLDEN, "model_kwargs.json")))
    model = JointGNN(protein_gnn_kwargs=kw["protein_gnn_kwargs"], molecule_gnn_kwargs=kw["molecule_gnn_kwargs"],
                     **dict(kw["joint_gnn_kwargs"], n_attention_heads=4, attention_dropout=0.1))
    model.load_state_dict(pretrained, strict=True)
    model = model.to(DEV).train()
    layer = model.cross_attn_module.cross_attn_layers[0]
    assert layer.embed1_to_2.head_dim == 32 and model.cross_attn_module.varlen_supported(torch.empty(1, 128, device=DEV))
    to = lambda d: {k: (tuple(t.to(DEV) for t in v) if isinstance(v, tuple) else v.to(DEV)) for k, v in d.items()}
    pb, mb = ds.pair_batch(4, 1, lengths=[60, 45, 80, 33])
    pd, md = to(ds.to_torch(pb)), to(ds.to_torch(mb))
    pd["ptr"], md["ptr"] = torch.as_tensor(pb.ptr).to(DEV), torch.as_tensor(mb.ptr).to(DEV)
    target = torch.randn(4, 1, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    runner = GraphedTrainStep(model, torch.nn.functional.mse_loss)
    first, _ = runner.run(pd, md, target)                    # warm-up passes, capture, one replay
    torch.cuda.synchronize()
    first = float(first)                                     # (the bucket's static loss tensor: the next replay overwrites it)
    assert len(runner.buckets) == 1 and np.isfinite(first)
    states = [head_ops._head_rng_state(torch.device(DEV))] + [v[1] for v in autograd_ops._RNG_STATE.values()]
    saved = [s.clone() for s in states]
    loss, pred = runner.run(pd, md, target)                  # a pure replay
    torch.cuda.synchronize()
    replay = float(loss)
    assert pred.shape == (4, 1) and replay != first          # fresh factors
    assert sum(b.steps for b in runner.buckets.values()) == 2
    for s, old in zip(states, saved):
        s.copy_(old)
    dense = []
    real = J.to_dense_batch
    try:
        J.to_dense_batch = lambda *a, **k: dense.append(1) or real(*a, **k)
        with torch.enable_grad():
            eager = float(torch.nn.functional.mse_loss(model(pd, md)[0], target).detach())
    finally:
        J.to_dense_batch = real
    torch.cuda.synchronize()
    print(f"replay loss {replay:.8f}, eager loss from the same states {eager:.8f}")
    assert not dense                                         # the eager step took the varlen path too
    assert abs(replay - eager) <= 1e-5 * abs(eager)
