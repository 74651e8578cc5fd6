"""Per-node attention scores for pair lists, each graph encoded once (csrc/attn_pairs_score_kernels.hip,
include/caster_gvp_pairscore.h, gvp_hip.pair_node_scores, JointGNN.score_pairs_with_node_attention).

REFERENCES.  The kernel: `caster_gvp::cross_attention_node_scores` on the per-pair rows gathered with index_select,
BITWISE (a pair's arithmetic is the same instruction sequence on the same values wherever its rows lie; neither kernel
uses atomics), and a per-pair dense softmax in float64 on the CPU (`_dense_ref` of tests/test_attention_scores.py
restated for any head width), rel_err < 1e-5, that file's bound.  The model: `predict_with_node_attention` on the same
pairs collated as an ordinary batch, rel_err < 1e-4 (the project's parity bar, conftest.rel_err), and `score_pairs` for
the affinities, bitwise."""
import ctypes as C
import functools
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import davis_synth as ds
from conftest import GOLDEN, REPO, rel_err
from gvp_hip import _lib, attention_ops, attention_scores, pair_node_scores as pns, pair_scoring as ps  # noqa: F401

DEV = "cuda:0"
BAD, UNSUPPORTED = -1, -2
NAMES = ("atom_mean", "atom_max", "residue_mean", "residue_max")
_TABLES = ("q_ptr", "k_ptr", "q_graph", "k_graph", "qout_ptr", "kout_ptr")
_COUNTS = ("num_q_graphs", "num_k_graphs", "num_q", "num_k", "num_qout", "num_kout")


def _ptr(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# CPU
def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(cgvp_[a-z0-9_]+)\s*\(", text))


def test_entry_point_has_a_header_and_a_version_of_its_own():
    header = os.path.join(REPO, "include", "caster_gvp_pairscore.h")
    assert _declared(header) == set(pns.exported_symbols())
    assert set(pns.exported_symbols()) == {"cgvp_pair_score_version", "cgvp_attn_node_scores_pairs"}
    main = open(os.path.join(REPO, "include", "caster_gvp.h")).read()
    handle = C.CDLL(_lib.LIB_PATH)
    for name in pns.exported_symbols():
        assert hasattr(handle, name), name
        assert name not in main and name not in _lib.exported_symbols(), name
        assert name not in ps.exported_symbols() and name not in attention_scores.exported_symbols(), name
    assert pns.lib().cgvp_pair_score_version() == 1 == pns.PAIR_SCORE_VERSION
    text = open(header).read()
    assert "#define CGVP_PAIR_SCORE_VERSION 1\n" in text
    # the struct's fields, in the header's order, are the binding's
    body = re.search(r"typedef struct \{(.*?)\} cgvp_attn_pairs_score_problem;", re.sub(r"/\*.*?\*/", "", text, flags=re.S), re.S).group(1)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            names = decl.replace("*", " ").split(",")
            fields += [names[0].split()[-1]] + [n.strip() for n in names[1:]]
    assert fields == [n for n, _ in pns.PairScoreProblem._fields_], fields
    assert _lib.abi_header_digest() == _lib.ABI_HEADER_SHA256          # the main C ABI did not move


def _bad_argument_cases():
    """(keyword changes of one call) -> expected code.  `p` is the valid address the other fields hold."""
    p = 0x1000
    cases = [(dict(nprob=0), BAD), (dict(nprob=3), BAD), (dict(heads=0), BAD), (dict(pairs=-1), BAD), (dict(pairs=1 << 30), BAD),
             (dict(problems=None), BAD)]
    for name in _COUNTS:
        cases.append(({name: -1}, BAD))
    for name in _TABLES:
        cases += [({name: 0}, BAD), ({name: p + 4}, BAD)]                 # NULL, not 8-byte aligned
    for name in ("q", "k"):
        cases += [({name: 0}, BAD), ({name: p + 8}, BAD)]                 # NULL with rows, not 16-byte aligned
    cases += [(dict(lse=0), BAD), (dict(lse=p + 4), BAD)]                 # 8 heads: the lse rows are read as float4
    for name in ("out_mean", "out_max"):
        cases += [({name: 0}, BAD), ({name: p + 2}, BAD)]
    for name in ("num_q", "num_k"):                                       # side_ok at width 128: (rows + 16) * 128 < 2^31
        cases.append(({name: (1 << 24) - 16}, BAD))
    cases.append((dict(num_qout=(1 << 28) - 16), BAD))                    # (rows + 16) * 8 heads < 2^31
    return cases


def test_entry_point_checks_its_arguments_on_the_host():
    """CGVP_ERR_* before any launch and before the `num_pairs == 0` return: every call but the refused ones asks for zero
    pairs, so nothing here could launch even if a check were missing.  Pointers are never dereferenced."""
    L, p = pns.lib(), 0x1000
    ptr_fields = [n for n, t in pns.PairScoreProblem._fields_ if t is C.c_void_p]

    def call(nprob=2, pairs=0, heads=8, head_dim=16, which=1, problems=True, **kw):
        P = (pns.PairScoreProblem * 2)()
        for x in P:
            for n in ptr_fields:
                setattr(x, n, p)
            x.num_q_graphs, x.num_k_graphs, x.num_q, x.num_k, x.num_qout, x.num_kout = 3, 4, 32, 48, 64, 96
        for n, val in kw.items():
            setattr(P[which], n, val)
        return L.cgvp_attn_node_scores_pairs(P if problems else None, nprob, pairs, heads, head_dim, 0.25, None)

    assert call() == 0 and call(nprob=1) == 0 and call(heads=4, head_dim=32) == 0 and call(heads=2, head_dim=64) == 0
    for kw, code in _bad_argument_cases():
        kw = dict(kw)
        if "problems" in kw:
            kw["problems"] = False
        for which in (0, 1):
            assert call(which=which, **kw) == code, (which, kw)
            assert call(which=which, head_dim=48, **kw) == UNSUPPORTED, (which, kw)   # first of all
    for hd in (0, 8, 48, 128):
        assert call(head_dim=hd) == UNSUPPORTED
    for heads, hd in ((9, 16), (16, 16), (5, 32), (8, 32), (3, 64), (4, 64)):     # heads * head_dim > 128
        assert call(heads=heads, head_dim=hd) == UNSUPPORTED, (heads, hd)
    # an empty side needs no buffers
    assert call(num_q=0, q=0) == 0 and call(num_k=0, k=0) == 0 and call(num_qout=0, lse=0) == 0
    assert call(num_kout=0, out_mean=0, out_max=0) == 0
    assert call(heads=3, lse=p + 4) == 0                                  # the lse rows are 16-byte units only when 4 | heads
    assert call(num_q=(1 << 24) - 17) == 0 and call(heads=4, head_dim=32, num_q=(1 << 24) - 16) == BAD
    assert call(num_qout=(1 << 28) - 17) == 0 and call(num_kout=(1 << 31) - 17) == 0 and call(num_kout=(1 << 31) - 16) == BAD


def test_fake_kernel_shapes_dtypes_and_refusals():
    """The fake kernel sizes the outputs from lse2 / lse1 (host-known shapes) and refuses what the op refuses: heads
    outside 1..8 and a width over 128, with NotImplementedError."""
    from torch._subclasses.fake_tensor import FakeTensorMode
    op = torch.ops.caster_gvp.cross_attention_pairs_node_scores
    with FakeTensorMode():
        f = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device="cuda")
        i = lambda n: f(n, dt=torch.long)
        tables = (i(4), i(3), i(5), i(5), i(6), i(6))
        outs = op(f(70, 128), f(9, 128), f(100, 4), f(9, 64), f(70, 64), f(20, 4), *tables, 4)
        assert [tuple(t.shape) for t in outs] == [(20,), (20,), (100,), (100,)]
        assert all(t.dtype == torch.float32 and t.device.type == "cuda" for t in outs)
        with pytest.raises(NotImplementedError, match="heads"):
            op(f(70, 144), f(9, 144), f(100, 9), f(9, 144), f(70, 144), f(20, 9), *tables, 9)
        with pytest.raises(NotImplementedError, match="128"):
            op(f(70, 256), f(9, 256), f(100, 8), f(9, 128), f(70, 128), f(20, 8), *tables, 8)
        with pytest.raises(NotImplementedError, match="128"):
            op(f(70, 128), f(9, 128), f(100, 4), f(9, 256), f(70, 256), f(20, 4), *tables, 4)
        with pytest.raises(NotImplementedError):
            pns._shapes(f(70, 96), f(9, 96), 2)                           # head_dim 48
        assert pns._shapes(f(70, 128), f(9, 64), 4) == ((128, 32), (64, 16))


def _joint(**over):
    from models.joint_gnn import JointGNN
    kw = json.load(open(os.path.join(GOLDEN, "model_kwargs.json")))
    return JointGNN(protein_gnn_kwargs=kw["protein_gnn_kwargs"], molecule_gnn_kwargs=kw["molecule_gnn_kwargs"],
                    **dict(kw["joint_gnn_kwargs"], **over))


def test_score_pairs_with_node_attention_refuses_cpu_batches():
    model = _joint()
    p, m = ds.pair_batch(2, 3, lengths=[20, 33])
    with pytest.raises(NotImplementedError, match="CUDA"):
        model.score_pairs_with_node_attention(ds.to_torch(p), ds.to_torch(m))
    assert model.training                                                  # untouched
    with pytest.raises(RuntimeError, match="no cross-attention"):
        _joint(num_cross_attn_layers=0).score_pairs_with_node_attention(ds.to_torch(p), ds.to_torch(m))


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the kernel
# exact and off-by-one key tiles, a 1-row graph, an empty graph on each side, and 129 / 130 / 273 query rows: waves take
# a second and a third trip of the 8 x 16-row stride and the partial tail lands on a wave other than wave 0
LEN1, LEN2 = [17, 0, 16, 33, 130, 273], [1, 15, 0, 16, 40, 129]
UNUSED1, UNUSED2 = 3, 4                                    # the graph of each side no pair references
NP = 70


def _pair_list():
    """70 unsorted pairs with repetition (locate's second 64-pair chunk): consecutive repeats of one graph, the first and
    the last graph of each side, the empty graph of each side as query and as key, then a seeded draw."""
    head = [(0, 0), (0, 0), (0, 1), (5, 5), (5, 5), (4, 5), (1, 2), (1, 0), (0, 2), (5, 2), (2, 3), (2, 3), (1, 5), (5, 0),
            (4, 3), (5, 1), (4, 0), (2, 5), (1, 3)]
    rng = np.random.default_rng(17)
    used1, used2 = [g for g in range(6) if g != UNUSED1], [g for g in range(6) if g != UNUSED2]
    rest = [(int(a), int(b)) for a, b in zip(rng.choice(used1, NP - len(head) - 2), rng.choice(used2, NP - len(head) - 2))]
    pairs = np.array(head + rest + [(5, 5), (0, 0)], dtype=np.int64)
    assert pairs.shape == (NP, 2) and list(pairs[:, 0]) != sorted(pairs[:, 0])
    assert set(pairs[:, 0]) == set(used1) and set(pairs[:, 1]) == set(used2)
    return pairs


@functools.lru_cache(maxsize=None)
def _tables():
    pairs = _pair_list()
    (chunk,) = ps.plan_pairs(LEN1, LEN2, pairs, 10 ** 9)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    t = dict(ptr1=dev(_ptr(LEN1)), ptr2=dev(_ptr(LEN2)), g1=dev(chunk.g1), g2=dev(chunk.g2), optr1=dev(chunk.optr1),
             optr2=dev(chunk.optr2), rows1=chunk.rows1, rows2=chunk.rows2, chunk=chunk)
    # the rows of every pair, gathered: what the batch kernels need
    rows = lambda ptr, g: np.concatenate([np.arange(ptr[x], ptr[x + 1]) for x in g] + [np.zeros(0, dtype=np.int64)])
    t["idx1"], t["idx2"] = dev(rows(_ptr(LEN1), chunk.g1)), dev(rows(_ptr(LEN2), chunk.g2))
    return t


def _table_args(t):
    return [t[k] for k in ("ptr1", "ptr2", "g1", "g2", "optr1", "optr2")]


def _operands(heads, w1, w2, seed=None):
    """(q1, k1, v1, q2, k2, v2): seeded randn on the CPU; side 1 holds the rows of q1 / k2 / v2"""
    g = torch.Generator().manual_seed(100 + heads + w2 if seed is None else seed)
    N1, N2 = sum(LEN1), sum(LEN2)
    return [torch.randn(n, w, generator=g) for n, w in ((N1, w1), (N2, w1), (N2, w1), (N2, w2), (N1, w2), (N1, w2))]


def _pair_scores(ops, t, heads):
    """forward over the pair tables (for the lse) + the new op on the unique rows -> (its four vectors, lse1, lse2)"""
    q1, k1, v1, q2, k2, v2 = ops
    _, _, lse1, lse2 = ps.cross_attention_pairs(q1, k1, v1, q2, k2, v2, *_table_args(t), heads, t["rows1"], t["rows2"], lse=True)
    return torch.ops.caster_gvp.cross_attention_pairs_node_scores(q1, k1, lse1, q2, k2, lse2, *_table_args(t), heads), lse1, lse2


SHAPES = [(8, 128, 128), (4, 128, 128), (2, 128, 128), (3, 48, 48), (4, 128, 64)]
SHAPE_IDS = ["8x16", "4x32", "2x64", "3x16", "4x32_and_4x16"]


@functools.lru_cache(maxsize=None)
def _case(heads, w1, w2):
    """One head shape, computed once for the tests that share it -> (operands on the CPU, got, again, want), the last three
    {name: CPU tensor}: the new op twice, and the batch kernel on the gathered rows."""
    t = _tables()
    cpu_ops = _operands(heads, w1, w2)
    ops = [x.to(DEV) for x in cpu_ops]
    got, _, _ = _pair_scores(ops, t, heads)
    again, _, _ = _pair_scores(ops, t, heads)
    sel = lambda x, idx: torch.index_select(x, 0, idx)
    q1, k1, v1, q2, k2, v2 = ops
    gathered = [sel(q1, t["idx1"]), sel(k1, t["idx2"]), sel(v1, t["idx2"]), sel(q2, t["idx2"]), sel(k2, t["idx1"]), sel(v2, t["idx1"])]
    _, _, lse_r, lse_a = torch.ops.caster_gvp.cross_attention(*gathered, t["optr1"], t["optr2"], heads)
    want = torch.ops.caster_gvp.cross_attention_node_scores(gathered[0], gathered[1], lse_r, gathered[3], gathered[4], lse_a,
                                                            t["optr1"], t["optr2"], heads)
    torch.cuda.synchronize()
    named = lambda outs: {n: o.cpu() for n, o in zip(NAMES, outs)}
    return cpu_ops, named(got), named(again), named(want)


@pytest.mark.gpu
@pytest.mark.parametrize("heads,w1,w2", SHAPES, ids=SHAPE_IDS)
def test_pair_kernel_equals_the_batch_kernel_on_gathered_rows_bitwise(heads, w1, w2):
    """(The two-launch case: one head count serves both directions, so widths 128 / 64 are 4 heads of 32 against 4 heads
    of 16.)"""
    t = _tables()
    _, got, again, want = _case(heads, w1, w2)
    for name, rows in zip(NAMES, (t["rows2"], t["rows2"], t["rows1"], t["rows1"])):
        a, b = got[name], want[name]
        assert a.shape == b.shape == (rows,) and a.dtype == b.dtype == torch.float32, name
        print(f"{name}: {tuple(a.shape)}, differing elements {int((a != b).sum())}")
        assert torch.equal(a, b), name
        assert torch.equal(a, again[name]), name                          # call to call bitwise
        assert torch.isfinite(a).all() and (a >= 0).all() and (a <= 1).all(), name
    c = t["chunk"]
    seen = [0, 0]
    for mean, mx, qlen, klen, kout, side in (("atom_mean", "atom_max", np.asarray(LEN1)[c.g1], np.asarray(LEN2)[c.g2], c.optr2, 0),
                                             ("residue_mean", "residue_max", np.asarray(LEN2)[c.g2], np.asarray(LEN1)[c.g1], c.optr1, 1)):
        for b in range(NP):
            ks = slice(int(kout[b]), int(kout[b + 1]))
            assert ks.stop - ks.start == klen[b]
            if qlen[b] == 0 and klen[b] > 0:                              # keys of a pair without queries: exactly 0
                assert (got[mean][ks] == 0.0).all() and (got[mx][ks] == 0.0).all(), (mean, b)
                seen[side] += 1
            if qlen[b] > 0 and klen[b] > 0:
                # every query's weights sum to 1 over the pair's keys, so the column means do
                assert abs(float(got[mean][ks].double().sum()) - 1.0) < 1e-5, (mean, b)
    assert min(seen) > 0


def _dense_ref(q, k, qptr, kptr, qg, kg, heads):
    """per pair, per head: p = softmax(q k^T / sqrt(head_dim)) in the dtype of the operands; w = p.mean over the heads;
    -> (mean, max) = w.mean(0), w.max(0).values per pair (inference/evaluation.py:98-102), concatenated in pair order.
    Keys of a pair without queries get 0 (the kernel's documented value; the reference has no such pair)."""
    hd = q.shape[1] // heads
    means, maxs = [], []
    for a, b in zip(qg, kg):
        lq, lk = int(qptr[a + 1] - qptr[a]), int(kptr[b + 1] - kptr[b])
        if lq == 0 or lk == 0:
            means.append(q.new_zeros(lk)), maxs.append(q.new_zeros(lk))
            continue
        qb = q[qptr[a]:qptr[a + 1]].view(lq, heads, hd).transpose(0, 1)
        kb = k[kptr[b]:kptr[b + 1]].view(lk, heads, hd).transpose(0, 1)
        w = torch.softmax(qb @ kb.transpose(1, 2) / math.sqrt(hd), dim=-1).mean(0)
        means.append(w.mean(0)), maxs.append(w.max(0).values)
    return torch.cat(means), torch.cat(maxs)


def _reference(cpu_ops, heads):
    c = _tables()["chunk"]
    d = [x.double() for x in cpu_ops]
    p1, p2 = _ptr(LEN1), _ptr(LEN2)
    atom_mean, atom_max = _dense_ref(d[0], d[1], p1, p2, c.g1, c.g2, heads)
    res_mean, res_max = _dense_ref(d[3], d[4], p2, p1, c.g2, c.g1, heads)
    return dict(zip(NAMES, (atom_mean, atom_max, res_mean, res_max)))


@pytest.mark.gpu
@pytest.mark.parametrize("heads,w1,w2", SHAPES, ids=SHAPE_IDS)
def test_pair_kernel_against_a_dense_float64_softmax(heads, w1, w2):
    cpu_ops, got, _, _ = _case(heads, w1, w2)
    ref = _reference(cpu_ops, heads)
    for name in NAMES:
        assert got[name].shape == ref[name].shape, name
        err = rel_err(got[name], ref[name])
        print(f"{name}: rel_err {err:.3e}")
        assert err < 1e-5, name


@pytest.mark.gpu
def test_refused_calls_launch_nothing_and_nothing_is_written_outside_the_outputs():
    """Every CGVP_ERR_* case on a call that WOULD launch (70 pairs, real buffers): the code is returned and the
    sentinel-filled outputs are untouched.  The outputs lie inside larger buffers (32 floats in front, and 32 behind
    that num_kout covers): the unmodified call then overwrites exactly the entries below optr[-1].  (No out-of-range
    device index is tried: the tables are the valid ones.)"""
    from gvp_hip.ops import _stream
    t, L, SENTINEL, PAD, heads = _tables(), pns.lib(), -7.0, 32, 8
    cpu_ops, want, _, _ = _case(heads, 128, 128)
    q1, k1, v1, q2, k2, v2 = [x.to(DEV) for x in cpu_ops]
    _, _, lse1, lse2 = ps.cross_attention_pairs(q1, k1, v1, q2, k2, v2, *_table_args(t), heads, t["rows1"], t["rows2"], lse=True)
    rows = dict(zip(NAMES, (t["rows2"], t["rows2"], t["rows1"], t["rows1"])))
    assert all(r % 16 for r in rows.values())
    bufs = {n: torch.full((r + 2 * PAD,), SENTINEL, device=DEV) for n, r in rows.items()}

    def call(nprob=2, pairs=NP, heads=heads, head_dim=16, which=1, problems=True, **kw):
        P = (pns.PairScoreProblem * 2)()
        for x, (q, k, lse, qp, kp, qg, kg, qo, ko, mean, mx) in zip(P, (
                (q1, k1, lse1, "ptr1", "ptr2", "g1", "g2", "optr1", "optr2", "atom_mean", "atom_max"),
                (q2, k2, lse2, "ptr2", "ptr1", "g2", "g1", "optr2", "optr1", "residue_mean", "residue_max"))):
            x.q, x.k, x.lse = (a.data_ptr() for a in (q, k, lse))
            x.out_mean, x.out_max = bufs[mean][PAD:].data_ptr(), bufs[mx][PAD:].data_ptr()
            x.q_ptr, x.k_ptr, x.q_graph, x.k_graph, x.qout_ptr, x.kout_ptr = (t[n].data_ptr() for n in (qp, kp, qg, kg, qo, ko))
            x.num_q_graphs, x.num_k_graphs = t[qp].numel() - 1, t[kp].numel() - 1
            x.num_q, x.num_k, x.num_qout, x.num_kout = q.shape[0], k.shape[0], lse.shape[0], rows[mean] + PAD
        for n, val in kw.items():
            base = getattr(P[which], n) if n in _TABLES + ("q", "k", "lse", "out_mean", "out_max") and val else 0
            setattr(P[which], n, base + (val - 0x1000 if base else val))   # (an offset from the case's nominal address)
        return L.cgvp_attn_node_scores_pairs(P if problems else None, nprob, pairs, heads, head_dim, 0.25, _stream())

    for kw, code in _bad_argument_cases():
        kw = dict(kw)
        if "problems" in kw:
            kw["problems"] = False
        for which in (0, 1):
            assert call(which=which, **kw) == code, (which, kw)
            assert call(which=which, head_dim=48, **kw) == UNSUPPORTED, (which, kw)
    assert call(head_dim=48) == UNSUPPORTED
    assert call(heads=16) == UNSUPPORTED and call(head_dim=32) == UNSUPPORTED      # a width of 256
    torch.cuda.synchronize()
    for name, b in bufs.items():
        assert (b == SENTINEL).all(), name
    assert call() == 0                                                     # the same call, unmodified, does run
    torch.cuda.synchronize()
    for name, r in rows.items():
        b = bufs[name].cpu()
        assert (b[:PAD] == SENTINEL).all() and (b[PAD + r:] == SENTINEL).all(), name
        assert (b[PAD:PAD + r] != SENTINEL).all(), name
        assert torch.equal(b[PAD:PAD + r], want[name]), name


@pytest.mark.gpu
def test_no_pairs():
    from gvp_hip.ops import _stream
    t, heads = _tables(), 8
    q1, k1, v1, q2, k2, v2 = [x.to(DEV) for x in _case(heads, 128, 128)[0]]
    none = torch.zeros(0, dtype=torch.int64, device=DEV)
    zero = torch.zeros(1, dtype=torch.int64, device=DEV)
    lse = torch.zeros(0, heads, device=DEV)
    outs = torch.ops.caster_gvp.cross_attention_pairs_node_scores(q1, k1, lse, q2, k2, lse, t["ptr1"], t["ptr2"], none, none,
                                                                  zero, zero, heads)
    torch.cuda.synchronize()
    assert len(outs) == 4 and all(o.shape == (0,) and o.dtype == torch.float32 and o.is_cuda for o in outs)
    P = (pns.PairScoreProblem * 2)()
    for x, (q, k, qp, kp) in zip(P, ((q1, k1, "ptr1", "ptr2"), (q2, k2, "ptr2", "ptr1"))):
        x.q, x.k, x.q_ptr, x.k_ptr = q.data_ptr(), k.data_ptr(), t[qp].data_ptr(), t[kp].data_ptr()
        x.q_graph = x.k_graph = x.qout_ptr = x.kout_ptr = zero.data_ptr()
        x.num_q_graphs, x.num_k_graphs, x.num_q, x.num_k = t[qp].numel() - 1, t[kp].numel() - 1, q.shape[0], k.shape[0]
    assert pns.lib().cgvp_attn_node_scores_pairs(P, 2, 0, heads, 16, 0.25, _stream()) == 0
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_opcheck():
    t, heads = _tables(), 8
    ops = [x.to(DEV) for x in _case(heads, 128, 128)[0]]
    _, lse1, lse2 = _pair_scores(ops, t, heads)
    args = (ops[0], ops[1], lse1, ops[3], ops[4], lse2, *_table_args(t), heads)
    torch.library.opcheck(torch.ops.caster_gvp.cross_attention_pairs_node_scores.default, args)

@pytest.mark.gpu
def test_the_op_replays_from_a_captured_graph():
    """Captured alone in one torch.cuda.graph (a single kernel, no parallel branches) after a warm-up call; q / k / lse
    overwritten in place with new values; the replay equals an eager call on the new values."""
    t, heads = _tables(), 8

    def batch(seed):
        ops = [x.to(DEV) for x in _operands(heads, 128, 128, seed)]
        _, lse1, lse2 = _pair_scores(ops, t, heads)
        return [ops[0], ops[1], lse1, ops[3], ops[4], lse2]

    op = torch.ops.caster_gvp.cross_attention_pairs_node_scores
    tables = [x.clone() for x in _table_args(t)]
    static = [x.clone() for x in batch(41)]
    want_first = op(*static, *tables, heads)                               # the warm-up call
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = op(*static, *tables, heads)
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(outs, want_first):
        assert torch.equal(got, want)
    nxt = batch(43)
    want_second = op(*nxt, *tables, heads)
    for dst, src in zip(static, nxt):
        dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    for got, want, name in zip(outs, want_second, NAMES):
        assert torch.equal(got, want), name
    assert not torch.equal(outs[0], want_first[0])


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the model (the graphs and the pair list of tests/test_pair_scoring.py)
PROT_LENGTHS = [20, 33, 48]
FIELDS = ("residue_mean", "residue_max", "atom_mean", "atom_max")


def _to(d):
    return {k: (tuple(t.to(DEV) for t in v) if isinstance(v, tuple) else v.to(DEV)) for k, v in d.items()}


def _batch(graphs, ptr=True):
    gb = ds.collate(graphs)
    d = _to(ds.to_torch(gb))
    if ptr:
        d["ptr"] = torch.as_tensor(gb.ptr).to(DEV)
    return d


@pytest.fixture(scope="module")
def graphs():
    rng = np.random.default_rng(2)
    prots = [ds.protein_graph(L, rng) for L in PROT_LENGTHS]
    drugs = [ds.drug_graph(rng) for _ in range(4)]
    pairs = [(p, d) for p in range(3) for d in range(4)] + [(2, 1), (0, 3), (2, 1)]
    order = np.random.default_rng(3).permutation(len(pairs))
    pairs = [pairs[i] for i in order]
    return prots, drugs, pairs


@pytest.fixture
def deterministic():
    """As tests/test_attention_scores.py makes its bitwise model comparisons: in the default mode the segment pooling of
    the head adds rows with float atomics (index_add_), so two plain calls of one model already differ in the last bit
    and "the same bits" would say nothing about this change."""
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    yield
    torch.use_deterministic_algorithms(was)


def _model_case(model, graphs, layers):
    prots, drugs, pairs = graphs
    K = len(pairs)
    model = model.to(DEV).eval()
    dp, dm = _batch(prots), _batch(drugs)
    len1, len2 = [PROT_LENGTHS[p] for p, _ in pairs], [drugs[d]["x_s"].shape[0] for _, d in pairs]
    plain = model.score_pairs(dp, dm, pairs)
    want_y, want = model.predict_with_node_attention(_batch([prots[p] for p, _ in pairs]), _batch([drugs[d] for _, d in pairs]))
    y, scores, (optr1, optr2) = model.score_pairs_with_node_attention(dp, dm, pairs)
    torch.cuda.synchronize()
    assert y.shape == (K, 1) and not y.requires_grad
    assert torch.equal(y, plain)                                          # asking for the scores changes no affinity
    assert model.score_pairs(dp, dm, pairs).equal(plain)
    assert len(scores) == len(want) == layers
    assert not optr1.is_cuda and not optr2.is_cuda and optr1.dtype == optr2.dtype == torch.int64
    assert optr1.tolist() == _ptr(len1).tolist() and optr2.tolist() == _ptr(len2).tolist()
    for i, (got, ref) in enumerate(zip(scores, want)):
        assert type(got).__name__ == "NodeAttention" and got._fields == FIELDS
        for name in FIELDS:
            a, b = getattr(got, name), getattr(ref, name)
            assert a.shape == b.shape == ((sum(len1),) if name.startswith("residue") else (sum(len2),)), name
            assert a.dtype == torch.float32 and a.is_cuda and not a.requires_grad, name
            err = rel_err(a, b)
            print(f"layer {i} {name}: rel_err against the collated batch {err:.3e}")
            assert err < 1e-4, (i, name)
        views = attention_scores.per_pair(got.residue_mean, optr1)
        assert len(views) == K and [v.shape[0] for v in views] == len1
        assert [v.shape[0] for v in attention_scores.per_pair(got.atom_max, optr2)] == len2
    # at least three chunks: a budget with chunks of one pair and of several, and one that some single pairs exceed
    unequal = []
    for max_rows in (150, 80):
        plan = ps.plan_pairs(PROT_LENGTHS, [g["x_s"].shape[0] for g in drugs], pairs, max_rows)
        assert len(plan) >= 3
        yc, chunked, (c1, c2) = model.score_pairs_with_node_attention(dp, dm, torch.tensor(pairs, device=DEV), max_rows=max_rows)
        assert torch.equal(c1, optr1) and torch.equal(c2, optr2)
        assert torch.equal(yc, model.score_pairs(dp, dm, pairs, max_rows=max_rows))
        assert rel_err(yc, want_y) < 1e-4
        assert len(chunked) == layers
        for i, (got, one, ref) in enumerate(zip(chunked, scores, want)):
            for name in FIELDS:
                a, b = getattr(got, name), getattr(one, name)
                print(f"{len(plan)} chunks, layer {i} {name}: differing elements {int((a != b).sum())} of {a.numel()}, "
                      f"rel_err against one chunk {rel_err(a, b):.3e}, against the collated batch {rel_err(a, getattr(ref, name)):.3e}")
                assert a.shape == b.shape and rel_err(a, getattr(ref, name)) < 1e-4, (max_rows, i, name)
                if not torch.equal(a, b):
                    unequal.append((max_rows, i, name))
    return unequal


VARIANTS = {"shipped": None, "num_cross_attn_layers=2": dict(num_cross_attn_layers=2), "n_attention_heads=4": dict(n_attention_heads=4),
            "include_residual_stream=False": dict(include_residual_stream=False)}
_UNEQUAL = {}


def _variant(key, pretrained, graphs):
    """`_model_case` of one model, run once for the two tests that share it -> its list of chunked vectors that are not
    bitwise the one-chunk vectors, as (max_rows, layer, name)."""
    if key not in _UNEQUAL:
        over = VARIANTS[key]
        if over is None:
            model = _joint()
            model.load_state_dict(pretrained, strict=True)
        else:
            torch.manual_seed(0)
            model = _joint(**over)
        _UNEQUAL[key] = _model_case(model, graphs, (over or {}).get("num_cross_attn_layers", 1))
    return _UNEQUAL[key]


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(VARIANTS))
def test_model_scores_equal_the_collated_batch(pretrained, graphs, deterministic, key):
    _variant(key, pretrained, graphs)


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(VARIANTS))
def test_chunked_vectors_are_bitwise_the_one_chunk_vectors(pretrained, graphs, deterministic, key):
    """max_rows = 150 and 80 (12 and 15 chunks) against one chunk, torch.equal for every vector of every layer.

    The first layer's vectors are computed from the rows of the unique graphs, which no chunking touches.  A later
    layer's queries and keys are per-pair rows that went through out-projections, feed-forwards and LayerNorms; on the
    pass that produces the affinities these are library GEMMs at the chunk's row count, and the second layer's vectors
    taken from it differed from chunking to chunking (239 - 483 of 520 / 668 elements in the last bits, rel_err <= 3.8e-7,
    with either LayerNorm kernel forced: it is the GEMMs).  [num_cross_attn_layers=2] holds the model to the row-count
    invariant pass that replaced it."""
    assert _variant(key, pretrained, graphs) == []


@pytest.mark.gpu
def test_contract(pretrained, graphs, monkeypatch):
    prots, drugs, pairs = graphs
    model = _joint()
    model.load_state_dict(pretrained, strict=True)
    model = model.to(DEV).train()
    model.attention_weights, model.node_attention = "always", "auto"
    marker = object()
    model.last_node_attention = marker
    dp, dm = _batch(prots), _batch(drugs)
    y, scores, optr = model.score_pairs_with_node_attention(dp, dm, pairs)
    assert model.training and all(m.training for m in model.modules())     # restored
    assert (model.attention_weights, model.node_attention) == ("always", "auto") and model.last_node_attention is marker
    assert not y.requires_grad and all(p.grad is None for p in model.parameters())
    assert not any(v.requires_grad for s in scores for v in s)
    y0, s0, (o1, o2) = model.score_pairs_with_node_attention(dp, dm, [])
    assert y0.shape == (0, 1) and len(s0) == 1 and all(v.shape == (0,) and v.dtype == torch.float32 for v in s0[0])
    assert o1.tolist() == [0] and o2.tolist() == [0]
    assert model.training
    with pytest.raises(RuntimeError, match="no cross-attention"):
        torch.manual_seed(0)
        _joint(num_cross_attn_layers=0).to(DEV).score_pairs_with_node_attention(dp, dm, pairs)
    # before any launch: no encoder, no entry point of the library
    ran = []
    torch.manual_seed(0)
    wide = _joint(residue_lin_depth=2).to(DEV)                              # residue width 256, 8 heads of 32
    assert wide.cross_attn_module.cross_attn_layers[0].embed1_to_2.embed_dim == 256
    assert wide.score_pairs(dp, dm, pairs).shape == (len(pairs), 1)         # (the affinities alone do run)
    hooks = [m.register_forward_pre_hook(lambda *a: ran.append("encoder"))
             for mod in (model, wide) for m in (mod.protein_gnn, mod.molecule_gnn)]
    monkeypatch.setattr(ps, "lib", lambda: ran.append("lib"))
    monkeypatch.setattr(pns, "lib", lambda: ran.append("lib"))
    try:
        with pytest.raises(NotImplementedError, match="128"):
            wide.score_pairs_with_node_attention(dp, dm, pairs)
        assert wide.training
        for bad in (pairs + [(3, 0)], pairs + [(0, 4)], [(-1, 0)]):
            with pytest.raises(IndexError):
                model.score_pairs_with_node_attention(dp, dm, bad)
    finally:
        for h in hooks:
            h.remove()
    assert ran == [] and model.training
