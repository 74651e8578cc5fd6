"""Scoring pair lists with every protein and every molecule encoded once (csrc/attn_pairs_kernels.hip,
include/caster_gvp_attnpairs.h, gvp_hip.pair_scoring, JointGNN.score_pairs).

REFERENCES.  The pair kernel: `caster_gvp::cross_attention` on the per-pair rows gathered with index_select, BITWISE
(a pair's arithmetic is the same instruction sequence on the same values wherever its rows lie; neither kernel uses
atomics).  `expand_rows`: index_select / repeat_interleave, bitwise.  The model: a plain eval forward over the same pairs
collated as an ordinary batch, |delta| <= 1e-4 * max(1, |prediction|) -- the project's forward bar; not bitwise, the
library GEMMs of the head run at other row counts."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import davis_synth as ds
from conftest import GOLDEN, REPO
from gvp_hip import _lib, attention_ops, pair_scoring as ps  # noqa: F401

DEV = "cuda:0"
BAD, UNSUPPORTED = -1, -2


def _ptr(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# CPU
def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(cgvp_[a-z0-9_]+)\s*\(", text))


def test_entry_points_have_a_header_and_a_version_of_their_own():
    header = os.path.join(REPO, "include", "caster_gvp_attnpairs.h")
    assert _declared(header) == set(ps.exported_symbols())
    assert set(ps.exported_symbols()) == {"cgvp_attn_pairs_version", "cgvp_attn_fwd_pairs", "cgvp_expand_rows"}
    main = open(os.path.join(REPO, "include", "caster_gvp.h")).read()
    handle = C.CDLL(_lib.LIB_PATH)
    for name in ps.exported_symbols():
        assert hasattr(handle, name), name
        assert name not in main and name not in _lib.exported_symbols(), name
    assert ps.lib().cgvp_attn_pairs_version() == 1 == ps.ATTN_PAIRS_VERSION
    assert "#define CGVP_ATTN_PAIRS_VERSION 1\n" in open(header).read()
    assert _lib.abi_header_digest() == _lib.ABI_HEADER_SHA256          # the main C ABI did not move


def _covers(chunks, g1, g2, len1, len2, max_rows):
    """what every plan must satisfy -> the chunk sizes"""
    at = 0
    for c in chunks:
        assert c.start == at and c.stop > c.start                       # once, in order, no empty chunk
        at = c.stop
        assert np.array_equal(c.g1, g1[c.start:c.stop]) and np.array_equal(c.g2, g2[c.start:c.stop])
        assert c.g1.dtype == c.g2.dtype == c.optr1.dtype == c.optr2.dtype == np.int64
        assert np.array_equal(c.optr1, _ptr(len1[c.g1])) and np.array_equal(c.optr2, _ptr(len2[c.g2]))
        assert (c.rows1, c.rows2) == (int(c.optr1[-1]), int(c.optr2[-1]))
        assert c.rows1 + c.rows2 <= max_rows or c.stop - c.start == 1
    assert at == len(g1)
    for a, b in zip(chunks[:-1], chunks[1:]):                           # greedy: the next pair did not fit any more
        assert a.rows1 + a.rows2 + len1[b.g1[0]] + len2[b.g2[0]] > max_rows
    return [c.stop - c.start for c in chunks]


def test_plan_pairs():
    len1, len2 = np.array([20, 33, 48, 0]), np.array([31, 28, 41, 0, 33])
    rng = np.random.default_rng(5)
    pairs = np.stack([rng.integers(0, 4, 40), rng.integers(0, 5, 40)], axis=1)
    for max_rows in (1, 60, 100, 250, 10 ** 6):
        sizes = _covers(ps.plan_pairs(len1, len2, pairs, max_rows), pairs[:, 0], pairs[:, 1], len1, len2, max_rows)
        print(max_rows, sizes)
    assert len(ps.plan_pairs(len1, len2, pairs, 10 ** 6)) == 1
    assert max(_covers(ps.plan_pairs(len1, len2, pairs, 100), pairs[:, 0], pairs[:, 1], len1, len2, 100)) > 1
    # a pair larger than the budget is a chunk of its own, between chunks that respect it
    big = ps.plan_pairs([5, 500, 5], [3], [[0, 0], [0, 0], [1, 0], [2, 0], [2, 0]], 20)
    assert [(c.start, c.stop) for c in big] == [(0, 2), (2, 3), (3, 5)] and big[1].rows1 == 500
    # None is the explicit protein-major product
    full, explicit = ps.plan_pairs(len1, len2, None, 300), ps.plan_pairs(len1, len2, [[p, d] for p in range(4) for d in range(5)], 300)
    assert len(full) == len(explicit) > 1
    for a, b in zip(full, explicit):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert np.array_equal(np.concatenate([c.g1 for c in full]), np.repeat(np.arange(4), 5))
    assert np.array_equal(np.concatenate([c.g2 for c in full]), np.tile(np.arange(5), 4))
    # lists, tensors and arrays are the same pair list
    assert all(np.array_equal(x, y) for a, b in zip(ps.plan_pairs(len1, len2, torch.as_tensor(pairs), 100),
                                                     ps.plan_pairs(len1, len2, pairs.tolist(), 100)) for x, y in zip(a, b))
    for bad in ([[-1, 0]], [[4, 0]], [[0, -1]], [[0, 5]], [[0, 0], [3, 4], [0, 5]]):
        with pytest.raises(IndexError):
            ps.plan_pairs(len1, len2, bad, 100)
    assert ps.plan_pairs(len1, len2, [], 100) == [] and ps.plan_pairs(len1, len2, np.zeros((0, 2), dtype=np.int64), 100) == []
    assert ps.plan_pairs([], len2, None, 100) == []


_TABLES = ("q_ptr", "k_ptr", "q_graph", "k_graph", "out_ptr")


def _bad_argument_cases():
    """(keyword changes of one call) -> expected code.  `p` is the valid address the other fields hold."""
    p = 0x1000
    cases = [(dict(nprob=0), BAD), (dict(nprob=3), BAD), (dict(heads=0), BAD), (dict(pairs=-1), BAD), (dict(pairs=1 << 30), BAD),
             (dict(problems=None), BAD)]
    for name in ("num_q_graphs", "num_k_graphs", "num_q", "num_k", "num_out"):
        cases.append(({name: -1}, BAD))
    for name in _TABLES:
        cases += [({name: 0}, BAD), ({name: p + 4}, BAD)]                 # NULL, not 8-byte aligned
    for name in ("q", "k", "v", "out"):
        cases += [({name: 0}, BAD), ({name: p + 8}, BAD)]                 # NULL with rows, not 16-byte aligned
    cases.append((dict(lse=p + 2), BAD))
    for name in ("num_q", "num_k", "num_out"):                            # side_ok at width 128: (rows + 16) * 128 < 2^31
        cases.append(({name: (1 << 24) - 16}, BAD))
    return cases


def test_entry_points_check_their_arguments_on_the_host():
    """CGVP_ERR_* before any launch and before the `num_pairs == 0` return: every call but the refused ones asks for zero
    pairs, so nothing here could launch even if a check were missing.  Pointers are never dereferenced."""
    L, p = ps.lib(), 0x1000
    ptr_fields = [n for n, t in ps.PairsProblem._fields_ if t is C.c_void_p]

    def call(nprob=2, pairs=0, heads=8, head_dim=16, which=1, problems=True, **kw):
        P = (ps.PairsProblem * 2)()
        for x in P:
            for n in ptr_fields:
                setattr(x, n, p)
            x.num_q_graphs, x.num_k_graphs, x.num_q, x.num_k, x.num_out = 3, 4, 32, 48, 64
        for n, val in kw.items():
            setattr(P[which], n, val)
        return L.cgvp_attn_fwd_pairs(P if problems else None, nprob, pairs, heads, head_dim, 0.25, None)

    assert call() == 0 and call(nprob=1) == 0 and call(head_dim=32) == 0 and call(head_dim=64) == 0
    for kw, code in _bad_argument_cases():
        kw = dict(kw)
        if "problems" in kw:
            kw["problems"] = False
        for which in (0, 1):
            assert call(which=which, **kw) == code, (which, kw)
            assert call(which=which, head_dim=48, **kw) == UNSUPPORTED, (which, kw)   # first of all
    for hd in (0, 8, 48, 128):
        assert call(head_dim=hd) == UNSUPPORTED
    assert call(lse=0) == 0                                                # the lse is optional
    assert call(num_q=0, q=0) == 0 and call(num_k=0, k=0, v=0) == 0 and call(num_out=0, out=0) == 0   # empty: no buffers
    assert call(num_q=(1 << 24) - 17) == 0 and call(num_q=(1 << 23) - 16, head_dim=32) == BAD

    def expand(src=p, src_ptr=p, graph=p, out_ptr=p, pairs=0, num_out=64, width=128, out=p, batch=p):
        return L.cgvp_expand_rows(src, src_ptr, graph, out_ptr, pairs, num_out, width, out, batch, None)

    assert expand() == 0 and expand(batch=0) == 0 and expand(width=4) == 0 and expand(num_out=0, src=0, out=0) == 0
    for kw in (dict(pairs=-1), dict(pairs=1 << 30), dict(num_out=-1), dict(num_out=1 << 33), dict(width=0), dict(width=2),
               dict(width=130), dict(width=-4), dict(src=0), dict(out=0), dict(src_ptr=0), dict(graph=0), dict(out_ptr=0),
               dict(src=p + 8), dict(out=p + 4), dict(src_ptr=p + 4), dict(graph=p + 4), dict(out_ptr=p + 4), dict(batch=p + 4)):
        assert expand(**kw) == BAD, kw


def test_fake_kernels_and_the_gradient_refusal():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        f = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device="cuda")
        i = lambda n: f(n, dt=torch.long)
        args = (f(70, 128), f(9, 128), f(9, 128), f(9, 256), f(70, 256), f(70, 256), i(4), i(3), i(5), i(5), i(6), i(6), 8)
        o1, o2 = torch.ops.caster_gvp.cross_attention_pairs(*args, 100, 20)
        assert (tuple(o1.shape), tuple(o2.shape)) == ((100, 128), (20, 256)) and o1.dtype == o2.dtype == torch.float32
        outs = torch.ops.caster_gvp.cross_attention_pairs_lse(*args, 100, 20)
        assert [tuple(t.shape) for t in outs] == [(100, 128), (20, 256), (100, 8), (20, 8)]
        rows, batch = torch.ops.caster_gvp.expand_rows(f(70, 64), i(4), i(5), i(6), 100)
        assert tuple(rows.shape) == (100, 64) and tuple(batch.shape) == (100,) and batch.dtype == torch.int64
    # no autograd formula: an input that requires grad while gradients are recorded is refused before anything else
    z = lambda *s: torch.zeros(*s)
    t = lambda n: torch.zeros(n, dtype=torch.long)
    leaf = torch.zeros(4, 128, requires_grad=True)
    with pytest.raises(RuntimeError, match="inference only"):
        ps.cross_attention_pairs(leaf, z(2, 128), z(2, 128), z(2, 128), z(4, 128), z(4, 128), t(2), t(2), t(1), t(1), t(2), t(2), 8, 4, 2)
    with pytest.raises(RuntimeError, match="inference only"):
        ps.expand_rows(leaf, t(2), t(1), t(2), 4)
    with torch.no_grad(), pytest.raises(RuntimeError) as e:                    # past the refusal: there is no CPU kernel
        ps.expand_rows(leaf, t(2), t(1), t(2), 4)
    assert "inference only" not in str(e.value)


def _joint(**over):
    from models.joint_gnn import JointGNN
    kw = json.load(open(os.path.join(GOLDEN, "model_kwargs.json")))
    return JointGNN(protein_gnn_kwargs=kw["protein_gnn_kwargs"], molecule_gnn_kwargs=kw["molecule_gnn_kwargs"],
                    **dict(kw["joint_gnn_kwargs"], **over))


def test_score_pairs_refuses_cpu_batches():
    model = _joint()
    p, m = ds.pair_batch(2, 3, lengths=[20, 33])
    with pytest.raises(NotImplementedError, match="CUDA"):
        model.score_pairs(ds.to_torch(p), ds.to_torch(m))
    assert model.training                                                  # untouched


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the kernels
LEN1, LEN2 = [17, 0, 16, 33], [1, 15, 0, 16, 40]      # the unique graphs of side 1 (4) and side 2 (5)


def _pair_list():
    """70 pairs with repetition (locate's second 64-pair chunk): consecutive repeats of one graph, the first and the last
    graph of each side, the empty graph of each side as query and as key, then a seeded draw."""
    head = [(0, 0), (0, 0), (0, 1), (3, 4), (3, 4), (2, 4), (1, 2), (1, 0), (0, 2), (3, 2), (2, 3), (2, 3), (1, 4), (3, 0)]
    rng = np.random.default_rng(17)
    rest = [(int(a), int(b)) for a, b in zip(rng.integers(0, 4, 70 - len(head)), rng.integers(0, 5, 70 - len(head)))]
    pairs = np.array(head + rest[:-2] + [(3, 4), (0, 0)], dtype=np.int64)
    assert pairs.shape == (70, 2)
    return pairs


def _tables():
    pairs = _pair_list()
    (chunk,) = ps.plan_pairs(LEN1, LEN2, pairs, 10 ** 9)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    t = dict(ptr1=dev(_ptr(LEN1)), ptr2=dev(_ptr(LEN2)), g1=dev(chunk.g1), g2=dev(chunk.g2), optr1=dev(chunk.optr1),
             optr2=dev(chunk.optr2), rows1=chunk.rows1, rows2=chunk.rows2)
    # the rows of every pair, gathered: what the batch kernels need
    rows = lambda ptr, g: np.concatenate([np.arange(ptr[x], ptr[x + 1]) for x in g] + [np.zeros(0, dtype=np.int64)])
    t["idx1"], t["idx2"] = dev(rows(_ptr(LEN1), chunk.g1)), dev(rows(_ptr(LEN2), chunk.g2))
    t["batch1"] = dev(np.repeat(np.arange(70), np.asarray(LEN1)[chunk.g1]))
    t["batch2"] = dev(np.repeat(np.arange(70), np.asarray(LEN2)[chunk.g2]))
    return t


@pytest.fixture(scope="module")
def tables():
    return _tables()


@pytest.mark.gpu
@pytest.mark.parametrize("heads,w1,w2", [(8, 128, 128), (4, 128, 128), (2, 128, 128), (8, 128, 256)],
                         ids=["8x16", "4x32", "2x64", "8x16_and_8x32"])
def test_pair_kernel_equals_the_batch_kernel_bitwise(tables, heads, w1, w2):
    t = tables
    g = torch.Generator().manual_seed(100 + heads + w2)
    N1, N2 = sum(LEN1), sum(LEN2)
    q1, k1, v1, q2, k2, v2 = [torch.randn(n, w, generator=g).to(DEV)
                              for n, w in ((N1, w1), (N2, w1), (N2, w1), (N2, w2), (N1, w2), (N1, w2))]
    got = ps.cross_attention_pairs(q1, k1, v1, q2, k2, v2, t["ptr1"], t["ptr2"], t["g1"], t["g2"], t["optr1"], t["optr2"],
                                   heads, t["rows1"], t["rows2"], lse=True)
    sel = lambda x, idx: torch.index_select(x, 0, idx)
    want = torch.ops.caster_gvp.cross_attention(sel(q1, t["idx1"]), sel(k1, t["idx2"]), sel(v1, t["idx2"]), sel(q2, t["idx2"]),
                                                sel(k2, t["idx1"]), sel(v2, t["idx1"]), t["optr1"], t["optr2"], heads)
    plain = ps.cross_attention_pairs(q1, k1, v1, q2, k2, v2, t["ptr1"], t["ptr2"], t["g1"], t["g2"], t["optr1"], t["optr2"], heads)
    torch.cuda.synchronize()
    assert got[0].shape == (t["rows1"], w1) and got[1].shape == (t["rows2"], w2)
    for name, a, b in zip(("o1", "o2", "lse1", "lse2"), got, want):
        assert a.shape == b.shape and a.dtype == b.dtype == torch.float32, name
        assert not torch.isnan(a).any(), name
        print(f"{name}: {tuple(a.shape)}, differing elements {int((a != b).sum())}")
        assert torch.equal(a, b), name
    assert len(plain) == 2 and torch.equal(plain[0], got[0]) and torch.equal(plain[1], got[1])   # row totals read back
    # pairs without keys: zero rows and an lse of -inf, in both directions
    optr1, optr2, g1, g2 = (t[k].cpu().numpy() for k in ("optr1", "optr2", "g1", "g2"))
    seen = [0, 0]
    for b in range(70):
        if LEN2[g2[b]] == 0 and LEN1[g1[b]] > 0:
            rows = slice(optr1[b], optr1[b + 1])
            assert (got[0][rows] == 0).all() and (got[2][rows] == float("-inf")).all()
            seen[0] += 1
        if LEN1[g1[b]] == 0 and LEN2[g2[b]] > 0:
            rows = slice(optr2[b], optr2[b + 1])
            assert (got[1][rows] == 0).all() and (got[3][rows] == float("-inf")).all()
            seen[1] += 1
    assert min(seen) > 0
    assert torch.isfinite(got[2]).any() and torch.isfinite(got[3]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("width", [4, 128])
def test_expand_rows(tables, width):
    t = tables
    g = torch.Generator().manual_seed(width)
    for src, ptr, gi, optr, n, idx, batch in ((torch.randn(sum(LEN1), width, generator=g).to(DEV), t["ptr1"], t["g1"], t["optr1"],
                                               t["rows1"], t["idx1"], t["batch1"]),
                                              (torch.randn(sum(LEN2), width, generator=g).to(DEV), t["ptr2"], t["g2"], t["optr2"],
                                               t["rows2"], t["idx2"], t["batch2"])):
        rows, b = ps.expand_rows(src, ptr, gi, optr, n)
        torch.cuda.synchronize()
        assert rows.shape == (n, width) and b.shape == (n,) and b.dtype == torch.int64
        assert torch.equal(rows, torch.index_select(src, 0, idx))
        assert torch.equal(b, batch)                                       # a pair of length 0 contributes nothing
        assert torch.equal(b, torch.repeat_interleave(torch.arange(70, device=DEV), optr[1:] - optr[:-1]))


@pytest.mark.gpu
def test_refused_calls_launch_nothing(tables):
    """Every CGVP_ERR_* case on a call that WOULD launch (70 pairs, real buffers): the code is returned and the
    sentinel-filled outputs are untouched.  (No out-of-range device index is tried: the tables are the valid ones.)"""
    from gvp_hip.ops import _stream
    t, L, SENTINEL = tables, ps.lib(), -7.0
    g = torch.Generator().manual_seed(9)
    N1, N2 = sum(LEN1), sum(LEN2)
    q1, k1, v1, q2, k2, v2 = [torch.randn(n, 128, generator=g).to(DEV) for n in (N1, N2, N2, N2, N1, N1)]
    outs = [torch.full((t["rows1"], 128), SENTINEL, device=DEV), torch.full((t["rows2"], 128), SENTINEL, device=DEV),
            torch.full((t["rows1"], 8), SENTINEL, device=DEV), torch.full((t["rows2"], 8), SENTINEL, device=DEV)]

    def call(nprob=2, pairs=70, heads=8, head_dim=16, which=1, problems=True, **kw):
        P = (ps.PairsProblem * 2)()
        for x, (q, k, v, qp, kp, qg, kg, op, o, lse) in zip(P, (
                (q1, k1, v1, "ptr1", "ptr2", "g1", "g2", "optr1", outs[0], outs[2]),
                (q2, k2, v2, "ptr2", "ptr1", "g2", "g1", "optr2", outs[1], outs[3]))):
            x.q, x.k, x.v, x.out, x.lse = (a.data_ptr() for a in (q, k, v, o, lse))
            x.q_ptr, x.k_ptr, x.q_graph, x.k_graph, x.out_ptr = (t[n].data_ptr() for n in (qp, kp, qg, kg, op))
            x.num_q_graphs, x.num_k_graphs = t[qp].numel() - 1, t[kp].numel() - 1
            x.num_q, x.num_k, x.num_out = q.shape[0], k.shape[0], o.shape[0]
        for n, val in kw.items():
            base = getattr(P[which], n) if n in _TABLES + ("q", "k", "v", "out", "lse") and val else 0
            setattr(P[which], n, base + (val - 0x1000 if base else val))   # (an offset from the case's nominal address)
        return L.cgvp_attn_fwd_pairs(P if problems else None, nprob, pairs, heads, head_dim, 0.25, _stream())

    for kw, code in _bad_argument_cases():
        kw = dict(kw)
        if "problems" in kw:
            kw["problems"] = False
        for which in (0, 1):
            assert call(which=which, **kw) == code, (which, kw)
            assert call(which=which, head_dim=48, **kw) == UNSUPPORTED, (which, kw)
    assert call(head_dim=48) == UNSUPPORTED
    src = torch.randn(N1, 128, generator=g).to(DEV)
    rows, batch = torch.full((t["rows1"], 128), SENTINEL, device=DEV), torch.full((t["rows1"],), -7, dtype=torch.int64, device=DEV)
    ex = lambda **kw: L.cgvp_expand_rows(*[kw.get(n, d) for n, d in (
        ("src", src.data_ptr()), ("src_ptr", t["ptr1"].data_ptr()), ("graph", t["g1"].data_ptr()), ("out_ptr", t["optr1"].data_ptr()),
        ("pairs", 70), ("num_out", t["rows1"]), ("width", 128), ("out", rows.data_ptr()), ("batch", batch.data_ptr()))], _stream())
    for kw in (dict(pairs=-1), dict(num_out=-1), dict(width=2), dict(width=130), dict(src=0), dict(out=0), dict(src_ptr=0),
               dict(graph=0), dict(out_ptr=0), dict(src=src.data_ptr() + 8), dict(out=rows.data_ptr() + 4),
               dict(graph=t["g1"].data_ptr() + 4), dict(batch=batch.data_ptr() + 4)):
        assert ex(**kw) == BAD, kw
    torch.cuda.synchronize()
    for o in outs + [rows]:
        assert (o == SENTINEL).all()
    assert (batch == -7).all()
    assert call() == 0 and ex() == 0                                       # the same calls, unmodified, do run
    torch.cuda.synchronize()
    assert not (outs[0] == SENTINEL).any() and not (rows == SENTINEL).any() and (batch >= 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the model
PROT_LENGTHS = [20, 33, 48]


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


def _close(got, want, what):
    bound = 1e-4 * want.abs().clamp_min(1.0)
    diff = (got - want).abs()
    print(f"{what}: max |delta| {float(diff.max()):.3e}, max |prediction| {float(want.abs().max()):.3e}")
    assert got.shape == want.shape and torch.isfinite(got).all(), what
    assert (diff <= bound).all(), what


def _model_case(model, graphs):
    prots, drugs, pairs = graphs
    model = model.to(DEV).eval()
    dp, dm = _batch(prots), _batch(drugs)
    with torch.no_grad():
        want = model(_batch([prots[p] for p, _ in pairs]), _batch([drugs[d] for _, d in pairs]))[0]
    got = model.score_pairs(dp, dm, pairs)
    assert got.shape == (len(pairs), 1) and not got.requires_grad
    _close(got, want, "one chunk")
    # at least three chunks: a budget with chunks of one pair and of several, and one that some single pairs exceed
    len2 = [g["x_s"].shape[0] for g in drugs]
    for max_rows in (150, 80):
        plan = ps.plan_pairs(PROT_LENGTHS, len2, pairs, max_rows)
        sizes, over = [c.stop - c.start for c in plan], [c.rows1 + c.rows2 > max_rows for c in plan]
        assert len(plan) >= 3 and 1 in sizes, sizes
        assert (max(sizes) > 1 and not any(over)) if max_rows == 150 else (any(over) and not all(over)), (sizes, over)
        chunked = model.score_pairs(dp, dm, torch.tensor(pairs, device=DEV), max_rows=max_rows)
        _close(chunked, want, f"{len(plan)} chunks")
        _close(chunked, got, f"{len(plan)} chunks against one chunk")
    # `batch` instead of `ptr`, and the full product
    full = model.score_pairs(_batch(prots, ptr=False), _batch(drugs, ptr=False))
    index = torch.tensor([p * 4 + d for p, d in pairs], device=DEV)
    _close(full[index], want, "full product")
    return model


@pytest.mark.gpu
def test_model_scores_equal_the_expanded_batch(pretrained, graphs):
    model = _joint()
    model.load_state_dict(pretrained, strict=True)
    _model_case(model, graphs)


@pytest.mark.gpu
@pytest.mark.parametrize("over", [dict(num_cross_attn_layers=2), dict(n_attention_heads=4), dict(include_residual_stream=False),
                                  dict(num_cross_attn_layers=0)], ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_model_variants_equal_the_expanded_batch(graphs, over):
    torch.manual_seed(0)
    _model_case(_joint(**over), graphs)


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
    y = model.score_pairs(dp, dm, pairs)
    assert model.training and all(m.training for m in model.modules())     # restored
    assert (model.attention_weights, model.node_attention) == ("always", "auto") and model.last_node_attention is marker
    assert not y.requires_grad and all(p.grad is None for p in model.parameters())
    assert model.score_pairs(dp, dm, []).shape == (0, 1)
    model.eval()
    _close(model.score_pairs(dp, dm, pairs), y, "eval against train mode")  # the flag changes nothing (pooling adds
                                                                           # with float atomics: not bitwise)
    assert not model.training
    with pytest.raises(NotImplementedError):
        model.score_pairs(ds.to_torch(ds.collate(prots)), ds.to_torch(ds.collate(drugs)), pairs)    # CPU dicts
    torch.manual_seed(0)
    narrow = _joint(n_attention_heads=16).to(DEV)                          # head_dim 8: the dense path of forward()
    with pytest.raises(NotImplementedError):
        narrow.score_pairs(dp, dm, pairs)
    assert narrow.training
    # an index equal to P: IndexError before anything runs -- no encoder, no entry point of the library
    ran = []
    hooks = [m.register_forward_pre_hook(lambda *a: ran.append("encoder")) for m in (model.protein_gnn, model.molecule_gnn)]
    monkeypatch.setattr(ps, "lib", lambda: ran.append("lib"))
    try:
        for bad in (pairs + [(3, 0)], pairs + [(0, 4)], [(-1, 0)]):
            with pytest.raises(IndexError):
                model.score_pairs(dp, dm, bad)
    finally:
        for h in hooks:
            h.remove()
    assert ran == [] and not model.training
