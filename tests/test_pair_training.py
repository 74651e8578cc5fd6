"""Training on pair lists with every protein and every molecule encoded once (csrc/attn_pairs_bwd_kernels.hip,
include/caster_gvp_pairtrain.h, gvp_hip.pair_training, JointGNN.forward_pairs).

REFERENCES.  The forward of `cross_attention_pairs_train` / `expand_rows_train`: the inference ops of
gvp_hip.pair_scoring, BITWISE (the same entry points).  The attention gradients: an fp64 dense softmax attention per
pair on the CPU with autograd through index_select of the unique rows; the yardstick beside it is the existing batch
path (index_select on the device -> caster_gvp::cross_attention -> its backward, index_select's own backward doing the
sum): relative error new <= 2 x yardstick + 1e-6 -- both do the same fp32 arithmetic with another order of summation
over at most about 20 referencing pairs.  `expand_rows_train`'s backward: index_add_ on integer-valued floats, bitwise.
The model: `score_pairs` (predictions, bitwise) and a plain forward + backward over the same pairs collated as an
ordinary batch (parameter gradients within relative 2e-4, the project's gradient bar)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import davis_synth as ds
from conftest import GOLDEN, REPO
from gvp_hip import _lib, attention_ops, pair_scoring as ps, pair_training as pt  # noqa: F401

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
    header = os.path.join(REPO, "include", "caster_gvp_pairtrain.h")
    assert _declared(header) == set(pt.exported_symbols())
    assert set(pt.exported_symbols()) == {"cgvp_pair_train_version", "cgvp_attn_bwd_pairs_floats", "cgvp_attn_bwd_pairs",
                                          "cgvp_reduce_rows"}
    main = open(os.path.join(REPO, "include", "caster_gvp.h")).read()
    pairs_header = os.path.join(REPO, "include", "caster_gvp_attnpairs.h")
    handle = C.CDLL(_lib.LIB_PATH)
    for name in pt.exported_symbols():
        assert hasattr(handle, name), name
        assert name not in main and name not in _lib.exported_symbols() and name not in ps.exported_symbols(), name
        assert name not in open(pairs_header).read(), name
    assert pt.lib().cgvp_pair_train_version() == 1 == pt.PAIR_TRAIN_VERSION
    assert "#define CGVP_PAIR_TRAIN_VERSION 1\n" in open(header).read()
    # the attention-pairs header and its version did not move, nor did the main C ABI
    assert _declared(pairs_header) == {"cgvp_attn_pairs_version", "cgvp_attn_fwd_pairs", "cgvp_expand_rows"}
    assert ps.lib().cgvp_attn_pairs_version() == 1 and "#define CGVP_ATTN_PAIRS_VERSION 1\n" in open(pairs_header).read()
    assert _lib.abi_header_digest() == _lib.ABI_HEADER_SHA256


def _check_plan(plan, g1, g2, len1, len2):
    len1, len2 = np.asarray(len1, dtype=np.int64), np.asarray(len2, dtype=np.int64)
    K = len(g1)
    assert all(getattr(plan, n).dtype == np.int64 for n in pt.TABLES)
    assert np.array_equal(plan.g1, g1) and np.array_equal(plan.g2, g2)
    assert np.array_equal(plan.optr1, _ptr(len1[g1])) and np.array_equal(plan.optr2, _ptr(len2[g2]))
    assert (plan.rows1, plan.rows2) == (int(plan.optr1[-1]), int(plan.optr2[-1]))
    for g, G, ip, ii in ((g1, len(len1), plan.inv1_ptr, plan.inv1_pairs), (g2, len(len2), plan.inv2_ptr, plan.inv2_pairs)):
        assert ip.shape == (G + 1,) and ii.shape == (K,) and ip[0] == 0 and ip[-1] == K and (np.diff(ip) >= 0).all()
        for x in range(G):
            mine = ii[ip[x]:ip[x + 1]]
            assert (np.diff(mine) > 0).all()                            # ascending pair index
            assert np.array_equal(mine, np.nonzero(np.asarray(g) == x)[0])
        assert np.array_equal(np.sort(ii), np.arange(K))                # the ranges together: a permutation of 0 .. K-1


def test_plan_pair_training():
    len1, len2 = [20, 0, 48, 7], [31, 28, 0]
    # a hand-written list with repeats; protein 3 and molecule 1 are referenced by no pair; graphs 1 / 2 are empty
    pairs = [[0, 0], [2, 2], [0, 0], [1, 0], [2, 0], [0, 2]]
    plan = pt.plan_pair_training(len1, len2, pairs)
    assert plan.inv1_ptr.tolist() == [0, 3, 4, 6, 6] and plan.inv1_pairs.tolist() == [0, 2, 5, 3, 1, 4]
    assert plan.inv2_ptr.tolist() == [0, 4, 4, 6] and plan.inv2_pairs.tolist() == [0, 2, 3, 4, 1, 5]
    assert plan.optr1.tolist() == [0, 20, 68, 88, 88, 136, 156] and plan.optr2.tolist() == [0, 31, 31, 62, 93, 124, 124]
    assert (plan.rows1, plan.rows2) == (156, 124)
    _check_plan(plan, [p[0] for p in pairs], [p[1] for p in pairs], len1, len2)
    # None is the explicit protein-major product
    full = pt.plan_pair_training(len1, len2, None)
    explicit = pt.plan_pair_training(len1, len2, [[p, d] for p in range(4) for d in range(3)])
    assert all(np.array_equal(a, b) for a, b in zip(full, explicit))
    _check_plan(full, np.repeat(np.arange(4), 3), np.tile(np.arange(3), 4), len1, len2)
    # lists, tensors and arrays are the same pair list
    assert all(np.array_equal(a, b) for a, b in zip(plan, pt.plan_pair_training(len1, len2, torch.tensor(pairs))))
    assert all(np.array_equal(a, b) for a, b in zip(plan, pt.plan_pair_training(len1, len2, np.asarray(pairs, dtype=np.int32))))
    # K = 0: every table of pairs is empty, every inverse range too
    for empty in ([], np.zeros((0, 2), dtype=np.int64)):
        e = pt.plan_pair_training(len1, len2, empty)
        assert e.g1.shape == e.g2.shape == e.inv1_pairs.shape == e.inv2_pairs.shape == (0,)
        assert e.optr1.tolist() == e.optr2.tolist() == [0] and (e.rows1, e.rows2) == (0, 0)
        assert e.inv1_ptr.tolist() == [0] * 5 and e.inv2_ptr.tolist() == [0] * 4
    assert pt.plan_pair_training([], len2, None).g1.shape == (0,)
    for bad in ([[-1, 0]], [[4, 0]], [[0, -1]], [[0, 3]], [[0, 0], [3, 2], [0, 3]]):
        with pytest.raises(IndexError):
            pt.plan_pair_training(len1, len2, bad)
    for bad in ([[0.0, 1.0]], np.array([[0.5, 1]]), torch.tensor([[0.0, 1.0]])):
        with pytest.raises(TypeError):
            pt.plan_pair_training(len1, len2, bad)
    # random lists
    rng = np.random.default_rng(11)
    for K in (1, 7, 64, 200):
        l1, l2 = rng.integers(0, 40, 6), rng.integers(0, 40, 9)
        pr = np.stack([rng.integers(0, 6, K), rng.integers(0, 9, K)], axis=1)
        _check_plan(pt.plan_pair_training(l1, l2, pr), pr[:, 0], pr[:, 1], l1, l2)


_TABLES = ("q_ptr", "k_ptr", "q_graph", "k_graph", "out_ptr", "kout_ptr", "q_inv_ptr", "q_inv_pairs", "k_inv_ptr", "k_inv_pairs")
_ROWS16 = ("q", "k", "v", "out", "g_out", "g_q", "g_k", "g_v")


def _bad_argument_cases():
    """(keyword changes of one call) -> expected code.  `p` is the valid address the other fields hold."""
    p = 0x1000
    cases = [(dict(nprob=0), BAD), (dict(nprob=3), BAD), (dict(heads=0), BAD), (dict(pairs=-1), BAD), (dict(pairs=1 << 30), BAD),
             (dict(problems=None), BAD), (dict(ws=0), BAD), (dict(ws=8), BAD), (dict(ws_floats=-1), BAD)]
    for name in ("num_q_graphs", "num_k_graphs", "num_q", "num_k", "num_out", "num_kout"):
        cases.append(({name: -1}, BAD))
    for name in _TABLES:
        cases += [({name: 0}, BAD), ({name: p + 4}, BAD)]                 # NULL, not 8-byte aligned
    for name in _ROWS16:
        cases += [({name: 0}, BAD), ({name: p + 8}, BAD)]                 # NULL with rows, not 16-byte aligned
    cases += [(dict(lse=0), BAD), (dict(lse=p + 2), BAD)]
    for name in ("num_q", "num_k", "num_out", "num_kout"):                # side_ok at width 128: (rows + 16) * 128 < 2^31
        cases.append(({name: (1 << 24) - 16}, BAD))
    return cases


def test_entry_points_check_their_arguments_on_the_host():
    """CGVP_ERR_* before any launch: every call but the refused ones asks for zero pairs over zero graphs, where there is
    nothing to launch, so nothing here could launch even if a check were missing.  Pointers are never dereferenced."""
    L, p = pt.lib(), 0x1000
    ptr_fields = [n for n, t in pt.PairsBwdProblem._fields_ if t is C.c_void_p]

    def problems(which, kw):
        P = (pt.PairsBwdProblem * 2)()
        for x in P:
            for n in ptr_fields:
                setattr(x, n, p)
            x.num_q_graphs, x.num_k_graphs, x.num_q, x.num_k, x.num_out, x.num_kout = 0, 0, 32, 48, 64, 80
        for n, val in kw.items():
            setattr(P[which], n, val)
        return P

    def call(nprob=2, pairs=0, heads=8, head_dim=16, which=1, problems_=True, ws=p, ws_floats=1 << 40, **kw):
        P = problems(which, kw)
        return L.cgvp_attn_bwd_pairs(P if problems_ else None, nprob, pairs, heads, head_dim, 0.25, ws, ws_floats, None)

    assert call() == 0 and call(nprob=1) == 0 and call(head_dim=32) == 0 and call(head_dim=64) == 0
    for kw, code in _bad_argument_cases():
        kw = dict(kw)
        if "problems" in kw:
            kw["problems_"] = bool(kw.pop("problems"))
        for which in (0, 1):
            assert call(which=which, **kw) == code, (which, kw)
            assert call(which=which, head_dim=48, **kw) == UNSUPPORTED, (which, kw)   # first of all
    for hd in (0, 8, 48, 128):
        assert call(head_dim=hd) == UNSUPPORTED
    assert call(num_q=0, q=0, g_q=0) == 0 and call(num_k=0, k=0, v=0, g_k=0, g_v=0) == 0     # empty: no buffers
    assert call(num_out=0, out=0, lse=0, g_out=0) == 0
    assert call(num_q=(1 << 24) - 17) == 0 and call(num_q=(1 << 23) - 16, head_dim=32) == BAD
    # the workspace: what the query function says, no less
    floats = lambda nprob=2, heads=8, hd=16, which=1, ok=True, **kw: L.cgvp_attn_bwd_pairs_floats(
        problems(which, kw) if ok else None, nprob, heads, hd)
    need = floats()
    assert need == 2 * (64 * 128 + 2 * 80 * 128 + 64 * 8) and need % 4 == 0
    assert floats(nprob=1) == need // 2 and floats(hd=64) == 2 * (64 * 512 + 2 * 80 * 512 + 64 * 8)
    assert floats(heads=3, num_out=1, num_kout=0, nprob=1, which=0) == 48 + 4          # delta padded to 16 bytes
    assert call(ws_floats=need) == 0 and call(ws_floats=need - 1) == BAD
    assert call(num_out=0, num_kout=0, out=0, lse=0, g_out=0, nprob=1, which=0, ws=0, ws_floats=0) == 0   # no need, no workspace
    assert floats(hd=48) == UNSUPPORTED and floats(ok=False, hd=48) == UNSUPPORTED
    for kw in (dict(ok=False), dict(nprob=0), dict(nprob=3), dict(heads=0), dict(num_out=-1), dict(num_kout=-1)):
        assert floats(**kw) == BAD, kw

    def reduce(part=p, optr=p, inv_ptr=p, inv_pairs=p, src_ptr=p, graphs=0, pairs=0, num_part=64, num_dst=32, width=128, dst=p):
        return L.cgvp_reduce_rows(part, optr, inv_ptr, inv_pairs, src_ptr, graphs, pairs, num_part, num_dst, width, dst, None)

    assert reduce() == 0 and reduce(width=4) == 0 and reduce(num_part=0, part=0) == 0 and reduce(num_dst=0, dst=0) == 0
    for kw in (dict(graphs=-1), dict(graphs=1 << 30), dict(pairs=-1), dict(pairs=1 << 30), dict(num_part=-1), dict(num_part=1 << 33),
               dict(num_dst=-1), dict(num_dst=1 << 33), dict(width=0), dict(width=2), dict(width=130), dict(width=-4),
               dict(part=0), dict(dst=0), dict(optr=0), dict(inv_ptr=0), dict(inv_pairs=0), dict(src_ptr=0), dict(part=p + 8),
               dict(dst=p + 4), dict(optr=p + 4), dict(inv_ptr=p + 4), dict(inv_pairs=p + 4), dict(src_ptr=p + 4)):
        assert reduce(**kw) == BAD, kw


def test_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        f = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device="cuda")
        i = lambda n: f(n, dt=torch.long)
        ops = (f(70, 128), f(9, 128), f(9, 128), f(9, 256), f(70, 256), f(70, 256))
        tabs = (i(4), i(3), i(5), i(5), i(6), i(6), i(4), i(5), i(3), i(5))
        outs = torch.ops.caster_gvp.cross_attention_pairs_train(*ops, *tabs, 8, 100, 20)
        assert [tuple(t.shape) for t in outs] == [(100, 128), (20, 256), (100, 8), (20, 8)]
        assert all(t.dtype == torch.float32 for t in outs)
        o1, o2 = pt.cross_attention_pairs_train(*ops, *tabs, 8, 100, 20)
        assert (tuple(o1.shape), tuple(o2.shape)) == ((100, 128), (20, 256))
        grads = torch.ops.caster_gvp.cross_attention_pairs_backward(f(100, 128), f(20, 256), *ops, *outs, *tabs, 8)
        assert [tuple(t.shape) for t in grads] == [tuple(t.shape) for t in ops] and all(t.dtype == torch.float32 for t in grads)
        rows, batch = torch.ops.caster_gvp.expand_rows_train(f(70, 64), i(4), i(5), i(6), i(4), i(5), 100)
        assert tuple(rows.shape) == (100, 64) and rows.dtype == torch.float32
        assert tuple(batch.shape) == (100,) and batch.dtype == torch.int64
        g_src = torch.ops.caster_gvp.expand_rows_backward(f(100, 64), i(4), i(6), i(4), i(5), 70)
        assert tuple(g_src.shape) == (70, 64) and g_src.dtype == torch.float32


def _joint(**over):
    from models.joint_gnn import JointGNN
    kw = json.load(open(os.path.join(GOLDEN, "model_kwargs.json")))
    return JointGNN(protein_gnn_kwargs=kw["protein_gnn_kwargs"], molecule_gnn_kwargs=kw["molecule_gnn_kwargs"],
                    **dict(kw["joint_gnn_kwargs"], **over))


def test_forward_pairs_refuses_cpu_batches_and_the_inference_ops_still_refuse_gradients():
    model = _joint()
    p, m = ds.pair_batch(2, 3, lengths=[20, 33])
    for mode in (True, False):
        model.train(mode)
        with pytest.raises(NotImplementedError, match="CUDA"):
            model.forward_pairs(ds.to_torch(p), ds.to_torch(m))
        assert model.training == mode and all(x.training == mode for x in model.modules())     # untouched
    z = lambda *s: torch.zeros(*s)
    t = lambda n: torch.zeros(n, dtype=torch.long)
    leaf = torch.zeros(4, 128, requires_grad=True)
    with pytest.raises(RuntimeError, match="inference only"):
        ps.cross_attention_pairs(leaf, z(2, 128), z(2, 128), z(2, 128), z(4, 128), z(4, 128), t(2), t(2), t(1), t(1), t(2), t(2), 8, 4, 2)
    with pytest.raises(RuntimeError, match="inference only"):
        ps.expand_rows(leaf, t(2), t(1), t(2), 4)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the kernels
LEN1, LEN2 = [17, 0, 16, 33, 5], [1, 15, 0, 16, 40, 3]      # the last graph of each side is referenced by no pair
HEAD_SHAPES = [(8, 128, 128), (4, 128, 128), (2, 128, 128), (8, 128, 256)]
HEAD_IDS = ["8x16", "4x32", "2x64", "8x16_and_8x32"]


def _pair_list():
    """The 70 pairs of test_pair_scoring: consecutive repeats of one graph, the first and the last REFERENCED graph of each
    side, the empty graph of each side as query and as key, more than 64 pairs (locate's second trip)."""
    head = [(0, 0), (0, 0), (0, 1), (3, 4), (3, 4), (2, 4), (1, 2), (1, 0), (0, 2), (3, 2), (2, 3), (2, 3), (1, 4), (3, 0)]
    rng = np.random.default_rng(17)
    rest = [(int(a), int(b)) for a, b in zip(rng.integers(0, 4, 70 - len(head)), rng.integers(0, 5, 70 - len(head)))]
    pairs = np.array(head + rest[:-2] + [(3, 4), (0, 0)], dtype=np.int64)
    assert pairs.shape == (70, 2) and pairs[:, 0].max() == 3 and pairs[:, 1].max() == 4
    return pairs


def _tables_of(pairs, LEN1=LEN1, LEN2=LEN2):
    plan = pt.plan_pair_training(LEN1, LEN2, pairs)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    t = dict(pt.upload(plan, DEV), ptr1=dev(_ptr(LEN1)), ptr2=dev(_ptr(LEN2)), rows1=plan.rows1, rows2=plan.rows2, plan=plan)
    rows = lambda ptr, g: np.concatenate([np.arange(ptr[x], ptr[x + 1]) for x in g] + [np.zeros(0, dtype=np.int64)])
    t["idx1"], t["idx2"] = dev(rows(_ptr(LEN1), plan.g1)), dev(rows(_ptr(LEN2), plan.g2))
    return t


@pytest.fixture(scope="module")
def tables():
    return _tables_of(_pair_list())


def _table_args(t):
    return tuple(t[n] for n in ("ptr1", "ptr2", "g1", "g2", "optr1", "optr2", "inv1_ptr", "inv1_pairs", "inv2_ptr", "inv2_pairs"))


def _operands(heads, w1, w2, seed=0):
    g = torch.Generator().manual_seed(100 + heads + w2 + seed)
    N1, N2 = sum(LEN1), sum(LEN2)
    ops = [torch.randn(n, w, generator=g) for n, w in ((N1, w1), (N2, w1), (N2, w1), (N2, w2), (N1, w2), (N1, w2))]
    return ops, g


def _train_grads(ops, t, heads, g_o1, g_o2):
    leaves = [x.to(DEV).requires_grad_() for x in ops]
    o1, o2 = pt.cross_attention_pairs_train(*leaves, *_table_args(t), heads, t["rows1"], t["rows2"])
    grads = torch.autograd.grad([o1, o2], leaves, [g_o1, g_o2])
    return (o1.detach(), o2.detach()), grads


@pytest.mark.gpu
@pytest.mark.parametrize("heads,w1,w2", HEAD_SHAPES, ids=HEAD_IDS)
def test_forward_is_the_inference_op_bitwise(tables, heads, w1, w2):
    t = tables
    ops, _ = _operands(heads, w1, w2)
    dops = [x.to(DEV) for x in ops]
    with torch.no_grad():
        want = ps.cross_attention_pairs(*dops, *_table_args(t)[:6], heads, t["rows1"], t["rows2"], lse=False)
        got = pt.cross_attention_pairs_train(*dops, *_table_args(t), heads, t["rows1"], t["rows2"])
    assert len(got) == 2 and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    leaves = [x.requires_grad_() for x in dops]
    got = pt.cross_attention_pairs_train(*leaves, *_table_args(t), heads, t["rows1"], t["rows2"])      # and with a graph
    assert got[0].requires_grad and got[1].requires_grad and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def _dense_reference(ops, pairs, heads, g_o1, g_o2, LEN1=LEN1, LEN2=LEN2):
    """fp64, CPU: softmax attention per pair on index_select-ed rows of the unique graphs; autograd sums over the pairs."""
    leaves = [x.double().requires_grad_() for x in ops]
    q1, k1, v1, q2, k2, v2 = leaves
    p1, p2 = _ptr(LEN1), _ptr(LEN2)

    def attend(q, k, v):
        hd = q.shape[1] // heads
        split = lambda x: x.view(x.shape[0], heads, hd).transpose(0, 1)            # [H, L, hd]
        w = torch.softmax(split(q) @ split(k).transpose(1, 2) / hd ** 0.5, dim=-1)  # no keys: an empty sum, zero rows
        return (w @ split(v)).transpose(0, 1).reshape(q.shape[0], heads * hd)

    o1, o2 = [], []
    for a, b in pairs:
        r1, r2 = torch.arange(p1[a], p1[a + 1]), torch.arange(p2[b], p2[b + 1])
        sel = lambda x, r: torch.index_select(x, 0, r)
        o1.append(attend(sel(q1, r1), sel(k1, r2), sel(v1, r2)))
        o2.append(attend(sel(q2, r2), sel(k2, r1), sel(v2, r1)))
    return torch.autograd.grad([torch.cat(o1), torch.cat(o2)], leaves, [g_o1.double(), g_o2.double()])


@pytest.mark.gpu
@pytest.mark.parametrize("heads,w1,w2", HEAD_SHAPES, ids=HEAD_IDS)
def test_gradients(tables, heads, w1, w2):
    """MEASURED (MI355X, relative max-abs error against the fp64 reference, new / yardstick; six gradients each):
    see profiles/pair_training/README.md."""
    t = tables
    ops, g = _operands(heads, w1, w2)
    g_o1, g_o2 = torch.randn(t["rows1"], w1, generator=g), torch.randn(t["rows2"], w2, generator=g)
    ref = _dense_reference(ops, _pair_list(), heads, g_o1, g_o2)
    _, got = _train_grads(ops, t, heads, g_o1.to(DEV), g_o2.to(DEV))
    # the yardstick: the batch kernels on gathered rows, index_select's backward doing the sum
    leaves = [x.to(DEV).requires_grad_() for x in ops]
    sel = lambda x, idx: torch.index_select(x, 0, idx)
    q1, k1, v1, q2, k2, v2 = leaves
    y = torch.ops.caster_gvp.cross_attention(sel(q1, t["idx1"]), sel(k1, t["idx2"]), sel(v1, t["idx2"]), sel(q2, t["idx2"]),
                                             sel(k2, t["idx1"]), sel(v2, t["idx1"]), t["optr1"], t["optr2"], heads)
    yard = torch.autograd.grad([y[0], y[1]], leaves, [g_o1.to(DEV), g_o2.to(DEV)])
    torch.cuda.synchronize()
    err = lambda a, r: float((a.double().cpu() - r).abs().max() / r.abs().max())
    for name, a, b, r in zip(("g_q1", "g_k1", "g_v1", "g_q2", "g_k2", "g_v2"), got, yard, ref):
        assert a.shape == r.shape and a.dtype == torch.float32 and torch.isfinite(a).all(), name
        e_new, e_yard = err(a, r), err(b, r)
        print(f"{heads} heads, widths {w1}/{w2}, {name}: new {e_new:.3e}, batch path {e_yard:.3e}")
        assert e_new <= 2 * e_yard + 1e-6, name


def _bwd_problems(ops, outs, g_os, grads, t):
    """The two cgvp_attn_pairs_bwd_problem of a call over the tables `t` (device tensors everywhere)."""
    P = (pt.PairsBwdProblem * 2)()
    sides = ((ops[0], ops[1], ops[2], "ptr1", "ptr2", "g1", "g2", "optr1", "optr2", "inv1", "inv2", 0),
             (ops[3], ops[4], ops[5], "ptr2", "ptr1", "g2", "g1", "optr2", "optr1", "inv2", "inv1", 1))
    for x, (q, k, v, qp, kp, qg, kg, op, kop, qi, ki, d) in zip(P, sides):
        x.q, x.k, x.v = q.data_ptr(), k.data_ptr(), v.data_ptr()
        x.q_ptr, x.k_ptr, x.q_graph, x.k_graph, x.out_ptr, x.kout_ptr = (t[n].data_ptr() for n in (qp, kp, qg, kg, op, kop))
        x.q_inv_ptr, x.q_inv_pairs = t[qi + "_ptr"].data_ptr(), t[qi + "_pairs"].data_ptr()
        x.k_inv_ptr, x.k_inv_pairs = t[ki + "_ptr"].data_ptr(), t[ki + "_pairs"].data_ptr()
        x.num_q_graphs, x.num_k_graphs, x.num_q, x.num_k = t[qp].numel() - 1, t[kp].numel() - 1, q.shape[0], k.shape[0]
        x.num_out, x.num_kout = outs[d].shape[0], outs[1 - d].shape[0]
        x.out, x.lse, x.g_out = outs[d].data_ptr(), outs[2 + d].data_ptr(), g_os[d].data_ptr()
        x.g_q, x.g_k, x.g_v = (grads[3 * d + j].data_ptr() for j in range(3))
    return P


@pytest.mark.gpu
def test_zero_rows_and_pairs_without_keys(tables):
    """Through the C entry point on SENTINEL-filled gradient buffers: rows of the unreferenced graphs become exactly 0,
    everything is finite, and the pairs with an empty side contribute nothing -- the gradients equal, bitwise, those of
    the list without them (adding an exact zero changes no sum)."""
    from gvp_hip.ops import _stream
    t, heads, SENTINEL = tables, 8, -7.0
    ops, g = _operands(heads, 128, 128, seed=5)
    dops = [x.to(DEV) for x in ops]
    g_os = [torch.randn(t["rows1"], 128, generator=g).to(DEV), torch.randn(t["rows2"], 128, generator=g).to(DEV)]

    def run(tt, g_os):
        outs = torch.ops.caster_gvp.cross_attention_pairs_lse(*dops, *_table_args(tt)[:6], heads, tt["rows1"], tt["rows2"])
        grads = [torch.full_like(x, SENTINEL) for x in dops]
        P = _bwd_problems(dops, outs, g_os, grads, tt)
        need = pt.lib().cgvp_attn_bwd_pairs_floats(P, 2, heads, 16)
        ws = torch.full((need,), float("nan"), device=DEV)              # nothing is read before it is written
        assert pt.lib().cgvp_attn_bwd_pairs(P, 2, tt["g1"].numel(), heads, 16, 0.25, ws.data_ptr(), need, _stream()) == 0
        torch.cuda.synchronize()
        return outs, grads

    outs, grads = run(t, g_os)
    p1, p2 = _ptr(LEN1), _ptr(LEN2)
    for i, x in enumerate(grads):
        assert torch.isfinite(x).all() and not (x == SENTINEL).any(), i
        ptr = p1 if i in (0, 4, 5) else p2                              # q1, k2, v2: side 1; k1, v1, q2: side 2
        assert (x[ptr[-2]:ptr[-1]] == 0).all() and ptr[-1] - ptr[-2] > 0, i
        assert x[:ptr[-2]].abs().max() > 0
    pairs = _pair_list()
    keep = np.array([LEN1[a] > 0 and LEN2[b] > 0 for a, b in pairs])
    assert 0 < keep.sum() < 70 and any(LEN1[a] > 0 and LEN2[b] == 0 for a, b in pairs) and any(LEN1[a] == 0 and LEN2[b] > 0 for a, b in pairs)
    kept = _tables_of(pairs[keep])
    row_mask = lambda lens, side: torch.from_numpy(np.repeat(keep, np.asarray(lens)[pairs[:, side]])).to(DEV)
    m1, m2 = row_mask(LEN1, 0), row_mask(LEN2, 1)
    assert (outs[0][~m1] == 0).all() and (outs[2][~m1] == float("-inf")).all()      # the dropped rows: pairs without keys
    _, want = run(kept, [g_os[0][m1].contiguous(), g_os[1][m2].contiguous()])
    for i, (a, b) in enumerate(zip(grads, want)):
        assert torch.equal(a, b), i


@pytest.mark.gpu
@pytest.mark.parametrize("heads,w1,w2", HEAD_SHAPES, ids=HEAD_IDS)
def test_backward_is_reproducible(tables, heads, w1, w2):
    assert not torch.are_deterministic_algorithms_enabled()
    t = tables
    ops, g = _operands(heads, w1, w2, seed=1)
    g_o1, g_o2 = torch.randn(t["rows1"], w1, generator=g).to(DEV), torch.randn(t["rows2"], w2, generator=g).to(DEV)
    _, a = _train_grads(ops, t, heads, g_o1, g_o2)
    _, b = _train_grads(ops, t, heads, g_o1, g_o2)
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), i


@pytest.mark.gpu
@pytest.mark.parametrize("width", [4, 128])
def test_expand_rows_train(tables, width):
    t = tables
    g = torch.Generator().manual_seed(width)
    for lens, ptr, gi, optr, ip, ii, n, idx in ((LEN1, "ptr1", "g1", "optr1", "inv1_ptr", "inv1_pairs", "rows1", "idx1"),
                                                (LEN2, "ptr2", "g2", "optr2", "inv2_ptr", "inv2_pairs", "rows2", "idx2")):
        src = torch.randn(sum(lens), width, generator=g).to(DEV)
        with torch.no_grad():
            want_rows, want_batch = ps.expand_rows(src, t[ptr], t[gi], t[optr], t[n])
        leaf = src.clone().requires_grad_()
        rows, batch = pt.expand_rows_train(leaf, t[ptr], t[gi], t[optr], t[ip], t[ii], t[n])
        assert rows.requires_grad and not batch.requires_grad
        assert torch.equal(rows, want_rows) and torch.equal(batch, want_batch)
        # integer-valued gradients: every order of summation is exact
        g_rows = torch.randint(-8, 9, (t[n], width), generator=g).float().to(DEV)
        (got,) = torch.autograd.grad(rows, leaf, g_rows)
        want = torch.zeros_like(src).index_add_(0, t[idx], g_rows)
        torch.cuda.synchronize()
        assert torch.equal(got, want)
        last = _ptr(lens)
        assert (got[last[-2]:] == 0).all() and got[:last[-2]].abs().max() > 0       # the unreferenced graph


@pytest.mark.gpu
def test_refused_calls_launch_nothing(tables):
    """Every CGVP_ERR_* case on a call that WOULD launch (70 pairs, real buffers): the code is returned and the
    sentinel-filled gradients and workspace are untouched.  (No out-of-range device index is tried: the tables are the
    valid ones.)"""
    from gvp_hip.ops import _stream
    t, L, SENTINEL, heads = tables, pt.lib(), -7.0, 8
    ops, g = _operands(heads, 128, 128, seed=9)
    dops = [x.to(DEV) for x in ops]
    outs = torch.ops.caster_gvp.cross_attention_pairs_lse(*dops, *_table_args(t)[:6], heads, t["rows1"], t["rows2"])
    g_os = [torch.randn(t["rows1"], 128, generator=g).to(DEV), torch.randn(t["rows2"], 128, generator=g).to(DEV)]
    grads = [torch.full_like(x, SENTINEL) for x in dops]
    need = L.cgvp_attn_bwd_pairs_floats(_bwd_problems(dops, outs, g_os, grads, t), 2, heads, 16)
    ws = torch.full((need,), SENTINEL, device=DEV)
    torch.cuda.synchronize()

    def call(nprob=2, pairs=70, heads=8, head_dim=16, which=1, problems=True, ws_=0x1000, ws_floats=None, **kw):
        P = _bwd_problems(dops, outs, g_os, grads, t)
        for n, val in kw.items():
            base = getattr(P[which], n) if n in _TABLES + _ROWS16 + ("lse",) and val else 0
            setattr(P[which], n, base + (val - 0x1000 if base else val))   # (an offset from the case's nominal address)
        wsp = ws.data_ptr() + (ws_ - 0x1000) if ws_ else 0
        return L.cgvp_attn_bwd_pairs(P if problems else None, nprob, pairs, heads, head_dim, 0.25, wsp,
                                     need if ws_floats is None else ws_floats, _stream())

    for kw, code in _bad_argument_cases():
        kw = dict(kw)
        if "problems" in kw:
            kw["problems"] = False
        if "ws" in kw:
            kw["ws_"] = 0x1000 + kw.pop("ws") if kw["ws"] else kw.pop("ws")
        for which in (0, 1):
            assert call(which=which, **kw) == code, (which, kw)
            assert call(which=which, head_dim=48, **kw) == UNSUPPORTED, (which, kw)
    assert call(head_dim=48) == UNSUPPORTED and call(ws_floats=need - 1) == BAD
    part = torch.randn(t["rows1"], 128, generator=g).to(DEV)
    dst = torch.full((sum(LEN1), 128), SENTINEL, device=DEV)
    red = lambda **kw: L.cgvp_reduce_rows(*[kw.get(n, d) for n, d in (
        ("part", part.data_ptr()), ("optr", t["optr1"].data_ptr()), ("inv_ptr", t["inv1_ptr"].data_ptr()),
        ("inv_pairs", t["inv1_pairs"].data_ptr()), ("src_ptr", t["ptr1"].data_ptr()), ("graphs", len(LEN1)), ("pairs", 70),
        ("num_part", t["rows1"]), ("num_dst", sum(LEN1)), ("width", 128), ("dst", dst.data_ptr()))], _stream())
    for kw in (dict(graphs=-1), dict(pairs=-1), dict(num_part=-1), dict(num_dst=-1), dict(width=2), dict(width=130), dict(part=0),
               dict(dst=0), dict(optr=0), dict(inv_ptr=0), dict(inv_pairs=0), dict(src_ptr=0), dict(part=part.data_ptr() + 8),
               dict(dst=dst.data_ptr() + 4), dict(inv_pairs=t["inv1_pairs"].data_ptr() + 4)):
        assert red(**kw) == BAD, kw
    torch.cuda.synchronize()
    for o in grads + [ws, dst]:
        assert (o == SENTINEL).all()
    assert call() == 0 and red() == 0                                      # the same calls, unmodified, do run
    torch.cuda.synchronize()
    assert not any((o == SENTINEL).any() for o in grads) and not (dst == SENTINEL).any()


@pytest.mark.gpu
def test_compiled_equals_eager_bitwise(tables):
    """torch.compile over the op, forward and backward (both have fake kernels): ONE graph, no graph break, same bits."""
    from torch._dynamo.testing import CompileCounterWithBackend
    t, heads = tables, 8
    ops, g = _operands(heads, 128, 128, seed=3)
    g_o1, g_o2 = torch.randn(t["rows1"], 128, generator=g).to(DEV), torch.randn(t["rows2"], 128, generator=g).to(DEV)
    (e1, e2), eager = _train_grads(ops, t, heads, g_o1, g_o2)
    tabs, rows1, rows2 = _table_args(t), t["rows1"], t["rows2"]
    counter = CompileCounterWithBackend("aot_eager")
    fn = torch.compile(lambda *x: pt.cross_attention_pairs_train(*x, *tabs, heads, rows1, rows2), backend=counter, fullgraph=True)
    leaves = [x.to(DEV).requires_grad_() for x in ops]
    o1, o2 = fn(*leaves)
    grads = torch.autograd.grad([o1, o2], leaves, [g_o1, g_o2])
    torch.cuda.synchronize()
    assert counter.frame_count == 1
    assert torch.equal(o1, e1) and torch.equal(o2, e2)
    for i, (a, b) in enumerate(zip(grads, eager)):
        assert torch.equal(a, b), i


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the model
PROT_LENGTHS = [20, 33, 48]


def _to(d):
    return {k: (tuple(t.to(DEV) for t in v) if isinstance(v, tuple) else v.to(DEV)) for k, v in d.items()}


def _batch(graphs):
    gb = ds.collate(graphs)
    d = _to(ds.to_torch(gb))
    d["ptr"] = torch.as_tensor(gb.ptr).to(DEV)
    return d


@pytest.fixture(scope="module")
def graphs():
    rng = np.random.default_rng(2)
    prots = [ds.protein_graph(L, rng) for L in PROT_LENGTHS]
    drugs = [ds.drug_graph(rng) for _ in range(4)]
    pairs = [(0, 1), (2, 3), (2, 3), (1, 0), (0, 2), (2, 1), (0, 1), (1, 3), (2, 0), (1, 1)]     # 10 pairs with repeats
    return prots, drugs, pairs


def _param_grads(model):
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    model.zero_grad(set_to_none=True)
    return grads


def _model_case(model, graphs):
    """eval mode, gradients on: predictions against score_pairs (bitwise), parameter gradients against the collated batch.
    The bitwise comparison runs under torch.use_deterministic_algorithms: the segment pooling of BOTH routes is an
    index_add_, which adds with float atomics (in no fixed order) outside that mode."""
    prots, drugs, pairs = graphs
    model = model.to(DEV).eval()
    dp, dm = _batch(prots), _batch(drugs)
    torch.use_deterministic_algorithms(True)
    try:
        want = model.score_pairs(dp, dm, pairs)
        pred, second = model.forward_pairs(dp, dm, pairs)
        assert second is None and pred.shape == (len(pairs), 1) and pred.requires_grad and not model.training
        assert torch.equal(pred.detach(), want)
        pred.sum().backward()
        got = _param_grads(model)
        # a ready plan: the same result without the host read
        plan = pt.plan_pair_training(PROT_LENGTHS, [g["x_s"].shape[0] for g in drugs], pairs)
        assert torch.equal(model.forward_pairs(dp, dm, plan)[0].detach(), want)
        assert torch.equal(model.forward_pairs(dp, dm, torch.tensor(pairs, device=DEV))[0].detach(), want)
    finally:
        torch.use_deterministic_algorithms(False)
    collated, _ = model(_batch([prots[p] for p, _ in pairs]), _batch([drugs[d] for _, d in pairs]))
    collated.sum().backward()
    ref = _param_grads(model)
    assert set(got) == set(ref) and len(got) > 20
    # Relative 2e-4 of the tensor's own maximum for every gradient but those that are analytically zero and hold
    # rounding noise alone: these take the project's gradient bar as test_hip_backward.py::_check_grads states it, with
    # its floor of 2e-6 of the global gradient scale.  Three are, in every variant: gvp_edge.0's wv.weight (1 x 1),
    # wsv.weight and wsv.bias only SCALE the single edge vector channel, which the vector LayerNorm behind them
    # renormalises to unit length -- they measure 1e-9 and less at a global scale of 10, on both routes, and the two
    # routes' noise differs by 20 - 270 % of itself.  "Noise": a maximum below one fp32 ulp (2^-23) of the global scale.
    scale = max(float(v.abs().max()) for v in ref.values())
    worst, noise = 0.0, []
    for n in sorted(ref):
        assert got[n].shape == ref[n].shape and torch.isfinite(got[n]).all(), n
        top, err = float(ref[n].abs().max()), float((got[n] - ref[n]).abs().max())
        if top <= 2.0 ** -23 * scale:
            noise.append(n)
            assert err <= 2e-4 * top + 2e-6 * scale, (n, err, top)
            continue
        worst = max(worst, err / top)
        assert err <= 2e-4 * top, (n, err / top)
    print(f"{len(ref)} parameter gradients, worst relative error against the collated batch {worst:.3e}; "
          f"below one ulp of the global scale {scale:.3e} (rounding noise on both routes): {noise}")
    assert model.forward_pairs(dp, dm, [])[0].shape == (0, 1)
    with pytest.raises(IndexError):
        model.forward_pairs(dp, dm, pairs + [(3, 0)])
    with pytest.raises(IndexError):
        model.forward_pairs(dp, dm, pairs + [(0, 4)])
    return model


@pytest.mark.gpu
def test_model_gradients_equal_the_collated_batch(pretrained, graphs):
    model = _joint()
    model.load_state_dict(pretrained, strict=True)
    _model_case(model, graphs)


@pytest.mark.gpu
@pytest.mark.parametrize("over", [dict(n_attention_heads=2), dict(num_cross_attn_layers=2), dict(num_cross_attn_layers=0)],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_model_variants_equal_the_collated_batch(graphs, over):
    torch.manual_seed(0)
    _model_case(_joint(**over), graphs)


@pytest.mark.gpu
def test_model_train_mode(pretrained, graphs):
    """Train mode, dropout on, under torch.use_deterministic_algorithms(True): two runs from the same generator states give
    bitwise equal loss, predictions and gradients; every gradient is finite; attention dropout is refused."""
    from gvp_hip import autograd_ops, head_ops
    prots, drugs, pairs = graphs
    model = _joint()
    model.load_state_dict(pretrained, strict=True)
    model = model.to(DEV).train()
    assert model.dropout.p > 0
    dp, dm = _batch(prots), _batch(drugs)
    target = torch.linspace(-1, 1, len(pairs), device=DEV).unsqueeze(-1)
    torch.cuda.manual_seed(1234)
    dev = torch.device(DEV)
    states = {k: autograd_ops.rng_state(k, dev) for k in ("lba", "gine")}
    states["head"] = head_ops._head_rng_state(dev)
    saved = {k: v.clone() for k, v in states.items()}
    cuda = torch.cuda.get_rng_state()
    torch.use_deterministic_algorithms(True)
    try:
        runs = []
        for _ in range(2):
            torch.cuda.set_rng_state(cuda)
            for k, v in states.items():
                v.copy_(saved[k])
            pred, _ = model.forward_pairs(dp, dm, pairs)
            loss = torch.nn.functional.mse_loss(pred, target)
            loss.backward()
            torch.cuda.synchronize()
            assert model.training and all(m.training for m in model.modules())
            runs.append((loss.detach().clone(), pred.detach().clone(), _param_grads(model)))
    finally:
        torch.use_deterministic_algorithms(False)
    (l0, p0, g0), (l1, p1, g1) = runs
    assert torch.equal(l0, l1) and torch.equal(p0, p1) and set(g0) == set(g1) and len(g0) > 100
    for n in g0:
        assert torch.isfinite(g0[n]).all(), n
        assert torch.equal(g0[n], g1[n]), n
    torch.manual_seed(0)
    dropping = _joint(attention_dropout=0.1).to(DEV).train()
    with pytest.raises(NotImplementedError, match="attention dropout"):
        dropping.forward_pairs(dp, dm, pairs)
    assert dropping.training
    dropping.eval()
    assert dropping.forward_pairs(dp, dm, pairs)[0].shape == (len(pairs), 1)             # eval mode draws nothing
