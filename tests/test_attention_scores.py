"""Per-node attention scores (csrc/attn_score_kernels.hip, include/caster_gvp_attnscore.h, gvp_hip.attention_scores,
JointGNN.node_attention): the column mean and column max of every pair's head-averaged attention weights, on compact
rows.  REFERENCE: a per-pair dense softmax in float64 on the CPU (`_dense_ref`, the one of tests/test_attention.py
restated for any head count), its head-averaged `w` reduced with `.mean(0)` and `.max(0).values` exactly as
inference/evaluation.py:98-102 reduces the weights.  Bound: rel_err < 1e-5 (conftest), the bar of the weights these
values are reduced from -- the mean is linear and the max 1-Lipschitz in the max-abs norm, so it carries over."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import davis_synth as ds
from conftest import GOLDEN, REPO, rel_err
from gvp_hip import _lib, attention_ops, attention_scores  # noqa: F401

DEV = "cuda:0"
H, HD = 8, 16
E = H * HD
NAMES = ("atom_mean", "atom_max", "residue_mean", "residue_max")


# ---------------------------------------------------------------------------------------------------------------------
# CPU
def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(cgvp_[a-z0-9_]+)\s*\(", text))


def test_entry_points_have_a_header_and_a_version_of_their_own():
    header = os.path.join(REPO, "include", "caster_gvp_attnscore.h")
    assert _declared(header) == set(attention_scores.exported_symbols())
    main = open(os.path.join(REPO, "include", "caster_gvp.h")).read()
    handle = C.CDLL(_lib.LIB_PATH)
    for name in attention_scores.exported_symbols():
        assert hasattr(handle, name), name
        assert name not in main and name not in _lib.exported_symbols(), name
    text = open(header).read()
    assert attention_scores.lib().cgvp_attn_score_version() == 1 == attention_scores.ATTN_SCORE_VERSION
    assert "#define CGVP_ATTN_SCORE_VERSION 1\n" in text
    assert f"#define CGVP_ATTN_SCORE_MAX_HEADS {attention_scores.MAX_HEADS}\n" in text
    assert _lib.abi_header_digest() == _lib.ABI_HEADER_SHA256          # the main C ABI did not move


def test_fake_kernel_shapes_and_dtypes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        f = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device="cuda")
        N, Na = 70, 9
        outs = torch.ops.caster_gvp.cross_attention_node_scores(f(N, E), f(Na, E), f(N, H), f(Na, E), f(N, E), f(Na, H),
                                                                f(3, dt=torch.long), f(3, dt=torch.long), H)
        assert [tuple(t.shape) for t in outs] == [(9,), (9,), (70,), (70,)]
        assert all(t.dtype == torch.float32 and t.device.type == "cuda" for t in outs)


def _joint():
    from models.joint_gnn import JointGNN
    kw = json.load(open(os.path.join(GOLDEN, "model_kwargs.json")))
    return JointGNN(protein_gnn_kwargs=kw["protein_gnn_kwargs"], molecule_gnn_kwargs=kw["molecule_gnn_kwargs"],
                    **kw["joint_gnn_kwargs"])


def test_a_fresh_model_keeps_no_node_attention():
    model = _joint()
    assert model.node_attention == "never" and model.last_node_attention is None


def test_entry_point_checks_its_arguments_on_the_host():
    """CGVP_ERR_BAD_ARG before any launch, and before the `num_pairs == 0` return: every case but the last asks for zero
    pairs, so nothing here could launch even if a check were missing.  Pointers are never dereferenced."""
    L = attention_scores.lib()
    BAD, p = -1, 0x1000
    fields = [n for n, t in attention_scores.ScoreProblem._fields_ if t is C.c_void_p]

    def call(nprob=2, pairs=0, heads=H, which=1, **kw):
        P = (attention_scores.ScoreProblem * 2)()
        for x in P:
            for n in fields:
                setattr(x, n, p)
            x.num_q, x.num_k = 32, 48
        for n, val in kw.items():
            setattr(P[which], n, val)
        return L.cgvp_attn_node_scores(P, nprob, pairs, heads, 0.25, None)

    assert call() == 0 and call(nprob=1) == 0                             # no pairs: not an error, launches nothing
    cases = [dict(q_ptr=0), dict(q=p + 4), dict(num_q=-1), dict(nprob=3), dict(out_mean=0), dict(out_max=0),   # the issue's
             dict(nprob=0), dict(heads=0), dict(pairs=-1), dict(num_k=-1), dict(k_ptr=0), dict(q=0), dict(lse=0), dict(k=0),
             dict(k=p + 8), dict(lse=p + 4), dict(out_mean=p + 2), dict(q_ptr=p + 4), dict(num_q=1 << 24), dict(num_k=1 << 24)]
    for kw in cases:
        for which in (0, 1):
            assert call(which=which, **kw) == BAD, (which, kw)
    assert call(heads=attention_scores.MAX_HEADS + 1) == -2
    assert L.cgvp_attn_node_scores(None, 2, 0, H, 0.25, None) == BAD
    assert call(num_q=0, q=0, lse=0) == 0 and call(num_k=0, k=0, out_mean=0, out_max=0) == 0   # an empty side needs no buffers
    assert call(heads=3, lse=p + 4) == 0                                  # the lse rows are 16-byte units only when 4 | heads
    assert call(num_q=(1 << 24) - 17) == 0 and call(num_q=(1 << 24) - 16) == BAD


def test_per_pair_and_the_dense_fallback_reductions():
    """`per_pair` cuts a compact vector at ptr; `_dense_node_attention` (the dense fallback of the model) gives the same
    four vectors as the per-pair reductions of the padded weights."""
    from models.joint_gnn import _dense_node_attention, to_dense_batch
    rl, al = [5, 3, 7], [2, 4, 1]
    parts = attention_scores.per_pair(torch.arange(15.0), torch.tensor(_ptr(rl)))
    assert [tuple(x.shape) for x in parts] == [(5,), (3,), (7,)] and float(parts[2][0]) == 8.0
    g = torch.Generator().manual_seed(1)
    w1, w2 = torch.rand(3, max(rl), max(al), generator=g), torch.rand(3, max(al), max(rl), generator=g)
    rb, ab = (torch.repeat_interleave(torch.arange(3), torch.tensor(x)) for x in (rl, al))
    _, rmask = to_dense_batch(torch.zeros(sum(rl), 1), rb)
    _, amask = to_dense_batch(torch.zeros(sum(al), 1), ab)
    got = _dense_node_attention(w1, w2, rmask, amask)
    want = dict(atom_mean=[w1[b, :r, :a].mean(0) for b, (r, a) in enumerate(zip(rl, al))],
                atom_max=[w1[b, :r, :a].max(0).values for b, (r, a) in enumerate(zip(rl, al))],
                residue_mean=[w2[b, :a, :r].mean(0) for b, (r, a) in enumerate(zip(rl, al))],
                residue_max=[w2[b, :a, :r].max(0).values for b, (r, a) in enumerate(zip(rl, al))])
    for name in NAMES:
        assert rel_err(getattr(got, name), torch.cat(want[name])) < 1e-6, name


# ---------------------------------------------------------------------------------------------------------------------
# the float64 reference
def _ptr(lens):
    return [0] + [int(x) for x in np.cumsum(lens)]


def _operands(rl, al, seed, heads=H):
    """(q_r, k_a, v_a, q_a, k_r, v_r): seeded randn on the CPU"""
    g = torch.Generator().manual_seed(seed)
    N, Na = sum(rl), sum(al)
    return [torch.randn(n, heads * HD, generator=g) for n in (N, Na, Na, Na, N, N)]


def _dense_ref(q, k, qp, kp, heads=H):
    """per pair, per head: p = softmax(q k^T / sqrt(16)) in the dtype of the operands; w = p.mean over the heads;
    -> (mean [Nk], max [Nk]) = w.mean(0), w.max(0).values per pair (inference/evaluation.py:98-102), concatenated.
    Keys of a pair without queries get 0 (the kernel's documented value; the reference has no such pair)."""
    means, maxs = [], []
    for b in range(len(qp) - 1):
        lq, lk = qp[b + 1] - qp[b], kp[b + 1] - kp[b]
        if lq == 0 or lk == 0:
            means.append(q.new_zeros(lk)), maxs.append(q.new_zeros(lk))
            continue
        qb = q[qp[b]:qp[b + 1]].view(lq, heads, HD).transpose(0, 1)
        kb = k[kp[b]:kp[b + 1]].view(lk, heads, HD).transpose(0, 1)
        w = torch.softmax(qb @ kb.transpose(1, 2) / 4.0, dim=-1).mean(0)
        means.append(w.mean(0)), maxs.append(w.max(0).values)
    return torch.cat(means), torch.cat(maxs)


def _reference(ops, rl, al, heads=H):
    rp, ap = _ptr(rl), _ptr(al)
    d = [t.double() for t in ops]
    atom_mean, atom_max = _dense_ref(d[0], d[1], rp, ap, heads)
    res_mean, res_max = _dense_ref(d[3], d[4], ap, rp, heads)
    return dict(zip(NAMES, (atom_mean, atom_max, res_mean, res_max)))


def _ours(ops, rl, al, heads=H):
    """forward op (for the lse) + the score op on the GPU, twice -> ({name: tensor}, the same of the second call)"""
    rptr, aptr = torch.tensor(_ptr(rl), device=DEV), torch.tensor(_ptr(al), device=DEV)
    q_r, k_a, v_a, q_a, k_r, v_r = [t.to(DEV) for t in ops]
    _, _, lse_r, lse_a = torch.ops.caster_gvp.cross_attention(q_r, k_a, v_a, q_a, k_r, v_r, rptr, aptr, heads)
    runs = [torch.ops.caster_gvp.cross_attention_node_scores(q_r, k_a, lse_r, q_a, k_r, lse_a, rptr, aptr, heads)
            for _ in range(2)]
    torch.cuda.synchronize()
    return [dict(zip(NAMES, r)) for r in runs]


def _check(ops, rl, al, heads=H):
    """Everything the issue asks of one case -> (ours on the CPU, reference)"""
    N, Na = sum(rl), sum(al)
    ref = _reference(ops, rl, al, heads)
    got, again = _ours(ops, rl, al, heads)
    for name in NAMES:
        assert torch.equal(got[name], again[name]), name                 # run to run bitwise
    got = {k: v.cpu() for k, v in got.items()}
    for name, rows in zip(NAMES, (Na, Na, N, N)):
        assert got[name].shape == (rows,) and got[name].dtype == torch.float32, name
        assert torch.isfinite(got[name]).all() and (got[name] >= 0).all() and (got[name] <= 1).all(), name
        err = rel_err(got[name], ref[name])
        print(f"{name}: rel_err {err:.3e}")
        assert err < 1e-5, name
    rp, ap = _ptr(rl), _ptr(al)
    for mean, mx, qp, kp in (("atom_mean", "atom_max", rp, ap), ("residue_mean", "residue_max", ap, rp)):
        for b in range(len(rl)):
            ks = slice(kp[b], kp[b + 1])
            if qp[b + 1] > qp[b] and kp[b + 1] > kp[b]:
                # every query's weights sum to 1 over the pair's keys, so the column means do (a pair without keys has
                # no weights at all: the sum of nothing is 0 and is not compared with 1)
                assert abs(float(got[mean][ks].double().sum()) - 1.0) < 1e-5, (mean, b)
            if qp[b + 1] == qp[b]:
                assert (got[mean][ks] == 0.0).all() and (got[mx][ks] == 0.0).all(), (mean, b)   # exactly
    return got, ref


# the edge lists of tests/test_attention_edges.py (copied), and one long pair: an atom key tile walks 258 query tiles
CASES = {
    "three_chunks": ([(7 * b) % 41 for b in range(131)], [(5 * b + 3) % 23 for b in range(131)]),
    "atoms_outnumber_residues": ([5, 16, 1], [48, 17, 33]),
    "empty_sides": ([20, 0, 16, 0, 3], [0, 9, 16, 0, 1]),
    "no_atoms_at_all": ([4, 9], [0, 0]),
    "whole_tiles_only": ([16, 32, 48], [16, 32, 16]),
    "tails_of_one_and_fifteen": ([17, 33], [15, 31]),
    "one_long_pair": ([4128, 215], [96, 12]),
}


# ---------------------------------------------------------------------------------------------------------------------
# GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_node_scores_edges(case):
    rl, al = CASES[case]
    got, _ = _check(_operands(rl, al, 11), rl, al)
    if case == "empty_sides":
        ap, rp = _ptr(al), _ptr(rl)
        assert (got["atom_mean"][ap[1]:ap[2]] == 0.0).all() and (got["atom_max"][ap[1]:ap[2]] == 0.0).all()    # no residues
        assert (got["residue_mean"][rp[0]:rp[1]] == 0.0).all() and (got["residue_max"][rp[0]:rp[1]] == 0.0).all()   # no atoms
    if case == "no_atoms_at_all":
        assert got["atom_mean"].shape == (0,) and (got["residue_mean"] == 0).all() and (got["residue_max"] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("heads", [3, 4])
def test_other_head_counts(heads):
    """the instantiations whose lse rows are read word by word (3) and as one float4 (4)"""
    rl, al = [40, 17, 5], [9, 33, 20]
    _check(_operands(rl, al, 13, heads), rl, al, heads)


@pytest.mark.gpu
def test_sharp_softmax():
    """q x 30: logits of magnitude ~100, most weights underflow to 0 and a few are ~1.  No NaN, nothing above 1 (both
    inside `_check`), and the same 1e-5 against float64."""
    rl, al = [50, 40], [37, 70]
    q_r, k_a, v_a, q_a, k_r, v_r = _operands(rl, al, 23)
    got, ref = _check([q_r * 30, k_a, v_a, q_a * 30, k_r, v_r], rl, al)
    top = float(((q_r[:50, :HD] * 30) @ k_a[:37, :HD].t() / 4.0).abs().max())      # pair 0, head 0
    print(f"max |logit| of pair 0, head 0: {top:.1f}")
    assert top > 60
    assert not any(torch.isnan(v).any() for v in got.values())


@pytest.mark.gpu
def test_nothing_is_written_outside_the_outputs():
    """The C entry point with out_mean / out_max inside larger sentinel-filled buffers (32 floats in front and behind),
    key counts (62 both ways) that are no multiple of 16: the margins are untouched, every element of [0, Nk) is written."""
    from gvp_hip.ops import _stream
    rl, al = [40, 17, 5], [9, 33, 20]
    ops = _operands(rl, al, 37)
    ref = _reference(ops, rl, al)
    rptr, aptr = torch.tensor(_ptr(rl), device=DEV), torch.tensor(_ptr(al), device=DEV)
    q_r, k_a, v_a, q_a, k_r, v_r = [t.to(DEV) for t in ops]
    _, _, lse_r, lse_a = torch.ops.caster_gvp.cross_attention(q_r, k_a, v_a, q_a, k_r, v_r, rptr, aptr, H)
    PAD, SENTINEL = 32, -7.0
    N, Na = sum(rl), sum(al)
    assert N % 16 and Na % 16
    bufs = {n: torch.full((rows + 2 * PAD,), SENTINEL, device=DEV) for n, rows in zip(NAMES, (Na, Na, N, N))}
    P = (attention_scores.ScoreProblem * 2)()
    for p, (q, k, lse, qp, kp, mean, mx) in zip(P, ((q_r, k_a, lse_r, rptr, aptr, "atom_mean", "atom_max"),
                                                     (q_a, k_r, lse_a, aptr, rptr, "residue_mean", "residue_max"))):
        p.q, p.k, p.lse, p.q_ptr, p.k_ptr = (t.data_ptr() for t in (q, k, lse, qp, kp))
        p.num_q, p.num_k = q.shape[0], k.shape[0]
        p.out_mean, p.out_max = bufs[mean][PAD:].data_ptr(), bufs[mx][PAD:].data_ptr()
    assert attention_scores.lib().cgvp_attn_node_scores(P, 2, len(rl), H, 0.25, _stream()) == 0
    torch.cuda.synchronize()
    for name, rows in zip(NAMES, (Na, Na, N, N)):
        b = bufs[name].cpu()
        assert (b[:PAD] == SENTINEL).all() and (b[PAD + rows:] == SENTINEL).all(), name
        assert (b[PAD:PAD + rows] != SENTINEL).all(), name
        assert rel_err(b[PAD:PAD + rows], ref[name]) < 1e-5, name


@pytest.mark.gpu
def test_module_scores_equal_the_reductions_of_the_dense_mha_weights():
    """CrossAttentionModule.forward_varlen(scores_out=[...]) against the module's dense `forward` through stock
    nn.MultiheadAttention (to_dense_batch + key-padding masks), its weights cut and reduced per pair."""
    from models.joint_gnn import CrossAttentionModule, NodeAttention, to_dense_batch
    torch.manual_seed(0)
    mod = CrossAttentionModule(128, 128, 8, 0.0, True, 2, 0.2).to(DEV).eval()
    rl, al = [57, 120, 33], [21, 40, 17]
    g = torch.Generator().manual_seed(3)
    r, m = torch.randn(sum(rl), 128, generator=g).to(DEV), torch.randn(sum(al), 128, generator=g).to(DEV)
    rb = torch.repeat_interleave(torch.arange(3), torch.tensor(rl)).to(DEV)
    mb = torch.repeat_interleave(torch.arange(3), torch.tensor(al)).to(DEV)
    rptr, aptr = torch.tensor(_ptr(rl)).to(DEV), torch.tensor(_ptr(al)).to(DEV)
    scores = []
    with torch.no_grad():
        e1, e2, none = mod.forward_varlen(r, m, rptr, aptr, scores_out=scores)
        plain = mod.forward_varlen(r, m, rptr, aptr)
        dr, rmask = to_dense_batch(r, rb)
        dm, mmask = to_dense_batch(m, mb)
        _, _, (x1, x2) = mod(dr, dm, rmask, mmask)
    assert none is None and len(scores) == 1 and isinstance(scores[0], NodeAttention)
    assert torch.equal(e1, plain[0]) and torch.equal(e2, plain[1])       # asking for the scores changes nothing else
    x1, x2 = x1.double().cpu(), x2.double().cpu()
    pairs = list(enumerate(zip(rl, al)))
    want = dict(atom_mean=[x1[b, :lr, :la].mean(0) for b, (lr, la) in pairs],
                atom_max=[x1[b, :lr, :la].max(0).values for b, (lr, la) in pairs],
                residue_mean=[x2[b, :la, :lr].mean(0) for b, (lr, la) in pairs],
                residue_max=[x2[b, :la, :lr].max(0).values for b, (lr, la) in pairs])
    for name in NAMES:
        got = attention_scores.per_pair(getattr(scores[0], name), aptr if name.startswith("atom") else rptr)
        for b, _ in pairs:
            err = rel_err(got[b], want[name][b])
            print(f"{name} pair {b}: rel_err {err:.3e}")
            assert err < 1e-5, (name, b)


@pytest.mark.gpu
def test_model_predict_with_node_attention(pretrained):
    """The forwards are made under torch.use_deterministic_algorithms(True), as tests/test_eval_metrics.py makes its
    bitwise model comparisons: in the default mode the segment pooling of the head adds rows with float atomics
    (index_add_), so two PLAIN eval forwards of one model already differ in the last bit (printed below; measured on an
    MI355X: not equal, max abs difference 1.19e-7 on affinities of magnitude 1) and "the same bits" would say nothing
    about the scores.  In the mode the affinity with node attention is the plain one, bitwise."""
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        _predict_with_node_attention(pretrained)
    finally:
        torch.use_deterministic_algorithms(was)


def _predict_with_node_attention(pretrained):
    model = _joint()
    model.load_state_dict(pretrained, strict=True)
    model = model.to(DEV).eval()
    lengths = [40, 75, 33, 120, 64]
    p, m = ds.pair_batch(5, 21, lengths=lengths)
    to = lambda d: {k: (tuple(t.to(DEV) for t in v) if isinstance(v, tuple) else v.to(DEV)) for k, v in d.items()}
    dp, dm = to(ds.to_torch(p)), to(ds.to_torch(m))
    dp["ptr"], dm["ptr"] = torch.as_tensor(p.ptr).to(DEV), torch.as_tensor(m.ptr).to(DEV)
    al = [int(x) for x in np.diff(m.ptr)]
    with torch.no_grad():
        torch.use_deterministic_algorithms(False)
        twice = [model(dp, dm)[0] for _ in range(2)]
        torch.use_deterministic_algorithms(True)
        print(f"default mode: two plain eval forwards bitwise equal: {torch.equal(*twice)}, "
              f"max abs difference {float((twice[0] - twice[1]).abs().max()):.3e}")
        model.attention_weights = "always"
        y_plain, attn = model(dp, dm)
        assert model.last_node_attention is None                         # the default: nothing is kept
        model.attention_weights = "never"
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        y_never, none = model(dp, dm)
        torch.cuda.synchronize()
        peak_plain = torch.cuda.max_memory_allocated() - base
        del y_never
        assert none is None and model.last_node_attention is None
        model.attention_weights = "auto"
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y, layers = model.predict_with_node_attention(dp, dm)
    torch.cuda.synchronize()
    peak_scores = torch.cuda.max_memory_allocated() - base
    dense_bytes = 4 * len(lengths) * max(lengths) * max(al)              # ONE of the two [B, Rmax, Amax] tensors
    print(f"peak bytes: forward {peak_plain}, with node attention {peak_scores}, one dense weight tensor {dense_bytes}")
    assert peak_scores - peak_plain < dense_bytes
    assert torch.equal(y, y_plain)                                        # bitwise the plain eval forward
    assert not model.training and model.node_attention == "never" and model.attention_weights == "auto"
    assert layers is model.last_node_attention and len(layers) == len(attn)
    w1, w2 = (w.double().cpu() for w in attn[0])
    pairs = list(enumerate(zip(lengths, al)))
    want = dict(atom_mean=[w1[b, :lr, :la].mean(0) for b, (lr, la) in pairs],
                atom_max=[w1[b, :lr, :la].max(0).values for b, (lr, la) in pairs],
                residue_mean=[w2[b, :la, :lr].mean(0) for b, (lr, la) in pairs],
                residue_max=[w2[b, :la, :lr].max(0).values for b, (lr, la) in pairs])
    for name in NAMES:
        got = getattr(layers[0], name)
        assert got.shape == ((sum(al),) if name.startswith("atom") else (sum(lengths),))
        err = rel_err(got, torch.cat(want[name]))
        print(f"{name}: rel_err {err:.3e}")
        assert err < 1e-5, name
    model.train()
    model.node_attention = "auto"
    model(dp, dm)
    assert model.last_node_attention is None                             # "auto": eval mode only
    model.eval()
    with torch.no_grad():
        model(dp, dm)
    assert len(model.last_node_attention) == len(attn)


@pytest.mark.gpu
def test_the_op_replays_from_a_captured_graph():
    """Captured alone in one torch.cuda.graph after a warm-up call; q / k / lse / ptr overwritten in place with a second
    batch of the same row counts and the same NUMBER of pairs (it sizes the grid on the host; the remainder are empty
    pairs); the replay equals an eager call on the second batch."""
    first, second = ([50, 40, 0, 0], [37, 70, 0, 0]), ([30, 25, 35, 0], [60, 7, 40, 0])
    assert [sum(x) for x in first] == [sum(x) for x in second]

    def batch(lens, seed):
        rl, al = lens
        rptr, aptr = torch.tensor(_ptr(rl), device=DEV), torch.tensor(_ptr(al), device=DEV)
        q_r, k_a, v_a, q_a, k_r, v_r = [t.to(DEV) for t in _operands(rl, al, seed)]
        _, _, lse_r, lse_a = torch.ops.caster_gvp.cross_attention(q_r, k_a, v_a, q_a, k_r, v_r, rptr, aptr, H)
        return [q_r, k_a, lse_r, q_a, k_r, lse_a, rptr, aptr]

    static = [t.clone() for t in batch(first, 41)]
    want_first = torch.ops.caster_gvp.cross_attention_node_scores(*static, H)          # the warm-up call
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = torch.ops.caster_gvp.cross_attention_node_scores(*static, H)
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(outs, want_first):
        assert torch.equal(got, want)
    nxt = batch(second, 43)
    want_second = torch.ops.caster_gvp.cross_attention_node_scores(*nxt, H)
    for dst, src in zip(static, nxt):
        dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    for got, want, name in zip(outs, want_second, NAMES):
        assert torch.equal(got, want), name
    assert not torch.equal(outs[0], want_first[0])
