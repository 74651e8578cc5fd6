"""The pair-list attention kernels (csrc/attn_pairs_kernels.hip, attn_pairs_bwd_kernels.hip, attn_pairs_score_kernels.hip)
at the launch and numeric edges their feature tests do not reach: both orders of the two problems in all four launches
and the tie, one graph against 131 (a third `locate` chunk, an inverse list that holds every pair, a `shift` of either
sign), 3 heads of 16 in the forward and the backward, the ORDER of the ordered sum of `reduce_rows_kernel`, and logits of
magnitude ~150 over a pair list.

REFERENCES.  Forward and node scores: the batch kernels on the rows gathered with index_select, BITWISE (the contract
attn_pairs_kernels.hip / attn_pairs_score_kernels.hip state), and for the scores a dense fp64 softmax, rel_err < 1e-5
(tests/test_pair_node_scores.py).  Gradients: the dense fp64 reference of tests/test_pair_training.py, relative error
new <= 2 x yardstick + 1e-6 with the batch kernels on gathered rows as yardstick.  The ordered sum: an fp32 loop on the
CPU that adds the pairs' rows one at a time in ascending pair index, bitwise.  Large logits: the cap of
tests/test_attention_edges.py, e_ours <= max(4 e_stock, 2e-6 scale) against fp64."""
import functools

import numpy as np
import pytest
import torch

import test_attention_edges as AE
import test_pair_node_scores as NS
import test_pair_training as PT
from conftest import rel_err
from gvp_hip import attention_ops, attention_scores, pair_node_scores as pns, pair_scoring as ps, pair_training as pt  # noqa: F401

DEV = "cuda:0"
NPAIR = 131
_rng = np.random.default_rng(23)
_draws = [_rng.permutation(NPAIR) for _ in range(3)]
# The first draw serves the drugs.  The second puts an empty protein at position 128 (the first pair of the third locate
# chunk would have no rows on side 1), so the proteins take the third: every property asserted below holds for it.
PERM_DRUGS, PERM_PROTEINS = _draws[0], _draws[2]

CASES = {
    # three locate chunks (64, 64, 3); an inverse list of 131 pairs; key-less pairs; shift of both signs on side 2
    "one_protein_many_drugs": ([37], [(5 * b + 3) % 23 for b in range(NPAIR)], [(0, int(PERM_DRUGS[b])) for b in range(NPAIR)]),
    # average 2 > average 1: the launch order no other test runs; query-less pairs; shift of both signs on side 1
    "many_proteins_one_drug": ([(7 * b) % 41 for b in range(NPAIR)], [45], [(int(PERM_PROTEINS[b]), 0) for b in range(NPAIR)]),
    # no swap in any of the four launches
    "equal_averages": ([16, 24], [20, 20], [(0, 0), (1, 1), (0, 1), (1, 0), (1, 1)]),
    # the mirrored orientation at whole-tile and one-row graphs
    "drugs_outnumber": ([5, 16, 1], [48, 17, 33], [(a, b) for a in range(3) for b in range(3)] + [(0, 0), (2, 2)]),
    # protein 0 and molecule 2 have rows and appear only in pairs whose other side is empty: their gradients are exact zeros
    "only_empty_partners": ([9, 20, 0], [0, 12, 7], [(0, 0), (1, 1), (2, 2), (1, 1), (0, 0)]),
}
SIGN = {"one_protein_many_drugs": 1, "many_proteins_one_drug": -1, "equal_averages": 0, "drugs_outnumber": -1,
        "only_empty_partners": 1}                                 # of avg(LEN1) - avg(LEN2)
HEAD_SHAPES = [(8, 128), (3, 48)]
HEAD_IDS = ["8x16", "3x16"]
GRADS = ("g_q1", "g_k1", "g_v1", "g_q2", "g_k2", "g_v2")
SIDE_OF_GRAD = (0, 1, 1, 1, 0, 0)                                 # q1, k2, v2 hold the rows of side 1; k1, v1, q2 those of side 2


def _ptr(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _lens(name):
    len1, len2, pairs = CASES[name]
    pairs = np.asarray(pairs, dtype=np.int64)
    return np.asarray(len1, dtype=np.int64), np.asarray(len2, dtype=np.int64), pairs


def _lonely(name):
    """-> per side, the graphs whose gradients must be exact zeros: referenced by no pair, or only by pairs whose other
    side is empty."""
    len1, len2, pairs = _lens(name)
    out = []
    for lens, other, col in ((len1, len2, 0), (len2, len1, 1)):
        out.append([x for x in range(len(lens)) if all(other[p[1 - col]] == 0 for p in pairs if p[col] == x)])
    return out


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the cases are what they are there for
@pytest.mark.parametrize("name", list(CASES))
def test_cases_reach_what_they_are_there_for(name):
    """The launch order of every pair-list launch is decided by the sign of avg(LEN1) - avg(LEN2) (`swap` of fwd_pairs,
    `swap_q` / `swap_k` of bwd_pairs, `swap` of node_scores_pairs): asserted per case, with the properties of the two
    131-pair lists, so that a later edit of the tables cannot hollow the GPU tests out."""
    len1, len2, pairs = _lens(name)
    plan = pt.plan_pair_training(len1, len2, pairs)
    avg = len1.sum() / len(len1) - len2.sum() / len(len2)
    assert np.sign(avg) == SIGN[name], avg
    # what the kernels compare, literally: rows x graphs of the other side
    assert np.sign(int(len1.sum()) * len(len2) - int(len2.sum()) * len(len1)) == SIGN[name]
    if len(pairs) == NPAIR:
        l1, l2 = len1[pairs[:, 0]], len2[pairs[:, 1]]
        assert all(l1[b] > 0 and l2[b] > 0 for b in (63, 64, 127, 128, 130))       # the chunk borders of locate()
        empty = (l1 == 0) | (l2 == 0)
        assert empty[:64].any() and empty[64:128].any()
        many, lens, optr = (1, len2, plan.optr2) if name == "one_protein_many_drugs" else (0, len1, plan.optr1)
        assert len(lens) == NPAIR and sorted(pairs[:, many]) == list(range(NPAIR))
        shift = optr[:-1] - _ptr(lens)[pairs[:, many]]
        print(f"{name}: shift < 0 for {(shift < 0).sum()} pairs, > 0 for {(shift > 0).sum()}")
        assert (shift < 0).any() and (shift > 0).any()
        # the single graph's inverse list holds every pair
        inv_ptr = plan.inv1_ptr if many == 1 else plan.inv2_ptr
        assert inv_ptr.tolist() == [0, NPAIR]
    if name == "equal_averages":
        assert avg == 0
    if name == "drugs_outnumber":
        assert {tuple(p) for p in pairs} == {(a, b) for a in range(3) for b in range(3)} and len(pairs) == 11
    if name == "only_empty_partners":
        lonely1, lonely2 = _lonely(name)
        assert any(len1[x] > 0 for x in lonely1) and any(len2[x] > 0 for x in lonely2)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: every case at 8 x 16 and 3 x 16
@functools.lru_cache(maxsize=None)
def _tables(name):
    len1, len2, pairs = _lens(name)
    return PT._tables_of(pairs, len1, len2)


def _operands(name, heads, width):
    len1, len2, _ = _lens(name)
    plan = pt.plan_pair_training(*_lens(name))
    g = torch.Generator().manual_seed(1000 + 16 * list(CASES).index(name) + heads)
    N1, N2 = int(len1.sum()), int(len2.sum())
    ops = [torch.randn(n, width, generator=g) for n in (N1, N2, N2, N2, N1, N1)]
    return ops, torch.randn(plan.rows1, width, generator=g), torch.randn(plan.rows2, width, generator=g)


def _gathered(dops, t):
    sel = lambda x, idx: torch.index_select(x, 0, idx)
    q1, k1, v1, q2, k2, v2 = dops
    return [sel(q1, t["idx1"]), sel(k1, t["idx2"]), sel(v1, t["idx2"]), sel(q2, t["idx2"]), sel(k2, t["idx1"]), sel(v2, t["idx1"])]


def _run_everything(ops, g_o1, g_o2, t, heads):
    """The three pair-list ops and the batch kernels on gathered rows -> {name: CPU tensor}: `fwd` / `batch_fwd` (o1, o2,
    lse1, lse2), `grads` / `again` (two runs of the train op) / `yard` (batch backward + index_select's backward),
    `scores` / `batch_scores` (the four vectors)."""
    dops = [x.to(DEV) for x in ops]
    tabs = PT._table_args(t)
    with torch.no_grad():
        fwd = ps.cross_attention_pairs(*dops, *tabs[:6], heads, t["rows1"], t["rows2"], lse=True)
        scores = torch.ops.caster_gvp.cross_attention_pairs_node_scores(dops[0], dops[1], fwd[2], dops[3], dops[4], fwd[3],
                                                                        *tabs[:6], heads)
    leaves = [x.to(DEV).requires_grad_() for x in ops]
    y = torch.ops.caster_gvp.cross_attention(*_gathered(leaves, t), t["optr1"], t["optr2"], heads)
    yard = torch.autograd.grad([y[0], y[1]], leaves, [g_o1.to(DEV), g_o2.to(DEV)])
    with torch.no_grad():
        g = _gathered(dops, t)
        batch_scores = torch.ops.caster_gvp.cross_attention_node_scores(g[0], g[1], y[2].detach(), g[3], g[4], y[3].detach(),
                                                                        t["optr1"], t["optr2"], heads)
    (o1, o2), grads = PT._train_grads(ops, t, heads, g_o1.to(DEV), g_o2.to(DEV))
    _, again = PT._train_grads(ops, t, heads, g_o1.to(DEV), g_o2.to(DEV))
    torch.cuda.synchronize()
    cpu = lambda ts: [x.detach().cpu() for x in ts]
    return dict(fwd=cpu(fwd), batch_fwd=cpu(y), train_fwd=cpu((o1, o2)), grads=cpu(grads), again=cpu(again), yard=cpu(yard),
                scores=cpu(scores), batch_scores=cpu(batch_scores))


@functools.lru_cache(maxsize=None)
def _case(name, heads, width):
    """One (case, head shape), run once for the tests that share it -> (operands, g_o1, g_o2 on the CPU, results)."""
    ops, g_o1, g_o2 = _operands(name, heads, width)
    return ops, g_o1, g_o2, _run_everything(ops, g_o1, g_o2, _tables(name), heads)


def _bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("heads,width", HEAD_SHAPES, ids=HEAD_IDS)
@pytest.mark.parametrize("name", list(CASES))
def test_forward_is_the_batch_kernel_bitwise(name, heads, width):
    """attn_fwd_pairs_kernel in both problem orders and at the tie.  `swap` of fwd_pairs is true only where avg(LEN1) >
    avg(LEN2): [many_proteins_one_drug] and [drugs_outnumber] run `probs[i]` unswapped, [equal_averages] the tie.  The
    131-pair lists reach the third trip of `locate(P.out_ptr, ...)` (pairs 128 .. 130), `q0 = q_ptr[qg] + (o0 -
    out_ptr[b])` for tiles behind a graph's first, and `k0 == k_end` pairs (no key tile: l == 0 -> out 0, lse -inf).
    [3x16] is the unit decode `h = u % a.H, t = u / a.H` with H no power of two and E = 48.
    out and lse equal `caster_gvp::cross_attention` on the index_select-ed rows bit for bit; rows of key-less pairs are
    exactly 0 / -inf."""
    len1, len2, pairs = _lens(name)
    t = _tables(name)
    _, _, _, res = _case(name, heads, width)
    for i, what in enumerate(("o1", "o2", "lse1", "lse2")):
        a, b = res["fwd"][i], res["batch_fwd"][i]
        rows = t["rows1"] if i % 2 == 0 else t["rows2"]
        assert a.shape == (rows, width if i < 2 else heads), what
        print(f"{name} {heads} heads {what}: differing elements {int((a != b).sum())} of {a.numel()}")
        assert _bits(a, b), what
    assert _bits(res["train_fwd"][0], res["fwd"][0]) and _bits(res["train_fwd"][1], res["fwd"][1])
    plan = t["plan"]
    seen = 0
    for o, lse, optr, qlen, klen in ((res["fwd"][0], res["fwd"][2], plan.optr1, len1[pairs[:, 0]], len2[pairs[:, 1]]),
                                     (res["fwd"][1], res["fwd"][3], plan.optr2, len2[pairs[:, 1]], len1[pairs[:, 0]])):
        keyless = torch.from_numpy(np.repeat(klen == 0, qlen))
        assert keyless.shape[0] == o.shape[0]
        assert (o[keyless] == 0).all() and (lse[keyless] == -float("inf")).all()
        assert torch.isfinite(lse[~keyless]).all() and torch.isfinite(o).all()
        seen += int(keyless.sum())
    if len(pairs) == NPAIR or name == "only_empty_partners":
        assert seen > 0


@pytest.mark.gpu
@pytest.mark.parametrize("heads,width", HEAD_SHAPES, ids=HEAD_IDS)
@pytest.mark.parametrize("name", list(CASES))
def test_gradients_in_both_launch_orders(name, heads, width):
    """bwd_pairs of attn_pairs_bwd_kernels.hip with `swap_q` false and `swap_k` TRUE ([many_proteins_one_drug],
    [drugs_outnumber]): the d K / d V launch maps `a.p[i] <- probs[1 - i]` and must take the workspace slices
    `plan[si]` (pq, pk, pv, delta) of the SAME si, while the reduce jobs keep the given order; d Q runs unswapped.
    [equal_averages]: neither swaps.  The 131-pair lists: the third `locate` chunk over out_ptr and kout_ptr, the wave-
    uniform `shift = out_ptr[b] - q0` of attn_bwd_pairs_dkv_kernel with either sign (dE, dH added modulo 2^32 to the
    clamped offsets), query-less pairs (zero d K / d V rows) and key-less pairs (zero d Q), and a reduce over an inverse
    list of all 131 pairs.  [3x16]: `h = u % a.H` in both backward kernels, the scalar lse / delta rows of 3 floats, the
    delta sub-buffer padded to 16 bytes.
    Against the fp64 dense reference: relative error new <= 2 x yardstick + 1e-6, the yardstick being the batch kernels on
    gathered rows with index_select's backward; exact zeros for graphs that only meet empty partners; two runs bitwise.
    (Tried on an MI355X: a build whose d K / d V launch reads `delta` at `plan[i]` instead of `plan[si]` fails exactly
    [many_proteins_one_drug], [drugs_outnumber] and the large-logit test below, at both head shapes.)"""
    len1, len2, pairs = _lens(name)
    ops, g_o1, g_o2, res = _case(name, heads, width)
    ref = PT._dense_reference(ops, [tuple(p) for p in pairs], heads, g_o1, g_o2, len1, len2)
    err = lambda a, r: float((a.double() - r).abs().max() / r.abs().max())
    lonely = _lonely(name)
    ptrs = (_ptr(len1), _ptr(len2))
    for gname, side, a, again, b, r in zip(GRADS, SIDE_OF_GRAD, res["grads"], res["again"], res["yard"], ref):
        assert a.shape == r.shape and a.dtype == torch.float32 and torch.isfinite(a).all(), gname
        assert _bits(a, again), gname
        e_new, e_yard = err(a, r), err(b, r)
        print(f"{name} {heads} heads {gname}: new {e_new:.3e}, batch path {e_yard:.3e}")
        assert e_new <= 2 * e_yard + 1e-6, gname
        ptr = ptrs[side]
        for x in lonely[side]:
            assert (a[ptr[x]:ptr[x + 1]] == 0).all() and (r[ptr[x]:ptr[x + 1]] == 0).all(), (gname, x)
        assert a.abs().max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("heads,width", HEAD_SHAPES, ids=HEAD_IDS)
@pytest.mark.parametrize("name", list(CASES))
def test_node_scores_in_both_launch_orders(name, heads, width):
    """attn_node_scores_pairs_kernel with `swap` of node_scores_pairs TRUE (avg(LEN2) > avg(LEN1): the problem whose
    queries are the molecules' atoms goes first; no other test swaps it), false, and at the tie; the third `locate`
    chunk over kout_ptr; `l0 = qout_ptr[b]` far from `q0` in either direction; [3x16] the scalar lse loads of the
    `H % 4 != 0` branch.  Bitwise the batch kernel on gathered rows, rel_err < 1e-5 against a dense fp64 softmax, exact
    0 for the keys of query-less pairs."""
    len1, len2, pairs = _lens(name)
    t = _tables(name)
    ops, _, _, res = _case(name, heads, width)
    d = [x.double() for x in ops]
    p1, p2, g1, g2 = _ptr(len1), _ptr(len2), pairs[:, 0], pairs[:, 1]
    ref = NS._dense_ref(d[0], d[1], p1, p2, g1, g2, heads) + NS._dense_ref(d[3], d[4], p2, p1, g2, g1, heads)
    plan = t["plan"]
    for i, vec in enumerate(NS.NAMES):
        a, b = res["scores"][i], res["batch_scores"][i]
        assert a.shape == ((t["rows2"],) if i < 2 else (t["rows1"],)), vec
        assert _bits(a, b), vec
        assert torch.isfinite(a).all() and (a >= 0).all() and (a <= 1).all(), vec
        e = rel_err(a, ref[i])
        print(f"{name} {heads} heads {vec}: rel_err {e:.3e}")
        assert e < 1e-5, vec
    seen = 0
    for mean, mx, qlen, klen in ((0, 1, len1[g1], len2[g2]), (2, 3, len2[g2], len1[g1])):
        queryless = torch.from_numpy(np.repeat(qlen == 0, klen))
        assert (res["scores"][mean][queryless] == 0).all() and (res["scores"][mx][queryless] == 0).all()
        seen += int(queryless.sum())
    if len(pairs) == NPAIR or name == "only_empty_partners":
        assert seen > 0


# ---------------------------------------------------------------------------------------------------------------------
# the order of the ordered sum
WIDTHS = [4, 36, 128, 260]       # one float4 per row; 36; 16 rows x 32 float4 = exactly one WAVE * EPL trip; three trips, the last partial
ORDER_TABLES = ("one_protein_many_drugs", "seventy_pairs")


@functools.lru_cache(maxsize=None)
def _order_lens(which):
    if which == "seventy_pairs":                 # graph lengths 17, 0, 16, 33, 5 / 1, 15, 0, 16, 40, 3: tiles of 1, 5 and 16 rows
        return np.asarray(PT.LEN1, dtype=np.int64), np.asarray(PT.LEN2, dtype=np.int64), PT._pair_list()
    return _lens(which)


def _sides(which):
    """-> per side (lens, graph of every pair, optr, inv_ptr, inv_pairs) on the host"""
    len1, len2, pairs = _order_lens(which)
    plan = pt.plan_pair_training(len1, len2, pairs)
    return ((len1, plan.g1, plan.optr1, plan.inv1_ptr, plan.inv1_pairs), (len2, plan.g2, plan.optr2, plan.inv2_ptr, plan.inv2_pairs))


@functools.lru_cache(maxsize=None)
def _g_rows(which, side, width):
    """non-integer fp32, magnitudes 10 ** U(-3, 3), random signs: fp32 addition of such rows does not commute in order"""
    rows = int(_sides(which)[side][2][-1])
    rng = np.random.default_rng(7 + 1000 * side + width + (0 if which == "seventy_pairs" else 500))
    mag = 10.0 ** rng.uniform(-3, 3, (rows, width))
    return (mag * rng.choice([-1.0, 1.0], (rows, width))).astype(np.float32)


def _ordered_sum(part, lens, graph, optr, descending=False):
    """fp32 on the CPU: for each unique row start from 0.0f and add the pairs' rows ONE AT A TIME, in ascending (or
    descending) pair index.  The pairs of a graph come from `graph` itself, not from the inverse tables."""
    src_ptr = _ptr(lens)
    dst = np.zeros((int(src_ptr[-1]), part.shape[1]), dtype=np.float32)
    for x in range(len(lens)):
        mine = np.nonzero(np.asarray(graph) == x)[0]
        acc = np.zeros((int(lens[x]), part.shape[1]), dtype=np.float32)
        for b in (mine[::-1] if descending else mine):
            acc = acc + part[optr[b]:optr[b] + lens[x]]
        assert acc.dtype == np.float32
        dst[src_ptr[x]:src_ptr[x + 1]] = acc
    return dst


@pytest.mark.parametrize("width", WIDTHS)
def test_the_inputs_tell_ascending_from_descending_order(width):
    """No GPU: on the inputs of the two GPU tests below, adding a graph's pairs in DESCENDING order gives other bits than
    adding them in ascending order, at every width, on both tables and on every side that has an order (the molecules of
    the 131-pair list are in one pair each) -- so a kernel that walks its inverse list in another order cannot pass them."""
    for which in ORDER_TABLES:
        for side, (lens, graph, optr, _, _) in enumerate(_sides(which)):
            part = _g_rows(which, side, width)
            up, down = _ordered_sum(part, lens, graph, optr), _ordered_sum(part, lens, graph, optr, descending=True)
            differ = int((up.view(np.int32) != down.view(np.int32)).sum())
            print(f"{which} side {side + 1} width {width}: {differ} of {up.size} elements differ between the orders")
            if (which, side) == ("one_protein_many_drugs", 1):       # every molecule is in ONE pair: nothing to order
                assert np.bincount(graph).max() == 1 and differ == 0
                continue
            assert np.bincount(graph).max() >= 13 and differ > 0, (which, side)
            assert np.allclose(up, down, rtol=1e-3, atol=1e-2)       # (the same sum all the same)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("width", WIDTHS)
def test_reduce_rows_adds_in_ascending_pair_order(width):
    """reduce_rows_kernel through `expand_rows_train`'s backward: the walk `nxt = optr[inv_pairs[j0]]; for j in j0 .. j1:
    src = part + (nxt + off) * W4; if (j + 1 < j1) nxt = optr[inv_pairs[j + 1]]; acc[e] += src[i]`, repeated per `base`
    trip of WAVE * EPL float4s (width 260: three trips, each must start again at j0 with fresh accumulators).  The
    kernel does `acc = 0; acc += src` per pair and the build has no fast-math, so the result is BITWISE the fp32 loop of
    `_ordered_sum` -- a skipped prefetch, an off-by-one at `j + 1 < j1` or a stale `nxt` in a later trip gives other
    bits, as the CPU test above shows for the reversed order.  131 pairs into one graph, and the 70-pair list.
    (Tried on an MI355X: a build that walks the list in descending order fails every width here and in the test below,
    one that keeps `nxt` across the `base` trips fails width 260 alone.)"""
    for which in ORDER_TABLES:
        for side, (lens, graph, optr, inv_ptr, inv_pairs) in enumerate(_sides(which)):
            part = _g_rows(which, side, width)
            want = torch.from_numpy(_ordered_sum(part, lens, graph, optr))
            src_ptr = _ptr(lens)
            leaf = torch.zeros(int(src_ptr[-1]), width, device=DEV, requires_grad=True)
            rows, _ = pt.expand_rows_train(leaf, _dev(src_ptr), _dev(graph), _dev(optr), _dev(inv_ptr), _dev(inv_pairs), int(optr[-1]))
            (got,) = torch.autograd.grad(rows, leaf, _dev(part))
            torch.cuda.synchronize()
            got = got.cpu()
            print(f"{which} side {side + 1} width {width}: {int((got != want).sum())} of {got.numel()} elements differ")
            assert _bits(got, want), (which, side)


@pytest.mark.gpu
@pytest.mark.parametrize("width", WIDTHS)
def test_reduce_rows_writes_its_graphs_rows_and_nothing_else(width):
    """`cgvp_reduce_rows` directly, `dst` a view of `num_dst > src_ptr[-1]` rows inside a canary-filled allocation: the
    rows of every graph are the ascending-order sum (bitwise), rows of a graph no pair references are exactly 0, and the
    rows behind src_ptr[-1] and the canaries on both sides are untouched, as the op's docstring promises (`units =
    ceil(num_dst / 16) + G` is an upper bound: `locate(J.src_ptr, J.G, ...)` returns false past the last graph's tile)."""
    from gvp_hip.ops import _stream
    CANARY, PAD, EXTRA = -7.0, 3, 21
    for which in ORDER_TABLES:
        for side, (lens, graph, optr, inv_ptr, inv_pairs) in enumerate(_sides(which)):
            part_h = _g_rows(which, side, width)
            want = torch.from_numpy(_ordered_sum(part_h, lens, graph, optr))
            src_ptr = _ptr(lens)
            n_src, num_dst = int(src_ptr[-1]), int(src_ptr[-1]) + EXTRA
            buf = torch.full((PAD + num_dst + PAD, width), CANARY, device=DEV)
            dst = buf[PAD:PAD + num_dst]
            assert dst.data_ptr() % 16 == 0 and dst.is_contiguous()
            part, tabs = _dev(part_h), [_dev(x) for x in (optr, inv_ptr, inv_pairs, src_ptr)]
            torch.cuda.synchronize()
            rc = pt.lib().cgvp_reduce_rows(part.data_ptr(), *(x.data_ptr() for x in tabs), len(lens), len(graph), part.shape[0],
                                           num_dst, width, dst.data_ptr(), _stream())
            torch.cuda.synchronize()
            assert rc == 0
            out = buf.cpu()
            assert (out[:PAD] == CANARY).all() and (out[PAD + n_src:] == CANARY).all(), (which, side)
            assert _bits(out[PAD:PAD + n_src].contiguous(), want), (which, side)
            unreferenced = [x for x in range(len(lens)) if lens[x] > 0 and not (np.asarray(graph) == x).any()]
            assert unreferenced or which != "seventy_pairs"
            for x in unreferenced:
                assert (out[PAD + src_ptr[x]:PAD + src_ptr[x + 1]] == 0).all(), (which, side, x)


# ---------------------------------------------------------------------------------------------------------------------
# logits of magnitude ~150 over a pair list
RESCALE_LEN1, RESCALE_LEN2 = [50, 40], [37, 70]
RESCALE_PAIRS = [(0, 0), (1, 1), (0, 1), (1, 0), (0, 0), (1, 1), (0, 1)]         # every graph is in at least three pairs
COMPARED = AE.OUTS + AE.GRADS          # o_r = o1, o_a = o2, lse_r = lse1, lse_a = lse2; g_q_r, g_k_a, g_v_a, g_q_a, g_k_r, g_v_r


def _rescale_plan():
    return pt.plan_pair_training(RESCALE_LEN1, RESCALE_LEN2, RESCALE_PAIRS)


def _rescale_idx(plan):
    rows = lambda lens, g: torch.from_numpy(np.concatenate([np.arange(_ptr(lens)[x], _ptr(lens)[x + 1]) for x in g]))
    return rows(RESCALE_LEN1, plan.g1), rows(RESCALE_LEN2, plan.g2)


def _stock_pairs(ops, g_o1, g_o2, dtype, dev="cpu"):
    """The dense formulation of test_attention_edges (`_dense`) on index_select-ed rows with autograd, in `dtype` on
    `dev` -> {name: tensor} of COMPARED; index_select's backward sums over the pairs."""
    plan = _rescale_plan()
    idx1, idx2 = (i.to(dev) for i in _rescale_idx(plan))
    leaves = [x.detach().to(device=dev, dtype=dtype).clone().requires_grad_() for x in ops]
    sel = lambda x, idx: torch.index_select(x, 0, idx)
    o1p, o2p = [int(x) for x in plan.optr1], [int(x) for x in plan.optr2]
    o_r, lse_r, _ = AE._dense(sel(leaves[0], idx1), sel(leaves[1], idx2), sel(leaves[2], idx2), o1p, o2p)
    o_a, lse_a, _ = AE._dense(sel(leaves[3], idx2), sel(leaves[4], idx1), sel(leaves[5], idx1), o2p, o1p)
    ((o_r * g_o1.to(device=dev, dtype=dtype)).sum() + (o_a * g_o2.to(device=dev, dtype=dtype)).sum()).backward()
    res = dict(zip(AE.OUTS, (o_r.detach(), o_a.detach(), lse_r, lse_a)))
    res.update({n: x.grad for n, x in zip(AE.GRADS, leaves)})
    return res


@functools.lru_cache(maxsize=None)
def _rescale_case():
    """The recipe of test_attention_edges._rescale_case on the rows of the UNIQUE graphs: seed 23, q x 2, k x 4, key row j
    of each graph x (1 + j / 16).  -> (operands, g_o1, g_o2, fp64 reference); shared by the CPU and the GPU test, never
    modified."""
    assert (AE.H, AE.HD, AE.Q_SCALE) == (8, 16, 2.0)
    plan = _rescale_plan()
    g = torch.Generator().manual_seed(23)
    N1, N2 = sum(RESCALE_LEN1), sum(RESCALE_LEN2)
    q1, k1, v1, q2, k2, v2 = [torch.randn(n, AE.E, generator=g) for n in (N1, N2, N2, N2, N1, N1)]
    g_o1, g_o2 = torch.randn(plan.rows1, AE.E, generator=g), torch.randn(plan.rows2, AE.E, generator=g)
    ramp = lambda lens: torch.cat([1 + torch.arange(n, dtype=torch.float32) / 16 for n in lens])[:, None]
    ops = (q1 * AE.Q_SCALE, k1 * 4 * ramp(RESCALE_LEN2), v1, q2 * AE.Q_SCALE, k2 * 4 * ramp(RESCALE_LEN1), v2)
    return ops, g_o1, g_o2, _stock_pairs(ops, g_o1, g_o2, torch.float64)


def _rescale_max_logit(ops):
    p1, p2 = _ptr(RESCALE_LEN1), _ptr(RESCALE_LEN2)
    top = 0.0
    for a, b in RESCALE_PAIRS:
        for q, k, qs, ks in ((ops[0], ops[1], slice(p1[a], p1[a + 1]), slice(p2[b], p2[b + 1])),
                             (ops[3], ops[4], slice(p2[b], p2[b + 1]), slice(p1[a], p1[a + 1]))):
            qb = q[qs].double().view(-1, AE.H, AE.HD).transpose(0, 1)
            kb = k[ks].double().view(-1, AE.H, AE.HD).transpose(0, 1)
            top = max(top, float((qb @ kb.transpose(1, 2) / 4.0).abs().max()))
    return top


def test_large_logits_over_a_pair_list_are_reachable_by_the_documented_arithmetic_cpu():
    """No GPU: the fp32 arithmetic the kernels are documented to do -- `_kernel_arithmetic_fp32` of
    test_attention_edges per pair on gathered fp32 rows, then the ascending-order fp32 sum over each graph's pairs -- stays
    within max(4 e_stock, 2e-6 scale) of fp64 for o, lse and all six gradients on exactly the inputs of the GPU test
    below, e_stock being the dense formulation in stock fp32 with autograd: the GPU test's cap is one the kernels can
    meet.  Measured e_emulation / e_stock here, at max |logit| = 189.7: o 1.00 / 1.00, lse 1.00 / 1.00, g_q 1.93 / 1.21,
    g_k 2.07 / 1.23, g_v 1.58 / 2.14 (direction 1 / direction 2)."""
    ops, g_o1, g_o2, ref = _rescale_case()
    top = _rescale_max_logit(ops)
    print(f"max |logit| {top:.1f}")
    assert 100 <= top <= 250
    stock = _stock_pairs(ops, g_o1, g_o2, torch.float32)
    plan = _rescale_plan()
    idx1, idx2 = _rescale_idx(plan)
    o1p, o2p = [int(x) for x in plan.optr1], [int(x) for x in plan.optr2]
    side1, side2 = (RESCALE_LEN1, plan.g1, plan.optr1), (RESCALE_LEN2, plan.g2, plan.optr2)
    osum = lambda part, side: torch.from_numpy(_ordered_sum(part.numpy(), *side))
    emu = {}
    for (q, k, v, g, qi, ki, qp, kp, qside, kside), (o, lse, g_q, g_k, g_v) in (
            ((ops[0], ops[1], ops[2], g_o1, idx1, idx2, o1p, o2p, side1, side2), ("o_r", "lse_r", "g_q_r", "g_k_a", "g_v_a")),
            ((ops[3], ops[4], ops[5], g_o2, idx2, idx1, o2p, o1p, side2, side1), ("o_a", "lse_a", "g_q_a", "g_k_r", "g_v_r"))):
        out, ls, pq, pk, pv, _ = AE._kernel_arithmetic_fp32(q[qi], k[ki], v[ki], g, qp, kp)
        assert all(x.dtype == torch.float32 for x in (out, ls, pq, pk, pv))
        emu.update({o: out, lse: ls, g_q: osum(pq, qside), g_k: osum(pk, kside), g_v: osum(pv, kside)})
    AE._no_worse_than_4x_stock(emu, stock, ref, "emulation", COMPARED)


@pytest.mark.gpu
def test_large_logits_over_a_pair_list():
    """Logits of magnitude ~150 through the pair-list kernels: `alpha = fexp(m - m_new)` < 1 at every key tile of
    attn_fwd_pairs_kernel for some queries and == 1 for others, exp underflows for most keys, and both backward kernels
    recompute `pr = fexp(st - lse)` from the fp32 lse stored per PAIR row (read through `shift` in the d K / d V kernel).
    Three checks on the same tensors: out / lse are bitwise the batch kernel on gathered rows; o, lse and the six
    gradients meet e_ours <= max(4 e_stock, 2e-6 scale) against fp64 with stock torch in fp32 on the device as yardstick
    (test_attention_edges.test_rescale_every_tile's cap); the four node-score vectors are bitwise the batch node-score
    kernel and meet the same cap with a stock fp32 softmax as yardstick.
    Measured e_ours / e_stock on an MI355X: o_r 1.14, o_a 0.85, lse_r 0.99, lse_a 1.00, g_q_r 1.36, g_k_a 0.81, g_v_a 1.90,
    g_q_a 1.15, g_k_r 1.74, g_v_r 2.06 (largest e_ours: g_q_r 3.9e-4 at scale 93); atom_mean 2.55, atom_max 1.17,
    residue_mean 2.10, residue_max 1.59 (e_ours at most 5.5e-7)."""
    ops, g_o1, g_o2, ref = _rescale_case()
    t = PT._tables_of(np.asarray(RESCALE_PAIRS), RESCALE_LEN1, RESCALE_LEN2)
    res = _run_everything(list(ops), g_o1, g_o2, t, AE.H)
    for i, what in enumerate(AE.OUTS):
        assert _bits(res["fwd"][i], res["batch_fwd"][i]), what
    ours = dict(zip(COMPARED, res["fwd"] + res["grads"]))
    for a, b in zip(res["grads"], res["again"]):
        assert _bits(a, b)
    stock = _stock_pairs(ops, g_o1, g_o2, torch.float32, DEV)
    AE._no_worse_than_4x_stock(ours, stock, ref, "kernel", COMPARED)
    # node scores
    p1, p2 = _ptr(RESCALE_LEN1), _ptr(RESCALE_LEN2)
    g1, g2 = t["plan"].g1, t["plan"].g2
    dense = lambda o: dict(zip(NS.NAMES, NS._dense_ref(o[0], o[1], p1, p2, g1, g2, AE.H) + NS._dense_ref(o[3], o[4], p2, p1, g2, g1, AE.H)))
    for i, vec in enumerate(NS.NAMES):
        assert _bits(res["scores"][i], res["batch_scores"][i]), vec
    AE._no_worse_than_4x_stock(dict(zip(NS.NAMES, res["scores"])), dense([x.to(DEV) for x in ops]), dense([x.double() for x in ops]),
                               "kernel", NS.NAMES)
