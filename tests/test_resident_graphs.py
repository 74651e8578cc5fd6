"""Batches collated on the device from a resident store (gvp_hip.resident, cgvp_collate_graphs), on the MI355X.

The oracle everywhere is the host collate the project already has, `davis_synth.to_torch(davis_synth.collate([...]))`
plus `ptr`, and every comparison of a collated tensor is BITWISE (floats through their int32 view: the kernel is a copy,
so NaN payloads and -0.0 must come through; the seeded inputs are random bit patterns and hold some of each)."""
import json
import os

import numpy as np
import pytest
import torch

import davis_synth as ds
from conftest import GOLDEN
from gvp_hip import resident

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

A_NODES = (1, 2, 3, 4, 5, 16, 17, 63, 64, 65, 129, 300, 301, 7)
A_EDGES = (0, 1, 4, 7, 48, 51, 190, 193, 200, 777, 900, 901, 0, 3)
B_ATOMS = (1, 2, 3, 5, 8, 13, 21, 34, 40, 4, 17, 29)


def _bits(rng, *shape):
    """float32 of random BIT PATTERNS (about one in 256 is a NaN with a random payload, some are denormal or inf) with a
    -0.0 and two chosen NaN payloads put in where there is room."""
    a = rng.integers(0, 2 ** 32, size=shape, dtype=np.uint32)
    flat = a.reshape(-1)
    for at, word in ((0, 0x80000000), (1, 0x7FC12345), (2, 0xFFA00001)):
        if flat.shape[0] > at:
            flat[at] = word
    return a.view(np.float32)


def _graph(rng, n, e, vector):
    ei = rng.integers(0, n, size=(2, e)).astype(np.int64)
    ids = lambda k, hi: rng.integers(0, hi, size=k).astype(np.int64)
    if vector:
        return dict(x_s=_bits(rng, n, 17), x_v=_bits(rng, n, 3, 3), edge_index=ei, e_s=_bits(rng, e, 32),
                    e_v=_bits(rng, e, 1, 3), ntypes=ids(n, 20), etypes=ids(e, 2))
    return dict(x_s=_bits(rng, n, 41), x_v=None, edge_index=ei, e_s=_bits(rng, e, 9), e_v=None, ntypes=ids(n, 11),
                etypes=ids(e, 5))


class Store:
    def __init__(self, name):
        rng = np.random.default_rng(2024 if name == "A" else 2025)
        if name == "A":       # protein layout: rows of 68, 36, 8 (nodes) and 128, 12, 8 (edges) bytes
            self.graphs = [_graph(rng, n, e, True) for n, e in zip(A_NODES, A_EDGES)]
        else:                 # drug layout: rows of 164, 8 and 36, 8 bytes
            edges = [0 if i in (0, len(B_ATOMS) - 2) else int(rng.integers(1, 3 * n + 1)) for i, n in enumerate(B_ATOMS)]
            self.graphs = [_graph(rng, n, e, False) for n, e in zip(B_ATOMS, edges)]
        self.store = resident.ResidentGraphs(self.graphs, DEV)
        self._oracles = {}

    def oracle(self, ids):
        """The host collate of graphs `ids`, uploaded, plus ptr (computed once per id list, never written to)."""
        key = tuple(int(i) for i in ids)
        if key not in self._oracles:
            gb = ds.collate([self.graphs[i] for i in key])
            d = {k: (tuple(t.to(DEV) for t in v) if isinstance(v, tuple) else v.to(DEV)) for k, v in ds.to_torch(gb).items()}
            d["ptr"] = torch.from_numpy(gb.ptr).to(DEV)
            self._oracles[key] = d
        return self._oracles[key]


@pytest.fixture(scope="module")
def stores():
    return {"A": Store("A"), "B": Store("B")}


def _flat(d):
    out = {}
    for k, v in d.items():
        if isinstance(v, tuple):
            out.update({f"{k}[{i}]": t for i, t in enumerate(v)})
        else:
            out[k] = v
    return out


def _bitwise(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, tuple(got.shape), tuple(want.shape))
    a, b = got.contiguous(), want.contiguous()
    if a.is_floating_point():
        a, b = a.view(torch.int32), b.view(torch.int32)
    assert torch.equal(a, b), what


def _check(got, want, fresh=True):
    assert list(got) == ["x", "edge_index", "ntypes", "etypes", "eattr", "batch", "ptr"]
    assert isinstance(got["x"], tuple) == isinstance(want["x"], tuple) == isinstance(got["eattr"], tuple)
    got, want = _flat(got), _flat(want)
    assert set(got) == set(want)
    for k in want:
        assert got[k].device == want[k].device, k
        if fresh:
            assert got[k].is_contiguous(), k
        _bitwise(got[k], want[k], k)


def _in_range(d):
    """edge_index stays inside each graph's node range, and batch / ptr describe the same partition."""
    ptr, batch, ei = d["ptr"].cpu(), d["batch"].cpu(), d["edge_index"].cpu()
    assert ptr[0] == 0 and ptr[-1] == batch.shape[0] and (ptr[1:] >= ptr[:-1]).all()
    assert torch.equal(batch, torch.repeat_interleave(torch.arange(ptr.shape[0] - 1), ptr[1:] - ptr[:-1]))
    if ei.shape[1]:
        g = batch[ei[0]]
        assert torch.equal(g, batch[ei[1]]) and (ei >= ptr[g]).all() and (ei < ptr[g + 1]).all()


CASES = {
    "first": lambda n: [0],
    "in_order": lambda n: list(range(n)),
    "reversed": lambda n: list(range(n))[::-1],
    "repeats": lambda n: [3, 3, 0, 3],
    "last": lambda n: [n - 1],
    "zero_edge_first": lambda n: [0, n - 2, 5, n - 1, 0],
}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("name", ["A", "B"])
def test_collate_is_bitwise_the_host_collate(stores, name, case):
    s = stores[name]
    ids = CASES[case](len(s.store))
    if case == "zero_edge_first":
        assert s.store.num_edges(ids[0]) == 0 and s.store.num_edges(ids[1]) == 0
    plan = s.store.plan(ids)
    got = s.store.collate(plan)
    _check(got, s.oracle(ids))
    _in_range(got)
    assert got["ptr"].data_ptr() == plan.table.data_ptr() + 8 * plan.B         # a slice of the one uploaded table
    assert (got["batch"].shape[0], got["edge_index"].shape[1]) == (plan.N, plan.E)


def test_collate_of_300_draws_with_replacement(stores):
    s = stores["B"]
    ids = np.random.default_rng(9).integers(0, len(s.store), size=300)
    got = s.store.collate(s.store.plan(ids))
    _check(got, s.oracle(ids))
    _in_range(got)


def test_collate_of_an_empty_batch(stores):
    for s in stores.values():
        got = _flat(s.store.collate(s.store.plan([])))
        assert got["ptr"].tolist() == [0] and got["edge_index"].shape == (2, 0)
        assert all(t.shape[0] == 0 for k, t in got.items() if k not in ("ptr", "edge_index"))


F_CANARY, I_CANARY = 0x7FC0BEEF, 0x5A5A5A5A5A5A5A5A


def _canary_buffers(store, plan, extra=37, behind=5):
    """`out=` buffers that are slices [1 : 1 + rows + extra] of larger allocations filled with a canary word: the
    destination base is one row off the allocation (68, 36, 12 ... bytes, none a multiple of 16) -> (out, big)."""
    like = _flat(store.collate(plan))
    big, out = {}, {}
    for k, t in like.items():
        if k == "ptr":
            continue
        rows = t.shape[1] if k == "edge_index" else t.shape[0]
        shape = (2, rows + 1 + extra + behind) if k == "edge_index" else (rows + 1 + extra + behind,) + tuple(t.shape[1:])
        if t.is_floating_point():
            big[k] = torch.full(shape, F_CANARY, dtype=torch.int32, device=DEV).view(torch.float32)
        else:
            big[k] = torch.full(shape, I_CANARY, dtype=torch.int64, device=DEV)
        out[k] = big[k][:, 1:1 + rows + extra] if k == "edge_index" else big[k][1:1 + rows + extra]
    nest = {k: v for k, v in out.items() if "[" not in k}
    for k in ("x", "eattr"):
        if f"{k}[0]" in out:
            nest[k] = (out[f"{k}[0]"], out[f"{k}[1]"])
    return nest, big


def _canaries_intact(big, plan):
    for k, t in big.items():
        edge = k in ("edge_index", "etypes") or k.startswith("eattr")
        rows = plan.E if edge else plan.N
        words = t.view(torch.int32) if t.is_floating_point() else t
        want = F_CANARY if t.is_floating_point() else I_CANARY
        if k == "edge_index":
            outside = torch.cat([words[:, :1], words[:, 1 + rows:]], dim=1)
        else:
            outside = torch.cat([words[:1], words[1 + rows:]])
        assert outside.numel() > 0 and bool((outside == want).all()), k     # in front of the slice, behind the rows, behind the slice


@pytest.mark.parametrize("name", ["A", "B"])
def test_misaligned_out_buffers_and_no_stray_writes(stores, name):
    s = stores[name]
    ids = list(range(len(s.store)))[::-1] + [3, 0]
    plan = s.store.plan(ids)
    out, big = _canary_buffers(s.store, plan)
    bases = {k: t.data_ptr() % 16 for k, t in _flat(out).items()}
    if name == "A":
        assert (bases["x[0]"], bases["x[1]"], bases["eattr[1]"], bases["batch"]) == (68 % 16, 36 % 16, 12, 8)
    got = s.store.collate(plan, out=out)
    for k, t in _flat(got).items():
        if k != "ptr":
            assert t.data_ptr() == _flat(out)[k].data_ptr(), k               # views of the caller's buffers
    _check(got, s.oracle(ids), fresh=False)
    _canaries_intact(big, plan)


@pytest.mark.parametrize("max_blocks", [1, 3])
def test_few_workgroups_walk_several_tiles_each(stores, max_blocks):
    s = stores["A"]
    ids = [11, 12, 9]
    plan = s.store.plan(ids)
    assert plan.E * 128 > 16 * 4096 * max_blocks                              # e_s alone: many 4 KB tiles per workgroup
    _check(s.store.collate(plan, max_blocks=max_blocks), s.oracle(ids))
    out, big = _canary_buffers(s.store, plan)
    _check(s.store.collate(plan, out=out, max_blocks=max_blocks), s.oracle(ids), fresh=False)
    _canaries_intact(big, plan)


def test_out_buffers_are_refused_before_any_launch(stores, monkeypatch):
    s = stores["A"]
    plan = s.store.plan([5, 6, 2])
    good, _ = _canary_buffers(s.store, plan)
    launches = []
    monkeypatch.setattr(resident, "lib", lambda: launches.append("lib") or pytest.fail("launched"))

    def with_(key, t, slot=None):
        d = dict(good)
        d[key] = t if slot is None else tuple(t if i == slot else v for i, v in enumerate(good[key]))
        return d

    xs, xv = good["x"]
    bad = [
        with_("x", xs[:plan.N - 1], 0),                                        # too few rows
        with_("eattr", good["eattr"][1][:plan.E - 1], 1),
        with_("edge_index", good["edge_index"][:, :plan.E - 1]),
        with_("batch", good["batch"][:plan.N - 1]),
        with_("x", xs.double(), 0),                                            # wrong dtype
        with_("ntypes", good["ntypes"].int()),
        with_("edge_index", good["edge_index"].float()),
        with_("x", xv.cpu(), 1),                                               # another device
        with_("etypes", good["etypes"].cpu()),
        with_("x", torch.empty(17, xs.shape[0], device=DEV).t(), 0),           # not contiguous
        with_("batch", torch.empty(2 * plan.N + 80, dtype=torch.int64, device=DEV)[::2]),
        with_("edge_index", torch.empty(plan.E + 40, 2, dtype=torch.int64, device=DEV).t()),
        with_("x", torch.empty(xs.shape[0], 18, device=DEV), 0),               # wrong trailing dimensions
        with_("eattr", torch.empty(good["eattr"][1].shape[0], 3, device=DEV), 1),
        with_("edge_index", torch.empty(3, plan.E, dtype=torch.int64, device=DEV)),
        with_("x", xs),                                                        # not the pair of tensors
        {k: v for k, v in good.items() if k != "batch"},                      # a tensor missing
    ]
    for d in bad:
        with pytest.raises(ValueError):
            s.store.collate(plan, out=d)
    with pytest.raises(ValueError):                                            # another store's plan: other graph sizes
        s.store.collate(stores["B"].store.plan([0, 1]))
    assert launches == []
    monkeypatch.undo()
    _check(s.store.collate(plan, out=good), s.oracle([5, 6, 2]), fresh=False)   # the good buffers do pass


def test_captured_collate_replays_another_plan_of_the_same_totals(stores):
    s = stores["A"]
    ids_a = [9, 3, 12, 0, 11, 6]
    ids_b = [0, 11, 9, 6, 3, 12]                                               # a permutation: the same (B, N, E)
    plan_a, plan_b = s.store.plan(ids_a), s.store.plan(ids_b)
    assert (plan_a.B, plan_a.N, plan_a.E) == (plan_b.B, plan_b.N, plan_b.E)
    bufs, big = _canary_buffers(s.store, plan_a)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s.store.collate(plan_a, out=bufs)                                      # warm-up on the capture stream
    side.synchronize()
    for t in _flat(bufs).values():                                             # forget the warm-up's result
        (t.view(torch.int32) if t.is_floating_point() else t).fill_(F_CANARY if t.is_floating_point() else I_CANARY)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        got = s.store.collate(plan_a, out=bufs)
    g.replay()
    torch.cuda.synchronize()
    _check(got, s.oracle(ids_a), fresh=False)
    plan_a.table.copy_(plan_b.table)
    g.replay()
    torch.cuda.synchronize()
    _check(got, s.oracle(ids_b), fresh=False)                                  # ptr too: it is a slice of the table
    _canaries_intact(big, plan_a)


# ------------------------------------------------------------------------------------------------ where the batches go
def _to(d):
    return {k: (tuple(t.to(DEV) for t in v) if isinstance(v, tuple) else v.to(DEV)) for k, v in d.items()}


def _host_batch(graphs):
    gb = ds.collate(graphs)
    d = _to(ds.to_torch(gb))
    d["ptr"] = torch.from_numpy(gb.ptr).to(DEV)
    return d


def _close(got, want, what):
    """The project's forward bar (tests/test_pair_scoring.py::_close)."""
    bound = 1e-4 * want.abs().clamp_min(1.0)
    diff = (got - want).abs()
    print(f"{what}: max |delta| {float(diff.max()):.3e}, max |prediction| {float(want.abs().max()):.3e}")
    assert got.shape == want.shape and torch.isfinite(got).all(), what
    assert (diff <= bound).all(), what


@pytest.fixture(scope="module")
def davis(pretrained):
    from models.joint_gnn import JointGNN
    rng = np.random.default_rng(17)
    prots = [ds.protein_graph(L, rng) for L in (20, 33, 47)]
    drugs = [ds.drug_graph(rng) for _ in range(4)]
    kw = json.load(open(os.path.join(GOLDEN, "model_kwargs.json")))
    model = JointGNN(protein_gnn_kwargs=kw["protein_gnn_kwargs"], molecule_gnn_kwargs=kw["molecule_gnn_kwargs"],
                     **kw["joint_gnn_kwargs"])
    model.load_state_dict(pretrained, strict=True)
    index = np.array([(p, m) for p in range(3) for m in range(4)], dtype=np.int64)
    y = torch.arange(12, dtype=torch.float32).reshape(12, 1) * 0.5
    rp = resident.ResidentPairs(resident.ResidentGraphs(prots, "cuda"), resident.ResidentGraphs(drugs, "cuda"), index, y)
    assert rp.device == torch.device(DEV)                                      # "cuda" is the device the tensors landed on
    return model.to(DEV).eval(), prots, drugs, rp


def test_pair_batches_feed_the_encoders_and_the_model(davis):
    model, prots, drugs, rp = davis
    ids = [7, 0, 11, 4, 4, 2]
    pdata, mdata, y = rp.batch(ids)
    assert torch.equal(y, rp.y[torch.tensor(ids, device=DEV)]) and y.shape == (6, 1)
    hp = _host_batch([prots[p] for p, _ in rp.pair_index[ids]])
    hm = _host_batch([drugs[m] for _, m in rp.pair_index[ids]])
    _check(pdata, hp)
    _check(mdata, hm)
    strip = lambda d: {k: v for k, v in d.items() if k != "ptr"}
    with torch.no_grad():
        # bitwise equal inputs and a bit-reproducible forward: bitwise equal encoder outputs
        _bitwise(model.protein_gnn(**strip(pdata)), model.protein_gnn(**strip(hp)), "protein_gnn")
        _bitwise(model.molecule_gnn(**strip(mdata)), model.molecule_gnn(**strip(hm)), "molecule_gnn")
        # the whole model pools with atomics: the project's forward bar
        _close(model(pdata, mdata)[0], model(hp, hm)[0], "forward")


def test_block_goes_into_forward_pairs_without_a_host_read(davis, monkeypatch):
    from models.joint_gnn import JointGNN
    model, prots, drugs, rp = davis
    pids, mids = [2, 0], [3, 1, 0]
    pairs = [(0, 0), (1, 2), (0, 1), (1, 1), (0, 2)]
    hp, hm = _host_batch([prots[i] for i in pids]), _host_batch([drugs[i] for i in mids])
    with torch.no_grad():
        want = model.forward_pairs(hp, hm, pairs)[0]                           # one host read: ptr of both sides

    def no_read(*a, **k):
        raise AssertionError("forward_pairs read its tables back to the host")

    monkeypatch.setattr(JointGNN, "_read_pair_tables", staticmethod(no_read))
    pdata, mdata, plan = rp.block(pids, mids, pairs)
    _check(pdata, hp)
    _check(mdata, hm)
    with torch.no_grad():
        got = model.forward_pairs(pdata, mdata, plan)[0]
    _close(got, want, "forward_pairs")
    assert got.shape == (len(pairs), 1)
