"""Resident graph stores, host side (no GPU): the header of the collate entry point, the plan tables, the refusals and
the batch sampler.  The kernel is tested in tests/test_resident_graphs.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import davis_synth as ds
from conftest import REPO
from gvp_hip import _lib, pair_training as pt, resident


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(cgvp_[a-z0-9_]+)\s*\(", text))


def test_entry_points_have_a_header_and_a_version_of_their_own():
    header = os.path.join(REPO, "include", "caster_gvp_resident.h")
    assert _declared(header) == set(resident.exported_symbols()) == {"cgvp_resident_version", "cgvp_collate_graphs"}
    main = open(os.path.join(REPO, "include", "caster_gvp.h")).read()
    handle = C.CDLL(_lib.LIB_PATH)
    for name in resident.exported_symbols():
        assert hasattr(handle, name), name
        assert name not in main and name not in _lib.exported_symbols(), name
    assert "#define CGVP_RESIDENT_VERSION 1\n" in open(header).read()
    assert resident.lib().cgvp_resident_version() == 1 == resident.RESIDENT_VERSION
    assert _lib.abi_header_digest() == _lib.ABI_HEADER_SHA256


def test_the_entry_point_refuses_bad_arguments_before_any_launch():
    """Every refusal returns before the first HIP call, so it can be asked for without a GPU."""
    L = resident.lib()
    table = np.zeros(8, dtype=np.int64)
    t = table.ctypes.data
    room = 0x100000                                  # a 16-byte aligned address; no refusal dereferences it
    items = (resident.CollateItem * 17)()
    items[0] = resident.CollateItem(room, room, 8, resident.NODE_ROWS)
    call = lambda its, n, sel=t, B=1, N=1, E=1, mb=0: L.cgvp_collate_graphs(its, n, sel, t, t, t, t, B, N, E, mb, None)
    BAD = -1
    assert call(None, 1) == BAD and call(items, 17) == BAD and call(items, -1) == BAD
    assert call(items, 1, sel=None) == BAD and call(items, 1, sel=t + 4) == BAD
    assert call(items, 1, B=-1) == BAD and call(items, 1, N=-1) == BAD and call(items, 1, E=-1) == BAD
    assert call(items, 1, mb=-1) == BAD
    for dst, src, row, kind in ((room, room, 6, 0), (room, room, 0, 1), (room + 2, room, 8, 0), (room, room + 2, 8, 1),
                                (room + 4, room, 8, resident.BATCH), (room, room + 4, 8, resident.ENDPOINTS),
                                (room, room, 12, resident.ENDPOINTS), (room, room, 8, 4), (0, room, 8, 0), (room, 0, 8, 1)):
        items[0] = resident.CollateItem(dst, src, row, kind)
        assert call(items, 1) == BAD, (dst - room, src - room, row, kind)
    # nothing to do is not an error, and launches nothing: no position, or no row
    items[0] = resident.CollateItem(room, room, 8, resident.NODE_ROWS)
    assert call(items, 1, B=0, N=0, E=0) == 0 and call(items, 1, B=1, N=0, E=0) == 0 and call(items, 0) == 0


def _graphs(seed=3):
    rng = np.random.default_rng(seed)
    prots = [ds.protein_graph(L, rng) for L in (5, 9, 1, 12, 7)]
    drugs = [ds.drug_graph(rng, n) for n in (3, 8, 1, 5)]
    return prots, drugs


def _ptr(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


@pytest.mark.parametrize("ids", [[0], [], [3, 3, 0, 3], [4, 3, 2, 1, 0], np.array([2, 2], dtype=np.int32), (1,)])
def test_plan_tables_are_cumulative_sums_over_the_selected_graphs(ids):
    prots, _ = _graphs()
    store = resident.ResidentGraphs(prots, "cpu")
    n = np.array([g["x_s"].shape[0] for g in prots])
    e = np.array([g["edge_index"].shape[1] for g in prots])
    assert len(store) == 5 and [store.num_nodes(i) for i in range(5)] == list(n)
    assert [store.num_edges(i) for i in range(5)] == list(e)
    assert np.array_equal(store.node_off, _ptr(n)) and np.array_equal(store.edge_off, _ptr(e))
    assert store.nbytes == sum(int(np.asarray(v).nbytes) for g in prots for v in g.values()) + 8 * 12
    plan = store.plan(ids)
    sel = np.asarray(ids, dtype=np.int64)
    assert isinstance(plan.N, int) and isinstance(plan.E, int) and isinstance(plan.B, int)
    assert (plan.B, plan.N, plan.E) == (len(sel), int(n[sel].sum()), int(e[sel].sum()))
    for got, want in ((plan.sel, sel), (plan.node_off, _ptr(n[sel])), (plan.edge_off, _ptr(e[sel]))):
        assert got.dtype == np.int64 and np.array_equal(got, want)
    # the one packed table: sel | node_off | edge_off, and ptr is a slice of it
    assert plan.table.dtype == torch.int64 and plan.table.shape == (3 * len(sel) + 2,)
    assert np.array_equal(plan.table.numpy(), np.concatenate([sel, _ptr(n[sel]), _ptr(e[sel])]))
    assert np.array_equal(plan.ptr.numpy(), _ptr(n[sel]))
    assert plan.ptr.data_ptr() == plan.table.data_ptr() + 8 * len(sel)
    # the same tables from the offsets alone
    for got, want in zip(resident.plan_tables(store.node_off, store.edge_off, ids), (plan.sel, plan.node_off, plan.edge_off)):
        assert np.array_equal(got, want)


def test_plan_refuses_bad_ids_before_any_upload(monkeypatch):
    prots, _ = _graphs()
    store = resident.ResidentGraphs(prots, "cpu")
    monkeypatch.setattr(torch, "from_numpy", lambda *a: pytest.fail("uploaded"))
    for bad in ([-1], [len(store)], [0, 5, 1], np.array([0, -1])):
        with pytest.raises(IndexError):
            store.plan(bad)
    for bad in ([0.0], np.array([1.0, 2.0]), [0, 1.5], torch.tensor([1.0]), [True]):
        with pytest.raises(TypeError):
            store.plan(bad)


def test_store_refuses_other_dtypes_and_a_cpu_store_does_not_collate():
    prots, drugs = _graphs()
    bf16 = dict(prots[1], x_s=torch.from_numpy(prots[1]["x_s"]).to(torch.bfloat16))
    with pytest.raises(NotImplementedError, match="bfloat16"):
        resident.ResidentGraphs([prots[0], bf16], "cpu")
    with pytest.raises(NotImplementedError, match="float64"):
        resident.ResidentGraphs([dict(drugs[0], e_s=drugs[0]["e_s"].astype(np.float64))], "cpu")
    with pytest.raises(NotImplementedError, match="int32"):
        resident.ResidentGraphs([dict(drugs[0], edge_index=drugs[0]["edge_index"].astype(np.int32))], "cpu")
    with pytest.raises(ValueError):
        resident.ResidentGraphs([prots[0], drugs[0]], "cpu")           # vector features for some graphs only
    store = resident.ResidentGraphs(drugs, "cpu")
    with pytest.raises(RuntimeError, match="MI355X"):
        store.collate(store.plan([0, 1]))                             # no CPU path


def _pairs(seed=5):
    prots, drugs = _graphs()
    P, M = resident.ResidentGraphs(prots, "cpu"), resident.ResidentGraphs(drugs, "cpu")
    index = np.array([(p, m) for p in range(len(prots)) for m in range(len(drugs))], dtype=np.int64)
    index = index[np.random.default_rng(seed).permutation(len(index))]
    y = torch.arange(len(index), dtype=torch.float32).reshape(-1, 1)
    return resident.ResidentPairs(P, M, index, y)


def _cost(rp, ids):
    ids = np.asarray(ids)
    return int(sum(rp.proteins.num_edges(p) + rp.molecules.num_edges(m) for p, m in rp.pair_index[ids]))


@pytest.mark.parametrize("max_bsize", [None, 3])
def test_batches_with_an_edge_budget(max_bsize):
    rp = _pairs()
    largest = max(_cost(rp, [i]) for i in range(len(rp)))
    for budget in (1, largest - 1, largest, 3 * largest):
        g = torch.Generator().manual_seed(11)
        epoch = list(rp.batches(max_num=budget, generator=g, max_bsize=max_bsize))
        assert sorted(i for b in epoch for i in b) == list(range(len(rp)))      # every pair once
        assert all(len(b) >= 1 for b in epoch)
        assert all(_cost(rp, b) <= budget or len(b) == 1 for b in epoch)
        if max_bsize is not None:
            assert all(len(b) <= max_bsize for b in epoch)
        # a batch is closed only by the budget or by max_bsize: the next pair would not have fitted
        for b, nxt in zip(epoch, epoch[1:]):
            assert _cost(rp, b) + _cost(rp, nxt[:1]) > budget or len(b) == max_bsize
        again = list(rp.batches(max_num=budget, generator=torch.Generator().manual_seed(11), max_bsize=max_bsize))
        assert again == epoch                                                   # the same seed, the same epoch
        other = list(rp.batches(max_num=budget, generator=torch.Generator().manual_seed(12), max_bsize=max_bsize))
        assert [i for b in other for i in b] != [i for b in epoch for i in b]
    in_order = list(rp.batches(max_num=3 * largest, shuffle=False))
    assert [i for b in in_order for i in b] == list(range(len(rp)))


def test_batches_of_a_fixed_size():
    rp = _pairs()
    epoch = list(rp.batches(batch_size=6, generator=torch.Generator().manual_seed(1)))
    assert [len(b) for b in epoch] == [6, 6, 6, 2] and sorted(i for b in epoch for i in b) == list(range(20))
    assert epoch == list(rp.batches(batch_size=6, generator=torch.Generator().manual_seed(1)))
    assert [len(b) for b in rp.batches(batch_size=6, max_bsize=4, shuffle=False)] == [4] * 5
    for bad in (dict(), dict(max_num=10, batch_size=2), dict(max_num=0), dict(batch_size=2, max_bsize=0)):
        with pytest.raises(ValueError):
            list(rp.batches(**bad))


def test_pairs_refuse_indices_outside_the_stores():
    rp = _pairs()
    y = torch.zeros(1, 1)
    for bad in ([[5, 0]], [[0, 4]], [[-1, 0]]):
        with pytest.raises(IndexError):
            resident.ResidentPairs(rp.proteins, rp.molecules, np.array(bad), y)
    with pytest.raises(TypeError):
        resident.ResidentPairs(rp.proteins, rp.molecules, np.array([[0.0, 1.0]]), y)
    with pytest.raises(ValueError):
        resident.ResidentPairs(rp.proteins, rp.molecules, np.array([[0, 1]]), torch.zeros(2, 1))


@pytest.mark.parametrize("pairs", [None, [(0, 1), (2, 0), (0, 0), (2, 1)], []])
def test_block_plans_the_pair_list_from_the_host_lengths(monkeypatch, pairs):
    rp = _pairs()
    pids, mids = [3, 0, 3], [1, 2]
    # the collate itself needs the GPU: here the two launches are replaced by the plans they were given
    monkeypatch.setattr(resident.ResidentGraphs, "collate", lambda self, plan, out=None, max_blocks=0: plan)
    pplan, mplan, plan = rp.block(pids, mids, pairs)
    assert np.array_equal(pplan.sel, pids) and np.array_equal(mplan.sel, mids)
    len1 = [rp.proteins.num_nodes(i) for i in pids]
    len2 = [rp.molecules.num_nodes(i) for i in mids]
    want = pt.plan_pair_training(len1, len2, pairs)
    assert isinstance(plan, pt.PairTrainPlan)
    for name in pt.PairTrainPlan._fields:
        assert np.array_equal(getattr(plan, name), getattr(want, name)), name
    with pytest.raises(IndexError):
        rp.block(pids, mids, [(3, 0)])
    with pytest.raises(IndexError):
        rp.block([5], mids)
