"""The CSR build, the source-order index and the collate kernel of csrc/graph_index_kernels.hip at the sizes their code branches
on: cgvp_csr_from_coo (count, one of two scans, fill, rank), cgvp_src_index (count, scan, fill, rank over sources) and
cgvp_csr_collate.  All of it is integer arithmetic: the references below are exact and every comparison is array_equal.

Which case is there for which branch (N = targets; E is about 2 N unless a case says otherwise):
  n0, n1            the smallest launches: N = 0 without edges, N = 1 with three copies of the self loop; rowptr[N] comes
                    from the zero padding of the counters
  1023, 1024, 1025  N + 1 crossing a 1024-entry chunk of csr_scan_multi_kernel: rowptr[N] is written by workgroup 0 or 1
  4097              five workgroups: every later one runs its `pre` loop and the wave reduction of `pre`
  65535             the last table of the multi-workgroup scan (SCAN_MULTI_MAX), 64 workgroups
  65536             the first table of csr_scan_kernel: one full tile of SCAN_LDS = 36,864 entries and one of 28,672
  73728             exactly two full tiles
  73729, 73731      a third tile of 1 and of 3 entries: no int4 at all, only the `n & 3` tail load and store
  110593            three full tiles + 1: the carry crosses more than one tile
  5000e10, 5000e1   fewer edges than counters: the rank launch is sized by the counters it has to zero
  hub               300 targets, 5000 edges all onto node 299, sources descending and repeated: one segment across 20 fill
                    workgroups, a rank over 5000 ids;  hub_swapped: the same with source and target exchanged, so that
                    ONE source owns all 5000 positions of the source index
  desc              2000 targets, edges listed by descending target: arrival order opposite to the result
Every graph gives node 0, the last node and the first and last node of every 1024-entry chunk and every 36,864-entry
tile at least one incoming edge, so no boundary is crossed with a trivial prefix.

Beside the tables every GPU test checks what the header promises around them: 64 canary words behind every table the
test hands in (and in front of a table it places 4 bytes past a 16-byte boundary), the counters all zero after each call,
a second call on the same counters without a fill in between, work_is_zero = 0 / 1 / 2, the -1 / 0 / 0 tail after dropped
edges, 64-bit endpoints tested before they are narrowed, and "work: any content" for the source index.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from gvp_hip import _lib, ops
from gvp_hip.ops import _ptr, _stream

DEV = "cuda:0"
BAD = -1                                  # CGVP_ERR_BAD_ARG
PAD = 64                                  # canary words behind every buffer
CANARY = -0x5A5A5A5B                      # no table entry, count or tail value ever equals it
DIRTY = 0x7FFFFFFF
SCAN_LDS, SCAN_CHUNK = 36 * 1024, 1024    # tile of csr_scan_kernel, chunk of csr_scan_multi_kernel
I32 = np.int32


def _round64(n):
    return (n + 63) // 64 * 64


# ------------------------------------------------------------------------------------------------------- exact references
def ref_csr(ei, N):
    """rowptr [N + 1], eperm [E], esrc [E], edst [E] as include/caster_gvp.h words them: the edges with both endpoints in
    [0, N) (tested on the int64 values), stable by target; positions rowptr[N] .. E hold -1 / 0 / 0."""
    ei = np.asarray(ei, np.int64).reshape(2, -1)
    src, dst = ei
    E = ei.shape[1]
    ids = np.nonzero((src >= 0) & (src < N) & (dst >= 0) & (dst < N))[0]
    ids = ids[np.argsort(dst[ids], kind="stable")]
    rowptr = np.zeros(N + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(dst[ids], minlength=N)[:N])
    eperm, esrc, edst = np.full(E, -1, np.int64), np.zeros(E, np.int64), np.zeros(E, np.int64)
    eperm[:ids.size], esrc[:ids.size], edst[:ids.size] = ids, src[ids], dst[ids]
    return rowptr.astype(I32), eperm.astype(I32), esrc.astype(I32), edst.astype(I32)


def ref_src_index(rowptr, esrc, N):
    """sptr [N + 1], spos [rowptr[N]]: the sorted positions of every source, in increasing position."""
    s = np.asarray(esrc[:int(rowptr[N])], np.int64)
    sptr = np.zeros(N + 1, np.int64)
    sptr[1:] = np.cumsum(np.bincount(s, minlength=N)[:N])
    return sptr.astype(I32), np.argsort(s, kind="stable").astype(I32)


def _loops_csr(ei, N):
    E = len(ei[0])
    rowptr, eperm, esrc, edst = [0], [], [], []
    for n in range(N):
        for e in range(E):
            if int(ei[1][e]) == n and 0 <= int(ei[0][e]) < N:
                eperm.append(e), esrc.append(int(ei[0][e])), edst.append(n)
        rowptr.append(len(eperm))
    tail = E - len(eperm)
    return rowptr, eperm + [-1] * tail, esrc + [0] * tail, edst + [0] * tail


def _loops_src_index(rowptr, esrc, N):
    sptr, spos = [0], []
    for s in range(N):
        for p in range(rowptr[N]):
            if esrc[p] == s:
                spos.append(p)
        sptr.append(len(spos))
    return sptr, spos


SMALL_GRAPHS = [
    # duplicates (1 -> 2 twice, 0 -> 0 twice), self loops, node 4 isolated, three dropped edges (7 -> 1, -1 -> 0, 2 -> 5)
    (5, [[1, 3, 7, 1, 0, -1, 2, 0, 2, 3], [2, 3, 1, 2, 0, 0, 5, 0, 1, 0]]),
    (1, [[0, 0, 0], [0, 0, 0]]),
    (3, [[], []]),
    (0, [[], []]),
    (4, [[0, 1, 2, 3, 3, 3], [3, 3, 2, 1, 0, 0]]),                                  # listed by descending target
    (2, [[2 ** 32 + 1, 0, -2 ** 63, 1, 2 ** 63 - 1], [0, 2 ** 32, 1, 1, 1]]),      # endpoints whose low words are valid ids
]


def _small_graphs():
    rng = np.random.default_rng(5)
    out = [(n, np.array(ei, np.int64).reshape(2, -1)) for n, ei in SMALL_GRAPHS]
    for n, e in ((12, 40), (7, 30), (12, 5)):
        out.append((n, rng.integers(-1, n + 1, (2, e))))             # -1 and n: dropped; the rest repeats and loops
    return out


def test_references_equal_a_double_loop_on_small_graphs():
    """The vectorised references against the definition written out as two nested loops, on graphs of at most 12 nodes with
    duplicate edges, self loops, an isolated node and dropped edges: the two share no NumPy call that could be misused
    the same way in both."""
    seen_drop = seen_dup = seen_loop = seen_isolated = False
    for N, ei in _small_graphs():
        rowptr, eperm, esrc, edst = ref_csr(ei, N)
        want = _loops_csr(ei.tolist(), N)
        for got, w in zip((rowptr, eperm, esrc, edst), want):
            assert got.dtype == I32 and got.tolist() == w, (N, ei)
        sptr, spos = ref_src_index(rowptr, esrc, N)
        w_sptr, w_spos = _loops_src_index(want[0], want[2], N)
        assert sptr.tolist() == w_sptr and spos.tolist() == w_spos, (N, ei)
        ev, E = int(rowptr[N]), ei.shape[1]
        seen_drop |= ev < E
        seen_dup |= len({(s, d) for s, d in zip(esrc[:ev].tolist(), edst[:ev].tolist())}) < ev
        seen_loop |= bool((esrc[:ev] == edst[:ev]).any())
        seen_isolated |= N > 0 and E > 0 and bool(((np.diff(rowptr) == 0) & (np.diff(sptr) == 0)).any())
    assert seen_drop and seen_dup and seen_loop and seen_isolated


# ------------------------------------------------------------------------------------------------------------ the graphs
def _boundary_nodes(N):
    """Node 0, the last node, and the last / first node on either side of every chunk and tile boundary below N."""
    nodes = [N - 1, 0]
    for step in (SCAN_CHUNK, SCAN_LDS):
        for b in range(step, N + 1, step):
            nodes += [b - 1] + ([b] if b < N else [])
    return list(dict.fromkeys(nodes))


def _random_graph(N, E, seed):
    rng = np.random.default_rng(seed)
    ei = rng.integers(0, N, (2, E))
    forced = _boundary_nodes(N)[:E]
    ei[1, rng.choice(E, len(forced), replace=False)] = forced
    return ei


SIZES = (1023, 1024, 1025, 4097, 65535, 65536, 73728, 73729, 73731, 110593)
CSR_CASES = ("n0", "n1") + tuple(str(n) for n in SIZES) + ("5000e10", "5000e1", "hub", "hub_swapped", "desc")
SRC_CASES = ("1024", "4097", "65535", "65536", "73729", "hub", "hub_swapped", "n17e0")
MODE_SIZES = (1500, 70001)
MISALIGNED_SIZES = (100, 70001)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(N, edge_index int64 [2, E]) of a named case; seeded, built once."""
    if name == "n0":
        return 0, np.zeros((2, 0), np.int64)
    if name == "n1":
        return 1, np.zeros((2, 3), np.int64)
    if name == "n17e0":
        return 17, np.zeros((2, 0), np.int64)
    if name in ("5000e10", "5000e1"):
        return 5000, _random_graph(5000, int(name[5:]), 77)
    if name in ("hub", "hub_swapped"):
        ei = np.stack([299 - np.arange(5000) // 17, np.full(5000, 299)]).astype(np.int64)   # sources 299 .. 5, 17 each
        return 300, np.ascontiguousarray(ei[::-1]) if name == "hub_swapped" else ei
    if name == "desc":
        ei = _random_graph(2000, 4000, 78)
        return 2000, np.ascontiguousarray(ei[:, np.argsort(-ei[1], kind="stable")])
    N = int(name)
    return N, _random_graph(N, 2 * N, N)


def _malformed_graph():
    """N = 1000, E = 4000, one edge in ten with an endpoint (source and target in turn) outside [0, N) as an int64.  The low
    32 bits of 2^32 + 7 (7) and of -2^63 (0) are valid node ids: a kernel that narrowed before testing would keep them."""
    N, E = 1000, 4000
    ei = _random_graph(N, E, 79)
    bad = [-1, N, 2 ** 31 + 5, 2 ** 32 + 7, 2 ** 63 - 1, -2 ** 63]
    for k, e in enumerate(range(3, E, 10)):
        ei[k % 2, e] = bad[(k // 2) % len(bad)]
    return N, ei


def test_every_boundary_node_of_every_case_has_incoming_edges():
    """The property the case table promises, checked on the CPU so that a change to the generator cannot quietly turn a
    boundary case into one with an empty prefix."""
    for name in CSR_CASES:
        N, ei = _case(name)
        if name.startswith("hub") or ei.shape[1] < len(_boundary_nodes(max(N, 1))):
            continue
        deg = np.bincount(ei[1], minlength=N)
        assert N == 0 or deg[_boundary_nodes(N)].min() >= 1, name
        assert ei.shape[1] == 0 or (0 <= ei.min() and ei.max() < N), name
    N, ei = _malformed_graph()
    rowptr = ref_csr(ei, N)[0]
    assert rowptr[N] == 4000 - 400 and set(ei[(ei < 0) | (ei >= N)].tolist()) == {-1, N, 2 ** 31 + 5, 2 ** 32 + 7,
                                                                                   2 ** 63 - 1, -2 ** 63}


# -------------------------------------------------------------------------------------------- host checks (CPU, no launch)
def test_csr_entry_points_refuse_bad_arguments_on_the_host():
    """Every refusal precedes the launch: no GPU is needed or touched and `p` is never dereferenced."""
    L = _lib.lib()
    p, big = 0x1000, 2 ** 31

    coo = lambda ei=p, N=8, E=8, rowptr=p, eperm=p, esrc=p, edst=p, work=p, mode=1, ids=p: \
        L.cgvp_csr_from_coo(ei, N, E, rowptr, eperm, esrc, edst, work, mode, ids, None)
    for kw in (dict(N=-1), dict(E=-1), dict(N=-1, E=0), dict(N=big), dict(E=big), dict(N=2 ** 40), dict(E=2 ** 40),
               dict(N=big, E=0), dict(rowptr=0), dict(work=0), dict(rowptr=0, E=0), dict(work=0, E=0),
               dict(work=p + 4), dict(work=p + 8), dict(work=p + 4, E=0),
               dict(ei=0), dict(eperm=0), dict(esrc=0), dict(edst=0), dict(ids=0)):
        for mode in (0, 1, 2):
            assert coo(mode=mode, **kw) == BAD, (kw, mode)

    src = lambda rowptr=p, esrc=p, N=8, E=8, sptr=p, spos=p, work=p: \
        L.cgvp_src_index(rowptr, esrc, N, E, sptr, spos, work, None)
    for kw in (dict(N=-1), dict(E=-1), dict(N=-1, E=0), dict(N=big), dict(E=big), dict(N=2 ** 40), dict(E=2 ** 40),
               dict(rowptr=0), dict(sptr=0), dict(work=0), dict(rowptr=0, E=0), dict(sptr=0, E=0), dict(work=0, E=0),
               dict(work=p + 4), dict(work=p + 8), dict(work=p + 4, E=0), dict(esrc=0), dict(spos=0)):
        assert src(**kw) == BAD, kw
    assert L.cgvp_src_index_work_ints(-1, 0) == BAD and L.cgvp_src_index_work_ints(0, -1) == BAD

    col = lambda st_rowptr=p, st_node_off=p, st_edge_off=p, sel=p, b_node_off=p, b_edge_off=p, B=1, rowptr=p, table=0: \
        L.cgvp_csr_collate(st_rowptr, p, p, p, st_node_off, st_edge_off, sel, b_node_off, b_edge_off, B, table, rowptr,
                           p, p, p, None)
    for kw in (dict(B=-1), dict(rowptr=0), dict(rowptr=0, B=0), dict(st_rowptr=0), dict(st_node_off=0),
               dict(st_edge_off=0), dict(sel=0), dict(b_node_off=0), dict(b_edge_off=0)):
        for table in (0, 1):
            assert col(table=table, **kw) == BAD, (kw, table)
    assert col(B=0) == 0 and col(B=0, table=1) == 0


def test_src_index_work_size_covers_counters_and_ids():
    """work = [counters: N + 1 rounded up to 64 | one id per edge], for every (N, E) this file runs."""
    L = _lib.lib()
    shapes = [(N, ei.shape[1]) for N, ei in map(_case, CSR_CASES + SRC_CASES)] + [(1000, 4000)]
    for N, E in shapes + [(0, 1), (63, 0), (64, 0), (2 ** 31 - 1, 2 ** 31 - 1)]:
        assert L.cgvp_src_index_work_ints(N, E) >= _round64(N + 1) + max(E, 1), (N, E)


def test_build_csr_zeroes_handed_counters_when_it_refuses_the_edge_index():
    """ops.build_csr(counted=...) is handed counters that a cgvp_lba_pass_begin launch has already counted into; when
    it raises before the build they must not stay half-used.  Without a GPU the refusal is the device check."""
    for ei in (torch.zeros(2, 5, dtype=torch.int64), torch.zeros(3, 5, dtype=torch.int64), torch.zeros(5, dtype=torch.int64)):
        counted = torch.full((64,), 3, dtype=torch.int32)
        with pytest.raises((RuntimeError, ValueError)):
            ops.build_csr(ei, 5, counted=counted)
        assert int(counted.abs().max()) == 0


# ------------------------------------------------------------------------------------------------------------ GPU plumbing
class _Buf:
    """`n` int32 words on the device with PAD canary words behind them (and `lead` in front: lead = 1 places the table
    4 bytes past a 16-byte boundary).  The pointer is computed, not taken from a view: an empty view has none."""

    def __init__(self, n, lead=0, fill=None):
        self.n, self.lead = int(n), lead
        self.whole = torch.full((lead + self.n + PAD,), CANARY, dtype=torch.int32, device=DEV)
        assert self.whole.data_ptr() % 16 == 0
        if fill is not None:
            self.view.fill_(fill)

    @property
    def view(self):
        return self.whole[self.lead:self.lead + self.n]

    @property
    def ptr(self):
        return C.c_void_p(self.whole.data_ptr() + 4 * self.lead)

    def numpy(self):
        return self.view.cpu().numpy()

    def intact(self):
        w = self.whole.cpu().numpy()
        return bool((w[:self.lead] == CANARY).all() and (w[self.lead + self.n:] == CANARY).all())


def _build(ei, N, mode=1, work=None, lead=0):
    """cgvp_csr_from_coo on buffers of the test's own: (rowptr, eperm, esrc, edst, ids), work."""
    E = ei.shape[1]
    d_ei = torch.from_numpy(np.ascontiguousarray(ei)).to(DEV)
    tabs = [_Buf(N + 1, lead)] + [_Buf(E) for _ in range(4)]
    if work is None:
        work = _Buf(_round64(N + 1), fill=0)
    rowptr, eperm, esrc, edst, ids = tabs
    rc = _lib.lib().cgvp_csr_from_coo(_ptr(d_ei), N, E, rowptr.ptr, eperm.ptr, esrc.ptr, edst.ptr, work.ptr, mode,
                                      ids.ptr, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    return tabs, work


def _assert_build(tabs, work, ref, what):
    for name, got, want in zip(("rowptr", "eperm", "esrc", "edst"), tabs, ref):
        assert np.array_equal(got.numpy(), want), (what, name)
    for name, b in zip(("rowptr", "eperm", "esrc", "edst", "ids", "work"), tabs + [work]):
        assert b.intact(), (what, name)
    assert not work.numpy().any(), what                     # every call leaves the counters it used zeroed again


@functools.lru_cache(maxsize=None)
def _ref(name):
    N, ei = _case(name)
    return ref_csr(ei, N)


# ------------------------------------------------------------------------------------------------------ cgvp_csr_from_coo
@pytest.mark.gpu
@pytest.mark.parametrize("name", CSR_CASES)
def test_csr_from_coo_at_its_scan_and_launch_edges(name):
    """All four tables equal the reference, twice on the same counters with no fill in between (work_is_zero = 1), with
    every canary intact and the counters zero after each call."""
    N, ei = _case(name)
    tabs, work = _build(ei, N)
    _assert_build(tabs, work, _ref(name), "first call")
    tabs, work = _build(ei, N, work=work)
    _assert_build(tabs, work, _ref(name), "second call")


@pytest.mark.gpu
@pytest.mark.parametrize("N", MODE_SIZES)
def test_work_is_zero_modes_give_the_same_tables(N):
    """0: counters full of 0x7fffffff, the call fills them; 1: zeros; 2: the per-target counts are there already, as a
    cgvp_lba_pass_begin launch leaves them for in-range edges (written by torch here), and the count launch is skipped."""
    ei = _random_graph(N, 2 * N, 3 * N)
    ref = ref_csr(ei, N)
    counters = _round64(N + 1)
    for mode in (0, 1, 2):
        work = _Buf(counters, fill=DIRTY if mode == 0 else 0)
        if mode == 2:
            work.view[:N] = torch.bincount(torch.from_numpy(ei[1]).to(DEV), minlength=N).int()
            assert int(work.view.sum()) == ei.shape[1]
        tabs, work = _build(ei, N, mode=mode, work=work)
        _assert_build(tabs, work, ref, f"work_is_zero = {mode}")


@pytest.mark.gpu
def test_malformed_endpoints_are_tested_as_int64_and_leave_the_documented_tail():
    """Dropped edges leave eperm = -1, esrc = edst = 0 behind rowptr[N]; the source index then indexes the rowptr[N] kept
    positions only and leaves spos[rowptr[N]:] alone."""
    N, ei = _malformed_graph()
    E = ei.shape[1]
    ref = ref_csr(ei, N)
    ev = int(ref[0][N])
    tabs, work = _build(ei, N)
    _assert_build(tabs, work, ref, "malformed")
    assert (tabs[1].numpy()[ev:] == -1).all() and not tabs[2].numpy()[ev:].any() and not tabs[3].numpy()[ev:].any()
    sptr, spos, swork = _src_index(tabs[0], tabs[2], N, E)
    want_sptr, want_spos = ref_src_index(ref[0], ref[2], N)
    assert np.array_equal(sptr.numpy(), want_sptr) and np.array_equal(spos.numpy()[:ev], want_spos)
    assert (spos.numpy()[ev:] == CANARY).all() and sptr.intact() and spos.intact() and swork.intact()


@pytest.mark.gpu
@pytest.mark.parametrize("N", MISALIGNED_SIZES)
def test_rowptr_four_bytes_past_a_16_byte_boundary(N):
    """N = 100: the multi-workgroup scan (scalar stores anyway); N = 70,001: the scalar store branch of csr_scan_kernel,
    which ops.build_csr's allocator-aligned rowptr never takes.  The word in front of the table is a canary too."""
    ei = _random_graph(N, 2 * N, 5 * N)
    ref = ref_csr(ei, N)
    tabs, work = _build(ei, N, lead=1)
    assert tabs[0].ptr.value % 16 == 4
    _assert_build(tabs, work, ref, "misaligned")
    aligned, work = _build(ei, N)
    _assert_build(aligned, work, ref, "aligned")


@pytest.mark.gpu
def test_build_csr_on_a_side_stream_equals_the_default_stream():
    N, ei = _case("4097")
    d_ei = torch.from_numpy(ei).to(DEV)
    want = ops.build_csr(d_ei, N)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        got = ops.build_csr(d_ei, N)
        again = ops.build_csr(d_ei, N)              # the side stream's own persistent counters, used a second time
    side.synchronize()
    for name, ref in zip(("rowptr", "eperm", "esrc", "edst"), _ref("4097")):
        for csr in (want, got, again):
            assert np.array_equal(getattr(csr, name).cpu().numpy(), ref), name


@pytest.mark.gpu
def test_build_csr_refuses_a_wrong_shape_and_zeroes_the_counters_it_was_handed():
    for shape in ((3, 5), (5,), (5, 2), (1, 2, 5)):
        counted = torch.full((64,), 3, dtype=torch.int32, device=DEV)
        with pytest.raises(ValueError, match="edge_index must be"):
            ops.build_csr(torch.zeros(shape, dtype=torch.int64, device=DEV), 5, counted=counted)
        assert int(counted.abs().max()) == 0, shape


# --------------------------------------------------------------------------------------------------------- cgvp_src_index
def _src_index(rowptr, esrc, N, E, work=None):
    """cgvp_src_index on the build's own rowptr / esrc buffers: sptr, spos, work.  `work` starts full of 0x7fffffff."""
    L = _lib.lib()
    if work is None:
        work = _Buf(L.cgvp_src_index_work_ints(N, E), fill=DIRTY)
    sptr, spos = _Buf(N + 1), _Buf(E)
    rc = L.cgvp_src_index(rowptr.ptr, esrc.ptr, N, E, sptr.ptr, spos.ptr, work.ptr, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    return sptr, spos, work


@pytest.mark.gpu
@pytest.mark.parametrize("name", SRC_CASES)
def test_src_index_lists_every_sources_positions_in_increasing_order(name):
    """sptr / spos equal the reference on a `work` of any content, twice; within every source the positions strictly
    increase (the summation order of the deterministic backward rests on exactly that); canaries behind sptr[N] and
    spos[E - 1] stay.  n17e0: sptr all zero and nothing else written."""
    N, ei = _case(name)
    E = ei.shape[1]
    rowptr, eperm, esrc, edst = _ref(name)
    tabs, _ = _build(ei, N)
    assert np.array_equal(tabs[0].numpy(), rowptr) and np.array_equal(tabs[2].numpy(), esrc)
    want_sptr, want_spos = ref_src_index(rowptr, esrc, N)
    work = None
    for call in ("first call", "second call"):
        sptr, spos, work = _src_index(tabs[0], tabs[2], N, E, work)
        got_sptr, got_spos = sptr.numpy(), spos.numpy()
        assert np.array_equal(got_sptr, want_sptr), call
        assert np.array_equal(got_spos, want_spos), call
        assert sptr.intact() and spos.intact() and work.intact(), call
        inner = np.ones(E, bool)
        inner[got_sptr[:-1][got_sptr[:-1] < E]] = False          # first position of every source
        assert (np.diff(got_spos.astype(np.int64), prepend=-1)[inner] > 0).all(), call
        assert np.array_equal(esrc[got_spos], np.repeat(np.arange(N), np.diff(got_sptr))), call
    if name == "n17e0":
        assert not want_sptr.any() and E == 0
    if name == "hub_swapped":
        assert want_sptr[299] == 0 and want_sptr[300] == 5000


# ------------------------------------------------------------------------------------------------------- cgvp_csr_collate
BATCHES = ([3], [0, 0, 0], [2, 0, 3, 0, 2, 4, 5, 1], [2, 0, 3, 0, 2, 4, 5, 1, 0])


@functools.lru_cache(maxsize=None)
def _stores():
    """Six graphs: no edge; one edge; a 37-node radius graph; 300 nodes / 900 edges (both 256-strided loops of
    csr_collate_kernel take a second trip); a star onto node 0; self loops only.  -> graphs, plain store, table store."""
    rng = np.random.default_rng(11)
    xyz = rng.normal(size=(37, 3)) * 3.0
    radius = np.stack(np.nonzero(np.linalg.norm(xyz[:, None] - xyz[None], axis=-1) <= 4.0))
    eis = [np.zeros((2, 0), np.int64), np.array([[0], [1]]), radius, rng.integers(0, 300, (2, 900)),
           np.stack([rng.integers(0, 20, 45), np.zeros(45, np.int64)]), np.stack([np.arange(5)[::-1]] * 2)]
    sizes = [1, 2, 37, 300, 20, 5]
    graphs = []
    for ei, n in zip(eis, sizes):
        e = ei.shape[1]
        graphs.append(dict(n=n, ei=np.ascontiguousarray(ei, np.int64), e_s=rng.normal(size=(e, 32)).astype(np.float32),
                           e_v=rng.normal(size=(e, 1, 3)).astype(np.float32), etypes=rng.integers(0, 7, e)))
    assert 100 < radius.shape[1] < 37 * 37
    T = lambda a: torch.from_numpy(a).to(DEV)
    # CsrStore gathers the feature rows with each graph's eperm ON THE DEVICE: a wrong build must fail here, as an
    # assertion, and not reach torch's index_select as an index out of range (which traps the GPU)
    for g in graphs:
        csr, want = ops.build_csr(T(g["ei"]), g["n"]), ref_csr(g["ei"], g["n"])
        for name, w in zip(("rowptr", "eperm", "esrc", "edst"), want):
            assert np.array_equal(getattr(csr, name)[:w.size].cpu().numpy(), w), ("store graph", g["n"], name)
    plain =ops.CsrStore([T(g["ei"]) for g in graphs], sizes)
    table = ops.CsrStore([T(g["ei"]) for g in graphs], sizes, edge_attr=[(T(g["e_s"]), T(g["e_v"])) for g in graphs],
                         edge_types=[T(g["etypes"]) for g in graphs])
    return graphs, plain, table


def _collate(store, plan, table):
    """cgvp_csr_collate with output tables of the test's own (canaries behind each)."""
    outs = [_Buf(plan["N"] + 1)] + [_Buf(plan["E"]) for _ in range(3)]
    rc = _lib.lib().cgvp_csr_collate(_ptr(store.rowptr), _ptr(store.eperm), _ptr(store.esrc), _ptr(store.edst),
                                     _ptr(store.node_off), _ptr(store.edge_off), _ptr(plan["sel"]), _ptr(plan["node_off"]),
                                     _ptr(plan["edge_off"]), plan["B"], 1 if table else 0, *[o.ptr for o in outs], _stream())
    torch.cuda.synchronize()
    assert rc == 0
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("batch", BATCHES, ids=lambda b: "-".join(map(str, b)))
def test_csr_collate_batches_with_repeats_and_edgeless_graphs(batch):
    """[3]: B = 1.  [0, 0, 0]: no edge in the whole batch, eperm[0] must not be written.  The long batch repeats graphs
    and has edgeless ones in the middle; with graph 0 appended, rowptr[N] comes from a slot with n = 1, e = 0.
    Plain mode equals the build on the concatenated, offset edge_index; in table mode eperm[p] is a row of the store's
    resident tables, which must hold, bit for bit, the features of the batch edge the reference puts at p."""
    graphs, plain, table = _stores()
    off = np.concatenate([[0], np.cumsum([graphs[g]["n"] for g in batch])])
    batch_ei = np.concatenate([graphs[g]["ei"] + off[b] for b, g in enumerate(batch)], axis=1)
    N, E = int(off[-1]), batch_ei.shape[1]
    ref = ref_csr(batch_ei, N)
    built = ops.build_csr(torch.from_numpy(batch_ei).to(DEV), N)
    for store, mode in ((plain, False), (table, False), (table, True)):
        plan = store.plan(batch)
        assert (plan["N"], plan["E"], plan["B"]) == (N, E, len(batch))
        outs = _collate(store, plan, mode)
        wrapped = store.collate(plan, table=mode)
        assert wrapped.table_rows == (sum(g["ei"].shape[1] for g in graphs) if mode else None)
        assert not mode or wrapped.table_rows == store.e_s.shape[0] == store.e_v.shape[0] == store.etypes.shape[0]
        for k, name in enumerate(("rowptr", "eperm", "esrc", "edst")):
            n = N + 1 if name == "rowptr" else E
            got = outs[k].numpy()
            assert outs[k].intact(), (mode, name)                      # with E = 0 that includes "eperm[0]"
            assert np.array_equal(getattr(wrapped, name)[:n].cpu().numpy(), got), (mode, name)
            if mode and name == "eperm":
                continue
            assert np.array_equal(got, ref[k]), (mode, name)
            assert np.array_equal(got, getattr(built, name)[:n].cpu().numpy()), (mode, name)
        if mode:
            rows = torch.from_numpy(outs[1].numpy().astype(np.int64))
            assert E == 0 or (0 <= int(rows.min()) and int(rows.max()) < store.e_s.shape[0])
            for key, tab in (("e_s", store.e_s), ("e_v", store.e_v), ("etypes", store.etypes)):
                want = np.concatenate([graphs[g][key] for g in batch])[ref[1]]
                got = tab.cpu()[rows].numpy()
                assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), key
