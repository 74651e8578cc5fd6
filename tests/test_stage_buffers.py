"""cgvp_stage_buffers (stage_kernel in csrc/pass_api.hip) on its own: the one launch that copies a batch into the padded
static buffers of a captured step.  Through GraphedTrainStep every pointer is a fresh allocation and every size a bucket
multiple, so only the aligned body of the 16-byte path ever runs there.  Here every path runs against a NumPy
restatement on uint32 words -- the first `copy` words of the source, `fill_word` up to the capacity -- and equality is
exact:

  * the 16-byte vector path with the copy boundary inside a vector (in the vector body and in the word tail), capacities
    with every remainder modulo 4;
  * the scalar path taken when either pointer is not 16-byte aligned (destination, source, both);
  * the grid-stride loop: one item larger than 2048 workgroups x 256 threads x 16 bytes beside tiny ones;
  * full (24 items), single-item and empty tables, an item of capacity 0;
  * the fill words 0, 0xFFFFFFFF (read back as int64 -1, what edge_index is padded with) and an asymmetric pattern;
  * what the host refuses (CGVP_ERR_BAD_ARG) without touching the destination.

Every destination sits inside a larger device buffer between two 64-byte sentinel zones, and the WHOLE buffer is
compared, so a word written before or behind any item fails the test.  Every address handed to the library is taken
from a device tensor the test allocated (`_addr` refuses anything else)."""
import ctypes as C

import numpy as np
import pytest
import torch

from gvp_hip import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAD_ARG = -1                      # CGVP_ERR_BAD_ARG
SENTINEL = 0xA5A5A5A5
GUARD = 16                        # words: 64 bytes on either side of every destination
FILLS = (0, 0xFFFFFFFF, 0x80C0FFEE)
# (copy words, capacity words): capacity = copy, copy + 1, copy + 5 for every copy size, then the two partial-vector cases:
# (5, 8) the copy ends inside a vector of the vector body, (5, 7) inside the word tail.  Capacities cover every words % 4.
SIZES = [(c, c + extra) for c in (0, 1, 2, 3, 4, 5, 7, 8, 1023) for extra in (0, 1, 5)] + [(5, 8), (5, 7)]
assert {cap % 4 for _, cap in SIZES} == {0, 1, 2, 3}


def _addr(t, word=0, byte=0):
    """Address of word `word` (+ `byte`) of a device tensor of the test's own: nothing else ever reaches the library."""
    assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and 0 <= word <= t.numel() and 0 <= byte < 4
    assert t.data_ptr() % 16 == 0
    return t.data_ptr() + 4 * word + byte


def _up4(n):
    return (n + 3) // 4 * 4


def _device_words(a):
    return torch.from_numpy(a.view(np.int32)).to(DEV)


def _host_words(t):
    return t.cpu().numpy().view(np.uint32)


def _call(items, n):
    rc = _lib.lib().cgvp_stage_buffers(items, n, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


class _Layout:
    """Destinations and sources of a table of (copy words, capacity words, fill word) items in two device buffers.
    Every region starts at a 16-byte boundary + `dst_off` / `src_off` bytes (multiples of 4); `null_empty_src` gives an
    item that copies nothing a NULL source."""

    def __init__(self, specs, dst_off=0, src_off=0, seed=0, null_empty_src=True):
        assert dst_off % 4 == 0 and src_off % 4 == 0 and len(specs) <= _lib.MAX_STAGE
        rng = np.random.default_rng(seed)
        self.n = len(specs)
        self.items = (_lib.StageItem * _lib.MAX_STAGE)()
        d_at, s_at, place = 0, 0, []
        for copy, cap, fill in specs:
            place.append((d_at + GUARD + dst_off // 4, s_at + src_off // 4))
            d_at += _up4(GUARD + dst_off // 4 + cap + GUARD)
            s_at += _up4(src_off // 4 + copy + 4)
        src = rng.integers(0, 2 ** 32, size=max(s_at, 4), dtype=np.uint64).astype(np.uint32)
        self.expected = np.full(max(d_at, 4), SENTINEL, dtype=np.uint32)
        self.dst = _device_words(self.expected)
        self.src = _device_words(src)
        for k, ((copy, cap, fill), (d0, s0)) in enumerate(zip(specs, place)):
            self.expected[d0:d0 + copy] = src[s0:s0 + copy]
            self.expected[d0 + copy:d0 + cap] = fill
            s_ptr = 0 if (copy == 0 and null_empty_src) else _addr(self.src, s0)
            self.items[k] = _lib.StageItem(_addr(self.dst, d0), s_ptr, 4 * copy, 4 * cap, fill)

    def run_and_check(self):
        assert _call(self.items, self.n) == 0
        got = _host_words(self.dst)
        bad = np.flatnonzero(got != self.expected)
        assert bad.size == 0, f"{bad.size} words differ, first at word {bad[0]}: {got[bad[0]]:#x} != {self.expected[bad[0]]:#x}"


# destination / source offsets in bytes: (0, 0) is the 16-byte vector path, every other one the scalar path
@pytest.mark.parametrize("dst_off,src_off", [(0, 0), (4, 0), (0, 4), (0, 8), (0, 12), (4, 4), (4, 12)])
def test_copy_and_fill_at_every_boundary(dst_off, src_off):
    for fill in FILLS:
        specs = [(copy, cap, fill) for copy, cap in SIZES]
        for at in range(0, len(specs), _lib.MAX_STAGE):
            _Layout(specs[at:at + _lib.MAX_STAGE], dst_off, src_off, seed=at + dst_off + 16 * src_off).run_and_check()


@pytest.mark.parametrize("dst_off", [0, 4])
def test_grid_stride_second_trip_beside_tiny_items(dst_off):
    """One item of 2048 * 256 * 16 + 3 * 256 * 16 + 12 bytes: the launch is capped at 2048 workgroups, so the words behind
    the first 2048 * 256 vectors are written in a second trip of the loop -- the copy ends there, in the middle of a
    vector -- and the word tail (3 words) is reached by the workgroups' first threads only.  The tiny items beside it get
    the same 2048 workgroups, nearly all of which have nothing to do."""
    cap = (2048 * 256 * 16 + 3 * 256 * 16 + 12) // 4
    copy = 2048 * 256 * 4 + 256 * 4 + 2
    assert copy % 4 == 2 and copy < cap and cap % 4 == 3
    _Layout([(1, 1, 0), (copy, cap, 0x80C0FFEE), (5, 7, 0xFFFFFFFF), (0, 0, 0), (3, 1023, 0)], dst_off, 0, seed=5).run_and_check()


def test_full_single_and_empty_tables():
    rng = np.random.default_rng(9)
    caps = [int(c) for c in rng.permutation(np.arange(1, 400))[:_lib.MAX_STAGE]]           # 24 different sizes in one launch
    full = [(int(rng.integers(0, cap + 1)), cap, FILLS[k % 3]) for k, cap in enumerate(caps)]
    assert len({cap for _, cap, _ in full}) == _lib.MAX_STAGE == 24
    _Layout(full, seed=1).run_and_check()
    _Layout([(6, 9, 0x80C0FFEE)], seed=2).run_and_check()
    # an item of capacity 0: with a destination inside the buffer (nothing may be written there) and with a NULL one
    _Layout([(0, 0, 0xFFFFFFFF), (2, 3, 0)], seed=3).run_and_check()
    lay = _Layout([(0, 0, 0xFFFFFFFF)], seed=4)
    lay.run_and_check()
    lay.items[0] = _lib.StageItem(0, 0, 0, 0, 7)
    lay.run_and_check()
    # an empty table is no launch and no error, whatever the pointer
    assert _call(lay.items, 0) == 0 and _call(None, 0) == 0
    assert np.array_equal(_host_words(lay.dst), lay.expected)


def test_all_ones_fill_reads_as_minus_one_through_int64():
    """edge_index rows are int64 and padded with -1: two 0xFFFFFFFF words each."""
    E, Ecap = 5, 8
    src = torch.arange(100, 100 + E, dtype=torch.int64, device=DEV)
    buf = _device_words(np.full(2 * GUARD + 2 * Ecap, SENTINEL, dtype=np.uint32))
    items = (_lib.StageItem * _lib.MAX_STAGE)()
    items[0] = _lib.StageItem(_addr(buf, GUARD), src.data_ptr(), 8 * E, 8 * Ecap, 0xFFFFFFFF)
    assert _call(items, 1) == 0
    row = buf[GUARD:GUARD + 2 * Ecap].view(torch.int64).cpu()
    assert row.tolist() == list(range(100, 100 + E)) + [-1] * (Ecap - E)
    guards = _host_words(buf)
    assert (guards[:GUARD] == SENTINEL).all() and (guards[GUARD + 2 * Ecap:] == SENTINEL).all()


def test_host_refuses_bad_tables_without_a_launch():
    """Each table is refused with CGVP_ERR_BAD_ARG before anything is launched: the destination keeps its sentinel.  The
    defects are in sizes and alignment; every non-NULL address still lies inside the test's own device buffers."""
    dst = _device_words(np.full(4 * GUARD, SENTINEL, dtype=np.uint32))
    src = _device_words(np.arange(4 * GUARD, dtype=np.uint32))
    d, s = _addr(dst, GUARD), _addr(src, GUARD)
    good = (d, s, 16, 32, 0)
    bad_items = {
        "copy larger than capacity": (d, s, 36, 32, 0),
        "negative copy": (d, s, -4, 32, 0),
        "negative capacity": (d, 0, 0, -4, 0),
        "copy not a multiple of 4": (d, s, 6, 32, 0),
        "capacity not a multiple of 4": (d, s, 16, 30, 0),
        "destination off by 2 bytes": (_addr(dst, GUARD, byte=2), s, 16, 32, 0),
        "source off by 2 bytes": (d, _addr(src, GUARD, byte=2), 16, 32, 0),
        "NULL source with a copy size": (d, 0, 16, 32, 0),
        "NULL destination with a capacity": (0, 0, 0, 32, 0),
    }
    big = (_lib.StageItem * (_lib.MAX_STAGE + 1))(*[_lib.StageItem(*good) for _ in range(_lib.MAX_STAGE + 1)])
    one = (_lib.StageItem * _lib.MAX_STAGE)()
    one[0] = _lib.StageItem(*good)
    assert _call(one, -1) == BAD_ARG, "n < 0"
    assert _call(C.cast(big, C.POINTER(_lib.StageItem)), _lib.MAX_STAGE + 1) == BAD_ARG, "n > CGVP_MAX_STAGE"
    assert _call(None, 1) == BAD_ARG, "items NULL with n > 0"
    for what, fields in bad_items.items():
        for slot in (0, 1):                       # the defect is found behind a good item as well
            items = (_lib.StageItem * _lib.MAX_STAGE)()
            items[0] = _lib.StageItem(*good)
            items[slot] = _lib.StageItem(*fields)
            assert _call(items, slot + 1) == BAD_ARG, what
    assert (_host_words(dst) == SENTINEL).all()
    assert _call(one, 1) == 0                     # (the good item alone is accepted: the refusals above were about the defects)
    want = np.full(4 * GUARD, SENTINEL, dtype=np.uint32)
    want[GUARD:GUARD + 4] = np.arange(GUARD, GUARD + 4)
    want[GUARD + 4:GUARD + 8] = 0
    assert np.array_equal(_host_words(dst), want)
