"""Device-side evaluation metrics (csrc/metrics_kernels.hip, include/caster_gvp_metrics.h, gvp_hip.metrics) and the
meter's place inside the captured training step (gvp_hip.graphed.GraphedTrainStep(meter=...)).

REFERENCE.  `restate` below restates include/caster_gvp_metrics.h in NumPy: the three pair counts as integer sums over
the lower-triangle index pairs (np.tril_indices, float32 comparisons), the concordance index as ONE float64 division
of exact operands, the moments in float64.  On the CPU it is pinned to tests/golden/eval_metrics.npz, which holds what
the reference's own calc_concordance_index and its own MSE / MAE / Pearson expressions (train_model.py:759-793) return
on seeded inputs (tests/golden/make_eval_metrics_golden.py): counts and index exactly, the moments to the float32
rounding of the reference.  It then serves the GPU tests.

BOUNDS.  Counts, n and the index (bitwise, as a float64) are exact on both sides: integer sums, and one correctly
rounded division of operands below 2^52.  MSE / MAE / Pearson of the kernels against `restate`: 1e-12 (relative;
absolute for Pearson) -- both are float64 sums of at most ~2k terms (n * 2^-53 = 2.3e-13), in another order.
`restate` against the float32 reference: 1e-6 (relative; absolute for Pearson) -- pairwise float32 summation of
n <= 1024 terms rounds to about (log2 n + 3) * 2^-24 = 8e-7.

Inputs of the kernel-level tests are 4-byte-misaligned views into canary-filled buffers; state, outputs and workspace
are surrounded by canaries; the canaries are compared bitwise after every call.
"""
import ctypes as C
import json
import os
import re
import struct

import numpy as np
import pytest
import torch

import davis_synth as ds
from conftest import GOLDEN, REPO, load_npz
from gvp_hip import _lib, metrics

DEV = "cuda:0"
T, CH = metrics.TILE, metrics.CHUNK                      # CGVP_METRICS_TILE, CGVP_METRICS_CHUNK (never hard-coded below)
SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 513, 700)
GOLDEN_CASES = [f"{kind}{n}" for n in SIZES for kind in ("cont", "davis", "nan")] + ["tied2", "constpred"]
EDGE_SIZES = sorted({T - 1, T, T + 1, 2 * T + 1, CH - 1, CH, CH + 1, 2 * CH + 1})
CANARY = float(np.float32(-7.25e11))
CANARY64 = 0x5A5AA5A55A5AA5A5
NAN = float("nan")


# ---------------------------------------------------------------------------------------------------------------------
# NumPy restatement of include/caster_gvp_metrics.h
def restate(pred, target):
    p = np.ascontiguousarray(pred, dtype=np.float32).reshape(-1)
    t = np.ascontiguousarray(target, dtype=np.float32).reshape(-1)
    n = int(p.size)
    assert t.size == n
    i, j = np.tril_indices(n, -1)                         # every pair i > j once
    with np.errstate(invalid="ignore"):
        above, below = t[i] > t[j], t[i] < t[j]
        comparable = above | below
        concordant = (above & (p[i] > p[j])) | (below & (p[i] < p[j]))
        tied = comparable & (p[i] == p[j])
    concordant, tied, comparable = int(concordant.sum()), int(tied.sum()), int(comparable.sum())
    ci = float(np.float64(concordant + 0.5 * tied) / np.float64(comparable)) if comparable else 0.0
    mse = mae = pearson = NAN
    if n:
        p64, t64 = p.astype(np.float64), t.astype(np.float64)
        with np.errstate(all="ignore"):
            d = p64 - t64
            mse, mae = float((d * d).sum() / n), float(np.abs(d).sum() / n)
            pc, tc = p64 - p64.sum() / n, t64 - t64.sum() / n
            sxx, syy = float((pc * pc).sum()), float((tc * tc).sum())
            pearson = NAN if sxx == 0.0 or syy == 0.0 else float((pc * tc).sum() / np.sqrt(sxx * syy))
    return {"n": n, "mse": mse, "rmse": float(np.sqrt(mse)), "mae": mae, "pearson": pearson, "ci": ci,
            "concordant": concordant, "tied_pred": tied, "comparable": comparable}


def restate_binned(pred, target):
    """`restate` for inputs of few distinct values, in O(n + bins^2): rows are binned by their (target, prediction)
    values, and two bins a != b hold m_a * m_b pairs that all compare alike (the definitions are symmetric in i and j,
    so every unordered pair is taken once; rows of one bin have equal targets and are not comparable).  A NaN target
    leaves its row out, NaN predictions form bins that compare false.  Pinned to `restate` on the CPU."""
    p = np.ascontiguousarray(pred, dtype=np.float32).reshape(-1)
    t = np.ascontiguousarray(target, dtype=np.float32).reshape(-1)
    keep = ~np.isnan(t)
    rows = np.stack([t[keep], np.nan_to_num(p[keep], nan=-1e30), np.isnan(p[keep]).astype(np.float32)], axis=1)
    keys, m = np.unique(rows, axis=0, return_counts=True)
    tb, pb = keys[:, 0], np.where(keys[:, 2] > 0, np.float32(np.nan), keys[:, 1]).astype(np.float32)
    w = np.triu(m[:, None].astype(object) * m[None, :].astype(object), 1)           # exact integers, every bin pair once
    with np.errstate(invalid="ignore"):
        above, below = tb[:, None] > tb[None, :], tb[:, None] < tb[None, :]
        comparable = above | below
        concordant = (above & (pb[:, None] > pb[None, :])) | (below & (pb[:, None] < pb[None, :]))
        tied = comparable & (pb[:, None] == pb[None, :])
    concordant, tied, comparable = (int(w[mask].sum()) for mask in (concordant, tied, comparable))
    out = restate(p[:0], t[:0])
    n = int(p.size)
    p64, t64 = p.astype(np.float64), t.astype(np.float64)
    with np.errstate(all="ignore"):
        d = p64 - t64
        pc, tc = p64 - p64.sum() / n, t64 - t64.sum() / n
        sxx, syy = float((pc * pc).sum()), float((tc * tc).sum())
        out.update(n=n, mse=float((d * d).sum() / n), mae=float(np.abs(d).sum() / n),
                   pearson=NAN if sxx == 0.0 or syy == 0.0 else float((pc * tc).sum() / np.sqrt(sxx * syy)))
    out.update(rmse=float(np.sqrt(out["mse"])), concordant=concordant, tied_pred=tied, comparable=comparable,
               ci=float(np.float64(concordant + 0.5 * tied) / np.float64(comparable)) if comparable else 0.0)
    return out


def bits(x):
    return struct.pack("<d", float(x))


def close(got, want, tol, relative=True):
    if np.isnan(want) or np.isnan(got):
        return bool(np.isnan(want) and np.isnan(got))
    return abs(got - want) <= tol * (abs(want) if relative else 1.0)


def assert_equal_to_restatement(got, want, what=""):
    for key in ("n", "concordant", "tied_pred", "comparable"):
        assert got[key] == want[key], (what, key, got[key], want[key])
    assert bits(got["ci"]) == bits(want["ci"]), (what, got["ci"], want["ci"])
    for key in ("mse", "rmse", "mae"):
        assert close(got[key], want[key], 1e-12), (what, key, got[key], want[key])
    assert close(got["pearson"], want["pearson"], 1e-12, relative=False), (what, got["pearson"], want["pearson"])


_golden = {}


def golden():
    if not _golden:
        _golden.update(load_npz("eval_metrics.npz"))
    return _golden


def davis_like(n, seed, nan_share=0.0):
    """Targets from eight values (5.0 three times as likely), predictions rounded to 0.25: ties on both sides."""
    rng = np.random.default_rng(seed)
    values = np.array([5.0, 5.5, 6.0, 6.5, 7.0, 7.5, 8.0, 9.0], dtype=np.float32)
    w = np.array([3.0] + [1.0] * 7)
    t = rng.choice(values, size=n, p=w / w.sum()).astype(np.float32)
    p = (np.round((t + rng.normal(0.0, 0.7, n)) * 4.0) / 4.0).astype(np.float32)
    if nan_share:
        p[rng.random(n) < nan_share] = np.nan
        t[rng.random(n) < nan_share] = np.nan
    return p, t


_cases = {}


def case(name):
    """(pred, target, restatement) of a golden case or of `edge<n>` / `empty`; computed once, never written to."""
    if name not in _cases:
        if name == "empty":
            p = t = np.zeros(0, dtype=np.float32)
        elif name.startswith("edge"):
            n = int(name[4:])
            p, t = davis_like(n, seed=n, nan_share=0.02 if n % 2 else 0.0)
        else:
            p, t = golden()[f"{name}_pred"], golden()[f"{name}_target"]
        p.setflags(write=False), t.setflags(write=False)
        _cases[name] = (p, t, restate(p, t))
    return _cases[name]


# ---------------------------------------------------------------------------------------------------------------------
# CPU
def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(cgvp_[a-z0-9_]+)\s*\(", text))


def test_metrics_entry_points_have_a_header_and_a_version_of_their_own():
    header = os.path.join(REPO, "include", "caster_gvp_metrics.h")
    assert _declared(header) == set(metrics.exported_symbols())
    handle = C.CDLL(_lib.LIB_PATH)
    main = open(os.path.join(REPO, "include", "caster_gvp.h")).read()
    assert "metrics" not in main
    for name in metrics.exported_symbols():
        assert hasattr(handle, name), name
        assert name not in main and name not in _lib.exported_symbols(), name
    text = open(header).read()
    assert metrics.lib().cgvp_metrics_version() == 1 == metrics.METRICS_VERSION and "#define CGVP_METRICS_VERSION 1\n" in text
    assert f"#define CGVP_METRICS_TILE {T}\n" in text and f"#define CGVP_METRICS_CHUNK {CH}\n" in text
    assert f"#define CGVP_METRICS_MAX_ROWS {metrics.MAX_ROWS}\n" in text and metrics.MAX_ROWS == 2 ** 26
    assert _lib.ABI_VERSION == 31 and _lib.lib().cgvp_abi_version() == 31
    assert _lib.abi_header_digest() == _lib.ABI_HEADER_SHA256


def test_entry_points_refuse_bad_arguments_on_the_host():
    """Every refusal is CGVP_ERR_BAD_ARG before any launch: no GPU is needed (or touched)."""
    L = metrics.lib()
    BAD, null, p, odd4, odd8 = -1, 0, 0x10000, 0x10002, 0x10004     # never dereferenced: the checks run on the host
    LIMIT = metrics.MAX_ROWS
    need = L.cgvp_metrics_workspace_bytes(100)

    def append(pred=p, target=p, n=5, pred_buf=p, target_buf=p, capacity=10, state=p):
        return L.cgvp_metrics_append(pred, target, n, pred_buf, target_buf, capacity, state, 0, null)

    for name in ("pred", "target", "pred_buf", "target_buf", "state"):
        assert append(**{name: null}) == BAD, (name, "null")
        assert append(**{name: odd4}) == BAD, (name, "misaligned")
    assert append(state=odd8) == BAD                                  # the state is int64: 8-byte alignment
    assert append(n=-1) == BAD and append(capacity=-1) == BAD and append(capacity=LIMIT + 1) == BAD
    assert append(n=0) == 0 and append(n=0, pred=null, target=null) == 0     # a no-op that launches nothing
    assert append(n=0, state=null) == BAD

    assert L.cgvp_metrics_reset(null, null) == BAD and L.cgvp_metrics_reset(odd8, null) == BAD

    def compute(pred_buf=p, target_buf=p, count=null, max_rows=100, counts=p, vals=p, ws=p, ws_bytes=need):
        return L.cgvp_metrics_compute(pred_buf, target_buf, count, max_rows, counts, vals, ws, ws_bytes, null)

    for name in ("pred_buf", "target_buf", "counts", "vals", "ws"):
        assert compute(**{name: null}) == BAD, (name, "null")
        assert compute(**{name: odd4}) == BAD, (name, "misaligned")
    for name in ("count", "counts", "vals", "ws"):
        assert compute(**{name: odd8}) == BAD, (name, "4-byte aligned only")
    assert compute(max_rows=-1) == BAD and compute(max_rows=LIMIT + 1, ws_bytes=1 << 40) == BAD
    assert compute(ws_bytes=need - 8) == BAD and compute(ws_bytes=0) == BAD and compute(ws_bytes=-8) == BAD
    # the size function
    sizes = [L.cgvp_metrics_workspace_bytes(n) for n in (0, 1, T, T + 1, CH + 1, 100000, LIMIT)]
    assert all(s > 0 and s % 8 == 0 for s in sizes) and sizes == sorted(sizes) and sizes[-1] < 1 << 30
    assert L.cgvp_metrics_workspace_bytes(-1) == BAD and L.cgvp_metrics_workspace_bytes(LIMIT + 1) == BAD
    with pytest.raises(ValueError):
        metrics.workspace_bytes(LIMIT + 1)


def test_module_refuses_cpu_tensors_and_unequal_sizes():
    x = torch.zeros(4)
    with pytest.raises(RuntimeError, match="MI355X only"):
        metrics.regression_metrics(x, x)
    with pytest.raises(RuntimeError, match="MI355X only"):
        metrics.concordance_index(x, x)
    with pytest.raises(RuntimeError, match="MI355X only"):
        metrics.RegressionMeter(16, "cpu")
    with pytest.raises(ValueError, match="capacity"):
        metrics.RegressionMeter(metrics.MAX_ROWS + 1, "cuda:0")


def test_restatement_equals_the_reference_on_the_golden_fixture():
    """Counts and index exactly (the index bitwise), MSE / MAE within 1e-6 relative and Pearson within 1e-6 absolute of
    the reference's float32 results; NaN where the reference has NaN."""
    g = golden()
    assert sorted(k[:-5] for k in g if k.endswith("_pred")) == sorted(GOLDEN_CASES)
    worst = {"mse": 0.0, "mae": 0.0, "pearson": 0.0}
    for name in GOLDEN_CASES:
        p, t, mine = case(name)
        assert p.dtype == t.dtype == np.float32
        assert [mine["concordant"], mine["tied_pred"], mine["comparable"]] == g[f"{name}_counts"].tolist(), name
        assert bits(mine["ci"]) == bits(g[f"{name}_ci"]), (name, mine["ci"], float(g[f"{name}_ci"]))
        if name.startswith("nan"):
            assert f"{name}_moments" not in g and (np.isnan(p).any() or np.isnan(t).any() or p.size < 8)
            continue
        mse, mae, pearson = (float(x) for x in g[f"{name}_moments"])
        assert close(mine["mse"], mse, 1e-6) and close(mine["mae"], mae, 1e-6), (name, mine, mse, mae)
        assert close(mine["pearson"], pearson, 1e-6, relative=False), (name, mine["pearson"], pearson)
        worst["mse"] = max(worst["mse"], abs(mine["mse"] - mse) / mse)
        worst["mae"] = max(worst["mae"], abs(mine["mae"] - mae) / mae)
        if not np.isnan(pearson):
            worst["pearson"] = max(worst["pearson"], abs(mine["pearson"] - pearson))
    print("largest difference to the float32 reference:", worst)
    assert case("tied2")[2]["comparable"] == 0 and case("tied2")[2]["ci"] == 0.0
    assert np.isnan(case("constpred")[2]["pearson"]) and np.isnan(g["constpred_moments"][2])
    assert any(g[f"davis{n}_counts"][1] > 0 for n in SIZES)            # ties in the predictions are covered


def test_binned_restatement_equals_the_pairwise_one():
    """The checker of the one size that is too large for the pairwise restatement, pinned to it where both run."""
    for n, share in ((1, 0.0), (2, 0.0), (65, 0.2), (700, 0.0), (700, 0.1), (2049, 0.03)):
        p, t = davis_like(n, seed=900 + n, nan_share=share)
        a, b = restate(p, t), restate_binned(p, t)
        assert all(bits(a[k]) == bits(b[k]) for k in a), (n, share, a, b)
        assert share == 0.0 or n < 8 or (np.isnan(p).any() and np.isnan(t).any())


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the module functions
def _dev(a):
    return torch.from_numpy(np.array(a, copy=True)).to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("name", GOLDEN_CASES + [f"edge{n}" for n in EDGE_SIZES] + ["empty"])
def test_regression_metrics_equals_the_restatement(name):
    p, t, want = case(name)
    got = metrics.regression_metrics(_dev(p), _dev(t))
    assert sorted(got) == sorted(want)
    assert_equal_to_restatement(got, want, name)
    assert bits(metrics.concordance_index(_dev(p).view(p.size, 1), _dev(t).view(1, t.size))) == bits(want["ci"])
    if name == "empty":
        assert got["n"] == 0 and got["ci"] == 0.0 and all(np.isnan(got[k]) for k in ("mse", "rmse", "mae", "pearson"))
    if name == "constpred":
        assert np.isnan(got["pearson"]) and got["mse"] > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("nan_share", [0.0, 0.01])
def test_a_triangle_of_more_tile_pairs_than_workgroups(nan_share):
    """n = 100 000: 391 tiles, 76 636 tile pairs -- more than the 65 536 workgroups the pair count launches at most, so
    workgroups walk the triangle with a stride (from n = 92 417 on at a tile of 256 rows), and counts beyond 2^31.
    Checked against the binned restatement; the moments are float64 sums of 1e5 terms in another order:
    n * 2^-53 = 1.1e-11 at worst, so 1e-10 here (relative; absolute for Pearson)."""
    n = 100000
    assert (n + T - 1) // T * ((n + T - 1) // T + 1) // 2 > 65536
    p, t = davis_like(n, seed=4242, nan_share=nan_share)
    want = restate_binned(p, t)
    assert want["comparable"] > 2 ** 31 and want["tied_pred"] > 0
    got = metrics.regression_metrics(_dev(p), _dev(t))
    for key in ("n", "concordant", "tied_pred", "comparable"):
        assert got[key] == want[key], (key, got[key], want[key])
    assert bits(got["ci"]) == bits(want["ci"])
    for key in ("mse", "rmse", "mae"):
        assert close(got[key], want[key], 1e-10), (key, got[key], want[key])
    assert close(got["pearson"], want["pearson"], 1e-10, relative=False)


@pytest.mark.gpu
def test_other_float_types_are_cast_and_shapes_are_flattened():
    p, t, _ = case("davis257")
    for dtype in (torch.bfloat16, torch.float16, torch.float64):
        pd, td = _dev(p).to(dtype).view(257, 1), _dev(t).to(dtype).view(1, 257)
        want = restate(pd.float().cpu().numpy(), td.float().cpu().numpy())
        assert_equal_to_restatement(metrics.regression_metrics(pd, td), want, str(dtype))
    with pytest.raises(ValueError, match="values"):
        metrics.regression_metrics(_dev(p), _dev(t)[:-1])


# ---------------------------------------------------------------------------------------------------------------------
# GPU, kernel level: misaligned views inside canary buffers
class Raw:
    """pred / target rows at 4 bytes behind an 8-byte boundary inside canary-filled float buffers of `capacity` rows;
    one int64 buffer [c, stored, dropped, c, n, concordant, tied, comparable, c, six doubles, c]; a workspace of the
    size the library asks for with canaries on both sides."""

    def __init__(self, pred, target, capacity=None):
        self.lib = metrics.lib()
        n = len(pred)
        self.capacity = cap = n if capacity is None else capacity
        self.bufs = []
        for rows in (pred, target):
            buf = torch.full((cap + 17,), CANARY, dtype=torch.float32, device=DEV)
            assert buf.data_ptr() % 16 == 0
            buf[9:9 + n] = _dev(np.asarray(rows, dtype=np.float32))
            assert cap == 0 or buf[9:].data_ptr() % 8 == 4
            self.bufs.append(buf)
        self.words = torch.full((16,), CANARY64, dtype=torch.int64, device=DEV)
        self.words[1:3] = 0
        self.ws_bytes = metrics.workspace_bytes(cap)
        self.ws = torch.full((self.ws_bytes // 8 + 4,), CANARY64, dtype=torch.int64, device=DEV)
        self.snap = None

    def rows(self, k):
        return self.bufs[k][9:9 + self.capacity]

    def at(self, tensor, index, size=8):
        return C.c_void_p(tensor.data_ptr() + size * index)

    def stream(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def compute(self, max_rows=None, counted=False):
        max_rows = self.capacity if max_rows is None else max_rows
        rc = self.lib.cgvp_metrics_compute(self.at(self.bufs[0], 9, 4), self.at(self.bufs[1], 9, 4),
                                           self.at(self.words, 1) if counted else None, max_rows, self.at(self.words, 4),
                                           self.at(self.words, 9), self.at(self.ws, 2), self.ws_bytes, self.stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        self.check_canaries()
        host = self.words.cpu()
        return metrics._result(torch.cat([host[4:8], host[9:15]])), host[4:8].tolist() + host[9:15].tolist()

    def append(self, pred, target, dry=False):
        n = len(pred)
        src = [torch.full((n + 6,), CANARY, dtype=torch.float32, device=DEV) for _ in range(2)]
        for s, rows in zip(src, (pred, target)):
            s[3:3 + n] = _dev(np.asarray(rows, dtype=np.float32))
        before = [b.clone() for b in self.bufs] + [self.words.clone()]
        rc = self.lib.cgvp_metrics_append(self.at(src[0], 3, 4), self.at(src[1], 3, 4), n, self.at(self.bufs[0], 9, 4),
                                          self.at(self.bufs[1], 9, 4), self.capacity, self.at(self.words, 1),
                                          1 if dry else 0, self.stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        self.check_canaries()
        for s, rows in zip(src, (pred, target)):                     # the sources are only read
            assert torch.equal(s[3:3 + n].view(torch.int32), _dev(np.asarray(rows, dtype=np.float32)).view(torch.int32))
            assert bool((s[:3] == CANARY).all()) and bool((s[3 + n:] == CANARY).all())
        return before

    def reset(self):
        assert self.lib.cgvp_metrics_reset(self.at(self.words, 1), self.stream()) == 0
        torch.cuda.synchronize()
        self.check_canaries()

    def state(self):
        return self.words[1:3].tolist()

    def check_canaries(self):
        for buf in self.bufs:
            assert bool((buf[:9] == CANARY).all()) and bool((buf[9 + self.capacity:] == CANARY).all()), \
                "a canary of a row buffer was overwritten"
        assert self.words[[0, 3, 8, 15]].tolist() == [CANARY64] * 4, "a canary beside the state or the outputs was overwritten"
        assert self.ws[:2].tolist() == [CANARY64] * 2 and self.ws[2 + self.ws_bytes // 8:].tolist() == [CANARY64] * 2, \
            "the workspace was overrun"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cont1", "davis65", f"edge{T + 1}", f"edge{2 * T + 1}", f"edge{2 * CH + 1}", "empty"])
def test_misaligned_views_between_canaries_and_two_calls_bitwise_equal(name):
    """The inputs are only read, nothing is written beside the outputs and inside the workspace, and a second call on
    the same buffers returns the same bits in out_counts and out_vals."""
    p, t, want = case(name)
    raw = Raw(p, t)
    inputs = [b.clone() for b in raw.bufs]
    got, first = raw.compute()
    assert_equal_to_restatement(got, want, name)
    raw.ws[2:2 + raw.ws_bytes // 8] = -1                                # any content: the workspace needs no preparation
    _, second = raw.compute()
    assert first == second                                             # (int64 words: the doubles compare as bits)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(inputs, raw.bufs))
    assert raw.state() == [0, 0]                                       # not passed, not touched


def _workgroup_sum(acc):
    """The fixed-order workgroup sum of csrc/gvp_block_sum.h over the last axis (256 threads) in float64: the 64 lanes
    of each wave by halving (acc[l] += acc[l + off], off = 32 .. 1), then the waves 0, 1, 2, 3."""
    lanes = acc.reshape(acc.shape[:-1] + (4, 64)).copy()
    off = 32
    while off:
        lanes[..., :off] = lanes[..., :off] + lanes[..., off:2 * off]
        off >>= 1
    total = lanes[..., 0, 0].copy()
    for w in range(1, 4):
        total = total + lanes[..., w, 0]
    return total


def ordered_mean(rows):
    """The mean of float32 `rows` as moments1_kernel and means_kernel form it, addition by addition: inside a chunk of
    CH rows thread t adds rows base + k * 256 + t, k = 0 .. CH / 256 - 1, then the workgroup sum; across the chunks
    thread t adds the partials t, t + 256, ..., then the workgroup sum; last the division by n.  Rows and partials that
    do not exist are skipped on the device and added as +0.0 here, which leaves an accumulator that began as +0.0
    bitwise as it was."""
    x = np.asarray(rows, dtype=np.float32).astype(np.float64)
    n = x.size
    chunks = -(-n // CH)
    x = np.concatenate([x, np.zeros(chunks * CH - n)]).reshape(chunks, CH // 256, 256)
    acc = np.zeros((chunks, 256))
    for k in range(CH // 256):
        acc = acc + x[:, k, :]
    partial = _workgroup_sum(acc)
    partial = np.concatenate([partial, np.zeros(-chunks % 256)]).reshape(-1, 256)
    acc = np.zeros(256)
    for r in range(partial.shape[0]):
        acc = acc + partial[r]
    return float(_workgroup_sum(acc) / np.float64(n))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [256, 2048, 1 << 19])
def test_the_two_means_are_bitwise_the_documented_order_of_additions(n):
    """out_vals[4] and out_vals[5] (mean_pred, mean_target; the module drops them) against `ordered_mean`, bit for bit:
    one partly filled chunk, two chunks, and 512 chunks of which every thread of means_kernel owns two.  n is a power
    of two: the division is exact.

    The inputs are randn * 10^uniform(-6, 6).  A float32 has 24 significant bits, so float64 sums of n values within D
    decades of each other are exact, in any order, while 24 + 3.32 D + log2(n) <= 53: at n = 256 six decades show
    nothing, twelve do.  That another order of the same additions has other bits is asserted first, on the host alone,
    with np.sum as the other order; the seed is one for which that holds at all three sizes (of the seeds 0 .. 39 it
    holds for 15 at n = 256 and for 23 at n = 2048)."""
    rng = np.random.default_rng(3)
    p, t = ((rng.standard_normal(n) * 10.0 ** rng.uniform(-6.0, 6.0, n)).astype(np.float32) for _ in range(2))
    want = [ordered_mean(p), ordered_mean(t)]
    for rows, mean in zip((p, t), want):
        assert bits(mean) != bits(rows.astype(np.float64).sum() / n), "the inputs do not tell one order from another"
    _, words = Raw(p, t).compute()
    got = [struct.pack("<q", w) for w in words[8:10]]
    print(f"n={n} mean_pred {got[0].hex()} want {bits(want[0]).hex()}  mean_target {got[1].hex()} want {bits(want[1]).hex()}")
    assert got == [bits(m) for m in want]


@pytest.mark.gpu
def test_rows_behind_the_device_count_are_never_looked_at():
    """Buffers of capacity 2T+1 hold T+1 rows: the results are those of the T+1 rows alone, whatever lies behind."""
    n, cap = T + 1, 2 * T + 1
    p, t, want = case(f"edge{n}")
    alone = metrics.regression_metrics(_dev(p), _dev(t))
    rng = np.random.default_rng(5)
    for garbage in ("nan", "huge", "ties"):
        tail_p, tail_t = rng.normal(size=cap - n).astype(np.float32), rng.normal(size=cap - n).astype(np.float32)
        if garbage == "nan":
            tail_p[::2], tail_t[1::3] = np.nan, np.nan
        elif garbage == "huge":
            tail_p[:], tail_t[:] = np.inf, -3e38
        else:
            tail_p[:], tail_t[:] = p[0], t[0]
        raw = Raw(np.concatenate([p, tail_p]), np.concatenate([t, tail_t]), capacity=cap)
        raw.words[1] = n
        got, _ = raw.compute(counted=True)
        assert_equal_to_restatement(got, want, garbage)
        assert got == alone or all(bits(got[k]) == bits(alone[k]) for k in got), garbage     # (NaN != NaN)
        assert raw.state() == [n, 0]                                   # the count is only read
        whole, _ = raw.compute(max_rows=cap)                           # without a count every row of max_rows is used
        assert whole["n"] == cap
    raw.words[1] = cap + 1000                                          # a count beyond max_rows is clamped
    assert raw.compute(counted=True)[0]["n"] == cap
    raw.words[1] = -5
    assert raw.compute(counted=True)[0]["n"] == 0


@pytest.mark.gpu
def test_append_lands_in_order_and_dry_writes_nothing():
    sizes = (1, 7, 64, 300)
    p, t = davis_like(sum(sizes), seed=31, nan_share=0.05)
    raw = Raw([], [], capacity=sum(sizes) + 11)
    at = 0
    for k in sizes:
        snap = raw.append(p[at:at + k], t[at:at + k], dry=True)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(snap[:2], raw.bufs))
        assert torch.equal(snap[2], raw.words)                         # neither the state nor any buffer byte
        raw.append(p[at:at + k], t[at:at + k])
        at += k
        assert raw.state() == [at, 0]
    for k, rows in enumerate((p, t)):
        stored = raw.rows(k)[:at].cpu().numpy()
        assert stored.tobytes() == rows.tobytes()                      # bitwise, NaN payloads included
        assert bool((raw.rows(k)[at:] == CANARY).all())                # the rest of the capacity is untouched
    got, _ = raw.compute(counted=True)
    assert_equal_to_restatement(got, restate(p, t))
    raw.reset()
    assert raw.state() == [0, 0]
    assert raw.compute(counted=True)[0]["n"] == 0


@pytest.mark.gpu
def test_append_beyond_the_capacity_drops_and_counts():
    p, t = davis_like(12, seed=41)
    raw = Raw([], [], capacity=10)
    raw.append(p[:6], t[:6])
    raw.append(p[6:], t[6:])
    assert raw.state() == [10, 2]
    assert raw.rows(0).cpu().numpy().tobytes() == p[:10].tobytes() and raw.rows(1).cpu().numpy().tobytes() == t[:10].tobytes()
    raw.append(p[:3], t[:3])                                           # full: everything is dropped
    assert raw.state() == [10, 5]
    none = Raw([], [], capacity=0)                                     # a capacity of nothing drops everything
    none.append(p[:4], t[:4])
    assert none.state() == [0, 4]


# ---------------------------------------------------------------------------------------------------------------------
# GPU: RegressionMeter
def _canaried_meter(capacity, **kw):
    """A meter whose two row buffers are views into canary-filled buffers."""
    m = metrics.RegressionMeter(capacity, DEV, **kw)
    big = [torch.full((capacity + 16,), CANARY, dtype=torch.float32, device=DEV) for _ in range(2)]
    m.pred, m.target = big[0][8:8 + capacity], big[1][8:8 + capacity]
    return m, big


def _canaries_intact(big, capacity):
    return all(bool((b[:8] == CANARY).all()) and bool((b[8 + capacity:] == CANARY).all()) for b in big)


@pytest.mark.gpu
def test_meter_appends_in_order_and_computes_the_metrics_of_the_concatenation():
    sizes = (1, 7, 64, 300)
    p, t = davis_like(sum(sizes), seed=51)
    m, big = _canaried_meter(sum(sizes) + 5)
    at = 0
    for k in sizes:
        m.update(_dev(p[at:at + k]).view(k, 1), _dev(t[at:at + k]).view(k, 1))
        at += k
    assert m.state.tolist() == [at, 0]
    assert m.pred[:at].cpu().numpy().tobytes() == p.tobytes() and m.target[:at].cpu().numpy().tobytes() == t.tobytes()
    got = m.compute()
    assert got.pop("dropped") == 0
    assert_equal_to_restatement(got, restate(p, t))
    assert _canaries_intact(big, m.capacity)
    snap = [b.clone() for b in big] + [m.state.clone()]
    m.update(_dev(p[:9]), _dev(t[:9]), dry=True)                       # dry: neither the state nor any buffer byte
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(snap[:2], big)) and torch.equal(snap[2], m.state)
    m.reset()
    assert m.state.tolist() == [0, 0] and m.compute()["n"] == 0


@pytest.mark.gpu
def test_meter_overflow_is_counted_and_refused_unless_allowed():
    p, t = davis_like(12, seed=61)
    m, big = _canaried_meter(10)
    m.update(_dev(p[:6]), _dev(t[:6]))
    m.update(_dev(p[6:]), _dev(t[6:]))
    assert m.state.tolist() == [10, 2] and _canaries_intact(big, 10)
    with pytest.raises(RuntimeError, match="capacity of 10"):
        m.compute()
    got = m.compute(allow_dropped=True)
    assert got.pop("dropped") == 2
    assert_equal_to_restatement(got, restate(p[:10], t[:10]))
    m.reset()
    after = m.compute()                                                # a reset forgets the dropped rows too
    assert after["n"] == 0 and after["dropped"] == 0


@pytest.mark.gpu
def test_meter_transform_equals_applying_it_by_hand():
    p, t = davis_like(130, seed=71)
    unscale = lambda x: torch.exp(x * 0.25) - 1.5                      # not affine, as dataset.unscale_target may be
    m = metrics.RegressionMeter(200, DEV, transform=unscale)
    m.update(_dev(p[:60]), _dev(t[:60]))
    m.update(_dev(p[60:]), _dev(t[60:]))
    up = torch.cat([unscale(_dev(p[:60])), unscale(_dev(p[60:]))])
    ut = torch.cat([unscale(_dev(t[:60])), unscale(_dev(t[60:]))])
    byhand = metrics.regression_metrics(up, ut)
    got = m.compute()
    assert got.pop("dropped") == 0
    assert all(bits(got[k]) == bits(byhand[k]) for k in byhand), (got, byhand)
    assert_equal_to_restatement(got, restate(up.cpu().numpy(), ut.cpu().numpy()))


@pytest.mark.gpu
def test_a_captured_update_replays_behind_the_device_cursor():
    """One captured `update` with static inputs, replayed three times with different contents: 3n rows, in order."""
    n = 70
    p, t = davis_like(3 * n, seed=81, nan_share=0.03)
    m, big = _canaried_meter(3 * n + 3)
    sp, st = torch.zeros(n, 1, device=DEV), torch.zeros(n, 1, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.update(sp, st, dry=True)                                     # warm-up on the capture stream
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        m.update(sp, st)
    torch.cuda.synchronize()
    assert m.state.tolist() == [0, 0]                                  # neither the warm-up nor the capture added a row
    for k in range(3):
        sp.copy_(_dev(p[k * n:(k + 1) * n]).view(n, 1))
        st.copy_(_dev(t[k * n:(k + 1) * n]).view(n, 1))
        g.replay()
    torch.cuda.synchronize()
    assert m.state.tolist() == [3 * n, 0] and _canaries_intact(big, m.capacity)
    assert m.pred[:3 * n].cpu().numpy().tobytes() == p.tobytes() and m.target[:3 * n].cpu().numpy().tobytes() == t.tobytes()
    got = m.compute()
    assert got.pop("dropped") == 0
    assert_equal_to_restatement(got, restate(p, t))


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the captured training step
def _to(d):
    return {k: (tuple(t.to(DEV) for t in v) if isinstance(v, tuple) else v.to(DEV)) for k, v in d.items()}


def _model(pretrained):
    from models.joint_gnn import JointGNN
    kw = json.load(open(os.path.join(GOLDEN, "model_kwargs.json")))
    model = JointGNN(protein_gnn_kwargs=kw["protein_gnn_kwargs"], molecule_gnn_kwargs=kw["molecule_gnn_kwargs"],
                     **kw["joint_gnn_kwargs"])
    model.load_state_dict(pretrained, strict=True)
    return model.to(DEV).eval()                                  # no dropout: the runs see the same numbers


def _batches():
    """The three six-pair batches of test_fused_optimizer.py (two share a bucket)."""
    out = []
    for seed, lengths in ((1, [120, 80, 95, 130, 60, 101]), (2, [118, 83, 95, 128, 62, 100]), (3, [200, 150, 170, 90, 60, 210])):
        p, m = ds.pair_batch(6, seed, lengths=lengths)
        pd, md = _to(ds.to_torch(p)), _to(ds.to_torch(m))
        pd["ptr"], md["ptr"] = torch.as_tensor(p.ptr).to(DEV), torch.as_tensor(m.ptr).to(DEV)
        target = torch.randn(6, 1, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
        out.append((pd, md, target))
    return out


@pytest.mark.gpu
def test_captured_step_records_exactly_its_real_pairs(pretrained):
    """GraphedTrainStep(meter=...): after three runs of six pairs the meter holds 18 rows -- it would hold 12 more per
    bucket if the warm-up passes of a capture were recorded --, bitwise the returned predictions and the targets, in
    order; its MSE is the batch-size-weighted mean of the returned losses; without a meter the step returns the same
    bits.

    The runs are made under torch.use_deterministic_algorithms(True): in the default mode two captured steps of two
    model instances do not agree bitwise with each other, with or without a meter (measured: the losses of the first
    batch were 2.98887587, 2.98887610 and 2.98887634 for two plain instances and a metered one; in the mode all three
    were 2.98887682), so only there does "the same bits" say something about the meter."""
    from gvp_hip.graphed import GraphedTrainStep
    assert _lib.bridge() is not None
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        _captured_step_with_and_without_a_meter(pretrained, GraphedTrainStep)
    finally:
        torch.use_deterministic_algorithms(was)


def _captured_step_with_and_without_a_meter(pretrained, GraphedTrainStep):
    batches = _batches()
    plain = GraphedTrainStep(_model(pretrained), torch.nn.functional.mse_loss)
    without = [tuple(x.clone() for x in plain.run(*b)) for b in batches]
    m = metrics.RegressionMeter(64, DEV)
    runner = GraphedTrainStep(_model(pretrained), torch.nn.functional.mse_loss, meter=m)
    losses, preds = [], []
    for pd, md, target in batches:
        loss, pred = runner.run(pd, md, target)
        assert loss.shape == () and pred.shape == (6, 1)
        losses.append(loss.clone()), preds.append(pred.clone())
    torch.cuda.synchronize()
    assert 1 <= len(runner.buckets) <= 3 and sum(b.steps for b in runner.buckets.values()) == 3
    got = m.compute()
    assert got["n"] == 18 and got["dropped"] == 0 and m.state.tolist() == [18, 0]
    same = lambda a, b: torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    assert same(m.pred[:18], torch.cat(preds).view(-1)) and same(m.target[:18], torch.cat([b[2] for b in batches]).view(-1))
    weighted = sum(6 * float(l) for l in losses) / 18
    print(f"meter mse {got['mse']!r}, weighted mean of the losses {weighted!r}")
    assert abs(got["mse"] - weighted) <= 1e-6 * weighted
    assert_equal_to_restatement({k: v for k, v in got.items() if k != "dropped"},
                                restate(torch.cat(preds).cpu().numpy(), torch.cat([b[2] for b in batches]).cpu().numpy()))
    for (loss0, pred0), loss, pred in zip(without, losses, preds):
        assert same(loss0.view(1), loss.view(1)) and same(pred0, pred)
    with pytest.raises(TypeError, match="RegressionMeter"):
        GraphedTrainStep(_model(pretrained), torch.nn.functional.mse_loss, meter=object())
