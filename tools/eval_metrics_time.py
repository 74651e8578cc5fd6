#!/usr/bin/env python3
"""What the device-side evaluation metrics cost on one MI355X.

Three measurements, each after a warm-up of every shape it times, each repeated --repeats times for at least --seconds
of work that ends in ONE device synchronise (a host clock around the window), the variants of a measurement alternating:

  1. `gvp_hip.metrics.regression_metrics` at n = 5 000, 20 000 and 100 000 rows of Davis-like values (targets from
     eight values, predictions rounded to 0.25): the whole call, host read included (`call_ms`), and the five kernels
     of cgvp_metrics_compute alone, enqueued back to back (`device_ms`).  Beside it what stock PyTorch needs for the
     same numbers on the same device: MSELoss / L1Loss / corrcoef with an `.item()` each, as the reference's test
     evaluation calls them (`stock_moments_ms`), and the pair counts as blocked broadcast comparisons
     (`stock_pairs_ms`; the reference itself runs a Python double loop on the host: profiles/eval_metrics/README.md).
     The counts of the two are compared exactly; the difference of the float64 moments to the stock float32 ones is
     recorded (relative; absolute for Pearson).
  2. one `RegressionMeter.update` of 64 rows, eager and as the replay of a captured graph.
  3. the step of `GraphedTrainStep` with and without `meter=`, on the batches and with the method of
     tools/optimizer_step_time.py (a DIFFERENT batch every step, whole passes over the batches).

Prints one JSON object and writes it to --out.

    python tools/eval_metrics_time.py --out profiles/eval_metrics/timing.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import optimizer_step_time as ost  # noqa: E402  (puts the package on sys.path; epoch_batches, entry)
from gvp_hip import metrics  # noqa: E402
from gvp_hip.graphed import GraphedTrainStep  # noqa: E402

DEV = ost.DEV


def davis_like(n, seed):
    rng = np.random.default_rng(seed)
    values = np.array([5.0, 5.5, 6.0, 6.5, 7.0, 7.5, 8.0, 9.0], dtype=np.float32)
    w = np.array([3.0] + [1.0] * 7)
    t = rng.choice(values, size=n, p=w / w.sum()).astype(np.float32)
    p = (np.round((t + rng.normal(0.0, 0.7, n)) * 4.0) / 4.0).astype(np.float32)
    return torch.from_numpy(p).to(DEV), torch.from_numpy(t).to(DEV)


def timed(fn, seconds):
    """ms per call of fn over at least `seconds` of calls that end in one synchronise."""
    torch.cuda.synchronize()
    calls, t0 = 0, time.perf_counter()
    while True:
        fn()
        calls += 1
        if time.perf_counter() - t0 >= seconds:
            break
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def summary(v):
    return {"median": round(sorted(v)[len(v) // 2], 5), "min": round(min(v), 5), "max": round(max(v), 5)}


def stock_moments(p, t):
    mse = torch.nn.MSELoss()(p, t).item()
    mae = torch.nn.L1Loss()(p, t).item()
    pearson = torch.corrcoef(torch.stack([p, t]))[0][1].item()
    return mse, mae, pearson


def stock_pairs(p, t, block=4096):
    """(concordant, tied_pred, comparable) over all i > j by blocked broadcast comparisons in stock PyTorch."""
    n = p.numel()
    cols = torch.arange(n, device=p.device)
    total = torch.zeros(3, dtype=torch.int64, device=p.device)
    for lo in range(0, n, block):
        hi = min(lo + block, n)
        ti, pi = t[lo:hi, None], p[lo:hi, None]
        tj, pj = t[None, :hi], p[None, :hi]
        lower = cols[lo:hi, None] > cols[None, :hi]
        above, below = (ti > tj) & lower, (ti < tj) & lower
        both = above | below
        total += torch.stack([((above & (pi > pj)) | (below & (pi < pj))).sum(), (both & (pi == pj)).sum(), both.sum()])
    return [int(x) for x in total.cpu()]


def measure_compute(n, seconds, repeats):
    p, t = davis_like(n, seed=n)
    L = metrics.lib()
    out = torch.empty(10, dtype=torch.int64, device=DEV)
    ws = torch.empty(metrics.workspace_bytes(n) // 8, dtype=torch.int64, device=DEV)
    ptr = lambda x: C.c_void_p(x.data_ptr())

    def device_only():
        rc = L.cgvp_metrics_compute(ptr(p), ptr(t), None, n, ptr(out[:4]), ptr(out[4:]), ptr(ws), ws.numel() * 8,
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc

    variants = {"call_ms": lambda: metrics.regression_metrics(p, t), "device_ms": device_only,
                "stock_moments_ms": lambda: stock_moments(p, t), "stock_pairs_ms": lambda: stock_pairs(p, t)}
    got = metrics.regression_metrics(p, t)
    counts = stock_pairs(p, t)
    mse, mae, pearson = stock_moments(p, t)
    mine = [got["concordant"], got["tied_pred"], got["comparable"]]
    moments = {"mse": abs(got["mse"] - mse) / mse, "mae": abs(got["mae"] - mae) / mae, "pearson": abs(got["pearson"] - pearson)}
    for fn in variants.values():                                 # warm-up of every variant at this shape
        fn()
    ms = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            ms[k].append(timed(fn, seconds if k != "stock_pairs_ms" else min(seconds, 0.5)))
    return {"n": n, "pairs": n * (n - 1) // 2, "ci": got["ci"], "comparable": got["comparable"],
            "counts_equal_stock_pytorch": counts == mine,
            "moments_difference_to_stock_float32": moments, **{k: summary(v) for k, v in ms.items()}}


def measure_update(seconds, repeats, rows=64, per_pass=1024):
    p, t = davis_like(rows, seed=1)
    meter = metrics.RegressionMeter(rows * per_pass, DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        meter.update(p, t, dry=True)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        meter.update(p, t)
    torch.cuda.synchronize()

    def eager():
        meter.reset()
        for _ in range(per_pass):
            meter.update(p, t)

    def replay():
        meter.reset()
        for _ in range(per_pass):
            g.replay()

    variants = {"eager_us": eager, "graph_replay_us": replay}
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    assert meter.state.tolist() == [rows * per_pass, 0]
    us = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            us[k].append(timed(fn, seconds) / per_pass * 1e3)
    return {"rows": rows, "updates_per_pass": per_pass, **{k: summary(v) for k, v in us.items()}}


def measure_step(steps, seconds, repeats):
    batches = ost.epoch_batches(steps, "nominal")
    target = torch.randn(64, 1, device=DEV, generator=torch.Generator(device=DEV).manual_seed(7))
    loops = {}
    with torch.enable_grad():
        for kind in ("step_only", "step_with_meter"):
            model, _ = ost.entry._load_model(DEV)
            model.train(True)
            meter = metrics.RegressionMeter(64 * steps, DEV) if kind == "step_with_meter" else None
            runner = GraphedTrainStep(model, torch.nn.functional.mse_loss, meter=meter)

            def one_pass(runner=runner, meter=meter):
                if meter is not None:
                    meter.reset()                                # an epoch's worth of rows per pass
                for pd, md in batches:
                    runner.run(pd, md, target)
            for _ in range(2):                                   # captures every bucket, then one more warm pass
                one_pass()
            torch.cuda.synchronize()
            loops[kind] = (one_pass, runner, meter)
        ms = {kind: [] for kind in loops}
        for _ in range(repeats):
            for kind, (one_pass, _, _) in loops.items():
                ms[kind].append(timed(one_pass, seconds) / steps)
    stats = loops["step_with_meter"][2].compute()
    return {"batches_per_pass": steps, "pairs_per_step": 64, "buckets": {k: len(v[1].buckets) for k, v in loops.items()},
            "rows_in_the_meter_after_a_pass": stats["n"], "ms_per_step": {k: summary(v) for k, v in ms.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", type=int, nargs="*", default=[5000, 20000, 100000])
    ap.add_argument("--steps", type=int, default=32, help="different batches in one pass of the step measurement (0: skip it)")
    ap.add_argument("--seconds", type=float, default=1.0, help="least wall time of one measurement")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    torch.manual_seed(1234)
    result = {"device": torch.cuda.get_device_name(0), "seconds_per_measurement": args.seconds, "repeats": args.repeats,
              "tile": metrics.TILE, "chunk": metrics.CHUNK,
              "regression_metrics": [measure_compute(n, args.seconds, args.repeats) for n in args.sizes],
              "meter_update": measure_update(args.seconds, args.repeats)}
    if args.steps:
        result["graphed_train_step"] = measure_step(args.steps, args.seconds, args.repeats)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
