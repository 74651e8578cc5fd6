"""Time of the four per-node attention vectors of a batch on one MI355X, two routes:

  (a) the parent commit's: caster_gvp::cross_attention_weights, its two `.max()` host reads of the longest protein /
      molecule included, then per-pair slices of the two dense tensors and `.mean(0)` / `.max(0).values` of each on the
      device (the pair lengths are host integers, as a data loader has them) -> four lists of per-pair arrays
  (b) caster_gvp::cross_attention_node_scores -> four compact vectors; (b+) the same followed by
      attention_scores.per_pair (one host read of each ptr) -> four lists of per-pair views, the form (a) ends in;
      (b graph) a replay of the op captured alone

on the davis_b64 batch (64 pairs x 300 residues, atom counts of davis_synth.drug_batch) and one long pair
([4128, 215] residues, [96, 12] atoms).  Every route is warmed up; a measurement is a host clock around at least
`--seconds` of calls that ends in one device synchronise; the routes alternate; `--rounds` rounds.  Also: the bytes
each route allocates (peak over one call) and the largest difference between the two routes' values.

    python profiles/attention_scores/time_scores.py --out profiles/attention_scores/timing.json

Kernel time, in a run of its own (`--calls N`: N calls of route (b) per batch and nothing else):

    rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/attention_scores/time_scores.py --calls 200
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(REPO, "caster-dta_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

import davis_synth as ds  # noqa: E402
from gvp_hip import attention_ops, attention_scores  # noqa: E402,F401

H, E = 8, 128
DEV = "cuda:0"


def make(rl, al, seed):
    g = torch.Generator().manual_seed(seed)
    N, Na = sum(rl), sum(al)
    q_r, k_a, v_a, q_a, k_r, v_r = [torch.randn(n, E, generator=g).to(DEV) for n in (N, Na, Na, Na, N, N)]
    rptr = torch.tensor([0] + list(np.cumsum(rl)), dtype=torch.long, device=DEV)
    aptr = torch.tensor([0] + list(np.cumsum(al)), dtype=torch.long, device=DEV)
    _, _, lse_r, lse_a = torch.ops.caster_gvp.cross_attention(q_r, k_a, v_a, q_a, k_r, v_r, rptr, aptr, H)
    return (q_r, k_a, lse_r, q_a, k_r, lse_a, rptr, aptr)


def route_a(t, rl, al):
    rptr, aptr = t[6], t[7]
    l1 = int((rptr[1:] - rptr[:-1]).max())                   # the two host reads of joint_gnn.py's need_weights branch
    l2 = int((aptr[1:] - aptr[:-1]).max())
    w_r, w_a = torch.ops.caster_gvp.cross_attention_weights(*t, H, l1, l2)
    atom_mean, atom_max, res_mean, res_max = [], [], [], []
    for b, (lr, la) in enumerate(zip(rl, al)):
        dp, pd = w_r[b, :lr, :la], w_a[b, :la, :lr]
        atom_mean.append(dp.mean(0)), atom_max.append(dp.max(0).values)
        res_mean.append(pd.mean(0)), res_max.append(pd.max(0).values)
    return atom_mean, atom_max, res_mean, res_max


def route_b(t):
    return torch.ops.caster_gvp.cross_attention_node_scores(*t, H)


def route_b_lists(t):
    am, ax, rm, rx = route_b(t)
    pp = attention_scores.per_pair
    return pp(am, t[7]), pp(ax, t[7]), pp(rm, t[6]), pp(rx, t[6])


def timed(fn, seconds):
    """microseconds per call over >= `seconds` of calls, one synchronise at the end"""
    fn()
    torch.cuda.synchronize()
    calls, t0 = 0, time.perf_counter()
    while True:
        for _ in range(20):
            fn()
        calls += 20
        if time.perf_counter() - t0 >= seconds:
            break
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=0, help="only call route (b) this often per batch (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: a timing taken without one says nothing")
    davis_al = [int(x) for x in np.diff(ds.drug_batch(64, 0).ptr)]
    batches = {"davis_b64": ([300] * 64, davis_al), "one_long_pair": ([4128, 215], [96, 12])}
    result = {"device": torch.cuda.get_device_name(0), "seconds_per_measurement": args.seconds, "batches": {}}
    for name, (rl, al) in batches.items():
        t = make(rl, al, 5)
        if args.calls:
            for _ in range(args.calls):
                route_b(t)
            torch.cuda.synchronize()
            continue
        routes = {"a_weights_then_torch": lambda: route_a(t, rl, al), "b_node_scores": lambda: route_b(t),
                  "b_node_scores_per_pair_lists": lambda: route_b_lists(t)}
        for fn in routes.values():                           # warm up every route
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            held = route_b(t)
        routes["b_graph_replay"] = graph.replay
        a, b = route_a(t, rl, al), route_b(t)
        diff = max(float((torch.cat(x) - y).abs().max()) for x, y in zip(a, b) if y.numel())
        us = {k: [] for k in routes}
        for _ in range(args.rounds):
            for k, fn in routes.items():                     # the routes alternate
                us[k].append(timed(fn, args.seconds))
        B, rmax, amax = len(rl), max(rl), max(al)
        entry = {"pairs": B, "residues": sum(rl), "atoms": sum(al), "r_max": rmax, "a_max": amax,
                 "dense_weight_bytes_2BRA": 2 * 4 * B * rmax * amax,
                 "max_abs_difference_a_vs_b": diff,
                 "peak_bytes": {"a_weights_then_torch": peak_bytes(routes["a_weights_then_torch"]),
                                "b_node_scores": peak_bytes(routes["b_node_scores"])},
                 "us_per_call": {k: {"median": float(np.median(v)), "min": min(v), "max": max(v)} for k, v in us.items()}}
        result["batches"][name] = entry
        print(name, json.dumps(entry), flush=True)
        del held, graph
    if args.out and not args.calls:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
