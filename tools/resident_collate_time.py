#!/usr/bin/env python3
"""What assembling one side of a batch costs on one MI355X from a resident store (`gvp_hip.resident`), beside the two
ways there were before.

The Davis batch-64 shape: 64 proteins with lengths drawn from the Davis table (`davis_synth.real_lengths`), 64 drugs.

  (a) resident   `store.collate(plan)` with a ready plan: ONE launch of cgvp_collate_graphs per side (fresh outputs),
                 and the same with `out=` static buffers
  (b) torch      the same batch from the same resident tensors with stock torch: torch.cat of the slices, the offset
                 add on edge_index, repeat_interleave for `batch` (about 8 launches a side)
  (c) host       what a user does without a store: `davis_synth.collate` on the host and `to_torch(..., device)`;
                 host clock around work that ends in a synchronise
  plan           `store.plan(ids)`: host arithmetic and the one upload; host clock ending in a synchronise

(a) and (b) are the median over --calls calls, each between two device events on the launch stream, after a warm-up;
they alternate, and the round is repeated --repeats times (all medians are kept: their spread is the run-to-run noise).
(c) and plan are medians of --host-calls calls per round.  The bytes a collate moves (read plus written, from the
shapes) are printed for the kernel-time rate: with `--kernel-only N` the tool just runs N collates per side, for

    rocprofv3 --kernel-trace --stats -d profiles/resident_collate/trace -o collate -- \\
        python tools/resident_collate_time.py --kernel-only 200 --side protein

Prints one JSON object and writes it to --out.

    python tools/resident_collate_time.py --out profiles/resident_collate/timing.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "caster-dta_amd"), REPO, os.path.dirname(os.path.abspath(__file__))):
    sys.path.insert(0, p)
import davis_synth as ds  # noqa: E402
from gvp_hip import resident  # noqa: E402
from pair_scoring_time import measure  # noqa: E402

DEV = torch.device("cuda:0")


def torch_collate(store, plan, slices):
    """(b): the batch of `plan` from the store's tensors with stock torch ops; `slices` are the host (start, stop) rows."""
    T = store.tensors
    nodes, edges = slices
    cat = lambda t, s: torch.cat([t[a:b] for a, b in s])
    ptr = plan.ptr
    eoff = plan.table[2 * plan.B + 1:]
    shift = torch.repeat_interleave(ptr[:-1], eoff[1:] - eoff[:-1], output_size=plan.E)
    ei = torch.cat([T["edge_index"][:, a:b] for a, b in edges], dim=1) + shift
    batch = torch.repeat_interleave(torch.arange(plan.B, device=DEV), ptr[1:] - ptr[:-1], output_size=plan.N)
    x = (cat(T["x_s"], nodes), cat(T["x_v"], nodes)) if store.vector else cat(T["x_s"], nodes)
    ea = (cat(T["e_s"], edges), cat(T["e_v"], edges)) if store.vector else cat(T["e_s"], edges)
    return dict(x=x, edge_index=ei, ntypes=cat(T["ntypes"], nodes), etypes=cat(T["etypes"], edges), eattr=ea, batch=batch,
                ptr=ptr)


def host_ms(fn, calls):
    out = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(out)), 4)


def moved_bytes(d):
    """Bytes one collate moves: every output tensor is written once; all but `batch` are read once from the store."""
    written = sum(t.numel() * t.element_size() for k, v in d.items() if k != "ptr" for t in (v if isinstance(v, tuple) else (v,)))
    return dict(written=int(written), read=int(written - d["batch"].numel() * 8), total=int(2 * written - d["batch"].numel() * 8))


def side(name, graphs, ids, args):
    store = resident.ResidentGraphs(graphs, DEV)
    plan = store.plan(ids)
    slices = ([(int(store.node_off[i]), int(store.node_off[i + 1])) for i in ids],
              [(int(store.edge_off[i]), int(store.edge_off[i + 1])) for i in ids])
    picked = [graphs[i] for i in ids]
    got = store.collate(plan)
    want = ds.to_torch(ds.collate(picked), DEV)
    other = torch_collate(store, plan, slices)
    torch.cuda.synchronize()
    for k, v in want.items():                                      # what is timed computes the same batch, bitwise
        for a, b, c in zip(*(d[k] if isinstance(d[k], tuple) else (d[k],) for d in (got, want, other))):
            view = (lambda t: t.view(torch.int32)) if a.is_floating_point() else (lambda t: t)
            assert torch.equal(view(a), view(b)) and torch.equal(view(c), view(b)), k
    static = {k: (tuple(torch.empty_like(t) for t in v) if isinstance(v, tuple) else torch.empty_like(v))
              for k, v in got.items() if k != "ptr"}
    res = dict(graphs=len(ids), unique=len(store), nodes=plan.N, edges=plan.E, store_bytes=store.nbytes, bytes=moved_bytes(got))
    if args.kernel_only:
        for _ in range(args.kernel_only):
            store.collate(plan, out=static)
        torch.cuda.synchronize()
        return res
    res["device_events_ms"] = measure({"a_resident_collate": lambda: store.collate(plan),
                                       "a_resident_collate_out": lambda: store.collate(plan, out=static),
                                       "b_torch_cat": lambda: torch_collate(store, plan, slices)}, args.calls, args.repeats)
    res["host_clock_to_sync_ms"] = {
        "c_host_collate_upload": [host_ms(lambda: ds.to_torch(ds.collate(picked), DEV), args.host_calls) for _ in range(args.repeats)],
        "plan": [host_ms(lambda: store.plan(ids), args.host_calls) for _ in range(args.repeats)],
        "plan_and_collate": [host_ms(lambda: store.collate(store.plan(ids)), args.host_calls) for _ in range(args.repeats)],
    }
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--host-calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--unique", type=int, default=64, help="unique proteins in the store (the batch holds 64 of them, permuted)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--kernel-only", type=int, default=0)
    ap.add_argument("--side", default="both", choices=["both", "protein", "molecule"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("resident_collate_time: needs the MI355X; nothing is measured without it")
    rng = np.random.default_rng(args.seed)
    lengths = ds.real_lengths("davis", args.unique, seed=args.seed)
    prots = [ds.protein_graph(int(n), rng, 4.0, "dist") for n in lengths]
    drugs = [ds.drug_graph(rng) for _ in range(68)]
    pids = [int(i) for i in rng.permutation(args.unique)[:64]]
    mids = [int(i) for i in rng.integers(0, 68, size=64)]
    result = dict(device=torch.cuda.get_device_name(0), calls=args.calls, repeats=args.repeats, host_calls=args.host_calls,
                  protein_lengths=[lengths[i] for i in pids])
    if args.side in ("both", "protein"):
        result["protein"] = side("protein", prots, pids, args)
    if args.side in ("both", "molecule"):
        result["molecule"] = side("molecule", drugs, mids, args)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
