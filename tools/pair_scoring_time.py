#!/usr/bin/env python3
"""What `JointGNN.score_pairs` costs on one MI355X beside the route it replaces.

Two pair lists over the shipped model, protein lengths drawn from the Davis table (`davis_synth.real_lengths`):

  screen   1 protein  x 1,024 drugs   (a library screened against one target)
  panel   16 proteins x    64 drugs   (a variant scan against a drug panel)

For each, two routes over the SAME 1,024 pairs in the same order:

  score_pairs    one call on the unique graphs (every protein and every drug encoded once)
  batched        eval forwards over the pairs collated 64 at a time -- 16 forwards, their batches built on the device
                 beforehand (the collation itself is not timed), `attention_weights = "never"` so that the forwards
                 build no dense weights and read nothing back

and for the screen the attention core alone: `caster_gvp::cross_attention_pairs` on the unique rows against
`caster_gvp::cross_attention` on per-pair rows gathered beforehand (random operands of the model's width).

Every figure is the median over --calls calls, each between two device events on the launch stream, after a warm-up of
that route; the routes of a workload alternate and the round is repeated --repeats times (all medians are kept).  The
two routes' predictions are compared before anything is timed.  Prints one JSON object and writes it to --out.

    python tools/pair_scoring_time.py --out profiles/pair_scoring/timing.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "caster-dta_amd"), REPO):
    sys.path.insert(0, p)
import __graft_entry__ as entry  # noqa: E402
import davis_synth as ds  # noqa: E402
from gvp_hip import pair_scoring as ps  # noqa: E402

DEV = torch.device("cuda:0")


def on_device(graphs):
    gb = ds.collate(graphs)
    d = {k: (tuple(t.to(DEV) for t in v) if isinstance(v, tuple) else v.to(DEV)) for k, v in ds.to_torch(gb).items()}
    d["ptr"] = torch.as_tensor(gb.ptr).to(DEV)
    return d


def event_ms(fn, calls):
    """ms of every one of `calls` calls of fn, each between two events; ONE synchronise at the end."""
    marks = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    torch.cuda.synchronize()
    for a, b in marks:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in marks]


def measure(variants, calls, repeats, warm=3):
    for fn in variants.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    medians = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            medians[k].append(round(float(np.median(event_ms(fn, calls))), 4))
            print(f"{k}: {medians[k][-1]} ms", file=sys.stderr, flush=True)
    return {k: {"median_ms_per_repeat": v, "median_ms": sorted(v)[len(v) // 2]} for k, v in medians.items()}


def workload(model, name, n_prot, n_drug, seed, calls, repeats, group=64):
    rng = np.random.default_rng(seed)
    lengths = ds.real_lengths("davis", n_prot, seed=seed)
    prots = [ds.protein_graph(int(n), rng, 4.0, "dist") for n in lengths]
    drugs = [ds.drug_graph(rng) for _ in range(n_drug)]
    pairs = [(p, d) for p in range(n_prot) for d in range(n_drug)]
    dp, dm = on_device(prots), on_device(drugs)
    batches = [(on_device([prots[p] for p, _ in pairs[i:i + group]]), on_device([drugs[d] for _, d in pairs[i:i + group]]))
               for i in range(0, len(pairs), group)]

    def batched():
        return torch.cat([model(bp, bm)[0] for bp, bm in batches])

    def scored():
        return model.score_pairs(dp, dm)                           # pairs=None: the same protein-major product

    with torch.no_grad():
        want, got = batched(), scored()
        torch.cuda.synchronize()
        diff = float((got - want).abs().max())
        len2 = [g["x_s"].shape[0] for g in drugs]
        chunks = ps.plan_pairs(lengths, len2, None, 262144)
        times = measure({"score_pairs": scored, "batched": batched}, calls, repeats)
    a, b = times["score_pairs"]["median_ms"], times["batched"]["median_ms"]
    out = {"workload": name, "proteins": n_prot, "drugs": n_drug, "pairs": len(pairs), "protein_lengths": lengths,
           "atoms_per_drug_mean": round(float(np.mean(len2)), 2), "unique_rows": [int(sum(lengths)), int(sum(len2))],
           "per_pair_rows": [int(sum(c.rows1 for c in chunks)), int(sum(c.rows2 for c in chunks))],
           "chunks_at_default_max_rows": len(chunks), "forwards_of_the_batched_route": len(batches),
           "max_abs_difference_of_the_predictions": diff, "max_abs_prediction": float(want.abs().max()),
           **times, "batched_over_score_pairs": round(b / a, 3)}
    return out, (lengths, len2)


def attention_core(lengths, len2, calls, repeats, heads=8, width=128):
    """The screen's attention core alone: the pair kernel on the unique rows, the batch kernel on gathered rows."""
    (c,) = ps.plan_pairs(lengths, len2, None, 1 << 40)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    ptr1 = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    ptr2 = np.concatenate([[0], np.cumsum(len2)]).astype(np.int64)
    g = torch.Generator().manual_seed(0)
    N1, N2 = int(ptr1[-1]), int(ptr2[-1])
    q1, k1, v1, q2, k2, v2 = [torch.randn(n, width, generator=g).to(DEV) for n in (N1, N2, N2, N2, N1, N1)]
    t = [dev(x) for x in (ptr1, ptr2, c.g1, c.g2, c.optr1, c.optr2)]
    rows = lambda ptr, gi: dev(np.concatenate([np.arange(ptr[x], ptr[x + 1]) for x in gi]))
    i1, i2 = rows(ptr1, c.g1), rows(ptr2, c.g2)
    gathered = [x.index_select(0, i) for x, i in ((q1, i1), (k1, i2), (v1, i2), (q2, i2), (k2, i1), (v2, i1))]
    pair_kernel = lambda: torch.ops.caster_gvp.cross_attention_pairs(q1, k1, v1, q2, k2, v2, *t, heads, c.rows1, c.rows2)
    batch_kernel = lambda: torch.ops.caster_gvp.cross_attention(*gathered, t[4], t[5], heads)
    with torch.no_grad():
        a, b = pair_kernel(), batch_kernel()
        equal = bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))
        times = measure({"cross_attention_pairs": pair_kernel, "cross_attention_on_gathered_rows": batch_kernel}, calls, repeats)
    return {"pairs": len(c.g1), "heads": heads, "width": width, "per_pair_rows": [c.rows1, c.rows2], "outputs_bitwise_equal": equal,
            "operand_bytes_pair_kernel": 4 * width * 3 * (N1 + N2), "operand_bytes_gathered": 4 * width * 3 * (c.rows1 + c.rows2),
            **times}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=200, help="calls per median")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    model, _ = entry._load_model(DEV)
    model.eval()
    model.attention_weights = "never"
    screen, shape = workload(model, "screen", 1, 1024, 11, args.calls, args.repeats)
    panel, _ = workload(model, "panel", 16, 64, 12, args.calls, args.repeats)
    result = {"device": torch.cuda.get_device_name(0), "calls_per_median": args.calls, "repeats": args.repeats,
              "workloads": [screen, panel], "screen_attention_core": attention_core(*shape, args.calls, args.repeats)}
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
