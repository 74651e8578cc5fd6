#!/usr/bin/env python3
"""What the per-node attention scores of a pair list cost on one MI355X beside the routes they replace.

Two pair lists over the shipped model, protein lengths drawn from the Davis table (`davis_synth.real_lengths`), the
workloads of tools/pair_scoring_time.py:

  screen   1 protein  x 1,024 drugs   (a library screened against one target)
  panel   16 proteins x    64 drugs   (a variant scan against a drug panel)

1. The op alone (seeded Gaussian operands of the model's width, all 1,024 pairs in one call), two routes to the same
   four vectors:

     pair op        `caster_gvp::cross_attention_pairs_node_scores` on the rows of the unique graphs
     gather route   `caster_gvp::expand_rows` of the unique q1 / k1 / q2 / k2 to per-pair rows, then
                    `caster_gvp::cross_attention_node_scores` on them -- the expansion IS timed, it is what the route
                    costs a caller who holds unique rows; the bytes it allocates are reported.  The batch kernel on rows
                    gathered beforehand is timed as well, to separate the kernel from the copies.

   The log-sum-exp both need comes from `caster_gvp::cross_attention_pairs_lse`, outside the clock.

2. The whole call, three routes over the SAME 1,024 pairs in the same order:

     score_pairs_with_node_attention   one call on the unique graphs
     score_pairs                       the affinities alone (what asking for the scores adds)
     batched                           `predict_with_node_attention` over the pairs collated 64 at a time -- 16 forwards,
                                       their batches built on the device beforehand (the collation is not timed)

Every figure is the median over --calls calls, each between two device events on the launch stream, after a warm-up of
that route; the routes of a workload alternate and the round is repeated --repeats times (all medians are kept).  The
routes' results are compared before anything is timed.  Prints one JSON object and writes it to --out.

    python tools/pair_node_scores_time.py --out profiles/pair_node_scores/timing.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "caster-dta_amd"), REPO, os.path.join(REPO, "tools")):
    sys.path.insert(0, p)
import __graft_entry__ as entry  # noqa: E402
import davis_synth as ds  # noqa: E402
from gvp_hip import pair_node_scores, pair_scoring as ps  # noqa: E402,F401  (pair_node_scores registers its op)
from pair_scoring_time import DEV, measure, on_device  # noqa: E402

FIELDS = ("residue_mean", "residue_max", "atom_mean", "atom_max")


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30)) if b.numel() else 0.0


def graphs_of(n_prot, n_drug, seed):
    rng = np.random.default_rng(seed)
    lengths = ds.real_lengths("davis", n_prot, seed=seed)
    prots = [ds.protein_graph(int(n), rng, 4.0, "dist") for n in lengths]
    drugs = [ds.drug_graph(rng) for _ in range(n_drug)]
    return lengths, prots, drugs


def op_alone(name, lengths, len2, calls, repeats, heads=8, width=128):
    (c,) = ps.plan_pairs(lengths, len2, None, 1 << 40)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    ptr1 = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    ptr2 = np.concatenate([[0], np.cumsum(len2)]).astype(np.int64)
    g = torch.Generator().manual_seed(0)
    N1, N2 = int(ptr1[-1]), int(ptr2[-1])
    q1, k1, v1, q2, k2, v2 = [torch.randn(n, width, generator=g).to(DEV) for n in (N1, N2, N2, N2, N1, N1)]
    t = [dev(x) for x in (ptr1, ptr2, c.g1, c.g2, c.optr1, c.optr2)]
    p1, p2, g1, g2, o1, o2 = t
    with torch.no_grad():
        _, _, lse1, lse2 = ps.cross_attention_pairs(q1, k1, v1, q2, k2, v2, *t, heads, c.rows1, c.rows2, lse=True)
        del v1, v2

        def expand():
            return (ps.expand_rows(q1, p1, g1, o1, c.rows1)[0], ps.expand_rows(k1, p2, g2, o2, c.rows2)[0],
                    ps.expand_rows(q2, p2, g2, o2, c.rows2)[0], ps.expand_rows(k2, p1, g1, o1, c.rows1)[0])

        batch_op = torch.ops.caster_gvp.cross_attention_node_scores
        pair_op = lambda: torch.ops.caster_gvp.cross_attention_pairs_node_scores(q1, k1, lse1, q2, k2, lse2, *t, heads)

        def gather_route():
            eq1, ek1, eq2, ek2 = expand()
            return batch_op(eq1, ek1, lse1, eq2, ek2, lse2, o1, o2, heads)

        gathered = expand()
        batch_kernel = lambda: batch_op(gathered[0], gathered[1], lse1, gathered[2], gathered[3], lse2, o1, o2, heads)
        a, b = pair_op(), gather_route()
        torch.cuda.synchronize()
        equal = all(bool(torch.equal(x, y)) for x, y in zip(a, b))
        times = measure({"pair_op": pair_op, "gather_route": gather_route, "batch_kernel_on_rows_gathered_beforehand": batch_kernel},
                        calls, repeats)
    return {"workload": name, "pairs": len(c.g1), "heads": heads, "width": width, "unique_rows": [N1, N2],
            "per_pair_rows": [c.rows1, c.rows2], "outputs_bitwise_equal": equal,
            "q_k_bytes_pair_op": 4 * width * 2 * (N1 + N2), "bytes_the_gather_route_allocates": 4 * width * 2 * (c.rows1 + c.rows2),
            **times, "gather_route_over_pair_op": round(times["gather_route"]["median_ms"] / times["pair_op"]["median_ms"], 3)}


def whole_call(model, name, lengths, prots, drugs, calls, repeats, group=64):
    pairs = [(p, d) for p in range(len(prots)) for d in range(len(drugs))]
    dp, dm = on_device(prots), on_device(drugs)
    batches = [(on_device([prots[p] for p, _ in pairs[i:i + group]]), on_device([drugs[d] for _, d in pairs[i:i + group]]))
               for i in range(0, len(pairs), group)]

    def batched():
        outs = [model.predict_with_node_attention(bp, bm) for bp, bm in batches]
        return torch.cat([y for y, _ in outs]), [torch.cat([getattr(s[0], f) for _, s in outs]) for f in FIELDS]

    with_scores = lambda: model.score_pairs_with_node_attention(dp, dm)       # pairs=None: the same protein-major product
    plain = lambda: model.score_pairs(dp, dm)
    (want_y, want), (y, scores, optr) = batched(), with_scores()
    torch.cuda.synchronize()
    diffs = {f: rel(getattr(scores[0], f), w) for f, w in zip(FIELDS, want)}
    len2 = [g["x_s"].shape[0] for g in drugs]
    chunks = ps.plan_pairs(lengths, len2, None, 262144)
    times = measure({"score_pairs_with_node_attention": with_scores, "score_pairs": plain, "batched_predict_with_node_attention": batched},
                    calls, repeats)
    ms = lambda k: times[k]["median_ms"]
    return {"workload": name, "proteins": len(prots), "drugs": len(drugs), "pairs": len(pairs), "protein_lengths": lengths,
            "per_pair_rows": [int(optr[0][-1]), int(optr[1][-1])], "chunks_at_default_max_rows": len(chunks),
            "forwards_of_the_batched_route": len(batches), "max_abs_difference_of_the_predictions": float((y - want_y).abs().max()),
            "rel_err_of_the_scores_against_the_batched_route": diffs, **times,
            "batched_over_with_scores": round(ms("batched_predict_with_node_attention") / ms("score_pairs_with_node_attention"), 3),
            "with_scores_over_score_pairs": round(ms("score_pairs_with_node_attention") / ms("score_pairs"), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=100, help="calls per median")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    model, _ = entry._load_model(DEV)
    model.eval()
    model.attention_weights = "never"
    ops, calls = [], []
    for name, n_prot, n_drug, seed in (("screen", 1, 1024, 11), ("panel", 16, 64, 12)):
        lengths, prots, drugs = graphs_of(n_prot, n_drug, seed)
        ops.append(op_alone(name, lengths, [g["x_s"].shape[0] for g in drugs], args.calls, args.repeats))
        torch.cuda.empty_cache()
        calls.append(whole_call(model, name, lengths, prots, drugs, args.calls, args.repeats))
        torch.cuda.empty_cache()
    result = {"device": torch.cuda.get_device_name(0), "calls_per_median": args.calls, "repeats": args.repeats,
              "op_alone": ops, "whole_call": calls}
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
