#!/usr/bin/env python3
"""What a training step over a BLOCK of pairs costs on one MI355X through `JointGNN.forward_pairs`, beside the collated
batch it replaces.

Shipped model, train mode (dropout on), forward + backward (`pred.sum().backward()`), protein lengths drawn from the
Davis table (`davis_synth.real_lengths`), 64 pairs per step:

  collated        model(the 64 pairs collated as an ordinary batch): 64 protein graphs, 64 drug graphs -- the route of
                  the parent code, the baseline
  block_8x8       forward_pairs on 8 proteins x 8 drugs (a ready PairTrainPlan: no host read)
  row_64x1        forward_pairs on 64 proteins x 1 drug
  column_1x64     forward_pairs on 1 protein x 64 drugs

The collated baseline of every shape holds exactly the pairs of that shape.  And the attention core alone, forward +
backward, on the 8 x 8 tables: `caster_gvp::cross_attention_pairs_train` on the unique rows against
`caster_gvp::cross_attention` on per-pair rows gathered beforehand (random operands of the model's width).

Every figure is the median over --calls calls, each between two device events on the launch stream, after a warm-up of
that route; the routes of a workload alternate and the round is repeated --repeats times (all medians are kept: their
spread is the run-to-run noise).  Prints one JSON object and writes it to --out.

    python tools/pair_training_time.py --out profiles/pair_training/timing.json
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
from gvp_hip import pair_training as pt  # noqa: E402
from pair_scoring_time import measure, on_device  # noqa: E402

DEV = torch.device("cuda:0")


def workload(model, name, n_prot, n_drug, seed, calls, repeats):
    rng = np.random.default_rng(seed)
    lengths = ds.real_lengths("davis", n_prot, seed=seed)
    prots = [ds.protein_graph(int(n), rng, 4.0, "dist") for n in lengths]
    drugs = [ds.drug_graph(rng) for _ in range(n_drug)]
    pairs = [(p, d) for p in range(n_prot) for d in range(n_drug)]
    len2 = [g["x_s"].shape[0] for g in drugs]
    dp, dm = on_device(prots), on_device(drugs)
    cp, cm = on_device([prots[p] for p, _ in pairs]), on_device([drugs[d] for _, d in pairs])
    plan = pt.plan_pair_training(lengths, len2, None)

    def collated():
        model.zero_grad(set_to_none=True)
        model(cp, cm)[0].sum().backward()

    def block():
        model.zero_grad(set_to_none=True)
        model.forward_pairs(dp, dm, plan)[0].sum().backward()

    # eval mode: the two routes compute the same function (in train mode their dropout draws differ by design)
    model.eval()
    with torch.no_grad():
        want = model(cp, cm)[0]
    got = model.forward_pairs(dp, dm, plan)[0].detach()
    torch.cuda.synchronize()
    diff = float((got - want).abs().max())
    model.train()
    times = measure({"forward_pairs": block, "collated": collated}, calls, repeats)
    a, b = times["forward_pairs"]["median_ms"], times["collated"]["median_ms"]
    return {"workload": name, "proteins": n_prot, "drugs": n_drug, "pairs": len(pairs), "protein_lengths": [int(n) for n in lengths],
            "atoms_per_drug_mean": round(float(np.mean(len2)), 2), "unique_rows": [int(sum(lengths)), int(sum(len2))],
            "per_pair_rows": [plan.rows1, plan.rows2], "eval_max_abs_difference_of_the_predictions": diff,
            "eval_max_abs_prediction": float(want.abs().max()), **times, "collated_over_forward_pairs": round(b / a, 3)}, (lengths, len2)


def trace(model, route, steps, seed=21):
    """`steps` training steps of one route of the block_8x8 workload (the graphs of `workload(.., 8, 8, 21, ..)`)."""
    rng = np.random.default_rng(seed)
    lengths = ds.real_lengths("davis", 8, seed=seed)
    prots = [ds.protein_graph(int(n), rng, 4.0, "dist") for n in lengths]
    drugs = [ds.drug_graph(rng) for _ in range(8)]
    pairs = [(p, d) for p in range(8) for d in range(8)]
    model.train()
    if route == "forward_pairs":
        dp, dm = on_device(prots), on_device(drugs)
        plan = pt.plan_pair_training(lengths, [g["x_s"].shape[0] for g in drugs], None)
        step = lambda: model.forward_pairs(dp, dm, plan)[0].sum().backward()
    else:
        cp, cm = on_device([prots[p] for p, _ in pairs]), on_device([drugs[d] for _, d in pairs])
        step = lambda: model(cp, cm)[0].sum().backward()
    for _ in range(steps):
        model.zero_grad(set_to_none=True)
        step()
    torch.cuda.synchronize()
    print(f"{route}: {steps} steps")


def attention_core(lengths, len2, calls, repeats, heads=8, width=128):
    """The 8 x 8 block's attention core alone, forward + backward."""
    plan = pt.plan_pair_training(lengths, len2, None)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    ptr1 = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    ptr2 = np.concatenate([[0], np.cumsum(len2)]).astype(np.int64)
    g = torch.Generator().manual_seed(0)
    N1, N2 = int(ptr1[-1]), int(ptr2[-1])
    ops = [torch.randn(n, width, generator=g).to(DEV).requires_grad_() for n in (N1, N2, N2, N2, N1, N1)]
    t = pt.upload(plan, DEV)
    tabs = (dev(ptr1), dev(ptr2), t["g1"], t["g2"], t["optr1"], t["optr2"], t["inv1_ptr"], t["inv1_pairs"], t["inv2_ptr"],
            t["inv2_pairs"])
    rows = lambda ptr, gi: dev(np.concatenate([np.arange(ptr[x], ptr[x + 1]) for x in gi]))
    i1, i2 = rows(ptr1, plan.g1), rows(ptr2, plan.g2)
    gathered = [x.detach().index_select(0, i).requires_grad_() for x, i in zip(ops, (i1, i2, i2, i2, i1, i1))]
    g_o1, g_o2 = torch.randn(plan.rows1, width, generator=g).to(DEV), torch.randn(plan.rows2, width, generator=g).to(DEV)

    def pair_kernels():
        o1, o2 = pt.cross_attention_pairs_train(*ops, *tabs, heads, plan.rows1, plan.rows2)
        return torch.autograd.grad([o1, o2], ops, [g_o1, g_o2])

    def batch_kernels():
        o = torch.ops.caster_gvp.cross_attention(*gathered, t["optr1"], t["optr2"], heads)
        return torch.autograd.grad([o[0], o[1]], gathered, [g_o1, g_o2])

    times = measure({"pairs_train_fwd_bwd": pair_kernels, "batch_on_gathered_rows_fwd_bwd": batch_kernels}, calls, repeats)
    return {"pairs": int(plan.g1.shape[0]), "heads": heads, "width": width, "unique_rows": [N1, N2],
            "per_pair_rows": [plan.rows1, plan.rows2], **times}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=100, help="calls per median")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--trace-route", default=None, choices=["forward_pairs", "collated"],
                    help="run --trace-steps steps of ONE route of the 8 x 8 block and nothing else (for a kernel trace: "
                         "rocprofv3 --kernel-trace --stats -- python tools/pair_training_time.py --trace-route ...)")
    ap.add_argument("--trace-steps", type=int, default=50)
    args = ap.parse_args()
    model, _ = entry._load_model(DEV)
    model.attention_weights = "never"
    if args.trace_route:
        trace(model, args.trace_route, args.trace_steps)
        return
    block, shape = workload(model, "block_8x8", 8, 8, 21, args.calls, args.repeats)
    row, _ = workload(model, "row_64x1", 64, 1, 22, args.calls, args.repeats)
    column, _ = workload(model, "column_1x64", 1, 64, 23, args.calls, args.repeats)
    result = {"device": torch.cuda.get_device_name(0), "calls_per_median": args.calls, "repeats": args.repeats,
              "mode": "train, forward + backward of pred.sum()", "workloads": [block, row, column],
              "block_attention_core": attention_core(*shape, args.calls, args.repeats)}
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
