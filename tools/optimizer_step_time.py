#!/usr/bin/env python3
"""What the optimizer update costs beside the captured training step on one MI355X, stock against fused.

The batches are those of bench.py's epoch leg (442 unique Davis-sized protein graphs x 68 drug graphs, 64 pairs per
step, a DIFFERENT batch every step, inputs resident on the device).  Five loops, each on a model of its own, run in
turn inside one process:

  1. GraphedTrainStep(scaler) + scaler.unscale_ / clip_grad_norm_ / scaler.step(Adam(fused=True)) / scaler.update()
     -- the stock sequence of the reference's train_model.py:578-587
  2. the same without a scaler (clip_grad_norm_ / optimizer.step())
  3. GraphedTrainStep(scaler, optimizer=FusedAdam): the update inside the captured step
  4. the same without a scaler
  5. GraphedTrainStep alone: the step without any update

Every loop first visits every batch once (captures every bucket), then is timed with a host clock around whole passes
over the batches and ONE final synchronise, for at least --seconds per measurement; the five loops alternate and the
round is repeated --repeats times.  Prints one JSON object and writes it to --out.

    python tools/optimizer_step_time.py --out profiles/fused_optimizer/step_time.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "caster-dta_amd"), REPO):
    sys.path.insert(0, p)
import __graft_entry__ as entry  # noqa: E402
import davis_synth as ds  # noqa: E402
from gvp_hip import optim  # noqa: E402
from gvp_hip.graphed import GraphedTrainStep  # noqa: E402

DEV = torch.device("cuda:0")


def epoch_batches(steps, variant, B=64, n_prot=442, n_drug=68):
    """The batches of bench.py's epoch_leg: (protein dict, drug dict), both with 'ptr'."""
    rng = np.random.default_rng(2024)
    lengths = ds.real_lengths("davis", n_prot, seed=7) if variant == "real" else [300] * n_prot
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    prots = [ds.protein_graph(int(n), rng, 4.0, "dist") for n in lengths]
    drugs = [ds.drug_graph(rng) for _ in range(n_drug)]
    P = [dict(x_s=f(g["x_s"]), x_v=f(g["x_v"]), ei=f(g["edge_index"]), e_s=f(g["e_s"]), e_v=f(g["e_v"]), nt=f(g["ntypes"]),
              et=f(g["etypes"]), n=g["x_s"].shape[0]) for g in prots]
    D = [dict(x=f(g["x_s"]), ei=f(g["edge_index"]), ea=f(g["e_s"]), nt=f(g["ntypes"]), et=f(g["etypes"]), n=g["x_s"].shape[0])
         for g in drugs]
    out = []
    for _ in range(steps):
        pi, di = rng.integers(0, n_prot, B), rng.integers(0, n_drug, B)
        off = np.concatenate([[0], np.cumsum([P[i]["n"] for i in pi])])
        pd = dict(x=(torch.cat([P[i]["x_s"] for i in pi]), torch.cat([P[i]["x_v"] for i in pi])),
                  edge_index=torch.cat([P[i]["ei"] + int(o) for i, o in zip(pi, off)], 1).contiguous(),
                  ntypes=torch.cat([P[i]["nt"] for i in pi]), etypes=torch.cat([P[i]["et"] for i in pi]),
                  eattr=(torch.cat([P[i]["e_s"] for i in pi]), torch.cat([P[i]["e_v"] for i in pi])),
                  ptr=torch.as_tensor(off).to(DEV))
        doff = np.concatenate([[0], np.cumsum([D[i]["n"] for i in di])])
        md = dict(x=torch.cat([D[i]["x"] for i in di]),
                  edge_index=torch.cat([D[i]["ei"] + int(o) for i, o in zip(di, doff)], 1).contiguous(),
                  ntypes=torch.cat([D[i]["nt"] for i in di]), etypes=torch.cat([D[i]["et"] for i in di]),
                  eattr=torch.cat([D[i]["ea"] for i in di]), ptr=torch.as_tensor(doff).to(DEV))
        out.append((pd, md))
    return out


def make_loop(kind, batches, target, lr, clip):
    """One of the five loops: a callable that runs ONE pass over the batches."""
    model, _ = entry._load_model(DEV)
    model.train(True)
    params = list(model.parameters())
    loss_fn = torch.nn.functional.mse_loss
    scaler = torch.amp.GradScaler("cuda") if kind in ("stock_scaler", "fused_scaler") else None
    if kind.startswith("stock"):
        opt = torch.optim.Adam(params, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, fused=True)
        runner = GraphedTrainStep(model, loss_fn, scaler=scaler)

        def one_pass():
            for pd, md in batches:
                runner.run(pd, md, target)
                if scaler is not None:
                    scaler.unscale_(opt)
                if clip is not None:
                    torch.nn.utils.clip_grad_norm_(params, clip)
                if scaler is not None:
                    scaler.step(opt)
                    scaler.update()
                else:
                    opt.step()
    elif kind.startswith("fused"):
        opt = optim.FusedAdam(params, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, max_grad_norm=clip)
        runner = GraphedTrainStep(model, loss_fn, scaler=scaler, optimizer=opt)

        def one_pass():
            for pd, md in batches:
                runner.run(pd, md, target)
    else:
        runner = GraphedTrainStep(model, loss_fn)

        def one_pass():
            for pd, md in batches:
                runner.run(pd, md, target)
    return one_pass, runner, model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=32, help="different batches in one pass")
    ap.add_argument("--variant", choices=("nominal", "real"), default="nominal", help="300 residues per protein / Davis lengths")
    ap.add_argument("--seconds", type=float, default=1.0, help="least wall time of one measurement")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--clip", type=float, default=None, help="max_grad_norm (the reference's default is none)")
    args = ap.parse_args()
    torch.manual_seed(1234)
    batches = epoch_batches(args.steps, args.variant)
    target = torch.randn(64, 1, device=DEV, generator=torch.Generator(device=DEV).manual_seed(7))
    kinds = ("stock_scaler", "stock", "fused_scaler", "fused", "step_only")
    loops = {}
    with torch.enable_grad():
        for kind in kinds:
            one_pass, runner, model = make_loop(kind, batches, target, args.lr, args.clip)
            for _ in range(2):                              # captures every bucket, then one more warm pass
                one_pass()
            torch.cuda.synchronize()
            loops[kind] = (one_pass, runner, model)
        ms = {kind: [] for kind in kinds}
        for _ in range(args.repeats):
            for kind in kinds:
                one_pass = loops[kind][0]
                torch.cuda.synchronize()
                passes, t0 = 0, time.perf_counter()
                while True:
                    one_pass()
                    passes += 1
                    if time.perf_counter() - t0 >= args.seconds:
                        break
                torch.cuda.synchronize()
                ms[kind].append((time.perf_counter() - t0) / (passes * args.steps) * 1e3)
    segments = sum(1 for p in loops["fused"][2].parameters() if p.numel())
    tables = -(-segments // optim.MAX_SEGMENTS)
    finite = all(bool(torch.isfinite(p).all()) for kind in kinds for p in loops[kind][2].parameters())
    result = {"device": torch.cuda.get_device_name(0), "variant": args.variant, "batches_per_pass": args.steps,
              "pairs_per_step": 64, "seconds_per_measurement": args.seconds, "lr": args.lr, "max_grad_norm": args.clip,
              "buckets": {kind: len(loops[kind][1].buckets) for kind in kinds},
              "ms_per_step": {kind: {"median": round(sorted(v)[len(v) // 2], 4), "min": round(min(v), 4), "max": round(max(v), 4),
                                     "runs": [round(x, 4) for x in v]} for kind, v in ms.items()},
              "update_launches_fused": {"parameter_tensors": segments, "norm": tables, "scalars": 1, "apply": tables,
                                        "total": 2 * tables + 1},
              "parameters_finite_at_the_end": finite}
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
