#!/usr/bin/env python3
"""What one `gvp_hip.ops.protein_graphs` call costs on one MI355X, beside the float64 NumPy restatement of
tests/test_backbone_graph.py on the same host (the reference featuriser itself does not travel with this repository).

Workloads: the davis_b64 protein batch (64 x 300 residues) and one 4,128-residue chain (KIBA's longest), radius 4.0
and kNN-30.  Each call is bracketed with device events; the figure is the median of 200 calls after 20 warm-up calls,
three repeats.  The 'dist' path includes its one host read of E.  Prints one JSON object and writes it to --out.

    python tools/backbone_graph_time.py --out profiles/backbone_graph/protein_graphs_time.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "caster-dta_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)
import davis_synth as ds  # noqa: E402
import test_backbone_graph as restated  # noqa: E402
from gvp_hip import ops  # noqa: E402

DEV = "cuda:0"


def backbones(lengths, seed):
    rng = np.random.default_rng(seed)
    return [restated._synthetic_backbone(ds.ca_trace(L, rng), rng) for L in lengths]


def device_ms(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu-runs", type=int, default=3)
    args = ap.parse_args()
    props = np.random.default_rng(0).uniform(size=(21, 11)).astype(np.float32)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    result = {"device": torch.cuda.get_device_name(0), "calls": args.calls, "repeats": args.repeats, "workloads": {}}
    for name, lengths in (("davis_b64_64x300", [300] * 64), ("kiba_longest_1x4128", [4128])):
        chains = backbones(lengths, 1)
        types = [np.random.default_rng(2).integers(0, 20, size=L).astype(np.int64) for L in lengths]
        coords, ty = T(np.concatenate(chains)), T(np.concatenate(types))
        ptr, pr = T(np.cumsum([0] + lengths).astype(np.int64)), T(props)
        entry = {"residues": int(sum(lengths))}
        for kind, thresh in (("dist", 4.0), ("num", 30)):
            call = lambda: ops.protein_graphs(coords, ty, ptr, pr, edge_thresh=thresh, thresh_type=kind)
            E = int(call()["edge_index"].shape[1])
            known = (lambda: ops.protein_graphs(coords, ty, ptr, pr, edge_thresh=thresh, thresh_type=kind, num_edges=E))
            gpu = [device_ms(call, args.calls, 20) for _ in range(args.repeats)]
            gpu_known = [device_ms(known, args.calls, 20) for _ in range(args.repeats)]
            cpu = []
            for _ in range(args.cpu_runs):
                t0 = time.perf_counter()
                for c, t in zip(chains, types):
                    restated.numpy_protein_graph(c, t, props, thresh, kind)
                cpu.append(1e3 * (time.perf_counter() - t0))
            entry[f"{kind}_{thresh:g}"] = {"edges": E, "gpu_ms_median_per_repeat": gpu,
                                           "gpu_ms_num_edges_given_per_repeat": gpu_known,
                                           "numpy_float64_ms_per_run": cpu,
                                           "speedup_of_medians": statistics.median(cpu) / statistics.median(gpu)}
        result["workloads"][name] = entry
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
