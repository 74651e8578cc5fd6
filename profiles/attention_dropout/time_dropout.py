"""Cost of attention dropout inside the varlen cross-attention kernels on one MI355X, at the Davis batch-64 shape
(64 pairs x 300 residues = 19,200 residue rows, the atom counts of davis_synth.drug_batch(64, 0), 8 heads):

  kernels   forward + backward (three launches) through the C entry points, 20 iterations captured in one HIP graph per
            route and the replay timed with device events -- device time only, no host in the window:
              base            cgvp_attn_fwd + cgvp_attn_bwd of this build
              parent          the same of the parent commit's library (--parent-lib; loaded beside this build's)
              dropout_p0      cgvp_attn_fwd_dropout + cgvp_attn_bwd_dropout, p = 0 (must equal base: the DROP = false kernels)
              dropout_p0.1    the same, p = 0.1 in both directions: its ratio to dropout_p0 is the price of the generator
              dropout_p0.5    the same, p = 0.5 (the generator's cost does not depend on p)
  head      JointGNN.head in training mode with attention_dropout = 0.1, forward + backward, eager, a host clock around
            calls that end in one synchronise:
              varlen          this build (caster_gvp::cross_attention_dropout)
              dense_fallback  `varlen_supported` forced to False: to_dense_batch + nn.MultiheadAttention, the code the
                              parent commit runs for such a model (unchanged by this feature)

  graphed   gvp_hip.graphed.GraphedTrainStep.run of the whole golden model in training mode (staging launch + one replay of
            the captured step) with attention_dropout = 0 and = 0.1, on one batch of the same shape; host clock as above

Every route is warmed up, the routes alternate, `--rounds` rounds; medians and the spread are reported.  `--sections`
runs a subset and keeps the other sections of an existing `--out` file.

    python profiles/attention_dropout/time_dropout.py --parent-lib <libcaster_gvp.so of the parent> \\
        --out profiles/attention_dropout/timing.json
"""
import argparse
import ctypes as C
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
from gvp_hip import _lib, attention_ops, head_ops  # noqa: E402,F401

H, E = 8, 128
DEV = "cuda:0"
ITERS = 20                  # forward + backward iterations per captured graph


def shape():
    rl = [300] * 64
    al = [int(x) for x in np.diff(ds.drug_batch(64, 0).ptr)]
    return rl, al


# ------------------------------------------------------------------------------------------------ kernels
class Problem:
    """The operands, outputs and gradient buffers of one forward + backward, and the C structs over them."""

    def __init__(self, rl, al):
        g = torch.Generator().manual_seed(5)
        N, Na = sum(rl), sum(al)
        f = lambda n, w=E: torch.randn(n, w, generator=g).to(DEV)
        self.t = dict(q_r=f(N), k_a=f(Na), v_a=f(Na), q_a=f(Na), k_r=f(N), v_r=f(N), g_r=f(N), g_a=f(Na))
        self.rptr = torch.tensor([0] + list(np.cumsum(rl)), dtype=torch.long, device=DEV)
        self.aptr = torch.tensor([0] + list(np.cumsum(al)), dtype=torch.long, device=DEV)
        e = lambda n, w: torch.empty(n, w, device=DEV)
        self.o = dict(o_r=e(N, E), o_a=e(Na, E), lse_r=e(N, H), lse_a=e(Na, H), d_r=e(N, H), d_a=e(Na, H),
                      gq_r=e(N, E), gk_a=e(Na, E), gv_a=e(Na, E), gq_a=e(Na, E), gk_r=e(N, E), gv_r=e(N, E))
        self.B = len(rl)
        t, o = self.t, self.o
        self.P = (_lib.AttnProblem * 2)()
        sides = ((t["q_r"], t["k_a"], t["v_a"], self.rptr, self.aptr, o["o_r"], o["lse_r"], t["g_r"], o["d_r"], o["gq_r"], o["gk_a"], o["gv_a"]),
                 (t["q_a"], t["k_r"], t["v_r"], self.aptr, self.rptr, o["o_a"], o["lse_a"], t["g_a"], o["d_a"], o["gq_a"], o["gk_r"], o["gv_r"]))
        for p, (q, k, v, qp, kp, out, lse, g_out, delta, g_q, g_k, g_v) in zip(self.P, sides):
            p.q, p.k, p.v, p.q_ptr, p.k_ptr = q.data_ptr(), k.data_ptr(), v.data_ptr(), qp.data_ptr(), kp.data_ptr()
            p.num_q, p.num_k = int(q.shape[0]), int(k.shape[0])
            p.out, p.lse, p.g_out, p.delta = out.data_ptr(), lse.data_ptr(), g_out.data_ptr(), delta.data_ptr()
            p.g_q, p.g_k, p.g_v = g_q.data_ptr(), g_k.data_ptr(), g_v.data_ptr()
        self.pair = torch.tensor([123456789, 1], dtype=torch.int64, device=DEV)

    def rng(self, p):
        R = (_lib.Rng * 2)()
        for r, site in zip(R, (1, 2)):
            r.seed, r.p, r.stream = self.pair.data_ptr(), p, site
        return R


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} returned {rc}")


def plain_route(handle, prob):
    for name in ("cgvp_attn_fwd", "cgvp_attn_bwd"):
        getattr(handle, name).restype, getattr(handle, name).argtypes = _lib._SIGNATURES[name]

    def run():
        st = _lib._stream()
        check(handle.cgvp_attn_fwd(prob.P, 2, prob.B, H, 0.25, st), "cgvp_attn_fwd")
        check(handle.cgvp_attn_bwd(prob.P, 2, prob.B, H, 0.25, st), "cgvp_attn_bwd")
    return run


def dropout_route(prob, p):
    L, R = attention_ops.dropout_lib(), prob.rng(p)

    def run():
        st = _lib._stream()
        check(L.cgvp_attn_fwd_dropout(prob.P, 2, prob.B, H, 0.25, R, st), "cgvp_attn_fwd_dropout")
        check(L.cgvp_attn_bwd_dropout(prob.P, 2, prob.B, H, 0.25, R, st), "cgvp_attn_bwd_dropout")
    return run


def captured(run):
    """A graph of ITERS forward + backward iterations -> a function returning the microseconds of one iteration."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(ITERS):
            run()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()

    def timed(replays):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(replays):
            graph.replay()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / (replays * ITERS)
    return timed, graph


# ------------------------------------------------------------------------------------------------ head
def head_routes(rl, al):
    from models.joint_gnn import CrossAttentionModule, JointGNN
    kw = json.load(open(os.path.join(REPO, "tests", "golden", "model_kwargs.json")))
    torch.manual_seed(0)
    model = JointGNN(protein_gnn_kwargs=kw["protein_gnn_kwargs"], molecule_gnn_kwargs=kw["molecule_gnn_kwargs"],
                     **dict(kw["joint_gnn_kwargs"], attention_dropout=0.1)).to(DEV).train()
    g = torch.Generator().manual_seed(7)
    residue = torch.randn(sum(rl), 64, generator=g).to(DEV).requires_grad_()
    atom = torch.randn(sum(al), 64, generator=g).to(DEV).requires_grad_()
    side = lambda lens: {"batch": torch.repeat_interleave(torch.arange(len(lens)), torch.tensor(lens)).to(DEV),
                         "ptr": torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.long, device=DEV)}
    pdata, mdata = side(rl), side(al)
    supported = CrossAttentionModule.varlen_supported

    def step():
        y, _ = model.head(residue, atom, pdata, mdata)
        y.square().mean().backward()
        model.zero_grad(set_to_none=True)
        residue.grad = atom.grad = None

    def varlen():
        CrossAttentionModule.varlen_supported = supported
        step()

    def dense():
        CrossAttentionModule.varlen_supported = lambda self, rows: False
        try:
            step()
        finally:
            CrossAttentionModule.varlen_supported = supported
    return {"varlen": varlen, "dense_fallback": dense}


# ------------------------------------------------------------------------------------------------ whole model, captured
def graphed_routes(rl, ps=(0.0, 0.1)):
    """GraphedTrainStep.run (staging launch + one replay of the whole training step) of the golden model in training mode
    with attention_dropout 0 and 0.1, on one Davis-shaped batch."""
    from gvp_hip.graphed import GraphedTrainStep
    from models.joint_gnn import JointGNN
    kw = json.load(open(os.path.join(REPO, "tests", "golden", "model_kwargs.json")))
    pb, mb = ds.pair_batch(len(rl), 0, lengths=rl)
    to = lambda d: {k: (tuple(t.to(DEV) for t in v) if isinstance(v, tuple) else v.to(DEV)) for k, v in d.items()}
    pd, md = to(ds.to_torch(pb)), to(ds.to_torch(mb))
    pd["ptr"], md["ptr"] = torch.as_tensor(pb.ptr).to(DEV), torch.as_tensor(mb.ptr).to(DEV)
    target = torch.randn(len(rl), 1, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    routes = {}
    for p in ps:
        torch.manual_seed(0)
        model = JointGNN(protein_gnn_kwargs=kw["protein_gnn_kwargs"], molecule_gnn_kwargs=kw["molecule_gnn_kwargs"],
                         **dict(kw["joint_gnn_kwargs"], attention_dropout=p)).to(DEV).train()
        runner = GraphedTrainStep(model, torch.nn.functional.mse_loss)
        routes[f"attention_dropout_{p:g}"] = (lambda r: (lambda: r.run(pd, md, target)))(runner)
    return routes


def host_timed(fn, seconds):
    """microseconds per call over >= `seconds` of calls, one synchronise at the end"""
    fn()
    torch.cuda.synchronize()
    calls, t0 = 0, time.perf_counter()
    while True:
        for _ in range(5):
            fn()
        calls += 5
        if time.perf_counter() - t0 >= seconds:
            break
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def alternate(routes, rounds, seconds):
    for fn in routes.values():                              # warm up every route
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            us[k].append(host_timed(fn, seconds))
    return {k: stats(v) for k, v in us.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="JSON file; sections not run keep what the file already holds")
    ap.add_argument("--parent-lib", default=None, help="libcaster_gvp.so built from the parent commit")
    ap.add_argument("--sections", default="kernels,head,graphed")
    ap.add_argument("--graphed-p", default="0,0.1", help="attention_dropout values of the graphed section (one value: for a "
                    "kernel trace of that model alone)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--replays", type=int, default=50, help="graph replays per kernel measurement")
    ap.add_argument("--seconds", type=float, default=1.0, help="seconds per head / whole-model measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: a timing taken without one says nothing")
    sections = args.sections.split(",")
    rl, al = shape()
    result = json.load(open(args.out)) if args.out and os.path.exists(args.out) else {}
    result.update({"device": torch.cuda.get_device_name(0), "pairs": len(rl), "residue_rows": sum(rl), "atom_rows": sum(al),
                   "heads": H, "rounds": args.rounds})

    if "kernels" in sections:
        prob = Problem(rl, al)
        routes = {"base": plain_route(_lib.lib(), prob)}
        if args.parent_lib:
            routes["parent"] = plain_route(C.CDLL(os.path.abspath(args.parent_lib)), prob)
        for p in (0.0, 0.1, 0.5):
            routes[f"dropout_p{p:g}"] = dropout_route(prob, p)
        held = {k: captured(fn) for k, fn in routes.items()}
        us = {k: [] for k in routes}
        for _ in range(args.rounds):
            for k, (timed, _) in held.items():              # the routes alternate
                us[k].append(timed(args.replays))
        kern = {k: stats(v) for k, v in us.items()}
        result["kernels_us_per_forward_backward"] = kern
        result["kernels_measured_as"] = f"{ITERS} iterations per HIP graph, {args.replays} replays between two device events"
        result["ratio_dropout_p0_to_base"] = kern["dropout_p0"]["median"] / kern["base"]["median"]
        result["ratio_base_to_parent"] = kern["base"]["median"] / kern["parent"]["median"] if "parent" in kern else "not measured"
        result["ratio_p0.1_to_p0"] = kern["dropout_p0.1"]["median"] / kern["dropout_p0"]["median"]
        print(json.dumps(kern), flush=True)
        del held

    if "head" in sections:
        head = alternate(head_routes(rl, al), max(3, args.rounds // 2), args.seconds)
        result["head_train_step_us_eager_attention_dropout_0.1"] = head
        result["ratio_varlen_to_dense_fallback"] = head["varlen"]["median"] / head["dense_fallback"]["median"]
        print(json.dumps(head), flush=True)

    if "graphed" in sections:
        whole = alternate(graphed_routes(rl, [float(x) for x in args.graphed_p.split(",")]), max(3, args.rounds // 2), args.seconds)
        result["whole_model_graphed_train_step_us"] = whole
        if "attention_dropout_0.1" in whole and "attention_dropout_0" in whole:
            result["ratio_graphed_attention_dropout_0.1_to_0"] = (whole["attention_dropout_0.1"]["median"]
                                                                  / whole["attention_dropout_0"]["median"])
        print(json.dumps(whole), flush=True)

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
