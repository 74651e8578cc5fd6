"""Forward + backward time of the varlen attention core per head shape on one MI355X, at the Davis batch-64 shape
(64 pairs x 300 residues = 19,200 residue rows, the atom counts of davis_synth.drug_batch(64, 0): about 40 per pair).

  hd16       (8 heads, head_dim 16), the shipped shape: cgvp_attn_fwd + cgvp_attn_bwd of the PARENT commit's library
             (--parent-lib, loaded beside this build's) and of this build, alternated in the same process; a second
             captured graph of this build's calls (`base_again`) alternates with them, and the spread of base and
             base_again together is the spread of a repeated same-code run.  `inside_spread` says whether
             |median(base) - median(parent)| lies inside it: if not, the M = 1 instantiation has changed.
  hd32_w128  (4, 32) at width 128      each: cgvp_attn_fwd_hd + cgvp_attn_bwd_hd (three launches) against `dense`, the
  hd64_w128  (2, 64) at width 128      formulation nn.MultiheadAttention runs between its projections on
  hd32_w256  (8, 32) at width 256      to_dense_batch-padded rows with key-padding masks (need_weights=True, as the
             model's dense path calls it: baddbmm of the mask, softmax, the head average of the weights, bmm), both
             directions, forward and torch.autograd backward for the same cotangents.  The padded [B, L, E] inputs are
             built once outside the timed window (the scatter and gather of to_dense_batch are NOT counted against the
             dense route).

Every route runs ITERS forward + backward iterations captured in one HIP graph, and the replay is timed with device
events: device time only, no host in the window.  Routes are warmed up and alternate, `--rounds` rounds; medians and the
spread are reported.  Each section runs in a child process of its own under a time limit, one after the other; the first
section that fails, faults or runs out of time ends the run, and nothing further is started on the GPU.

    python profiles/attention_head_dims/time_head_dims.py --parent-lib <libcaster_gvp.so of the parent> \\
        --out profiles/attention_head_dims/times.json
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(REPO, "caster-dta_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

DEV = "cuda:0"
ITERS = 20                  # forward + backward iterations per captured graph
SECTIONS = {"hd16": (8, 16), "hd32_w128": (4, 32), "hd64_w128": (2, 64), "hd32_w256": (8, 32)}
SECTION_SECONDS = 240       # time limit of one section's child process


def shape():
    import davis_synth as ds
    rl = [300] * 64
    al = [int(x) for x in np.diff(ds.drug_batch(64, 0).ptr)]
    return rl, al


class Problem:
    """The operands, outputs and gradient buffers of one forward + backward, and the C structs over them."""

    def __init__(self, rl, al, H, HD):
        import torch
        from gvp_hip import _lib
        E = H * HD
        g = torch.Generator().manual_seed(5)
        N, Na = sum(rl), sum(al)
        f = lambda n: torch.randn(n, E, generator=g).to(DEV)
        self.t = dict(q_r=f(N), k_a=f(Na), v_a=f(Na), q_a=f(Na), k_r=f(N), v_r=f(N), g_r=f(N), g_a=f(Na))
        self.rl, self.al, self.H, self.HD, self.B = rl, al, H, HD, len(rl)
        self.rptr = torch.tensor([0] + list(np.cumsum(rl)), dtype=torch.long, device=DEV)
        self.aptr = torch.tensor([0] + list(np.cumsum(al)), dtype=torch.long, device=DEV)
        e = lambda n, w: torch.empty(n, w, device=DEV)
        self.o = dict(o_r=e(N, E), o_a=e(Na, E), lse_r=e(N, H), lse_a=e(Na, H), d_r=e(N, H), d_a=e(Na, H),
                      gq_r=e(N, E), gk_a=e(Na, E), gv_a=e(Na, E), gq_a=e(Na, E), gk_r=e(N, E), gv_r=e(N, E))
        t, o = self.t, self.o
        self.P = (_lib.AttnProblem * 2)()
        sides = ((t["q_r"], t["k_a"], t["v_a"], self.rptr, self.aptr, o["o_r"], o["lse_r"], t["g_r"], o["d_r"], o["gq_r"], o["gk_a"], o["gv_a"]),
                 (t["q_a"], t["k_r"], t["v_r"], self.aptr, self.rptr, o["o_a"], o["lse_a"], t["g_a"], o["d_a"], o["gq_a"], o["gk_r"], o["gv_r"]))
        for p, (q, k, v, qp, kp, out, lse, g_out, delta, g_q, g_k, g_v) in zip(self.P, sides):
            p.q, p.k, p.v, p.q_ptr, p.k_ptr = q.data_ptr(), k.data_ptr(), v.data_ptr(), qp.data_ptr(), kp.data_ptr()
            p.num_q, p.num_k = int(q.shape[0]), int(k.shape[0])
            p.out, p.lse, p.g_out, p.delta = out.data_ptr(), lse.data_ptr(), g_out.data_ptr(), delta.data_ptr()
            p.g_q, p.g_k, p.g_v = g_q.data_ptr(), g_k.data_ptr(), g_v.data_ptr()


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} returned {rc}")


def plain_route(handle, prob):
    """cgvp_attn_fwd + cgvp_attn_bwd (head_dim 16) of `handle`: this build's library or the parent's."""
    from gvp_hip import _lib
    for name in ("cgvp_attn_fwd", "cgvp_attn_bwd"):
        getattr(handle, name).restype, getattr(handle, name).argtypes = _lib._SIGNATURES[name]

    def run():
        st = _lib._stream()
        check(handle.cgvp_attn_fwd(prob.P, 2, prob.B, prob.H, 0.25, st), "cgvp_attn_fwd")
        check(handle.cgvp_attn_bwd(prob.P, 2, prob.B, prob.H, 0.25, st), "cgvp_attn_bwd")
    return run


def hd_route(prob):
    from gvp_hip import _lib, attention_ops
    L, scale = attention_ops.hd_lib(), 1.0 / prob.HD ** 0.5

    def run():
        st = _lib._stream()
        check(L.cgvp_attn_fwd_hd(prob.P, 2, prob.B, prob.H, prob.HD, scale, None, st), "cgvp_attn_fwd_hd")
        check(L.cgvp_attn_bwd_hd(prob.P, 2, prob.B, prob.H, prob.HD, scale, None, st), "cgvp_attn_bwd_hd")
    return run


def dense_route(prob):
    """What nn.MultiheadAttention(need_weights=True) runs between its projections, on padded rows, both directions."""
    import torch
    from models.joint_gnn import to_dense_batch
    H, HD, B = prob.H, prob.HD, prob.B
    batch = lambda lens: torch.repeat_interleave(torch.arange(len(lens)), torch.tensor(lens)).to(DEV)
    rb, ab = batch(prob.rl), batch(prob.al)
    t = prob.t
    pad = lambda x, b: to_dense_batch(x, b)
    (q_r, rmask), (k_r, _), (v_r, _), (g_r, _) = (pad(t[n], rb) for n in ("q_r", "k_r", "v_r", "g_r"))
    (q_a, amask), (k_a, _), (v_a, _), (g_a, _) = (pad(t[n], ab) for n in ("q_a", "k_a", "v_a", "g_a"))
    leaves = [x.clone().requires_grad_() for x in (q_r, k_a, v_a, q_a, k_r, v_r)]
    heads = lambda x: x.view(B, x.shape[1], H, HD).transpose(1, 2).reshape(B * H, x.shape[1], HD)

    def bias(kmask):                                         # the key-padding mask as MHA merges it: [B * H, 1, Lk] of 0 / -inf
        m = torch.zeros(kmask.shape, device=DEV).masked_fill(~kmask, float("-inf"))
        return m.view(B, 1, 1, -1).expand(-1, H, -1, -1).reshape(B * H, 1, -1)
    bias_a, bias_r = bias(amask), bias(rmask)

    def direction(q, k, v, kb):
        Lq = q.shape[1]
        qh, kh, vh = heads(q) * (1.0 / HD ** 0.5), heads(k), heads(v)
        w = torch.softmax(torch.baddbmm(kb, qh, kh.transpose(-2, -1)), dim=-1)
        out = torch.bmm(w, vh).view(B, H, Lq, HD).transpose(1, 2).reshape(B, Lq, H * HD)
        return out, w.view(B, H, Lq, -1).mean(dim=1)

    def run():
        o_r, w_r = direction(leaves[0], leaves[1], leaves[2], bias_a)
        o_a, w_a = direction(leaves[3], leaves[4], leaves[5], bias_r)
        return torch.autograd.grad([o_r, o_a], leaves, [g_r, g_a]), w_r, w_a
    return run


def captured(run, replays):
    """A graph of ITERS forward + backward iterations -> a function returning the microseconds of one iteration."""
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    keep = []
    with torch.cuda.graph(graph):
        for _ in range(ITERS):
            keep.append(run())
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()

    def timed():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(replays):
            graph.replay()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / (replays * ITERS)
    return timed, graph, keep


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def section(name, args):
    """One section in this process -> its result dict."""
    import torch
    from gvp_hip import _lib
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: a timing taken without one says nothing")
    H, HD = SECTIONS[name]
    rl, al = shape()
    prob = Problem(rl, al, H, HD)
    if name == "hd16":
        routes = {"base": plain_route(_lib.lib(), prob), "base_again": plain_route(_lib.lib(), prob)}
        if args.parent_lib:
            routes["parent"] = plain_route(C.CDLL(os.path.abspath(args.parent_lib)), prob)
    else:
        routes = {"varlen": hd_route(prob), "dense": dense_route(prob)}
    held = {k: captured(fn, args.replays) for k, fn in routes.items()}
    us = {k: [] for k in routes}
    for _ in range(args.rounds):
        for k, h in held.items():                            # the routes alternate
            us[k].append(h[0]())
    out = {"heads": H, "head_dim": HD, "width": H * HD, "us_per_forward_backward": {k: stats(v) for k, v in us.items()}}
    if name == "hd16":
        same = us["base"] + us["base_again"]
        out["same_code_spread_us"] = float(max(same) - min(same))
        if "parent" in us:
            diff = abs(float(np.median(us["base"])) - float(np.median(us["parent"])))
            out["base_minus_parent_us"] = float(np.median(us["base"])) - float(np.median(us["parent"]))
            out["inside_spread"] = bool(diff <= out["same_code_spread_us"])
        else:
            out["inside_spread"] = "parent not measured"
    else:
        out["ratio_varlen_to_dense"] = out["us_per_forward_backward"]["varlen"]["median"] / out["us_per_forward_backward"]["dense"]["median"]
    out["device"] = torch.cuda.get_device_name(0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="JSON file; sections not run keep what the file already holds")
    ap.add_argument("--parent-lib", default=None, help="libcaster_gvp.so built from the parent commit")
    ap.add_argument("--sections", default=",".join(SECTIONS))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--replays", type=int, default=50, help="graph replays per measurement")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:                                           # one section, in a process of its own
        print("RESULT " + json.dumps(section(args.child, args)), flush=True)
        return
    rl, al = shape()
    result = json.load(open(args.out)) if args.out and os.path.exists(args.out) else {}
    result.update({"pairs": len(rl), "residue_rows": sum(rl), "atom_rows": sum(al), "rounds": args.rounds,
                   "measured_as": f"{ITERS} iterations per HIP graph, {args.replays} replays between two device events"})
    for name in args.sections.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--rounds", str(args.rounds), "--replays", str(args.replays)]
        if args.parent_lib:
            cmd += ["--parent-lib", args.parent_lib]
        try:
            done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=SECTION_SECONDS)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"section {name} ran out of its {SECTION_SECONDS} s: nothing further is started")
        if done.returncode != 0:
            raise SystemExit(f"section {name} ended with status {done.returncode}: nothing further is started")
        line = [l for l in done.stdout.splitlines() if l.startswith("RESULT ")][-1]
        result[name] = json.loads(line[len("RESULT "):])
        print(name, json.dumps(result[name]), flush=True)
        if args.out:                                         # after every section: a later failure keeps what was measured
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
