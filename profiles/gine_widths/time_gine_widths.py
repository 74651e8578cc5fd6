"""Device time of the GINE drug encoder per layer shape and per stack width on one MI355X, at the Davis batch-64 drug
shape (davis_synth.drug_batch(64, 0): 2,560-odd atoms, 8.2k edges incl. self loops).

Everything is timed at the C pass level -- cgvp_gine_forward_pass (training pass: aggregates and ReLU patterns saved,
CSR tables given, no dropout) and cgvp_gine_backward_pass_ex (zero fill of d x, one gine_quad_bwd_kernel per layer, one
reduce) -- with seeded nn.Linear-style weights.  A route's ITERS iterations are captured in one HIP graph and the replays
are timed between two device events: device time only, no host in the window.  Routes alternate, `--rounds` rounds;
medians and the spread are reported.

  shipped    the 2-layer 52 -> 16 -> 64 stack: forward alone (two gine_quad_fwd_kernel launches) and forward + backward,
             of the PARENT commit's library (--parent-lib, loaded beside this build's) and of this build (`base`, and
             `base_again`, a second captured graph: the spread of the two is the spread of a repeated same-code run).
  shapes     each of the 15 compiled layer shapes (cin, c, c; nt) as a ONE-layer pass: `fwd` = one gine_quad_fwd_kernel
             launch, `bwd` = (forward + backward) - forward = d x zero fill + one gine_quad_bwd_kernel + the reduce.
  chain      the drug chain alone, 52 -> h -> 64 for h in 16 / 32 / 64, forward + backward at backward caps 16 / 24 / 32
             (`max_workgroups`), and the CPU oracle's time for the same pass on the same host.
  steps      bench.py children under CGVP_LIB_PATH (same host path for both libraries): the captured Davis batch-64
             encoders step of the parent's library and of this build, alternated, and `--only protein` / `--only drug`
             of this build (the protein chain the drug chain hides behind).

Sections run in child processes under a time limit, one after the other; the first one that fails, faults or runs out
of time ends the run, and nothing further is started on the GPU.

    python profiles/gine_widths/time_gine_widths.py --parent-lib <libcaster_gvp.so of the parent> \\
        --out profiles/gine_widths/times.json
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(REPO, "caster-dta_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

DEV = "cuda:0"
ITERS = 10                  # passes per captured graph
SECTION_SECONDS = 300       # time limit of one child process
SHAPES = ([(52, c, nt) for c in (16, 32, 64) for nt in (11, 0)] + [(cin, c, 0) for cin in (16, 32, 64) for c in (16, 32, 64)])
CAPS = (16, 24, 32)
PASS_FNS = ("cgvp_gine_forward_pass", "cgvp_gine_backward_pass_ex", "cgvp_gine_bwd_workspace_bytes_ex")


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} returned {rc}")


class Stack:
    """One GINE stack on the Davis batch-64 drug batch: weights, buffers, and forward / backward calls into `handle`."""

    def __init__(self, widths, nt):
        import torch
        import davis_synth as ds
        from gvp_hip import _lib, autograd_ops, ops
        d = ds.to_torch(ds.drug_batch(64, 0))
        g = torch.Generator().manual_seed(7)
        self.N, self.E = N, E = int(d["x"].shape[0]), int(d["edge_index"].shape[1])
        self.widths, self.nt, self.cpu = widths, nt, d
        x = d["x"] if widths[0] - nt == 41 else torch.randn(N, widths[0] - nt, generator=g)
        self.x_cpu = x
        self.params_cpu = []
        for a, b in zip(widths[:-1], widths[1:]):        # _GINE_KEYS order: eps w0 b0 w1 b1 we be
            u = lambda o, i, fan: (torch.rand(o, i, generator=g) * 2 - 1) / fan ** 0.5
            self.params_cpu += [torch.tensor([0.05]), u(b, a, a), u(1, b, a)[0], u(b, b, b), u(1, b, b)[0], u(a, 14, 14),
                                u(1, a, 14)[0]]
        self.params = [p.to(DEV).contiguous() for p in self.params_cpu]
        self.cfg = autograd_ops._gine_cfg(widths, nt, 5, 9, 0.01)
        self.warr, self.keep = autograd_ops._gine_weights(self.params, len(widths) - 1)
        t = {k: v.to(DEV) for k, v in d.items()}
        csr = ops.build_csr(t["edge_index"], N)
        self.hold = (x.to(DEV).contiguous(), t["ntypes"], t["eattr"].contiguous(), t["etypes"], csr)
        self.batch = autograd_ops._batch(_lib.GineBatch, (self.hold[0], t["ntypes"] if nt else None),
                                         (self.hold[2], t["etypes"]), None, [csr.rowptr, csr.eperm, csr.esrc, csr.edst], N, E)
        self.ws = torch.zeros(autograd_ops.gine_fwd_ws_bytes(N, E, widths, True), dtype=torch.uint8, device=DEV)
        self.out = torch.empty(N, widths[-1], device=DEV)
        self.g_out = torch.randn(N, widths[-1], generator=g).to(DEV)
        nb = int(_lib.lib().cgvp_gine_bwd_workspace_bytes_ex(C.byref(self.cfg), N, E, 0))
        assert nb > 0
        self.bws = torch.empty(nb, dtype=torch.uint8, device=DEV)
        self.gflat = torch.empty(sum(p.numel() for p in self.params), device=DEV)
        self.g_x = torch.empty(N, widths[0] - nt, device=DEV)

    def routes(self, handle, cap=0):
        from gvp_hip import _lib
        for name in PASS_FNS:
            getattr(handle, name).restype, getattr(handle, name).argtypes = _lib._SIGNATURES[name]
        p = lambda t: C.c_void_p(t.data_ptr())

        def fwd():
            check(handle.cgvp_gine_forward_pass(C.byref(self.cfg), self.warr, C.byref(self.batch), 0.0, None, None, None,
                                                p(self.ws), 1, 0, p(self.out), _lib._stream()), "cgvp_gine_forward_pass")

        def fwdbwd():
            fwd()
            check(handle.cgvp_gine_backward_pass_ex(C.byref(self.cfg), self.warr, C.byref(self.batch), 0.0, None, p(self.ws),
                                                    p(self.g_out), p(self.bws), p(self.gflat), p(self.g_x), cap, 0,
                                                    _lib._stream()), "cgvp_gine_backward_pass_ex")
        return fwd, fwdbwd

    def oracle_seconds(self, runs=3):
        """The CPU oracle's forward + autograd backward of the same pass on this host: best of `runs`."""
        import torch
        from oracle import gvp_oracle as O
        names = ("eps", "nn.lins.0.weight", "nn.lins.0.bias", "nn.lins.1.weight", "nn.lins.1.bias", "lin.weight", "lin.bias")
        L = len(self.widths) - 1
        best = None
        for _ in range(runs):
            P = {f"conv_list.{l}.{n}": self.params_cpu[7 * l + k].clone().requires_grad_() for l in range(L) for k, n in enumerate(names)}
            x = self.x_cpu.clone().requires_grad_()
            t0 = time.perf_counter()
            d = self.cpu
            out = O.molecule_gine_forward(P, x, d["edge_index"], d["ntypes"], d["etypes"], d["eattr"], num_convs=L)
            (out * self.g_out.cpu()).sum().backward()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        return best


def captured(run, replays):
    """A graph of ITERS calls of `run` -> a function returning the microseconds of one call."""
    import torch
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

    def timed():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(replays):
            graph.replay()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / (replays * ITERS)
    return timed, graph


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def measure(routes, args):
    held = {k: captured(fn, args.replays) for k, fn in routes.items()}
    us = {k: [] for k in routes}
    for _ in range(args.rounds):
        for k, h in held.items():                            # the routes alternate
            us[k].append(h[0]())
    return us


def section_shipped(args):
    from gvp_hip import _lib
    s = Stack([52, 16, 64], 11)
    libs = {"base": _lib.lib(), "base_again": _lib.lib()}
    if args.parent_lib:
        libs["parent"] = C.CDLL(os.path.abspath(args.parent_lib))
    routes = {}
    for k, h in libs.items():
        routes[k + ".fwd"], routes[k + ".fwdbwd"] = s.routes(h)
    us = measure(routes, args)
    out = {"atoms": s.N, "edges": s.E, "us": {k: stats(v) for k, v in us.items()}}
    for what in ("fwd", "fwdbwd"):
        same = us["base." + what] + us["base_again." + what]
        out[what + ".same_code_spread_us"] = float(max(same) - min(same))
        if args.parent_lib:
            diff = float(np.median(us["base." + what])) - float(np.median(us["parent." + what]))
            out[what + ".base_minus_parent_us"] = diff
            out[what + ".inside_spread"] = bool(abs(diff) <= out[what + ".same_code_spread_us"])
    return out


def section_shapes(args):
    from gvp_hip import _lib
    out = {}
    for cin, c, nt in SHAPES:
        s = Stack([cin, c], nt)
        fwd, fwdbwd = s.routes(_lib.lib())
        us = measure({"fwd": fwd, "fwdbwd": fwdbwd}, args)
        bwd = [b - a for a, b in zip(us["fwd"], us["fwdbwd"])]
        out[f"({cin},{c},{c}) nt={nt}"] = {"fwd_us": stats(us["fwd"]), "bwd_us": stats(bwd)}
        print(cin, c, nt, out[f"({cin},{c},{c}) nt={nt}"], file=sys.stderr, flush=True)
    return out


def section_chain(args):
    from gvp_hip import _lib
    out = {}
    for h in (16, 32, 64):
        s = Stack([52, h, 64], 11)
        routes = {"fwd": s.routes(_lib.lib())[0]}
        for cap in CAPS:
            routes[f"fwdbwd.cap{cap}"] = s.routes(_lib.lib(), cap)[1]
        us = measure(routes, args)
        out[f"52-{h}-64"] = {"us": {k: stats(v) for k, v in us.items()}, "cpu_oracle_fwdbwd_ms": 1e3 * s.oracle_seconds()}
        print(h, out[f"52-{h}-64"], file=sys.stderr, flush=True)
    return out


def bench_ms(lib, extra):
    env = dict(os.environ)
    if lib:
        env["CGVP_LIB_PATH"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "300", "--warmup", "20"] + extra
    done = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=SECTION_SECONDS)
    if done.returncode != 0:
        raise SystemExit(f"bench.py {extra} ended with status {done.returncode}: nothing further is started")
    return float(json.loads(done.stdout.strip().splitlines()[-1])["ms_per_step"])


def section_steps(args):
    """(runs in the parent process: every bench.py is a child of its own)"""
    this = os.path.join(REPO, "caster-dta_amd", "lib", "libcaster_gvp.so")
    out = {"both_encoders_ms": {"this": [], "parent": []}}
    for _ in range(2):
        for k, lib in (("parent", args.parent_lib), ("this", this)):
            if lib:
                out["both_encoders_ms"][k].append(bench_ms(lib, []))
                print(k, out["both_encoders_ms"][k], file=sys.stderr, flush=True)
    out["protein_only_ms"] = bench_ms(this, ["--only", "protein"])
    out["drug_only_ms"] = bench_ms(this, ["--only", "drug"])
    return out


CHILD_SECTIONS = {"shipped": section_shipped, "shapes": section_shapes, "chain": section_chain}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="JSON file; sections not run keep what the file already holds")
    ap.add_argument("--parent-lib", default=None, help="libcaster_gvp.so built from the parent commit")
    ap.add_argument("--sections", default="shipped,shapes,chain,steps")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replays", type=int, default=20, help="graph replays per measurement")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:                                           # one section, in a process of its own
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("needs an MI355X: a timing taken without one says nothing")
        res = CHILD_SECTIONS[args.child](args)
        res["device"] = torch.cuda.get_device_name(0)
        print("RESULT " + json.dumps(res), flush=True)
        return
    result = json.load(open(args.out)) if args.out and os.path.exists(args.out) else {}
    result["measured_as"] = f"{ITERS} passes per HIP graph, {args.replays} replays between two device events, {args.rounds} rounds"
    for name in args.sections.split(","):
        if name == "steps":
            result[name] = section_steps(args)
        else:
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
