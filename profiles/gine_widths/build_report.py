"""Compile time per translation unit and register / LDS / scratch lines of the GINE kernels, without a GPU.

    python profiles/gine_widths/build_report.py --csrc caster-dta_amd/csrc [--parent-csrc <csrc of the parent commit>] \\
        --out profiles/gine_widths/build.json --resources profiles/gine_widths/resource_usage.txt

Every .hip file of a csrc directory is compiled the way csrc/build.sh compiles it (one hipcc per file, all at once, -O3
for gfx950, -Rpass-analysis=kernel-resource-usage); the wall time of each is recorded, so the times include the contention
of the parallel build they are part of.  The resource remarks of the translation units whose name starts with `gine_quad`
are reduced to one line per kernel instantiation.
"""
import argparse
import json
import os
import re
import subprocess
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

FIELDS = {"VGPRs": "VGPRs", "AGPRs": "AGPRs", "TotalSGPRs": "SGPRs", "ScratchSize [bytes/lane]": "scratch",
          "Occupancy [waves/SIMD]": "waves/SIMD", "VGPRs Spill": "VGPR spills", "LDS Size [bytes/block]": "static LDS"}


def compile_all(csrc, tmp):
    files = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))

    def one(f):
        stem = f[:-4]
        t0 = time.perf_counter()
        with open(os.path.join(tmp, stem + ".log"), "w") as log:
            subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", "-o",
                                   os.path.join(tmp, stem + ".o"), os.path.join(csrc, f),
                                   "-Rpass-analysis=kernel-resource-usage"], stderr=log)
        return stem, time.perf_counter() - t0
    t0 = time.perf_counter()
    with ThreadPoolExecutor(len(files)) as pool:
        times = dict(pool.map(one, files))
    return times, time.perf_counter() - t0


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True).stdout.splitlines()
    return dict(zip(names, out)) if len(out) == len(names) else {n: n for n in names}


def resources(log):
    """{mangled kernel name: {field: value}} from the remarks of one translation unit"""
    out, cur = {}, None
    for line in open(log):
        m = re.search(r"remark:\s+(?:\S+:\d+:\d+:\s+)?(.+?): (\S+) \[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        k, v = m.group(1).strip(), m.group(2)
        if k == "Function Name":
            cur = out.setdefault(v, {})
        elif cur is not None:
            cur[k] = v
    return out


def short(name):
    m = re.search(r"gine_quad_(fwd|bwd)_kernel<(.*?)>\(", name)
    if not m:
        return name
    a = [x.strip() for x in m.group(2).split(",")]
    flags = ""
    if m.group(1) == "bwd":
        b = [x.replace("(bool)", "").strip() in ("true", "1") for x in a[6:9]]
        flags = " " + ("SAVED" if b[0] else "recompute") + (" STORE" if b[1] else "") + (" EG" if b[2] else "")
    return f"{m.group(1)} ({a[0]},{a[1]},{a[2]}) nt={a[3]}{flags}"


def gine_lines(tmp):
    rows = {}
    for f in sorted(os.listdir(tmp)):
        if f.startswith("gine_quad") and f.endswith(".log"):
            r = resources(os.path.join(tmp, f))
            names = demangle(list(r))
            for k, v in r.items():
                rows[short(names[k])] = "  ".join(f"{label} {v.get(fld, '?')}" for fld, label in FIELDS.items())
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", required=True)
    ap.add_argument("--parent-csrc", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--resources", default=None)
    args = ap.parse_args()
    doc, lines = {}, {}
    for tag, csrc in (("parent", args.parent_csrc), ("this", args.csrc)):
        if not csrc:
            continue
        with tempfile.TemporaryDirectory() as tmp:
            times, wall = compile_all(csrc, tmp)
            doc[tag] = {"seconds_per_translation_unit": {k: round(v, 1) for k, v in sorted(times.items(), key=lambda kv: -kv[1])},
                        "all_units_in_parallel_seconds": round(wall, 1), "cpus": os.cpu_count()}
            lines[tag] = gine_lines(tmp)
    print(json.dumps(doc, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    if args.resources:
        with open(args.resources, "w") as f:
            this, parent = lines["this"], lines.get("parent", {})
            if parent:
                same = [k for k in parent if this.get(k) == parent[k]]
                f.write(f"# {len(parent)} instantiations of the parent commit; {len(same)} of them have the same line in this build\n")
                for k in sorted(parent):
                    f.write(f"{k:48s} parent: {parent[k]}\n{'':48s} this:   {this.get(k, 'absent')}\n")
            new = sorted(k for k in this if k not in parent)
            f.write(f"# {len(new)} instantiations new in this build\n")
            for k in new:
                f.write(f"{k:48s} {this[k]}\n")


if __name__ == "__main__":
    main()
