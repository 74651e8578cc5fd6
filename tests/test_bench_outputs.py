"""bench.py --dump-outputs on the MI355X: the timed step's outputs are written, and two runs with the same arguments
compute the same arrays (seeded inputs, seeded dropout), so two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, rel_err

ARGS = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--epoch", "off", "--no-cpu-baseline"]


def _bench(out_dir, args=ARGS):
    res = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *args, "--dump-outputs", str(out_dir)],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), {p.name[:-4]: np.load(p) for p in sorted(out_dir.iterdir())}


@pytest.mark.gpu
def test_bench_dump_outputs_repeat_run_to_run(tmp_path):
    line_a, a = _bench(tmp_path / "a")
    line_b, b = _bench(tmp_path / "b")
    for line in (line_a, line_b):
        assert line["steps"] == 3 and line["ms_per_step"] > 0
    assert {"residues", "atoms"} <= set(a)
    assert any(k.startswith("grad.protein_gnn.") for k in a) and any(k.startswith("grad.molecule_gnn.") for k in a)
    assert sorted(a) == sorted(b)
    assert a["residues"].shape == (line_a["config"]["residues_per_gpu"], 64)
    assert a["atoms"].shape == (line_a["config"]["atoms_per_gpu"], 64)
    for k in a:
        assert a[k].dtype == np.float32 and np.isfinite(a[k]).all(), k
        # float atomics in the backward may reorder sums, nothing more.  The edge-embedding weights' gradients are sums
        # over every edge that cancel to a small fraction of their terms: the reordering shows there at ~1e-2 (eval mode,
        # measured); an unseeded dropout draw moves every array by O(1)
        tol = 5e-2 if k.startswith("grad.protein_gnn.gnn_model.gvp_edge.") else 1e-5
        assert rel_err(b[k], a[k]) < tol, k


@pytest.mark.gpu
def test_bench_plain_run_reports_the_headline_alone(tmp_path):
    """Without --full the run stops after the timed steps and their outputs: every side leg's field is null."""
    line, a = _bench(tmp_path / "plain", ["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert line["steps"] == 3 and line["value"] > 0 and line["ms_per_step"] > 0 and line["unit"] == "graph-pairs/sec"
    assert line["config"]["full"] is False
    assert line["roofline"] is None and line["cpu_baseline"] is None
    assert all(line["config"][k] is None for k in ("collated_csr", "epoch", "epoch_real"))
    assert {"residues", "atoms"} <= set(a)
