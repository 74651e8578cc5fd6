"""The golden recipe (tests/golden/make_golden.py) drives the REFERENCE, never this repo's own `models` package.  That it
reproduces the committed fixtures bit for bit is the recipe's own check, run where an upstream checkout is at hand:
`CASTER_DTA_REFERENCE=<checkout> python tests/golden/make_golden.py --out-dir <dir> --check`."""
import os
import subprocess
import sys

from conftest import GOLDEN


def test_recipe_refuses_to_run_without_the_reference(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("PYTHONPATH", "CASTER_DTA_REFERENCE")}
    res = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden.py"), "--out-dir", str(tmp_path), "--check"],
                         cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 2 and "CASTER_DTA_REFERENCE" in res.stderr
    assert not list(tmp_path.iterdir())                                  # nothing written


def test_recipe_never_imports_this_repo():
    """Static guard for the failure VERDICT r01 found: caster-dta_amd/ on sys.path makes `import models`
    resolve to the product (regular package beats the reference's namespace package)."""
    src = open(os.path.join(GOLDEN, "make_golden.py")).read()
    assert "sys.path.insert(0, os.path.join(REPO" not in src
    assert 'startswith(REF + "/")' in src


def test_sparse_golden_is_in_the_fused_regime(lba_sparse):
    g = lba_sparse
    assert g["edge_index"].shape[1] <= 4 * g["x_s"].shape[0]        # gvp_hip.ops.fuse_layer's condition
    assert len(g["ptr"]) == 4 and len({int(b - a) for a, b in zip(g["ptr"][:-1], g["ptr"][1:])}) == 3   # ragged
