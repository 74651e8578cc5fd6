#!/usr/bin/env python3
"""Generate tests/golden/eval_metrics.npz from the reference's own test evaluation.

Like make_backbone_golden.py this runs ONLY where a checkout of the upstream CASTER-DTA repository is at hand
($CASTER_DTA_REFERENCE); the test-suite reads the .npz alone.  Nothing from the reference is copied: the fixture holds
seeded inputs and the numbers the reference computes from them.

What is driven, unmodified, and how: train_model.py is never imported (it is a script).  It is parsed with `ast`, and

  * the function definition `calc_concordance_index` (a nested def of its evaluation function) is compiled from its
    own syntax tree and called;
  * the right-hand sides of the assignments to `mse_loss`, `mae_loss` and `pearson_corr` are compiled from their own
    syntax trees and evaluated with `test_preds_unscaled` / `test_targets_unscaled` bound to float32 torch tensors.

The reference's function returns only the index.  The three counts behind it are read off the same unmodified
function by handing it predictions that count the comparisons it makes: `Watched` is a float whose `>`, `<` and `==`
return what float's do and count the True results.  The function compares predictions only on comparable pairs, `>`
where t_i > t_j, `<` where t_i < t_j and `==` on both, so concordant = hits(>) + hits(<), tied_pred = hits(==) and
comparable = calls(==).  The recipe asserts that the index of this run equals, bit for bit, the index of a second run
on plain NumPy arrays (the types the reference passes) and (concordant + tied_pred / 2) / comparable in float64.

Cases: n in {1, 2, 3, 63, 64, 65, 255, 256, 257, 513, 700}, each as `cont` (continuous targets and predictions),
`davis` (targets drawn from eight values, 5.0 three times as likely as each other one, predictions rounded to 0.25:
ties on both sides) and `nan` (davis with about 10 % NaN in the predictions and, separately, in the targets); `tied2`
is t = [5, 5] (nothing comparable: the index is 0) and `constpred` has constant predictions (Pearson is NaN).
Per case `<name>_pred`, `<name>_target` (float32), `<name>_counts` (int64: concordant, tied_pred, comparable),
`<name>_ci` (float64) and, except for the `nan` cases, `<name>_moments` (float64: mse, mae, pearson as float32 torch
returned them).

`--out-dir DIR --check` regenerates into DIR and compares bit for bit with the committed fixture.
"""
import argparse
import ast
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.path.abspath(os.environ["CASTER_DTA_REFERENCE"]) if os.environ.get("CASTER_DTA_REFERENCE") else None
sys.dont_write_bytecode = True

NAME = "eval_metrics.npz"
SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 513, 700)
DAVIS_VALUES = np.array([5.0, 5.5, 6.0, 6.5, 7.0, 7.5, 8.0, 9.0], dtype=np.float32)


class Watched(float):
    """A float that counts what its comparisons answer."""
    hits = {">": 0, "<": 0, "==": 0}
    calls = {">": 0, "<": 0, "==": 0}

    @classmethod
    def clear(cls):
        cls.hits, cls.calls = dict.fromkeys(cls.hits, 0), dict.fromkeys(cls.calls, 0)

    def _note(self, op, answer):
        Watched.calls[op] += 1
        Watched.hits[op] += bool(answer)
        return answer

    def __gt__(self, other):
        return self._note(">", float.__gt__(self, other))

    def __lt__(self, other):
        return self._note("<", float.__lt__(self, other))

    def __eq__(self, other):
        return self._note("==", float.__eq__(self, other))

    __hash__ = float.__hash__


def reference_pieces(path):
    """(calc_concordance_index, {name: code of the right-hand side}) from the reference's train_model.py."""
    tree = ast.parse(open(path).read(), filename=path)
    defs = [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "calc_concordance_index"]
    assert len(defs) == 1, "train_model.py: expected one calc_concordance_index"
    space = {}
    exec(compile(ast.fix_missing_locations(ast.Module(body=[defs[0]], type_ignores=[])), path, "exec"), space)
    rhs = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name) \
                and node.targets[0].id in ("mse_loss", "mae_loss", "pearson_corr"):
            assert node.targets[0].id not in rhs, node.targets[0].id
            rhs[node.targets[0].id] = compile(ast.fix_missing_locations(ast.Expression(body=node.value)), path, "eval")
    assert sorted(rhs) == ["mae_loss", "mse_loss", "pearson_corr"], sorted(rhs)
    return space["calc_concordance_index"], rhs


def cases():
    out = {}
    weights = np.array([3.0] + [1.0] * (len(DAVIS_VALUES) - 1))
    weights /= weights.sum()
    for n in SIZES:
        rng = np.random.default_rng(7000 + n)
        t = rng.normal(6.0, 1.2, n).astype(np.float32)
        out[f"cont{n}"] = ((t + rng.normal(0.0, 0.8, n)).astype(np.float32), t)
        t = rng.choice(DAVIS_VALUES, size=n, p=weights).astype(np.float32)
        p = (np.round((t + rng.normal(0.0, 0.7, n)) * 4.0) / 4.0).astype(np.float32)
        out[f"davis{n}"] = (p, t)
        p, t = p.copy(), t.copy()
        p[rng.random(n) < 0.1] = np.nan
        t[rng.random(n) < 0.1] = np.nan
        out[f"nan{n}"] = (p, t)
    out["tied2"] = (np.array([6.25, 4.5], dtype=np.float32), np.array([5.0, 5.0], dtype=np.float32))
    rng = np.random.default_rng(77)
    out["constpred"] = (np.full(64, 5.5, dtype=np.float32), rng.choice(DAVIS_VALUES, size=64).astype(np.float32))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=HERE)
    ap.add_argument("--check", action="store_true", help="compare the regenerated file bit for bit with the committed one")
    args = ap.parse_args()
    if REF is None or not os.path.isfile(os.path.join(REF, "train_model.py")):
        ap.error("set CASTER_DTA_REFERENCE to a checkout of the upstream CASTER-DTA repository")
    if args.check and os.path.abspath(args.out_dir) == HERE:
        ap.error("--check compares against the committed fixture: give --out-dir another directory")
    calc_ci, rhs = reference_pieces(os.path.join(REF, "train_model.py"))

    arrays = {}
    for name, (pred, target) in cases().items():
        assert pred.dtype == target.dtype == np.float32 and pred.shape == target.shape
        plain = float(calc_ci(target, pred))                          # the call of train_model.py:793
        Watched.clear()
        ci = float(calc_ci(target, [Watched(x) for x in pred]))
        concordant, tied, comparable = Watched.hits[">"] + Watched.hits["<"], Watched.hits["=="], Watched.calls["=="]
        assert Watched.calls[">"] + Watched.calls["<"] == comparable
        want = (concordant + 0.5 * tied) / comparable if comparable else 0.0
        assert np.float64(ci).tobytes() == np.float64(plain).tobytes() == np.float64(want).tobytes(), (name, ci, plain, want)
        arrays.update({f"{name}_pred": pred, f"{name}_target": target, f"{name}_ci": np.float64(ci),
                       f"{name}_counts": np.array([concordant, tied, comparable], dtype=np.int64)})
        line = f"eval metrics {name}: n {pred.size} concordant {concordant} tied_pred {tied} comparable {comparable} ci {ci:.6f}"
        if not name.startswith("nan"):
            space = {"torch": torch, "np": np, "test_preds_unscaled": torch.from_numpy(pred),
                     "test_targets_unscaled": torch.from_numpy(target)}
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")                       # (corrcoef of one row, of constant rows)
                moments = [float(eval(rhs[k], space)) for k in ("mse_loss", "mae_loss", "pearson_corr")]
            arrays[f"{name}_moments"] = np.array(moments, dtype=np.float64)
            line += f" mse {moments[0]:.6f} mae {moments[1]:.6f} pearson {moments[2]:.6f}"
        print(line)
    assert arrays["tied2_counts"].tolist() == [0, 0, 0] and float(arrays["tied2_ci"]) == 0.0
    assert np.isnan(arrays["constpred_moments"][2]) and np.isnan(arrays["cont1_moments"][2])
    os.makedirs(args.out_dir, exist_ok=True)
    np.savez_compressed(os.path.join(args.out_dir, NAME), **arrays)
    print("wrote", NAME, os.path.getsize(os.path.join(args.out_dir, NAME)), "bytes")
    if args.check:
        new, old = np.load(os.path.join(args.out_dir, NAME)), np.load(os.path.join(HERE, NAME))
        same = set(new.files) == set(old.files) and all(
            new[k].dtype == old[k].dtype and new[k].shape == old[k].shape and new[k].tobytes() == old[k].tobytes()
            for k in old.files)
        print("check:", "the regenerated fixture matches bit for bit" if same else "DIFFERENT")
        if not same:
            sys.exit(1)


if __name__ == "__main__":
    main()
