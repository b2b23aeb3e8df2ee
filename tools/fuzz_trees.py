#!/usr/bin/env python3
"""Randomised parity soak of tree-ensemble SCORING (config 5's kernels; src/model.rs:64-84,104-112): random small
datasets (1..40 features, integer / duplicated / heavy-tailed columns, NaN, +-inf, -0.0, denormals) and random
forests -- depths 0..11, 1..400 trees, feature subsets of every size (odd and even slot counts of the threshold-rank
kernel), thresholds drawn from the data (x == thr ties), from between data values, repeated across trees, non-f32
doubles, beyond the f32 range; features the dataset does not have; negative / zero / huge weights; bare single trees.
Every dataset's second forest is one of the deterministic shapes of tools/forest_shapes.py (leaf-wise trees, stumps at the
threshold-count limits, combs at the child-offset limit of the LDS walk, chains of up to 40 levels), and every third dataset
is wide (200, 320 or 700 features, few documents), so that the 128- and 64-document shapes of the LDS walk and both variants
of the L2 walk are reached; the summary counts the paths the library reports (native.last_tree_plan).
The device scores must equal the oracle's bit for bit (NaN features compare false, as in the oracle; a sum that overflows to
inf - inf = NaN must be NaN on both sides).
Usage: python tools/fuzz_trees.py --iters 300 [--seed 0]"""
import argparse
import collections
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))
import fastrank_amd as fr  # noqa: E402
from fastrank_amd import native  # noqa: E402
from oracle import pyoracle as o  # noqa: E402
import forest_shapes as ts  # noqa: E402  (tools/forest_shapes.py, beside this file)

WIDE = (200, 320, 700)
SHAPE_KINDS = ("leafwise", "stumps", "comb", "chain")


def make_matrix(rng, wide=None):
    n = int(rng.choice([1, 7, 64, 65, 191, 192, 193, 500, 1500, 4000]))
    d = int(rng.choice([1, 2, 3, 4, 5, 8, 13, 24, 40]))
    if wide is not None:  # few documents: the columns, not the rows, are what these reach
        n, d = int(rng.choice([1, 65, 193, 449])), wide
    X = np.empty((n, d), dtype=np.float32)
    for j in range(d):
        kind = rng.integers(0, 6)
        if kind == 0:
            col = rng.integers(-3, 4, n).astype(np.float32)                      # few distinct integers
        elif kind == 1:
            col = rng.lognormal(0, 3, n).astype(np.float32)                      # heavy tail
        elif kind == 2:
            col = rng.normal(0, 1, n).astype(np.float32)
        elif kind == 3:
            col = np.float32(rng.choice([0.0, -0.0, 1e-45, -1e-45, 1.0, 3.4028235e38, -3.4028235e38], n))
        elif kind == 4:
            col = np.round(rng.normal(0, 2, n), 1).astype(np.float32)            # decimals that are not f32-exact
        else:
            col = np.zeros(n, dtype=np.float32)                                  # constant column
        if rng.random() < 0.25:
            bad = rng.random(n) < 0.05
            col[bad] = rng.choice(np.float32([np.nan, np.inf, -np.inf]), int(bad.sum()))
        X[:, j] = col
    y = rng.integers(0, 5, n).astype(np.float64)
    qid = np.sort(rng.integers(0, max(1, n // 20) + 1, n)).astype(np.int64)
    return X, y, qid


def draw_weights(rng, ntrees):
    wk = rng.integers(0, 4)
    if wk == 0:
        return [1.0] * ntrees
    if wk == 1:
        return rng.uniform(-1, 1, ntrees).tolist()
    if wk == 2:
        return rng.choice([0.0, -0.0, 1.0, 1e-300, 3.0], ntrees).tolist()
    return rng.lognormal(0, 2, ntrees).tolist()


def feature_pool(rng, d):
    nfeat_pool = int(rng.integers(1, min(d, 40) + 1))
    pool = rng.choice(d, size=nfeat_pool, replace=False)
    if rng.random() < 0.3:
        pool = np.concatenate([pool, [d + int(rng.integers(0, 5))]])             # a feature the dataset lacks: reads 0.0
    return pool


def make_forest(rng, X, kind=None, turn=0):
    n, d = X.shape
    pool = feature_pool(rng, d)
    depth = int(rng.choice([0, 1, 2, 3, 5, 7, 8, 9, 10, 11], p=[.03, .07, .1, .1, .15, .2, .15, .08, .07, .05]))
    ntrees = int(rng.choice([1, 2, 3, 8, 31, 32, 33, 77, 200, 400], p=[.1, .05, .05, .1, .1, .1, .1, .2, .15, .05]))
    if depth >= 9:
        ntrees = min(ntrees, 33)
    p_leaf = float(rng.choice([0.0, 0.05, 0.2]))
    shared = [float(v) for v in rng.normal(0, 1, 4)]                              # thresholds repeated across trees

    def threshold(f):
        col = X[:, f] if f < d else np.zeros(1, dtype=np.float32)
        fin = col[np.isfinite(col)]
        k = rng.integers(0, 6)
        if k == 0 and len(fin):
            return float(fin[rng.integers(0, len(fin))])                          # exactly a data value
        if k == 1 and len(fin):
            return float(np.nextafter(np.float64(fin[rng.integers(0, len(fin))]), rng.choice([-np.inf, np.inf])))
        if k == 2:
            return shared[int(rng.integers(0, len(shared)))]
        if k == 3:
            return float(rng.choice([0.0, -0.0, 1e300, -1e300, 1e-46, 0.1, 3.4028235e38, -3.4028236e38]))
        if len(fin):
            return float(np.quantile(fin.astype(np.float64), rng.random()))
        return float(rng.normal())

    def draw_leaf():
        return {"LeafNode": float(rng.choice([rng.uniform(-2, 4), 0.0, -0.0, 1e300, rng.integers(-3, 4)]))}

    def grow(dd):
        if dd == 0 or rng.random() < p_leaf:
            return draw_leaf()
        f = int(pool[rng.integers(0, len(pool))])
        return {"FeatureSplit": {"fid": f, "split": threshold(f), "lhs": grow(dd - 1), "rhs": grow(dd - 1)}}

    if kind is None:
        trees = [grow(depth) for _ in range(ntrees)]
        return trees, draw_weights(rng, ntrees)

    class Pick:  # what the builders of forest_shapes.py draw nodes and leaves from
        pass
    pick = Pick()
    pick.rng = rng
    pick.leaf = draw_leaf

    def node():
        f = int(pool[rng.integers(0, len(pool))])
        return f, threshold(f)
    pick.node = node
    stumps = [ts.chain(1, "left", pick) for _ in range(int(rng.choice([0, 3, 11])))]
    if kind == "leafwise":
        trees = [ts.leafwise(int(rng.choice([32, 255])), pick) for _ in range(int(rng.choice([1, 5, 33])))]
    elif kind == "stumps":  # distinct thresholds of one feature next to the limits of the rank tables (data values: x == thr ties)
        f = int(pool[0]) if pool[0] < d else 0
        count = int(rng.choice([255, 256, 511, 512, 1023, 1024]))
        values = np.unique(np.concatenate([X[:, f][np.isfinite(X[:, f])].astype(np.float64), rng.normal(0, 2, count).astype(np.float32).astype(np.float64)]))
        trees = ts.stumps_with_thresholds(f, rng.permutation(values)[:count], pick) + stumps
    elif kind == "comb":    # the LDS walk's child offset is 8 bits: (12, 7, right) is its last admitted comb, left combs one level lower
        trees = [ts.comb(12, (8, 6, 7)[turn % 3], pick, ts.SIDES[turn % 3])] + stumps  # refused (L2 walk), admitted, admitted at the limit
    else:
        trees = stumps + [ts.chain(int(rng.choice([10, 11, 12, 33, 40])), str(rng.choice(ts.SIDES)), pick)] + stumps[:2]
    return trees, draw_weights(rng, len(trees))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    rng = np.random.default_rng(args.seed)
    t0 = time.time()
    bad = 0
    paths = collections.Counter()
    for it in range(args.iters):
        wide = WIDE[(it // 3) % len(WIDE)] if it % 3 == 1 else None
        X, y, qid = make_matrix(rng, wide)
        g, c = fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)
        for j in range(3):
            trees, weights = make_forest(rng, X, SHAPE_KINDS[it % len(SHAPE_KINDS)] if j == 1 else None, it // len(SHAPE_KINDS))
            # a wide matrix's last forest skips the threshold-rank walk (which does not depend on d): the LDS walk's
            # 128- and 64-document shapes at d = 200 and 320, the L2 walk over rows in global memory at d = 700
            if wide is not None and j == 2:
                os.environ["FR_TREE_RANK"] = "0"
            else:
                os.environ.pop("FR_TREE_RANK", None)
            if len(trees) == 1 and rng.random() < 0.5:  # a bare tree (its output is the leaf itself)
                model = fr.CModel.from_dict({"DecisionTree": trees[0]})
                exp = c.score_ensemble(trees, [1.0])
            else:
                model = fr.CModel.from_dict({"Ensemble": {"weights": weights, "models": [{"DecisionTree": t} for t in trees]}})
                exp = c.score_ensemble(trees, weights)
            got = native.predict_scores_dense(model, g)
            plan = native.last_tree_plan()
            paths[plan["path"] + {"rank": "", "lds": "_%dx%d" % (plan.get("docs", 0), plan.get("parts", 0)),
                                  "l2": "_rows_in_lds" if plan.get("rows_in_lds") else "_rows_in_hbm"}[plan["path"]]] += 1
            same = np.array_equal(got, exp, equal_nan=True)
            if not same:
                bad += 1
                print("MISMATCH iter", it, "n,d", X.shape, "trees", len(trees), "max |diff|", np.nanmax(np.abs(got - exp)), "plan", plan, flush=True)
    print("fuzz_trees: %d datasets x 3 forests, %d mismatches, paths %s, %.0f s" % (args.iters, bad, dict(sorted(paths.items())), time.time() - t0))
    print(json.dumps({"iters": args.iters, "forests": 3 * args.iters, "mismatches": bad, "paths": dict(sorted(paths.items())), "seconds": round(time.time() - t0, 1)}))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
