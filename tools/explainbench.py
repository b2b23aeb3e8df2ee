"""explainbench.py -- model explanation on an MSLR-WEB30K-shaped matrix (bench.py's generator): a
default histogram-grower LambdaMART model is trained, then timed three times each

    feature_importance over every document        (explain_kernel + the |phi| reduction, tile by tile; nothing downloaded)
    explain on a view of every hundredth query    (kernel time and download apart)
    the cover pass alone                          (the background routed through every tree, integer atomics)

    python tools/explainbench.py --shape 30k --trees 100 --out profiles/explain_30k_bench.json

One JSON line (and the file): milliseconds per run, (document, leaf-path) items per second, the kernel's f64 operations per
second by the model's own count of them.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bench import SHAPES, gen_mslr_shaped  # noqa: E402


def path_lengths(tree, seen=()):
    """distinct features on every root-to-leaf path, depth first"""
    if "LeafNode" in tree:
        return [len(seen)]
    s = tree["FeatureSplit"]
    here = seen if s["fid"] in seen else seen + (s["fid"],)
    return path_lengths(s["lhs"], here) + path_lengths(s["rhs"], here)


def f64_ops_per_document(lengths):
    """f64 operations explain_kernel spends on one document: per leaf of m elements, m EXTENDs over the other m - 1 (step l
    has l inner iterations of 5 operations), m - 1 additions for the sum and 4 operations for the contribution"""
    total = 0
    for m in lengths:
        total += m * (5 * (m - 1) * m // 2 + m + 4)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="30k", choices=sorted(SHAPES))
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--view-step", type=int, default=100, help="explain a view of every N-th query")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import fastrank_amd as fr
    from fastrank_amd import native

    n, d, q, seed = SHAPES[args.shape]
    X, y, qid = gen_mslr_shaped(seed, n, d, q)
    ds = fr.CDataset.from_numpy(X, y, qid)
    req = fr.TrainRequest.lambdamart()
    req.measure = "ndcg"
    req.params.quiet, req.params.grower, req.params.num_trees = True, "histogram", args.trees
    t0 = time.perf_counter()
    model = ds.train_model(req)
    train_s = time.perf_counter() - t0
    trees = [m["DecisionTree"] for m in model.to_dict()["Ensemble"]["models"]]
    lengths = [m for t in trees for m in path_lengths(t)]
    ops = f64_ops_per_document(lengths)

    def timed(fn):
        t = time.perf_counter()
        rep = fn()
        return rep, (time.perf_counter() - t) * 1e3

    importance, covers = [], []
    for _ in range(args.runs):
        (_, _, rep), wall = timed(lambda: native.feature_importance(model, ds))
        importance.append({"wall_ms": wall, "kernel_ms": rep["kernel_ms"], "cover_ms": rep["cover_ms"],
                           "items_per_s": rep["documents"] * rep["leaf_paths"] / (rep["kernel_ms"] * 1e-3),
                           "f64_ops_per_s": rep["documents"] * ops / (rep["kernel_ms"] * 1e-3)})
        covers.append(rep["cover_ms"])
    queries = sorted(ds.queries(), key=int)[::args.view_step]
    view = ds.subsample_queries(queries)
    native.device_info(view)
    explain = []
    for _ in range(args.runs):
        ex, wall = timed(lambda: native.explain_dense(model, view, n_total=n))
        rep = ex.status
        explain.append({"wall_ms": wall, "kernel_ms": rep["kernel_ms"], "download_ms": rep["copy_ms"], "cover_ms": rep["cover_ms"],
                        "documents": rep["documents"], "items_per_s": rep["documents"] * rep["leaf_paths"] / (rep["kernel_ms"] * 1e-3)})
    out = {
        "metric": "model explanation (exact TreeSHAP) on MSLR-WEB30K shape" if args.shape == "30k" else "model explanation (exact TreeSHAP)",
        "shape": args.shape, "n": int(n), "d": int(d), "queries": int(q), "trees": len(trees), "leaf_paths": len(lengths),
        "mean_path": float(np.mean(lengths)), "max_path": int(np.max(lengths)), "f64_ops_per_document": int(ops), "train_seconds": train_s,
        "feature_importance": importance, "explain_view": explain, "cover_pass_ms": covers,
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
