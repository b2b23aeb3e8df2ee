"""permimpbench.py -- permutation importance at the 30K shape, all 136 features, R = 5, both scopes, for

    linear      the coordinate-ascent model under ndcg@10
    lambdamart  a 100-tree LambdaMART model (histogram grower) under ndcg@10
    forest      the 500 random trees of bench.py's config 5 under ndcg

Per model and scope, --runs alternating rounds of fr_permutation_importance (values only, nothing per query downloaded): the
wall time of the whole call and its stats (scoring, metric pass, upload of the sources, the host's sort of the stream).  The
yardstick is fr_evaluate_dense of the same model on the same dataset in the same rounds: `ratio` = the call's wall time over
F * R such calls (below 1: cheaper than doing it by hand even if the hand-made datasets cost nothing to build and upload).
--tiles repeats the dataset-scope calls on a dataset built without the column-major copy (FR_XCOL=0): the gather's share.

    python tools/permimpbench.py --tiles --out profiles/permimp_30k_bench.json

One JSON line (and the file).
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

from bench import SHAPES, gen_mslr_shaped, random_trees  # noqa: E402

STAT_KEYS = ("gather", "rows", "chunks", "slots", "score_ms", "metric_ms", "upload_ms", "baseline_ms", "sources_ms", "launches")


def spread(vals):
    return {"min": min(vals), "median": float(np.median(vals)), "max": max(vals)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="30k", choices=sorted(SHAPES))
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--eval-calls", type=int, default=5, help="fr_evaluate_dense calls timed per model and round")
    ap.add_argument("--models", default="linear,lambdamart,forest")
    ap.add_argument("--tiles", action="store_true", help="also time the dataset-scope calls on a dataset without the column-major copy")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import fastrank_amd as fr
    from fastrank_amd import native

    n, d, q, seed = SHAPES[args.shape]
    X, y, qid = gen_mslr_shaped(seed, n, d, q)
    ds = fr.CDataset.from_numpy(X, y, qid)
    native.device_info(ds)
    wanted = args.models.split(",")
    models, train_s = {}, {}
    if "linear" in wanted:
        req = fr.TrainRequest.coordinate_ascent()
        req.measure = "ndcg@10"
        req.params.quiet, req.params.seed = True, 42
        t = time.perf_counter()
        models["linear"] = (ds.train_model(req), "ndcg@10")
        train_s["linear"] = time.perf_counter() - t
    if "lambdamart" in wanted:
        req = fr.TrainRequest.lambdamart()
        req.measure = "ndcg@10"
        req.params.quiet, req.params.grower, req.params.num_trees = True, "histogram", 100
        t = time.perf_counter()
        models["lambdamart"] = (ds.train_model(req), "ndcg@10")
        train_s["lambdamart"] = time.perf_counter() - t
    if "forest" in wanted:
        trees = random_trees(np.random.default_rng(7), X, 500, 8)
        models["forest"] = (fr.CModel.from_dict({"Ensemble": {"weights": [1.0] * len(trees), "models": [{"DecisionTree": t} for t in trees]}}), "ndcg")
    datasets = {"xcol": ds}
    if args.tiles:
        os.environ["FR_XCOL"] = "0"
        try:
            datasets["tiles"] = fr.CDataset.from_numpy(X, y, qid)
            native.device_info(datasets["tiles"])
        finally:
            os.environ.pop("FR_XCOL", None)

    def call(model, dataset, evaluator, scope):
        t = time.perf_counter()
        rep, values, _ = native.permutation_importance_dense(model, dataset, evaluator, repeats=args.repeats, seed=1, scope=scope, per_query=False)
        out = {k: rep["stats"][k] for k in STAT_KEYS}
        out["wall_ms"] = (time.perf_counter() - t) * 1e3
        out["skipped"] = len(rep["skipped"])
        return out, values, rep

    def evaluate_ms(model, dataset, evaluator):
        native.evaluate_dense(model, dataset, evaluator)
        t = time.perf_counter()
        for _ in range(args.eval_calls):
            native.evaluate_dense(model, dataset, evaluator)
        return (time.perf_counter() - t) * 1e3 / args.eval_calls

    cases = [(name, gather, scope) for name in models for gather in datasets for scope in (("dataset", "query") if gather == "xcol" else ("dataset",))]
    runs = {"%s/%s/%s" % c: [] for c in cases}
    evals = {"%s/%s" % (name, gather): [] for name in models for gather in datasets}
    first = {}
    for name, (model, evaluator) in models.items():  # (pays the first launches' set-up, outside the rounds)
        out, values, rep = call(model, ds, evaluator, "dataset")
        first[name] = dict(out, baseline=rep["baseline"], top5=[[rep["names"][k], rep["importance"][k], rep["std"][k]]
                                                              for k in np.argsort(-np.asarray(rep["importance"]), kind="stable")[:5]])
        if "tiles" in datasets:  # the two gathers give the same bytes
            _, values_t, _ = call(model, datasets["tiles"], evaluator, "dataset")
            first[name]["tiles_same_bytes"] = bool(np.array_equal(values.view(np.uint64), values_t.view(np.uint64)))
    for _ in range(args.runs):
        for name, gather, scope in cases:
            model, evaluator = models[name]
            runs["%s/%s/%s" % (name, gather, scope)].append(call(model, datasets[gather], evaluator, scope)[0])
        for name, (model, evaluator) in models.items():
            for gather in datasets:
                evals["%s/%s" % (name, gather)].append(evaluate_ms(model, datasets[gather], evaluator))
    F = d
    summary = {}
    for name, gather, scope in cases:
        rs, ev = runs["%s/%s/%s" % (name, gather, scope)], evals["%s/%s" % (name, gather)]
        launched = F - rs[0]["skipped"]
        summary["%s/%s/%s" % (name, gather, scope)] = {
            "wall_ms": spread([r["wall_ms"] for r in rs]), "score_ms": spread([r["score_ms"] for r in rs]), "metric_ms": spread([r["metric_ms"] for r in rs]),
            "upload_ms": spread([r["upload_ms"] for r in rs]), "sources_ms": spread([r["sources_ms"] for r in rs]), "evaluate_dense_ms": spread(ev),
            "features_launched": launched,
            # the worst case for the call: its slowest run over the yardstick's fastest
            "ratio_to_F_R_evaluations": spread([r["wall_ms"] / (F * args.repeats * e) for r in rs for e in ev]),
            "ratio_to_launched_R_evaluations": spread([r["wall_ms"] / (max(1, launched) * args.repeats * e) for r in rs for e in ev]),
        }
    out = {"metric": "permutation importance on MSLR-WEB30K shape" if args.shape == "30k" else "permutation importance", "shape": args.shape, "n": int(n),
           "d": int(d), "queries": int(q), "repeats": args.repeats, "features": F, "train_seconds": train_s, "first_call": first, "runs": runs,
           "evaluate_dense_ms": evals, "summary": summary}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
