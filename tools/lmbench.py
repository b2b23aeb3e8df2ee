"""lmbench.py -- LambdaMART training time on an MSLR-WEB30K-shaped matrix (bench.py's generator), one JSON line.

    python tools/lmbench.py --shape 30k --trees 100            # the device: seconds per tree and the per-stage split
    python tools/lmbench.py --shape 30k --trees 100 --grower histogram   # the histogram grower
    python tools/lmbench.py --shape 30k --trees 100 --grower histogram --query-sampling-rate 0.5 --feature-sampling-rate 0.5 --seed 1
                                                               # per-tree samples of the queries and the features
    python tools/lmbench.py --shape 30k --trees 100 --grower histogram --validation-rate 0.1 --early-stopping-rounds 10
                                                               # a held-out tenth of the queries, stop 10 trees after its best
    python tools/lmbench.py --shape 30k --cpu-baseline 0.01    # the numpy restatement (tests/lambdamart_model.py) timed on
                                                               # a query sample, scaled to the full shape (labelled as such)
    python tools/lmbench.py --shape 30k --trees 100 --grower histogram --split-gain newton --lambda-l2 1
                                                               # the second-order split gain with an L2 term
    python tools/lmbench.py --shape 30k --trees 100 --grower histogram --max-leaves 32 --max-depth 32
                                                               # leaf-wise growth under a leaf budget (reports the trees' shape)
    python tools/lmbench.py --shape 30k --trees 100 --grower histogram --truncation-level 30 --lambda-norm
                                                               # the objective's truncation level and per-query normalisation
    python tools/lmbench.py --shape 30k --trees 100 --grower histogram --objective map --validation-rate 0.1
                                                               # gradients for MAP ("mrr": for MRR); reports the held-out AP and RR
    python tools/lmbench.py --shape 30k --trees 100 --grower histogram --objective xendcg --validation-rate 0.1 --held-out-measures
                                                               # the listwise objective; the held-out NDCG next to AP and RR
    python tools/lmbench.py --shape 30k --trees 100 --grower histogram --split-gain newton --monotone 8
                                                               # monotone constraints on the first 8 features, signs +1, -1, +1, ...
    python tools/lmbench.py --shape 30k --trees 100 --grower histogram --split-gain newton --goss-top-rate 0.2 --goss-other-rate 0.1
                                                               # gradient-based one-side sampling (reports goss_ms and the lists' sizes)
    python tools/lmbench.py --shape 30k --trees 100 --grower histogram --split-gain newton --grad-quant-bits 4
                                                               # quantised gradients: 4 bits per gradient (reports quant_ms)
    python tools/lmbench.py --shape 30k --trees 100 --grower histogram --symmetric --validation-rate 0.1
                                                               # symmetric trees (reports the levels that split per tree)
    python tools/lmbench.py --shape 30k --trees 100 --grower histogram --valid-dataset-rate 0.1
                                                               # a second generated dataset of a tenth of the queries as the validation
                                                               # dataset (reports valid_ms per tree)
    python tools/lmbench.py --shape 30k --trees 50 --grower histogram --init-trees 50
                                                               # 50 trees first, then --trees more from that model (reports the
                                                               # one-off cost of forming the initial scores)
Every other parameter is the LambdaMART default (TrainRequest.lambdamart()).
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


def device_run(args, X, y, qid):
    import fastrank_amd as fr
    from fastrank_amd import native

    t0 = time.perf_counter()
    ds = fr.CDataset.from_numpy(X, y, qid)
    req = fr.TrainRequest.lambdamart()
    req.measure = args.measure
    req.params.num_trees = args.trees
    req.params.quiet = True
    req.params.grower = args.grower
    req.params.query_sampling_rate = args.query_sampling_rate
    req.params.feature_sampling_rate = args.feature_sampling_rate
    req.params.seed = args.seed
    if args.validation_rate > 0:
        from fastrank_amd.training import hold_out_queries

        req.params.validation_queries = hold_out_queries(ds.queries(), args.validation_rate, args.seed)
    req.params.early_stopping_rounds = args.early_stopping_rounds
    req.params.split_gain = args.split_gain
    req.params.lambda_l2, req.params.min_sum_hessian, req.params.min_split_gain = args.lambda_l2, args.min_sum_hessian, args.min_split_gain
    if args.max_leaves:
        req.params.max_leaves = args.max_leaves
    if args.max_depth:
        req.params.max_depth = args.max_depth
    req.params.truncation_level, req.params.lambda_norm = args.truncation_level, args.lambda_norm
    req.params.objective = args.objective
    req.params.drop_rate = args.drop_rate
    if args.drop_rate > 0:  # (the two other keys need a drop rate)
        req.params.max_drop, req.params.skip_drop = args.max_drop, args.skip_drop
    if args.goss_top_rate > 0:  # (the other rate needs a top rate)
        req.params.goss_top_rate, req.params.goss_other_rate = args.goss_top_rate, args.goss_other_rate
    if args.symmetric:
        req.params.symmetric_trees = True
    req.params.lambda_l1, req.params.max_delta_step, req.params.path_smooth = args.lambda_l1, args.max_delta_step, args.path_smooth
    req.params.grad_quant_bits = args.grad_quant_bits
    if args.monotone:  # the first N features of the dataset, alternating signs from +1
        names = ds.feature_index_to_name()
        first = sorted(names)[:args.monotone]
        req.params.monotone_constraints = {names[f]: (1 if i % 2 == 0 else -1) for i, f in enumerate(first)}
    # upload and first touch of the device (not part of training)
    native.device_info(ds)
    t_ds = time.perf_counter() - t0
    extra, valid_info, init_info = {}, None, None
    if args.valid_dataset_rate > 0:  # a second dataset of its own: that share of the shape's queries and documents, another seed
        n, d, q, gen_seed = SHAPES[args.shape]
        Xv, yv, qv = gen_mslr_shaped(gen_seed + 1, max(1, int(n * args.valid_dataset_rate)), d, max(1, int(q * args.valid_dataset_rate)))
        tv = time.perf_counter()
        extra["valid"] = fr.CDataset.from_numpy(Xv, yv, qv)
        native.device_info(extra["valid"])
        valid_info = {"n": int(Xv.shape[0]), "queries": int(len(np.unique(qv))), "dataset_seconds": time.perf_counter() - tv}
    if args.init_trees > 0:  # the model the timed training continues from (its own training is timed, kernels unprofiled)
        first = req.clone()
        first.params.num_trees = args.init_trees
        ti = time.perf_counter()
        extra["init_model"] = ds.train_model(first, **extra)
        init_info = {"init_train_seconds": time.perf_counter() - ti}
    if args.warmup_trees > 0:  # an untimed training first: the device, its allocations and the bins are warm afterwards
        warm = req.clone()
        warm.params.num_trees = args.warmup_trees
        ds.train_model(warm, **extra)
    native.profile_enable(not args.no_kernel_profile)
    native.profile_reset()
    t1 = time.perf_counter()
    model = ds.train_model(req, **extra) if extra else ds.train_model(req)
    wall = time.perf_counter() - t1
    st = native.last_train_stats()["lambdamart"]
    prof = native.profile_stats()
    native.profile_enable(False)
    T = st["trees"]
    sample = {k: st[k] for k in ("sample_queries", "sample_instances", "sample_features") if k in st}
    out = {
        "metric": "LambdaMART seconds per tree (device) on MSLR-WEB30K shape" if args.shape == "30k" else "LambdaMART seconds per tree (device)",
        "shape": args.shape, "n": int(X.shape[0]), "d": int(X.shape[1]), "queries": int(len(np.unique(qid))),
        "measure": args.measure, "trees": T, "params": {k: v for k, v in req.params.to_dict().items() if k != "validation_queries"},
        "dataset_seconds": t_ds, "train_seconds": wall, "seconds_per_tree": wall / T,
        "grower": st["grower"], "bins_ms": st["bins_ms"],
        "per_tree_ms": {k: st[k + "_ms"] / T for k in ("gradient", "grow", "leaves", "update")},
        "train_measure_first": st["train_measure"][0], "train_measure_last": st["train_measure"][-1],
        "kernel_profile": {k: v for k, v in prof.items() if "lambda" in k or "rf_" in k or "tree" in k or "hist_" in k or "dart_" in k or "goss_" in k},
        "model_nodes": len(json.dumps(model.to_dict())),
    }
    if sample:  # (only when a rate is below 1, like the stats object)
        out["sample"] = sample
    if valid_info is not None:  # (only with a validation dataset, like the stats object)
        out["valid_dataset"] = dict(valid_info, valid_ms_per_tree=st["valid_ms"] / T, update_ms_per_tree=st["update_ms"] / T,
                                    **{k: st[k] for k in ("valid_dataset_queries", "valid_dataset_instances", "best_iteration",
                                                          "best_valid_measure", "stopped_early", "early_stopping_rounds", "valid_measure")})
    if init_info is not None:  # (only with an init model, like the stats object)
        out["init_model"] = dict(init_info, **{k: st[k] for k in ("init_trees", "init_train_measure", "init_valid_measure", "init_ms") if k in st})
        out["model_trees"] = len(model.to_dict()["Ensemble"]["models"])
    if "validation_queries" in st:  # (only with held-out queries, like the stats object)
        out["validation"] = {k: st[k] for k in ("validation_queries", "training_queries", "best_iteration", "best_valid_measure",
                                                "stopped_early", "early_stopping_rounds", "valid_measure", "train_measure")}
        out["model_trees"] = len(model.to_dict()["Ensemble"]["models"])
    if args.max_leaves:  # (only under leaf-wise growth, like the stats object)
        def depth(node):
            return 1 if "LeafNode" in node else 1 + max(depth(node["FeatureSplit"]["lhs"]), depth(node["FeatureSplit"]["rhs"]))

        depths = [depth(m["DecisionTree"]) for m in model.to_dict()["Ensemble"]["models"]]
        out["leafwise"] = {"max_leaves": st["max_leaves"], "mean_leaves": st["mean_leaves"], "mean_depth": float(np.mean(depths)),
                           "max_depth": int(np.max(depths)), "pool_bytes": st["pool_bytes"]}
    if args.truncation_level or args.lambda_norm:  # (only when set, like the stats object)
        out["objective"] = {k: st[k] for k in ("truncation_level", "lambda_norm") if k in st}
    if args.objective != "ndcg":
        out.setdefault("objective", {})["objective"] = st["objective"]
    if args.drop_rate > 0:  # (only under DART, like the stats object)
        out["dart"] = {"drop_rate": st["drop_rate"], "max_drop": st["max_drop"], "skip_drop": st["skip_drop"], "dropped": st["dropped"],
                       "dart_ms": st["dart_ms"], "dart_ms_per_tree": st["dart_ms"] / T, "dart_cache_bytes": st["dart_cache_bytes"],
                       "weights_min": float(np.min(model.to_dict()["Ensemble"]["weights"])),
                       "weights_max": float(np.max(model.to_dict()["Ensemble"]["weights"]))}
        # the same re-forming by re-traversal: the finished model scored by score_trees (scores left on the device), three times
        native.profile_enable(True)
        native.profile_reset()
        walls = []
        for _ in range(3):
            tw = time.perf_counter()
            native.predict_scores_dense(model, ds, n_total=0)
            walls.append((time.perf_counter() - tw) * 1e3)
        out["dart"]["retraverse_wall_ms"] = walls
        out["dart"]["retraverse_kernels"] = {k: v for k, v in native.profile_stats().items() if "tree" in k}
        native.profile_enable(False)
    if args.monotone:  # (only with the key, like the stats object)
        out["monotone"] = {"features": len(st["monotone_constraints"]), "clamped_leaves_per_tree": float(np.mean(st["monotone_clamped_leaves"])),
                           "clamped_leaves_max": int(np.max(st["monotone_clamped_leaves"]))}
    if args.goss_top_rate > 0:  # (only under GOSS, like the stats object)
        out["goss"] = {"goss_top_rate": st["goss_top_rate"], "goss_other_rate": st["goss_other_rate"], "goss_ms_per_tree": st["goss_ms"] / T,
                       "instances_mean": float(np.mean(st["goss_instances"])), "instances_min": int(np.min(st["goss_instances"])),
                       "instances_max": int(np.max(st["goss_instances"])), "top": int(st["goss_top"][0])}
    if args.symmetric:  # (only with the key, like the stats object)
        out["symmetric"] = {"levels_mean": float(np.mean(st["levels"])), "levels_min": int(np.min(st["levels"])),
                            "levels_max": int(np.max(st["levels"]))}
    if args.grad_quant_bits:  # (only with the key, like the stats object)
        out["grad_quant"] = {"grad_quant_bits": st["grad_quant_bits"], "quant_ms_per_tree": st["quant_ms"] / T}
    if args.lambda_l1 or args.max_delta_step or args.path_smooth:  # (only with a key, like the stats object)
        out["leaf_regularisation"] = {k: st[k] for k in ("lambda_l1", "max_delta_step", "path_smooth")}
    if args.held_out_measures and args.validation_rate > 0:  # AP / RR / NDCG of the model over the held-out queries
        held = set(req.params.validation_queries)
        out["held_out"] = {}
        for name in ("ap", "rr", "ndcg"):
            by_q = ds.evaluate(model, name)
            out["held_out"][name] = float(np.mean([v for q, v in sorted(by_q.items()) if q in held]))
    return out


def cpu_run(args, X, y, qid):
    from oracle import pyoracle as o
    from tests import lambdamart_model as lm

    rng = np.random.default_rng(1)
    uq = np.unique(qid)
    keep = rng.choice(uq, size=max(1, int(round(len(uq) * args.cpu_baseline))), replace=False)
    rows = np.isin(qid, keep)
    Xs, ys, qs = np.ascontiguousarray(X[rows]), np.ascontiguousarray(y[rows]), np.ascontiguousarray(qid[rows])
    c = o.Dataset(Xs, ys, qs)
    queries = lm.query_lists(c)
    order_ids = np.concatenate(queries)
    norms = c.default_norms(args.measure)
    s = np.zeros(len(ys))
    t0 = time.perf_counter()
    lam, wt = lm.gradients(s, ys, queries, norms, lm.depth_of(args.measure), 1.0)
    t1 = time.perf_counter()
    lm.fit_tree(Xs, lam, wt, order_ids, range(Xs.shape[1]), 6, 10, 64)
    t2 = time.perf_counter()
    scale = X.shape[0] / Xs.shape[0]
    return {
        "metric": "LambdaMART seconds per tree, CPU restatement (numpy, one thread), SCALED from a %g query sample" % args.cpu_baseline,
        "shape": args.shape, "sample_rows": int(Xs.shape[0]), "sample_queries": int(len(keep)),
        "sample_gradient_seconds": t1 - t0, "sample_fit_seconds": t2 - t1,
        "scaled_seconds_per_tree": (t2 - t0) * scale, "scale": scale,
        "note": "linear scaling by rows; not a measurement of the full shape",
    }


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="30k", choices=sorted(SHAPES))
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--measure", default="ndcg")
    ap.add_argument("--grower", default="exact", choices=["exact", "histogram"])
    ap.add_argument("--query-sampling-rate", type=float, default=1.0, help="share of the queries every tree is fitted to")
    ap.add_argument("--feature-sampling-rate", type=float, default=1.0, help="share of the features every tree may split on")
    ap.add_argument("--seed", type=int, default=0, help="master seed of the per-tree samples")
    ap.add_argument("--validation-rate", type=float, default=0.0, help="share of the queries held out (hold_out_queries under --seed; 0: none)")
    ap.add_argument("--valid-dataset-rate", type=float, default=0.0,
                    help="a second generated dataset of this share of the shape's queries as the validation dataset (0: none)")
    ap.add_argument("--init-trees", type=int, default=0, help="train this many trees first, then continue from them with --trees new ones (0: from nothing)")
    ap.add_argument("--early-stopping-rounds", type=int, default=0, help="stop this many trees after the held-out measure's best (0: never)")
    ap.add_argument("--split-gain", default="variance", choices=["variance", "newton"], help="the split criterion (newton: histogram grower only)")
    ap.add_argument("--lambda-l2", type=float, default=0.0, help="L2 term of the Newton gain and leaves")
    ap.add_argument("--min-sum-hessian", type=float, default=0.0, help="least hessian mass of a child under the Newton gain")
    ap.add_argument("--min-split-gain", type=float, default=0.0, help="gain a split must exceed under the Newton gain")
    ap.add_argument("--max-leaves", type=int, default=0, help="leaf budget of leaf-wise growth (histogram grower only; 0: level-wise)")
    ap.add_argument("--max-depth", type=int, default=0, help="max_depth of the request (0: the default)")
    ap.add_argument("--truncation-level", type=int, default=0, help="a pair counts only when its better ranked document is in the top T (0: every pair)")
    ap.add_argument("--lambda-norm", action="store_true", help="scale every query's gradients by log2(1 + S_q) / S_q")
    ap.add_argument("--objective", default="ndcg", choices=["ndcg", "map", "mrr", "xendcg"], help="what the gradients optimise (the measure stays an NDCG spelling)")
    ap.add_argument("--drop-rate", type=float, default=0.0, help="DART: the chance of every earlier tree to be dropped before a tree is fitted (0: plain boosting)")
    ap.add_argument("--max-drop", type=int, default=50, help="DART: the most trees one step drops (0: no cap)")
    ap.add_argument("--skip-drop", type=float, default=0.5, help="DART: the chance of a step to drop nothing")
    ap.add_argument("--monotone", type=int, default=0, help="monotone constraints on the first N features, signs alternating from +1 (needs --split-gain newton)")
    ap.add_argument("--goss-top-rate", type=float, default=0.0, help="GOSS: the share of a tree's documents kept for their |gradient| (0: off; needs --split-gain newton)")
    ap.add_argument("--goss-other-rate", type=float, default=0.1, help="GOSS: the share of a tree's documents drawn from the others")
    ap.add_argument("--grad-quant-bits", type=int, default=0, help="quantised gradients: bits per gradient, 2..8 (0: off; needs --split-gain newton)")
    ap.add_argument("--symmetric", action="store_true", help="symmetric trees: every node of a level splits on one candidate (histogram grower, level-wise)")
    ap.add_argument("--lambda-l1", type=float, default=0.0, help="leaf regularisation: soft threshold of a node's gradient sum (needs --split-gain newton)")
    ap.add_argument("--max-delta-step", type=float, default=0.0, help="leaf regularisation: cap of an output's magnitude (0: none; needs --split-gain newton)")
    ap.add_argument("--path-smooth", type=float, default=0.0, help="leaf regularisation: pull of a child's output toward its parent's (0: none; needs --split-gain newton)")
    ap.add_argument("--held-out-measures", action="store_true", help="with --validation-rate: report the model's mean AP, RR and NDCG over the held-out queries")
    ap.add_argument("--warmup-trees", type=int, default=0, help="train this many trees untimed before the measured training")
    ap.add_argument("--no-kernel-profile", action="store_true", help="leave the library's per-kernel event timing off during the timed training")
    ap.add_argument("--cpu-baseline", type=float, default=0.0, help="query fraction for the CPU restatement (0: device run)")
    return ap


def main():
    args = parser().parse_args()
    n, d, q, seed = SHAPES[args.shape]
    X, y, qid = gen_mslr_shaped(seed, n, d, q)
    out = cpu_run(args, X, y, qid) if args.cpu_baseline > 0 else device_run(args, X, y, qid)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
