#!/usr/bin/env python3
"""Randomised soak of LambdaMART TRAINING, both growers: random small datasets built on
fuzz_parity.make_case -- 1..40 features (7, 8, 9, 16, 17 often: the histogram kernel's blocks of 8), constant columns, -0.0,
denormals and +-3e38, columns of a few distinct values, the rows of a query scattered through the input, label sets
{0..4}, {0, 0.5, 1, 2}, {0, 1, 30} and now and then -1, query- / feature- / doubly sampled views, now and then a ranksvm
file with sparse rows (absent values) -- and random parameters: 1..6 trees, depth 1..12, min_leaf_support from 1 to beyond
n, split_candidates 2..256 (1 and 300 for the exact grower), sigma and learning_rate over a few decades, ndcg / ndcg@k.
Features stay finite (NaN has its own test).

Per case, stage by stage: the device's gradients of the prefix model against the restatement's (exact zeros, rtol 1e-12,
per-query sum ~ 0); tree t bit-equal to the restatement's fit from the DEVICE's gradients; bins bit-equal; ensemble
weights; train_measure[t] = the oracle evaluator's mean of the prefix prediction; the final prediction = the oracle's
score_ensemble; a second run gives the same JSON.  The library's evaluator error (actual above ideal DCG, with negative
gains) is a mismatch unless the oracle's evaluator reports an error for the same running scores: "both_error", at most
10 % of a run.  Any other error, from the device or from a restatement, is a mismatch that ENDS the run: nothing more is
started on a device that may have faulted.
--objective: every case also draws a truncation level (0, 1, 2, 5, 30) and lambda_norm ("Truncation
and normalisation") from a generator of its own, so the cases themselves are those of a run without the flag; gradients
are then held to tests/lambdamart_trunc_model.py (under lambda_norm at the tolerance derived in
tests/test_gpu_lambdamart_trunc.py).
--rank-objective map | mrr | mixed (off by default; `--objective` was taken by the options above): every case trains with
that `objective` key ("mixed": drawn per case from ndcg, map, mrr) and is held to tests/lambdamart_objective_model.py; the
measure every stage reports is then AP / RR ("Objectives").
--dry: no device; the restatement trains each generated case on the CPU, and the share of cases on which the oracle's
evaluator reports an error -- at zero scores or after any tree -- is printed.
Usage: python tools/fuzz_lambdamart.py --iters 300 [--seed 0]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from fuzz_parity import make_case  # noqa: E402
from oracle import pyoracle as o  # noqa: E402
from tests import lambdamart_hist_model as hm  # noqa: E402
from tests import lambdamart_model as lm  # noqa: E402
from tests import lambdamart_objective_model as om  # noqa: E402
from tests import lambdamart_trunc_model as tm  # noqa: E402
from tests.conftest import ranksvm_presence  # noqa: E402

LABEL_SETS = [[0.0, 0.0, 1.0, 2.0, 3.0, 4.0], [0.0, 0.0, 0.5, 1.0, 2.0], [0.0, 0.0, 1.0, 30.0]]
EVALUATOR_ERROR = "actual DCG exceeds ideal DCG"  # (csrc/host.hpp, check_flags)
SPECIALS = np.float32([0.0, -0.0, 1e-45, -1e-45, 1e-39, 1.0, -1.0, 3e38, -3e38])


def make_column(rng, n, plain):
    kind = int(rng.integers(0, 8))
    if kind == 0:
        col = rng.uniform(0, 1, n)
    elif kind == 1:
        col = np.floor(rng.exponential(2.0, n))
    elif kind == 2:
        col = rng.lognormal(0, 2, n) * rng.choice([-1, 1], n)
    elif kind == 3:
        col = np.where(rng.random(n) < 0.7, rng.choice([0.0, -0.0]), rng.uniform(0, 1, n))
    elif kind == 4:
        col = np.full(n, float(rng.choice([0.0, 2.5, -7.0])))                    # a constant column
    elif kind == 5:
        col = rng.choice(rng.normal(0, 3, int(rng.integers(2, 9))), n)            # at most k distinct values
    elif kind == 6 and not plain:
        col = rng.choice(SPECIALS, n).astype(np.float64)                          # -0.0, denormals, +-3e38
    else:
        col = rng.integers(-2, 3, n).astype(float)
    if plain:  # values a text file carries exactly
        col = np.round(col * 8.0) / 8.0
    return col.astype(np.float32)


def make_lm_case(rng):
    """(X, y, qid, measure, params, from_file)."""
    _, _, qid, _, _ = make_case(rng)
    negative = bool(rng.random() < 0.15)  # (make_case's rate for labels below zero)
    p = dict(grower=str(rng.choice(["exact", "histogram"])), num_trees=int(rng.integers(1, 7)),
             max_depth=int(rng.integers(1, 13)), sigma=float(10.0 ** rng.uniform(-1.5, 1.0)),
             learning_rate=float(10.0 ** rng.uniform(-2.0, 0.5)))
    d = int(rng.choice([7, 8, 9, 16, 17])) if rng.random() < 0.5 else int(rng.integers(1, 41))
    # the python restatement is the slow side: about 15 us per (instance, feature, level, tree)
    n_cap = int(np.clip(200000 // (d * p["max_depth"] * p["num_trees"]), 20, 1200))
    qid = qid[: max(1, min(len(qid), int(rng.integers(1, n_cap + 1))))]
    n = len(qid)
    if rng.random() < 0.6:  # the rows of a query scattered through the input
        qid = qid[rng.permutation(n)]
    from_file = bool(rng.random() < 0.12)
    X = np.stack([make_column(rng, n, from_file) for _ in range(d)], axis=1)
    if rng.random() < 0.4 and n > 2:  # duplicated documents: exact score ties
        k = int(rng.integers(1, max(2, n // 3)))
        src, dst = rng.integers(0, n, k), rng.integers(0, n, k)
        X[dst] = X[src]
    labels = list(LABEL_SETS[int(rng.integers(0, len(LABEL_SETS)))]) + ([-1.0] if negative else [])
    y = rng.choice(labels, n)
    if rng.random() < 0.2:
        y[qid == qid[0]] = 0.0
    longest = int(np.bincount(qid).max())
    measure = "ndcg" if rng.random() < 0.4 else "ndcg@%d" % int(rng.choice([1, 2, 3, 5, 10, 20, longest, longest + 7]))
    p["min_leaf_support"] = int(rng.choice([1, 1, 2, 5, 10, max(1, n // 3), n, n + 5]))
    ks = [2, 3, 7, 16, 64, 255, 256] + ([1, 300] if p["grower"] == "exact" else [])
    p["split_candidates"] = int(rng.choice(ks))
    return X, y, qid, measure, p, from_file


def write_ranksvm(rng, path, X, y, qid):
    """Writes the rows with features 1..d (column 0 of the returned matrix is never listed); about a third of the rows are
    sparse: most of their values are dropped (they read 0.0) and only the non-zero ones are listed."""
    n, d = X.shape
    full = np.zeros((n, d + 1), dtype=np.float32)
    full[:, 1:] = X
    with open(path, "w") as fh:
        for i in range(n):
            sparse = rng.random() < 0.35
            if sparse:
                full[i, 1:][rng.random(d) < 0.7] = 0.0
            cols = [j for j in range(1, d + 1) if not sparse or full[i, j] != 0.0]
            cols = cols or [1]  # (a row that lists no feature is a parse error)
            fh.write("%s qid:%d %s # doc%d\n" % (repr(float(y[i])), int(qid[i]), " ".join("%d:%s" % (j, repr(float(full[i, j]))) for j in cols), i))
    return full


RANK_OBJECTIVE, RANK_RNG = "ndcg", None  # --rank-objective, and the generator "mixed" draws from


def draw_objective(rng):
    """The objective's keys for a case (none without --objective / --rank-objective)."""
    out = {}
    if RANK_OBJECTIVE != "ndcg":
        name = RANK_OBJECTIVE
        if name == "mixed":
            name = str(RANK_RNG.choice(["ndcg", "map", "mrr"]))
        if name != "ndcg":
            out["objective"] = name
    if rng is None:
        return out
    out.update(truncation_level=int(rng.choice([0, 1, 2, 5, 30])), lambda_norm=bool(rng.random() < 0.5))
    return out


def training_measure(measure, p):
    """The measure the trainer reports: the objective's under map / mrr, else the request's."""
    return {"map": "ap", "mrr": "rr"}.get(p.get("objective", "ndcg"), measure)


def expected_gradients(s, y, queries, norms, depth, p):
    """(lambda, w, per-query rtol) of the restatement for the case's parameters."""
    T, norm = p.get("truncation_level", 0), p.get("lambda_norm", False)
    if p.get("objective", "ndcg") != "ndcg":
        elam, ewt, _, S, _ = om.gradients(s, y, queries, norms, p["objective"], p["sigma"], T, norm, parts=True)
        rtol = np.full(len(queries), 1e-12)
        if norm:
            live = S > 0.0
            rtol[live] = 3e-12 + 2.0 ** -52 / np.log1p(S[live]) + 12.0 * 2.0 ** -53
        return elam, ewt, rtol
    if not T and not norm:
        elam, ewt = lm.gradients(s, y, queries, norms, depth, p["sigma"])
        return elam, ewt, np.full(len(queries), 1e-12)
    elam, ewt, _, S, _ = tm.gradients(s, y, queries, norms, depth, p["sigma"], T, norm, parts=True)
    rtol = np.full(len(queries), 1e-12)
    if norm:
        live = S > 0.0
        rtol[live] = 3e-12 + 2.0 ** -52 / np.log1p(S[live]) + 12.0 * 2.0 ** -53
    return elam, ewt, rtol


def request(fr, measure, p, num_trees=None):
    req = fr.TrainRequest.lambdamart()
    req.measure = measure
    req.params.quiet = True
    for k, v in p.items():
        setattr(req.params, k, v)
    if num_trees is not None:
        req.params.num_trees = num_trees
    return req


class EvaluatorError(Exception):
    """The library refused a training run because some query's DCG exceeds its ideal DCG."""


class Case:
    """One generated case on the device: the view `g`, and the rows / matrix / oracle dataset the restatement works on
    (instance ids renumbered 0.. over the view's rows, ascending)."""

    def __init__(self, fr, native, rng, tmp, objective_rng=None):
        self.fr, self.native = fr, native
        X, y, qid, self.measure, self.p, self.from_file = make_lm_case(rng)
        self.p.update(draw_objective(objective_rng))
        self.present, self.views = None, 0
        if self.from_file:
            path = os.path.join(tmp, "case.train")
            X = write_ranksvm(rng, path, X, y, qid)
            g = fr.CDataset.open_ranksvm(path)
            self.present = ranksvm_presence(path, X.shape[1])
            feats = sorted(g.feature_ids())
        else:
            g = fr.CDataset.from_numpy(X, y, qid)
            feats = list(range(X.shape[1]))
        self.n_total = len(y)
        rows = np.arange(len(y))
        if rng.random() < 0.3 and len(np.unique(qid)) > 2:
            keep = rng.choice(np.unique(qid), size=max(1, len(np.unique(qid)) // 2), replace=False)
            g = g.subsample_queries([str(int(q)) for q in keep])
            rows = np.flatnonzero(np.isin(qid, keep))
            self.views += 1
        if rng.random() < 0.3 and len(feats) > 2:
            feats = sorted(int(f) for f in rng.choice(feats, size=max(1, len(feats) // 2), replace=False))
            names = g.feature_index_to_name()
            g = g.subsample_feature_names([names[f] for f in feats])
            self.views += 1
        self.g, self.rows, self.feats = g, rows, feats
        self.X, self.y = np.ascontiguousarray(X[rows]), np.ascontiguousarray(y[rows])
        if self.present is not None:
            self.present = self.present[rows]
        self.c = o.Dataset(self.X, self.y, np.ascontiguousarray(qid[rows]))
        self.queries = lm.query_lists(self.c)
        self.order_ids = np.concatenate(self.queries)
        self.reported = training_measure(self.measure, self.p)
        self.norms = self.c.default_norms(self.reported)

    def train(self, req):
        try:
            return self.g.train_model(req)
        except Exception as exc:
            if EVALUATOR_ERROR in str(exc):
                raise EvaluatorError(str(exc)) from None
            raise

    def prefix(self, trees, t):
        return self.fr.CModel.from_dict({"Ensemble": {"weights": [self.p["learning_rate"]] * t,
                                                      "models": [{"DecisionTree": x} for x in trees[:t]]}})

    def fit(self, lam, wt, binned):
        p = self.p
        if p["grower"] == "histogram":
            return hm.fit_tree(self.X, lam, wt, self.order_ids, self.feats, p["max_depth"], p["min_leaf_support"], p["split_candidates"], binned)
        return lm.fit_tree(self.X, lam, wt, self.order_ids, self.feats, p["max_depth"], p["min_leaf_support"], p["split_candidates"],
                           self.present)

    def device_gradients(self, model):
        lam, wt = self.native.lambda_gradients(model, self.g, self.measure, self.p["sigma"], n_total=self.n_total,
                                               truncation_level=self.p.get("truncation_level", 0), lambda_norm=self.p.get("lambda_norm", False),
                                               objective=self.p.get("objective", "ndcg"))
        return lam[self.rows], wt[self.rows]

    def scores(self, model):
        return self.native.predict_scores_dense(model, self.g, n_total=self.n_total)[self.rows]

    def check(self):
        """None when every stage agrees, else what differs first."""
        p, native = self.p, self.native
        T = p["num_trees"]
        req = request(self.fr, self.measure, p)
        model = self.train(req)
        st = native.last_train_stats()["lambdamart"]
        d = model.to_dict()
        trees = [m["DecisionTree"] for m in d["Ensemble"]["models"]]
        if d["Ensemble"]["weights"] != [p["learning_rate"]] * T or len(trees) != T:
            return "ensemble weights"
        binned = None
        if p["grower"] == "histogram":
            ids, fids, edges, bins = native.hist_bins(self.g, p["split_candidates"])
            binned = hm.bin_matrix(self.X, self.order_ids, self.feats, p["split_candidates"])
            if not np.array_equal(ids, self.rows[self.order_ids]) or list(fids) != self.feats:
                return "instance or feature list of the bins"
            if any(a.tobytes() != b.tobytes() for a, b in zip(edges, binned[0])) or not np.array_equal(bins, binned[1]):
                return "bins"
        depth = lm.depth_of(self.measure)
        for t in range(T + 1):
            prefix = self.prefix(trees, t)
            s = self.scores(prefix)
            if t > 0:
                per_q, err = self.c.metric_from_scores(self.reported, s, self.norms)
                if err != 0 or st["train_measure"][t - 1] != o.mean(per_q):
                    return "train_measure[%d]" % (t - 1)
            if t == T:
                break
            lam, wt = self.device_gradients(prefix)
            if not (np.all(np.isfinite(lam)) and np.all(np.isfinite(wt))):
                return "non-finite gradient before tree %d" % t
            elam, ewt, rtol_q = expected_gradients(s, self.y, self.queries, self.norms, depth, p)
            rtol = np.empty(len(s))
            for q, ids in enumerate(self.queries):
                rtol[ids] = rtol_q[q]
            for name, got, exp in (("lambda", lam, elam), ("w", wt, ewt)):
                zero = exp == 0.0
                if not np.array_equal(got[zero], exp[zero]) or not np.all(np.abs(got - exp) <= rtol * np.abs(exp)):
                    return "%s before tree %d" % (name, t)
            for ids in self.queries:
                if not abs(lam[ids].sum()) <= 1e-9 * max(1.0, np.abs(lam[ids]).sum()):
                    return "sum of lambda over a query before tree %d" % t
            if trees[t] != self.fit(lam, wt, binned):
                return "tree %d" % t
        if not np.array_equal(s, self.c.score_ensemble(trees, d["Ensemble"]["weights"])):
            return "final prediction"
        if json.dumps(self.train(req).to_dict()) != json.dumps(d):
            return "second run differs"
        self.split_nodes = json.dumps(d).count("FeatureSplit")
        return None

    def oracle_errors_too(self):
        """After the library's evaluator error: train one tree fewer until it works, then the restatement's next tree from the device's
        gradients; does the oracle's evaluator report an error for those running scores?"""
        trees = []
        for T in range(self.p["num_trees"] - 1, 0, -1):
            try:
                trees = [m["DecisionTree"] for m in self.train(request(self.fr, self.measure, self.p, T)).to_dict()["Ensemble"]["models"]]
                break
            except EvaluatorError:
                continue
        binned = hm.bin_matrix(self.X, self.order_ids, self.feats, self.p["split_candidates"]) if self.p["grower"] == "histogram" else None
        lam, wt = self.device_gradients(self.prefix(trees, len(trees)))
        trees = trees + [self.fit(lam, wt, binned)]
        s = self.c.score_ensemble(trees, [self.p["learning_rate"]] * len(trees))
        return self.c.metric_from_scores(self.measure, s, self.norms)[1] != 0


def dry_case(rng, objective_rng=None):
    """Does the oracle's evaluator report an error while the restatement trains the case (no views, no file)?"""
    X, y, qid, measure, p, _ = make_lm_case(rng)
    p.update(draw_objective(objective_rng))
    c = o.Dataset(X, y, qid)
    queries = lm.query_lists(c)
    reported = training_measure(measure, p)
    order_ids, norms, feats = np.concatenate(queries), c.default_norms(reported), list(range(X.shape[1]))
    binned = hm.bin_matrix(X, order_ids, feats, p["split_candidates"]) if p["grower"] == "histogram" else None
    s = np.zeros(len(y))
    for t in range(p["num_trees"] + 1):
        if c.metric_from_scores(reported, s, norms)[1] != 0:
            return True
        if t == p["num_trees"]:
            break
        lam, wt, _ = expected_gradients(s, y, queries, norms, lm.depth_of(measure), p)
        args = (X, lam, wt, order_ids, feats, p["max_depth"], p["min_leaf_support"], p["split_candidates"])
        tree = hm.fit_tree(*args, binned) if p["grower"] == "histogram" else lm.fit_tree(*args)
        s = s + p["learning_rate"] * lm.tree_scores(tree, X)
    return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dry", action="store_true", help="no device: the oracle evaluator's error rate while the restatement trains")
    ap.add_argument("--objective", action="store_true", help="draw a truncation level and lambda_norm for every case")
    ap.add_argument("--rank-objective", default="ndcg", choices=["ndcg", "map", "mrr", "mixed"], help="the `objective` key of every case (mixed: drawn per case)")
    args = ap.parse_args()
    global RANK_OBJECTIVE, RANK_RNG
    RANK_OBJECTIVE, RANK_RNG = args.rank_objective, np.random.default_rng([args.seed, 2])
    rng = np.random.default_rng(args.seed)
    objective_rng = np.random.default_rng([args.seed, 1]) if args.objective else None
    o.set_mean_segment(o.DEVICE_MEAN_SEGMENT)
    t0 = time.time()
    if args.dry:
        errs = sum(dry_case(rng, objective_rng) for _ in range(args.iters))
        print(json.dumps({"iters": args.iters, "dry": True, "oracle_error_while_training": int(errs), "seconds": round(time.time() - t0, 1)}))
        return 0 if errs * 10 <= args.iters else 1
    import fastrank_amd as fr
    from fastrank_amd import native
    bad = errs = nodes = views = files = 0
    growers, ended = {}, None
    with tempfile.TemporaryDirectory() as tmp:
        for it in range(args.iters):
            case = Case(fr, native, rng, tmp, objective_rng)
            growers[case.p["grower"]] = growers.get(case.p["grower"], 0) + 1
            views += case.views
            files += case.from_file
            what = None
            try:
                try:
                    what = case.check()
                except EvaluatorError as exc:
                    if case.oracle_errors_too():
                        errs += 1
                        continue
                    what = "device error, none from the oracle: %s" % str(exc)[:160]
            except Exception as exc:  # not the evaluator's: the device may have faulted, so nothing more is started
                what, ended = "error that ends the run: %s: %s" % (type(exc).__name__, str(exc)[:200]), it
            if what is None:
                nodes += case.split_nodes
                continue
            bad += 1
            print("MISMATCH iter", it, what, json.dumps({"n": len(case.y), "d": case.X.shape[1], "feats": len(case.feats), "measure": case.measure,
                                                        "views": case.views, "file": case.from_file, "params": case.p}), flush=True)
            if ended is not None:
                break
    if errs * 10 > args.iters:
        print("too many cases where device and oracle both report an error: %d of %d" % (errs, args.iters))
    print(json.dumps({"iters": args.iters, "mismatches": bad, "both_error": errs, "split_nodes": nodes, "growers": growers,
                      "sampled_views": views, "file_loaded": int(files), "ended_at_iter": ended, "seconds": round(time.time() - t0, 1)}))
    return 1 if bad or errs * 10 > args.iters else 0


if __name__ == "__main__":
    sys.exit(main())
