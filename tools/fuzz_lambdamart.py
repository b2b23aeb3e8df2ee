#!/usr/bin/env python3
"""Randomised soak of LambdaMART TRAINING, both growers: random small datasets built on
fuzz_parity.make_case -- 1..40 features (7, 8, 9, 16, 17 often: the histogram kernel's blocks of 8), constant columns, -0.0,
denormals and +-3e38, columns of a few distinct values, the rows of a query scattered through the input, label sets
{0..4}, {0, 0.5, 1, 2}, {0, 1, 30} and now and then -1, query- / feature- / doubly sampled views, now and then a ranksvm
file with sparse rows (absent values) -- and random parameters: 1..6 trees, depth 1..12, min_leaf_support from 1 to beyond
n, split_candidates 2..256 (1 and 300 for the exact grower), sigma and learning_rate over a few decades, ndcg / ndcg@k.
Features stay finite (NaN has its own test).

Per case, stage by stage, against tests/lambdamart_composed_model.py (which only dispatches to the restatements of the
single features): the stats echo the request (a feature's keys are present exactly when it is set); bins bit-equal; the
query names and every tree's sample; the device's gradients of the prefix model against the restatement's (exact zeros, rtol
1e-12, per-query sum ~ 0) and, where a tree's query list is not the whole view, the same launched over that list (inside
it the full launch's bytes, outside it NaN); tree t bit-equal to the restatement's fit, on the tree's sample, from the
DEVICE's gradients; ensemble weights; train_measure[t] / valid_measure[t] = the oracle evaluator's (subset) means of the
prefix prediction; best_iteration, best_valid_measure, stopped_early and the number of trees follow the stopping rule, and
under early_stopping_rounds the returned model is, byte for byte, the first best_iteration trees of a run without the rule;
the final prediction = the oracle's score_ensemble; a second run gives the same JSON.  The library's evaluator error
(actual above ideal DCG, with negative gains) is a mismatch unless the oracle's evaluator reports an error for the same
running scores: "both_error", at most 10 % of a run.  Any other error, from the device or from a restatement, is a mismatch
that ENDS the run: nothing more is started on a device that may have faulted.
--objective: every case also draws a truncation level (0, 1, 2, 5, 30) and lambda_norm ("Truncation
and normalisation") from a generator of its own, so the cases themselves are those of a run without the flag; gradients
are then held to tests/lambdamart_trunc_model.py (under lambda_norm at the tolerance derived in
tests/test_gpu_lambdamart_trunc.py).
--rank-objective map | mrr | mixed (off by default; `--objective` was taken by the options above): every case trains with
that `objective` key ("mixed": drawn per case from ndcg, map, mrr) and is held to tests/lambdamart_objective_model.py; the
measure every stage reports is then AP / RR ("Objectives").
--compose: every case also draws, from a third generator of its own (datasets and base parameters stay those of a run
without the flag): query_sampling_rate and feature_sampling_rate from 1, 0.5, 0.25 and a rate that leaves a single entry,
with a seed; for about half the cases validation_queries (one name up to all but one query of the view) with
early_stopping_rounds 0, 1 or 2; and for the histogram grower split_gain "newton" with lambda_l2, min_sum_hessian and
min_split_gain (0, the feature tests' values, one that refuses the root, and now and then a floor exactly on the edge of
its comparison: the hessian sum of the left side of the first tree's root split, or that split's gain) and max_leaves 2, 3, 5, 12, 31 or 255 (then
now and then a max_depth up to 32).  The three flags combine freely.
--symmetric (off by default): about half of the histogram-grower cases without a leaf budget also set symmetric_trees
("Symmetric trees"), drawn from a fourth generator of its own, so the committed seeds' cases do not
move; their trees are held to tests/lambdamart_symmetric_model.py on the tree's sample, under either gain, and the stats must
carry `symmetric_trees` and one `levels` entry per tree.  The closing line counts them as "symmetric".
The closing JSON line counts, per key, the cases that DREW it (set it away from its default) and those in which it BOUND
(tests/lambdamart_composed_model.py says what that means), both from the restatement's side.
--dry: no device; the composed restatement trains each generated case (views and files included) on the CPU, and the share
of cases on which the oracle's evaluator reports an error -- at zero scores or after any tree -- is printed with the same
drawn and bound counts.
Usage: python tools/fuzz_lambdamart.py --iters 300 [--seed 0] [--objective] [--rank-objective mixed] [--compose] [--symmetric] [--dry]"""
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
from tests import lambdamart_composed_model as cm  # noqa: E402
from tests import lambdamart_leafwise_model as lw  # noqa: E402
from tests import lambdamart_sample_model as sm  # noqa: E402
from tests import lambdamart_symmetric_model as sy  # noqa: E402
from tests.conftest import ranksvm_presence  # noqa: E402
from tests.lambdamart_composed_model import expected_gradients, training_measure  # noqa: E402,F401

LABEL_SETS = [[0.0, 0.0, 1.0, 2.0, 3.0, 4.0], [0.0, 0.0, 0.5, 1.0, 2.0], [0.0, 0.0, 1.0, 30.0]]
EVALUATOR_ERROR = "actual DCG exceeds ideal DCG"  # (csrc/host.hpp, check_flags)
SPECIALS = np.float32([0.0, -0.0, 1e-45, -1e-45, 1e-39, 1.0, -1.0, 3e38, -3e38])
SINGLE = 1e-9  # a sampling rate at which lambdamart_sample_model.count gives 1


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


def draw_compose(rng, p, names):
    """--compose: the sampling, validation, Newton and leaf-budget keys of a case (only those away from their defaults, so
    the request carries a key exactly when it is set); names: the view's queries."""
    out = {}
    for key in ("query_sampling_rate", "feature_sampling_rate"):
        rate = float(rng.choice([1.0, 0.5, 0.25, SINGLE], p=[0.4, 0.3, 0.2, 0.1]))
        if rate < 1.0:
            out[key] = rate
    out["seed"] = int(rng.integers(0, 2 ** 62))
    if rng.random() < 0.5 and len(names) >= 2:
        held = int(rng.integers(1, len(names)))  # from a single name to all but one training query
        out["validation_queries"] = [names[i] for i in rng.permutation(len(names))[:held]]
        rounds = int(rng.choice([0, 1, 2]))
        if rounds:
            out["early_stopping_rounds"] = rounds
    if p["grower"] != "histogram":
        return out
    if rng.random() < 0.6:  # the values of tests/test_gpu_lambdamart_newton.py and test_lambdamart_newton_host.py, 0, and one that refuses the root
        out["split_gain"] = "newton"
        for key, values in (("lambda_l2", [0.0, 2.0 ** -10, 0.5, 1.0]), ("min_sum_hessian", [0.0, 0.0, 2.0 ** -6, 0.25, 1e30]),
                            ("min_split_gain", [0.0, 2.0 ** -20, 1e-6, 1e30])):
            v = float(rng.choice(values))
            if v != 0.0:
                out[key] = v
    if rng.random() < 0.5:
        out["max_leaves"] = int(rng.choice([2, 3, 5, 12, 31, 255]))
        if rng.random() < 0.5:  # (a leaf budget bounds the work, whatever the depth)
            out["max_depth"] = int(rng.integers(1, 33))
    return out


def request(fr, measure, p, num_trees=None):
    req = fr.TrainRequest.lambdamart()
    req.measure = measure
    req.params.quiet = True
    for k, v in p.items():
        setattr(req.params, k, v)
    if num_trees is not None:
        req.params.num_trees = num_trees
    return req


class SymmetricComposed(cm.Composed):
    """The composed restatement of a case that sets symmetric_trees: only the tree changes."""

    def tree(self, lam, wt, fsel, qsel, **override):
        p = dict(self.p, **override)
        rows = sm.instance_rows(self.queries, qsel)
        return sy.tree_on_sample(self.X, lam, wt, self.order_ids, self.feats, self.binned, rows, fsel, p["max_depth"], p["min_leaf_support"],
                                 p["split_candidates"], split_gain=p["split_gain"], **{k: p[k] for k in cm.NEWTON_NUMBERS})


def composed(p):
    return SymmetricComposed if p.get("symmetric_trees") else cm.Composed


class EvaluatorError(Exception):
    """The library refused a training run because some query's DCG exceeds its ideal DCG."""


class CaseData:
    """One generated case, host side only: the input (matrix or ranksvm file), the view as row and feature lists, and the
    rows / matrix / oracle dataset / composed restatement the checks work on (instance ids renumbered 0.. over the view's
    rows, ascending)."""

    def __init__(self, rng, tmp, objective_rng=None, compose_rng=None, symmetric_rng=None):
        X, y, qid, self.measure, self.p, self.from_file = make_lm_case(rng)
        self.p.update(draw_objective(objective_rng))
        self.present, self.views, self.path = None, 0, None
        if self.from_file:
            self.path = os.path.join(tmp, "case.train")
            X = write_ranksvm(rng, self.path, X, y, qid)
            self.present = ranksvm_presence(self.path, X.shape[1])
            feats = [int(f) for f in np.flatnonzero(self.present.any(axis=0))]  # (the features some row holds)
        else:
            feats = list(range(X.shape[1]))
        self.input = (X, y, qid)
        self.all_feats = list(feats)
        self.n_total = len(y)
        rows = np.arange(len(y))
        self.keep_queries = self.keep_feats = None
        if rng.random() < 0.3 and len(np.unique(qid)) > 2:
            keep = rng.choice(np.unique(qid), size=max(1, len(np.unique(qid)) // 2), replace=False)
            self.keep_queries = [str(int(q)) for q in keep]
            rows = np.flatnonzero(np.isin(qid, keep))
            self.views += 1
        if rng.random() < 0.3 and len(feats) > 2:
            feats = sorted(int(f) for f in rng.choice(feats, size=max(1, len(feats) // 2), replace=False))
            self.keep_feats = feats
            self.views += 1
        self.rows, self.feats = rows, feats
        self.X, self.y = np.ascontiguousarray(X[rows]), np.ascontiguousarray(y[rows])
        if self.present is not None:
            self.present = self.present[rows]
        self.c = o.Dataset(self.X, self.y, np.ascontiguousarray(qid[rows]))
        self.names = cm._names(qid[rows])
        if compose_rng is not None:
            self.p.update(draw_compose(compose_rng, self.p, self.names))
        if symmetric_rng is not None and symmetric_rng.random() < 0.5 and self.p["grower"] == "histogram" and not self.p.get("max_leaves"):
            self.p["symmetric_trees"] = True
        self.model = composed(self.p)(self.X, self.y, self.c, self.measure, self.p, self.feats, self.present, self.names)
        if compose_rng is not None and self.p.get("split_gain") == "newton" and compose_rng.random() < 0.75:
            # a floor exactly on the edge of its comparison: the hessian sum of the left side of the first tree's root split
            # (still admitted), or that split's gain (refused)
            edge = self.model.first_root()
            key = str(compose_rng.choice(["min_sum_hessian", "min_split_gain"]))
            value = None if edge is None else edge[key == "min_split_gain"]
            if value is not None and np.isfinite(value) and value > 0.0:
                self.p[key] = value
                self.model = composed(self.p)(self.X, self.y, self.c, self.measure, self.p, self.feats, self.present, self.names, self.model.binned)
        self.queries, self.order_ids = self.model.queries, self.model.order_ids
        self.reported, self.norms = self.model.reported, self.model.norms

    def drawn(self):
        """The optional keys the case sets away from their defaults."""
        return [k for k, v in cm.DEFAULTS.items() if k in self.p and self.p[k] != v]

    def describe(self):
        return {"n": len(self.y), "d": self.X.shape[1], "feats": len(self.feats), "queries": len(self.queries), "measure": self.measure,
                "views": self.views, "file": self.from_file, "params": self.p}


class Case(CaseData):
    """The case on the device: the view `g`."""

    def __init__(self, fr, native, rng, tmp, objective_rng=None, compose_rng=None, symmetric_rng=None):
        CaseData.__init__(self, rng, tmp, objective_rng, compose_rng, symmetric_rng)
        self.fr, self.native = fr, native
        X, y, qid = self.input
        g = fr.CDataset.open_ranksvm(self.path) if self.from_file else fr.CDataset.from_numpy(X, y, qid)
        self.loaded_feats = sorted(int(f) for f in g.feature_ids())
        if self.keep_queries is not None:
            g = g.subsample_queries(self.keep_queries)
        if self.keep_feats is not None:
            names = g.feature_index_to_name()
            g = g.subsample_feature_names([names[f] for f in self.keep_feats])
        self.g = g

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

    def device_gradients(self, model, queries=None):
        lam, wt = self.native.lambda_gradients(model, self.g, self.measure, self.p["sigma"], n_total=self.n_total, queries=queries,
                                               truncation_level=self.p.get("truncation_level", 0), lambda_norm=self.p.get("lambda_norm", False),
                                               objective=self.p.get("objective", "ndcg"))
        return lam[self.rows], wt[self.rows]

    def scores(self, model):
        return self.native.predict_scores_dense(model, self.g, n_total=self.n_total)[self.rows]

    def check_stats(self, st):
        """The stats echo the request: a feature's keys are present exactly when it is set."""
        exp = self.model.expected_stats()
        if set(st) & cm.OPTIONAL_STATS != set(exp):
            return "stats keys: %s" % sorted((set(st) & cm.OPTIONAL_STATS) ^ set(exp))
        if st["grower"] != self.p["grower"] or any(v is not None and st[k] != v for k, v in exp.items()):
            return "stats do not echo the request"
        if ("symmetric_trees" in st or "levels" in st) != bool(self.p.get("symmetric_trees")):
            return "stats keys: symmetric_trees / levels"
        if self.p.get("symmetric_trees") and (st["symmetric_trees"] is not True or len(st["levels"]) != st["trees"]):
            return "stats do not echo symmetric_trees"
        return None

    def check(self):
        """None when every stage agrees, else what differs first."""
        p, native, model = self.p, self.native, self.model
        if self.loaded_feats != self.all_feats:
            return "feature ids of the loaded dataset"
        T = p["num_trees"]
        req = request(self.fr, self.measure, p)
        dev = self.train(req)
        st = native.last_train_stats()["lambdamart"]
        d = dev.to_dict()
        got = [m["DecisionTree"] for m in d["Ensemble"]["models"]]
        what = self.check_stats(st)
        if what:
            return what
        held, rounds, trained = len(model.H) > 0, model.p["early_stopping_rounds"], st["trees"]
        if d["Ensemble"]["weights"] != [p["learning_rate"]] * len(got) or len(st["train_measure"]) != trained or not 1 <= trained <= T:
            return "ensemble weights"
        trees = got
        if held and rounds > 0:  # the trees the stats speak of: those of a run without the rule
            free = {k: v for k, v in p.items() if k != "early_stopping_rounds"}
            trees = [m["DecisionTree"] for m in self.train(request(self.fr, self.measure, free, trained)).to_dict()["Ensemble"]["models"]]
            if len(trees) != trained or json.dumps(got) != json.dumps(trees[:st["best_iteration"]]):
                return "early stopping: the model is not the first best_iteration trees of the run without the rule"
        elif len(got) != T or trained != T:
            return "ensemble weights"
        if native.evaluate_dense(self.prefix(trees, 0), self.g, "mrr")[0] != self.names:
            return "query names"
        if p["grower"] == "histogram":
            ids, fids, edges, bins = native.hist_bins(self.g, p["split_candidates"])
            binned = model.binned
            if not np.array_equal(ids, self.rows[self.order_ids]) or list(fids) != self.feats:
                return "instance or feature list of the bins"
            if any(a.tobytes() != b.tobytes() for a, b in zip(edges, binned[0])) or not np.array_equal(bins, binned[1]):
                return "bins"
        nq_t = nf_t = ni_t = leaves = 0
        for t in range(trained + 1):
            prefix = self.prefix(trees, t)
            s = self.scores(prefix)
            if t > 0:
                tr, va, err = model.measures(s)
                if err != 0 or st["train_measure"][t - 1] != tr:
                    return "train_measure[%d]" % (t - 1)
                if held and st["valid_measure"][t - 1] != va:
                    return "valid_measure[%d]" % (t - 1)
            if t == trained:
                break
            fsel, qsel = model.sample(t)
            hf, hq = native.lambdamart_sample(self.g, req.params, t)
            if not np.array_equal(hf, np.asarray(self.feats)[fsel]) or not np.array_equal(hq, qsel):
                return "sample of tree %d" % t
            nq_t, nf_t, ni_t = nq_t + len(qsel), nf_t + len(fsel), ni_t + sum(len(self.queries[q]) for q in qsel)
            lam, wt = self.device_gradients(prefix)
            if not (np.all(np.isfinite(lam)) and np.all(np.isfinite(wt))):
                return "non-finite gradient before tree %d" % t
            elam, ewt, rtol_q = model.gradients(s)
            rtol = np.empty(len(s))
            for q, ids in enumerate(self.queries):
                rtol[ids] = rtol_q[q]
            for name, have, exp in (("lambda", lam, elam), ("w", wt, ewt)):
                zero = exp == 0.0
                if not np.array_equal(have[zero], exp[zero]) or not np.all(np.abs(have - exp) <= rtol * np.abs(exp)):
                    return "%s before tree %d" % (name, t)
            for ids in self.queries:
                if not abs(lam[ids].sum()) <= 1e-9 * max(1.0, np.abs(lam[ids]).sum()):
                    return "sum of lambda over a query before tree %d" % t
            if model.subset(qsel):  # as the trainer launches it: over the tree's query list
                lam_s, wt_s = self.device_gradients(prefix, queries=qsel)
                inside = np.zeros(len(s), dtype=bool)
                inside[np.concatenate([self.queries[q] for q in qsel])] = True
                if lam_s[inside].tobytes() != lam[inside].tobytes() or wt_s[inside].tobytes() != wt[inside].tobytes():
                    return "gradients over the query list of tree %d differ from the full launch's" % t
                if not (np.all(np.isnan(lam_s[~inside])) and np.all(np.isnan(wt_s[~inside]))):
                    return "gradients over the query list of tree %d touch other queries" % t
            if trees[t] != model.tree(lam, wt, fsel, qsel):
                return "tree %d" % t
            leaves += lw.n_leaves(trees[t])
            model.observe(s, lam, wt, fsel, qsel, trees[t])
        if "sample_queries" in st and (st["sample_queries"], st["sample_features"], st["sample_instances"]) != (nq_t / trained, nf_t / trained, ni_t / trained):
            return "mean sample sizes"
        if "mean_leaves" in st and st["mean_leaves"] != leaves / trained:
            return "mean_leaves"
        if held:
            best, n_trained, stopped, kept = model.stopping(st["valid_measure"])
            if (st["best_iteration"], trained, st["stopped_early"], len(got)) != (best, n_trained, stopped, kept):
                return "early stopping: best_iteration, trees or stopped_early"
            if len(st["valid_measure"]) != trained or st["best_valid_measure"] != st["valid_measure"][best - 1]:
                return "best_valid_measure"
            model.bound["early_stopping_rounds"] = bool(stopped)
        if not np.array_equal(self.scores(dev), self.c.score_ensemble(got, d["Ensemble"]["weights"])):
            return "final prediction"
        if json.dumps(self.train(req).to_dict()) != json.dumps(d):
            return "second run differs"
        self.split_nodes = json.dumps(d).count("FeatureSplit")
        return None

    def oracle_errors_too(self):
        """After the library's evaluator error: train one tree fewer (without the stopping rule) until it works, then the
        restatement's next tree from the device's gradients; does the oracle's evaluator report an error for those running scores?"""
        trees = []
        free = {k: v for k, v in self.p.items() if k != "early_stopping_rounds"}
        for T in range(self.p["num_trees"] - 1, 0, -1):
            try:
                trees = [m["DecisionTree"] for m in self.train(request(self.fr, self.measure, free, T)).to_dict()["Ensemble"]["models"]]
                break
            except EvaluatorError:
                continue
        lam, wt = self.device_gradients(self.prefix(trees, len(trees)))
        trees = trees + [self.model.tree(lam, wt, *self.model.sample(len(trees)))]
        s = self.c.score_ensemble(trees, [self.p["learning_rate"]] * len(trees))
        return self.c.metric_from_scores(self.reported, s, self.norms)[1] != 0


class Counts:
    """How often each optional key was drawn and how often it bound."""

    def __init__(self, compose, objective, rank_objective):
        keys = []
        if objective:
            keys += ["truncation_level", "lambda_norm"]
        if rank_objective != "ndcg":
            keys += ["objective"]
        if compose:
            keys += ["max_leaves", "min_sum_hessian", "min_split_gain", "early_stopping_rounds", "query_sampling_rate"]
        self.drawn, self.bound = {}, {k: 0 for k in cm.BOUND_KEYS if k in keys}

    def add(self, case):
        for k in case.drawn():
            self.drawn[k] = self.drawn.get(k, 0) + 1
        for k in self.bound:
            self.bound[k] += bool(case.model.bound[k])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dry", action="store_true", help="no device: the oracle evaluator's error rate while the restatement trains")
    ap.add_argument("--objective", action="store_true", help="draw a truncation level and lambda_norm for every case")
    ap.add_argument("--rank-objective", default="ndcg", choices=["ndcg", "map", "mrr", "mixed"], help="the `objective` key of every case (mixed: drawn per case)")
    ap.add_argument("--compose", action="store_true", help="draw the sampling, validation, Newton and leaf-budget keys for every case")
    ap.add_argument("--symmetric", action="store_true", help="set symmetric_trees for about half of the histogram-grower cases without a leaf budget")
    args = ap.parse_args()
    global RANK_OBJECTIVE, RANK_RNG
    RANK_OBJECTIVE, RANK_RNG = args.rank_objective, np.random.default_rng([args.seed, 2])
    rng = np.random.default_rng(args.seed)
    objective_rng = np.random.default_rng([args.seed, 1]) if args.objective else None
    compose_rng = np.random.default_rng([args.seed, 3]) if args.compose else None
    symmetric_rng = np.random.default_rng([args.seed, 4]) if args.symmetric else None
    counts = Counts(args.compose, args.objective, args.rank_objective)
    o.set_mean_segment(o.DEVICE_MEAN_SEGMENT)
    t0 = time.time()
    growers, views, files, symmetric = {}, 0, 0, 0

    def tally(case):
        nonlocal views, files, symmetric
        symmetric += bool(case.p.get("symmetric_trees"))
        growers[case.p["grower"]] = growers.get(case.p["grower"], 0) + 1
        views += case.views
        files += case.from_file

    if args.dry:
        errs = 0
        with tempfile.TemporaryDirectory() as tmp:
            for _ in range(args.iters):
                case = CaseData(rng, tmp, objective_rng, compose_rng, symmetric_rng)
                tally(case)
                errs += case.model.train(observe=True)["oracle_error"]
                counts.add(case)
        print(json.dumps({"iters": args.iters, "dry": True, "oracle_error_while_training": int(errs), "growers": growers, "sampled_views": views,
                          "file_loaded": int(files), "drawn": counts.drawn, "bound": counts.bound, **({"symmetric": symmetric} if args.symmetric else {}),
                          "seconds": round(time.time() - t0, 1)}))
        return 0 if errs * 10 <= args.iters else 1
    import fastrank_amd as fr
    from fastrank_amd import native
    bad = errs = nodes = 0
    ended = None
    with tempfile.TemporaryDirectory() as tmp:
        for it in range(args.iters):
            case = Case(fr, native, rng, tmp, objective_rng, compose_rng, symmetric_rng)
            tally(case)
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
            counts.add(case)
            if what is None:
                nodes += case.split_nodes
                continue
            bad += 1
            print("MISMATCH iter", it, what, json.dumps(case.describe()), flush=True)
            if ended is not None:
                break
    if errs * 10 > args.iters:
        print("too many cases where device and oracle both report an error: %d of %d" % (errs, args.iters))
    print(json.dumps({"iters": args.iters, "mismatches": bad, "both_error": errs, "split_nodes": nodes, "growers": growers,
                      "sampled_views": views, "file_loaded": int(files), "drawn": counts.drawn, "bound": counts.bound, "ended_at_iter": ended,
                      **({"symmetric": symmetric} if args.symmetric else {}), "seconds": round(time.time() - t0, 1)}))
    return 1 if bad or errs * 10 > args.iters else 0


if __name__ == "__main__":
    sys.exit(main())
