"""Every LambdaMART training key at once ("Randomised soak"), for the tests: one place that turns a
full parameter dict into the expected stage results.  It holds no arithmetic of its own; it only dispatches to the
restatements of the single features:
  * samples: lambdamart_valid_model.split / .sample (the tree's features, and its queries drawn from the training queries);
  * gradients: lambdamart_model / lambdamart_trunc_model / lambdamart_objective_model (`expected_gradients`, with the
    per-query tolerance derived in tests/test_gpu_lambdamart_trunc.py);
  * the tree on the sampled rows: lambdamart_sample_model.tree_for (exact, with the present mask, and the plain histogram
    grower), lambdamart_newton_model.tree_on_sample (split_gain "newton"), lambdamart_leafwise_model.tree_on_sample (a leaf
    budget, under either gain);
  * measures: subset means of the oracle's per-query NDCG / AP / RR; stopping: lambdamart_valid_model.stopping.
`Composed` also notes, from the restatement's side alone, which keys BOUND in a case (`bound`):
  truncation_level       the truncated pair masses A differ from the untruncated ones for some query of a tree's list;
  lambda_norm            some query of a tree's list has S_q > 0;
  max_leaves             a tree reached the budget while a leaf was still open (or would have been, had the last split's
                         children been searched);
  min_sum_hessian /      the tree differs from the one fitted with that threshold at 0 (it refused a candidate or a split
  min_split_gain         that would otherwise have been taken);
  early_stopping_rounds  the rule ended training before num_trees;
  query_sampling_rate    some tree's query sample is a single query;
  objective              under map / mrr a training query has no relevant document.
"""
import numpy as np

from oracle import pyoracle as o
from tests import lambdamart_hist_model as hm
from tests import lambdamart_leafwise_model as lw
from tests import lambdamart_model as lm
from tests import lambdamart_newton_model as nm
from tests import lambdamart_objective_model as om
from tests import lambdamart_sample_model as sm
from tests import lambdamart_trunc_model as tm
from tests import lambdamart_valid_model as vm

NEWTON_NUMBERS = ("lambda_l2", "min_sum_hessian", "min_split_gain")
# the keys of the trainer's stats that are present exactly when the request sets their feature
SAMPLING_STATS = {"query_sampling_rate", "feature_sampling_rate", "seed", "sample_queries", "sample_instances", "sample_features"}
VALID_STATS = {"validation_queries", "training_queries", "valid_measure", "best_iteration", "best_valid_measure", "stopped_early",
               "early_stopping_rounds"}
NEWTON_STATS = {"split_gain"} | set(NEWTON_NUMBERS)
LEAFWISE_STATS = {"max_leaves", "mean_leaves", "pool_bytes"}
OPTIONAL_STATS = SAMPLING_STATS | VALID_STATS | NEWTON_STATS | LEAFWISE_STATS | {"bins", "truncation_level", "lambda_norm", "objective"}
BOUND_KEYS = ("truncation_level", "lambda_norm", "max_leaves", "min_sum_hessian", "min_split_gain", "early_stopping_rounds",
              "query_sampling_rate", "objective")
DEFAULTS = dict(query_sampling_rate=1.0, feature_sampling_rate=1.0, seed=0, validation_queries=[], early_stopping_rounds=0,
                split_gain="variance", lambda_l2=0.0, min_sum_hessian=0.0, min_split_gain=0.0, max_leaves=0, truncation_level=0,
                lambda_norm=False, objective="ndcg")

# the soaks of the suite (tests/test_gpu_lambdamart_compose.py on the device, tests/test_lambdamart_compose_host.py with --dry):
# (flags of tools/fuzz_lambdamart.py, seed, cases); the seeds were chosen with --dry so that every key binds
SOAKS = {"objective": (["--objective", "--rank-objective", "mixed"], 5, 30),
         "compose": (["--compose"], 7, 30),
         "compose_objective": (["--compose", "--objective", "--rank-objective", "mixed"], 7, 30)}


def soak_bound_keys(flags):
    """The keys whose bound count a run with these flags reports."""
    keys = ["truncation_level", "lambda_norm"] if "--objective" in flags else []
    keys += ["objective"] if "--rank-objective" in flags else []
    if "--compose" in flags:
        keys += ["max_leaves", "min_sum_hessian", "min_split_gain", "early_stopping_rounds", "query_sampling_rate"]
    return keys


# --- what the stage-by-stage GPU tests share -----------------------------------------------------

def _request(measure="ndcg", grower="histogram", **kw):
    import fastrank_amd as fr
    req = fr.TrainRequest.lambdamart()
    req.measure = measure
    req.params.quiet = True
    req.params.grower = grower
    for k, v in kw.items():
        setattr(req.params, k, v)
    return req


def _ensemble(trees, lr):
    import fastrank_amd as fr
    return fr.CModel.from_dict({"Ensemble": {"weights": [lr] * len(trees), "models": [{"DecisionTree": x} for x in trees]}})


def _names(qid):
    """The view's queries in its order (first appearance), as the dataset spells them."""
    _, first = np.unique(qid, return_index=True)
    return [str(int(qid[i])) for i in np.sort(first)]


# --- gradients -----------------------------------------------------------------------------------

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


def pair_mass(s, y, queries, norms, depth, p, truncation_level):
    """(A by instance id, S per query) of the restatement at the given truncation level (before any scaling)."""
    if p.get("objective", "ndcg") != "ndcg":
        _, _, A, S, _ = om.gradients(s, y, queries, norms, p["objective"], p["sigma"], truncation_level, False, parts=True)
    else:
        _, _, A, S, _ = tm.gradients(s, y, queries, norms, depth, p["sigma"], truncation_level, False, parts=True)
    return A, S


# --- the composed restatement --------------------------------------------------------------------

class Composed:
    """A case: the rows X / y of a view (instance ids 0..n-1), its oracle dataset `c`, the request's `measure` and the full
    parameter dict `p` (absent keys at their defaults), the view's feature ids `feats` (columns of X), the present mask of a
    file-loaded dataset, the view's query names in its order."""

    def __init__(self, X, y, c, measure, p, feats=None, present=None, names=None, binned=None):
        self.X, self.y, self.c, self.measure, self.present = X, y, c, measure, present
        self.p = dict(DEFAULTS, **p)
        p = self.p
        if p["grower"] != "histogram" and (p["split_gain"] != "variance" or p["max_leaves"]):
            raise ValueError("split_gain `newton` and max_leaves need the histogram grower")
        self.queries = lm.query_lists(c)
        self.order_ids = np.concatenate(self.queries)
        self.feats = sorted(range(X.shape[1]) if feats is None else feats)
        self.reported = training_measure(measure, p)
        self.norms = c.default_norms(self.reported)
        self.depth = lm.depth_of(measure)
        nq = len(self.queries)
        held = list(p["validation_queries"])
        if held:
            self.T, self.H = vm.split(names, held)
        else:
            self.T, self.H = np.arange(nq, dtype=np.int64), np.zeros(0, dtype=np.int64)
        if p["early_stopping_rounds"] > 0 and not len(self.H):
            raise ValueError("early_stopping_rounds needs a validation query")
        self.rates = (p["query_sampling_rate"], p["feature_sampling_rate"])
        self._binned = binned
        self.bound = {k: False for k in BOUND_KEYS}
        if p["objective"] != "ndcg":
            self.bound["objective"] = any(not np.any(np.asarray(y, dtype=np.float32)[self.queries[q]] > np.float32(0.0)) for q in self.T)

    # -- stages --

    @property
    def binned(self):
        """(edges, bins) of the FULL lists: every document of the view, held-out ones included."""
        if self._binned is None and self.p["grower"] == "histogram":
            self._binned = hm.bin_matrix(self.X, self.order_ids, self.feats, self.p["split_candidates"])
        return self._binned

    def sample(self, t):
        """Tree t's (indices into the ascending feature list, indices of the view's queries), the queries drawn from T."""
        return vm.sample(self.p["seed"], t, len(self.feats), self.T, self.rates)

    def subset(self, qsel):
        """Is the tree's query list a proper subset of the view's (the trainer then launches the gradients over the list)?"""
        return len(qsel) < len(self.queries)

    def gradients(self, s, qsel=None):
        """(lambda, w by instance id, rtol per query of the list) for the scores s; qsel: only these queries (others 0)."""
        qs = range(len(self.queries)) if qsel is None else qsel
        return expected_gradients(s, self.y, [self.queries[q] for q in qs], [self.norms[q] for q in qs], self.depth, self.p)

    def newton(self):
        return {k: self.p[k] for k in NEWTON_NUMBERS}

    def tree(self, lam, wt, fsel, qsel, **override):
        """The expected tree for gradients lam / wt (by instance id; only the sample's are read) on the sample."""
        p = dict(self.p, **override)
        rows = sm.instance_rows(self.queries, qsel)
        common = (p["max_depth"], p["min_leaf_support"], p["split_candidates"])
        if p["max_leaves"]:
            return lw.tree_on_sample(self.X, lam, wt, self.order_ids, self.feats, self.binned, rows, fsel, *common, p["max_leaves"],
                                     split_gain=p["split_gain"], **{k: p[k] for k in NEWTON_NUMBERS})
        if p["split_gain"] == "newton":
            return nm.tree_on_sample(self.X, lam, wt, self.order_ids, self.feats, self.binned, rows, fsel, *common,
                                     **{k: p[k] for k in NEWTON_NUMBERS})
        return sm.tree_for(p["grower"], self.X, lam, wt, self.queries, self.feats, self.binned, qsel, fsel, *common, self.present)

    def first_root(self):
        """Under split_gain "newton": (H_L, gain) of the split the FIRST tree's root takes with both floors at 0, from the
        restatement's gradients at zero scores, or None when that root does not split.  A floor set exactly at one of the two
        sits on the edge of its comparison: min_sum_hessian = H_L still admits the candidate (>=), min_split_gain = gain
        refuses the split (strict >)."""
        p = self.p
        fsel, qsel = self.sample(0)
        lam, wt, _ = self.gradients(np.zeros(self.X.shape[0]), qsel)
        ids = self.order_ids[sm.instance_rows(self.queries, qsel)]
        Q, S, W, Sw = nm.quantise_pair(lam[ids], wt[ids], len(ids))
        if S is None or not hm._enterable(len(ids), 1, p["max_depth"], p["min_leaf_support"]):
            return None
        edges, xbin = self.binned
        sub = xbin[np.ix_(np.asarray(fsel, dtype=np.int64), sm.instance_rows(self.queries, qsel))]
        best, node = nm.best_split(sub, [edges[f] for f in fsel], Q, W, np.arange(len(ids)), p["min_leaf_support"], S, Sw, p["lambda_l2"], 0.0)
        if best is None or not nm.accepts(best, node, S, Sw, p["lambda_l2"], 0.0):
            return None
        with np.errstate(over="ignore", invalid="ignore"):
            gain = float(np.float64(best[0]) - nm.term(node[1], node[2], S, Sw, p["lambda_l2"]))
        return float(nm.hess(best[5], Sw)), gain

    def measures(self, s):
        """(train_measure, valid_measure or None, the oracle evaluator's error flag) of the scores s."""
        per_q, err = self.c.metric_from_scores(self.reported, s, self.norms)
        if len(self.H):
            return vm.subset_mean(per_q, self.T), vm.subset_mean(per_q, self.H), err
        return o.mean(per_q), None, err

    def stopping(self, valid):
        """(best_iteration, trees trained, stopped_early, trees in the model) for the held-out measures so far."""
        T = self.p["num_trees"]
        return vm.stopping(list(valid) + [0.0] * (T - len(valid)), self.p["early_stopping_rounds"], T)

    def expected_stats(self):
        """The optional keys the trainer's stats must hold, with the values that echo the request."""
        p, out = self.p, {}
        if p["grower"] == "histogram":
            out["bins"] = p["split_candidates"]
            if p["split_gain"] == "newton":
                out.update(split_gain="newton", **self.newton())
            if p["max_leaves"]:
                out.update(max_leaves=p["max_leaves"], mean_leaves=None, pool_bytes=None)
        if min(self.rates) < 1.0:
            out.update(query_sampling_rate=self.rates[0], feature_sampling_rate=self.rates[1], seed=p["seed"], sample_queries=None,
                       sample_instances=None, sample_features=None)
        if len(self.H):
            out.update(validation_queries=len(self.H), training_queries=len(self.T), early_stopping_rounds=p["early_stopping_rounds"],
                       valid_measure=None, best_iteration=None, best_valid_measure=None, stopped_early=None)
        if p["truncation_level"]:
            out["truncation_level"] = p["truncation_level"]
        if p["lambda_norm"]:
            out["lambda_norm"] = True
        if p["objective"] != "ndcg":
            out["objective"] = p["objective"]
        return out

    # -- which keys bound --

    def observe(self, s, lam, wt, fsel, qsel, tree):
        """Notes what bound in this tree: s the prefix scores, lam / wt the gradients the tree was fitted to."""
        p, b = self.p, self.bound
        if p["query_sampling_rate"] < 1.0 and len(qsel) == 1:
            b["query_sampling_rate"] = True
        T = p["truncation_level"]
        cuts = T and not b["truncation_level"] and any(len(self.queries[q]) >= T + 2 for q in qsel)  # (two ranks outside the top T)
        if cuts or (p["lambda_norm"] and not b["lambda_norm"]):
            args = (s, self.y, [self.queries[q] for q in qsel], [self.norms[q] for q in qsel], self.depth, p)
            A, S = pair_mass(*args, T)
            if p["lambda_norm"] and np.any(S > 0.0):
                b["lambda_norm"] = True
            if cuts and A.tobytes() != pair_mass(*args, 0)[0].tobytes():
                b["truncation_level"] = True
        if p["max_leaves"] and not b["max_leaves"] and lw.n_leaves(tree) == p["max_leaves"]:
            b["max_leaves"] = lw.n_leaves(self.tree(lam, wt, fsel, qsel, max_leaves=p["max_leaves"] + 1)) > p["max_leaves"]
        for key in ("min_sum_hessian", "min_split_gain"):
            if p[key] != 0.0 and not b[key]:
                b[key] = self.tree(lam, wt, fsel, qsel, **{key: 0.0}) != tree

    # -- the whole loop on the CPU --

    def train(self, observe=False):
        """dict(model, scores of the returned model, trees (all that were trained), train_measure, valid_measure, samples,
        best_iteration, trained, stopped_early, oracle_error: the oracle's evaluator reported an error at zero scores or
        after some tree)."""
        p = self.p
        s = np.zeros(self.X.shape[0], dtype=np.float64)
        trees, train_m, valid_m, samples, prefix = [], [], [], [], [s]
        error = self.measures(s)[2] != 0
        best_it, trained, stopped, kept = 0, 0, False, 0
        for t in range(p["num_trees"]):
            fsel, qsel = self.sample(t)
            lam, wt, _ = self.gradients(s, qsel)
            tree = self.tree(lam, wt, fsel, qsel)
            if observe:
                self.observe(s, lam, wt, fsel, qsel, tree)
            s = s + p["learning_rate"] * lm.tree_scores(tree, self.X)  # every document of the view, held-out ones too
            trees.append(tree)
            samples.append((fsel, qsel))
            prefix.append(s)
            tr, va, err = self.measures(s)
            error = error or err != 0
            train_m.append(tr)
            trained = kept = t + 1
            if va is not None:
                valid_m.append(va)
                if self.stopping(valid_m)[1] <= t + 1:  # (the measures still to come are not read that far)
                    break
        if len(self.H):
            best_it, trained, stopped, kept = self.stopping(valid_m)
            self.bound["early_stopping_rounds"] = bool(stopped)
        model = {"Ensemble": {"weights": [p["learning_rate"]] * kept, "models": [{"DecisionTree": t} for t in trees[:kept]]}}
        return dict(model=model, scores=prefix[kept], trees=trees, train_measure=train_m, valid_measure=valid_m, samples=samples,
                    best_iteration=best_it, trained=trained, stopped_early=stopped, oracle_error=bool(error))
