"""numpy restatement of LambdaMART's held-out validation queries and early stopping ("Validation and
early stopping"), for the tests.  Built on the restatements of the trainer (lambdamart_model), the histogram grower
(lambdamart_hist_model) and the per-tree samples (lambdamart_sample_model).

The definition, restated:
  * Q = the view's queries in the view's order; H = the held-out ones, T = Q \\ H the training ones, both in that order.
    With H empty everything is lambdamart_sample_model.train.
  * A tree is fitted to queries of T only.  Without a query rate its query list is T; with one it is count(|T|, rate)
    queries: shuffle(0..|T|-1) under qseed_t, the first count entries, sorted, mapped through T.  The master generator
    still hands every tree fseed_t then qseed_t.  The tree's instance list is the subsequence of the full list that
    belongs to those queries; the histogram grower's bins and edges stay those of the FULL instance list (held-out
    documents included) and its fixed-point scale is taken over the tree's list.
  * A query's gradients depend on its own documents, scores and norm only.  Without judgments a query's norm is a function
    of its own labels, so the labels of H reach no tree; judgments that name a training query change that query's norm and
    so its gradients, whichever queries are held out.
  * The update adds the tree to every document of the view, held-out ones included.
  * After tree t: train_measure = mean(per_q[T]), valid_measure = mean(per_q[H]), each the project's two-level mean
    (oracle.pyoracle.mean under the current segment setting) over the subset's per-query values in the view's order,
    compacted; zero-norm queries count 0.0 and count in the divisor.
  * best_iteration = the 1-based number of the tree with the FIRST maximum of valid_measure (strict >).  With
    early_stopping_rounds = r > 0 training ends after tree t as soon as t - best_iteration >= r, and the model is the first
    best_iteration trees -- whether training ended early or ran out of trees.  With r = 0 all trees are trained and kept.
"""
import numpy as np

from oracle import pyoracle as o
from tests import lambdamart_hist_model as hm
from tests import lambdamart_model as lm
from tests import lambdamart_sample_model as sm


def split(names, held):
    """(T, H): indices into `names` (the view's queries in its order) of the training / held-out queries, ascending."""
    names = [str(x) for x in names]
    held = set(str(x) for x in held)
    assert held <= set(names) and len(held) < len(names)
    H = np.array([i for i, q in enumerate(names) if q in held], dtype=np.int64)
    T = np.array([i for i, q in enumerate(names) if q not in held], dtype=np.int64)
    return T, H


def sample(seed, t, nF, T, rates):
    """Tree t's (indices into the ascending feature list, indices of the view's queries): the queries are drawn from T."""
    T = np.asarray(T, dtype=np.int64)
    fsel, q = sm.sample(seed, t, nF, len(T), rates)
    return fsel, T[q]


def subset_mean(per_q, idx):
    return o.mean(np.asarray(per_q, dtype=np.float64)[np.asarray(idx, dtype=np.int64)])


def stopping(valid, r, num_trees=None):
    """The rule on a sequence of held-out measures, one per tree in training order: (best_iteration, trees trained,
    stopped_early, trees in the model).  `valid` may be longer than what is trained: it is read only as far as training goes."""
    num_trees = len(valid) if num_trees is None else num_trees
    best_it, best = 0, 0.0
    for t in range(1, num_trees + 1):
        v = valid[t - 1]
        if best_it == 0 or v > best:
            best_it, best = t, v
        if r > 0 and t - best_it >= r:
            return best_it, t, t < num_trees, best_it
    return best_it, num_trees, False, best_it if r > 0 else num_trees


def train(X, y, c, held_idx=(), grower="exact", measure="ndcg", num_trees=10, learning_rate=0.1, max_depth=6, min_leaf_support=10,
          split_candidates=64, sigma=1.0, norms=None, feats=None, rates=(1.0, 1.0), seed=0, early_stopping_rounds=0):
    """The boosting loop.  held_idx: indices of the held-out queries in the oracle dataset's query order.  Returns a dict:
    model, scores (of the RETURNED model), train_measure, valid_measure, samples, best_iteration, trees, stopped_early."""
    queries = lm.query_lists(c)
    nq = len(queries)
    H = np.array(sorted(int(q) for q in held_idx), dtype=np.int64)
    T = np.array([q for q in range(nq) if q not in set(H.tolist())], dtype=np.int64)
    assert len(T) > 0 and (early_stopping_rounds == 0 or len(H) > 0)
    order_ids = np.concatenate(queries)
    if norms is None:
        norms = c.default_norms(measure)
    feats = sorted(range(X.shape[1]) if feats is None else feats)
    binned = hm.bin_matrix(X, order_ids, feats, split_candidates) if grower == "histogram" else None  # (the FULL list)
    s = np.zeros(X.shape[0], dtype=np.float64)
    trees, train_m, valid_m, samples, prefix_scores = [], [], [], [], []
    best_it, best, stopped = 0, 0.0, False
    for t in range(num_trees):
        fsel, qsel = sample(seed, t, len(feats), T, rates)
        lam, wt = lm.gradients(s, y, [queries[q] for q in qsel], [norms[q] for q in qsel], lm.depth_of(measure), sigma)
        tree = sm.tree_for(grower, X, lam, wt, queries, feats, binned, qsel, fsel, max_depth, min_leaf_support, split_candidates)
        s = s + learning_rate * lm.tree_scores(tree, X)  # every document of the view, held-out ones too
        trees.append(tree)
        samples.append((fsel, qsel))
        prefix_scores.append(s)
        per_q, _ = c.metric_from_scores(measure, s, norms)
        if len(H):
            train_m.append(subset_mean(per_q, T))
            valid_m.append(subset_mean(per_q, H))
            if best_it == 0 or valid_m[-1] > best:
                best_it, best = t + 1, valid_m[-1]
            if early_stopping_rounds > 0 and (t + 1) - best_it >= early_stopping_rounds:
                stopped = t + 1 < num_trees
                break
        else:
            train_m.append(o.mean(per_q))
    trained = len(trees)
    keep = best_it if (len(H) and early_stopping_rounds > 0) else trained
    model = {"Ensemble": {"weights": [learning_rate] * keep, "models": [{"DecisionTree": t} for t in trees[:keep]]}}
    return dict(model=model, scores=prefix_scores[keep - 1], train_measure=train_m, valid_measure=valid_m, samples=samples,
                best_iteration=best_it, trees=trained, stopped_early=stopped, T=T, H=H)
