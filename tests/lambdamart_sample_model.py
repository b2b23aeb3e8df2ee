"""numpy restatement of LambdaMART's per-tree query and feature samples ("Sampling"), for the tests.

The definition, restated:
  * F = the view's features ascending, Q = the view's queries in the view's order.  count(len, rate) =
    min(len, max(1, int(len * rate))), the random-forest trainer's rule.
  * The master generator Rand64(seed) gives tree t = 0, 1, ... two values in order: fseed_t, qseed_t.
  * A tree's features: shuffle(0..|F|-1) under Rand64(fseed_t), the first count(|F|, feature rate) entries, sorted.  Its
    queries: the same with qseed_t over 0..|Q|-1 and the query rate.  A rate of 1.0 gives the full list and still uses up
    the seed.
  * The tree's instance list: the sampled queries in the view's order, instance ids ascending inside each (a subsequence
    of the full list).  Gradients are those of the full pass; the tree is grown over that list and those features --
    the exact grower as lambdamart_model.fit_tree on them; the histogram grower on the bins and edges of the FULL lists,
    with the fixed-point scale taken over the tree's list (c = bit length of its size) -- and added to the scores of
    every document of the view.
The generator is the oracle's (oracle.pyoracle.rand64_stream / shuffle_with_seed); gradients and both growers' trees are
the existing restatements', called on the sampled lists.
"""
import numpy as np

from oracle import pyoracle as o
from tests import lambdamart_hist_model as hm
from tests import lambdamart_model as lm


def count(length, rate):
    x = float(length) * float(rate)
    c = 0 if (x != x or x <= 0.0) else (length if x >= float(length) else int(x))
    return min(length, max(1, c))


def _draw(seed, length, rate):
    if rate >= 1.0:
        return np.arange(length, dtype=np.int64)
    return np.sort(o.shuffle_with_seed(int(seed), length)[:count(length, rate)].astype(np.int64))


def sample(seed, t, nF, nQ, rates):
    """(indices into the ascending feature list, indices into the view's queries), both ascending, of tree t.
    rates = (query_sampling_rate, feature_sampling_rate)."""
    qrate, frate = rates
    seeds = o.rand64_stream(int(seed), 2 * (t + 1))
    return _draw(seeds[2 * t], nF, frate), _draw(seeds[2 * t + 1], nQ, qrate)


def instance_rows(queries, qsel):
    """Indices into the full instance list (the concatenation of `queries`) of the entries whose query is in qsel."""
    offs = np.concatenate([[0], np.cumsum([len(ids) for ids in queries])]).astype(np.int64)
    if len(qsel) == 0:
        return np.zeros(0, dtype=np.int64)
    return np.concatenate([np.arange(offs[q], offs[q + 1], dtype=np.int64) for q in qsel])


def hist_tree(X, lam, wt, order_ids, feats, binned, rows, fsel, max_depth, min_leaf, k):
    """The histogram grower's tree on a sample: rows = indices into the full instance list, fsel = indices into the
    ascending feature list `feats`; binned = (edges, xbin) of the FULL lists."""
    edges, xbin = binned
    rows = np.asarray(rows, dtype=np.int64)
    sub = ([edges[s] for s in fsel], xbin[np.ix_(np.asarray(fsel, dtype=np.int64), rows)])
    return hm.fit_tree(X, lam, wt, np.asarray(order_ids, dtype=np.int64)[rows], [feats[s] for s in fsel], max_depth, min_leaf, k, sub)


def tree_for(grower, X, lam, wt, queries, feats, binned, qsel, fsel, max_depth, min_leaf, k, present=None):
    """One tree of either grower on the sample (qsel, fsel); lam / wt by instance id (only the sample's are read)."""
    order_ids = np.concatenate(queries)
    rows = instance_rows(queries, qsel)
    if grower == "histogram":
        return hist_tree(X, lam, wt, order_ids, feats, binned, rows, fsel, max_depth, min_leaf, k)
    return lm.fit_tree(X, lam, wt, order_ids[rows], [feats[s] for s in fsel], max_depth, min_leaf, k, present)


def train(X, y, c, grower="exact", measure="ndcg", num_trees=10, learning_rate=0.1, max_depth=6, min_leaf_support=10,
          split_candidates=64, sigma=1.0, norms=None, feats=None, rates=(1.0, 1.0), seed=0):
    """The boosting loop with per-tree samples; returns (model dict, train scores, training measure after each tree,
    the samples used)."""
    queries = lm.query_lists(c)
    order_ids = np.concatenate(queries)
    if norms is None:
        norms = c.default_norms(measure)
    feats = sorted(range(X.shape[1]) if feats is None else feats)
    binned = hm.bin_matrix(X, order_ids, feats, split_candidates) if grower == "histogram" else None
    s = np.zeros(X.shape[0], dtype=np.float64)
    trees, measures, samples = [], [], []
    for t in range(num_trees):
        fsel, qsel = sample(seed, t, len(feats), len(queries), rates)
        # per query, nothing crosses queries: the sampled queries' gradients are all a tree needs
        lam, wt = lm.gradients(s, y, [queries[q] for q in qsel], [norms[q] for q in qsel], lm.depth_of(measure), sigma)
        tree = tree_for(grower, X, lam, wt, queries, feats, binned, qsel, fsel, max_depth, min_leaf_support, split_candidates)
        s = s + learning_rate * lm.tree_scores(tree, X)  # every document of the view
        trees.append(tree)
        samples.append((fsel, qsel))
        per_q, _ = c.metric_from_scores(measure, s)
        measures.append(float(np.nanmean(per_q)))
    model = {"Ensemble": {"weights": [learning_rate] * num_trees, "models": [{"DecisionTree": t} for t in trees]}}
    return model, s, measures, samples
