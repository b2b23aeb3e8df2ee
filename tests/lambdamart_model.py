"""numpy restatement of LambdaMART training, for the tests.

It restates the definition, not the device code:
  * `gradients`: the LambdaRank gradient pass, each document's pair terms summed sequentially in f64 over its partners in
    the query's stored order (instance ids ascending);
  * `fit_tree`: the random-forest grower's SquaredError split search on given f32 targets (k - 1 thresholds spread evenly
    over the node's value range, sequential sums over the (value, list index)-sorted instances, the last maximum wins,
    features ascending), then Newton leaves sum lambda / sum w over the SCORING partition (x <= split -> lhs);
  * `train`: the boosting loop (scores start at 0.0, s = s + learning_rate * tree(x)).
Sequential f64 sums are np.cumsum (np.add.accumulate: one addition after the other, unlike np.sum).
"""
import math

import numpy as np


def seq_sum(a) -> float:
    a = np.asarray(a, dtype=np.float64)
    return float(np.cumsum(a)[-1]) if a.size else 0.0


def query_lists(c):
    """Per query of the oracle dataset `c` (its query order, which is the library's), the instance ids ascending."""
    offs = np.asarray(c.query_offsets(), dtype=np.int64)
    docs = np.asarray(c.query_docs(), dtype=np.int64)
    return [np.sort(docs[offs[q]:offs[q + 1]]) for q in range(len(offs) - 1)]


def depth_of(measure: str):
    return int(measure.split("@", 1)[1]) if "@" in measure else None


def gradients(scores, y, queries, norms, depth=None, sigma=1.0):
    """lambda, w by instance id (0.0 for every instance of a query without pairs or without a positive norm)."""
    n = len(y)
    lam = np.zeros(n, dtype=np.float64)
    wt = np.zeros(n, dtype=np.float64)
    sigma = float(sigma)
    sigma2 = sigma * sigma
    for q, ids in enumerate(queries):
        z = float(norms[q])
        if not (z > 0.0):
            continue
        m = len(ids)
        s = np.asarray(scores, dtype=np.float64)[ids]
        g = np.asarray(y, dtype=np.float32)[ids]
        G = np.array([2.0 ** float(x) - 1.0 for x in g], dtype=np.float64)
        # RankedInstance order: score descending, gain ascending, id ascending
        order = sorted(range(m), key=lambda i: (-s[i], g[i], ids[i]))
        rank = np.empty(m, dtype=np.int64)
        rank[order] = np.arange(m)
        k = m if depth is None else depth
        D = np.array([1.0 / math.log2(r + 2.0) if r < k else 0.0 for r in rank], dtype=np.float64)
        for i in range(m):
            other = g != g[i]
            high = g[i] > g
            diff = np.where(high, s[i] - s, s - s[i])
            delta = np.abs(G[i] - G) * np.abs(D[i] - D) / z
            rho = 1.0 / (1.0 + np.exp(sigma * diff))
            t = sigma * rho * delta
            tl = np.where(other, np.where(high, t, -t), 0.0)
            tw = np.where(other, sigma2 * rho * (1.0 - rho) * delta, 0.0)
            lam[ids[i]] = seq_sum(tl)
            wt[ids[i]] = seq_sum(tw)
    return lam, wt


def _sq_error(t):
    if t.size == 0:
        return 0.0
    mean = seq_sum(t) / float(t.size)
    return seq_sum((mean - t) ** 2)


def _grow(X, target, rows, ridx, feats, depth, max_depth, min_leaf, k, present=None):
    """rows: instance ids of the node, ridx: their index in the instance list.  Returns a nested dict whose leaves are
    {"LeafNode": rows} (values filled in later).  present[i, f] (file-loaded datasets): False where instance i does not
    hold feature f; such a value reads 0.0, but a feature's range is taken over the held values only, and a feature fewer
    than two of the node's instances hold yields no candidate (the RF grower's FeatureStats rule)."""
    n = len(rows)
    leaf = {"LeafNode": None}
    if n == 0 or depth >= max_depth or n < min_leaf or n <= 1:
        return leaf
    t_all = target[rows]
    if t_all.min() == t_all.max():
        return leaf
    have, best = False, None
    for f in feats:
        v = X[rows, f].astype(np.float64)
        held = v if present is None else v[present[rows, f]]
        if held.size <= 1:
            continue
        fmin, fmax = float(held.min()), float(held.max())
        order = np.lexsort((ridx, v))
        vs = v[order]
        ts = target[rows[order]].astype(np.float64)
        rng = fmax - fmin
        fhave, fbest = False, None
        prev = None
        for i in range(1, k):
            position = (float(i) / float(k)) * rng + fmin
            ids_i = int(np.searchsorted(vs, position, side="left"))
            if prev == ids_i:
                continue
            prev = ids_i
            nl, nr = ids_i, n - ids_i
            if nl < min_leaf or nr < min_leaf:
                continue
            imp = -(_sq_error(ts[:nl]) + _sq_error(ts[nl:]))
            if not fhave or imp >= fbest[0]:
                fhave, fbest = True, (imp, position, ids_i)
        if fhave and (not have or fbest[0] >= best[0]):
            have, best = True, (fbest[0], fbest[1], fbest[2], f, order)
    if not have:
        return leaf
    _, split, pos, f, order = best
    r, x = rows[order], ridx[order]
    return {"FeatureSplit": {"fid": int(f), "split": float(split),
                             "lhs": _grow(X, target, r[:pos], x[:pos], feats, depth + 1, max_depth, min_leaf, k, present),
                             "rhs": _grow(X, target, r[pos:], x[pos:], feats, depth + 1, max_depth, min_leaf, k, present)}}


def route(tree, X, ids):
    """Leaf (as the dict object) each instance reaches by the scoring rule: f64(x[fid]) <= split -> lhs."""
    out = []
    for i in ids:
        node = tree
        while "FeatureSplit" in node:
            fs = node["FeatureSplit"]
            node = fs["lhs"] if float(X[i, fs["fid"]]) <= fs["split"] else fs["rhs"]
        out.append(node)
    return out


def _leaves(tree):
    if "LeafNode" in tree:
        return [tree]
    return _leaves(tree["FeatureSplit"]["lhs"]) + _leaves(tree["FeatureSplit"]["rhs"])


def fit_tree(X, lam, wt, order_ids, feats, max_depth, min_leaf, k, present=None):
    """One boosting round's tree for gradients lam / wt (by instance id); order_ids: the instance list; present: see
    `_grow` (None: every value is held)."""
    order_ids = np.asarray(order_ids, dtype=np.int64)
    target = np.asarray(lam, dtype=np.float64).astype(np.float32)
    feats = sorted(int(f) for f in feats)
    if k < 2:
        tree = {"LeafNode": None}
    else:
        tree = _grow(X, target, order_ids, np.arange(len(order_ids)), feats, 1, max_depth, min_leaf, k, present)
    reached = route(tree, X, order_ids)
    for leaf in _leaves(tree):
        sel = np.array([r is leaf for r in reached], dtype=bool)
        sl, sw = seq_sum(np.asarray(lam)[order_ids[sel]]), seq_sum(np.asarray(wt)[order_ids[sel]])
        leaf["LeafNode"] = sl / sw if sw != 0.0 else 0.0
    return tree


def tree_scores(tree, X):
    n = X.shape[0]
    reached = route(tree, X, range(n))
    return np.array([r["LeafNode"] for r in reached], dtype=np.float64)


def train(X, y, c, measure="ndcg", num_trees=10, learning_rate=0.1, max_depth=6, min_leaf_support=10,
          split_candidates=64, sigma=1.0, norms=None, feats=None):
    """The whole boosting loop on the CPU; returns (model dict, train scores)."""
    queries = query_lists(c)
    order_ids = np.concatenate(queries) if queries else np.zeros(0, dtype=np.int64)
    if norms is None:
        norms = c.default_norms(measure)
    feats = range(X.shape[1]) if feats is None else feats
    s = np.zeros(X.shape[0], dtype=np.float64)
    trees = []
    for _ in range(num_trees):
        lam, wt = gradients(s, y, queries, norms, depth_of(measure), sigma)
        tree = fit_tree(X, lam, wt, order_ids, feats, max_depth, min_leaf_support, split_candidates)
        s = s + learning_rate * tree_scores(tree, X)
        trees.append(tree)
    model = {"Ensemble": {"weights": [learning_rate] * num_trees, "models": [{"DecisionTree": t} for t in trees]}}
    return model, s
