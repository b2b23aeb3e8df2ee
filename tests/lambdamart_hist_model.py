"""numpy restatement of LambdaMART's histogram grower ("Histogram grower"), for the tests.

It restates the definition, not the device code:
  * `bin_edges` / `bin_column`: at most k - 1 edges per feature from the sorted f32 column (all distinct values but the
    largest when there are at most k of them, else the k-quantile picks, duplicates and the maximum removed);
    bin(x) = number of edges strictly below x, so "bins 0..j" is exactly x <= edge_j, the scoring rule's partition;
  * `quantise`: gradients as int64 fixed point (S = 61 - e - c, round half to even), so sums do not depend on order;
  * `fit_tree`: per node and feature the count / integer-sum histogram, every edge a candidate with importance
    (sL*sL)/nL + (sR*sR)/nR in f64, the last maximum wins (later edge, then later feature); leaves are
    ldexp(Q, -S) / ldexp(W, -S_w) over the node's own instances;
  * `train`: lambdamart_model's boosting loop with this grower.
Gradients, routing and scoring are lambdamart_model's.
"""
import math

import numpy as np

from tests import lambdamart_model as lm


def canon(col):
    """The f32 column with -0.0 read as 0.0 (x + 0.0 under round to nearest)."""
    return np.asarray(col, dtype=np.float32) + np.float32(0.0)


def bin_edges(col, k):
    v = canon(col)
    if np.isnan(v).any():
        raise ValueError("NaN feature value")
    if np.isinf(v).any():  # (an edge is a data value: -inf would become a split no model file can hold; training refuses both)
        raise ValueError("infinite feature value")
    s = np.sort(v)
    n = len(s)
    if n == 0:
        return np.zeros(0, dtype=np.float32)
    distinct = np.unique(s)
    if len(distinct) <= k:
        return distinct[:-1].astype(np.float32)
    j = np.arange(1, k, dtype=np.int64)
    e = np.unique(s[(j * n + k - 1) // k - 1])
    return e[e != s[-1]].astype(np.float32)


def bin_column(col, edges):
    return np.searchsorted(edges, canon(col), side="left").astype(np.uint8)


def bin_matrix(X, order_ids, feats, k):
    """(edges per feature slot, xbin[slot][i] over the instance list)."""
    order_ids = np.asarray(order_ids, dtype=np.int64)
    edges, rows = [], []
    for f in feats:
        col = X[order_ids, f]
        e = bin_edges(col, k)
        edges.append(e)
        rows.append(bin_column(col, e))
    return edges, (np.stack(rows) if rows else np.zeros((0, len(order_ids)), dtype=np.uint8))


def quantise(v, n_instances):
    """(Q int64, S) for the values of the instance list; S is None when they are all zero (Q = 0)."""
    v = np.asarray(v, dtype=np.float64)
    m = float(np.max(np.abs(v))) if v.size else 0.0
    if m == 0.0:
        return np.zeros(v.shape, dtype=np.int64), None
    if not math.isfinite(m):
        raise ValueError("non-finite gradient")
    _, e = math.frexp(m)
    c = int(n_instances).bit_length()  # ceil(log2(N + 1))
    S = 61 - e - c
    return np.rint(np.ldexp(v, S)).astype(np.int64), S


_M21 = (1 << 21) - 1


def int_hist(b, q, nb):
    """Exact int64 sums of q per bin: three 21-bit limbs through bincount (each limb's f64 sums stay below 2^53 for up
    to 2^31 items)."""
    out = np.zeros(nb, dtype=np.int64)
    for shift, mask in ((0, True), (21, True), (42, False)):
        limb = (q >> shift) & _M21 if mask else q >> shift
        out += np.bincount(b, weights=limb.astype(np.float64), minlength=nb).astype(np.int64) << shift
    return out


def best_split(xbin, edges, Q, rows, min_leaf):
    """(importance, slot, edge index, nL, QL) of the node holding list indices `rows`, or None."""
    n = len(rows)
    q = Q[rows]
    qtot = int(q.sum())
    best = None
    for slot, e in enumerate(edges):
        ne = len(e)
        if ne == 0:
            continue
        b = xbin[slot][rows]
        nL = np.cumsum(np.bincount(b, minlength=ne + 1).astype(np.int64))[:ne]
        qL = np.cumsum(int_hist(b, q, ne + 1))[:ne]
        nR, qR = n - nL, qtot - qL
        ok = (nL >= min_leaf) & (nR >= min_leaf) & (nL > 0) & (nR > 0)
        if not ok.any():
            continue
        sL, sR = qL.astype(np.float64), qR.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            imp = (sL * sL) / nL.astype(np.float64) + (sR * sR) / nR.astype(np.float64)
        imp = np.where(ok, imp, -np.inf)
        j = ne - 1 - int(np.argmax(imp[::-1]))  # the last maximum
        if best is None or imp[j] >= best[0]:
            best = (float(imp[j]), slot, j, int(nL[j]), int(qL[j]))
    return best


def _enterable(n, depth, max_depth, min_leaf):
    return n >= 2 and depth < max_depth and n >= min_leaf


def _leaf(Q, W, S, Sw, rows):
    ql, wl = int(Q[rows].sum()), int(W[rows].sum())
    if wl == 0 or S is None:
        return {"LeafNode": 0.0}
    return {"LeafNode": math.ldexp(float(ql), -S) / math.ldexp(float(wl), -Sw)}


def _grow(xbin, edges, feats, Q, W, S, Sw, rows, depth, max_depth, min_leaf):
    if _enterable(len(rows), depth, max_depth, min_leaf):
        best = best_split(xbin, edges, Q, rows, min_leaf)
        if best is not None:
            _, slot, j, _, _ = best
            left = xbin[slot][rows] <= j
            return {"FeatureSplit": {"fid": int(feats[slot]), "split": float(edges[slot][j]),
                                     "lhs": _grow(xbin, edges, feats, Q, W, S, Sw, rows[left], depth + 1, max_depth, min_leaf),
                                     "rhs": _grow(xbin, edges, feats, Q, W, S, Sw, rows[~left], depth + 1, max_depth, min_leaf)}}
    return _leaf(Q, W, S, Sw, rows)


def fit_tree(X, lam, wt, order_ids, feats, max_depth, min_leaf, k, binned=None):
    """One boosting round's tree for gradients lam / wt (by instance id); order_ids: the instance list."""
    order_ids = np.asarray(order_ids, dtype=np.int64)
    feats = sorted(int(f) for f in feats)
    edges, xbin = binned if binned is not None else bin_matrix(X, order_ids, feats, k)
    n = len(order_ids)
    Q, S = quantise(np.asarray(lam, dtype=np.float64)[order_ids], n)
    if S is None:
        return {"LeafNode": 0.0}
    W, Sw = quantise(np.asarray(wt, dtype=np.float64)[order_ids], n)
    return _grow(xbin, edges, feats, Q, W, S, Sw, np.arange(n), 1, max_depth, min_leaf)


def train(X, y, c, measure="ndcg", num_trees=10, learning_rate=0.1, max_depth=6, min_leaf_support=10,
          split_candidates=64, sigma=1.0, norms=None, feats=None):
    """The whole boosting loop on the CPU; returns (model dict, train scores, training measure after each tree)."""
    queries = lm.query_lists(c)
    order_ids = np.concatenate(queries) if queries else np.zeros(0, dtype=np.int64)
    if norms is None:
        norms = c.default_norms(measure)
    feats = sorted(range(X.shape[1]) if feats is None else feats)
    binned = bin_matrix(X, order_ids, feats, split_candidates)
    s = np.zeros(X.shape[0], dtype=np.float64)
    trees, measures = [], []
    for _ in range(num_trees):
        lam, wt = lm.gradients(s, y, queries, norms, lm.depth_of(measure), sigma)
        tree = fit_tree(X, lam, wt, order_ids, feats, max_depth, min_leaf_support, split_candidates, binned)
        s = s + learning_rate * lm.tree_scores(tree, X)
        trees.append(tree)
        per_q, _ = c.metric_from_scores(measure, s)
        measures.append(float(np.nanmean(per_q)))
    model = {"Ensemble": {"weights": [learning_rate] * num_trees, "models": [{"DecisionTree": t} for t in trees]}}
    return model, s, measures
