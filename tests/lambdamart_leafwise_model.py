"""numpy restatement of the histogram grower's leaf-wise growth ("Leaf-wise growth"), for the tests.

Bins, edges, the lists, the fixed-point step, a node's candidates and its choice among them (`best_split`), `term`, the
Newton acceptance rule (`accepts`), the `enterable` rule and the leaf values are lambdamart_hist_model's and
lambdamart_newton_model's.  What is new, restated:
  * every node has a creation index: the root 0; a split gives its lhs the next index, then its rhs;
  * a leaf that is enterable is searched when it is created, and is open when it has a valid candidate that is accepted
    (variance: any valid candidate; newton: importance - term(node) > min_split_gain);
  * the gain of an open leaf is importance - term(Qnode, Wnode) under "newton" and importance - (sN * sN) / n under the
    variance criterion (sN = float(Qnode), n the node's count), f64, every operation rounded on its own; it only ranks;
  * while the tree has fewer than max_leaves leaves and a leaf is open, the open leaf with the largest gain is split, the
    smallest creation index among equal gains.
"""
import numpy as np

from tests import lambdamart_hist_model as hm
from tests import lambdamart_newton_model as nm


def search(xbin, edges, Q, W, S, Sw, rows, min_leaf, newton):
    """The record of a searched leaf, or None when it does not become open: dict(gain, imp, slot, edge, nL, QL, WL, n,
    Qnode, Wnode); newton: None (the variance criterion) or (lambda_l2, min_sum_hessian, min_split_gain)."""
    n = len(rows)
    if newton is None:
        best = hm.best_split(xbin, edges, Q, rows, min_leaf)
        if best is None:
            return None
        imp, slot, j, nL, qL = best
        qn = int(Q[rows].sum())
        sN = np.float64(qn)
        gain = float(np.float64(imp) - (sN * sN) / np.float64(n))
        return dict(gain=gain, imp=imp, slot=slot, edge=j, nL=nL, QL=qL, WL=None, n=n, Qnode=qn, Wnode=None)
    l2, min_hess, min_gain = newton
    best, node = nm.best_split(xbin, edges, Q, W, rows, min_leaf, S, Sw, l2, min_hess)
    if best is None or not nm.accepts(best, node, S, Sw, l2, min_gain):
        return None
    with np.errstate(over="ignore", invalid="ignore"):
        gain = float(np.float64(best[0]) - nm.term(node[1], node[2], S, Sw, l2))
    return dict(gain=gain, imp=best[0], slot=best[1], edge=best[2], nL=best[3], QL=best[4], WL=best[5], n=n, Qnode=node[1],
                Wnode=node[2])


def pick_open(open_leaves):
    """The open leaf to split: the largest gain, the smallest creation index among equals."""
    at = 0
    for i in range(1, len(open_leaves)):
        a, b = open_leaves[i], open_leaves[at]
        if a["rec"]["gain"] > b["rec"]["gain"] or (a["rec"]["gain"] == b["rec"]["gain"] and a["index"] < b["index"]):
            at = i
    return at


def grow(xbin, edges, feats, Q, W, S, Sw, n, max_depth, min_leaf, max_leaves, newton=None, trace=None):
    """The tree (a dict like the model's) over list indices 0..n-1.  trace (a list): one entry per split, in order:
    dict(index, depth, rec, open=[(index, rec) of every leaf open at that moment, the split one included]), and a last entry
    dict(index=None, leaves, open=[(index, rec) of the leaves still open when growth stopped])."""
    if max_leaves < 2:
        raise ValueError("max_leaves must be at least 2 here (0 is level-wise growth: lambdamart_hist_model)")
    root = {}
    closed, open_leaves = [], []

    def made(node, rows, depth, index, searched):
        rec = search(xbin, edges, Q, W, S, Sw, rows, min_leaf, newton) if searched and hm._enterable(len(rows), depth, max_depth, min_leaf) else None
        if rec is None:
            closed.append((node, rows))
        else:
            open_leaves.append(dict(node=node, rows=rows, depth=depth, index=index, rec=rec))

    made(root, np.arange(n), 1, 0, True)
    leaves, next_index = 1, 1
    while leaves < max_leaves and open_leaves:
        at = pick_open(open_leaves)
        if trace is not None:
            trace.append(dict(index=open_leaves[at]["index"], depth=open_leaves[at]["depth"], rec=open_leaves[at]["rec"],
                              open=[(o["index"], o["rec"]) for o in open_leaves]))
        o = open_leaves.pop(at)
        rec, rows = o["rec"], o["rows"]
        left = xbin[rec["slot"]][rows] <= rec["edge"]
        lhs, rhs = {}, {}
        o["node"]["FeatureSplit"] = {"fid": int(feats[rec["slot"]]), "split": float(edges[rec["slot"]][rec["edge"]]), "lhs": lhs, "rhs": rhs}
        leaves += 1
        more = leaves < max_leaves  # the split that reaches max_leaves searches no child
        made(lhs, rows[left], o["depth"] + 1, next_index, more)
        made(rhs, rows[~left], o["depth"] + 1, next_index + 1, more)
        next_index += 2
    if trace is not None:
        trace.append(dict(index=None, leaves=leaves, open=[(o["index"], o["rec"]) for o in open_leaves]))
    for node, rows in closed + [(o["node"], o["rows"]) for o in open_leaves]:
        ql, wl = int(Q[rows].sum()), int(W[rows].sum())
        if newton is None:
            node.update(hm._leaf(Q, W, S, Sw, rows))
        else:
            node["LeafNode"] = nm.leaf_value(ql, wl, S, Sw, newton[0])
    return root


def _newton(split_gain, lambda_l2, min_sum_hessian, min_split_gain):
    if split_gain == "variance":
        return None
    if split_gain != "newton":
        raise ValueError(split_gain)
    return (float(lambda_l2), float(min_sum_hessian), float(min_split_gain))


def fit_tree(X, lam, wt, order_ids, feats, max_depth, min_leaf, k, max_leaves, binned=None, split_gain="variance", lambda_l2=0.0,
             min_sum_hessian=0.0, min_split_gain=0.0, trace=None):
    """One leaf-wise tree for gradients lam / wt (by instance id); order_ids: the tree's instance list."""
    order_ids = np.asarray(order_ids, dtype=np.int64)
    feats = sorted(int(f) for f in feats)
    edges, xbin = binned if binned is not None else hm.bin_matrix(X, order_ids, feats, k)
    n = len(order_ids)
    newton = _newton(split_gain, lambda_l2, min_sum_hessian, min_split_gain)
    lam_l, wt_l = np.asarray(lam, dtype=np.float64)[order_ids], np.asarray(wt, dtype=np.float64)[order_ids]
    if newton is None:
        Q, S = hm.quantise(lam_l, n)
        W, Sw = hm.quantise(wt_l, n)
    else:
        Q, S, W, Sw = nm.quantise_pair(lam_l, wt_l, n)
    if S is None:
        return {"LeafNode": 0.0}
    return grow(xbin, edges, feats, Q, W, S, Sw, n, max_depth, min_leaf, max_leaves, newton, trace)


def tree_on_sample(X, lam, wt, order_ids, feats, binned, rows, fsel, max_depth, min_leaf, k, max_leaves, **kw):
    """The tree on a sample, as lambdamart_newton_model.tree_on_sample: rows = indices into the full instance list, fsel =
    indices into the ascending feature list `feats`; binned = (edges, xbin) of the FULL lists."""
    edges, xbin = binned
    rows = np.asarray(rows, dtype=np.int64)
    sub = ([edges[s] for s in fsel], xbin[np.ix_(np.asarray(fsel, dtype=np.int64), rows)])
    return fit_tree(X, lam, wt, np.asarray(order_ids, dtype=np.int64)[rows], [feats[s] for s in fsel], max_depth, min_leaf, k, max_leaves,
                    sub, **kw)


def n_leaves(node):
    if "LeafNode" in node:
        return 1
    return n_leaves(node["FeatureSplit"]["lhs"]) + n_leaves(node["FeatureSplit"]["rhs"])


def depth(node):
    if "LeafNode" in node:
        return 1
    return 1 + max(depth(node["FeatureSplit"]["lhs"]), depth(node["FeatureSplit"]["rhs"]))


def mirrored_halves(seed, half):
    """(X[2 half, 2], lam, wt): feature 0 tells the halves apart, feature 1 is the same in both, and the second half's lambda is
    the first half's negated.  The root splits on feature 0 (no split on feature 1 separates anything at the root: its two
    sides' sums are 0), and the two children are mirror images: the same counts and hessian sums and negated gradient sums
    per bin, so the same importances and the same gain bit for bit under either criterion."""
    rng = np.random.default_rng(seed)
    inner = rng.integers(0, 6, half).astype(np.float32)
    X = np.zeros((2 * half, 2), dtype=np.float32)
    X[:, 0] = np.concatenate([np.zeros(half), np.ones(half)])
    X[:, 1] = np.concatenate([inner, inner])
    g = rng.normal(0.0, 1.0, half)
    g = g - g.mean() - 4.0
    w = rng.random(half) + 0.5
    return X, np.concatenate([g, -g]), np.concatenate([w, w])


def copied_halves(seed, half):
    """(X[2 half, 2], lam, wt) for the variance criterion: feature 0 is the same in both halves, feature 1 (the LAST feature)
    tells them apart, lambda is 1 everywhere.  Every candidate of a node then has the importance n exactly, so the last one
    wins: the root splits the halves apart, and its children have identical histograms and the gain 0."""
    rng = np.random.default_rng(seed)
    inner = rng.integers(0, 6, half).astype(np.float32)
    X = np.zeros((2 * half, 2), dtype=np.float32)
    X[:, 0] = np.concatenate([inner, inner])
    X[:, 1] = np.concatenate([np.zeros(half), np.ones(half)])
    return X, np.ones(2 * half), np.full(2 * half, 0.5)
