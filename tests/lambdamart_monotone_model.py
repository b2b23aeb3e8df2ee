"""numpy restatement of the histogram grower's monotone constraints ("Monotone constraints"), for the
tests.

Bins, edges, the lists, the fixed-point step, Newton's validity conditions and the leaf-wise order of splits are
lambdamart_hist_model's, lambdamart_newton_model's and lambdamart_leafwise_model's.  What is new, restated:
  * every node carries an interval [lo, hi] of f64, the root (-inf, +inf);
  * out(G, H) = G / (H + lambda_l2), 0.0 for a zero denominator; v = out below lo ? lo : out, then v above hi ? hi : v;
  * term(G, H, v) = (G * G) / (H + lambda_l2) when v == out, else (2.0 * G) * v - ((H + lambda_l2) * v) * v, every operation
    rounded on its own;
  * a candidate on a feature of sign c has Newton's conditions and, for c = +1, vL <= vR, for c = -1, vL >= vR; its importance
    is term_L + term_R, the last maximum wins;
  * the node's gain is the importance minus term of the node's own sums under the node's own interval;
  * a split on a feature of sign 0 hands [lo, hi] to both children; otherwise mid = (vL + vR) * 0.5, and +1 gives the lhs
    [lo, mid] and the rhs [mid, hi], -1 the lhs [mid, hi] and the rhs [lo, mid];
  * a leaf is its own out, clamped to its interval; a leaf whose value the clamp changed counts as clamped.
"""

import numpy as np

from tests import lambdamart_hist_model as hm
from tests import lambdamart_leafwise_model as lw
from tests import lambdamart_newton_model as nm

INF = float("inf")


def clamp(out, lo, hi):
    v = np.where(out < lo, np.float64(lo), out)
    return np.where(v > hi, np.float64(hi), v)


def term(q, w, S, Sw, l2, lo, hi):
    """(term, v) of integer sums (python ints or int64 arrays) under [lo, hi]."""
    G = np.ldexp(np.asarray(q, dtype=np.int64).astype(np.float64), -S)
    den = np.ldexp(np.asarray(w, dtype=np.int64).astype(np.float64), -Sw) + np.float64(l2)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        out = np.where(den != 0.0, G / den, np.float64(0.0))
        v = clamp(out, lo, hi)
        plain = (G * G) / den
        bound = (np.float64(2.0) * G) * v - (den * v) * v
    return np.where(v == out, plain, bound), v


def candidates(xbin, edges, Q, W, rows, min_leaf, S, Sw, l2, min_hess, lo, hi, signs):
    """Per feature slot with at least one edge: (slot, nL, QL, WL, valid, importance, vL, vR); and the node's (n, Qnode, Wnode)."""
    n = len(rows)
    q, w = Q[rows], W[rows]
    qtot, wtot = int(q.sum()), int(w.sum())
    out = []
    for slot, e in enumerate(edges):
        ne = len(e)
        if ne == 0:
            continue
        b = xbin[slot][rows]
        nL = np.cumsum(np.bincount(b, minlength=ne + 1).astype(np.int64))[:ne]
        qL = np.cumsum(hm.int_hist(b, q, ne + 1))[:ne]
        wL = np.cumsum(hm.int_hist(b, w, ne + 1))[:ne]
        nR, qR, wR = n - nL, qtot - qL, wtot - wL
        hL, hR = nm.hess(wL, Sw), nm.hess(wR, Sw)
        ok = (nL >= min_leaf) & (nR >= min_leaf) & (nL > 0) & (nR > 0)
        ok &= (hL >= min_hess) & (hR >= min_hess) & (hL + np.float64(l2) > 0.0) & (hR + np.float64(l2) > 0.0)
        tL, vL = term(qL, wL, S, Sw, l2, lo, hi)
        tR, vR = term(qR, wR, S, Sw, l2, lo, hi)
        if signs[slot] > 0:
            ok &= vL <= vR
        elif signs[slot] < 0:
            ok &= vL >= vR
        with np.errstate(over="ignore", invalid="ignore"):
            imp = tL + tR
        out.append((slot, nL, qL, wL, ok, imp, vL, vR))
    return out, (n, qtot, wtot)


def best_split(xbin, edges, Q, W, rows, min_leaf, S, Sw, l2, min_hess, lo, hi, signs):
    """((importance, slot, edge index, nL, QL, WL, vL, vR) or None, (n, Qnode, Wnode))."""
    cands, node = candidates(xbin, edges, Q, W, rows, min_leaf, S, Sw, l2, min_hess, lo, hi, signs)
    best = None
    for slot, nL, qL, wL, ok, imp, vL, vR in cands:
        if not ok.any():
            continue
        imp = np.where(ok, imp, -np.inf)
        ne = len(imp)
        j = ne - 1 - int(np.argmax(imp[::-1]))  # the last maximum
        if best is None or imp[j] >= best[0]:
            best = (float(imp[j]), slot, j, int(nL[j]), int(qL[j]), int(wL[j]), float(vL[j]), float(vR[j]))
    return best, node


def gain(best, node, S, Sw, l2, lo, hi):
    with np.errstate(over="ignore", invalid="ignore"):
        return float(np.float64(best[0]) - term(node[1], node[2], S, Sw, l2, lo, hi)[0])


def child_bounds(lo, hi, c, vL, vR):
    """((lo, hi) of the lhs, (lo, hi) of the rhs)."""
    if c == 0:
        return (lo, hi), (lo, hi)
    mid = float((np.float64(vL) + np.float64(vR)) * np.float64(0.5))
    return ((lo, mid), (mid, hi)) if c > 0 else ((mid, hi), (lo, mid))


def leaf(Q, W, S, Sw, l2, rows, lo, hi):
    """(value, 1 when the clamp changed it else 0)."""
    out = nm.leaf_value(int(Q[rows].sum()), int(W[rows].sum()), S, Sw, l2)
    v = lo if out < lo else out
    v = hi if v > hi else v
    return v, int(v != out)


def _split_node(node, feats, edges, slot, j):
    lhs, rhs = {}, {}
    node["FeatureSplit"] = {"fid": int(feats[slot]), "split": float(edges[slot][j]), "lhs": lhs, "rhs": rhs}
    return lhs, rhs


def grow_levels(xbin, edges, feats, Q, W, S, Sw, n, max_depth, min_leaf, newton, signs):
    l2, min_hess, min_gain = newton
    root, clamped = {}, 0
    todo = [(root, np.arange(n), 1, -INF, INF)]
    while todo:
        node, rows, depth, lo, hi = todo.pop()
        if hm._enterable(len(rows), depth, max_depth, min_leaf):
            best, tot = best_split(xbin, edges, Q, W, rows, min_leaf, S, Sw, l2, min_hess, lo, hi, signs)
            if best is not None and gain(best, tot, S, Sw, l2, lo, hi) > np.float64(min_gain):
                slot, j = best[1], best[2]
                left = xbin[slot][rows] <= j
                lhs, rhs = _split_node(node, feats, edges, slot, j)
                bl, br = child_bounds(lo, hi, signs[slot], best[6], best[7])
                todo.append((lhs, rows[left], depth + 1) + bl)
                todo.append((rhs, rows[~left], depth + 1) + br)
                continue
        node["LeafNode"], c = leaf(Q, W, S, Sw, l2, rows, lo, hi)
        clamped += c
    return root, clamped


def grow_leaves(xbin, edges, feats, Q, W, S, Sw, n, max_depth, min_leaf, max_leaves, newton, signs):
    """lambdamart_leafwise_model.grow with an interval per leaf: a searched leaf is never searched again."""
    l2, min_hess, min_gain = newton
    root = {}
    closed, open_leaves = [], []

    def made(node, rows, depth, index, searched, lo, hi):
        rec = None
        if searched and hm._enterable(len(rows), depth, max_depth, min_leaf):
            best, tot = best_split(xbin, edges, Q, W, rows, min_leaf, S, Sw, l2, min_hess, lo, hi, signs)
            if best is not None:
                g = gain(best, tot, S, Sw, l2, lo, hi)
                if g > np.float64(min_gain):
                    rec = dict(gain=g, best=best)
        if rec is None:
            closed.append((node, rows, lo, hi))
        else:
            open_leaves.append(dict(node=node, rows=rows, depth=depth, index=index, rec=rec, lo=lo, hi=hi))

    made(root, np.arange(n), 1, 0, True, -INF, INF)
    leaves, next_index = 1, 1
    while leaves < max_leaves and open_leaves:
        o = open_leaves.pop(lw.pick_open(open_leaves))
        best, rows = o["rec"]["best"], o["rows"]
        slot, j = best[1], best[2]
        left = xbin[slot][rows] <= j
        lhs, rhs = _split_node(o["node"], feats, edges, slot, j)
        bl, br = child_bounds(o["lo"], o["hi"], signs[slot], best[6], best[7])
        leaves += 1
        more = leaves < max_leaves
        made(lhs, rows[left], o["depth"] + 1, next_index, more, *bl)
        made(rhs, rows[~left], o["depth"] + 1, next_index + 1, more, *br)
        next_index += 2
    clamped = 0
    for node, rows, lo, hi in closed + [(o["node"], o["rows"], o["lo"], o["hi"]) for o in open_leaves]:
        node["LeafNode"], c = leaf(Q, W, S, Sw, l2, rows, lo, hi)
        clamped += c
    return root, clamped


def fit_tree(X, lam, wt, order_ids, feats, max_depth, min_leaf, k, monotone, max_leaves=0, binned=None, lambda_l2=0.0,
             min_sum_hessian=0.0, min_split_gain=0.0):
    """(tree, number of clamped leaves) for gradients lam / wt (by instance id) under the Newton gain and the constraints
    monotone = {feature id: sign}; order_ids: the tree's instance list; max_leaves = 0: level-wise, >= 2: leaf-wise."""
    order_ids = np.asarray(order_ids, dtype=np.int64)
    feats = sorted(int(f) for f in feats)
    signs = [int(monotone.get(f, 0)) for f in feats]
    edges, xbin = binned if binned is not None else hm.bin_matrix(X, order_ids, feats, k)
    n = len(order_ids)
    Q, S, W, Sw = nm.quantise_pair(np.asarray(lam, dtype=np.float64)[order_ids], np.asarray(wt, dtype=np.float64)[order_ids], n)
    if S is None:
        return {"LeafNode": 0.0}, 0
    newton = (float(lambda_l2), float(min_sum_hessian), float(min_split_gain))
    if max_leaves:
        return grow_leaves(xbin, edges, feats, Q, W, S, Sw, n, max_depth, min_leaf, max_leaves, newton, signs)
    return grow_levels(xbin, edges, feats, Q, W, S, Sw, n, max_depth, min_leaf, newton, signs)


def tree_on_sample(X, lam, wt, order_ids, feats, binned, rows, fsel, max_depth, min_leaf, k, monotone, max_leaves=0, **newton):
    """The tree on a sample, as lambdamart_newton_model.tree_on_sample: rows = indices into the full instance list, fsel =
    indices into the ascending feature list `feats`; binned = (edges, xbin) of the FULL lists."""
    edges, xbin = binned
    rows = np.asarray(rows, dtype=np.int64)
    sub = ([edges[s] for s in fsel], xbin[np.ix_(np.asarray(fsel, dtype=np.int64), rows)])
    return fit_tree(X, lam, wt, np.asarray(order_ids, dtype=np.int64)[rows], [feats[s] for s in fsel], max_depth, min_leaf, k, monotone,
                    max_leaves, sub, **newton)


def predict(tree, X):
    """The tree's value for every row of X (x <= split -> lhs)."""
    X = np.asarray(X)
    out = np.zeros(len(X), dtype=np.float64)

    def walk(node, idx):
        if "LeafNode" in node:
            out[idx] = node["LeafNode"]
            return
        sp = node["FeatureSplit"]
        left = X[idx, sp["fid"]].astype(np.float64) <= sp["split"]
        walk(sp["lhs"], idx[left])
        walk(sp["rhs"], idx[~left])

    walk(tree, np.arange(len(X)))
    return out


def splits_of(tree, fid, acc=None):
    """Every split value of the tree on feature fid."""
    acc = [] if acc is None else acc
    if "FeatureSplit" in tree:
        sp = tree["FeatureSplit"]
        if sp["fid"] == fid:
            acc.append(sp["split"])
        splits_of(sp["lhs"], fid, acc)
        splits_of(sp["rhs"], fid, acc)
    return acc


def probe_grid(values):
    """Ascending f32 grid: every value, its two f32 neighbours, and the extremes."""
    v = np.asarray(sorted(set(values)), dtype=np.float32)
    big = np.float32(np.finfo(np.float32).max)
    g = np.concatenate([v, np.nextafter(v, -big), np.nextafter(v, big), np.asarray([-big, big], dtype=np.float32)])
    return np.unique(g)


def violations(score_fn, X_rows, fid, grid, sign):
    """The number of (row, adjacent grid pair) at which the scores move against `sign`: score_fn(X) -> scores; every row of
    X_rows is copied once per grid value of feature fid."""
    X_rows = np.asarray(X_rows, dtype=np.float32)
    R, G = len(X_rows), len(grid)
    P = np.repeat(X_rows, G, axis=0)
    P[:, fid] = np.tile(np.asarray(grid, dtype=np.float32), R)
    s = np.asarray(score_fn(P), dtype=np.float64).reshape(R, G)
    return int(np.sum(s[:, 1:] < s[:, :-1])) if sign > 0 else int(np.sum(s[:, 1:] > s[:, :-1]))
