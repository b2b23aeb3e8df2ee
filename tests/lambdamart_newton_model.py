"""numpy restatement of the histogram grower's Newton split gain ("Newton split gain"), for the tests.

Bins, edges, the instance and feature lists and the fixed-point step (Q with exponent S, W with its own exponent S_w, both
over the tree's list, c = bit length of its size) are lambdamart_hist_model's.  What changes, restated:
  * units: for an integer pair (Qx, Wx), G = ldexp(float(Qx), -S) and H = ldexp(float(Wx), -S_w) (the conversions round to
    nearest even); term(Qx, Wx) = (G * G) / (H + lambda_l2), every operation rounded on its own;
  * a candidate (feature, edge j) with (nL, QL, WL) over bins 0..j and (nR, QR, WR) by subtraction from the node's totals is
    valid when both counts are > 0 and >= min_leaf_support, H_L and H_R are >= min_sum_hessian, and H_L + lambda_l2 and
    H_R + lambda_l2 are > 0;
  * its importance is term(L) + term(R); the last maximum wins (later edge, then later feature of the tree's list);
  * the node splits only when importance - term(node) > min_split_gain (strict, in f64 as written), else it is a leaf;
  * a leaf is ldexp(Q, -S) / (ldexp(W, -S_w) + lambda_l2), 0.0 when that denominator is 0;
  * all-zero lambda: LeafNode(0.0); all-zero w: W = 0 and S_w = 0.
"""
import math

import numpy as np

from tests import lambdamart_hist_model as hm


def term(q, w, S, Sw, l2):
    """term of integer sums (python ints or int64 arrays)."""
    G = np.ldexp(np.asarray(q, dtype=np.int64).astype(np.float64), -S)
    H = np.ldexp(np.asarray(w, dtype=np.int64).astype(np.float64), -Sw)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        return (G * G) / (H + np.float64(l2))


def hess(w, Sw):
    return np.ldexp(np.asarray(w, dtype=np.int64).astype(np.float64), -Sw)


def candidates(xbin, edges, Q, W, rows, min_leaf, S, Sw, l2, min_hess):
    """Per feature slot with at least one edge: (slot, nL[ne], QL[ne], WL[ne], valid[ne], importance[ne]); and the node's
    (n, Qnode, Wnode)."""
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
        hL, hR = hess(wL, Sw), hess(wR, Sw)
        ok = (nL >= min_leaf) & (nR >= min_leaf) & (nL > 0) & (nR > 0)
        ok &= (hL >= min_hess) & (hR >= min_hess) & (hL + np.float64(l2) > 0.0) & (hR + np.float64(l2) > 0.0)
        with np.errstate(over="ignore", invalid="ignore"):
            imp = term(qL, wL, S, Sw, l2) + term(qR, wR, S, Sw, l2)
        out.append((slot, nL, qL, wL, ok, imp))
    return out, (n, qtot, wtot)


def best_split(xbin, edges, Q, W, rows, min_leaf, S, Sw, l2, min_hess):
    """((importance, slot, edge index, nL, QL, WL) or None, (n, Qnode, Wnode))."""
    cands, node = candidates(xbin, edges, Q, W, rows, min_leaf, S, Sw, l2, min_hess)
    best = None
    for slot, nL, qL, wL, ok, imp in cands:
        if not ok.any():
            continue
        imp = np.where(ok, imp, -np.inf)
        ne = len(imp)
        j = ne - 1 - int(np.argmax(imp[::-1]))  # the last maximum
        if best is None or imp[j] >= best[0]:
            best = (float(imp[j]), slot, j, int(nL[j]), int(qL[j]), int(wL[j]))
    return best, node


def accepts(best, node, S, Sw, l2, min_gain):
    with np.errstate(over="ignore", invalid="ignore"):
        return bool(np.float64(best[0]) - term(node[1], node[2], S, Sw, l2) > np.float64(min_gain))


def leaf_value(ql, wl, S, Sw, l2):
    den = math.ldexp(float(wl), -Sw) + float(l2)
    return math.ldexp(float(ql), -S) / den if den != 0.0 else 0.0


def _grow(xbin, edges, feats, Q, W, S, Sw, rows, depth, max_depth, min_leaf, l2, min_hess, min_gain):
    if hm._enterable(len(rows), depth, max_depth, min_leaf):
        best, node = best_split(xbin, edges, Q, W, rows, min_leaf, S, Sw, l2, min_hess)
        if best is not None and accepts(best, node, S, Sw, l2, min_gain):
            _, slot, j = best[:3]
            left = xbin[slot][rows] <= j
            args = (depth + 1, max_depth, min_leaf, l2, min_hess, min_gain)
            return {"FeatureSplit": {"fid": int(feats[slot]), "split": float(edges[slot][j]),
                                     "lhs": _grow(xbin, edges, feats, Q, W, S, Sw, rows[left], *args),
                                     "rhs": _grow(xbin, edges, feats, Q, W, S, Sw, rows[~left], *args)}}
    return {"LeafNode": leaf_value(int(Q[rows].sum()), int(W[rows].sum()), S, Sw, l2)}


def quantise_pair(lam, wt, n):
    """(Q, S, W, S_w) over a tree's list of n entries; S is None when every lambda is zero; all-zero w: W = 0, S_w = 0."""
    Q, S = hm.quantise(lam, n)
    W, Sw = hm.quantise(wt, n)
    return Q, S, W, (0 if Sw is None else Sw)


def fit_tree(X, lam, wt, order_ids, feats, max_depth, min_leaf, k, binned=None, lambda_l2=0.0, min_sum_hessian=0.0,
             min_split_gain=0.0):
    """One tree under the Newton gain for gradients lam / wt (by instance id); order_ids: the tree's instance list."""
    order_ids = np.asarray(order_ids, dtype=np.int64)
    feats = sorted(int(f) for f in feats)
    edges, xbin = binned if binned is not None else hm.bin_matrix(X, order_ids, feats, k)
    n = len(order_ids)
    Q, S, W, Sw = quantise_pair(np.asarray(lam, dtype=np.float64)[order_ids], np.asarray(wt, dtype=np.float64)[order_ids], n)
    if S is None:
        return {"LeafNode": 0.0}
    return _grow(xbin, edges, feats, Q, W, S, Sw, np.arange(n), 1, max_depth, min_leaf, float(lambda_l2), float(min_sum_hessian),
                 float(min_split_gain))


def tree_on_sample(X, lam, wt, order_ids, feats, binned, rows, fsel, max_depth, min_leaf, k, **newton):
    """The tree on a sample, as lambdamart_sample_model.hist_tree: rows = indices into the full instance list, fsel = indices
    into the ascending feature list `feats`; binned = (edges, xbin) of the FULL lists."""
    edges, xbin = binned
    rows = np.asarray(rows, dtype=np.int64)
    sub = ([edges[s] for s in fsel], xbin[np.ix_(np.asarray(fsel, dtype=np.int64), rows)])
    return fit_tree(X, lam, wt, np.asarray(order_ids, dtype=np.int64)[rows], [feats[s] for s in fsel], max_depth, min_leaf, k, sub,
                    **newton)
