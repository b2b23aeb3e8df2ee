"""numpy restatement of the histogram grower's symmetric trees ("Symmetric trees"), for the tests.

Bins, edges, the fixed-point step, `enterable`, a candidate's validity and importance, and the leaves are
lambdamart_hist_model's (variance criterion) and lambdamart_newton_model's (Newton gain), unchanged.  Only the split search of
a level changes, restated here:
  * a level holds its open nodes left to right: the root; then, parent by parent in the level's order, the lhs and the rhs of
    every node that split, each only if it is enterable (the others are leaves);
  * candidates are every feature slot f of the tree's list and every edge j of it;
  * v_a(f, j): node a's importance of the candidate, as the plain grower computes it: (sL*sL)/nL + (sR*sR)/nR, or
    term(L) + term(R) under the Newton gain;
  * u_a: the node's unsplit term: (s*s)/n with s = float(Qnode), n = float(count), or term(Qnode, Wnode) under Newton;
  * node a splits under (f, j) iff the candidate is valid for it by the plain rule: both counts > 0 and >= min_leaf_support;
    under Newton also H_L, H_R >= min_sum_hessian, H_L + lambda_l2 > 0, H_R + lambda_l2 > 0 and v_a - u_a > min_split_gain;
  * t_a = v_a where the node splits under the candidate, else u_a; I(f, j) = ((t_0 + t_1) + t_2) + ... in f64 over the open
    nodes in order, every addition rounded on its own; the candidate is valid iff some open node splits under it;
  * the last maximum of I over the valid candidates wins: the later edge, then the later feature; an I that is NaN compares
    as -inf (this makes the rule total: a NaN needs an open node with H + lambda_l2 = 0, which no valid split can make);
  * no valid candidate: every open node is a leaf.  Else every node that splits under the winner is split on it, and every
    other open node is a leaf.
With one open node I = v_0: the root's split, and a max_depth = 1 tree, are the plain grower's.
"""
import numpy as np

from tests import lambdamart_hist_model as hm
from tests import lambdamart_newton_model as nm


class Gain:
    """The split criterion: the variance one, or Newton with its three numbers."""

    def __init__(self, split_gain="variance", lambda_l2=0.0, min_sum_hessian=0.0, min_split_gain=0.0):
        if split_gain not in ("variance", "newton"):
            raise ValueError(split_gain)
        self.newton = split_gain == "newton"
        self.l2, self.min_hess, self.min_gain = float(lambda_l2), float(min_sum_hessian), float(min_split_gain)


def variance_candidates(xbin, edges, Q, rows, min_leaf):
    """lambdamart_hist_model.best_split's arithmetic with every edge kept: per feature slot with at least one edge
    (slot, valid[ne], importance[ne]); and the node's (n, Qnode)."""
    n = len(rows)
    q = Q[rows]
    qtot = int(q.sum())
    out = []
    for slot, e in enumerate(edges):
        ne = len(e)
        if ne == 0:
            continue
        b = xbin[slot][rows]
        nL = np.cumsum(np.bincount(b, minlength=ne + 1).astype(np.int64))[:ne]
        qL = np.cumsum(hm.int_hist(b, q, ne + 1))[:ne]
        nR, qR = n - nL, qtot - qL
        ok = (nL >= min_leaf) & (nR >= min_leaf) & (nL > 0) & (nR > 0)
        sL, sR = qL.astype(np.float64), qR.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            imp = (sL * sL) / nL.astype(np.float64) + (sR * sR) / nR.astype(np.float64)
        out.append((slot, ok, imp))
    return out, (n, qtot)


def node_terms(xbin, edges, Q, W, S, Sw, rows, min_leaf, gain):
    """{slot: (t[ne], splits[ne])} of one open node."""
    out = {}
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if gain.newton:
            cands, (n, qtot, wtot) = nm.candidates(xbin, edges, Q, W, rows, min_leaf, S, Sw, gain.l2, gain.min_hess)
            own = np.float64(nm.term(qtot, wtot, S, Sw, gain.l2))
            for slot, _, _, _, ok, imp in cands:
                splits = ok & (imp - own > np.float64(gain.min_gain))
                out[slot] = (np.where(splits, imp, own), splits)
        else:
            cands, (n, qtot) = variance_candidates(xbin, edges, Q, rows, min_leaf)
            s = np.float64(qtot)
            own = (s * s) / np.float64(n)
            for slot, ok, imp in cands:
                out[slot] = (np.where(ok, imp, own), ok)
    return out


def level_importance(terms):
    """{slot: (I[ne], valid[ne])} of a level from its open nodes' terms, in their order."""
    out = {}
    for slot in terms[0]:
        I, valid = terms[0][slot][0].copy(), terms[0][slot][1].copy()
        with np.errstate(invalid="ignore", over="ignore"):
            for t in terms[1:]:
                I = I + t[slot][0]  # (elementwise f64: every addition rounded on its own)
                valid = valid | t[slot][1]
        out[slot] = (I, valid)
    return out


def level_choice(terms):
    """(slot, edge index) of the level's winner, or None."""
    best = None
    for slot, (I, valid) in sorted(level_importance(terms).items()):
        if not valid.any():
            continue
        key = np.where(np.isnan(I), -np.inf, I)
        top = key[valid].max()
        j = int(np.flatnonzero(valid & (key == top))[-1])  # the last maximum
        if best is None or key[j] >= best[0]:
            best = (key[j], slot, j)
    return None if best is None else (best[1], best[2])


def _leaf(Q, W, S, Sw, rows, gain):
    if gain.newton:
        return {"LeafNode": nm.leaf_value(int(Q[rows].sum()), int(W[rows].sum()), S, Sw, gain.l2)}
    return hm._leaf(Q, W, S, Sw, rows)


def _grow(xbin, edges, feats, Q, W, S, Sw, n, max_depth, min_leaf, gain, levels_out=None, open_out=None):
    root = {}
    rows = np.arange(n)
    level = []
    if hm._enterable(n, 1, max_depth, min_leaf):
        level.append((root, rows, 1))
    else:
        root.update(_leaf(Q, W, S, Sw, rows, gain))
    levels = 0
    while level:
        if open_out is not None:
            open_out.append(len(level))
        terms = [node_terms(xbin, edges, Q, W, S, Sw, r, min_leaf, gain) for _, r, _ in level]
        choice = level_choice(terms)
        levels += choice is not None
        nxt = []
        for (node, r, depth), tm in zip(level, terms):
            if choice is None or not tm[choice[0]][1][choice[1]]:
                node.update(_leaf(Q, W, S, Sw, r, gain))
                continue
            slot, j = choice
            left = xbin[slot][r] <= j
            lhs, rhs = {}, {}
            node["FeatureSplit"] = {"fid": int(feats[slot]), "split": float(edges[slot][j]), "lhs": lhs, "rhs": rhs}
            for child, cr in ((lhs, r[left]), (rhs, r[~left])):
                if hm._enterable(len(cr), depth + 1, max_depth, min_leaf):
                    nxt.append((child, cr, depth + 1))
                else:
                    child.update(_leaf(Q, W, S, Sw, cr, gain))
        level = nxt
    if levels_out is not None:
        levels_out.append(levels)
    return root


def fit_tree(X, lam, wt, order_ids, feats, max_depth, min_leaf, k, binned=None, split_gain="variance", lambda_l2=0.0,
             min_sum_hessian=0.0, min_split_gain=0.0, levels_out=None, open_out=None):
    """One symmetric tree for gradients lam / wt (by instance id); order_ids: the tree's instance list.  levels_out (a list):
    the number of levels that split is appended; open_out (a list): the number of open nodes of every level searched."""
    gain = Gain(split_gain, lambda_l2, min_sum_hessian, min_split_gain)
    order_ids = np.asarray(order_ids, dtype=np.int64)
    feats = sorted(int(f) for f in feats)
    edges, xbin = binned if binned is not None else hm.bin_matrix(X, order_ids, feats, k)
    n = len(order_ids)
    lam_l, wt_l = np.asarray(lam, dtype=np.float64)[order_ids], np.asarray(wt, dtype=np.float64)[order_ids]
    if gain.newton:
        Q, S, W, Sw = nm.quantise_pair(lam_l, wt_l, n)
    else:
        Q, S = hm.quantise(lam_l, n)
        W, Sw = hm.quantise(wt_l, n)
    if S is None:
        if levels_out is not None:
            levels_out.append(0)
        return {"LeafNode": 0.0}
    return _grow(xbin, edges, feats, Q, W, S, Sw, n, max_depth, min_leaf, gain, levels_out, open_out)


def tree_on_sample(X, lam, wt, order_ids, feats, binned, rows, fsel, max_depth, min_leaf, k, **kw):
    """The tree on a sample, as lambdamart_newton_model.tree_on_sample: rows = indices into the full instance list, fsel =
    indices into the ascending feature list `feats`; binned = (edges, xbin) of the FULL lists."""
    edges, xbin = binned
    rows = np.asarray(rows, dtype=np.int64)
    sub = ([edges[s] for s in fsel], xbin[np.ix_(np.asarray(fsel, dtype=np.int64), rows)])
    return fit_tree(X, lam, wt, np.asarray(order_ids, dtype=np.int64)[rows], [feats[s] for s in fsel], max_depth, min_leaf, k, sub, **kw)
