"""numpy restatement of the histogram grower's leaf regularisation ("Leaf regularisation"), for the
tests.

Bins, edges, the lists, the fixed-point step, Newton's validity conditions, the leaf-wise order of splits, the monotone
intervals and the symmetric level choice are lambdamart_hist_model's, lambdamart_newton_model's, lambdamart_leafwise_model's,
lambdamart_monotone_model's and lambdamart_symmetric_model's.  What is new, restated: for a node or candidate side with
integer sums (Q, W), n instances, parent output p (None for the root) and interval [lo, hi], with G = ldexp(Q, -S),
H = ldexp(W, -S_w), den = H + lambda_l2, every operation f64 and rounded on its own:
  1. T  = G - l1 if G > l1, G + l1 if G < -l1, else 0.0
  2. q0 = T / den, 0.0 when den == 0
  3. o  = q0; with max_delta_step > 0: o = mds if o > mds, then o = -mds if o < -mds
  4. with path_smooth > 0 and a parent: r = float(n) / path_smooth, o = (o * r) / (r + 1.0) + p / (r + 1.0)
  5. v  = lo if o < lo else o, then hi if v > hi
  6. term = (T * T) / den when v == q0, else (2.0 * T) * v - (den * v) * v
  * a candidate's validity is Newton's, with the monotone order on vL, vR under a sign; its importance is term(L) + term(R),
    both sides pulled toward the splitting node's own output v_node, n the side's count;
  * the node's own output is its v (the root: step 4 skipped), its own term is step 6 at that v; it splits when
    importance - own > min_split_gain;
  * the children carry vL, vR as their outputs; mid = (vL + vR) * 0.5 cuts the interval under a sign;
  * a leaf's value is its v from its own sums, count, parent output and interval;
  * symmetric trees (no path_smooth): steps 1 to 3 and 6 for both sides and for a node's unsplit term.
reg = (lambda_l1, max_delta_step, path_smooth) throughout.
"""
import numpy as np

from tests import lambdamart_hist_model as hm
from tests import lambdamart_leafwise_model as lw
from tests import lambdamart_monotone_model as mm
from tests import lambdamart_newton_model as nm
from tests import lambdamart_symmetric_model as sy

INF = float("inf")


def sums(q, w, S, Sw, l1, l2):
    """(T, den, q0) of integer sums (python ints or int64 arrays)."""
    G = np.ldexp(np.asarray(q, dtype=np.int64).astype(np.float64), -S)
    den = np.ldexp(np.asarray(w, dtype=np.int64).astype(np.float64), -Sw) + np.float64(l2)
    l1 = np.float64(l1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        T = np.where(G > l1, G - l1, np.where(G < -l1, G + l1, np.float64(0.0)))
        q0 = np.where(den != 0.0, T / den, np.float64(0.0))
    return T, den, q0


def output(q0, n, reg, parent, lo, hi):
    """Steps 3 to 5."""
    _, mds, smooth = (np.float64(x) for x in reg)
    o = np.asarray(q0, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        if mds > 0.0:
            o = np.where(o > mds, mds, o)
            o = np.where(o < -mds, -mds, o)
        if smooth > 0.0 and parent is not None:
            r = np.asarray(n, dtype=np.int64).astype(np.float64) / smooth
            o = (o * r) / (r + np.float64(1.0)) + np.float64(parent) / (r + np.float64(1.0))
    return mm.clamp(o, lo, hi)


def term_at(T, den, q0, v):
    """Step 6."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        return np.where(v == q0, (T * T) / den, (np.float64(2.0) * T) * v - (den * v) * v)


def side(q, w, n, S, Sw, l2, reg, parent, lo=-INF, hi=INF):
    """(term, v) of integer sums (python ints or int64 arrays) and counts."""
    T, den, q0 = sums(q, w, S, Sw, reg[0], l2)
    v = output(q0, n, reg, parent, lo, hi)
    return term_at(T, den, q0, v), v


def own_term(q, w, S, Sw, l2, reg, v_node):
    T, den, q0 = sums(q, w, S, Sw, reg[0], l2)
    return float(term_at(T, den, q0, np.float64(v_node)))


def candidates(xbin, edges, Q, W, rows, min_leaf, S, Sw, l2, min_hess, reg, v_node, lo, hi, signs):
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
        tL, vL = side(qL, wL, nL, S, Sw, l2, reg, v_node, lo, hi)
        tR, vR = side(qR, wR, nR, S, Sw, l2, reg, v_node, lo, hi)
        if signs[slot] > 0:
            ok &= vL <= vR
        elif signs[slot] < 0:
            ok &= vL >= vR
        with np.errstate(over="ignore", invalid="ignore"):
            imp = tL + tR
        out.append((slot, nL, qL, wL, ok, imp, vL, vR))
    return out, (n, qtot, wtot)


def search(xbin, edges, Q, W, S, Sw, rows, min_leaf, newton, reg, parent, lo, hi, signs):
    """The record of a searched node, or None when it does not split: dict(gain, imp, slot, edge, nL, vL, vR, v: the node's
    own output, rival: the (slot, edge) that wins with path_smooth at 0 and everything else the same)."""
    l2, min_hess, min_gain = newton
    n = len(rows)
    v_node = float(side(int(Q[rows].sum()), int(W[rows].sum()), n, S, Sw, l2, reg, parent, lo, hi)[1])

    def winner(r):
        cands, node = candidates(xbin, edges, Q, W, rows, min_leaf, S, Sw, l2, min_hess, r, v_node, lo, hi, signs)
        best = None
        for slot, nL, qL, wL, ok, imp, vL, vR in cands:
            if not ok.any():
                continue
            imp = np.where(ok, imp, -np.inf)
            j = len(imp) - 1 - int(np.argmax(imp[::-1]))  # the last maximum
            if best is None or imp[j] >= best[0]:
                best = (float(imp[j]), slot, j, int(nL[j]), float(vL[j]), float(vR[j]))
        return best, node

    best, node = winner(reg)
    if best is None:
        return None
    with np.errstate(over="ignore", invalid="ignore"):
        gain = float(np.float64(best[0]) - np.float64(own_term(node[1], node[2], S, Sw, l2, reg, v_node)))
    if not gain > np.float64(min_gain):
        return None
    rival = winner((reg[0], reg[1], 0.0))[0] if reg[2] > 0.0 else best
    return dict(gain=gain, imp=best[0], slot=best[1], edge=best[2], nL=best[3], vL=best[4], vR=best[5], v=v_node,
                rival=None if rival is None else (rival[1], rival[2]))


def leaf(Q, W, S, Sw, l2, reg, rows, parent, lo, hi):
    return float(side(int(Q[rows].sum()), int(W[rows].sum()), len(rows), S, Sw, l2, reg, parent, lo, hi)[1])


def _note(trace, depth, rec, parent):
    if trace is not None:
        trace.append(dict(depth=depth, parent=parent, **rec))


def grow_levels(xbin, edges, feats, Q, W, S, Sw, n, max_depth, min_leaf, newton, reg, signs, trace=None):
    root = {}
    todo = [(root, np.arange(n), 1, None, -INF, INF)]
    while todo:
        node, rows, depth, parent, lo, hi = todo.pop()
        if hm._enterable(len(rows), depth, max_depth, min_leaf):
            rec = search(xbin, edges, Q, W, S, Sw, rows, min_leaf, newton, reg, parent, lo, hi, signs)
            if rec is not None:
                _note(trace, depth, rec, parent)
                slot, j = rec["slot"], rec["edge"]
                left = xbin[slot][rows] <= j
                lhs, rhs = mm._split_node(node, feats, edges, slot, j)
                bl, br = mm.child_bounds(lo, hi, signs[slot], rec["vL"], rec["vR"])
                todo.append((lhs, rows[left], depth + 1, rec["v"]) + bl)
                todo.append((rhs, rows[~left], depth + 1, rec["v"]) + br)
                continue
        node["LeafNode"] = leaf(Q, W, S, Sw, newton[0], reg, rows, parent, lo, hi)
    return root


def grow_leaves(xbin, edges, feats, Q, W, S, Sw, n, max_depth, min_leaf, max_leaves, newton, reg, signs, trace=None):
    """lambdamart_monotone_model.grow_leaves with an output per leaf."""
    root = {}
    closed, open_leaves = [], []

    def made(node, rows, depth, index, searched, parent, lo, hi):
        rec = None
        if searched and hm._enterable(len(rows), depth, max_depth, min_leaf):
            rec = search(xbin, edges, Q, W, S, Sw, rows, min_leaf, newton, reg, parent, lo, hi, signs)
        if rec is None:
            closed.append((node, rows, parent, lo, hi))
        else:
            open_leaves.append(dict(node=node, rows=rows, depth=depth, index=index, rec=rec, parent=parent, lo=lo, hi=hi))

    made(root, np.arange(n), 1, 0, True, None, -INF, INF)
    leaves, next_index = 1, 1
    while leaves < max_leaves and open_leaves:
        o = open_leaves.pop(lw.pick_open(open_leaves))
        rec, rows = o["rec"], o["rows"]
        _note(trace, o["depth"], rec, o["parent"])
        slot, j = rec["slot"], rec["edge"]
        left = xbin[slot][rows] <= j
        lhs, rhs = mm._split_node(o["node"], feats, edges, slot, j)
        bl, br = mm.child_bounds(o["lo"], o["hi"], signs[slot], rec["vL"], rec["vR"])
        leaves += 1
        more = leaves < max_leaves
        made(lhs, rows[left], o["depth"] + 1, next_index, more, rec["v"], *bl)
        made(rhs, rows[~left], o["depth"] + 1, next_index + 1, more, rec["v"], *br)
        next_index += 2
    for node, rows, parent, lo, hi in closed + [(o["node"], o["rows"], o["parent"], o["lo"], o["hi"]) for o in open_leaves]:
        node["LeafNode"] = leaf(Q, W, S, Sw, newton[0], reg, rows, parent, lo, hi)
    return root


def _sym_terms(xbin, edges, Q, W, S, Sw, rows, min_leaf, newton, reg):
    """lambdamart_symmetric_model.node_terms under steps 1 to 3 and 6."""
    l2, min_hess, min_gain = newton
    none = [0] * len(edges)
    out = {}
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        cands, (n, qtot, wtot) = candidates(xbin, edges, Q, W, rows, min_leaf, S, Sw, l2, min_hess, reg, None, -INF, INF, none)
        own = np.float64(side(qtot, wtot, n, S, Sw, l2, reg, None)[0])
        for slot, _, _, _, ok, imp, _, _ in cands:
            splits = ok & (imp - own > np.float64(min_gain))
            out[slot] = (np.where(splits, imp, own), splits)
    return out


def grow_symmetric(xbin, edges, feats, Q, W, S, Sw, n, max_depth, min_leaf, newton, reg):
    if reg[2] != 0.0:
        raise ValueError("symmetric trees take no path_smooth")
    root = {}
    level = []

    def close(node, rows):
        node["LeafNode"] = leaf(Q, W, S, Sw, newton[0], reg, rows, None, -INF, INF)

    if hm._enterable(n, 1, max_depth, min_leaf):
        level.append((root, np.arange(n), 1))
    else:
        close(root, np.arange(n))
    while level:
        terms = [_sym_terms(xbin, edges, Q, W, S, Sw, r, min_leaf, newton, reg) for _, r, _ in level]
        choice = sy.level_choice(terms)
        nxt = []
        for (node, r, depth), tm in zip(level, terms):
            if choice is None or not tm[choice[0]][1][choice[1]]:
                close(node, r)
                continue
            slot, j = choice
            left = xbin[slot][r] <= j
            lhs, rhs = mm._split_node(node, feats, edges, slot, j)
            for child, cr in ((lhs, r[left]), (rhs, r[~left])):
                if hm._enterable(len(cr), depth + 1, max_depth, min_leaf):
                    nxt.append((child, cr, depth + 1))
                else:
                    close(child, cr)
        level = nxt
    return root


def fit_tree(X, lam, wt, order_ids, feats, max_depth, min_leaf, k, reg, monotone=None, max_leaves=0, symmetric=False, binned=None,
             lambda_l2=0.0, min_sum_hessian=0.0, min_split_gain=0.0, trace=None):
    """One tree under the Newton gain and reg = (lambda_l1, max_delta_step, path_smooth) for gradients lam / wt (by instance
    id); order_ids: the tree's instance list; monotone = {feature id: sign}; max_leaves = 0: level-wise, >= 2: leaf-wise.
    trace (a list): one dict per split (see `search`, plus depth and the node's parent output)."""
    reg = tuple(float(x) for x in reg)
    order_ids = np.asarray(order_ids, dtype=np.int64)
    feats = sorted(int(f) for f in feats)
    signs = [int((monotone or {}).get(f, 0)) for f in feats]
    edges, xbin = binned if binned is not None else hm.bin_matrix(X, order_ids, feats, k)
    n = len(order_ids)
    Q, S, W, Sw = nm.quantise_pair(np.asarray(lam, dtype=np.float64)[order_ids], np.asarray(wt, dtype=np.float64)[order_ids], n)
    if S is None:
        return {"LeafNode": 0.0}
    newton = (float(lambda_l2), float(min_sum_hessian), float(min_split_gain))
    if symmetric:
        return grow_symmetric(xbin, edges, feats, Q, W, S, Sw, n, max_depth, min_leaf, newton, reg)
    if max_leaves:
        return grow_leaves(xbin, edges, feats, Q, W, S, Sw, n, max_depth, min_leaf, max_leaves, newton, reg, signs, trace)
    return grow_levels(xbin, edges, feats, Q, W, S, Sw, n, max_depth, min_leaf, newton, reg, signs, trace)


def tree_on_sample(X, lam, wt, order_ids, feats, binned, rows, fsel, max_depth, min_leaf, k, reg, **kw):
    """The tree on a sample, as lambdamart_newton_model.tree_on_sample: rows = indices into the full instance list, fsel =
    indices into the ascending feature list `feats`; binned = (edges, xbin) of the FULL lists."""
    edges, xbin = binned
    rows = np.asarray(rows, dtype=np.int64)
    sub = ([edges[s] for s in fsel], xbin[np.ix_(np.asarray(fsel, dtype=np.int64), rows)])
    return fit_tree(X, lam, wt, np.asarray(order_ids, dtype=np.int64)[rows], [feats[s] for s in fsel], max_depth, min_leaf, k, reg,
                    binned=sub, **kw)


def leaves_of(tree, acc=None):
    """Every leaf value of the tree."""
    acc = [] if acc is None else acc
    if "LeafNode" in tree:
        acc.append(tree["LeafNode"])
    else:
        leaves_of(tree["FeatureSplit"]["lhs"], acc)
        leaves_of(tree["FeatureSplit"]["rhs"], acc)
    return acc
