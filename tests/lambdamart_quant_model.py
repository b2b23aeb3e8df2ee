"""numpy restatement of LambdaMART's quantised gradients ("Quantised gradients"), for the tests.

It restates the definition, not the device code (no packing, no atomics).  For tree t, after the fixed-point step (which
gives Q_i and W_i (int64) per entry of the tree's list of n entries and the exponents S and S_w; c = the bit length of n):
  1. K_t = the t-th rand_u64() of Rand64(seed ^ 0x5155414E54475244) (the oracle's generator; "QUANTGRD").
  2. with b = grad_quant_bits: d = 62 - c - b, d_w = 61 - c - b.
  3. r_i = mix(K_t + phi (2 id_i + 1)) >> (64 - d), r'_i = mix(K_t + phi (2 id_i + 2)) >> (64 - d_w), phi =
     0x9E3779B97F4A7C15, mix = the splitmix64 finaliser, id = the document's original instance id; all in 64-bit
     wrap-around arithmetic.
  4. q_i = (Q_i + r_i) >> d (floor), w_i = (W_i + r'_i) >> d_w.
  5. the tree's shape is that of the Newton histogram tree (level-wise, leaf-wise or symmetric) over (q_i, w_i) under the
     exponents S - d and S_w - d_w.
  6. every leaf's value is G / (H + lambda_l2) from the sums of Q_i and W_i of its own entries under (S, S_w) (0.0 for a zero
     denominator).  All-zero lambda: LeafNode(0.0).
Python integers carry the 64-bit arithmetic (masked), so nothing here can overflow silently.
"""
import numpy as np

from oracle import pyoracle as o
from tests import lambdamart_goss_model as gm
from tests import lambdamart_hist_model as hm
from tests import lambdamart_leafwise_model as lw
from tests import lambdamart_newton_model as nm
from tests import lambdamart_symmetric_model as sy

QUANT_STREAM = 0x5155414E54475244  # "QUANTGRD"
PHI = 0x9E3779B97F4A7C15
MASK = 2 ** 64 - 1


def keys(seed: int, trees: int):
    """K_0 .. K_{trees-1} of the request's seed, as Python integers."""
    return [int(k) for k in o.rand64_stream((int(seed) ^ QUANT_STREAM) & MASK, trees)]


def mix(z: int) -> int:
    z &= MASK
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return z


def shifts(n: int, bits: int):
    """(d, d_w) for a list of n entries."""
    c = int(n).bit_length()
    return 62 - c - int(bits), 61 - c - int(bits)


def offsets(key: int, ids, which: int, shift: int):
    """r (which = 1, shift = d) or r' (which = 2, shift = d_w) of the original instance ids, as Python integers."""
    return [mix(int(key) + PHI * (2 * int(i) + which)) >> (64 - shift) for i in ids]


def quantise(Q, W, ids, bits: int, key: int):
    """(q, w) as int64 arrays, and (d, d_w), for the fixed-point values Q / W of a list whose entries have the original
    instance ids `ids`."""
    n = len(ids)
    d, dw = shifts(n, bits)
    q = [(int(v) + r) >> d for v, r in zip(Q, offsets(key, ids, 1, d))]  # (Python's >> of a negative integer is floor)
    w = [(int(v) + r) >> dw for v, r in zip(W, offsets(key, ids, 2, dw))]
    return np.asarray(q, dtype=np.int64), np.asarray(w, dtype=np.int64), d, dw


def renew(node, X, rows_ids, Q, W, S, Sw, l2, at=None):
    """The leaves of `node` (a dict like the model's) renewed in place from the full-precision sums: X by instance id,
    rows_ids the original instance ids of the list, Q / W by list index.  A split sends x <= split left, which is the
    partition the tree was trained on."""
    if at is None:
        at = np.arange(len(rows_ids))
    if "LeafNode" in node:
        node["LeafNode"] = nm.leaf_value(int(Q[at].sum()), int(W[at].sum()), S, Sw, l2)
        return node
    sp = node["FeatureSplit"]
    left = X[rows_ids[at], sp["fid"]] <= np.float32(sp["split"])
    renew(sp["lhs"], X, rows_ids, Q, W, S, Sw, l2, at[left])
    renew(sp["rhs"], X, rows_ids, Q, W, S, Sw, l2, at[~left])
    return node


def fit_tree(X, lam, wt, order_ids, feats, max_depth, min_leaf, k, bits, key, binned=None, lambda_l2=0.0, min_sum_hessian=0.0,
             min_split_gain=0.0, max_leaves=0, symmetric=False):
    """One quantised tree for gradients lam / wt (by instance id); order_ids: the tree's instance list (original ids)."""
    order_ids = np.asarray(order_ids, dtype=np.int64)
    feats = sorted(int(f) for f in feats)
    edges, xbin = binned if binned is not None else hm.bin_matrix(X, order_ids, feats, k)
    n = len(order_ids)
    Q, S, W, Sw = nm.quantise_pair(np.asarray(lam, dtype=np.float64)[order_ids], np.asarray(wt, dtype=np.float64)[order_ids], n)
    if S is None:
        return {"LeafNode": 0.0}
    q, w, d, dw = quantise(Q, W, order_ids, bits, key)
    l2, mh, mg = float(lambda_l2), float(min_sum_hessian), float(min_split_gain)
    if symmetric:
        tree = sy._grow(xbin, edges, feats, q, w, S - d, Sw - dw, n, max_depth, min_leaf, sy.Gain("newton", l2, mh, mg))
    elif max_leaves:
        tree = lw.grow(xbin, edges, feats, q, w, S - d, Sw - dw, n, max_depth, min_leaf, max_leaves, (l2, mh, mg))
    else:
        tree = nm._grow(xbin, edges, feats, q, w, S - d, Sw - dw, np.arange(n), 1, max_depth, min_leaf, l2, mh, mg)
    return renew(tree, np.asarray(X, dtype=np.float32), order_ids, Q, W, S, Sw, l2)


def tree_on_sample(X, lam, wt, order_ids, feats, binned, rows, fsel, max_depth, min_leaf, k, bits, key, **kw):
    """The tree on a sample, as lambdamart_newton_model.tree_on_sample: rows = indices into the full instance list, fsel =
    indices into the ascending feature list `feats`; binned = (edges, xbin) of the FULL lists."""
    edges, xbin = binned
    rows = np.asarray(rows, dtype=np.int64)
    sub = ([edges[s] for s in fsel], xbin[np.ix_(np.asarray(fsel, dtype=np.int64), rows)])
    return fit_tree(X, lam, wt, np.asarray(order_ids, dtype=np.int64)[rows], [feats[s] for s in fsel], max_depth, min_leaf, k, bits, key, sub,
                    **kw)


def goss_tree(X, lam, wt, order_ids, feats, binned, L, fsel, max_depth, min_leaf, k, bits, key, a, b, goss_key, **kw):
    """The quantised tree under GOSS: the GOSS list of L with the amplified values (lambdamart_goss_model), then as above."""
    rows, top, _, amp = gm.goss_list(lam, L, order_ids, a, b, goss_key)
    lam2, wt2 = gm.amplified(lam, wt, order_ids, rows, top, amp)
    return tree_on_sample(X, lam2, wt2, order_ids, feats, binned, rows, fsel, max_depth, min_leaf, k, bits, key, **kw), rows
