"""numpy restatement of LambdaMART's gradient-based one-side sampling ("GOSS"), for the tests.

It restates the definition, not the device code (no radix passes, no scans).  For tree t, after the gradient pass:
  1. L = the tree's instance list: indices into the view's full instance list, ascending (the query sample, without the
     held-out queries); n_t entries.
  2. key_i = the 64 bits of fabs(lambda_i) read as an unsigned integer.
  3. n_top = sample_count(n_t, a) = min(n_t, max(1, int(n_t * a))).
  4. tau = the n_top-th largest key.
  5. top = every entry with key > tau, and the first n_top - #{key > tau} entries with key == tau in list order.
  6. every other entry is kept iff u < p, p = b / (1.0 - a) in f64, u = (mix(K_t + 0x9E3779B97F4A7C15 (id + 1)) >> 11) 2^-53,
     mix = the splitmix64 finaliser, id = the document's original instance id, K_t = the t-th rand_u64() of
     Rand64(seed ^ 0x474F5353474F5353) (the oracle's generator; "GOSSGOSS").
  7. kept others: lambda' = lambda amp, w' = w amp, amp = (1.0 - a) / b, one rounded product each; the top set keeps its values.
  8. the GOSS list = the kept entries, ascending; n_g entries.
  9. the tree is the Newton histogram tree (lambdamart_newton_model, or the leaf-wise / monotone one) over that list with the
     amplified values: both exponents over the list's amplified values, c the bit length of n_g.
"""
import numpy as np

from oracle import pyoracle as o
from tests import lambdamart_leafwise_model as lw
from tests import lambdamart_monotone_model as mm
from tests import lambdamart_newton_model as nm
from tests import lambdamart_sample_model as sm
from tests import lambdamart_xendcg_model as xm

GOSS_STREAM = 0x474F5353474F5353  # "GOSSGOSS"
MASK = 2 ** 64 - 1


def keys(seed: int, trees: int):
    """K_0 .. K_{trees-1} of the request's seed, as Python integers."""
    return [int(k) for k in o.rand64_stream((int(seed) ^ GOSS_STREAM) & MASK, trees)]


def uniform(key: int, ids) -> np.ndarray:
    """u of the original instance ids under the tree key (exact: 53 bits times 2^-53)."""
    return xm.gamma(key, ids)


def plan(n_t: int, a: float, b: float):
    """(n_top, p, amp)."""
    a, b = np.float64(a), np.float64(b)
    return sm.count(int(n_t), float(a)), float(b / (np.float64(1.0) - a)), float((np.float64(1.0) - a) / b)


def bit_keys(lam) -> np.ndarray:
    return np.abs(np.asarray(lam, dtype=np.float64)).view(np.uint64)


def select(lam_list, ids_list, a, b, key):
    """lam_list / ids_list: lambda and original instance id of every entry of L, in list order.  Returns (kept: indices into
    L ascending, is_top per kept entry, tau, amp)."""
    k = bit_keys(lam_list)
    n_t = len(k)
    n_top, p, amp = plan(n_t, a, b)
    tau = int(np.sort(k)[n_t - n_top])
    above = k > np.uint64(tau)
    ties = np.flatnonzero(k == np.uint64(tau))
    top = above.copy()
    top[ties[: n_top - int(above.sum())]] = True
    keep = top | (uniform(key, ids_list) < p)
    kept = np.flatnonzero(keep)
    return kept, top[kept], tau, amp


def goss_list(lam, L, order_ids, a, b, key):
    """lam by instance id; L: the tree's list as indices into the full instance list `order_ids`.  Returns (rows: the GOSS
    list as full-list indices, is_top, tau, amp)."""
    L = np.asarray(L, dtype=np.int64)
    ids = np.asarray(order_ids, dtype=np.int64)[L]
    kept, top, tau, amp = select(np.asarray(lam, dtype=np.float64)[ids], ids, a, b, key)
    return L[kept], top, tau, amp


def amplified(lam, wt, order_ids, rows, top, amp):
    """(lambda', w') by instance id: the kept others of the GOSS list multiplied by amp, everything else as it was."""
    lam2, wt2 = np.array(lam, dtype=np.float64), np.array(wt, dtype=np.float64)
    others = np.asarray(order_ids, dtype=np.int64)[np.asarray(rows, dtype=np.int64)[~np.asarray(top, dtype=bool)]]
    lam2[others] = lam2[others] * np.float64(amp)
    wt2[others] = wt2[others] * np.float64(amp)
    return lam2, wt2


def tree(X, lam, wt, order_ids, feats, binned, L, fsel, max_depth, min_leaf, k, a, b, key, max_leaves=0, monotone=None,
         lambda_l2=0.0, min_sum_hessian=0.0, min_split_gain=0.0):
    """The GOSS tree for gradients lam / wt (by instance id) of the list L (full-list indices) and the feature sample fsel
    (indices into `feats`); binned = (edges, xbin) of the FULL lists.  Returns (tree, rows, is_top)."""
    rows, top, _, amp = goss_list(lam, L, order_ids, a, b, key)
    lam2, wt2 = amplified(lam, wt, order_ids, rows, top, amp)
    newton = dict(lambda_l2=lambda_l2, min_sum_hessian=min_sum_hessian, min_split_gain=min_split_gain)
    common = (X, lam2, wt2, order_ids, feats, binned, rows, fsel, max_depth, min_leaf, k)
    if monotone and any(int(c) != 0 for c in monotone.values()):
        t = mm.tree_on_sample(*common, {int(f): int(c) for f, c in monotone.items()}, max_leaves, **newton)[0]
    elif max_leaves:
        t = lw.tree_on_sample(*common, max_leaves, split_gain="newton", **newton)
    else:
        t = nm.tree_on_sample(*common, **newton)
    return t, rows, top
