"""numpy restatement of the LambdaRank truncation level and per-query normalisation ("Truncation and
normalisation"), for the tests.  Built on tests/lambdamart_model.py: the same ranks, gains, discounts, pair terms and
sequential sums (np.cumsum); what is added is the pair mask, A, S and f.

  * pair mask: document i's partner j counts iff the labels differ and min(r_i, r_j) < T (T = 0: every rank is inside);
  * lambda_i, w_i, A_i: the masked terms +-t, sigma^2 rho (1 - rho) delta and t, each summed sequentially over the partners
    in the query's stored order (a masked-out partner adds +0.0, which changes no bit: no sum here is ever -0.0);
  * S_q: the A_i summed sequentially in stored order; under lambda_norm and S_q > 0 every lambda_i and w_i of the query is
    multiplied by f = log2(1 + S_q) / S_q.
"""
import math

import numpy as np

from tests import lambdamart_model as lm


def ranks(s, g, ids):
    """0-based ranks in the RankedInstance order (score descending, gain ascending, id ascending), as lm.gradients has them."""
    m = len(ids)
    order = sorted(range(m), key=lambda i: (-s[i], g[i], ids[i]))
    rank = np.empty(m, dtype=np.int64)
    rank[order] = np.arange(m)
    return rank


def pair_mask(g, rank, i, truncation_level):
    """Which partners of document i contribute."""
    other = g != g[i]
    if truncation_level == 0:
        return other
    return other & (np.minimum(rank, rank[i]) < truncation_level)


def scale(S):
    """f of a query whose pair mass is S (1.0: nothing is scaled)."""
    return math.log2(1.0 + S) / S if S > 0.0 else 1.0


def gradients(scores, y, queries, norms, depth=None, sigma=1.0, truncation_level=0, lambda_norm=False, parts=False):
    """lambda, w by instance id.  parts=True: also A by instance id (before any scaling) and S, f per query."""
    n = len(y)
    lam = np.zeros(n, dtype=np.float64)
    wt = np.zeros(n, dtype=np.float64)
    A = np.zeros(n, dtype=np.float64)
    S_q = np.zeros(len(queries), dtype=np.float64)
    f_q = np.ones(len(queries), dtype=np.float64)
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
        rank = ranks(s, g, ids)
        k = m if depth is None else depth
        D = np.array([1.0 / math.log2(r + 2.0) if r < k else 0.0 for r in rank], dtype=np.float64)
        for i in range(m):
            keep = pair_mask(g, rank, i, truncation_level)
            high = g[i] > g
            diff = np.where(high, s[i] - s, s - s[i])
            delta = np.abs(G[i] - G) * np.abs(D[i] - D) / z
            with np.errstate(over="ignore"):
                rho = 1.0 / (1.0 + np.exp(sigma * diff))
            t = sigma * rho * delta
            lam[ids[i]] = lm.seq_sum(np.where(keep, np.where(high, t, -t), 0.0))
            wt[ids[i]] = lm.seq_sum(np.where(keep, sigma2 * rho * (1.0 - rho) * delta, 0.0))
            A[ids[i]] = lm.seq_sum(np.where(keep, t, 0.0))
        S_q[q] = lm.seq_sum(A[ids])
        if lambda_norm and S_q[q] > 0.0:
            f_q[q] = scale(float(S_q[q]))
            lam[ids] = lam[ids] * f_q[q]
            wt[ids] = wt[ids] * f_q[q]
    if parts:
        return lam, wt, A, S_q, f_q
    return lam, wt
