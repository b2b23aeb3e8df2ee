"""numpy restatement of LambdaMART's MAP and MRR objectives ("Objectives"), for the tests.  Built on
tests/lambdamart_model.py and tests/lambdamart_trunc_model.py: the same ranks, rho, pair terms, sequential sums, pair
filter and scale; what is new is which documents pair up and the pair weight delta.

  * rel_i = (f32 gain > 0).  A pair is one relevant document h and one non-relevant document l, whatever their grades.
  * map: c[r] = relevant documents of rank <= r, P[r] = np.cumsum of 1 / (r' + 1) at the relevant ranks (0.0 at the others:
    adding +0.0 changes no bit), R_q = uint32(norm), or the list's own relevant count when that is 0.  With a = min(r_h, r_l),
    b = max, up = (r_l < r_h):  delta = |((c[a] + up) / (a + 1) - c[b] / (b + 1)) + (P[b - 1] - P[a])| / R_q.
  * mrr: f = the smallest relevant rank, f2 = the second smallest.  r_l < f: delta = 1 / (r_l + 1) - 1 / (f + 1);
    r_h == f: delta = 1 / (f + 1) - 1 / (min(f2, r_l) + 1); else 0.  The norm is not read.
It restates the definition, not the kernel: a sort for the ranks, np.cumsum for P, a delta table over all pairs.
"""
import numpy as np

from tests import lambdamart_model as lm
from tests import lambdamart_trunc_model as tm

OBJECTIVES = ("map", "mrr")


def delta_table(rank, rel, norm, objective, rows=None):
    """delta[i, j] for the documents of one query (any order), 0.0 where (i, j) is not a pair; None when the whole query
    has lambda = w = 0.  rank: 0-based ranks, rel: booleans, norm: the evaluator's norm of the query.  rows: only these i."""
    rank = np.asarray(rank, dtype=np.int64)
    rel = np.asarray(rel, dtype=bool)
    m = len(rank)
    by_rank = np.empty(m, dtype=bool)
    by_rank[rank] = rel
    rows = np.arange(m) if rows is None else np.asarray(rows, dtype=np.int64)
    pair = rel[rows, None] != rel[None, :]
    rh = np.where(rel[rows, None], rank[rows, None], rank[None, :])  # the relevant one's rank, the other's
    rl = np.where(rel[rows, None], rank[None, :], rank[rows, None])
    if objective == "map":
        R = int(np.uint32(norm))
        if R == 0:
            R = int(by_rank.sum())
        if R == 0:
            return None
        c = np.cumsum(by_rank.astype(np.int64))
        P = np.cumsum(np.where(by_rank, 1.0 / (np.arange(m) + 1).astype(np.float64), 0.0))
        a, b = np.minimum(rh, rl), np.maximum(rh, rl)
        up = (rl < rh).astype(np.int64)
        x = (c[a] + up).astype(np.float64) / (a + 1).astype(np.float64)
        y = c[b].astype(np.float64) / (b + 1).astype(np.float64)
        M = (x - y) + (P[np.maximum(b - 1, 0)] - P[a])  # (b = 0 only on the diagonal, which is no pair)
        return np.where(pair, np.abs(M) / float(R), 0.0)
    if objective == "mrr":
        at = np.flatnonzero(by_rank)
        if at.size == 0:
            return None
        f = int(at[0])
        f2 = int(at[1]) if at.size > 1 else None
        before = 1.0 / (rl + 1).astype(np.float64) - 1.0 / float(f + 1)
        mm = rl if f2 is None else np.minimum(f2, rl)
        first = 1.0 / float(f + 1) - 1.0 / (mm + 1).astype(np.float64)
        return np.where(pair & (rl < f), before, np.where(pair & (rl >= f) & (rh == f), first, 0.0))
    raise ValueError(objective)


def gradients(scores, y, queries, norms, objective, sigma=1.0, truncation_level=0, lambda_norm=False, parts=False):
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
        s = np.asarray(scores, dtype=np.float64)[ids]
        g = np.asarray(y, dtype=np.float32)[ids]
        rel = g > np.float32(0.0)
        rank = tm.ranks(s, g, ids)
        if delta_table(rank, rel, norms[q], objective, rows=[]) is None:
            continue
        for i in range(len(ids)):
            if i % 256 == 0:  # (a long query's table, 256 rows at a time)
                table = delta_table(rank, rel, norms[q], objective, rows=np.arange(i, min(i + 256, len(ids))))
            delta = table[i % 256]
            keep = delta != 0.0
            if truncation_level != 0:
                keep = keep & (np.minimum(rank, rank[i]) < truncation_level)
            high = np.full(len(ids), bool(rel[i]))
            diff = np.where(high, s[i] - s, s - s[i])  # s_h - s_l
            with np.errstate(over="ignore"):
                rho = 1.0 / (1.0 + np.exp(sigma * diff))
            t = sigma * rho * delta
            lam[ids[i]] = lm.seq_sum(np.where(keep, np.where(high, t, -t), 0.0))
            wt[ids[i]] = lm.seq_sum(np.where(keep, sigma2 * rho * (1.0 - rho) * delta, 0.0))
            A[ids[i]] = lm.seq_sum(np.where(keep, t, 0.0))
        S_q[q] = lm.seq_sum(A[ids])
        if lambda_norm and S_q[q] > 0.0:
            f_q[q] = tm.scale(float(S_q[q]))
            lam[ids] = lam[ids] * f_q[q]
            wt[ids] = wt[ids] * f_q[q]
    if parts:
        return lam, wt, A, S_q, f_q
    return lam, wt
