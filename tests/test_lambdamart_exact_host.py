"""The LambdaRank gradient pass held to exact arithmetic (tests/lambdamart_exact.py), on the CPU.

Three independent properties; each fails for its own class of mistake that the restatement (tests/lambdamart_model.py)
and the kernel could share, because they were written together:

  1. accuracy: `lm.gradients` lies within a derived bound of the exact value (wrong formula, wrong order of magnitude);
  2. `delta_ij` is what the C oracle's NDCG evaluator changes by when i and j swap ranks (tie order, `@k` cut, norm);
  3. `lambda = -dC/ds`, `w = d2C/ds2` of the pairwise cost with `delta` frozen (sign and scale).

The bound of property 1 is derived, operation by operation, in the docstring of tests/lambdamart_bound.py (its one home:
the GPU test holds the kernel to the same function); no constant in it was adjusted after seeing a result.  The worst
error / bound seen is printed (and recorded in profiles/lm_fuzz.txt).
"""
import decimal
from decimal import Decimal

import numpy as np
import pytest

from oracle import pyoracle as o
from tests import lambdamart_exact as ex
from tests import lambdamart_model as lm
from tests.lambdamart_bound import (C, MEASURES, SIGMAS, SLACK, U, WEIGHTS, as_dataset, check_dataset, designed_queries, gradient_bound,
                                    random_queries)


# --- 1. accuracy ---------------------------------------------------------------------------------------------------------

def _restatement_against_exact(queries, combos, scores_of=None):
    X, y, qid = as_dataset(queries)
    c = o.Dataset(X, y, qid)
    scores = c.score_linear(WEIGHTS) if scores_of is None else scores_of(X)
    worst = 0.0
    for measure, sigma in combos:
        norms = c.default_norms(measure)
        lam, wt = lm.gradients(scores, y, lm.query_lists(c), norms, lm.depth_of(measure), sigma)
        worst = max(worst, check_dataset(c, scores, y, lam, wt, measure, sigma, norms))
    return worst


def test_restatement_within_bound_of_exact_on_designed_queries():
    worst = _restatement_against_exact(designed_queries(), [(m, s) for m in MEASURES for s in SIGMAS])
    print("designed queries: worst error / bound = %.4f" % worst)
    # the signed zeros as scores themselves (a linear model's sum would turn -0.0 into +0.0)
    zeros = [t for t in designed_queries() if t[0] == "signed zeros"]
    worst = _restatement_against_exact(zeros, [("ndcg", 1.0), ("ndcg@10", 1.5)], scores_of=lambda X: X[:, 0].astype(np.float64))
    print("signed-zero scores: worst error / bound = %.4f" % worst)


@pytest.mark.parametrize("seed", [1, 2])
def test_restatement_within_bound_of_exact_on_random_queries(seed):
    rng = np.random.default_rng(100 + seed)
    queries = random_queries(seed, 24)
    worst = 0.0
    for t in queries:  # one depth and one sigma per query
        measure, sigma = MEASURES[int(rng.integers(0, 4))], float(rng.choice(SIGMAS + [0.05, 4.0]))
        worst = max(worst, _restatement_against_exact([t], [(measure, sigma)]))
    print("random queries (seed %d): worst error / bound = %.4f" % (seed, worst))


def test_saturated_wrongly_ordered_pair_shows_the_cancellation():
    """The case the rho mass is there for: 1 - rho is 0 in f64 while the exact term is sigma^2 exp(x) delta > 0; and the
    denormal case: the exact lambda of a rightly ordered saturated pair is a number f64 cannot hold."""
    scores, y, ids = np.array([0.0, 800.0]), np.array([1.0, 0.0]), np.array([0, 1])
    q = ex.ExactQuery(scores, y, ids, None, 1.0)
    lam, wt = lm.gradients(scores, y, [ids], [float(q.Z)], None, 1.0)
    el, ew, bl, bw = gradient_bound(q, 0)
    assert wt[0] == 0.0 and 0 < ew < Decimal("1e-340") and ew <= bw
    assert abs(ex.dec(lam[0]) - el) <= bl and el > Decimal("0.1")
    q = ex.ExactQuery(scores[::-1].copy(), y, ids, None, 1.0)
    lam, wt = lm.gradients(scores[::-1].copy(), y, [ids], [float(q.Z)], None, 1.0)
    el, ew, bl, bw = gradient_bound(q, 0)
    assert lam[0] == 0.0 and 0 < el < Decimal("1e-340") and el <= bl < Decimal("1e-300")


# --- 2. delta is the evaluator's NDCG change -----------------------------------------------------------------------------

def _ndcg_terms(q, rank):
    """T = sum over the documents inside the cut of (|G| + 2^g) D(r): what one evaluation's rounding errors scale with
    (per term: pow 4u of 2^g, the subtraction, log2, the division: at most 6u (|G| + 2^g) D; the sequential sum gamma_L)."""
    return sum((abs(q.G[p]) + q.G[p] + 1) * (ex.discount(rank[p]) if rank[p] < q.k else 0) for p in range(q.m))


@pytest.mark.parametrize("measure", ["ndcg", "ndcg@1", "ndcg@3", "ndcg@10", "ndcg@5000"])
@pytest.mark.parametrize("norm_kind", ["default", "qrel"])
def test_delta_is_the_evaluators_ndcg_change(measure, norm_kind):
    """|NDCG(ranking with i and j swapped) - NDCG(ranking)| from the C oracle's evaluator equals the exact delta_ij.
    The current ranking is evaluated with the (tied) scores themselves: the oracle's comparator places the ties.  The
    swapped ranking is realised by distinct scores m - rank.  Tolerance, absolute: each evaluation is a sequential f64 sum
    of L terms, each carrying at most 6u and the division by Z one more: gamma_(L + 7) T / Z per evaluation (the form of
    tests/test_error_bound.py); the default norm Z is such a sum itself, so the difference scales by 1 +- gamma_(L + 7)
    T_ideal / Z on top."""
    rng = np.random.default_rng(11)
    m = 30
    labels = [rng.choice(s, m).astype(np.float64) for s in ([0, 1, 2, 3, 4], [0, 0.5, 1, 2], [0, 1, 30], [-1, 0, 1, 2])]
    X = np.zeros((m * len(labels), 1), dtype=np.float32)
    y = np.concatenate(labels)
    qid = np.repeat(np.arange(1, len(labels) + 1, dtype=np.int64), m)
    scores = np.floor(rng.exponential(2.0, len(y)))  # many ties, all gains inside a tie group
    scores[:m][:6] = 0.0
    c = o.Dataset(X, y, qid)
    depth = lm.depth_of(measure)
    if norm_kind == "qrel":  # judgments that know more relevant documents than the query holds: a larger norm
        qrel = {str(k + 1): {"d%d" % i: float(g) for i, g in enumerate(list(labels[k]) + [4.0, 3.0, 3.0])} for k in range(len(labels))}
        norms = c.qrel_norms(measure, qrel)
    else:
        norms = c.default_norms(measure)
    base, err = c.metric_from_scores(measure, scores, norms)
    assert err == 0
    checked = 0
    for k, ids in enumerate(lm.query_lists(c)):
        q = ex.ExactQuery(scores[ids], y[ids], ids, depth, 1.0, None if norm_kind == "default" else norms[k])
        assert q.live
        L = q.k if depth is not None else q.m
        gamma = (L + 7) * U / (1 - (L + 7) * U)
        by_gain = sorted(range(m), key=lambda p: -q.g[p])
        ideal_rank = [0] * m
        for pos, p in enumerate(by_gain):
            ideal_rank[p] = pos
        rel_z = gamma * _ndcg_terms(q, ideal_rank) / q.Z if norm_kind == "default" else Decimal(0)
        pairs = [(int(a), int(b)) for a, b in rng.integers(0, m, (40, 2)) if a != b]
        # ... and pairs inside one tie group, and across the cut
        by_rank = sorted(range(m), key=lambda p: q.rank[p])
        if 0 < q.k < m:
            pairs += [(by_rank[q.k - 1], by_rank[q.k]), (by_rank[0], by_rank[q.k])]
        tied = [p for p in range(m) if scores[ids[p]] == scores[ids[by_rank[m // 2]]]]
        pairs += [(tied[0], tied[-1])] if len(tied) > 1 else []
        for i, j in pairs:
            rank2 = list(q.rank)
            rank2[i], rank2[j] = q.rank[j], q.rank[i]
            swapped = scores.copy()
            swapped[ids] = [float(m - r) for r in rank2]
            got, err = c.metric_from_scores(measure, swapped, norms)
            assert err == 0
            change = abs(ex.dec(got[k]) - ex.dec(base[k]))
            delta = q.delta(i, j) if q.g[i] != q.g[j] else Decimal(0)
            tol = gamma * (_ndcg_terms(q, q.rank) + _ndcg_terms(q, rank2)) / q.Z + SLACK * rel_z * delta
            assert abs(change - delta) <= tol, (measure, k, i, j, float(change), float(delta), float(tol))
            checked += 1
    assert checked > 100


# --- 3. lambda and w are the cost's derivatives --------------------------------------------------------------------------

@pytest.mark.parametrize("sigma", [0.3, 1.0, 1.5])
@pytest.mark.parametrize("depth", [None, 2])
def test_lambda_and_w_are_first_and_second_derivatives(sigma, depth):
    """With delta frozen at the current ranking, C(s) = sum over pairs (h, l) of delta_hl log(1 + exp(-sigma (s_h - s_l)))
    (DESIGN.md section 11 carries this sign convention: lambda is the NEGATIVE gradient, the direction scores should
    move).  lambda_p = -dC/ds_p and w_p = d2C/ds_p2, by symmetric differences at 60 digits with step h = 1e-12: the
    truncation error is h^2 times a fourth / third derivative, about 1e-24 sigma^4 sum delta, the rounding error
    1e-60 / h^2 = 1e-36; the tolerance is 1e-20 (sigma + sigma^4 + 1) sum delta."""
    rng = np.random.default_rng(5)
    m = 7
    scores = np.round(rng.normal(0, 2, m), 1)
    scores[3] = scores[4]  # a tie
    y = np.array([0, 2, 1, 0.5, 3, 0, 1], dtype=np.float64)
    q = ex.ExactQuery(scores, y, np.arange(m), depth, sigma)
    h = Decimal("1e-12")
    total = sum(q.delta(a, b) for a in range(m) for b in range(m) if q.g[a] > q.g[b])
    tol = Decimal("1e-20") * (q.sigma + q.sigma ** 4 + 1) * total
    c0 = q.cost()
    nonzero = 0
    with decimal.localcontext(C):  # (the operators below at 60 digits, not the default 28)
        for p in range(m):
            up, dn = list(q.s), list(q.s)
            up[p], dn[p] = q.s[p] + h, q.s[p] - h
            cu, cd = q.cost(up), q.cost(dn)
            lam, w = q.document(p)
            assert abs(lam - (-(cu - cd) / (2 * h))) <= tol, p
            assert abs(w - (cu - 2 * c0 + cd) / (h * h)) <= tol, p
            nonzero += lam != 0
    assert nonzero >= 2
    # ... and the restatement carries the same sign and scale (property 1 holds it to the digits)
    lam64, w64 = lm.gradients(scores, y, [np.arange(m)], [float(q.Z)], depth, sigma)
    for p in range(m):
        lam, w = q.document(p)
        assert abs(ex.dec(lam64[p]) - lam) <= Decimal("1e-12") * (abs(lam) + 1) and abs(ex.dec(w64[p]) - w) <= Decimal("1e-12") * (w + 1)
