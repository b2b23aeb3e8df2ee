"""The error bound that holds an f64 LambdaRank gradient pass to exact arithmetic (tests/lambdamart_exact.py), the inputs
it is checked on, and the loop that checks a dataset.  Shared by tests/test_lambdamart_exact_host.py (the restatement, CPU)
and tests/test_gpu_lambdamart.py (the kernel); not a test file itself.

The bound (`gradient_bound`), from the operations the definition performs, to first
order in u = 2^-53 (a factor 1 + 2^-20 covers the products of two such terms: every relative error below is under 1e-9).
Library functions (`exp`, and the `log2` / `pow` behind the discount table and the gains): the ROCm device-library
documentation that ships with the toolchain states no ulp bound for f64 `exp`, so K = 2 ulp is ASSUMED, for every library
function and on both the CPU and the device side; an ulp is at most 2u relative, so a library result carries 2Ku = 4u.

  inputs   s, sigma, Z and the f32 label are exact.  G = fl(fl(2^g) - 1): exact for an integer label, else off by at most
           eG = 4u 2^g + u |G|.  D = fl(1 / fl(log2(r + 2))): relative 4u + u = 5u (D = 0 beyond the cut: exact).
  delta  = fl(fl(fl|G_i - G_j| * fl|D_i - D_j|) / Z): two subtractions, a product, a division: 4u, plus the inputs' errors
           amplified by the subtractions: a_G = (eG_i + eG_j) / |G_i - G_j|, a_D = 5u (D_i + D_j) / |D_i - D_j| (adjacent
           ranks far down a long list cancel; this is the definition's own conditioning, not slack).
           e_delta = a_G + a_D + 4u.
  rho    = fl(1 / fl(1 + exp(fl(sigma * fl(s_h - s_l))))): the argument x carries 2u relative, so exp(x) carries
           2u |x| (argument) + 4u (library); 1 + e and the division add 2u.  e_rho = (2 |x| + 6) u.
  t      = fl(fl(sigma * rho) * delta): e_t = e_rho + e_delta + 2u.
  lambda = the terms added one after the other, at most m - 1 additions: gamma_m = m u / (1 - m u) of sum |t|.
           |lambda - exact| <= (1 + 2^-20) sum_j |t_ij| (e_t,ij + gamma_m) + sum_j eta_ij.
  w      : the term is fl(fl(fl(fl(sigma sigma) rho) fl(1 - rho)) delta).  fl(1 - rho) is off by rho e_rho + u (1 - rho) in
           ABSOLUTE terms: for a wrongly ordered saturated pair rho -> 1 and 1 - rho = exp(x) is lost entirely.  So the
           term's error is sigma^2 delta rho [(1 - rho)(e_rho + e_delta + 5u) + rho e_rho] <= sigma^2 delta rho (e_rho +
           e_delta + 5u): measured against the mass sum sigma^2 rho delta, not sum sigma^2 rho (1 - rho) delta.
           |w - exact| <= (1 + 2^-20) sum_j sigma^2 rho_ij delta_ij (e_rho + e_delta + 5u + gamma_m) + sum_j eta_ij.
  eta    : absolute, per pair, for results below the smallest normal.  exp overflows to inf (rho = 0) only where the true
           rho < 2^-1023; a denormal result is off by at most 2^-1075.  Through the remaining factors:
           eta_lambda = 2^-1023 sigma delta + 2^-1075 (delta + 1 + sigma (1 + 1/Z)),
           eta_w      = 2^-1023 sigma^2 delta + 2^-1075 (2 delta + 1 + sigma^2 (1 + 1/Z)).
           With well-separated scores and a depth cut every term of a document can be denormal; then eta is the bound.

No constant above was adjusted after seeing a result.  The worst error / bound seen is printed (and recorded in
profiles/lm_fuzz.txt).
"""
import decimal
from decimal import Decimal

import numpy as np
from tests import lambdamart_exact as ex
from tests import lambdamart_model as lm

U = Decimal(2) ** -53
K_ULP = 2                      # assumed: see the module docstring
LIB = 2 * K_ULP * U            # relative error of one library-function result
SLACK = 1 + Decimal(2) ** -20  # second-order terms
ETA_RHO = Decimal(2) ** -1023
ETA_DEN = Decimal(2) ** -1075
C = ex.CTX

MEASURES = ["ndcg", "ndcg@1", "ndcg@10", "ndcg@5000"]
SIGMAS = [0.3, 1.0, 1.5]


def _gain_error(g, G):
    return Decimal(0) if float(g).is_integer() else LIB * (G + 1) + U * abs(G)


def gradient_bound(q, i):
    """(lambda, w, bound on |lambda - .|, bound on |w - .|) of document i of the ExactQuery q, all Decimal."""
    with decimal.localcontext(C):
        return _gradient_bound(q, i)


def _gradient_bound(q, i):
    pairs = list(q.pairs(i))
    lam, w = q.document(i, pairs)
    m, sigma = q.m, q.sigma
    s2 = sigma * sigma
    gamma = m * U / (1 - m * U)
    rel_l = rel_w = eta_l = eta_w = Decimal(0)
    for p in pairs:
        a_g = C.divide(_gain_error(q.g[i], p.Gi) + _gain_error(q.g[p.j], p.Gj), abs(p.Gi - p.Gj))
        a_d = C.divide(5 * U * (p.Di + p.Dj), abs(p.Di - p.Dj))
        e_delta = a_g + a_d + 4 * U
        e_rho = (2 * abs(p.x) + 6) * U
        t = C.multiply(C.multiply(sigma, p.rho), p.delta)
        rel_l += C.multiply(t, e_rho + e_delta + 2 * U + gamma)
        rel_w += C.multiply(C.multiply(C.multiply(s2, p.rho), p.delta), e_rho + e_delta + 5 * U + gamma)
        inv_z = C.divide(1, q.Z)
        eta_l += ETA_RHO * sigma * p.delta + ETA_DEN * (p.delta + 1 + sigma * (1 + inv_z))
        eta_w += ETA_RHO * s2 * p.delta + ETA_DEN * (2 * p.delta + 1 + s2 * (1 + inv_z))
    return lam, w, C.add(SLACK * rel_l, eta_l), C.add(SLACK * rel_w, eta_w)


def worst_ratio(q, docs, lam, wt):
    """Asserts |got - exact| <= bound for the documents `docs` (indices into the query) of ExactQuery q, given the f64
    results lam / wt of the whole query; returns the worst error / bound."""
    worst = 0.0
    for i in docs:
        el, ew, bl, bw = gradient_bound(q, i)
        for name, got, exact, bound in (("lambda", lam[i], el, bl), ("w", wt[i], ew, bw)):
            assert np.isfinite(got), (name, i)
            err = abs(ex.dec(got) - exact)
            if bound == 0:
                assert got == 0.0 and exact == 0, (name, i, got, exact)
                continue
            assert err <= bound, "%s of document %d: |%r - exact| = %.3e > bound %.3e (m = %d, depth %r, sigma %s)" % (
                name, i, float(got), err, bound, q.m, q.depth, q.sigma)
            worst = max(worst, float(err / bound))
    return worst


def chosen_documents(q, limit=40):
    """Every document of a short query; of a long one the first and last stored, the cut's two sides (r = k - 1, k), the
    best and worst ranked, members of tie groups -- first of groups that hold different labels (two documents of
    different labels: the gain rule; a second one of the first label: the id rule), then of one-label groups -- and a
    spread of the rest."""
    if q.m <= limit:
        return list(range(q.m))
    by_rank = sorted(range(q.m), key=lambda p: q.rank[p])
    pick = [0, q.m - 1, by_rank[0], by_rank[-1]]
    if 0 < q.k < q.m:
        pick += [by_rank[q.k - 1], by_rank[q.k]]
    seen = {}
    for p in range(q.m):
        seen.setdefault(q.s[p], []).append(p)
    ties = [v for v in seen.values() if len(v) > 1]
    mixed = [v for v in ties if len({q.g[p] for p in v}) > 1]
    for v in mixed[:6]:
        other = next(p for p in v if q.g[p] != q.g[v[0]])
        same = [p for p in v[1:] if q.g[p] == q.g[v[0]]]
        pick += [v[0], other] + same[:1]
    for v in [v for v in ties if v not in mixed][:3]:
        pick += v[:2]
    step = max(1, q.m // max(1, limit - len(set(pick))))
    pick += list(range(q.m))[step // 2::step]
    out = []
    for p in pick:
        if p not in out:
            out.append(p)
    return out[:limit + 10]


def coverage(q, docs):
    """(the documents hold two of one score and different labels, they hold both sides of the cut or there is none)."""
    by_score = {}
    for p in docs:
        by_score.setdefault(q.s[p], set()).add(q.g[p])
    cut = True
    if 0 < q.k < q.m:
        at = {q.rank[p] for p in docs}
        cut = q.k - 1 in at and q.k in at
    return any(len(v) > 1 for v in by_score.values()), cut


# --- inputs ------------------------------------------------------------------------------------------------------------
# A query is (name, x [m, 2] f32, y [m]); its scores are the linear model WEIGHTS on x, so that the GPU test can hand the
# same queries to the device as one dataset (tests/test_gpu_lambdamart.py).
WEIGHTS = [1.0, 0.001]
LABEL_SETS = [[0, 1, 2, 3, 4], [0, 0.5, 1, 2], [0, 1, 30], [-1, 0, 0.5, 1, 2, 30]]


def designed_queries():
    rng = np.random.default_rng(2024)
    out = []

    def add(name, x0, y, x1=None):
        x = np.zeros((len(x0), 2), dtype=np.float32)
        x[:, 0] = x0
        if x1 is not None:
            x[:, 1] = x1
        out.append((name, x, np.asarray(y, dtype=np.float64)))

    m = 24
    mixed = rng.choice([0, 1, 2, 3, 4], m)
    add("all scores equal", np.full(m, 3.25), mixed)
    add("signed zeros", np.where(rng.random(m) < 0.5, -0.0, 0.0), mixed)
    # gaps that saturate both ways for every sigma in SIGMAS (0.3 * 3000 = 900 > 745), labels independent of the scores, so
    # rightly and wrongly ordered saturated pairs both occur; and three levels, so some pairs stay unsaturated
    add("saturated +-3000", rng.choice([-3000.0, 0.0, 3000.0], m), mixed)
    add("saturated +-800 with near ties", rng.choice([-800.0, 800.0], m) + rng.integers(0, 3, m), mixed, rng.integers(0, 4, m))
    add("well separated, hundreds apart", np.arange(m) * 150.0, rng.permutation(mixed))
    add("labels 0.5, -1, 30", rng.normal(0, 2, m), rng.choice([0.5, -1.0, 30.0], m), rng.integers(0, 4, m))
    one = np.zeros(m)
    one[rng.integers(0, m)] = 3.0
    add("one positive label", np.round(rng.normal(0, 2, m)), one, rng.integers(0, 2, m))
    add("two documents", [1.0, 2.0], [1, 0])
    add("two documents, tied", [1.0, 1.0], [0, 2])
    return out


def random_queries(seed, count):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        m = int(rng.choice([2, 3, 5, 17, 64, 150, 400]))
        scale = float(rng.choice([0.0, 1e-3, 1.0, 30.0, 400.0]))
        x = np.zeros((m, 2), dtype=np.float32)
        x[:, 0] = rng.normal(0, 1, m) * scale
        if rng.random() < 0.5:
            x[:, 0] = np.round(x[:, 0])  # tie groups
        x[:, 1] = rng.integers(0, 4, m)
        y = rng.choice(LABEL_SETS[int(rng.integers(0, len(LABEL_SETS)))], m).astype(np.float64)
        out.append(("random %d (m = %d, scale %g)" % (k, m, scale), x, y))
    return out


def as_dataset(queries):
    """(X, y, qid) holding the queries one after the other, qid = 1, 2, ..."""
    X = np.concatenate([x for _, x, _ in queries])
    y = np.concatenate([v for _, _, v in queries])
    qid = np.concatenate([np.full(len(v), k + 1, dtype=np.int64) for k, (_, _, v) in enumerate(queries)])
    return X, y, qid


def check_dataset(c, scores, y, lam, wt, measure, sigma, norms, limit=40, only=None, demand_ties_from=None):
    """Holds lam / wt (by instance id) to the exact statement, query by query of the oracle dataset c; returns the worst
    error / bound.  Of every query whose documents are not all checked, the chosen ones must hold both sides of the cut;
    of every live query of at least `demand_ties_from` documents they must also hold a tie group with different labels."""
    worst = 0.0
    for k, ids in enumerate(lm.query_lists(c)):
        if only is not None and k not in only:
            continue
        q = ex.ExactQuery(scores[ids], y[ids], ids, lm.depth_of(measure), sigma, norms[k])
        if not q.live:
            assert not lam[ids].any() and not wt[ids].any()
            continue
        docs = chosen_documents(q, limit)
        mixed_tie, cut = coverage(q, docs)
        assert cut, "query %d: the chosen documents miss r = k - 1 or r = k" % k
        if demand_ties_from is not None and q.m >= demand_ties_from:
            assert mixed_tie, "query %d (%d documents): no tie group with different labels among the chosen documents" % (k, q.m)
        worst = max(worst, worst_ratio(q, docs, lam[ids], wt[ids]))
    return worst
