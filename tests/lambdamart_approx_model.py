"""The ApproxNDCG objective ("ApproxNDCG objective") for the tests, twice, and the bound between them.
Shared by tests/test_lambdamart_approx_host.py, tests/test_gpu_lambdamart_approx.py and
tests/test_gpu_neural_lambdarank_approx.py; not a test file itself.

`query_gradients`: numpy f64 in the definition's order -- one chain per document, from +0.0, partners in ascending stored
order, every operation rounded where the definition writes it.  What lambda_grad_approx_kernel computes, bit for bit wherever
`exp` and `log2` are exact.

`ExactApprox`: 60-digit `decimal`, objective and gradient, from the same formulas; every sum is exact (a 2 000-digit context),
the scores, gains, norm and alpha enter as the exact values of their f64.  `exact_objective` takes Decimal scores, so that a
finite difference can step by 1e-20.

`ApproxBound`: |f64 lambda - exact| per document, operation by operation; u = 2^-53, every quantity carries an absolute error.
  rounding  r = fl(x op y) adds u (|r| + propagated error) + ETA;  product  d(xy) <= |x| dy + |y| dx + dx dy.
  q_ij      d = fl(s_j - s_i), t = fl(alpha d); e = exp(-t) is off by a relative dt (1 + 2 dt) from its argument plus the
            library's LIB = 4u (2 ulp, ASSUMED as in tests/lambdamart_xendcg_bound.py; the same figure is charged to log2);
            D = fl(1 + e), q = fl(1 / D) is off by q dD / (D - dD) plus its rounding; q_ji = fl(1 - q), p = fl(q q_ji).
            |t| above 700 is outside the bound's domain (exp would leave the normal range).
  chains    a term passes through at most m = n - 1 additions: d chain <= sum dx + g_m sum (|x| + dx), g_m = m u / (1 - m u).
  c_i       r = fl(1 + chain), x = fl(1 + r); the error of r reaches l = log2(x) through the derivative 1 / (x ln 2), charged
            at the near end of x's interval: dl = dx / ((x - dx) ln 2), plus LIB (l + that).  g = fl(G / N);
            den = fl(fl(x LN2) fl(l l)) by the product rule (the f64 LN2 is off by u ln 2);
            c = -fl(g / den) is off by (dg + |g / den| dden) / (den - dden) plus its rounding.  x >= 2, so l >= 1.
  lambda_k  fl(c_i - c_k) is off by dc_i + dc_k + u |c_i - c_k|: absolute, so the cancellation costs what the c are worth,
            at most (|c_i| + |c_k|) times their relative errors, and through the product with p_ik and the chain this is the
            alpha sum_i (|c_i| + |c_k|) p_ik scale; then the chain rule above and fl(alpha chain).
No constant was adjusted after seeing a result.
"""
import decimal
from decimal import Decimal

import numpy as np

from tests import lambdamart_exact as ex
from tests.lambdamart_xendcg_bound import ETA, ETA_EXP, LIB, U, _mul, _rnd

CTX, SUM = ex.CTX, ex.SUM
ZERO, ONE = Decimal(0), Decimal(1)
LN2 = float.fromhex("0x1.62e42fefa39efp-1")
LN2D = CTX.ln(Decimal(2))


def query_gradients(s, G, N, alpha):
    """(lambda, A) of one query in f64: scores s, gains G = 2^label - 1, norm N, steepness alpha."""
    s, G = np.asarray(s, dtype=np.float64), np.asarray(G, dtype=np.float64)
    n = len(s)
    if n < 2 or not (N > 0.0):
        return np.zeros(n), 0.0
    t = np.float64(alpha) * (s[None, :] - s[:, None])  # [i, j]: alpha (s_j - s_i)
    with np.errstate(over="ignore"):
        q = 1.0 / (1.0 + np.exp(-t))
    up = np.triu(np.ones((n, n), dtype=bool), 1)
    Q = np.where(up, q, 1.0 - q.T)          # q_ij: the upper triangle as computed, the lower mirrored
    p = q * (1.0 - q)
    P = np.where(up, p, p.T)
    idx = np.arange(n)
    chain = np.zeros(n)
    for j in range(n):
        m = idx != j
        chain[m] = chain[m] + Q[m, j]
    r = 1.0 + chain
    x = 1.0 + r
    l = np.log2(x)
    c = -((G / np.float64(N)) / ((x * LN2) * (l * l)))
    chain = np.zeros(n)
    for i in range(n):
        m = idx != i
        chain[m] = chain[m] + (c[i] - c[m]) * P[m, i]
    return np.float64(alpha) * chain, float(np.sum(G / l) / N)


def gradients(scores, G, queries, norms, alpha):
    """lambda by instance id over `queries` (lists of ids in stored order), and the mean objective."""
    lam, total = np.zeros(len(scores)), 0.0
    for ids, N in zip(queries, norms):
        lam[ids], A = query_gradients(scores[ids], G[ids], N, alpha)
        total += A
    return lam, total / len(queries)


def exact_objective(s, G, N, alpha) -> Decimal:
    """A of Decimal scores s, gains G, norm N, steepness alpha (call under CTX)."""
    n = len(s)
    chain = [ZERO] * n
    for i in range(n):
        for j in range(i + 1, n):
            q = CTX.divide(ONE, CTX.add(ONE, CTX.exp(-CTX.multiply(alpha, SUM.subtract(s[j], s[i])))))
            chain[i] = SUM.add(chain[i], q)
            chain[j] = SUM.add(chain[j], SUM.subtract(ONE, q))
    acc = ZERO
    for Gi, ch in zip(G, chain):
        acc = SUM.add(acc, CTX.divide(CTX.multiply(Gi, LN2D), CTX.ln(SUM.add(Decimal(2), ch))))
    return CTX.divide(acc, N)


class ExactApprox:
    """One live query (n >= 2, N > 0) in 60-digit arithmetic: s, G (f64 arrays), N, alpha (floats)."""

    def __init__(self, s, G, N, alpha):
        with decimal.localcontext(CTX):
            self.n = n = len(s)
            self.s, self.G = [ex.dec(v) for v in s], [ex.dec(v) for v in G]
            self.N, self.alpha = ex.dec(N), ex.dec(alpha)
            self.e = [[None] * n for _ in range(n)]   # exp(-t) of i < j
            self.Q = [[ZERO] * n for _ in range(n)]   # q_ij, every i != j
            self.P = [[ZERO] * n for _ in range(n)]
            for i in range(n):
                for j in range(i + 1, n):
                    e = CTX.exp(-CTX.multiply(self.alpha, SUM.subtract(self.s[j], self.s[i])))
                    q = CTX.divide(ONE, CTX.add(ONE, e))
                    self.e[i][j], self.Q[i][j], self.Q[j][i] = e, q, SUM.subtract(ONE, q)
                    self.P[i][j] = self.P[j][i] = CTX.multiply(q, self.Q[j][i])
            self.chain = [sum(row, ZERO) for row in self.Q]
            self.x = [SUM.add(Decimal(2), ch) for ch in self.chain]
            self.l = [CTX.divide(CTX.ln(x), LN2D) for x in self.x]
            self.g = [CTX.divide(Gi, self.N) for Gi in self.G]
            self.den = [CTX.multiply(CTX.multiply(x, LN2D), CTX.multiply(l, l)) for x, l in zip(self.x, self.l)]
            self.c = [-CTX.divide(g, d) for g, d in zip(self.g, self.den)]
            self.chain2 = [sum((CTX.multiply(SUM.subtract(self.c[i], self.c[k]), self.P[i][k]) for i in range(n) if i != k), ZERO) for k in range(n)]
            self.lam = [CTX.multiply(self.alpha, ch) for ch in self.chain2]
            self.A = CTX.divide(sum((CTX.divide(Gi, l) for Gi, l in zip(self.G, self.l)), ZERO), self.N)


class ApproxBound:
    """dlam[k] >= |f64 lambda_k - exact| for the ExactApprox query e (the module docstring)."""

    def __init__(self, e):
        with decimal.localcontext(CTX):
            self._derive(e)

    def _derive(self, e):
        n, a = e.n, e.alpha
        m = n - 1
        gm = m * U / (1 - m * U)
        dQ = [[ZERO] * n for _ in range(n)]
        dP = [[ZERO] * n for _ in range(n)]
        for i in range(n):
            for j in range(i + 1, n):
                d = e.s[j] - e.s[i]
                dt = _mul(a, ZERO, d, _rnd(d, ZERO))
                if abs(a * d) + dt > 700:
                    raise ValueError("alpha |s_j - s_i| above 700: no bound")
                de = e.e[i][j] * (dt * (1 + 2 * dt) + LIB) + ETA_EXP
                D = 1 + e.e[i][j]
                q, qm = e.Q[i][j], e.Q[j][i]
                dq = _rnd(q, q * _rnd(D, de) / (D - _rnd(D, de)))
                dqm = _rnd(qm, dq)
                dQ[i][j], dQ[j][i] = dq, dqm
                dP[i][j] = dP[j][i] = _mul(q, dq, qm, dqm)
        dc = []
        for i in range(n):
            dchain = sum(dQ[i]) + gm * (sum(e.Q[i]) + sum(dQ[i]))
            dx = _rnd(e.x[i], _rnd(e.x[i] - 1, dchain))
            near = dx / ((e.x[i] - dx) * LN2D)
            dl = near + LIB * (e.l[i] + near)
            dxl = _mul(e.x[i], dx, LN2D, U * LN2D)
            dll = _mul(e.l[i], dl, e.l[i], dl)
            dden = _mul(e.x[i] * LN2D, dxl, e.l[i] * e.l[i], dll)
            quot = abs(e.c[i])
            dc.append(_rnd(quot, (_rnd(e.g[i], ZERO) + quot * dden) / (e.den[i] - dden)))
        self.dlam = []
        for k in range(n):
            terms = dterms = ZERO
            for i in range(n):
                if i == k:
                    continue
                diff = e.c[i] - e.c[k]
                dterm = _mul(diff, _rnd(diff, dc[i] + dc[k]), e.P[i][k], dP[i][k])
                terms, dterms = terms + abs(diff * e.P[i][k]), dterms + dterm
            self.dlam.append(_mul(a, ZERO, e.chain2[k], dterms + gm * (terms + dterms)))


def worst_ratio(e, lam):
    """Asserts |lam_k - exact| <= bound for every document of the ExactApprox e; returns the worst error / bound."""
    bound = ApproxBound(e)
    worst = 0.0
    for k in range(e.n):
        assert np.isfinite(lam[k]), k
        err = abs(ex.dec(lam[k]) - e.lam[k])
        assert err <= bound.dlam[k], "lambda of document %d of %d: |%r - exact| = %.3e > bound %.3e" % (k, e.n, float(lam[k]), err, bound.dlam[k])
        worst = max(worst, float(err / bound.dlam[k]))
    return worst
