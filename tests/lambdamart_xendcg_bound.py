"""The error bound that holds an f64 pass of LambdaMART's listwise objective (the numpy restatement
tests/lambdamart_xendcg_model.py, or lambda_grad_xe_kernel) to exact arithmetic (tests/lambdamart_xendcg_exact.py), the
inputs it is checked on, and the loop that checks a query.  Shared by tests/test_lambdamart_xendcg_host.py and
tests/test_gpu_lambdamart_xendcg.py; not a test file itself.

The bound (`XeBound`) follows the definition's operations one by one ("Listwise objective").  Every
quantity q carries an absolute error dq against its exact value; u = 2^-53.  Nothing is first order: the rules below bound
the f64 result's distance from the exact one for any size of the operands' errors, which matters because 1 / u_i can
amplify an error of 1e-16 beyond all bounds.
  rounding  a result r = fl(x op y) adds u (|r_exact| + the propagated error) and ETA = 2^-1074 for a result below the
            smallest normal.
  product   d(xy) <= |x| dy + |y| dx + dx dy.
  SUM       every element passes through at most A = ceil(n / 64) + 6 additions (its lane's chain, then the six tree
            steps): d SUM <= sum dx_i + g_A sum (|x_i| + dx_i), g_A = A u / (1 - A u).
  inputs    s and gamma are exact; gexp = fl(fl(2^g) - 1) is exact for an integer label, else off by 4u 2^g + u |gexp|
            (tests/lambdamart_bound.py's figure).  phi_i = fl(fl(gexp + 1) - gamma): two roundings on top.
  exp       the argument x_i = fl(s_i - m) is off by u |x_i|, which exp turns into a relative u |x_i| (1 + tiny); the
            ROCm device library states no ulp bound for f64 exp, so K = 2 ulp = 4u relative is ASSUMED, on both sides,
            as in tests/lambdamart_bound.py; a result below the smallest normal is off by at most 2 ulp of that range.
  rho_i     = fl(e_i / E): a quotient x / y with y > dy is off by at most (dx + |x / y| dy) / (y - dy).  E >= 1.
  u_i       = fl(1 - rho_i): du_i = drho_i + u u_i.  THE AMPLIFICATION: the f64 u_i is 0 or a multiple of 2^-53 whenever
            rho_i >= 1/2, and it lies in [u_i - du_i, u_i + du_i], so the divisor Q sees is 0 or at least
            u_lo = max(u_i - du_i, 2^-53).
  Q(x, i)   the f64 divisor is 0 (possible only if u_i <= du_i): the result is +0.0, off by |x / u_i|.  Otherwise
            |x~ / u~ - x / u_i| <= dx / u_lo + |x| du_i / (u_i u_lo).  dQ is the larger of the two cases (the second
            alone if u_i > du_i), plus the quotient's own rounding.
            Where rho_max is close to 1 this is the definition's own conditioning, charged here explicitly: the document
            on top has u_i of the order of du_i, a_i is off by as much as its own size, and that error reaches every other
            document through S1 and S2, scaled by rho_j.
  t1, t2, t3, lambda, w: products, differences and sums by the rules above.
No constant was adjusted after seeing a result.  The worst error / bound seen on the device is printed by the GPU test
(and recorded in profiles/lm_xendcg_grad_error.txt).
"""
import decimal
from decimal import Decimal

import numpy as np

from tests import lambdamart_exact as ex
from tests import lambdamart_xendcg_exact as xe

U = Decimal(2) ** -53
K_ULP = 2                       # assumed: see the module docstring
LIB = 2 * K_ULP * U             # relative error of one exp result
ETA = Decimal(2) ** -1074       # absolute error of a rounding below the smallest normal
ETA_EXP = K_ULP * ETA * 2       # ... of an exp result there
C = ex.CTX

N_DESIGNED = [2, 3, 63, 64, 65, 129, 1300]
SPREADS = [0.5, 5.0, 30.0]


def _rnd(value, err):
    """The error after rounding a result whose exact value is `value` and whose propagated error is `err`."""
    return err + U * (abs(value) + err) + ETA


def _mul(x, dx, y, dy):
    return _rnd(x * y, abs(x) * dy + abs(y) * dx + dx * dy)


def _gain_error(g, G):
    return Decimal(0) if float(g).is_integer() else LIB * (G + 1) + U * abs(G)


class XeBound:
    """Bounds on |lambda_i - exact| (`dlam`) and |w_i - exact| (`dw`) for every document of the live ExactXe query q."""

    def __init__(self, q):
        with decimal.localcontext(C):
            self._derive(q)

    def _derive(self, q):
        n = q.n
        A = (n + 63) // 64 + 6
        gA = A * U / (1 - A * U)

        def dsum(xs, dxs):
            return sum(dxs) + gA * sum(abs(x) + dx for x, dx in zip(xs, dxs))

        one = Decimal(1)
        # phi, Phi, inv
        dphi = []
        for g, G, phi in zip(q.g, q.G, q.phi):
            e1 = _rnd(G + 1, _gain_error(g, G))
            dphi.append(_rnd(phi, e1))
        dPhi = dsum(q.phi, dphi)
        inv = one / q.Phi
        if not dPhi < q.Phi:
            raise ValueError("Phi is not known to be positive in f64: no bound")
        dinv = _rnd(inv, inv * dPhi / (q.Phi - dPhi))
        # e, E, rho, u
        de = [e * ((U * abs(x)) * (1 + 2 * U * abs(x)) + LIB) + ETA_EXP for e, x in zip(q.e, q.x)]  # (exp(d) - 1 <= d (1 + 2d), d < 1/2)
        dE = dsum(q.e, de)
        drho = [_rnd(r, (d + r * dE) / (q.E - dE)) for r, d in zip(q.rho, de)]
        du = [d + U * ui + ETA for d, ui in zip(drho, q.u)]
        u_lo = [max(ui - d, U) for ui, d in zip(q.u, du)]

        def dQ(x, dx, i):
            quot = abs(x) / q.u[i]
            err = dx / u_lo[i] + abs(x) * du[i] / (q.u[i] * u_lo[i])
            err = _rnd(quot, err)
            if q.u[i] <= du[i]:
                err = max(err, quot)
            return err

        dt1 = []
        for i in range(n):
            dprod = _mul(q.phi[i], dphi[i], inv, dinv)
            dt1.append(_rnd(q.t1[i], dprod + drho[i]))
        da = [dQ(q.t1[i], dt1[i], i) for i in range(n)]
        dS1 = dsum(q.a, da)
        dt2 = []
        for i in range(n):
            diff = q.S1 - q.a[i]
            ddiff = _rnd(diff, dS1 + da[i])
            dt2.append(_mul(q.rho[i], drho[i], diff, ddiff))
        db = [dQ(q.t2[i], dt2[i], i) for i in range(n)]
        dS2 = dsum(q.b, db)
        self.dlam, self.dw = [], []
        for i in range(n):
            diff = q.S2 - q.b[i]
            ddiff = _rnd(diff, dS2 + db[i])
            dt3 = _mul(q.rho[i], drho[i], diff, ddiff)
            d12 = _rnd(q.t1[i] + q.t2[i], dt1[i] + dt2[i])
            self.dlam.append(_rnd(q.lam[i], d12 + dt3))
            self.dw.append(_mul(q.rho[i], drho[i], q.u[i], du[i]))


def worst_ratio(q, lam, wt):
    """Asserts |got - exact| <= bound for every document of the live ExactXe q, given the f64 results of the whole query;
    returns (the worst error / bound, the sum of the lambda bounds)."""
    bound = XeBound(q)
    worst = 0.0
    for i in range(q.n):
        for name, got, exact, b in (("lambda", lam[i], q.lam[i], bound.dlam[i]), ("w", wt[i], q.w[i], bound.dw[i])):
            assert np.isfinite(got), (name, i)
            err = abs(ex.dec(got) - exact)
            assert err <= b, "%s of document %d of %d: |%r - exact| = %.3e > bound %.3e" % (name, i, q.n, float(got), err, b)
            worst = max(worst, float(err / b))
    return worst, sum(bound.dlam)


# --- inputs ------------------------------------------------------------------------------------------------------------

def designed_queries():
    """(name, scores, labels) of the designed queries: every length with every score spread (scores uniform over the spread),
    and one document 800 above the rest."""
    rng = np.random.default_rng(406)
    out = []
    for n in N_DESIGNED:
        for spread in SPREADS:
            out.append(("n = %d, spread %g" % (n, spread), rng.random(n) * spread, rng.choice([0, 0, 1, 2, 3, 4], n).astype(np.float64)))
        s = rng.random(n)
        s[int(rng.integers(0, n))] += 800.0
        out.append(("n = %d, one score 800 above" % n, s, rng.choice([0, 1, 2, 3, 4], n).astype(np.float64)))
    return out
