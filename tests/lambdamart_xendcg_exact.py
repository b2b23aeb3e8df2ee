"""LambdaMART's listwise objective ("Listwise objective") in `decimal` arithmetic, for the tests.

Written from the definition, with no f64 in it: every score enters as the exact value of its f64, the label as the exact
value of its f32 (gains 2^g - 1: tests/lambdamart_exact.py's), gamma as the exact 53-bit fraction.  Every single operation
is rounded to 60 digits; every sum is taken in a 2 000-digit context and is exact, so there is no summation shape.
`exp` is the 60-digit one, with an exponent range that never underflows: a document 800 below the top keeps its true, tiny
rho, and u_i = 1 - rho_i is formed as (E - e_i) / E from the exact sum, which does not cancel: it is positive for every
document of a query of two or more, so Q is always the quotient here.
Standard library only (gamma's integers come from the restatement's `mix`, which is integer arithmetic).
"""
import decimal
from decimal import Decimal

from tests import lambdamart_exact as ex
from tests.lambdamart_xendcg_model import GOLDEN, mix

CTX, SUM = ex.CTX, ex.SUM
ZERO, ONE = Decimal(0), Decimal(1)


def gamma(key, i) -> Decimal:
    return SUM.divide(Decimal(mix(int(key) + GOLDEN * (int(i) + 1)) >> 11), Decimal(2 ** 53))  # (exact: at most 53 binary places)


def total(xs) -> Decimal:
    acc = ZERO
    for x in xs:
        acc = SUM.add(acc, x)
    return acc


class ExactXe:
    """One query: scores s (f64), labels y (stored as f32), instance ids, the tree key.  live: Phi > 0 and n >= 2."""

    def __init__(self, s, y, ids, key):
        with decimal.localcontext(CTX):
            self.n = n = len(s)
            self.s = [ex.dec(v) for v in s]
            self.g = [ex.label32(v) for v in y]
            self.G = [ex.gain(g) for g in self.g]
            self.gamma = [gamma(key, i) for i in ids]
            self.phi = [SUM.subtract(SUM.add(G, ONE), c) for G, c in zip(self.G, self.gamma)]
            self.Phi = total(self.phi)
            self.live = n >= 2 and self.Phi > 0
            if not self.live:
                return
            m = max(self.s)
            self.x = [SUM.subtract(v, m) for v in self.s]  # (exact: the difference of two f64)
            self.e = [CTX.exp(x) for x in self.x]
            self.E = total(self.e)
            self.rho = [CTX.divide(e, self.E) for e in self.e]
            self.u = [CTX.divide(SUM.subtract(self.E, e), self.E) for e in self.e]
            inv = CTX.divide(ONE, self.Phi)
            self.t1 = [CTX.subtract(CTX.multiply(p, inv), r) for p, r in zip(self.phi, self.rho)]
            self.a = [CTX.divide(t, u) for t, u in zip(self.t1, self.u)]
            self.S1 = total(self.a)
            self.t2 = [CTX.multiply(r, SUM.subtract(self.S1, a)) for r, a in zip(self.rho, self.a)]
            self.b = [CTX.divide(t, u) for t, u in zip(self.t2, self.u)]
            self.S2 = total(self.b)
            self.t3 = [CTX.multiply(r, SUM.subtract(self.S2, b)) for r, b in zip(self.rho, self.b)]
            self.lam = [SUM.add(SUM.add(x, y2), z) for x, y2, z in zip(self.t1, self.t2, self.t3)]
            self.w = [CTX.multiply(r, u) for r, u in zip(self.rho, self.u)]
