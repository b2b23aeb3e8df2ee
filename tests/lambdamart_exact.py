"""LambdaMART's gradient pass ("Definition") in `decimal` arithmetic, for the tests.

Written from the definition, not from tests/lambdamart_model.py or the kernel, and with no f64 in it:
  * every input (score, sigma, the norm when one is given) enters as the exact value of its f64, the label as the exact
    value of its f32;
  * gains `2^g - 1` from that label (integer labels: exact; others: the 60-digit power);
  * discounts `1 / log2(r + 2)` = `ln 2 / ln(r + 2)` from 60-digit logarithms, no table;
  * `rho = 1 / (1 + exp(sigma (s_h - s_l)))` from the 60-digit `exp`, with an exponent range that never under- or
    overflows, so a saturated pair keeps its true, tiny term; `1 - rho` as `exp(.) / (1 + exp(.))`, which does not cancel;
  * the norm `Z` = the ideal DCG at the depth (every gain, descending, the first k of them), unless the caller passes the
    evaluator's number (the definition takes `Z_q` from the evaluator; with judgments it is not the query's own);
  * a document's terms are added in a 2 000-digit context: the sum is exact unless the terms span more than 1 900 decimal
    orders, so there is no summation order to speak of.
Each single operation is rounded to 60 digits (relative 1e-60), 44 orders below anything an f64 comparison can see.

A query is ranked once (a sort); after that any chosen document costs O(m): `ExactQuery.document(i)`.
Standard library only.
"""
import decimal
from decimal import Decimal

CTX = decimal.Context(prec=60, rounding=decimal.ROUND_HALF_EVEN, Emax=decimal.MAX_EMAX, Emin=decimal.MIN_EMIN,
                      traps=[decimal.InvalidOperation, decimal.DivisionByZero, decimal.Overflow])
SUM = decimal.Context(prec=2000, rounding=decimal.ROUND_HALF_EVEN, Emax=decimal.MAX_EMAX, Emin=decimal.MIN_EMIN,
                      traps=[decimal.InvalidOperation, decimal.DivisionByZero, decimal.Overflow])
ZERO, ONE, TWO = Decimal(0), Decimal(1), Decimal(2)
_LN2 = CTX.ln(TWO)
_discounts = {}
_gains = {}


def dec(x) -> Decimal:
    """The exact value of a Python / numpy float."""
    return Decimal(float(x))


def label32(y) -> float:
    """The label as the f32 the dataset stores (struct round trip: no numpy needed)."""
    import struct

    return struct.unpack("f", struct.pack("f", float(y)))[0]


def gain(g: float) -> Decimal:
    """2^g - 1 for the f32 label g."""
    v = _gains.get(g)
    if v is None:
        if float(g).is_integer() and abs(g) <= 4096:
            p = SUM.power(TWO, int(g)) if g >= 0 else SUM.divide(ONE, SUM.power(TWO, int(-g)))  # exact: a power of two has a finite decimal form
            v = SUM.subtract(p, ONE)
        else:
            v = CTX.subtract(CTX.power(TWO, dec(g)), ONE)
        _gains[g] = v
    return v


def discount(r: int) -> Decimal:
    """1 / log2(r + 2)."""
    v = _discounts.get(r)
    if v is None:
        v = ONE if r == 0 else CTX.divide(_LN2, CTX.ln(Decimal(r + 2)))
        _discounts[r] = v
    return v


def ideal_dcg(labels, depth=None) -> Decimal:
    """sum over the first k of the gains sorted descending of G / log2(i + 2), k = depth or all of them."""
    g = sorted((label32(y) for y in labels), reverse=True)
    k = len(g) if depth is None else min(depth, len(g))
    z = ZERO
    for i, x in enumerate(g[:k]):
        z = SUM.add(z, CTX.multiply(gain(x), discount(i)))
    return z


def ranks(scores, labels, ids):
    """0-based rank of every document in the RankedInstance order: score descending, gain ascending, id ascending
    (-0.0 and +0.0 are one score)."""
    m = len(scores)
    order = sorted(range(m), key=lambda p: (-(float(scores[p]) + 0.0), label32(labels[p]), int(ids[p])))
    r = [0] * m
    for pos, p in enumerate(order):
        r[p] = pos
    return r


class Pair:
    """One ordered pair (i, its partner j) with different labels: everything a term is made of."""
    __slots__ = ("j", "high", "x", "rho", "one_minus_rho", "delta", "Gi", "Gj", "Di", "Dj")


class ExactQuery:
    """One query: scores (f64), labels, instance ids (stored order = ids ascending), the depth k (None: all), sigma,
    and the norm Z (None: the query's own ideal DCG)."""

    def __init__(self, scores, labels, ids, depth=None, sigma=1.0, norm=None):
        self.m = len(scores)
        self.s = [dec(float(v) + 0.0) for v in scores]
        self.g = [label32(y) for y in labels]
        self.ids = [int(v) for v in ids]
        self.depth = depth
        self.k = self.m if depth is None else depth
        self.sigma = dec(sigma)
        self.rank = ranks(scores, labels, ids)
        self.G = [gain(g) for g in self.g]
        self.D = [discount(r) if r < self.k else ZERO for r in self.rank]
        self.Z = ideal_dcg(labels, depth) if norm is None else dec(norm)
        self.live = (not self.Z.is_nan()) and self.Z > 0

    def delta(self, i, j) -> Decimal:
        """|G_i - G_j| |D(r_i) - D(r_j)| / Z: what swapping the two ranks changes NDCG by."""
        dG = SUM.subtract(self.G[i], self.G[j]).copy_abs()  # (abs() would round to the ambient context)
        dD = SUM.subtract(self.D[i], self.D[j]).copy_abs()
        return CTX.divide(CTX.multiply(dG, dD), self.Z)

    def pairs(self, i):
        """The pairs of document i, partners in stored order; pairs whose delta is exactly 0 are left out (their terms
        are exactly 0 on every side)."""
        if not self.live:
            return
        gi = self.g[i]
        for j in range(self.m):
            gj = self.g[j]
            if gj == gi or self.D[i] == self.D[j]:
                continue
            p = Pair()
            p.j, p.high = j, gi > gj
            diff = SUM.subtract(self.s[i], self.s[j]) if p.high else SUM.subtract(self.s[j], self.s[i])  # s_h - s_l, exact
            p.x = CTX.multiply(self.sigma, diff)
            e = CTX.exp(p.x)
            p.rho = CTX.divide(ONE, CTX.add(ONE, e))
            p.one_minus_rho = CTX.divide(e, CTX.add(ONE, e))  # (not 1 - rho: that cancels at any fixed precision)
            p.delta = self.delta(i, j)
            p.Gi, p.Gj, p.Di, p.Dj = self.G[i], self.G[j], self.D[i], self.D[j]
            yield p

    def document(self, i, pairs=None):
        """(lambda_i, w_i): lambda_i = sum over partners of +-sigma rho delta (+ when i holds the higher label),
        w_i = sum of sigma^2 rho (1 - rho) delta."""
        lam, w = ZERO, ZERO
        s2 = SUM.multiply(self.sigma, self.sigma)
        for p in (self.pairs(i) if pairs is None else pairs):
            t = CTX.multiply(CTX.multiply(self.sigma, p.rho), p.delta)
            lam = SUM.add(lam, t) if p.high else SUM.subtract(lam, t)
            w = SUM.add(w, CTX.multiply(CTX.multiply(CTX.multiply(s2, p.rho), p.one_minus_rho), p.delta))
        return lam, w

    def cost(self, scores=None) -> Decimal:
        """C(s) = sum over pairs (h, l) of delta_hl log(1 + exp(-sigma (s_h - s_l))), with delta frozen at this query's
        ranking; `scores`: Decimals to evaluate it at (default: the query's own)."""
        s = self.s if scores is None else scores
        c = ZERO
        if not self.live:
            return c
        for h in range(self.m):
            for l in range(self.m):
                if self.g[h] > self.g[l] and self.D[h] != self.D[l]:
                    x = CTX.multiply(self.sigma, CTX.subtract(s[h], s[l]))
                    c = SUM.add(c, CTX.multiply(self.delta(h, l), CTX.ln(CTX.add(ONE, CTX.exp(x.copy_negate())))))
        return c
