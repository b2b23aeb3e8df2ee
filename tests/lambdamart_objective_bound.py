"""Exact statements and the error bound for the MAP / MRR pair weights ("Objectives").  Shared by
tests/test_lambdamart_objective_host.py; not a test file itself.

`swap_delta` is the definition the closed forms stand for: |metric(i and j swapped) - metric| in exact rationals.

`oracle_bound` bounds |delta_f64 - |fl(m') - fl(m)|| where delta_f64 is the closed form evaluated in f64 (the restatement,
the kernel) and fl(m), fl(m') are the evaluator's f64 metric of the list before and after the swap.  Method of
tests/lambdamart_bound.py: first order in u = 2^-53 with its factor SLACK = 1 + 2^-20 for the second-order terms, u per
correctly rounded operation, gamma_n = n u / (1 - n u) on a sequential sum of n terms.  There is no library call.

  map, closed form  x = fl(C_a / (a + 1)), y = fl(c_b / (b + 1)): u x, u y.  fl(x - y): u |x - y|.
                    P[r]: k_r terms fl(1 / (r' + 1)) (u each) added one after the other (the zeros of the other ranks add
                    exactly): gamma_{k_r + 1} P[r] each, for P[b-1] and for P[a].  THE DIFFERENCE CANCELS: the two prefix sums
                    share their first k_a terms and differ by the few in between, so the error is measured against
                    P[b-1] + P[a], not against their difference.  fl(P[b-1] - P[a]): u |P[b-1] - P[a]|.
                    The sum M, and the division by R_q: 2u |M|.
                    e_closed = [u (x + y + |x - y| + |P[b-1] - P[a]|) + gamma_{k_{b-1} + 1} P[b-1] + gamma_{k_a + 1} P[a] + 2u |M|] / R_q
  map, evaluator    AP = fl(S / R_q), S = the k precisions fl(c / (r + 1)) (u each) added in rank order: gamma_{k + 1} S, and
                    u for the division: |fl(AP) - AP| <= gamma_{k + 2} AP, for both lists; their difference adds u |AP' - AP|.
                    e_eval = gamma_{k + 2} (AP + AP') + u |AP' - AP|
  mrr               both sides are fl(1 / (p + 1)) for two ranks p and one subtraction: u (1/(p+1) + 1/(p'+1)) + u |delta| each.
No constant above was adjusted after seeing a result; the test prints the worst error / bound it meets.
"""
from fractions import Fraction

U = Fraction(1, 2 ** 53)
SLACK = 1 + Fraction(1, 2 ** 20)


def gamma(n):
    return n * U / (1 - n * U)


def metric(rel_by_rank, norm, objective):
    """AP or RR of a ranked list of relevance flags, exact.  norm: the evaluator's (map: 0 = the list's own count)."""
    rel = [bool(x) for x in rel_by_rank]
    if objective == "mrr":
        return Fraction(1, rel.index(True) + 1) if True in rel else Fraction(0)
    R = int(norm) or sum(rel)
    if R == 0:
        return Fraction(0)
    c, total = 0, Fraction(0)
    for r, x in enumerate(rel):
        if x:
            c += 1
            total += Fraction(c, r + 1)
    return total / R


def by_rank(rank, rel):
    out = [False] * len(rank)
    for p, r in enumerate(rank):
        out[int(r)] = bool(rel[p])
    return out


def swap_delta(rank, rel, i, j, norm, objective):
    """|metric with documents i and j swapped - metric|, exact."""
    before = by_rank(rank, rel)
    after = list(before)
    after[int(rank[i])], after[int(rank[j])] = before[int(rank[j])], before[int(rank[i])]
    return abs(metric(after, norm, objective) - metric(before, norm, objective))


def oracle_bound(rank, rel, i, j, norm, objective):
    """Bound on |closed form in f64 - |evaluator after the swap - evaluator before|| for the pair (i, j): see the module."""
    before = by_rank(rank, rel)
    after = list(before)
    ri, rj = int(rank[i]), int(rank[j])
    after[ri], after[rj] = before[rj], before[ri]
    rh, rl = (ri, rj) if rel[i] else (rj, ri)
    if objective == "mrr":
        f, f_after = before.index(True), after.index(True)
        one = U * (Fraction(1, f + 1) + Fraction(1, f_after + 1)) + U * abs(Fraction(1, f + 1) - Fraction(1, f_after + 1))
        return SLACK * 2 * one
    R = int(norm) or sum(before)
    a, b = min(rh, rl), max(rh, rl)
    up = 1 if rl < rh else 0
    c = [sum(before[:r + 1]) for r in range(len(before))]
    P = [sum((Fraction(1, r2 + 1) for r2 in range(r + 1) if before[r2]), Fraction(0)) for r in range(len(before))]
    x, y = Fraction(c[a] + up, a + 1), Fraction(c[b], b + 1)
    pd = P[b - 1] - P[a]
    M = (x - y) + pd
    closed = (U * (x + y + abs(x - y) + abs(pd)) + gamma(c[b - 1] + 1) * P[b - 1] + gamma(c[a] + 1) * P[a] + 2 * U * abs(M)) / R
    k = sum(before)
    ap, ap2 = metric(before, norm, "map"), metric(after, norm, "map")
    evaluator = gamma(k + 2) * (ap + ap2) + U * abs(ap2 - ap)
    return SLACK * (closed + evaluator)
