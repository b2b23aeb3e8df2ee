"""The evaluation measures of DESIGN.md section 17 (csrc/measures_host.hpp) restated in numpy, each over a RANKED list of gains:
once vectorised and once term by term in Python floats (the *_scalar forms).  The ranking is made from scores with the
reference comparator: score descending, gain ascending, id ascending.

    r = 1..n the ranked list, rel_r = gain_r > 0, gexp_r = 2^gain_r - 1, disc_{r-1} = log2(r + 1), L = min(k, n) or n
    dcg[@k]      sum_{r<=L} gexp_r / disc_{r-1}
    precision@k  #{rel_r, r<=L} / k
    recall[@k]   #{rel_r, r<=L} / num_rel        num_rel: the judged count, else the dataset's; 0: the list's own; 0 again: 0.0
    success@k    1.0 if any rel_r, r<=L
    err[@k]      p = 1, e = 0; for r<=L: R = rel_r ? gexp_r / den : 0; e = e + (p R) / r; p = p (1 - R)      den = 2^gmax

Every sum is a sequential float64 sum from 0.0 in rank order.  Gains are float32 values, as the library holds them."""
import math
from fractions import Fraction

import numpy as np

NAMES = ("dcg", "precision", "recall", "success", "err")
NEEDS_DEPTH = ("precision", "success")


def parse(evaluator):
    """("precision", 10) of "Precision@10"; depth None without one; aliases folded"""
    name, _, k = evaluator.partition("@")
    name = {"prec": "precision"}.get(name.lower(), name.lower())
    return name, (int(k) if k else None)


def gexp_of(gains):
    g = np.asarray(gains, dtype=np.float32).astype(np.float64)
    return np.array([math.pow(2.0, float(v)) - 1.0 for v in g], dtype=np.float64)


def discounts(n):
    return np.array([math.log2(i + 2.0) for i in range(n)], dtype=np.float64)


def cut(n, depth):
    return n if depth is None else min(int(depth), n)


def _seq_sum(terms):
    """0.0 + t_0 + t_1 + ... left to right (np.cumsum adds sequentially)"""
    return float(np.cumsum(np.concatenate(([0.0], np.asarray(terms, dtype=np.float64))))[-1])


def rank_order(scores, gains, ids):
    """positions of the list in rank order: score descending, gain ascending, id ascending"""
    scores = np.asarray(scores, dtype=np.float64)
    return np.lexsort((np.asarray(ids), np.asarray(gains, dtype=np.float32), -scores))


# ---- vectorised ------------------------------------------------------------------------------------------------------------

def dcg(gains, depth=None):
    L = cut(len(gains), depth)
    return _seq_sum(gexp_of(gains[:L]) / discounts(L))


def relevant(gains, depth=None):
    g = np.asarray(gains, dtype=np.float32)
    return int((g[:cut(len(g), depth)] > 0).sum())


def precision(gains, depth):
    return relevant(gains, depth) / float(depth)


def recall(gains, depth=None, num_rel=0):
    num_rel = int(num_rel) or relevant(gains)
    return relevant(gains, depth) / float(num_rel) if num_rel else 0.0


def success(gains, depth):
    return 1.0 if relevant(gains, depth) else 0.0


def err(gains, depth=None, den=1.0):
    g = np.asarray(gains, dtype=np.float32)
    L = cut(len(g), depth)
    R = np.where(g[:L] > 0, gexp_of(g[:L]) / float(den), 0.0)
    p = np.cumprod(np.concatenate(([1.0], 1.0 - R)))[:-1]  # p_r = ((1 (1 - R_1)) (1 - R_2)) ..., sequential
    return _seq_sum((p * R) / np.arange(1, L + 1, dtype=np.float64))


# ---- term by term, Python floats -----------------------------------------------------------------------------------------------

def dcg_scalar(gains, depth=None):
    total = 0.0
    for i in range(cut(len(gains), depth)):
        total = total + (math.pow(2.0, float(np.float32(gains[i]))) - 1.0) / math.log2(i + 2.0)
    return total


def relevant_scalar(gains, depth=None):
    c = 0
    for i in range(cut(len(gains), depth)):
        if float(np.float32(gains[i])) > 0.0:
            c += 1
    return c


def precision_scalar(gains, depth):
    return relevant_scalar(gains, depth) / float(depth)


def recall_scalar(gains, depth=None, num_rel=0):
    num_rel = int(num_rel)
    if num_rel == 0:
        num_rel = relevant_scalar(gains)
    return relevant_scalar(gains, depth) / float(num_rel) if num_rel != 0 else 0.0


def success_scalar(gains, depth):
    return 1.0 if relevant_scalar(gains, depth) != 0 else 0.0


def err_scalar(gains, depth=None, den=1.0):
    p, e = 1.0, 0.0
    for i in range(cut(len(gains), depth)):
        g = float(np.float32(gains[i]))
        R = (math.pow(2.0, g) - 1.0) / float(den) if g > 0.0 else 0.0
        e = e + (p * R) / float(i + 1)
        p = p * (1.0 - R)
    return e


# ---- exact statements (integer gains; rounded once by float()) -----------------------------------------------------------------

def err_exact(gains, depth=None, den=1):
    p, e = Fraction(1), Fraction(0)
    for i in range(cut(len(gains), depth)):
        g = int(gains[i])
        R = Fraction(2 ** g - 1, int(den)) if g > 0 else Fraction(0)
        e += p * R / (i + 1)
        p *= 1 - R
    return e


def dcg_exact(gains, depth=None):
    """only for lists whose non-zero gains stand at ranks r with r + 1 a power of two (an exact discount)"""
    total = Fraction(0)
    for i in range(cut(len(gains), depth)):
        g = int(gains[i])
        if g != 0:
            lg = (i + 2).bit_length() - 1
            assert 1 << lg == i + 2
            total += Fraction(2 ** g - 1, lg)
    return total


# ---- a dataset --------------------------------------------------------------------------------------------------------------

def value(name, depth, gains, norm=0.0, scalar=False):
    """one of the five over a ranked list; norm: recall's count of relevant documents (0: the list's own), err's den"""
    if name == "dcg":
        return (dcg_scalar if scalar else dcg)(gains, depth)
    if name == "precision":
        return (precision_scalar if scalar else precision)(gains, depth)
    if name == "recall":
        return (recall_scalar if scalar else recall)(gains, depth, norm)
    if name == "success":
        return (success_scalar if scalar else success)(gains, depth)
    if name == "err":
        return (err_scalar if scalar else err)(gains, depth, norm)
    raise ValueError(name)


def gmax(core_y, judged=None):
    """the largest gain of the dataset's core and of every judgment, floored at 0"""
    g = max(0.0, float(np.asarray(core_y, dtype=np.float32).max())) if len(core_y) else 0.0
    for docs in (judged or {}).values():
        for v in docs.values():
            g = max(g, float(np.float32(v)))
    return g


def ranked_lists(scores, y, qid, ids=None):
    """{query id: the query's gains (float32) in rank order} of a dataset (rows in instance order; ids: the rows' instance ids,
    default 0..n-1)"""
    scores, qid = np.asarray(scores, dtype=np.float64), np.asarray(qid)
    y32 = np.asarray(y, dtype=np.float32)
    ids = np.arange(len(y32)) if ids is None else np.asarray(ids)
    out = {}
    for q in np.unique(qid):
        rows = np.flatnonzero(qid == q)
        out[int(q)] = y32[rows][rank_order(scores[rows], y32[rows], ids[rows])]
    return out


def per_query(evaluator, ranked, core_y, judged=None):
    """{query id: value} from ranked_lists' output.  core_y: the labels of the whole core the rows belong to (ERR's gmax is the
    core's, not a view's); judged: {str(qid): {doc: gain}} as a CQRel holds it."""
    name, depth = parse(evaluator)
    den = math.pow(2.0, gmax(core_y, judged)) if name == "err" else 0.0
    out = {}
    for q, gains in ranked.items():
        norm = den
        if name == "recall":
            docs = (judged or {}).get(str(q))
            norm = sum(1 for v in docs.values() if float(np.float32(v)) > 0.0) if docs is not None else int((gains > 0).sum())
        out[q] = value(name, depth, gains, norm)
    return out
