"""The numpy restatement of permutation importance (csrc/permute.hpp states the definition): the stream,
the sources under both scopes, and the host's report.  `sources_scalar` / `report_scalar` say the same once more, term by term
in Python integers and floats, and hold the vectorised forms (tests/test_permute_host.py); the device's values are held to
an oracle made with `sources` (tests/test_gpu_permutation_importance.py).

G, mix_int, mix and means are those of tests/resample_model.py.  Every f64 operation of the report is one rounded subtract,
add, multiply, divide or square root, in the definition's order."""
import math

import numpy as np

from tests import resample_model as rm

G = rm.G
MASK = rm.MASK
MAX_REPEATS = 64


def stream_key(seed):
    return rm.mix_int(seed + 3 * G)


def repeat_key(seed, r):
    return rm.mix_int(stream_key(seed) + (r + 1) * G)


def keys(seed, r, n):
    """u_i = mix(key_r + (i + 1) G), i = 0 .. n-1: uint64[n]"""
    with np.errstate(over="ignore"):
        return rm.mix(np.uint64(repeat_key(seed, r)) + np.uint64(G) * np.arange(1, n + 1, dtype=np.uint64))


def keys_many(seeds, repeats, n):
    """u for every (seed, repeat) pair of two equally long lists: uint64[len, n]"""
    key_r = np.array([repeat_key(s, r) for s, r in zip(seeds, repeats)], dtype=np.uint64)
    with np.errstate(over="ignore"):
        return rm.mix(key_r[:, None] + np.uint64(G) * np.arange(1, n + 1, dtype=np.uint64)[None, :])


def order_of(u):
    """list indices sorted by (u_i, i) ascending (last axis)"""
    return np.argsort(u, axis=-1, kind="stable")


def sources(ids, seed, r, scope="dataset", query_of=None):
    """src_r of every instance of `ids` (the view's instance ids ASCENDING), aligned with ids.  query_of[i]: the query of
    ids[i] (scope "query")."""
    ids = np.asarray(ids, dtype=np.int64)
    assert np.all(np.diff(ids) > 0)
    n = len(ids)
    u = keys(seed, r, n)
    if scope == "dataset":
        return ids[order_of(u)]
    assert scope == "query"
    query_of = np.asarray(query_of)
    out = np.empty(n, dtype=np.int64)
    for q in np.unique(query_of):
        members = np.nonzero(query_of == q)[0]  # ascending list indices
        out[members] = ids[members[order_of(u[members])]]
    return out


def sources_scalar(ids, seed, r, scope="dataset", query_of=None):
    """The same in Python integers, one element at a time."""
    ids = [int(i) for i in ids]
    n = len(ids)
    key = rm.mix_int((seed + 3 * G) & MASK)
    key_r = rm.mix_int((key + (r + 1) * G) & MASK)
    u = [rm.mix_int((key_r + (i + 1) * G) & MASK) for i in range(n)]
    out = [None] * n
    if scope == "dataset":
        groups = [list(range(n))]
    else:
        seen = {}
        for i in range(n):
            seen.setdefault(query_of[i], []).append(i)
        groups = list(seen.values())
    for members in groups:
        ranked = sorted(members, key=lambda i: (u[i], i))
        for m, i in enumerate(members):
            out[i] = ids[ranked[m]]
    return out


def report(baseline, values):
    """(importance, std) of one feature's values[R]"""
    values = np.asarray(values, dtype=np.float64)
    R = len(values)
    d = np.float64(baseline) - values
    importance = np.cumsum(np.concatenate([[0.0], d]))[-1] / np.float64(R)
    if R == 1:
        return float(importance), 0.0
    e = d - importance
    return float(importance), float(np.sqrt(np.cumsum(np.concatenate([[0.0], e * e]))[-1] / np.float64(R - 1)))


def report_scalar(baseline, values):
    R = len(values)
    total = 0.0
    for v in values:
        total = total + (float(baseline) - float(v))
    importance = total / float(R)
    if R == 1:
        return importance, 0.0
    ss = 0.0
    for v in values:
        e = (float(baseline) - float(v)) - importance
        ss = ss + e * e
    return importance, math.sqrt(ss / float(R - 1))


def permuted_matrix(X, ids, src, f):
    """D_{f,r}: a copy of X with x'[id][f] = x[src(id)][f] for the view's ids"""
    Xp = X.copy()
    Xp[np.asarray(ids), f] = X[np.asarray(src), f]
    return Xp


def permutation_index(rows):
    """rows: int[T, 4] permutations of 0..3 -> int[T] in 0..23"""
    rows = np.asarray(rows, dtype=np.int64)
    code = rows[:, 0] * 64 + rows[:, 1] * 16 + rows[:, 2] * 4 + rows[:, 3]
    table = {}
    import itertools

    for k, p in enumerate(itertools.permutations(range(4))):
        table[p[0] * 64 + p[1] * 16 + p[2] * 4 + p[3]] = k
    lookup = np.full(256, -1, dtype=np.int64)
    for c, k in table.items():
        lookup[c] = k
    out = lookup[code]
    assert out.min() >= 0
    return out


def chi_square(counts, expected):
    counts = np.asarray(counts, dtype=np.float64)
    return float(((counts - expected) ** 2 / expected).sum())
