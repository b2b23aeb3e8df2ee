"""Feature normalisation restated in numpy, operation for operation; not a test file itself.
Written from the definition: the reference's StreamingStats.push (src/stats.rs:53-104) over the values the instances HOLD
(src/normalizers.rs:23-27), records per chunk of 256 consecutive instances folded in chunk order, and the per-value functions
(src/normalizers.rs:55-108) in f32.

  sequential(xs)                 the plain loop of the reference over one list of values
  group_records(V, H, starts, lens)   the same push, vectorised ACROSS groups and features: step j pushes the j-th row of
                                 every group that has one (numpy's f64 operations are IEEE and never fused)
  dataset_records(V, H)          chunks of 256 rows of the list, then the fold in chunk order
  fit / apply / per_query / sigmoid   what Normalizer.fit, .apply and the query scope compute
  bounded_column(xs, held)       one column again in Python floats, every operation carrying a bound on its distance from
                                 the exact value (see its docstring), for the host test's derived bound
"""
import math
from fractions import Fraction

import numpy as np

CHUNK = 256
DBL_MAX = np.finfo(np.float64).max
KEYS = ("num_elements", "mean", "variance", "max", "min", "total")


# ---------------------------------------------------------------------------------------------------------------------
# the reference's loop
# ---------------------------------------------------------------------------------------------------------------------
def empty():
    return [0, 0.0, 0.0, -DBL_MAX, DBL_MAX, 0.0]  # n, mean, s, max, min, total


def push(r, x):
    x = float(x)
    r[0] += 1
    old_mean, old_s = r[1], r[2]
    if r[3] < x:
        r[3] = x
    if r[4] > x:
        r[4] = x
    r[5] = r[5] + x
    if r[0] == 1:
        r[1] = x
        return
    dx = x - old_mean
    r[1] = old_mean + dx / float(r[0])
    dm = x - r[1]
    r[2] = old_s + dx * dm


def sequential(xs):
    r = empty()
    for x in xs:
        push(r, x)
    return r


def fold(a, b):
    """a followed by b; an empty side leaves the other as it is"""
    if b[0] == 0:
        return list(a)
    if a[0] == 0:
        return list(b)
    na, nb = a[0], b[0]
    n = na + nb
    delta = b[1] - a[1]
    mean = a[1] + delta * (float(nb) / float(n))
    s = (a[2] + b[2]) + (delta * delta) * ((float(na) * float(nb)) / float(n))
    return [n, mean, s, b[3] if a[3] < b[3] else a[3], b[4] if a[4] > b[4] else a[4], a[5] + b[5]]


def chunked(xs, held):
    acc = empty()
    for c in range(0, len(xs), CHUNK):
        acc = fold(acc, sequential([x for x, h in zip(xs[c:c + CHUNK], held[c:c + CHUNK]) if h]))
    return acc


def finish(r):
    """ComputedStats, or None for fewer than two values (src/stats.rs:54-63, :97-102)"""
    if r[0] <= 1:
        return None
    return {"num_elements": int(r[0]), "mean": float(r[1]), "variance": float(r[2]) / float(r[0] - 1), "max": float(r[3]), "min": float(r[4]),
            "total": float(r[5])}


# ---------------------------------------------------------------------------------------------------------------------
# the same, vectorised across groups and features
# ---------------------------------------------------------------------------------------------------------------------
def group_records(V, H, starts, lens):
    """Records [groups, d] (a dict of arrays n, mean, s, max, min, total) of the rows starts[g] .. starts[g] + lens[g] of V
    (float32 [m, d]) where H (bool [m, d]) says the value is held."""
    starts, lens = np.asarray(starts, dtype=np.int64), np.asarray(lens, dtype=np.int64)
    G, d = len(starts), V.shape[1]
    n = np.zeros((G, d), dtype=np.int64)
    mean, s, total = np.zeros((G, d)), np.zeros((G, d)), np.zeros((G, d))
    mx, mn = np.full((G, d), -DBL_MAX), np.full((G, d), DBL_MAX)
    order = np.argsort(-lens, kind="stable")  # the groups still live at step j are a prefix of this order
    slens = lens[order]
    with np.errstate(all="ignore"):
        for j in range(int(lens.max()) if G else 0):
            live = order[:int(np.searchsorted(-slens, -j, side="left"))]  # groups with lens > j
            rows = starts[live] + j
            x, h = V[rows].astype(np.float64), H[rows]
            n0, m0, s0 = n[live], mean[live], s[live]
            n1 = n0 + 1
            first = n1 == 1
            dx = x - m0
            m1 = np.where(first, x, m0 + dx / n1.astype(np.float64))
            dm = x - m1
            s1 = np.where(first, s0, s0 + dx * dm)
            n[live] = np.where(h, n1, n0)
            mean[live] = np.where(h, m1, m0)
            s[live] = np.where(h, s1, s0)
            mx[live] = np.where(h & (mx[live] < x), x, mx[live])
            mn[live] = np.where(h & (mn[live] > x), x, mn[live])
            total[live] = np.where(h, total[live] + x, total[live])
    return {"n": n, "mean": mean, "s": s, "max": mx, "min": mn, "total": total}


def fold_records(rec):
    """[groups, d] -> [d]: the groups folded in their order"""
    G, d = rec["n"].shape
    n = np.zeros(d, dtype=np.int64)
    mean, s, total = np.zeros(d), np.zeros(d), np.zeros(d)
    mx, mn = np.full(d, -DBL_MAX), np.full(d, DBL_MAX)
    with np.errstate(all="ignore"):
        for g in range(G):
            nb, mb, sb = rec["n"][g], rec["mean"][g], rec["s"][g]
            take = (nb > 0) & (n == 0)
            both = (nb > 0) & (n > 0)
            nn = n + nb
            fn = np.where(nn > 0, nn, 1).astype(np.float64)
            delta = mb - mean
            m2 = mean + delta * (nb.astype(np.float64) / fn)
            s2 = (s + sb) + (delta * delta) * ((n.astype(np.float64) * nb.astype(np.float64)) / fn)
            mean = np.where(take, mb, np.where(both, m2, mean))
            s = np.where(take, sb, np.where(both, s2, s))
            total = np.where(take, rec["total"][g], np.where(both, total + rec["total"][g], total))
            mx = np.where(take, rec["max"][g], np.where(both & (mx < rec["max"][g]), rec["max"][g], mx))
            mn = np.where(take, rec["min"][g], np.where(both & (mn > rec["min"][g]), rec["min"][g], mn))
            n = np.where(nb > 0, nn, n)
    return {"n": n, "mean": mean, "s": s, "max": mx, "min": mn, "total": total}


def dataset_records(V, H):
    m = V.shape[0]
    starts = np.arange(0, m, CHUNK, dtype=np.int64)
    return fold_records(group_records(V, H, starts, np.minimum(CHUNK, m - starts)))


def held_mask(present_bits, present_words, n, d):
    """bool [n, d] from the presence bits of a file-loaded dataset (empty: every value is held)"""
    if present_bits is None or len(present_bits) == 0:
        return np.ones((n, d), dtype=bool)
    bits = np.asarray(present_bits, dtype=np.uint32).reshape(n, present_words)
    f = np.arange(d)
    return ((bits[:, f >> 5] >> (f & 31).astype(np.uint32)) & 1).astype(bool)


def fit(X, H, instances, features):
    """{fid: ComputedStats} of the rows `instances` (the view's order) for `features`"""
    idx = np.asarray(instances, dtype=np.int64)
    rec = dataset_records(np.ascontiguousarray(X[idx]), np.ascontiguousarray(H[idx]))
    out = {}
    for f in features:
        if rec["n"][f] >= 2:
            out[int(f)] = {"num_elements": int(rec["n"][f]), "mean": float(rec["mean"][f]), "variance": float(rec["s"][f] / np.float64(rec["n"][f] - 1)),
                           "max": float(rec["max"][f]), "min": float(rec["min"][f]), "total": float(rec["total"][f])}
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the per-value functions, f32 throughout (src/normalizers.rs:55-108)
# ---------------------------------------------------------------------------------------------------------------------
KEEP, ZERO, AFFINE = 0, 1, 2


def params(stats, method, d):
    """(kind, a, b) per column: (val - a) / b, 0.0, or the value as it is (no record)"""
    kind, a, b = np.zeros(d, dtype=np.int64), np.zeros(d, dtype=np.float32), np.ones(d, dtype=np.float32)
    with np.errstate(all="ignore"):
        for f, st in stats.items():
            if f >= d:
                continue
            if method == "maxmin":
                mx, mn = np.float32(st["max"]), np.float32(st["min"])
                kind[f], a[f], b[f] = (ZERO, 0, 1) if mx == mn else (AFFINE, mn, mx - mn)
            else:
                sd = np.float32(np.sqrt(np.float64(st["variance"])))
                kind[f], a[f], b[f] = (ZERO, 0, 1) if sd == 0 else (AFFINE, np.float32(st["mean"]), sd)
    return kind, a, b


def transform(X, H, kind, a, b):
    """kind / a / b broadcast against X ([d] for the dataset scope, [n, d] for the query scope)"""
    X = np.asarray(X, dtype=np.float32)
    with np.errstate(all="ignore"):
        aff = (X - a.astype(np.float32)) / b.astype(np.float32)
    out = np.where(kind == AFFINE, aff, np.where(kind == ZERO, np.float32(0.0), X)).astype(np.float32)
    return np.where(H, out, np.float32(0.0)).astype(np.float32)


def first_nan(out, H):
    """(instance, feature) of the lowest held NaN result: instance first, then feature; None when there is none"""
    bad = np.argwhere(np.isnan(out) & H)
    return None if len(bad) == 0 else (int(bad[0][0]), int(bad[0][1]))


def first_nonfinite(X, H, instances, features):
    mask = np.zeros(X.shape, dtype=bool)
    mask[np.ix_(np.asarray(instances, dtype=np.int64), np.asarray(features, dtype=np.int64))] = True
    bad = np.argwhere(~np.isfinite(X) & H & mask)
    return None if len(bad) == 0 else (int(bad[0][0]), int(bad[0][1]))


def apply(X, H, stats, method):
    kind, a, b = params(stats, method, X.shape[1])
    return transform(X, H, kind, a, b)


def sigmoid_value(v):
    """the two-branch form in f64, rounded to f32 once"""
    x = float(np.float32(v))
    if x != x:
        return np.float32(np.nan)
    if x > 0.0:
        z = math.exp(-x) if x < 800 else 0.0
        return np.float32(1.0 / (1.0 + z))
    z = math.exp(x) if x > -800 else 0.0
    return np.float32(z / (1.0 + z))


def per_query(X, H, qid, method):
    """Query scope: statistics per (query, feature) over the query's rows in instance order, fewer than two held values -> 0.0"""
    qid = np.asarray(qid)
    n, d = X.shape
    order = np.argsort(qid, kind="stable")  # rows grouped by query, instance order inside
    uq, starts, lens = np.unique(qid[order], return_index=True, return_counts=True)
    rec = group_records(np.ascontiguousarray(X[order]), np.ascontiguousarray(H[order]), starts, lens)
    G = len(uq)
    kind = np.full((G, d), ZERO, dtype=np.int64)
    a, b = np.zeros((G, d), dtype=np.float32), np.ones((G, d), dtype=np.float32)
    ok = rec["n"] >= 2
    with np.errstate(all="ignore"):
        if method == "maxmin":
            mx, mn = rec["max"].astype(np.float32), rec["min"].astype(np.float32)
            aff = ok & (mx != mn)
            a, b = np.where(aff, mn, a).astype(np.float32), np.where(aff, mx - mn, b).astype(np.float32)
        else:
            var = rec["s"] / np.where(ok, rec["n"] - 1, 1).astype(np.float64)
            sd = np.sqrt(var).astype(np.float32)
            aff = ok & ~(sd == 0)
            a, b = np.where(aff, rec["mean"].astype(np.float32), a).astype(np.float32), np.where(aff, sd, b).astype(np.float32)
    kind[aff] = AFFINE
    group_of_sorted = np.repeat(np.arange(G), lens)
    group = np.empty(n, dtype=np.int64)
    group[order] = group_of_sorted
    return transform(X, H, kind[group], a[group], b[group])


# ---------------------------------------------------------------------------------------------------------------------
# one column with a running error bound
# ---------------------------------------------------------------------------------------------------------------------
U = Fraction(1, 2 ** 53)
ETA = Fraction(1, 2 ** 1074)


def _up(fr):
    """a dyadic rational >= fr (keeps the bounds' denominators small)"""
    return Fraction(math.nextafter(float(fr), math.inf)) if fr else Fraction(0)


def _F(x):
    return abs(Fraction(x))


def _bounded_push(xs):
    """sequential(xs) with em >= |mean - exact mean of xs| and es >= |s - exact sum of squared deviations of xs|.

    A rounded result r~ = fl(r) is off by at most U |r~| (round to nearest), a product or quotient that may be subnormal by
    ETA = 2^-1074 more.  Step k with the exact M' = M + (x - M) / k, S' = S + (x - M)(x - M'):
      dx~ = fl(x - m~)          |dx~ - (x - M)| <= em + U |dx~| = e_dx
      q~  = fl(dx~ / k)         m~' = fl(m~ + q~):  m~ + (x - m~) / k is off M' by em (k - 1) / k, the three roundings add
                                U |dx~| / k + U |q~| + ETA + U |m~'|
      dm~ = fl(x - m~')         e_dm = em' + U |dm~|
      p~  = fl(dx~ dm~)         |dx~| e_dm + (|dm~| + e_dm) e_dx + U |p~| + ETA
      s~' = fl(s~ + p~)         es + the line above + U |s~'|"""
    r = empty()
    em, es = Fraction(0), Fraction(0)
    for x in xs:
        x = float(x)
        old_mean, old_s = r[1], r[2]
        push(r, x)
        k = r[0]
        if k == 1:
            continue
        dx = x - old_mean
        q = dx / float(k)
        e_dx = em + U * _F(dx)
        em = _up(em * Fraction(k - 1, k) + U * _F(dx) / k + U * _F(q) + ETA + U * _F(r[1]))
        dm = x - r[1]
        e_dm = em + U * _F(dm)
        p = dx * dm
        es = _up(es + _F(dx) * e_dm + (_F(dm) + e_dm) * e_dx + U * _F(p) + ETA + U * _F(r[2]))
    return r, em, es


def _bounded_fold(a, ea, b, eb):
    """fold(a, b) with its (em, es).  Exact: M = Ma + D nb / n, S = Sa + Sb + D^2 na nb / n, D = Mb - Ma.
      d~  = fl(mb~ - ma~)       e_d = ema + emb + U |d~|
      sh~ = fl(nb / n)          U sh~
      t~  = fl(d~ sh~)          against (mb~ - ma~) nb / n: |d~| U sh~ + (nb / n) U |d~| + U |t~| + ETA
      m~  = fl(ma~ + t~)        ema na / n + emb nb / n + the line above + U |m~|
      ss~ = fl(sa~ + sb~)       esa + esb + U |ss~|
      d2~ = fl(d~ d~)           2 |d~| e_d + e_d^2 + U |d2~| + ETA
      w~  = fl((na nb) / n)     na nb is exact below 2^53;  U |w~|
      pr~ = fl(d2~ w~)          |d2~| e_w + (|w~| + e_w) e_d2 + U |pr~| + ETA
      s~  = fl(ss~ + pr~)       e_ss + e_pr + U |s~|"""
    if b[0] == 0:
        return list(a), ea[0], ea[1]
    if a[0] == 0:
        return list(b), eb[0], eb[1]
    out = fold(a, b)
    na, nb, n = a[0], b[0], a[0] + b[0]
    assert na * nb < 2 ** 53
    d = b[1] - a[1]
    sh = float(nb) / float(n)
    t = d * sh
    e_d = ea[0] + eb[0] + U * _F(d)
    e_t = _F(d) * U * _F(sh) + Fraction(nb, n) * U * _F(d) + U * _F(t) + ETA
    em = _up(ea[0] * Fraction(na, n) + eb[0] * Fraction(nb, n) + e_t + U * _F(out[1]))
    ss = a[2] + b[2]
    e_ss = ea[1] + eb[1] + U * _F(ss)
    d2 = d * d
    e_d2 = 2 * _F(d) * e_d + e_d * e_d + U * _F(d2) + ETA
    w = (float(na) * float(nb)) / float(n)
    e_w = U * _F(w)
    pr = d2 * w
    e_pr = _F(d2) * e_w + (_F(w) + e_w) * e_d2 + U * _F(pr) + ETA
    es = _up(e_ss + e_pr + U * _F(out[2]))
    return out, em, es


def bounded_column(xs, held):
    """chunked(xs, held) with bounds: (record, bound on |mean - exact|, bound on |variance - exact|); the variance's last
    division adds U |variance~| + ETA to es / (n - 1)."""
    acc, ea = empty(), (Fraction(0), Fraction(0))
    for c in range(0, len(xs), CHUNK):
        r, em, es = _bounded_push([x for x, h in zip(xs[c:c + CHUNK], held[c:c + CHUNK]) if h])
        acc, em, es = _bounded_fold(acc, ea, r, (em, es))
        ea = (em, es)
    if acc[0] <= 1:
        return acc, ea[0], None
    var = acc[2] / float(acc[0] - 1)
    return acc, ea[0], ea[1] / (acc[0] - 1) + U * _F(var) + ETA


def exact_column(xs, held):
    """(mean, variance) of the held values in exact rationals"""
    fx = [Fraction(float(x)) for x, h in zip(xs, held) if h]
    n = len(fx)
    mu = sum(fx) / n
    return mu, sum((f - mu) ** 2 for f in fx) / (n - 1)
