"""The numpy restatement of model comparison (csrc/resample.hpp states the definition): both streams,
SUM, the bootstrap and the permutation procedure, and the host's report.  The device's arrays are held to `boot` / `perm`
bit for bit and the report to `report` (tests/test_gpu_resample.py, tests/test_gpu_compare_models.py); `boot_scalar` /
`perm_scalar` say the same once more, term by term in Python integers and floats, and hold the vectorised forms
(tests/test_resample_host.py).

Every f64 operation here is one rounded add, subtract, multiply or divide, in the definition's order: np.cumsum adds its
terms one after the other, and a running sum that starts at +0.0 is never -0.0, so padding a segment with +0.0 changes no bit."""
import math

import numpy as np

G = 0x9E3779B97F4A7C15
MASK = (1 << 64) - 1
SEG = 256
MAX_SYSTEMS = 8
MAX_TRIALS = 1 << 20
LDS_BYTES = 128 * 1024
CHUNK_CELLS = 1 << 22  # (trials x queries cells held at once)


def mix_int(z):
    z &= MASK
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return z


def boot_key(seed):
    return mix_int(seed + 1 * G)


def perm_key(seed):
    return mix_int(seed + 2 * G)


def mix(z):
    """mix_int over a uint64 array (arithmetic mod 2^64)"""
    with np.errstate(over="ignore"):
        z = z ^ (z >> np.uint64(30))
        z = z * np.uint64(0xBF58476D1CE4E5B9)
        z = z ^ (z >> np.uint64(27))
        z = z * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z


def _high_words(key, trials, Q):
    """(mix(key + G (t Q + k + 1)) >> 32) for the trials `trials` (an int array) and k = 0 .. Q-1: uint64[len(trials), Q]"""
    with np.errstate(over="ignore"):
        ctr = np.asarray(trials, dtype=np.uint64)[:, None] * np.uint64(Q) + np.arange(1, Q + 1, dtype=np.uint64)[None, :]
        z = mix(np.uint64(key) + np.uint64(G) * ctr)
    return z >> np.uint64(32)


def draws(seed, trials, Q):
    """i(t, k) of the bootstrap: int64[len(trials), Q]"""
    return ((_high_words(boot_key(seed), trials, Q) * np.uint64(Q)) >> np.uint64(32)).astype(np.int64)


def permutations(seed, trials, Q, M):
    """p of the permutation procedure: int64[len(trials), Q, M]"""
    r = ((_high_words(perm_key(seed), trials, Q) * np.uint64(math.factorial(M))) >> np.uint64(32)).astype(np.int64)
    p = np.broadcast_to(np.arange(M, dtype=np.int64), r.shape + (M,)).copy()
    for i in range(M - 1, 0, -1):
        j = (r % (i + 1))[..., None]
        r = r // (i + 1)
        at_i = p[..., i:i + 1].copy()
        at_j = np.take_along_axis(p, j, axis=-1)
        np.put_along_axis(p, j, at_i, axis=-1)
        p[..., i:i + 1] = at_j  # (j == i: at_j is the old p[i], which is put back)
    return p


def seq_sum(X):
    """SUM along the last axis: segments of SEG terms added one after the other from +0.0, the partials likewise"""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[-1]
    nseg = max(1, -(-n // SEG))
    padded = np.zeros(X.shape[:-1] + (nseg * SEG,), dtype=np.float64)
    padded[..., :n] = X
    segs = padded.reshape(X.shape[:-1] + (nseg, SEG))
    zero = np.zeros(segs.shape[:-1] + (1,), dtype=np.float64)
    parts = np.cumsum(np.concatenate([zero, segs], axis=-1), axis=-1)[..., -1]
    zero = np.zeros(parts.shape[:-1] + (1,), dtype=np.float64)
    return np.cumsum(np.concatenate([zero, parts], axis=-1), axis=-1)[..., -1]


def means(V):
    V = np.asarray(V, dtype=np.float64)
    return seq_sum(V.T) / np.float64(V.shape[0])


def _chunks(T, Q):
    step = max(1, CHUNK_CELLS // max(1, Q))
    for t0 in range(0, T, step):
        yield np.arange(t0, min(T, t0 + step))


def boot(V, T, seed):
    """boot[t][c] = SUM_k V[i(t,k)][c] / Q: float64[T, M]"""
    V = np.asarray(V, dtype=np.float64)
    Q, M = V.shape
    out = np.empty((T, M), dtype=np.float64)
    for ts in _chunks(T, Q):
        idx = draws(seed, ts, Q)
        for c in range(M):
            out[ts, c] = seq_sum(V[:, c][idx]) / np.float64(Q)
    return out


def perm(V, T, seed):
    """perm[t][c] = SUM_q V[q][p[c]] / Q: float64[T, M]"""
    V = np.asarray(V, dtype=np.float64)
    Q, M = V.shape
    out = np.empty((T, M), dtype=np.float64)
    for ts in _chunks(T, Q * M):
        p = permutations(seed, ts, Q, M)
        W = np.take_along_axis(np.broadcast_to(V, p.shape), p, axis=-1)
        for c in range(M):
            out[ts, c] = seq_sum(W[:, :, c]) / np.float64(Q)
    return out


def _sum_scalar(xs):
    total = 0.0
    for s0 in range(0, len(xs), SEG):
        part = 0.0
        for x in xs[s0:s0 + SEG]:
            part = part + x
        total = total + part
    return total


def boot_scalar(V, T, seed):
    """`boot`, term by term"""
    V = np.asarray(V, dtype=np.float64)
    Q, M = V.shape
    K = boot_key(seed)
    out = np.empty((T, M), dtype=np.float64)
    for t in range(T):
        rows = [(((mix_int(K + G * (t * Q + k + 1)) >> 32) * Q) >> 32) for k in range(Q)]
        for c in range(M):
            out[t, c] = _sum_scalar([float(V[i, c]) for i in rows]) / float(Q)
    return out


def perm_scalar(V, T, seed):
    """`perm`, term by term"""
    V = np.asarray(V, dtype=np.float64)
    Q, M = V.shape
    K = perm_key(seed)
    out = np.empty((T, M), dtype=np.float64)
    for t in range(T):
        cols = [[] for _ in range(M)]
        for q in range(Q):
            r = ((mix_int(K + G * (t * Q + q + 1)) >> 32) * math.factorial(M)) >> 32
            p = list(range(M))
            for i in range(M - 1, 0, -1):
                j = r % (i + 1)
                r = r // (i + 1)
                p[i], p[j] = p[j], p[i]
            for c in range(M):
                cols[c].append(float(V[q, p[c]]))
        for c in range(M):
            out[t, c] = _sum_scalar(cols[c]) / float(Q)
    return out


def percentile(sorted_values, percentile_):
    """The reference's PercentileStats::percentile (src/stats.rs:142-155) as written: the fractional part of the position
    weighs the LOWER order statistic, one minus it the upper one."""
    data = [float(x) for x in sorted_values]
    n = percentile_ * float(len(data) - 1)
    lhs = int(math.trunc(n))
    rhs = min(len(data), int(math.ceil(n)))
    interp = n - math.trunc(n)
    if lhs == rhs:
        return data[lhs]
    return (interp * data[lhs]) + (1.0 - interp) * data[rhs]


def interval(sorted_values, alpha):
    last = float(len(sorted_values) - 1)
    lo = int(math.floor(alpha / 2.0 * last))
    hi = min(len(sorted_values) - 1, int(math.ceil((1.0 - alpha / 2.0) * last)))
    return [float(sorted_values[lo]), float(sorted_values[hi])]


def p_values(V, perm_means):
    """{(i, j): (1 + #{t : range[t] >= |m[i] - m[j]|}) / (T + 1)}"""
    m = means(V)
    rng = perm_means.max(axis=1) - perm_means.min(axis=1)
    T = perm_means.shape[0]
    M = len(m)
    return {(i, j): float(1 + int(np.count_nonzero(rng >= abs(m[i] - m[j])))) / float(T + 1) for i in range(M) for j in range(i + 1, M)}


def report(V, alpha, boot_means=None, perm_means=None):
    """The host's report (csrc/resample_host.hpp, resample_report) of the table and the two arrays; a part whose array is
    None is left out, as the C call leaves it out."""
    V = np.asarray(V, dtype=np.float64)
    Q, M = V.shape
    m = means(V)
    out = {"means": [float(x) for x in m]}
    if boot_means is not None:
        cols = [np.sort(boot_means[:, c]) for c in range(M)]
        out["intervals"] = [interval(col, alpha) for col in cols]
        out["summary"] = [dict((name, percentile(col, at)) for name, at in (("p5", 0.05), ("p25", 0.25), ("p50", 0.5), ("p75", 0.75), ("p95", 0.95)))
                          for col in cols]
    ps = p_values(V, perm_means) if perm_means is not None else {}
    out["pairs"] = []
    for i in range(M):
        for j in range(i + 1, M):
            rec = {"i": i, "j": j, "diff": float(m[i] - m[j])}
            if boot_means is not None:
                rec["diff_interval"] = interval(np.sort(boot_means[:, i] - boot_means[:, j]), alpha)
            if perm_means is not None:
                rec["p"] = ps[(i, j)]
            rec["wins"] = int(np.count_nonzero(V[:, i] > V[:, j]))
            rec["losses"] = int(np.count_nonzero(V[:, i] < V[:, j]))
            rec["ties"] = int(np.count_nonzero(V[:, i] == V[:, j]))
            out["pairs"].append(rec)
    return out


REPORT_KEYS = ("means", "intervals", "summary", "pairs")


def designed_table(Q, M, seed):
    """N(0,1) 10^U{-8..8}: magnitudes so far apart that the order of the additions shows in the sum's bits"""
    rng = np.random.default_rng(seed)
    return rng.normal(size=(Q, M)) * 10.0 ** rng.integers(-8, 9, size=(Q, M)).astype(np.float64)


def visible_table(Q, M):
    """The first designed_table(Q, M, seed), seed = 0, 1, .., on every column of which the sum's shape shows (at Q = 258 the
    second segment holds two terms, and about half of all columns cannot tell)."""
    for seed in range(100000):
        V = designed_table(Q, M, seed)
        if all(sum_shape_is_visible(V)):
            return V
    raise AssertionError("no table of %d x %d shows the sum's shape" % (Q, M))


def sum_shape_is_visible(V):
    """per column: SUM over the queries differs from the plain sequential sum and from np.sum (pairwise) on this input"""
    V = np.asarray(V, dtype=np.float64)
    plain = np.cumsum(V, axis=0)[-1]
    shaped = seq_sum(V.T)
    return [bool(shaped[c] != plain[c] and shaped[c] != np.sum(V[:, c])) for c in range(V.shape[1])]
