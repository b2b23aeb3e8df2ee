"""numpy restatement of LambdaMART's listwise objective "xendcg" ("Listwise objective"), for the tests.

It restates the definition, not the device code.  Per visited query, documents i = 0..n-1 in stored order (instance ids
ascending), every operation f64 and rounded on its own:
  gamma_i = (mix(k + 0x9E3779B97F4A7C15 (id_i + 1)) >> 11) 2^-53, arithmetic mod 2^64, mix = the splitmix64 finaliser;
  phi_i = (gexp_i + 1.0) - gamma_i, Phi = SUM(phi); !(Phi > 0): zeros; inv = 1.0 / Phi;
  m = max s, e_i = exp(s_i - m), E = SUM(e), rho_i = e_i / E, u_i = 1.0 - rho_i, Q(x, i) = x / u_i if u_i > 0 else +0.0;
  t1_i = phi_i inv - rho_i, a_i = Q(t1_i, i), S1 = SUM(a); t2_i = rho_i (S1 - a_i), b_i = Q(t2_i, i), S2 = SUM(b);
  t3_i = rho_i (S2 - b_i); lambda_i = (t1_i + t2_i) + t3_i; w_i = rho_i u_i.
  SUM: 64 partials P_l = the elements i = l (mod 64) added one after the other in ascending i from +0.0, then
  P_l = P_l + P_{l+h} for l < h, h = 32, 16, 8, 4, 2, 1; the sum is P_0.
A query of one document, or whose norm is NaN or not > 0, gets lambda = w = +0.0.
The key of tree t is the t-th rand_u64() of Rand64(seed ^ 0x58454E4443475845) (the oracle's generator).
"""
import numpy as np

from oracle import pyoracle as o

XENDCG_STREAM = 0x58454E4443475845  # "XENDCGXE"
GOLDEN = 0x9E3779B97F4A7C15
MASK = 2 ** 64 - 1


def mix(z: int) -> int:
    """The splitmix64 finaliser, on Python integers."""
    z &= MASK
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return z


def gamma(key: int, ids) -> np.ndarray:
    """gamma of the original instance ids under the tree key (exact: 53 bits times 2^-53)."""
    return np.array([float(mix(int(key) + GOLDEN * (int(i) + 1)) >> 11) * 2.0 ** -53 for i in ids], dtype=np.float64)


def keys(seed: int, trees: int):
    """k_0 .. k_{trees-1} of the request's seed, as Python integers."""
    return [int(k) for k in o.rand64_stream((int(seed) ^ XENDCG_STREAM) & MASK, trees)]


def fixed_sum(x) -> np.float64:
    """SUM: the one fixed shape."""
    x = np.asarray(x, dtype=np.float64)
    P = np.zeros(64, dtype=np.float64)
    for b in range(0, len(x), 64):  # (row by row: lane l adds its next element)
        row = x[b:b + 64]
        P[:len(row)] = P[:len(row)] + row
    h = 32
    while h >= 1:
        P[:h] = P[:h] + P[h:2 * h]
        h //= 2
    return P[0]


def gains(y) -> np.ndarray:
    """The dataset's table 2^g - 1 of the f32 labels."""
    return np.array([2.0 ** float(x) - 1.0 for x in np.asarray(y, dtype=np.float32)], dtype=np.float64)


def query_gradients(s, gexp, ids, key, parts=False):
    """(lambda, w) of one live query of at least two documents; parts: also the dict of every intermediate value."""
    s = np.asarray(s, dtype=np.float64)
    n = len(s)
    zeros = np.zeros(n, dtype=np.float64)
    g = gamma(key, ids)
    phi = (np.asarray(gexp, dtype=np.float64) + 1.0) - g
    Phi = fixed_sum(phi)
    if not (Phi > 0.0):
        return (zeros, zeros.copy(), None) if parts else (zeros, zeros.copy())
    inv = np.float64(1.0) / Phi
    m = np.max(s)
    with np.errstate(under="ignore", over="ignore", invalid="ignore", divide="ignore"):
        e = np.exp(s - m)
        E = fixed_sum(e)
        rho = e / E
        u = 1.0 - rho
        live = u > 0.0
        safe = np.where(live, u, 1.0)

        def Q(x):
            return np.where(live, x / safe, 0.0)

        t1 = phi * inv - rho
        a = Q(t1)
        S1 = fixed_sum(a)
        t2 = rho * (S1 - a)
        b = Q(t2)
        S2 = fixed_sum(b)
        t3 = rho * (S2 - b)
        lam = (t1 + t2) + t3
        w = rho * u
    if parts:
        return lam, w, dict(gamma=g, phi=phi, Phi=Phi, e=e, E=E, rho=rho, u=u, t1=t1, a=a, S1=S1, t2=t2, b=b, S2=S2, t3=t3)
    return lam, w


def gradients(scores, y, queries, norms, key):
    """lambda, w by instance id (0.0 for every instance of a query that has nothing to learn from).  queries: per query the
    instance ids ascending; norms: the NDCG evaluator's, read for `> 0` only."""
    n = len(y)
    lam = np.zeros(n, dtype=np.float64)
    wt = np.zeros(n, dtype=np.float64)
    scores = np.asarray(scores, dtype=np.float64)
    G = gains(y)
    for q, ids in enumerate(queries):
        if len(ids) < 2 or not (float(norms[q]) > 0.0):
            continue
        lam[ids], wt[ids] = query_gradients(scores[ids], G[ids], ids, key)
    return lam, wt
