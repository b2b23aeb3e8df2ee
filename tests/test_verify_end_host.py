"""The arithmetic of a query's end in the NDCG@k bound-and-verify kernel (csrc/verify_end.hpp), on the CPU, through the copy of
it the library compiles for the host (fr_debug_verify_end):

  * the per-query gap bound: `diff > tau` must imply the exact pair test `verify_far` for every pair of a sorted list -- held
    against a numpy restatement of both on more than 10^7 lists (mixed signs, magnitudes 1e-300 .. 1e290, gaps at the bound and
    one and two ulps to either side of it, -inf tails behind queries of 1 .. K + 1 documents);
  * the division-free quotient: bitwise the IEEE division for every sequential sum the bench's term tables (five gain classes)
    can produce at K <= 10 against every ideal DCG those classes can produce at depth 5 and 10, and for 10^8 random pairs
    spread over the whole range the argument in verify_end.hpp covers."""
import ctypes
import itertools
from fractions import Fraction

import numpy as np

from fastrank_amd import clib

K = 10


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _hook(which, a, b, c=None, d=None, n_out=None):
    arrs = [None if v is None else np.ascontiguousarray(v, dtype=np.float64) for v in (a, b, c, d)]
    out = np.empty(len(arrs[0]) if n_out is None else n_out, dtype=np.float64)
    rc = clib._load().fr_debug_verify_end(int(which), len(arrs[0]), *[_ptr(v) for v in arrs], _ptr(out))
    assert rc == 0
    return out


def _fma(a, b, c):
    a, b, c = np.broadcast_arrays(a, b, c)
    return _hook(2, a.ravel(), b.ravel(), c.ravel()).reshape(a.shape)


# ---- the numpy restatement ------------------------------------------------------------------------------------------
def tau_np(first, last, gam, eps0):
    B = np.maximum(np.abs(first), np.abs(last))
    return np.where(gam >= 0.0, _fma(gam, B + B, eps0), np.inf)


def cheap_np(ka, kb, tau):
    return (ka - kb) > tau


def far_np(ka, kb, eps0, gam):
    return (ka - kb) > _fma(gam, np.abs(ka) + np.abs(kb), eps0)


def test_fma_primitive_is_the_correctly_rounded_fma():
    rng = np.random.default_rng(1)
    n = 3000
    a = rng.normal(0, 1, n) * 2.0 ** rng.integers(-200, 200, n)
    b = rng.normal(0, 1, n) * 2.0 ** rng.integers(-200, 200, n)
    c = -(a * b) * (1.0 + rng.normal(0, 1, n) * 2.0 ** rng.integers(-60, 1, n))   # heavy cancellation
    c[::7] = rng.normal(0, 1, len(c[::7]))
    got = _fma(a, b, c)
    for x, y, z, g in zip(a.tolist(), b.tolist(), c.tolist(), got.tolist()):
        assert g == float(Fraction(x) * Fraction(y) + Fraction(z)), (x, y, z)   # (int / int division rounds correctly)


GAMMAS = np.array([0.0, 2.5 * 7 * 2.0 ** -53, 2.5 * 137 * 2.0 ** -53, 2.5 * 701 * 2.0 ** -53, 1e-10, 0.5])
EPS_REL = np.array([0.0, 1e-16, 1e-13, 1e-9, 1e-3, 1.0])


def _lists(rng, n, kind):
    """n lists of K + 1 keys, sorted descending"""
    e = rng.uniform(-996.0, 963.0, (n, 1))                        # 1e-300 .. 1e290
    M = 2.0 ** np.floor(e) * (1.0 + rng.random((n, 1)))
    if kind == 0:    # one scale, mixed signs
        keys = M * rng.uniform(-1.0, 1.0, (n, K + 1))
    elif kind == 1:  # near-ties: relative gaps 2^-20 .. 2^-60 (and exact ties), either sign
        gaps = 2.0 ** -rng.integers(20, 61, (n, K + 1)).astype(np.float64) * (rng.random((n, K + 1)) < 0.8)
        keys = rng.choice([-1.0, 1.0], (n, 1)) * M * (1.0 - np.cumsum(gaps, axis=1))
    else:            # every magnitude in one list
        ee = rng.uniform(-996.0, 963.0, (n, K + 1))
        keys = rng.choice([-1.0, 1.0], (n, K + 1)) * 2.0 ** np.floor(ee) * (1.0 + rng.random((n, K + 1)))
    keys = -np.sort(-keys, axis=1)
    gam = rng.choice(GAMMAS, n)
    eps0 = rng.choice(EPS_REL, n) * M[:, 0] * rng.choice([1.0, 1e-30, 0.0], n, p=[0.8, 0.1, 0.1])
    eps0[::97] = 5e-324
    return keys, gam, eps0


def test_gap_bound_implies_verify_far_on_sorted_lists():
    rng = np.random.default_rng(2)
    chunks, per = 21, 500_000           # 1.05e7 lists, 1.05e8 pairs
    seen = dict(cheap=0, open_far=0, close=0, at_bound=0, lists=0)
    with np.errstate(all="ignore"):
        for ch in range(chunks):
            keys, gam, eps0 = _lists(rng, per, ch % 3)
            tau = tau_np(keys[:, 0], keys[:, K], gam, eps0)
            assert np.array_equal(tau, _hook(1, keys[:, 0], keys[:, K], gam, eps0))   # the kernel's own function
            # a gap at the bound: an inner key (never the first or the last, which make the bound) moved to tau below its upper
            # neighbour, where it stays above its lower one -- then 0, 1, 2 ulps up or down
            j = rng.integers(0, K - 1, per)
            rows = np.arange(per)
            ka = keys[rows, j]
            kb = ka - tau
            for _ in range(abs((ch % 5) - 2)):
                kb = np.nextafter(kb, np.inf if ch % 5 > 2 else -np.inf)
            fits = np.isfinite(tau) & (kb <= ka) & (kb >= keys[rows, j + 2]) & (ch % 2 == 0 or rng.random(per) < 0.5)
            keys[rows[fits], j[fits] + 1] = kb[fits]
            assert (np.diff(keys, axis=1) <= 0.0).all()
            ka, kb = keys[:, :K], keys[:, 1:]
            cheap = cheap_np(ka, kb, tau[:, None])
            far = far_np(ka, kb, eps0[:, None], gam[:, None])
            assert not (cheap & ~far).any(), ch
            seen["cheap"] += int(cheap.sum())
            seen["open_far"] += int((~cheap & far).sum())
            seen["close"] += int((~far).sum())
            seen["at_bound"] += int(((ka - kb) == tau[:, None]).sum())
            seen["lists"] += per
    print("gap bound:", seen)
    assert seen["lists"] >= 10_000_000 and min(seen.values()) > 0, seen   # every outcome occurred, exact hits of the bound too


def test_gap_bound_ignores_the_padding_of_short_queries():
    rng = np.random.default_rng(3)
    per = 20_000
    with np.errstate(all="ignore"):
        for Kk in (5, 10):
            for depth in (Kk, Kk - 3):
                for n in range(1, Kk + 2):
                    keys, gam, eps0 = _lists(rng, per, n % 3)
                    keys = keys[:, :Kk + 1].copy()
                    keys[:, n:] = -np.inf                      # the list of a query with n documents
                    Ld = min(depth, n)
                    npair = min(Ld, n - 1)                     # pairs (i, i + 1) with i < Ld and i + 1 < n
                    assert [i for i in range(Kk) if i < Ld and i + 1 < n] == list(range(npair))
                    last = keys[:, npair]
                    assert np.isfinite(last).all()
                    tau = tau_np(keys[:, 0], last, gam, eps0)
                    assert np.array_equal(tau, _hook(1, keys[:, 0], last, gam, eps0))
                    assert np.isfinite(tau[np.isfinite(eps0)]).all()   # no -inf entered the bound
                    for i in range(npair):
                        cheap = cheap_np(keys[:, i], keys[:, i + 1], tau)
                        assert not (cheap & ~far_np(keys[:, i], keys[:, i + 1], eps0, gam)).any(), (Kk, depth, n, i)


def test_gap_bound_never_passes_on_a_meaningless_bound():
    first = np.array([5.0, 5.0, np.inf, 5.0, 1e308, 5.0])
    last = np.array([1.0, 1.0, 1.0, -np.inf, -1e308, 1.0])
    gam = np.array([-1e-16, np.nan, 1e-16, 1e-16, 1.0, 1e-16])
    eps0 = np.array([0.0, 0.0, 0.0, 0.0, 0.0, np.nan])
    with np.errstate(all="ignore"):
        tau = _hook(1, first, last, gam, eps0)
        assert not cheap_np(first, last, tau).any()            # inf or NaN: the comparison is false, the exact test decides


# ---- the quotient ---------------------------------------------------------------------------------------------------
GAINS = np.array([0.0, 1.0, 3.0, 7.0, 15.0])                     # 2^label - 1 for the bench's labels 0 .. 4
TERMS = GAINS[:, None] / np.log2(np.arange(K) + 2.0)[None, :]    # [class][rank]


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _all_sequential_sums():
    level, every = np.array([0.0]), [np.array([0.0])]
    for i in range(K):
        level = np.unique((level[:, None] + TERMS[None, :, i]).ravel())   # the sum after rank i depends on the sum before it only
        every.append(level)
    return np.unique(np.concatenate(every))


def _all_ideal_dcgs():
    norms = set()
    for depth in (5, K):
        for n in range(1, depth + 1):
            for seq in itertools.combinations_with_replacement((4, 3, 2, 1, 0), n):   # gain classes, descending
                if seq[0] == 0:
                    continue
                s = 0.0
                for i, c in enumerate(seq):
                    s = s + float(TERMS[c, i])
                norms.add(s)
    return np.array(sorted(norms))


def test_quotient_is_the_division_for_every_sum_and_norm_of_the_bench_tables():
    dcg, norms = _all_sequential_sums(), _all_ideal_dcgs()
    print("quotient: %d sums x %d norms" % (len(dcg), len(norms)))
    assert len(dcg) > 1_000_000 and len(norms) == 1000   # (non-increasing lists of 1 .. 10 classes from four positive gains)
    out = _hook(3, dcg, norms, np.array([float(len(norms))]), None, n_out=3)
    assert out[0] == 0.0, "first mismatch: dcg %r norm %r" % (out[1], out[2])
    sample = norms[:: max(1, len(norms) // 7)]
    for nm in sample:                                            # (and the elementwise entry point agrees with numpy's division)
        assert np.array_equal(_bits(_hook(0, dcg, np.full(len(dcg), nm))), _bits(dcg / nm))


def _random_doubles(rng, n, lo_exp, hi_exp):
    mant = rng.integers(0, 1 << 52, n, dtype=np.uint64)
    special = rng.integers(0, 10, n)
    mant[special == 0] = 0
    mant[special == 1] = (1 << 52) - 1
    mant[special == 2] = 1
    expo = rng.integers(lo_exp + 1023, hi_exp + 1023, n, dtype=np.uint64)
    return ((expo << np.uint64(52)) | mant).view(np.float64)


def test_quotient_is_the_division_on_random_pairs_over_the_proven_range():
    rng = np.random.default_rng(4)
    total = 0
    for ch in range(10):
        n = 10_000_000
        dcg = _random_doubles(rng, n, -112, 205) * rng.choice([1.0, -1.0], n, p=[0.8, 0.2])
        dcg[::1001] = 0.0
        norm = _random_doubles(rng, n, -256, 256)
        got = _hook(0, dcg, norm)
        bad = np.flatnonzero(_bits(got) != _bits(dcg / norm))
        assert len(bad) == 0, (dcg[bad[0]], norm[bad[0]])
        total += n
    assert total >= 100_000_000


def test_quotient_divides_outside_the_proven_range():
    dcg = np.array([0.0, 1.5, 1.5, 1.5, 1.5, 1.5, 0.0, 2.0 ** 300])
    norm = np.array([0.0, 0.0, np.inf, 5e-324, -3.0, 2.0 ** 300, np.nan, 2.0 ** -300])
    with np.errstate(all="ignore"):
        got, exp = _hook(0, dcg, norm), dcg / norm
    assert np.array_equal(got, exp, equal_nan=True) and np.array_equal(np.signbit(got), np.signbit(exp))
