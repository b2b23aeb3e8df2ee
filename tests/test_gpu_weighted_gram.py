"""The weighted Gram kernel pair (csrc/kernels_gram.inc) through native.weighted_gram: bit for bit
against integer sums where every product and partial sum is exact in float64, and within the summation bound against exact
rational sums on continuous data."""
import os
from fractions import Fraction

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import native
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

# query lengths: one document; 63 / 64 / 65 in one query; a second query across a tile boundary; three one-tile stretches + 1
LAYOUTS = {"one": [1], "q63": [63], "q64": [64], "q65": [65], "straddle": [40, 50], "three_stretches_plus_one": [193]}
# 143 columns fill one pass (144 with lambda's); 144 is the first width that takes a second one
WIDTHS = [1, 15, 16, 17, 136, 144]


def _exact_case(seed, d, lens):
    rng = np.random.default_rng(seed)
    n = int(sum(lens))
    X = rng.integers(-8, 9, size=(n, d)).astype(np.float32)
    qid = np.repeat(np.arange(1, len(lens) + 1, dtype=np.int64), lens)
    y = rng.integers(0, 3, n).astype(np.float64)
    k = rng.integers(0, 65, n)
    m = rng.integers(-64, 65, n)
    return X, y, qid, k, m


def _exact_sums(X, k, m, rows):
    """H and g over `rows` as float64 of integer sums / 64 (exact: every sum is far below 2^53)."""
    Xi = X[rows].astype(np.int64)
    return (Xi.T * k[rows]) @ Xi / 64.0, Xi.T @ m[rows] / 64.0


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("d", WIDTHS)
def test_integer_data_gives_the_exact_sums(d, layout):
    lens = LAYOUTS[layout]
    X, y, qid, k, m = _exact_case(1000 * d + len(layout), d, lens)
    ds = fr.CDataset.from_numpy(X, y, qid)
    plan = {}
    H, g = native.weighted_gram(ds, m / 64.0, k / 64.0, plan=plan)
    eH, eg = _exact_sums(X, k, m, np.arange(len(qid)))
    assert _same_bits(H, eH) and _same_bits(g, eg)
    assert _same_bits(H, H.T)
    assert plan["passes"] == (1 if d <= 143 else 2) and plan["stretch_tiles"] == 1
    if layout == "three_stretches_plus_one":
        assert plan["workgroups"] == 4


def test_only_visited_queries_are_read():
    """A query-sampled view and a `queries` list: the other queries' lambda and w are NaN in the uploaded arrays (and the hook
    uploads NaN wherever no document sits), and none of it reaches a sum."""
    lens = [30, 70, 1, 64, 90, 5, 129]
    X, y, qid, k, m = _exact_case(5, 17, lens)
    ds = fr.CDataset.from_numpy(X, y, qid)
    visit = [1, 3, 6]  # indices of the dataset's queries, its order
    rows = np.flatnonzero(np.isin(qid, [q + 1 for q in visit]))
    lam, wt = np.full(len(qid), np.nan), np.full(len(qid), np.nan)
    lam[rows], wt[rows] = m[rows] / 64.0, k[rows] / 64.0
    eH, eg = _exact_sums(X, k, m, rows)
    H, g = native.weighted_gram(ds, lam, wt, queries=visit)
    assert _same_bits(H, eH) and _same_bits(g, eg)
    view = ds.subsample_queries([str(q + 1) for q in visit])
    H, g = native.weighted_gram(view, lam, wt)
    assert _same_bits(H, eH) and _same_bits(g, eg)
    H, g = native.weighted_gram(view, lam, wt, queries=[0, 2])  # (the view's own order: queries 2 and 7 of the dataset)
    rows = np.flatnonzero(np.isin(qid, [2, 7]))
    eH, eg = _exact_sums(X, k, m, rows)
    assert _same_bits(H, eH) and _same_bits(g, eg)


def test_a_file_loaded_dataset_reads_absent_values_as_zero(tmp_path):
    rng = np.random.default_rng(9)
    n, d = 150, 21  # (feature ids 1..20 of the file; the last row is dense, so the dataset has d columns)
    held = rng.random((n, d)) < np.where(np.arange(n) % 2, 0.9, 0.2)[:, None]
    held[:, 0], held[:, 1], held[n - 1, 1:] = False, True, True
    X = np.where(held, rng.integers(-8, 9, (n, d)), 0).astype(np.float32)
    path = tmp_path / "absent.train"
    path.write_text("".join("%d qid:%d %s\n" % (i % 3, 1 + i // 60, " ".join("%d:%d" % (f, X[i, f]) for f in np.flatnonzero(held[i])))
                            for i in range(n)))
    ds = fr.CDataset.open_ranksvm(str(path))
    k, m = rng.integers(0, 65, n), rng.integers(-64, 65, n)
    H, g = native.weighted_gram(ds, m / 64.0, k / 64.0)
    eH, eg = _exact_sums(X, k, m, np.arange(n))
    assert H.shape == (d, d) and _same_bits(H, eH) and _same_bits(g, eg)


@pytest.mark.parametrize("d,n", [(17, 200), (136, 66)])
def test_continuous_data_stays_within_the_summation_bound(d, n):
    """Random f32 features and f64 lambda, w against sums of exact Fraction products.  Every entry lies within
    gamma_(n+1) * sum_p |x_pi w_p x_pj|, gamma_k = k u / (1 - k u), u = 2^-53: a term carries at most two roundings (w x_pj,
    then its product with x_pi, fused into the addition or not) and the n terms meet in n - 1 additions, in any order.  g has
    one rounding less per term and is held to the same bound.  The largest error / bound ratio goes to profiles/gram_error.txt."""
    rng = np.random.default_rng(d)
    X = rng.normal(0.0, 1.0, (n, d)).astype(np.float32)
    qid = np.repeat(np.arange(1, 4, dtype=np.int64), [n - 2 * (n // 3), n // 3, n // 3])
    y = rng.integers(0, 3, n).astype(np.float64)
    lam, wt = rng.normal(0.0, 1.0, n), rng.random(n)
    ds = fr.CDataset.from_numpy(X, y, qid)
    H, g = native.weighted_gram(ds, lam, wt)
    assert _same_bits(H, H.T)
    H2, g2 = native.weighted_gram(ds, lam, wt)
    assert _same_bits(H, H2) and _same_bits(g, g2)
    u = Fraction(1, 2 ** 53)
    gamma = (n + 1) * u / (1 - (n + 1) * u)
    xf = [[Fraction(float(v)) for v in row] for row in X]
    right = [[Fraction(float(wt[p])) * xf[p][j] for j in range(d)] + [Fraction(float(lam[p]))] for p in range(n)]  # B = [w x | lambda]
    worst = Fraction(0)
    for i in range(d):
        for j in list(range(i, d)) + [d]:
            terms = [xf[p][i] * right[p][j] for p in range(n)]
            bound = gamma * sum(abs(t) for t in terms)
            err = abs(Fraction(float(g[i] if j == d else H[i, j])) - sum(terms))
            assert err <= bound, (i, j, float(err), float(bound))
            if bound > 0:
                worst = max(worst, err / bound)
    path = os.path.join(ROOT, "profiles", "gram_error.txt")  # (rewritten only when a figure moved: the kernel is deterministic)
    old = open(path).read() if os.path.exists(path) else ""
    new = "\n".join(sorted([ln for ln in old.splitlines() if not ln.startswith("d=%d " % d)]
                           + ["d=%d n=%d largest |error| / bound = %.6f" % (d, n, float(worst))])) + "\n"
    if new != old:
        with open(path, "w") as fh:
            fh.write(new)
