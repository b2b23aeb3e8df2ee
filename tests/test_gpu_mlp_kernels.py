"""The NeuralNet kernels (csrc/kernels_mlp.inc) through their hooks: bit for bit against integer sums
where every product and partial sum is exact, and within derived bounds against exact rational sums on continuous data."""
import os
from fractions import Fraction

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import native
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

# query lengths: one document; 63 / 64 / 65 in one query; a second query across a tile boundary
# and 70 queries of 11 whole tiles + one document = 771 tiles: above 768 tiles a workgroup's stretch is two tiles
LAYOUTS = {"one": [1], "q63": [63], "q64": [64], "q65": [65], "straddle": [40, 50], "stretches_plus_one": [704] * 70 + [1]}
WIDTHS = [1, 15, 16, 17, 136, 144, 145]  # 144 features fill one panel; 145 is the first width of a second one
HIDDEN = [1, 16, 17, 64, 65]        # 65 is the first unit of a second hidden panel
KEYS = ("hidden_weights", "hidden_bias", "output_weights")


def _net(W1, b1, w2, b2):
    return fr.CModel.from_dict({"NeuralNet": {"activation": "relu", "hidden_weights": np.asarray(W1).tolist(), "hidden_bias": np.asarray(b1).tolist(),
                                              "output_weights": np.asarray(w2).tolist(), "output_bias": float(b2)}})


def _exact_case(seed, d, h, lens):
    """Integer features in [-8, 8], parameters / lambda in eighths: every product and partial sum is exact in any order.  With
    two units or more, unit 0 has z = 0 everywhere (derivative 0) and the last unit's bias keeps it mostly negative."""
    rng = np.random.default_rng(seed)
    n = int(sum(lens))
    X = rng.integers(-8, 9, size=(n, d)).astype(np.float32)
    qid = np.repeat(np.arange(1, len(lens) + 1, dtype=np.int64), lens)
    y = rng.integers(0, 3, n).astype(np.float64)
    W8, b8, w8 = rng.integers(-4, 5, (h, d)), rng.integers(-16, 17, h), rng.integers(-8, 9, h)
    if h > 1:
        W8[0], b8[0], b8[-1] = 0, 0, -200
    return X, y, qid, W8, b8, w8, int(rng.integers(-8, 9)), rng.integers(-16, 17, n)


def _exact_sums(X, W8, b8, w8, b2_8, lam8, rows):
    """(scores of every row; the four gradient sums over `rows`), float64 of integer sums scaled by powers of two."""
    Xi = X.astype(np.int64)
    z8 = b8 + Xi @ W8.T
    a8 = np.maximum(z8, 0)
    scores = (8 * b2_8 + a8 @ w8) / 64.0
    on, lam = (z8[rows] > 0), lam8[rows]
    delta64 = on * (lam[:, None] * w8[None, :])
    return scores, {"hidden_weights": delta64.T @ Xi[rows] / 64.0, "hidden_bias": delta64.sum(0) / 64.0,
                    "output_weights": (lam[:, None] * a8[rows]).sum(0) / 64.0, "output_bias": lam.sum() / 8.0}


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64), np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))


def _check(ds, model, lam, exp_scores, exp_grads, score_rows=None, **kw):
    got = native.predict_scores_dense(model, ds, n_total=len(exp_scores))
    rows = np.arange(len(exp_scores)) if score_rows is None else score_rows
    assert _same_bits(got[rows], exp_scores[rows]) and np.isnan(np.delete(got, rows)).all()
    grads = native.mlp_gradients(ds, model, lam, **kw)
    for key in KEYS:
        assert _same_bits(grads[key], exp_grads[key]), key
    assert grads["output_bias"] == exp_grads["output_bias"]
    return grads


@pytest.mark.parametrize("h", HIDDEN)
@pytest.mark.parametrize("d", WIDTHS)
def test_every_width_gives_the_exact_sums(d, h):
    X, y, qid, W8, b8, w8, b2_8, lam8 = _exact_case(1000 * d + h, d, h, [65])
    ds, model = fr.CDataset.from_numpy(X, y, qid), _net(W8 / 8.0, b8 / 8.0, w8 / 8.0, b2_8 / 8.0)
    scores, grads = _exact_sums(X, W8, b8, w8, b2_8, lam8, np.arange(len(qid)))
    assert h == 1 or (grads["hidden_weights"][0] == 0).all()
    plan = {}
    _check(ds, model, lam8 / 8.0, scores, grads, plan=plan)
    assert plan["feature_panels"] == (1 if d <= 144 else 2) and plan["hidden_panels"] == (1 if h <= 64 else 2)
    assert plan["resident"] == (d <= 144) and plan["workgroups"] == 2 and plan["stretch_tiles"] == 1


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("d,h", [(17, 17), (145, 65)])
def test_every_layout_gives_the_exact_sums(d, h, layout):
    """One tile per workgroup; and above 768 tiles a stretch of several (accumulators in registers): whole stretches plus one document."""
    X, y, qid, W8, b8, w8, b2_8, lam8 = _exact_case(7 * d + len(layout), d, h, LAYOUTS[layout])
    ds, model = fr.CDataset.from_numpy(X, y, qid), _net(W8 / 8.0, b8 / 8.0, w8 / 8.0, b2_8 / 8.0)
    scores, grads = _exact_sums(X, W8, b8, w8, b2_8, lam8, np.arange(len(qid)))
    plan = {}
    first = _check(ds, model, lam8 / 8.0, scores, grads, plan=plan)
    stretch = plan["stretch_tiles"]
    assert plan["tiles"] == (len(qid) + 63) // 64 and plan["workgroups"] == -(-plan["tiles"] // stretch)
    if layout == "stretches_plus_one":
        assert stretch >= 2 and (len(qid) - 1) % (64 * stretch) == 0
    again = native.mlp_gradients(ds, model, lam8 / 8.0)  # two calls, the same bytes
    assert all(_same_bits(first[k], again[k]) for k in KEYS) and first["output_bias"] == again["output_bias"]
    assert _same_bits(native.predict_scores_dense(model, ds), native.predict_scores_dense(model, ds))


def test_only_visited_queries_are_read():
    """A query-sampled view and a `queries` list: every other lambda is NaN and reaches no sum; a view scores its own documents only."""
    lens = [30, 70, 1, 64, 90, 5, 129]
    X, y, qid, W8, b8, w8, b2_8, lam8 = _exact_case(5, 17, 20, lens)
    ds, model = fr.CDataset.from_numpy(X, y, qid), _net(W8 / 8.0, b8 / 8.0, w8 / 8.0, b2_8 / 8.0)
    visit = [1, 3, 6]  # indices of the dataset's queries, its order
    rows = np.flatnonzero(np.isin(qid, [q + 1 for q in visit]))
    lam = np.full(len(qid), np.nan)
    lam[rows] = lam8[rows] / 8.0
    scores, grads = _exact_sums(X, W8, b8, w8, b2_8, lam8, rows)
    _check(ds, model, lam, scores, grads, queries=visit)
    view = ds.subsample_queries([str(q + 1) for q in visit])
    _check(view, model, lam, scores, grads, score_rows=rows)
    rows2 = np.flatnonzero(np.isin(qid, [2, 7]))  # (the view's own order: queries 2 and 7 of the dataset)
    _check(view, model, lam, scores, _exact_sums(X, W8, b8, w8, b2_8, lam8, rows2)[1], score_rows=rows, queries=[0, 2])


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
    _, _, _, W8, b8, w8, b2_8, lam8 = _exact_case(11, d, 9, [n])
    scores, grads = _exact_sums(X, W8, b8, w8, b2_8, lam8, np.arange(n))
    _check(ds, _net(W8 / 8.0, b8 / 8.0, w8 / 8.0, b2_8 / 8.0), lam8 / 8.0, scores, grads)
    short = _net(W8[:, :5] / 8.0, b8 / 8.0, w8 / 8.0, b2_8 / 8.0)  # a model with fewer columns reads the others as 0
    W5 = np.where(np.arange(d) < 5, W8, 0)
    scores, grads = _exact_sums(X, W5, b8, w8, b2_8, lam8, np.arange(n))
    _check(ds, short, lam8 / 8.0, scores, grads)


def continuous_case(d, h, n):
    """Seeded normal data and its exact sums as Fractions: (arrays, z, per-(p, j) bound on the error of z)."""
    rng = np.random.default_rng(100 * d + h)
    X = rng.normal(0.0, 1.0, (n, d)).astype(np.float32)
    W1, b1, w2, b2, lam = rng.normal(0.0, 0.3, (h, d)), rng.normal(0.0, 0.5, h), rng.normal(0.0, 1.0, h), float(rng.normal()), rng.normal(0.0, 1.0, n)
    F = lambda a: [Fraction(float(v)) for v in a]  # noqa: E731
    xf, wf, bf = [F(r) for r in X], [F(r) for r in W1], F(b1)
    u = Fraction(1, 2 ** 53)
    gamma = lambda k: k * u / (1 - k * u)  # noqa: E731
    z = [[bf[j] + sum(x * w for x, w in zip(xf[p], wf[j])) for j in range(h)] for p in range(n)]
    ez = [[gamma(d + 1) * (abs(bf[j]) + sum(abs(x * w) for x, w in zip(xf[p], wf[j]))) for j in range(h)] for p in range(n)]
    return (X, W1, b1, w2, b2, lam), (xf, F(w2), Fraction(b2), F(lam)), z, ez, gamma


@pytest.mark.parametrize("d,h,n", [(17, 17, 150), (136, 64, 24)])
def test_continuous_data_stays_within_the_derived_bounds(d, h, n):
    """z carries d + 1 terms (each product rounded at most once, d additions in some order): |error| <= gamma_(d+1) (|b1| + sum
    |x W1|) = ez.  The sign of z, which ReLU and its derivative read, is therefore the exact one wherever |z| > ez: asserted for
    every (p, j) first.  Then, to first order: a score's h + 1 terms fl(a w2) add gamma_(h+1) sum |a w2| to sum |w2| ez; G_b2 is
    n terms; G_b1 n terms of one rounding each; G_w2 n terms fl(lambda a) whose a carries ez; G_W1 n terms of two roundings
    (lambda w2, then the product with x).  gamma_k = k u / (1 - k u), u = 2^-53.  The largest error / bound ratios go to
    profiles/mlp_error.txt."""
    (X, W1, b1, w2, b2, lam), (xf, w2f, b2f, lamf), z, ez, gamma = continuous_case(d, h, n)
    assert all(abs(z[p][j]) > ez[p][j] for p in range(n) for j in range(h))
    qid = np.repeat(np.arange(1, 4, dtype=np.int64), [n - 2 * (n // 3), n // 3, n // 3])
    ds, model = fr.CDataset.from_numpy(X, np.zeros(n), qid), _net(W1, b1, w2, b2)
    scores, grads = native.predict_scores_dense(model, ds), native.mlp_gradients(ds, model, lam)
    worst = {"score": Fraction(0), **{k: Fraction(0) for k in KEYS}, "output_bias": Fraction(0)}

    def hold(name, got, exact, bound):
        err = abs(Fraction(float(got)) - exact)
        assert err <= bound, (name, float(err), float(bound))
        if bound > 0:
            worst[name] = max(worst[name], err / bound)

    a = [[max(z[p][j], 0) for j in range(h)] for p in range(n)]
    for p in range(n):
        terms = [a[p][j] * w2f[j] for j in range(h)]
        hold("score", scores[p], b2f + sum(terms),
             gamma(h + 1) * sum(abs(t) for t in terms) + sum(abs(w2f[j]) * ez[p][j] for j in range(h)))
    hold("output_bias", grads["output_bias"], sum(lamf), gamma(n) * sum(abs(v) for v in lamf))
    for j in range(h):
        on = [p for p in range(n) if z[p][j] > 0]
        dl = [lamf[p] * w2f[j] for p in on]
        hold("hidden_bias", grads["hidden_bias"][j], sum(dl), gamma(n + 1) * sum(abs(t) for t in dl))
        la = [lamf[p] * a[p][j] for p in on]
        hold("output_weights", grads["output_weights"][j], sum(la), gamma(n + 1) * sum(abs(t) for t in la) + sum(abs(lamf[p]) * ez[p][j] for p in on))
        for i in range(d):
            terms = [t * xf[p][i] for t, p in zip(dl, on)]
            hold("hidden_weights", grads["hidden_weights"][j, i], sum(terms), gamma(n + 2) * sum(abs(t) for t in terms))
    path = os.path.join(ROOT, "profiles", "mlp_error.txt")  # (rewritten only when a figure moved: the kernels are deterministic)
    old = open(path).read() if os.path.exists(path) else ""
    line = "d=%d h=%d n=%d largest |error| / bound: " % (d, h, n) + ", ".join("%s %.6f" % (k, float(v)) for k, v in worst.items())
    new = "\n".join(sorted([ln for ln in old.splitlines() if not ln.startswith("d=%d " % d)] + [line])) + "\n"
    if new != old:
        with open(path, "w") as fh:
            fh.write(new)
