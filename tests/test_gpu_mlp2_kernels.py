"""The two-hidden-layer NeuralNet kernels (csrc/kernels_mlp2.inc; DESIGN.md section 19, "Two hidden layers") through
native.predict_scores_dense and native.mlp2_gradients: bit for bit against integer sums where every product and partial sum is
exact, and within derived bounds against exact rational sums on continuous data."""
import json
import os
from fractions import Fraction

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import clib, native
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

KEYS = ("hidden_weights", "hidden_bias", "hidden2_weights", "hidden2_bias", "output_weights")


def _net(W1, b1, W2, c, w3, b_out):
    return {"NeuralNet": {"activation": "relu", "hidden_weights": np.asarray(W1).tolist(), "hidden_bias": np.asarray(b1).tolist(),
                          "hidden2_weights": np.asarray(W2).tolist(), "hidden2_bias": np.asarray(c).tolist(),
                          "output_weights": np.asarray(w3).tolist(), "output_bias": float(b_out)}}


def exact_case(seed, d, h, h2, lens):
    """Integer features in [-8, 8], parameters and lambda in eighths.  First layer (h > 1): unit 0 has z = 0 everywhere, the last
    unit is mostly negative.  Second layer: unit 0 has z = 0 everywhere (h2 > 1), the last is mostly negative, and unit 1
    (h2 > 2, h > 1) is fed only by the dead first-layer unit 0 and stays at its positive bias."""
    rng = np.random.default_rng(seed)
    n = int(sum(lens))
    X = rng.integers(-8, 9, size=(n, d)).astype(np.float32)
    qid = np.repeat(np.arange(1, len(lens) + 1, dtype=np.int64), lens)
    W8, b8 = rng.integers(-4, 5, (h, d)).astype(np.float64), rng.integers(-16, 17, h).astype(np.float64)
    V8, c8, w8 = rng.integers(-4, 5, (h2, h)).astype(np.float64), rng.integers(-16, 17, h2).astype(np.float64), rng.integers(-8, 9, h2).astype(np.float64)
    if h > 1:
        W8[0], b8[0], b8[-1] = 0, 0, -200
    if h2 > 1:
        V8[0], c8[0], c8[-1] = 0, 0, -200
    if h2 > 2 and h > 1:
        V8[1], c8[1] = 0, 5
        V8[1, 0] = 3
    return X, qid, (W8, b8, V8, c8, w8, float(rng.integers(-8, 9))), rng.integers(-16, 17, n).astype(np.float64)


def exact_sums(X, par, lam8, rows):
    """(scores of every row; the six gradient sums over `rows`): integers held in float64, scaled by powers of two at the end.
    Every intermediate is an integer below 2^53 (asserted), so numpy's sums are exact in any order, and so are the kernels'."""
    W8, b8, V8, c8, w8, bo8 = par
    Xi, big = X.astype(np.float64), [0.0]

    def chk(a):
        big[0] = max(big[0], float(np.abs(a).max(initial=0.0)))
        return a

    z8 = chk(b8 + Xi @ W8.T)                    # 8 z1
    a8 = np.maximum(z8, 0)
    z64 = chk(8 * c8 + a8 @ V8.T)               # 64 z2
    a64 = np.maximum(z64, 0)
    scores = chk(64 * bo8 + chk(a64 * w8).sum(1) + 0.0) / 512.0
    lam, a8, a64, Xr = lam8[rows], a8[rows], a64[rows], Xi[rows]
    d64 = (z64[rows] > 0) * (lam[:, None] * w8[None, :])      # 64 d2
    d512 = (z8[rows] > 0) * chk(d64 @ V8)                     # 512 d1
    grads = {"hidden_weights": chk(d512.T @ Xr) / 512.0, "hidden_bias": chk(d512.sum(0)) / 512.0, "hidden2_weights": chk(d64.T @ a8) / 512.0,
             "hidden2_bias": chk(d64.sum(0)) / 64.0, "output_weights": chk(chk(lam[:, None] * a64).sum(0)) / 512.0, "output_bias": lam.sum() / 8.0}
    assert big[0] * max(1, len(rows)) < 2.0 ** 53  # (times the rows: every partial sum of the matrix products too)
    return scores, grads


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64), np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))


def _check(ds, model, lam, exp_scores, exp_grads, score_rows=None, **kw):
    got = native.predict_scores_dense(model, ds, n_total=len(exp_scores))
    rows = np.arange(len(exp_scores)) if score_rows is None else score_rows
    assert _same_bits(got[rows], exp_scores[rows]) and np.isnan(np.delete(got, rows)).all()
    grads = native.mlp2_gradients(ds, model, lam, **kw)
    for key in KEYS:
        assert _same_bits(grads[key] + 0.0, exp_grads[key] + 0.0), key  # (+ 0.0: a sum of products with 0 may be -0)
    assert grads["output_bias"] == exp_grads["output_bias"]
    return grads


def _models(par):
    W8, b8, V8, c8, w8, bo8 = par
    return fr.CModel.from_dict(_net(W8 / 8.0, b8 / 8.0, V8 / 8.0, c8 / 8.0, w8 / 8.0, bo8 / 8.0))


@pytest.mark.parametrize("n", [1, 64, 65])
@pytest.mark.parametrize("h2", [1, 15, 17, 64])
@pytest.mark.parametrize("h", [1, 3, 4, 5, 64, 65, 129])
@pytest.mark.parametrize("d", [17, 145])
def test_every_shape_gives_the_exact_sums(d, h, h2, n):
    X, qid, par, lam8 = exact_case(((d * 1000 + h) * 100 + h2) * 100 + n, d, h, h2, [n])
    scores, grads = exact_sums(X, par, lam8, np.arange(n))
    if h > 1 and h2 > 2:
        assert (grads["hidden_weights"][0] == 0).all() and (grads["hidden2_weights"][0] == 0).all() and (grads["hidden2_weights"][:, 0] == 0).all()
        assert grads["hidden2_bias"][1] == lam8.sum() * par[4][1] / 64.0  # (unit 1 is on for every document)
    plan = {}
    _check(fr.CDataset.from_numpy(X, np.zeros(n), qid), _models(par), lam8 / 8.0, scores, grads, plan=plan)
    assert (plan["feature_panels"], plan["hidden_panels"], plan["hidden2"]) == (1 + (d > 144), -(-h // 64), h2) and plan["workgroups"] == -(-n // 64)


def test_stretches_of_several_tiles_and_a_query_across_a_tile_boundary():
    """Above 620 tiles (the records' cap at four passes) a workgroup's stretch is two tiles: accumulators and running sums stay in
    registers from tile to tile.  The same call twice gives the same bytes."""
    lens = [40, 50] + [704] * 70 + [1]
    X, qid, par, lam8 = exact_case(3, 145, 65, 17, lens)
    ds, model = fr.CDataset.from_numpy(X, np.zeros(len(qid)), qid), _models(par)
    scores, grads = exact_sums(X, par, lam8, np.arange(len(qid)))
    plan = {}
    first = _check(ds, model, lam8 / 8.0, scores, grads, plan=plan)
    assert plan["tiles"] > 768 and plan["stretch_tiles"] >= 2 and plan["workgroups"] == -(-plan["tiles"] // plan["stretch_tiles"])
    again = native.mlp2_gradients(ds, model, lam8 / 8.0)
    assert all(_same_bits(first[k], again[k]) for k in KEYS) and first["output_bias"] == again["output_bias"]
    assert _same_bits(native.predict_scores_dense(model, ds), native.predict_scores_dense(model, ds))


def test_only_visited_queries_are_read():
    """A query-sampled view and a `queries` list: every other lambda is NaN and reaches no sum; a view scores its own documents only."""
    lens = [30, 70, 1, 64, 90, 5, 129]
    X, qid, par, lam8 = exact_case(5, 17, 20, 9, lens)
    ds, model, visit = fr.CDataset.from_numpy(X, np.zeros(len(qid)), qid), _models(par), [1, 3, 6]
    rows = np.flatnonzero(np.isin(qid, [q + 1 for q in visit]))
    lam = np.full(len(qid), np.nan)
    lam[rows] = lam8[rows] / 8.0
    scores, grads = exact_sums(X, par, lam8, rows)
    _check(ds, model, lam, scores, grads, queries=visit)
    _check(ds.subsample_queries([str(q + 1) for q in visit]), model, lam, scores, grads, score_rows=rows)


def test_a_second_layer_that_is_the_identity_gives_the_one_layer_scores():
    """h = h2 = 4 units with a1 >= 0, W2 = I, c = 0: a2 = a1, and on integer data both paths are exact.  The one-layer model goes
    through mlp_score_kernel as before."""
    X, qid, (W8, b8, _, _, _, bo8), _ = exact_case(8, 17, 4, 4, [65])
    w8 = np.array([3.0, -5.0, 8.0, 1.0])
    one = fr.CModel.from_dict({"NeuralNet": {"activation": "relu", "hidden_weights": (W8 / 8.0).tolist(), "hidden_bias": (b8 / 8.0).tolist(),
                                             "output_weights": (w8 / 8.0).tolist(), "output_bias": bo8 / 8.0}})
    assert "hidden2_weights" not in one.to_dict()["NeuralNet"]
    two = fr.CModel.from_dict(_net(W8 / 8.0, b8 / 8.0, np.eye(4), np.zeros(4), w8 / 8.0, bo8 / 8.0))
    ds = fr.CDataset.from_numpy(X, np.zeros(65), qid)
    exact = (8 * bo8 + np.maximum(b8 + X.astype(np.float64) @ W8.T, 0) @ w8) / 64.0
    assert _same_bits(native.predict_scores_dense(one, ds), exact) and _same_bits(native.predict_scores_dense(two, ds), exact)


def continuous_case(d, h, h2, n):
    """Seeded normal data, its exact z1, z2 as Fractions and their error bounds ez1, ez2 (the test's docstring)."""
    rng = np.random.default_rng(100 * d + h2)
    X = rng.normal(0.0, 1.0, (n, d)).astype(np.float32)
    par = [rng.normal(0.0, 0.3, (h, d)), rng.normal(0.0, 0.5, h), rng.normal(0.0, 0.4, (h2, h)), rng.normal(0.0, 0.5, h2), rng.normal(0.0, 1.0, h2),
           float(rng.normal())]
    lam = rng.normal(0.0, 1.0, n)
    F = lambda a: [Fraction(float(v)) for v in a]  # noqa: E731
    x, w1, b1, w2, c = [F(r) for r in X], [F(r) for r in par[0]], F(par[1]), [F(r) for r in par[2]], F(par[3])
    u = Fraction(1, 2 ** 53)
    gamma = lambda k: k * u / (1 - k * u)  # noqa: E731
    dot = lambda a, b: sum(p * q for p, q in zip(a, b))  # noqa: E731
    adot = lambda a, b: sum(abs(p * q) for p, q in zip(a, b))  # noqa: E731
    z1 = [[b1[j] + dot(x[p], w1[j]) for j in range(h)] for p in range(n)]
    ez1 = [[gamma(d + 1) * (abs(b1[j]) + adot(x[p], w1[j])) for j in range(h)] for p in range(n)]
    a1 = [[max(v, 0) for v in row] for row in z1]
    up1 = [[a1[p][j] + ez1[p][j] if a1[p][j] > 0 else 0 for j in range(h)] for p in range(n)]   # the computed a1 is at most this
    in1 = [[ez1[p][j] if a1[p][j] > 0 else 0 for j in range(h)] for p in range(n)]               # ... and this far from a1
    z2 = [[c[k] + dot(a1[p], w2[k]) for k in range(h2)] for p in range(n)]
    ez2 = [[gamma(h + 1) * (abs(c[k]) + adot(up1[p], w2[k])) + adot(in1[p], w2[k]) for k in range(h2)] for p in range(n)]
    return (X, par, lam), (x, w2, F(par[4]), Fraction(par[5]), F(lam)), (z1, ez1, a1, up1, in1, z2, ez2), gamma


@pytest.mark.parametrize("d,h,h2,n", [(17, 17, 17, 70), (136, 64, 32, 20)])
def test_continuous_data_stays_within_the_derived_bounds(d, h, h2, n):
    """u = 2^-53, gamma_k = k u / (1 - k u); a sum of k terms, each carrying at most one rounding of its own, is within gamma_k of
    its exact value times the sum of the terms' magnitudes, in any order.  z1: d + 1 terms, ez1 = gamma_(d+1) (|b1| + sum |x W1|).
    Where |z1| > ez1 (asserted) ReLU reads the exact sign: the computed a1 is within in1 = ez1 of a1 and at most up1 = a1 + ez1
    on active units, exactly 0 on the others.  z2: h + 1 terms over the computed a1, ez2 = gamma_(h+1) (|c| + sum up1 |W2|) + sum in1
    |W2|; |z2| > ez2 (asserted), so a2, up2, in2 likewise.  Score: h2 + 1 terms fl(a2 w3) and b_out.  d2 = fl(lambda w3) carries one
    rounding; G_bout, G_c: n terms; G_w3: n terms fl(lambda a2) over the computed a2; G_W2: n terms of two roundings over the computed
    a1; e = d2 W2: h2 terms of two roundings, ee = gamma_(h2+1) sum |d2 W2|, and d1 = e where z1 > 0; G_b1: n terms within ee each;
    G_W1: n terms of one more rounding.  Nothing here is measured.  The largest error / bound ratios go to profiles/mlp2_error.txt."""
    (X, par, lam), (x, w2, w3, bout, lamf), (z1, ez1, a1, up1, in1, z2, ez2), gamma = continuous_case(d, h, h2, n)
    assert all(abs(z1[p][j]) > ez1[p][j] for p in range(n) for j in range(h)) and all(abs(z2[p][k]) > ez2[p][k] for p in range(n) for k in range(h2))
    ds, model = fr.CDataset.from_numpy(X, np.zeros(n), np.repeat(np.arange(1, 3, dtype=np.int64), [n - n // 2, n // 2])), fr.CModel.from_dict(_net(*par))
    scores, grads = native.predict_scores_dense(model, ds), native.mlp2_gradients(ds, model, lam)
    worst = {key: Fraction(0) for key in ("score",) + KEYS + ("output_bias",)}

    def hold(name, got, exact, bound):
        err = abs(Fraction(float(got)) - exact)
        assert err <= bound, (name, float(err), float(bound))
        if bound > 0:
            worst[name] = max(worst[name], err / bound)

    P, on2 = range(n), [[z2[p][k] > 0 for k in range(h2)] for p in range(n)]
    a2 = [[max(v, 0) for v in row] for row in z2]
    up2 = [[a2[p][k] + ez2[p][k] if on2[p][k] else 0 for k in range(h2)] for p in P]
    in2 = [[ez2[p][k] if on2[p][k] else 0 for k in range(h2)] for p in P]
    d2 = [[lamf[p] * w3[k] if on2[p][k] else 0 for k in range(h2)] for p in P]
    for p in P:
        hold("score", scores[p], bout + sum(a2[p][k] * w3[k] for k in range(h2)),
             gamma(h2 + 1) * (abs(bout) + sum(up2[p][k] * abs(w3[k]) for k in range(h2))) + sum(in2[p][k] * abs(w3[k]) for k in range(h2)))
    hold("output_bias", grads["output_bias"], sum(lamf), gamma(n) * sum(abs(v) for v in lamf))
    for k in range(h2):
        hold("hidden2_bias", grads["hidden2_bias"][k], sum(d2[p][k] for p in P), gamma(n + 1) * sum(abs(d2[p][k]) for p in P))
        hold("output_weights", grads["output_weights"][k], sum(lamf[p] * a2[p][k] for p in P),
             gamma(n + 1) * sum(abs(lamf[p]) * up2[p][k] for p in P) + sum(abs(lamf[p]) * in2[p][k] for p in P))
        for j in range(h):
            hold("hidden2_weights", grads["hidden2_weights"][k, j], sum(d2[p][k] * a1[p][j] for p in P),
                 gamma(n + 2) * sum(abs(d2[p][k]) * up1[p][j] for p in P) + sum(abs(d2[p][k]) * in1[p][j] for p in P))
    for j in range(h):
        on = [p for p in P if z1[p][j] > 0]
        d1 = [sum(d2[p][k] * w2[k][j] for k in range(h2)) for p in on]
        ee = [gamma(h2 + 1) * sum(abs(d2[p][k] * w2[k][j]) for k in range(h2)) for p in on]
        hold("hidden_bias", grads["hidden_bias"][j], sum(d1), gamma(n) * sum(abs(v) + e for v, e in zip(d1, ee)) + sum(ee))
        for i in range(d):
            ax = [abs(x[p][i]) for p in on]
            hold("hidden_weights", grads["hidden_weights"][j, i], sum(v * x[p][i] for v, p in zip(d1, on)),
                 gamma(n + 1) * sum((abs(v) + e) * t for v, e, t in zip(d1, ee, ax)) + sum(e * t for e, t in zip(ee, ax)))
    path = os.path.join(ROOT, "profiles", "mlp2_error.txt")  # (rewritten only when a figure moved: the kernels are deterministic)
    old = open(path).read() if os.path.exists(path) else ""
    line = "d=%d h=%d h2=%d n=%d largest |error| / bound: " % (d, h, h2, n) + ", ".join("%s %.6f" % (k, float(v)) for k, v in worst.items())
    new = "\n".join(sorted([ln for ln in old.splitlines() if not ln.startswith("d=%d " % d)] + [line])) + "\n"
    if new != old:
        with open(path, "w") as fh:
            fh.write(new)


NET = _net([[0.5, -1.0, 0.0], [2.0, 0.25, -0.125]], [0.0, -1.5], [[1.0, 0.5], [0.0, -2.0], [0.25, 0.0]], [0.5, 0.0, -1.0], [1.0, -2.0, 0.5], 0.75)


@pytest.mark.parametrize("change,text", [
    ({"hidden2_weights": [], "hidden2_bias": [], "output_weights": []}, "hidden2_weights must have between 1 and 64 rows"),
    ({"hidden2_weights": [[0.0, 1.0]] * 65, "hidden2_bias": [0.0] * 65, "output_weights": [0.0] * 65}, "hidden2_weights must have between 1 and 64 rows"),
    ({"hidden2_weights": [[1.0, 0.5], [0.0], [0.25, 0.0]]}, "every row of hidden2_weights must hold one number per row of hidden_weights"),
    ({"hidden2_weights": [[1.0, 0.5, 0.0]] * 3}, "every row of hidden2_weights must hold one number per row of hidden_weights"),
    ({"hidden2_bias": [0.5, 0.0]}, "hidden2_bias and output_weights must hold one number per row of hidden2_weights"),
    ({"output_weights": [1.0, -2.0]}, "hidden2_bias and output_weights must hold one number per row of hidden2_weights"),
    ({"hidden_bias": [0.0]}, "hidden_bias must hold one number per row of hidden_weights"),
    ({"hidden2_weights": None}, "hidden2_weights and hidden2_bias must appear together"),
    ({"hidden2_bias": None}, "hidden2_weights and hidden2_bias must appear together"),
    ({"hidden2_bias": [0.5, 1e999, -1.0]}, "number out of range"),  # (the JSON reader's own words: no number it accepts is non-finite)
    ({"hidden2_weights": [[1.0, 0.5], [0.0, -1e999], [0.25, 0.0]]}, "number out of range"),
])
def test_model_refusals(change, text):
    inner = {k: v for k, v in {**NET["NeuralNet"], **change}.items() if v is not None}
    with pytest.raises(Exception, match=text):
        clib._unwrap(clib._load().model_from_json(json.dumps({"NeuralNet": inner}).replace("Infinity", "1e999").encode()))


def test_each_gradient_hook_refuses_the_other_form():
    """output_weights of a two-layer net holds h2 numbers where the one-layer launcher reads h: neither hook takes the other's model."""
    ds = fr.CDataset.from_numpy(np.zeros((2, 3), dtype=np.float32), np.zeros(2), np.ones(2, dtype=np.int64))
    with pytest.raises(Exception, match="the model has hidden2_weights; its gradients come from fr_debug_mlp2_gradients"):
        native.mlp_gradients(ds, fr.CModel.from_dict(NET), np.zeros(2))
    one = {"NeuralNet": {k: v for k, v in NET["NeuralNet"].items() if not k.startswith("hidden2")}}
    one["NeuralNet"]["output_weights"] = [1.0, -2.0]
    with pytest.raises(Exception, match="the model must be a NeuralNet with hidden2_weights"):
        native.mlp2_gradients(ds, fr.CModel.from_dict(one), np.zeros(2))
