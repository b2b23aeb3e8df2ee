"""Model explanation without a device: the numpy restatement of the algorithm
(tests/explain_model.py) against the definition in exact rationals, on designed and seeded random small models; the path
table the library builds against the restatement's; wire and argument errors."""
from fractions import Fraction

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import native
from tests import explain_model as em

# The one tolerance of the feature, relative to sum_t |w_t| * max |leaf_t|: 8 x the largest error of the restatement against
# the exact values over the cases of this file (measured 9.47e-17, test_measured_error prints it).
MEASURED = 9.47e-17
BOUND = 8 * MEASURED

RANDOM_SEEDS = [(11, 6, 3, 6, 12), (12, 5, 4, 4, 16), (13, 8, 2, 6, 10), (14, 3, 6, 5, 20), (15, 7, 3, 6, 12)]  # seed, d, trees, depth, n


def _cases():
    out = [(name, trees, weights, X, XB) for name, trees, weights, X, XB, _ in em.designed_cases()]
    for seed, d, trees, depth, n in RANDOM_SEEDS:
        t, w, X = em.random_forest_model(seed, d=d, trees=trees, depth=depth, n=n)
        out.append(("random_%d" % seed, t, w, X, None))
    return out


CASES = _cases()
_CACHE = {}


def _solved(name):
    """(restated phi, exact phi, features, restated bias, exact bias), computed once per case"""
    if name not in _CACHE:
        _, trees, weights, X, XB = next(c for c in CASES if c[0] == name)
        phi, feats, bias = em.explain(trees, weights, X, XB)
        ephi, efeats, ebias = em.brute(trees, weights, X, XB, exact=True)
        assert feats == efeats and len(feats) <= 8 and len(X) <= 40
        _CACHE[name] = (phi, ephi, feats, bias, ebias)
    return _CACHE[name]


def _rel_error(name):
    _, trees, weights, X, XB = next(c for c in CASES if c[0] == name)
    phi, ephi, feats, bias, ebias = _solved(name)
    sc = em.scale(trees, weights)
    worst = abs(Fraction(float(bias)) - ebias)
    for i in range(len(X)):
        for c in range(len(feats)):
            assert np.isfinite(phi[i, c])
            worst = max(worst, abs(Fraction(float(phi[i, c])) - ephi[i][c]))
    return float(worst / Fraction(sc))


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_restatement_against_exact(name):
    err = _rel_error(name)
    print("%s: relative error %.3e (bound %.3e)" % (name, err, BOUND))
    assert err <= BOUND


def test_measured_error():
    worst = max(_rel_error(c[0]) for c in CASES)
    print("largest relative error of the restatement: %.3e" % worst)
    assert worst <= MEASURED * 1.0000001  # the constant above is the measurement, not a guess
    # the division-free form was chosen so that zero covers and tiny ratios cost nothing: far below the 1e-9 of the issue
    assert _rel_error("zero_cover_background") < 1e-9 and _rel_error("tiny_ratio") < 1e-9


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_efficiency_exact(name):
    """sum_f phi_f + bias = f(x), exactly, in rationals"""
    _, trees, weights, X, XB = next(c for c in CASES if c[0] == name)
    _, ephi, feats, _, ebias = _solved(name)
    fx = em.exact_predict(trees, weights, X)
    for i in range(len(X)):
        assert sum(ephi[i], Fraction(0)) + ebias == fx[i]


def test_float_definition_agrees():
    for name in ("repeated_feature", "zero_cover_background", "random_12"):
        _, trees, weights, X, XB = next(c for c in CASES if c[0] == name)
        fphi, _, fbias = em.brute(trees, weights, X, XB, exact=False)
        _, ephi, _, _, ebias = _solved(name)
        sc = em.scale(trees, weights)
        assert abs(fbias - float(ebias)) <= 1e-12 * sc
        assert max(abs(fphi[i][c] - float(ephi[i][c])) for i in range(len(X)) for c in range(len(ephi[0]))) <= 1e-12 * sc


def test_null_features():
    # a feature the dataset does not hold: exactly 0.0 (o = z = 1 on every path that uses it)
    _, trees, weights, X, XB = next(c for c in CASES if c[0] == "feature_beyond")
    phi, ephi, feats, _, _ = _solved("feature_beyond")
    col = feats.index(9)
    assert np.all(phi[:, col] == 0.0) and not np.any(np.signbit(phi[:, col]))
    assert all(row[col] == 0 for row in ephi)
    # zero-cover branches an explained document walks through: finite, and the row still sums to the score
    phi, _, _, bias, _ = _solved("zero_cover_background")
    _, trees, weights, X, XB = next(c for c in CASES if c[0] == "zero_cover_background")
    assert np.all(np.isfinite(phi))
    assert np.max(np.abs(phi.sum(1) + bias - em.predict(trees, weights, X))) <= BOUND * em.scale(trees, weights) * (len(phi[0]) + 1)


# --- the library's path table ------------------------------------------------------------------------------------------

def _model(trees, weights, single=False):
    if single:
        return fr.CModel.from_dict({"DecisionTree": trees[0]})
    return fr.CModel.from_dict({"Ensemble": {"weights": [float(w) for w in weights], "models": [{"DecisionTree": t} for t in trees]}})


def _same_table(rep, tab):
    for key in ("leaf0", "feat0", "m", "eoff", "slot", "fid", "col", "features"):
        assert [int(v) for v in rep[key]] == [int(v) for v in tab[key]], key
    for key in ("weight", "value", "lo", "hi", "z"):
        assert np.array_equal(np.asarray(rep[key]).view(np.uint64), np.asarray(tab[key], dtype=np.float64).view(np.uint64)), key
    assert np.float64(rep["bias"][0]).view(np.uint64) == np.float64(tab["bias"]).view(np.uint64)
    assert rep["max_path"] == tab["max_path"] and rep["max_tree_feats"] == tab["max_tree_feats"]


def test_path_table_hand_written():
    # x0 <= 0.5 ? (x0 <= -0.25 ? 1 : (x2 <= 0 ? 2 : -3)) : (x0 <= 1 ? (x1 <= 1 ? 4 : 0.5) : 7), leaf counts 3 2 1 4 0 6
    tree = em.designed_cases()[2][1][0]
    counts = [3, 2, 1, 4, 0, 6]
    rep = native.explain_table(_model([tree], [1.0], single=True), counts, 4)
    assert rep["m"] == [1, 2, 2, 2, 2, 1] and rep["features"] == [0, 1, 2] and rep["fid"] == [0, 2, 1] and rep["col"] == [0, 2, 1]
    inf = np.inf
    # leaf 0: x0 to the left twice -> one element, hi = the smaller split, z = (6/16) * (3/6)
    assert (rep["lo"][0], rep["hi"][0]) == (-inf, -0.25) and rep["z"][0] == (6 / 16) * (3 / 6)
    # leaf 1: x0 left then right -> the interval (-0.25, 0.5], then x2
    assert (rep["lo"][1], rep["hi"][1], rep["slot"][1], rep["slot"][2]) == (-0.25, 0.5, 0, 1)
    assert rep["z"][1] == (6 / 16) * (3 / 6) and rep["z"][2] == 2 / 3
    # leaf 4 has no background document, leaf 5: x0 right twice -> lo = the larger split
    assert rep["z"][8] == 0.0 and (rep["lo"][9], rep["hi"][9]) == (1.0, inf) and rep["z"][9] == (10 / 16) * (6 / 10)
    _same_table(rep, em.path_table([tree], [1.0], counts, 4))


@pytest.mark.parametrize("name", [c[0] for c in em.designed_cases()])
def test_path_table_designed(name):
    _, trees, weights, X, XB, single = next(c for c in em.designed_cases() if c[0] == name)
    counts = em.leaf_counts(trees, X if XB is None else XB)
    _same_table(native.explain_table(_model(trees, weights, single), counts, X.shape[1]), em.path_table(trees, weights, counts, X.shape[1]))


def test_path_table_zero_cover_parent():
    # no background document at all under a split: both ratios are 0.0, nothing is NaN
    tree = em.S(0, 0.0, em.L(1.0), em.S(1, 0.0, em.L(2.0), em.L(3.0)))
    rep = native.explain_table(_model([tree], [1.0], single=True), [5, 0, 0], 2)
    assert list(rep["z"]) == [1.0, 0.0, 0.0, 0.0, 0.0] and rep["bias"][0] == 1.0
    _same_table(rep, em.path_table([tree], [1.0], [5, 0, 0], 2))


def _chain(n_feats):
    node = em.L(1.0)
    for f in reversed(range(n_feats)):
        node = em.S(f, 0.0, em.L(float(-f)), node)
    return node


def test_path_limit():
    rep = native.explain_table(_model([_chain(32)], [1.0], single=True), [1] * 33, 40)
    assert rep["max_path"] == 32 and rep["lds_bytes"] == 33 * 512 + 32 * 768
    with pytest.raises(Exception, match="more than 32 distinct features"):
        native.explain_table(_model([_chain(33)], [1.0], single=True), [1] * 34, 40)


# --- errors that need no device ------------------------------------------------------------------------------------------

def _tiny_dataset():
    X = np.arange(12, dtype=np.float32).reshape(6, 2)
    return fr.CDataset.from_numpy(X, np.zeros(6), np.array([1, 1, 1, 2, 2, 2], dtype=np.int64))


@pytest.mark.parametrize("model,what", [
    ({"Linear": {"weights": [1.0, 2.0]}}, "Linear model"),
    ({"SingleFeature": {"fid": 0, "dir": 1.0}}, "SingleFeature model"),
    ({"Ensemble": {"weights": [1.0], "models": [{"Ensemble": {"weights": [1.0], "models": [{"DecisionTree": {"LeafNode": 1.0}}]}}]}}, "nested ensembles"),
    ({"Ensemble": {"weights": [1.0, 1.0], "models": [{"DecisionTree": {"LeafNode": 1.0}}, {"Linear": {"weights": [1.0]}}]}}, "must be a DecisionTree"),
])
def test_refused_models(model, what):
    m, ds = fr.CModel.from_dict(model), _tiny_dataset()
    with pytest.raises(Exception, match=what):
        m.explain(ds)
    with pytest.raises(Exception, match=what):
        m.feature_importance(ds)
    with pytest.raises(Exception, match=what):
        native.explain_table(m, [1], 2)


def test_empty_background_refused():
    ds = _tiny_dataset()
    m = _model([em.S(0, 0.0, em.L(1.0), em.L(2.0))], [1.0], single=True)
    with pytest.raises(Exception, match="background dataset holds no instance"):
        m.explain(ds, ds.subsample_queries([]))
    with pytest.raises(Exception, match="background dataset holds no instance"):
        m.feature_importance(ds, ds.subsample_queries([]))


def test_argument_errors():
    m = _model([em.S(0, 0.0, em.L(1.0), em.L(2.0))], [1.0], single=True)
    with pytest.raises(Exception, match="the model has 2 leaves"):
        native.explain_table(m, [1, 2, 3], 2)
    lib = native._load()
    for call in (lambda: lib.fr_explain_dense(None, None, None, None, 0, 0), lambda: lib.fr_feature_importance(m.pointer, None, None, None, 0)):
        with pytest.raises(Exception, match="pointer is null"):
            native._json_reply(call())


def test_host_headers_under_address_and_undefined_sanitizers(tmp_path):
    """tests/explain_host_sanitize.cpp: a program of its own over csrc/explain_host.hpp (a chain at the path limit and one
    past it, a repeated feature, empty branches), built with -fsanitize=address,undefined and run directly."""
    import os
    import shutil
    import subprocess

    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "explain_host_sanitize")
    build = subprocess.run([cxx, "-std=c++17", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                            "-I", os.path.join(here, "..", "fastrank_amd", "csrc"), os.path.join(here, "explain_host_sanitize.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "explain_host ok" in run.stdout, run.stdout
