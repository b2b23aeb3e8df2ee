"""Model explanation without a device: the numpy restatement of the algorithm
(tests/explain_model.py) against the definition in exact rationals, on designed and seeded random small models; the path
table the library builds against the restatement's; the models of the device's limit tests shown to sit at their limits;
wire and argument errors."""
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


# --- the models of the device's limit tests sit where they claim (tests/test_gpu_explain.py relies on every line) ---------

def test_limit_constants_are_the_sources():
    """tests/explain_model.py's copies of the kernels' limits are what csrc/explain.hpp and explain.hip say"""
    import os
    import re

    csrc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "fastrank_amd", "csrc")
    text = open(os.path.join(csrc, "explain.hpp")).read() + open(os.path.join(csrc, "explain.hip")).read()

    def const(name):
        expr = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([0-9u* ]+);" % name, text).group(1)
        out = 1
        for factor in expr.replace("u", "").split("*"):
            out *= int(factor)
        return out

    for name in ("EX_LDS_MAX", "EX_REG_PATH", "EX_CHUNK_TILES", "EX_COVER_LDS", "EX_COVER_GRID"):
        print("%s = %d" % (name, const(name)))
        assert const(name) == getattr(em, name), name
    assert const("EX_MAX_PATH") == em.MAX_PATH
    assert re.search(r"t0 \+= %d\)" % em.EX_COVER_TREES, text) and em.EX_COVER_TREES == 65535  # (gridDim.y's limit)
    assert em.EX_LDS_MAX == 159744 and em.EX_LDS_MAX > 48 * 1024


def test_cover_limit_models():
    X, XB, models = em.cover_limit_case()
    assert X.shape == (70, 4) and len(XB) == 70000 and len(XB) > em.EX_COVER_GRID * 256  # the stride loop runs
    want = {"leaves_4096": [4096], "leaves_4097": [4097], "mixed": [2, 4097, 32, 4097]}
    for name, (trees, weights, single) in models.items():
        leaves = [len(em.leaves_of(t)) for t in trees]
        counts = em.leaf_counts(trees, XB)
        tab = em.path_table(trees, weights, counts, 4)
        zero, reached = sum(c == 0 for c in counts), sum(c > 0 for c in counts)
        print("%s: leaves %s, max_tree_feats %d, max_path %d, LDS %d bytes; %d leaves without a background document, %d with, at most %d"
              % (name, leaves, tab["max_tree_feats"], tab["max_path"], em.lds_bytes(tab["max_path"], tab["max_tree_feats"]), zero, reached, max(counts)))
        assert leaves == want[name] and sum(counts) == len(XB) * len(trees)
        assert tab["max_tree_feats"] == 4 and tab["max_path"] == 4
        assert zero >= 500 and reached >= 1000  # many leaves of either kind: a lost or doubled count changes a ratio
    assert em.EX_COVER_LDS == 4096  # 4096 leaves are counted in LDS, 4097 in the global counters
    # the two large trees of the mixed model differ (other features per level, other thresholds); LDS and global alternate
    mixed = models["mixed"][0]
    assert [len(em.leaves_of(t)) > em.EX_COVER_LDS for t in mixed] == [False, True, False, True] and mixed[1] != mixed[3]
    # every document the device explains reaches a leaf some background document reaches, or not: both happen
    counts = em.leaf_counts(models["leaves_4097"][0], XB)
    at = em.route(models["leaves_4097"][0][0], X)
    print("explained rows at leaves with covers", sorted(counts[i] for i in at)[:5], "...")


WIDE_EXPECTED = {  # name: (max_tree_feats, max_path, LDS bytes)
    "wide_63": (63, 8, 48384), "wide_64": (64, 8, 49152), "wide_65": (65, 8, 49920), "wide_136": (136, 8, 104448),
    "wide_208": (208, 8, 159744), "wide_209": (209, 8, 160512), "wide_136_chain_9": (136, 9, 10 * 512 + 104448),
    "long_186": (186, 32, 159744), "long_187": (187, 32, 160512),
}


@pytest.mark.parametrize("name", em.WIDE_FITS + em.WIDE_REFUSED)
def test_wide_models(name):
    trees, weights, single = em.wide_case(name)
    leaves = sum(len(em.leaves_of(t)) for t in trees)
    counts = em.leaf_counts(trees, em.wide_data())
    tab = em.path_table(trees, weights, counts, em.WIDE_COLS)
    lds = em.lds_bytes(tab["max_path"], tab["max_tree_feats"])
    print("%s: %d leaves, max_tree_feats %d, max_path %d, LDS %d bytes (48 KiB = %d, limit %d)"
          % (name, leaves, tab["max_tree_feats"], tab["max_path"], lds, 48 * 1024, em.EX_LDS_MAX))
    assert (tab["max_tree_feats"], tab["max_path"], lds) == WIDE_EXPECTED[name]
    assert len(em.model_features(trees)) == WIDE_EXPECTED[name][0] and max(em.model_features(trees)) < em.WIDE_COLS
    assert (lds <= em.EX_LDS_MAX) == (name in em.WIDE_FITS)
    rep = native.explain_table(_model(trees, weights, single), counts, em.WIDE_COLS)
    assert rep["lds_bytes"] == lds
    _same_table(rep, tab)


def test_wide_models_straddle_the_lines():
    """64 features are the last that need no attribute (not above 48 KiB), 208 and 186 fill the limit to the byte"""
    lds = {name: v[2] for name, v in WIDE_EXPECTED.items()}
    assert lds["wide_63"] < lds["wide_64"] == 48 * 1024 < lds["wide_65"]
    assert lds["wide_208"] == lds["long_186"] == em.EX_LDS_MAX and lds["wide_209"] > em.EX_LDS_MAX and lds["long_187"] > em.EX_LDS_MAX
    # the long tree holds chain(32) whole: its last 32 leaves are the chain's, with 1, 2, .. 32, 32 elements
    trees, weights, _ = em.wide_case("long_186")
    tab = em.path_table(trees, weights, [1] * 288, em.WIDE_COLS)
    assert tab["m"][256:] == list(range(2, 33)) + [32] and max(tab["m"][:256]) == 9


def test_stumps_restatement():
    """The vectorised restatement of one-element paths equals path_table + restate, bit for bit, on the first 200 trees
    (and on 200 others), covers and bias included."""
    trees, weights, X = em.stumps_case()
    assert len(trees) == em.STUMP_TREES == 65539 and len(trees) > em.EX_COVER_TREES
    bare = sum(em.is_leaf(t) for t in trees)
    w = np.asarray(weights)
    print("%d trees, %d bare leaves, weights: %d negative, %d zero, %d positive" % (len(trees), bare, (w < 0).sum(), (w == 0).sum(), (w > 0).sum()))
    assert bare > 100 and (w < 0).sum() > 1000 and (w == 0).sum() > 1000 and (w > 0).sum() > 1000
    # the last trees of the cover pass's first launch and the first of its second read their covers: a split with documents
    # on both sides and a weight (a bare leaf's cover is never read, a zero weight hides the tree)
    for t in range(em.EX_COVER_TREES - 2, em.EX_COVER_TREES + 3):
        assert not em.is_leaf(trees[t]) and weights[t] != 0.0 and min(em.leaf_counts([trees[t]], X)) > 0, t
    for lo in (0, 65400):
        tt, ww = trees[lo:lo + 200], weights[lo:lo + 200]
        assert any(em.is_leaf(t) for t in tt) and any(v == 0.0 for v in ww)
        counts = em.leaf_counts(tt, X)
        tab = em.path_table(tt, ww, counts, 2)
        assert tab["max_path"] == 1 and tab["max_tree_feats"] == 1 and tab["features"] == [0, 1]
        want = em.restate(tab, X[:64])
        phi, feats, bias, cnt = em.restate_stumps(tt, ww, X[:64], X)
        assert feats == tab["features"] and cnt == counts
        assert np.array_equal(phi.view(np.uint64), want.view(np.uint64))
        assert np.float64(bias).view(np.uint64) == np.float64(tab["bias"]).view(np.uint64)
        assert np.array_equal(em.predict_stumps(tt, ww, X[:64]).view(np.uint64), em.predict(tt, ww, X[:64]).view(np.uint64))
    print("max_tree_feats 1, max_path 1, LDS %d bytes" % em.lds_bytes(1, 1))


def test_importance_restatement_is_sequential():
    """importance_restate against the same sums written as plain loops, on a row count with a partial last tile"""
    rng = np.random.default_rng(6)
    for n in (64, 130, 191):
        v = rng.normal(0, 1, (n, 3)) * 10.0 ** rng.integers(-8, 8, (n, 3))
        total = [0.0, 0.0, 0.0]
        for t0 in range(0, n, 64):
            for c in range(3):
                s = 0.0
                for i in range(t0, min(t0 + 64, n)):
                    s = s + abs(float(v[i, c]))
                total[c] = total[c] + s
        want = np.array([t / n for t in total])
        assert np.array_equal(em.importance_restate(v).view(np.uint64), want.view(np.uint64))


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
