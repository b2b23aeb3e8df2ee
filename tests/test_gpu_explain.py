"""Model explanation on the device: the bytes of fr_explain_dense against the numpy restatement
(tests/explain_model.py) on the designed models of the host test, odd row counts, a sampled view, a separate background, a
path at the kernel's limit and trained models; local accuracy, unused features, the reduced feature importance, refusals."""
import math
import os

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import native
from tests import explain_model as em
from tests.conftest import GOLDEN, synth_dataset
from tests.test_explain_host import BOUND

pytestmark = pytest.mark.gpu

MAX_ROWS = 192  # rows of a larger dataset the restatement is run on (every row's covers still come from all rows)


def _dataset(X, queries=4):
    n = len(X)
    qid = (np.arange(n, dtype=np.int64) * queries // n) + 1
    y = (np.arange(n) % 3).astype(np.float64)
    return fr.CDataset.from_numpy(np.ascontiguousarray(X, dtype=np.float32), y, qid)


def _model(trees, weights, single=False):
    if single:
        return fr.CModel.from_dict({"DecisionTree": trees[0]})
    return fr.CModel.from_dict({"Ensemble": {"weights": [float(w) for w in weights], "models": [{"DecisionTree": t} for t in trees]}})


def _trees_of(model):
    wire = model.to_dict()
    if "DecisionTree" in wire:
        return [wire["DecisionTree"]], [1.0], True
    ens = wire["Ensemble"]
    return [m["DecisionTree"] for m in ens["models"]], ens["weights"], False


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check(model, ds, X, rows=None, bg=None, XB=None, ids=None):
    """Device bytes = restatement's on `rows` (indices into X; None: all), unused columns exactly 0.0, local accuracy on every
    row.  ids: the instance ids X's rows have in `ds` (None: 0..n-1)."""
    trees, weights, single = _trees_of(model)
    ex = model.explain(ds, bg)
    ids = np.arange(len(X)) if ids is None else np.asarray(ids)
    rows = np.arange(len(X)) if rows is None else np.asarray(rows)
    tab = em.path_table(trees, weights, em.leaf_counts(trees, X if XB is None else XB), X.shape[1])
    want = em.restate(tab, X[rows])
    got = ex.values[ids[rows]]
    feats = tab["features"]
    held = [f for f in feats if f < X.shape[1]]
    assert list(ex.feature_ids) == list(range(X.shape[1])) and len(ex.feature_names) == X.shape[1]
    for f in held:
        assert np.array_equal(_bits(got[:, f]), _bits(want[:, feats.index(f)])), "feature %d" % f
    for f in feats:  # a feature the dataset does not hold has no column, and the restatement says exactly 0.0
        if f >= X.shape[1]:
            assert np.all(want[:, feats.index(f)] == 0.0)
    unused = [f for f in range(X.shape[1]) if f not in held]
    assert np.all(ex.values[ids][:, unused] == 0.0) and not np.any(np.signbit(ex.values[ids][:, unused]))
    assert _bits(ex.expected_value) == _bits(tab["bias"])
    assert ex.status["leaf_paths"] == len(tab["m"]) and ex.status["max_path"] == tab["max_path"]
    print("%d trees, %d leaf paths, longest %d elements" % (len(trees), len(tab["m"]), tab["max_path"]))
    # local accuracy, with the row summed exactly (math.fsum): what is left is the contributions' own error and the score's
    scores = native.predict_scores_dense(model, ds)[ids]
    sc = em.scale(trees, weights)
    worst = max(abs(math.fsum(list(ex.values[i]) + [ex.expected_value]) - s) for i, s in zip(ids, scores))
    print("local accuracy: worst |sum phi + bias - f(x)| = %.3e = %.3e x scale (bound %.3e)" % (worst, worst / sc if sc else 0.0, BOUND))
    assert worst <= BOUND * sc
    return ex


@pytest.mark.parametrize("name", [c[0] for c in em.designed_cases()])
def test_designed(name):
    _, trees, weights, X, XB, single = next(c for c in em.designed_cases() if c[0] == name)
    bg = None if XB is None else _dataset(XB)
    _check(_model(trees, weights, single), _dataset(X), X, bg=bg, XB=XB)


@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_row_counts(n):
    trees, weights, _ = em.random_forest_model(21, d=6, trees=4, depth=5, n=16)
    X = np.random.default_rng(n).normal(0, 1, (n, 6)).astype(np.float32)
    X[:, 1] = np.floor(np.abs(X[:, 1]) * 2)
    _check(_model(trees, weights), _dataset(X, queries=min(n, 5)), X)


def test_sampled_view():
    trees, weights, _ = em.random_forest_model(22, d=5, trees=5, depth=5, n=16)
    X = np.random.default_rng(5).normal(0, 1, (300, 5)).astype(np.float32)
    ds = _dataset(X, queries=10)
    keep = ["2", "3", "7", "10"]
    view = ds.subsample_queries(keep)
    ids = np.array(sorted(i for q in keep for i in view.instances_by_query()[q]))
    model = _model(trees, weights)
    ex = _check(model, view, X[ids], ids=ids)  # the covers come from the view: X[ids] is explained set and background
    outside = np.setdiff1d(np.arange(ex.values.shape[0]), ids)
    assert len(outside) and np.all(np.isnan(ex.values[outside]))
    # ... and explaining the view against the whole dataset is something else: the parent's covers
    _check(model, view, X[ids], bg=ds, XB=X, ids=ids)


def test_separate_background():
    trees, weights, X = em.random_forest_model(23, d=6, trees=3, depth=6, n=90)
    XB = np.random.default_rng(9).normal(0.5, 2, (130, 6)).astype(np.float32)
    _check(_model(trees, weights), _dataset(X), X, bg=_dataset(XB), XB=XB)


def _chain(n_feats):
    node = em.L(1.0)
    for f in reversed(range(n_feats)):
        node = em.S(f, 0.0, em.L(float(-f) * 0.5), node)
    return node


def test_path_limit():
    X = np.random.default_rng(3).normal(0.6, 1, (70, 40)).astype(np.float32)
    ds = _dataset(X)
    ex = _check(_model([_chain(32), em.S(39, 0.0, em.L(1.0), em.L(2.0))], [1.0, -0.5]), ds, X)
    assert ex.status["max_path"] == 32
    with pytest.raises(Exception, match="more than 32 distinct features"):
        _model([_chain(33)], [1.0], single=True).explain(ds)


def test_register_and_lds_paths():
    # paths of up to 8 elements keep their permutation weights in registers, longer ones in LDS: both sides of the threshold
    # in one model, and a model that stays below it (no LDS rows for the weights at all)
    X = np.random.default_rng(8).normal(0.4, 1, (130, 16)).astype(np.float32)
    ds = _dataset(X)
    ex = _check(_model([_chain(8), _chain(9), _chain(12), _chain(3)], [1.0, -0.75, 0.5, 2.0]), ds, X)
    assert ex.status["max_path"] == 12
    ex = _check(_model([_chain(8), _chain(7)], [1.0, 0.3]), ds, X)
    assert ex.status["max_path"] == 8


# --- trained models ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def trec():
    d = np.load(os.path.join(GOLDEN, "trec_news_2018.npz"))
    X, y, qid = d["train_X"], d["train_y"], d["train_qid"]
    return X, fr.CDataset.from_numpy(X, y, qid)


@pytest.fixture(scope="module")
def synth():
    X, y, qid = synth_dataset(7, 5000, 10, 50)
    return X, fr.CDataset.from_numpy(X, y, qid)


def _lambdamart(ds, **kw):
    req = fr.TrainRequest.lambdamart()
    req.measure = "ndcg@10"
    req.params.quiet, req.params.grower, req.params.num_trees = True, "histogram", 10
    for k, v in kw.items():
        setattr(req.params, k, v)
    return ds.train_model(req)


def _some_rows(n):
    return np.unique(np.linspace(0, n - 1, MAX_ROWS).astype(np.int64))


@pytest.mark.parametrize("how", ["depth6", "max_leaves", "dart"])
def test_trained_lambdamart(trec, how):
    X, ds = trec
    kw = {"depth6": dict(max_depth=6), "max_leaves": dict(max_depth=12, max_leaves=24),
          "dart": dict(max_depth=4, drop_rate=0.5, skip_drop=0.0, seed=3)}[how]
    model = _lambdamart(ds, **kw)
    trees, weights, _ = _trees_of(model)
    assert len(trees) == 10
    if how == "dart":
        assert len(set(weights)) > 1
    _check(model, ds, X, rows=_some_rows(len(X)))


def test_trained_random_forest(synth):
    X, ds = synth
    req = fr.TrainRequest.random_forest()
    req.measure = "ndcg@10"
    req.params.quiet, req.params.num_trees, req.params.max_depth, req.params.seed = True, 10, 8, 5
    model = ds.train_model(req)
    _check(model, ds, X, rows=_some_rows(len(X)))


def test_seventy_trees(synth):
    X, ds = synth
    rng = np.random.default_rng(70)
    trees = []
    for t in range(70):
        tt, _, _ = em.random_forest_model(100 + t, d=10, trees=1, depth=3, n=16)
        trees.append(tt[0])
    _check(_model(trees, rng.uniform(-1, 1, 70)), ds, X, rows=_some_rows(len(X))[::2])


# --- feature importance ----------------------------------------------------------------------------------------------------

def test_feature_importance():
    X, y, qid = synth_dataset(11, 20000, 16, 150)
    ds = fr.CDataset.from_numpy(X, y, qid)
    trees, weights, _ = em.random_forest_model(31, d=14, trees=6, depth=5, n=16)  # features 14 and 15 are never split on
    model = _model(trees, weights)
    ids, a, rep = native.feature_importance(model, ds)
    _, b, _ = native.feature_importance(model, ds)
    assert np.array_equal(_bits(a), _bits(b))  # a fixed reduction shape: the same bytes every run
    ex = model.explain(ds)
    ref = np.abs(ex.values).mean(0)
    n = len(X)
    gamma = n * 2.0 ** -53 / (1 - n * 2.0 ** -53)
    print("importance: worst |device - numpy| / mean = %.3e (gamma_n %.3e)" % (np.max(np.abs(a - ref) / np.maximum(ref, 1e-300)), gamma))
    assert np.all(np.abs(a - ref) <= gamma * ref)
    split_on = em.model_features(trees)
    assert a[14] == 0.0 and a[15] == 0.0 and all(a[f] == 0.0 for f in range(16) if f not in split_on) and np.count_nonzero(a) >= 8
    counts = em.split_counts(trees)
    assert [int(c) for c in rep["split_counts"]] == [counts.get(f, 0) for f in range(16)]
    assert rep["documents"] == n and rep["leaf_paths"] == sum(len(em.leaves_of(t)) for t in trees)
    named = model.feature_importance(ds)
    assert named == {ds.feature_index_to_name()[int(f)]: float(v) for f, v in zip(ids, a)}


def test_feature_importance_chunks():
    # more than one launch of 1024 tiles: 70 000 documents; the running sum carries across the launches
    rng = np.random.default_rng(4)
    X = rng.normal(0, 1, (70000, 3)).astype(np.float32)
    ds = _dataset(X, queries=700)
    model = _model([em.S(0, 0.0, em.S(1, 0.5, em.L(1.0), em.L(-2.0)), em.L(3.0))], [1.0], single=True)
    _, a, rep = native.feature_importance(model, ds)
    ref = np.abs(model.explain(ds).values).mean(0)
    n = len(X)
    gamma = n * 2.0 ** -53 / (1 - n * 2.0 ** -53)
    assert np.all(np.abs(a - ref) <= gamma * ref) and a[2] == 0.0 and a[0] > 0.0


# --- refusals --------------------------------------------------------------------------------------------------------------

def test_refusals(monkeypatch):
    X = np.random.default_rng(1).normal(0, 1, (200, 4)).astype(np.float32)
    ds = _dataset(X)
    tree = em.S(0, 0.0, em.L(1.0), em.S(1, 0.0, em.L(2.0), em.L(3.0)))
    model = _model([tree], [1.0], single=True)
    for wire, what in [({"Linear": {"weights": [1.0, 2.0, 0.0, 0.0]}}, "Linear model"), ({"SingleFeature": {"fid": 0, "dir": 1.0}}, "SingleFeature model"),
                       ({"Ensemble": {"weights": [1.0], "models": [{"Ensemble": {"weights": [1.0], "models": [{"DecisionTree": tree}]}}]}}, "nested ensembles")]:
        with pytest.raises(Exception, match=what):
            fr.CModel.from_dict(wire).explain(ds)
    # an output that does not fit: 200 documents x 2 features x 8 bytes in whole tiles = 4096 bytes
    monkeypatch.setenv("FR_EXPLAIN_MAX_BYTES", "4095")
    with pytest.raises(Exception, match="need 4096 bytes on the device"):
        model.explain(ds)
    native.feature_importance(model, ds)  # (reduced tile by tile: not bound by the matrix)
    monkeypatch.setenv("FR_EXPLAIN_MAX_BYTES", "4096")
    model.explain(ds)
    monkeypatch.delenv("FR_EXPLAIN_MAX_BYTES")
    with pytest.raises(Exception, match="background dataset holds no instance"):
        model.explain(ds, ds.subsample_queries([]))
    # a feature sample that hides a feature the model splits on has no column for its contribution
    hidden = ds.subsample_feature_names([n for n in ds.feature_names() if ds.feature_name_to_index()[n] != 1])
    with pytest.raises(Exception, match="this feature sample does not list"):
        model.explain(hidden)
    ok = ds.subsample_feature_names([n for n in ds.feature_names() if ds.feature_name_to_index()[n] != 3])
    ex = model.explain(ok)
    assert list(ex.feature_ids) == [0, 1, 2] and np.array_equal(_bits(ex.values), _bits(model.explain(ds).values[:, :3]))


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
def test_a_dataset_with_inf_or_nan_is_refused_and_its_finite_copy_explains_as_before(bad):
    """One non-finite value anywhere -- also in a column the model does not read, also as the background -- and the dataset
    is refused; the same rows with that value replaced explain to the restatement's bytes, before and after the refusal."""
    trees, weights, _ = em.random_forest_model(24, d=5, trees=3, depth=4, n=16)
    X = np.random.default_rng(6).normal(0, 1, (130, 5)).astype(np.float32)
    model = _model(trees, weights)
    fine = _dataset(X)
    before = _check(model, fine, X)
    for col in range(5):
        Xb = X.copy()
        Xb[77, col] = bad
        ds = _dataset(Xb)
        with pytest.raises(Exception, match="holds inf or NaN"):
            model.explain(ds)
        with pytest.raises(Exception, match="holds inf or NaN"):
            model.explain(fine, ds)
    after = model.explain(fine)
    assert np.array_equal(_bits(after.values), _bits(before.values)) and _bits(after.expected_value) == _bits(before.expected_value)
