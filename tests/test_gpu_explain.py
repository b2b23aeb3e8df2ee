"""Model explanation on the device: the bytes of fr_explain_dense against the numpy restatement
(tests/explain_model.py) on the designed models of the host test, odd row counts, a sampled view, a separate background, a
path at the kernel's limit and trained models; local accuracy, unused features, the reduced feature importance, refusals;
and every limit of the three kernels from both sides: the cover pass's LDS table, grid and tree count, the contribution
kernel's LDS size, the importance reduction's chunk boundary."""
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


def _check(model, ds, X, rows=None, bg=None, XB=None, ids=None, counts=None, local=True):
    """Device bytes = restatement's on `rows` (indices into X; None: all), unused columns exactly 0.0, local accuracy on every
    row.  ids: the instance ids X's rows have in `ds` (None: 0..n-1).  counts: em.leaf_counts of the background, where the
    caller has them.  local=False: the local-accuracy ratio is printed, not held to BOUND (a model far larger than those
    BOUND was measured on: the limit tests say which)."""
    trees, weights, single = _trees_of(model)
    ex = model.explain(ds, bg)
    ids = np.arange(len(X)) if ids is None else np.asarray(ids)
    rows = np.arange(len(X)) if rows is None else np.asarray(rows)
    tab = em.path_table(trees, weights, em.leaf_counts(trees, X if XB is None else XB) if counts is None else counts, X.shape[1])
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
    assert not local or worst <= BOUND * sc
    return ex


@pytest.mark.parametrize("name", [c[0] for c in em.designed_cases()])
def test_designed(name):
    _, trees, weights, X, XB, single = next(c for c in em.designed_cases() if c[0] == name)
    bg = None if XB is None else _dataset(XB)
    _check(_model(trees, weights, single), _dataset(X), X, bg=bg, XB=XB)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 128, 257])
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


# --- the kernels' limits (tests/test_explain_host.py shows that every model below sits where it claims) ----------------------
# Local accuracy against BOUND: BOUND is 8 x the restatement's measured error on models of at most 6 trees and 64 leaves a
# tree.  It is kept for the wide trees (256 to 288 leaves, like the depth-8 forest of test_trained_random_forest, and the
# chain of test_path_limit) and the small trees of the view tests; the 4096- and 4097-leaf trees and the 65 539-tree model
# add thousands of terms to one accumulator, which no case of that measurement does: there the ratio is printed and only
# the bytes are held.

@pytest.fixture(scope="module")
def cover_limit():
    X, XB, _ = em.cover_limit_case()
    return X, XB, _dataset(X), _dataset(XB, queries=700)


@pytest.mark.parametrize("name", ["leaves_4096", "leaves_4097", "mixed"])
def test_cover_pass_on_both_sides_of_the_lds_limit(cover_limit, name):
    """4096 leaves are counted in LDS, 4097 in the global counters; `mixed` alternates the two over blockIdx.y.  70 000
    background documents: more than the grid's 256 x 256, so every workgroup takes a second stretch.  The covers' reference
    is numpy's count on the 70 000 rows: the bias and every contribution depend on all of them."""
    X, XB, ds, bg = cover_limit
    trees, weights, single = em.cover_limit_case()[2][name]
    counts = em.leaf_counts(trees, XB)
    zero, reached = sum(c == 0 for c in counts), sum(c > 0 for c in counts)
    print("%s: %d leaves, %d without a background document, %d with" % (name, len(counts), zero, reached))
    assert zero >= 500 and reached >= 1000 and len(XB) > em.EX_COVER_GRID * 256
    ex = _check(_model(trees, weights, single), ds, X, bg=bg, XB=XB, counts=counts, local=False)
    assert ex.status["leaf_paths"] == len(counts)


def _view_rows(view):
    return np.array(sorted(i for ids in view.instances_by_query().values() for i in ids))


@pytest.fixture(scope="module")
def big3():
    X = np.random.default_rng(140).normal(0, 1, (140000, 3)).astype(np.float32)
    ds = _dataset(X, queries=1400)
    view = ds.subsample_queries([str(q) for q in range(1, 1401) if q % 3])  # two queries of every three
    return X, ds, view, _view_rows(view)


def test_cover_pass_background_is_a_sampled_view(cover_limit, big3):
    """The background's position list with gaps: every other query of the 70 000 documents (more than half the grid's
    reach), and two queries of three of 140 000 (more than the grid's reach: the stride loop over a list with gaps)."""
    X, XB, ds, bg = cover_limit
    trees, weights, _ = em.random_forest_model(25, d=4, trees=2, depth=4, n=16, p_leaf=0.1)
    view = bg.subsample_queries([str(q) for q in range(1, 701, 2)])
    rows = _view_rows(view)
    assert len(rows) == 35000 and len(rows) > em.EX_COVER_GRID * 256 // 2 and np.any(np.diff(rows) > 1)
    _check(_model(trees, weights), ds, X, bg=view, XB=XB[rows])
    X3, _, view3, rows3 = big3
    assert len(rows3) > em.EX_COVER_GRID * 256 and np.any(np.diff(rows3) > 1)
    trees, weights, _ = em.random_forest_model(26, d=3, trees=2, depth=4, n=16, p_leaf=0.1)
    _check(_model(trees, weights), _dataset(X[:, :3]), X[:, :3], bg=view3, XB=X3[rows3])


def test_more_trees_than_one_cover_launch():
    """65 539 trees: gridDim.y takes 65 535, so the cover pass launches twice, the second time from offset pointers.  The
    reference is em.restate_stumps (held to path_table + restate by tests/test_explain_host.py::test_stumps_restatement)."""
    import time

    trees, weights, X = em.stumps_case()
    assert len(trees) > em.EX_COVER_TREES
    ds = _dataset(X)
    model = _model(trees, weights)
    t0 = time.perf_counter()
    ex = model.explain(ds)
    took = time.perf_counter() - t0
    print("explain of 200 documents x %d trees: %.2f s (cover pass %.1f ms, kernel %.1f ms)" % (len(trees), took, ex.status["cover_ms"], ex.status["kernel_ms"]))
    phi, feats, bias, counts = em.restate_stumps(trees, weights, X[:64], X)
    assert feats == [0, 1] and list(ex.feature_ids) == [0, 1]
    for c in range(2):
        assert np.array_equal(_bits(ex.values[:64, c]), _bits(phi[:, c])), "feature %d" % c
    assert _bits(ex.expected_value) == _bits(bias)
    assert ex.status["trees"] == len(trees) and ex.status["leaf_paths"] == len(counts) and ex.status["max_path"] == 1
    # local accuracy, printed (see the note above): f(x) in numpy, the sum in tree order
    score = em.predict_stumps(trees, weights, X[:64])
    sc = em.scale(trees, weights)
    worst = max(abs(math.fsum(list(ex.values[i]) + [ex.expected_value]) - s) for i, s in enumerate(score))
    print("local accuracy: worst |sum phi + bias - f(x)| = %.3e = %.3e x scale (BOUND %.3e, not asserted)" % (worst, worst / sc, BOUND))


@pytest.fixture(scope="module")
def wide():
    X = em.wide_data()
    return X, _dataset(X)


@pytest.mark.parametrize("name", em.WIDE_FITS)
def test_contribution_kernel_lds_sizes(wide, name):
    """Dynamic LDS of 48 384 B (63 features), 49 152 B (64: exactly 48 KiB, the last size that needs no attribute), 49 920 B
    (65: the first that does), 104 448 B (all 136 of MSLR), a wide tree beside W rows, and 159 744 B = the limit to the byte,
    without W rows (208) and with all 33 of them (186 features and the 32-element chain)."""
    X, ds = wide
    trees, weights, single = em.wide_case(name)
    _check(_model(trees, weights, single), ds, X)


def test_lds_refusals_leave_nothing_behind(wide):
    X, ds = wide
    m208 = _model(*em.wide_case("wide_208"))
    before = _check(m208, ds, X)
    for name, n, need in (("wide_209", 209, 160512), ("long_187", 187, 160512)):
        refused = _model(*em.wide_case(name))
        what = "a tree that splits on %d distinct features needs %d bytes of LDS per wave, the explain kernel has %d" % (n, need, em.EX_LDS_MAX)
        with pytest.raises(Exception, match=what):
            refused.explain(ds)
        with pytest.raises(Exception, match=what):
            native.feature_importance(refused, ds)
        after = m208.explain(ds)
        assert np.array_equal(_bits(after.values), _bits(before.values)) and _bits(after.expected_value) == _bits(before.expected_value)


def test_lds_attribute_is_set_per_call(wide):
    # above 48 KiB, then far below it, then above again: each launch gets the LDS it asked for
    X, ds = wide
    m65 = _model(*em.wide_case("wide_65"))
    small = _model([em.S(0, 0.1, em.S(1, 0.0, em.L(1.0), em.L(-2.0)), em.S(2, 0.3, em.L(0.5), em.L(4.0)))], [1.0], single=True)
    first = _check(m65, ds, X)
    _check(small, ds, X)
    again = m65.explain(ds)
    assert np.array_equal(_bits(again.values), _bits(first.values)) and _bits(again.expected_value) == _bits(first.expected_value)


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


def _document_order(ds):
    """the instance ids in the order of the explained document list: positions ascending"""
    perm = native.device_form(ds)["perm_host"]
    return perm[perm != 0xFFFFFFFF].astype(np.int64)


def _importance_bits(model, ds, n):
    """feature_importance = em.importance_restate of the device's own contributions (which the tests above hold to the
    restatement), bit for bit: a tile or a lane dropped or doubled is one part in n, inside gamma_n but not inside this"""
    values = model.explain(ds).values
    order = _document_order(ds)
    assert len(order) == n and len(set(order.tolist())) == n and not np.any(np.isnan(values[order]))
    want = em.importance_restate(values[order])
    _, a, rep = native.feature_importance(model, ds)
    assert rep["documents"] == n
    print("n = %d (%d tiles, %d in the last): device %s, restated %s" % (n, (n + 63) // 64, n - (n - 1) // 64 * 64, a, want))
    assert np.array_equal(_bits(a), _bits(want))
    ref = np.abs(values[order]).mean(0)
    gamma = n * 2.0 ** -53 / (1 - n * 2.0 ** -53)
    assert np.all(np.abs(a - ref) <= gamma * ref)
    return a


IMPORTANCE_TREE = em.S(0, 0.0, em.S(1, 0.5, em.L(1.0), em.L(-2.0)), em.L(3.0))  # (test_feature_importance_chunks')


@pytest.mark.parametrize("n", [65535, 65536, 65537, 65600, 131073])
def test_feature_importance_reduction_at_the_chunk_boundary(n):
    """One launch is 1024 tiles = 65 536 documents: a partial tile that ends the first launch, the exact boundary, one lane
    and a partial tile in a second launch, one lane in a third."""
    assert em.EX_CHUNK_TILES * 64 == 65536
    X = np.random.default_rng(n).normal(0, 1, (n, 3)).astype(np.float32)
    ds = _dataset(X, queries=600)
    a = _importance_bits(_model([IMPORTANCE_TREE], [1.0], single=True), ds, n)
    assert a[2] == 0.0 and a[0] > 0.0 and a[1] > 0.0
    if n == 65600:
        two = _model([IMPORTANCE_TREE, em.S(2, -0.25, em.L(0.5), em.S(0, 1.0, em.L(-1.5), em.L(2.5)))], [0.75, -1.25])
        assert np.all(_importance_bits(two, ds, n) > 0.0)


def test_feature_importance_reduction_on_a_sampled_view(big3):
    X, ds, view, rows = big3
    assert len(rows) > em.EX_CHUNK_TILES * 64
    order = _document_order(view)
    assert np.array_equal(np.sort(order), rows)
    _importance_bits(_model([IMPORTANCE_TREE], [1.0], single=True), view, len(rows))


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
