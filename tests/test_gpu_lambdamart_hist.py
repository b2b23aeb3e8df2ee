"""LambdaMART's histogram grower on the device against the numpy restatement (tests/lambdamart_hist_model.py, DESIGN.md
section 11): every stage on its own (bins, one tree from given gradients), then training stage by stage."""
import json
import os
import time

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import native
from oracle import pyoracle as o
from tests import lambdamart_hist_model as hm
from tests import lambdamart_model as lm
from tests.conftest import GOLDEN, synth_dataset
from tests.test_lambdamart_hist_host import LEARNING_CASE

pytestmark = pytest.mark.gpu


def _request(measure="ndcg", grower="histogram", **kw):
    req = fr.TrainRequest.lambdamart()
    req.measure = measure
    req.params.quiet = True
    if grower is not None:
        req.params.grower = grower
    for k, v in kw.items():
        setattr(req.params, k, v)
    return req


@pytest.fixture(scope="module")
def trec():
    d = np.load(os.path.join(GOLDEN, "trec_news_2018.npz"))
    X, y, qid = d["train_X"], d["train_y"], d["train_qid"]
    return X, y, qid, fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)


@pytest.fixture(scope="module")
def synth():
    X, y, qid = synth_dataset(7, 5000, 10, 50)
    X = X.copy()
    X[::7, 3] = -0.0  # signed zeros in a sparse column
    X[:, 9] = 2.5     # a constant column: no edge, never split on
    return X, y, qid, fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)


def _order_ids(c):
    return np.concatenate(lm.query_lists(c))


def _check_bins(g, X, order_ids, feats, k):
    ids, fids, edges, bins = native.hist_bins(g, k)
    assert np.array_equal(ids, order_ids)
    assert list(fids) == list(feats)
    eedges, ebins = hm.bin_matrix(X, order_ids, feats, k)
    for s, f in enumerate(feats):
        assert edges[s].dtype == np.float32
        assert edges[s].tobytes() == eedges[s].tobytes(), "feature %d (k = %d): edges differ" % (f, k)
    assert np.array_equal(bins, ebins)
    return edges, bins


# --- bins ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [2, 16, 64, 256])
def test_bins_trec(trec, k):
    X, y, qid, g, c = trec
    _check_bins(g, X, _order_ids(c), range(X.shape[1]), k)


@pytest.mark.parametrize("k", [2, 7, 64, 256])
def test_bins_synthetic_integer_sparse_constant_columns(synth, k):
    X, y, qid, g, c = synth
    edges, bins = _check_bins(g, X, _order_ids(c), range(X.shape[1]), k)
    assert len(edges[9]) == 0 and not bins[9].any()
    assert len(edges[1]) < min(k, len(np.unique(X[:, 1])))  # the integer column: one bin per value when they fit


def test_bins_of_a_sampled_view(trec):
    X, y, qid, g, c = trec
    names = sorted(g.queries())
    sub = g.subsample_queries(names[::2]).subsample_feature_names(sorted(g.feature_names())[1::2])
    feats = sorted(sub.feature_ids())
    ids, fids, edges, bins = native.hist_bins(sub, 16)
    rows = np.flatnonzero(np.isin(np.array([str(int(q)) for q in qid]), names[::2]))
    assert sorted(ids) == list(rows) and list(fids) == feats
    by_q = {}
    for i in ids:  # queries contiguous, ids ascending inside each
        by_q.setdefault(int(qid[i]), []).append(int(i))
    assert np.array_equal(np.concatenate([by_q[q] for q in by_q]), ids)
    assert all(v == sorted(v) for v in by_q.values())
    eedges, ebins = hm.bin_matrix(X, ids, feats, 16)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(edges, eedges))
    assert np.array_equal(bins, ebins)


def test_bins_of_a_file_loaded_dataset_read_absent_values_as_zero():
    rd = fr.CDataset.open_ranksvm(os.path.join(GOLDEN, "data", "trec_news_2018.train"))
    d = np.load(os.path.join(GOLDEN, "trec_news_2018.npz"))
    X, y, qid = d["train_X"], d["train_y"], d["train_qid"]
    c = o.Dataset(X, y, qid)
    for k in (8, 256):
        _check_bins(rd, X, _order_ids(c), sorted(rd.feature_ids()), k)


def test_nan_feature_is_a_plain_error():
    X, y, qid = synth_dataset(5, 400, 4, 8)
    X = X.copy()
    X[17, 2] = np.nan
    g = fr.CDataset.from_numpy(X, y, qid)
    with pytest.raises(Exception, match="a feature value is NaN"):
        native.hist_bins(g, 16)
    with pytest.raises(Exception, match="a feature value is NaN"):
        g.train_model(_request(num_trees=1))


# --- one tree from given gradients ---------------------------------------------------------------

def _one_tree(g, X, order_ids, lam, wt, k, depth, min_leaf):
    got = native.hist_tree(g, lam, wt, k, depth, min_leaf).to_dict()["DecisionTree"]
    exp = hm.fit_tree(X, lam, wt, order_ids, range(X.shape[1]), depth, min_leaf, k)
    assert got == exp, "k = %d, depth %d, min_leaf %d" % (k, depth, min_leaf)
    return got


def _depth(node):
    if "LeafNode" in node:
        return 1
    return 1 + max(_depth(node["FeatureSplit"]["lhs"]), _depth(node["FeatureSplit"]["rhs"]))


@pytest.mark.parametrize("k", [2, 16, 64, 256])
@pytest.mark.parametrize("depth,min_leaf", [(1, 1), (4, 1), (4, 400), (10, 1), (10, 25)])
def test_one_tree_equals_restatement(synth, k, depth, min_leaf):
    X, y, qid, g, c = synth
    rng = np.random.default_rng(100 * k + depth)
    lam = rng.normal(0.0, 1.0, len(y)) + 0.5 * (y - y.mean())
    wt = rng.random(len(y))
    tree = _one_tree(g, X, _order_ids(c), lam, wt, k, depth, min_leaf)
    assert _depth(tree) <= depth
    if depth > 1:
        assert "FeatureSplit" in tree


def test_one_tree_special_gradients(synth):
    X, y, qid, g, c = synth
    n = len(y)
    ids = _order_ids(c)
    rng = np.random.default_rng(8)
    wt = rng.random(n)
    assert native.hist_tree(g, np.zeros(n), wt, 16, 4, 1).to_dict() == {"DecisionTree": {"LeafNode": 0.0}}
    # largest magnitude a power of two; every weight zero (leaves 0.0 under splits); tiny and huge magnitudes
    lam = rng.integers(-8, 9, n) / 8.0
    lam[5] = -4.0
    _one_tree(g, X, ids, lam, wt, 16, 5, 10)
    tree = _one_tree(g, X, ids, lam, np.zeros(n), 16, 3, 10)
    assert "FeatureSplit" in tree
    _one_tree(g, X, ids, lam * 1e-300, wt * 1e-12, 64, 4, 10)
    _one_tree(g, X, ids, lam * 1e200, wt * 1e100, 64, 4, 10)
    # gradients equal inside every bin of every feature: ties between candidates, the last one wins on both sides
    _one_tree(g, X, ids, np.where(X[:, 1] > 2, 1.0, -1.0), np.ones(n), 64, 3, 1)


def test_one_tree_with_many_workgroups_per_histogram():
    """60 000 instances: eight workgroups per feature block add into the root's histogram, and the children's stretches
    are cut as well."""
    X, y, qid = synth_dataset(19, 60000, 12, 300)
    g, c = fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)
    rng = np.random.default_rng(4)
    lam = rng.normal(0.0, 1.0, len(y)) * np.exp(rng.normal(0.0, 3.0, len(y))) + 0.3 * (y - 1)
    wt = rng.random(len(y))
    ids = _order_ids(c)
    _check_bins(g, X, ids, range(X.shape[1]), 256)
    for k, depth, min_leaf in ((256, 6, 10), (64, 10, 1)):
        _one_tree(g, X, ids, lam, wt, k, depth, min_leaf)


# --- training ------------------------------------------------------------------------------------

def _stagewise(g, c, X, measure, T, params):
    req = _request(measure, num_trees=T, **params)
    model = g.train_model(req)
    st = native.last_train_stats()["lambdamart"]
    d = model.to_dict()
    trees = [m["DecisionTree"] for m in d["Ensemble"]["models"]]
    assert d["Ensemble"]["weights"] == [req.params.learning_rate] * T
    order_ids = _order_ids(c)
    feats = list(range(X.shape[1]))
    binned = hm.bin_matrix(X, order_ids, feats, req.params.split_candidates)
    for t in range(T):
        prefix = fr.CModel.from_dict({"Ensemble": {"weights": [req.params.learning_rate] * t,
                                                   "models": [{"DecisionTree": x} for x in trees[:t]]}})
        lam, wt = native.lambda_gradients(prefix, g, measure, req.params.sigma)
        exp = hm.fit_tree(X, lam, wt, order_ids, feats, req.params.max_depth, req.params.min_leaf_support,
                          req.params.split_candidates, binned)
        assert trees[t] == exp, "tree %d differs from the restatement's fit" % t
        _, per_q = native.evaluate_dense(fr.CModel.from_dict({"Ensemble": {
            "weights": [req.params.learning_rate] * (t + 1), "models": [{"DecisionTree": x} for x in trees[:t + 1]]}}), g, measure)
        assert st["train_measure"][t] == o.mean(per_q)
    exp_scores = c.score_ensemble(trees, d["Ensemble"]["weights"])
    assert np.array_equal(native.predict_scores_dense(model, g), exp_scores)
    return model, st


def test_stagewise_identity_trec(trec):
    X, y, qid, g, c = trec
    _, st = _stagewise(g, c, X, "ndcg@10", 20, dict(max_depth=5, min_leaf_support=5, split_candidates=16))
    assert st["grower"] == "histogram" and st["bins"] == 16 and st["bins_ms"] >= 0.0 and st["trees"] == 20
    for key in ("seconds", "gradient_ms", "grow_ms", "leaves_ms", "update_ms"):
        assert st[key] >= 0.0


def test_stagewise_identity_synthetic(synth):
    X, y, qid, g, c = synth
    _stagewise(g, c, X, "ndcg", 20, dict(max_depth=6, min_leaf_support=10, split_candidates=64))


def test_learns_like_the_restatement():
    """The case the host test shows the restatement learning on: the device's training measure rises the same way."""
    k = LEARNING_CASE
    X, y, qid = synth_dataset(k["seed"], k["n"], k["d"], k["q"])
    g, c = fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)
    _, st = _stagewise(g, c, X, k["measure"], k["num_trees"], dict(max_depth=k["max_depth"], min_leaf_support=k["min_leaf_support"],
                                                                   split_candidates=k["split_candidates"]))
    assert st["train_measure"][-1] > st["train_measure"][0] + 0.02


def test_deterministic_and_bins_are_reused(trec):
    X, y, qid, g, c = trec
    g = fr.CDataset.from_numpy(X, y, qid)  # (a dataset of its own: no bins yet)
    req = _request("ndcg", num_trees=6, max_depth=4, min_leaf_support=5, split_candidates=16)
    a = json.dumps(g.train_model(req).to_dict())
    first = native.last_train_stats()["lambdamart"]
    b = json.dumps(g.train_model(req).to_dict())
    second = native.last_train_stats()["lambdamart"]
    assert a == b
    assert first["bins_ms"] > 0.0 and second["bins_ms"] == 0.0
    req.params.split_candidates = 8  # another k: binned again
    g.train_model(req)
    assert native.last_train_stats()["lambdamart"]["bins_ms"] > 0.0


def test_exact_path_is_untouched(trec):
    X, y, qid, g, c = trec
    kw = dict(num_trees=5, max_depth=4, min_leaf_support=5, split_candidates=16)
    absent = _request("ndcg@10", grower=None, **kw)
    assert "grower" not in absent.to_dict()["params"]["LambdaMART"]
    a = json.dumps(g.train_model(absent).to_dict())
    st = native.last_train_stats()["lambdamart"]
    assert st["grower"] == "exact" and st["bins_ms"] == 0.0 and "bins" not in st
    wire = absent.to_dict()
    wire["params"]["LambdaMART"]["grower"] = "exact"
    from fastrank_amd import clib
    m = fr.CModel(clib._unwrap(clib._load().train_model(json.dumps(wire).encode(), g.pointer)))
    assert json.dumps(m.to_dict()) == a
    hist = json.dumps(g.train_model(_request("ndcg@10", **kw)).to_dict())
    assert hist != a
    # ... and what it gives is the exact grower's restatement, as before
    exp = lm.fit_tree(X, *native.lambda_gradients(fr.CModel.from_dict({"Ensemble": {"weights": [], "models": []}}), g, "ndcg@10", 1.0),
                      _order_ids(c), range(X.shape[1]), 4, 5, 16)
    assert json.loads(a)["Ensemble"]["models"][0]["DecisionTree"] == exp


def test_query_subsample_trains_like_its_own_rows(trec):
    X, y, qid, g, c = trec
    names = sorted(g.queries())
    sub = g.subsample_queries(names[::2])
    rows = np.isin(np.array([str(int(q)) for q in qid]), names[::2])
    own = fr.CDataset.from_numpy(np.ascontiguousarray(X[rows]), np.ascontiguousarray(y[rows]), np.ascontiguousarray(qid[rows]))
    req = _request("ndcg@10", num_trees=8, max_depth=4, min_leaf_support=4, split_candidates=16)
    assert sub.train_model(req).to_dict() == own.train_model(req).to_dict()


def test_30k_shape_view_equals_restatement():
    """The 30K shape (3.8 M documents x 136 features): three default-depth trees with 64 bins on a view of every tenth
    query (about 380 000 documents: the restatement of the bins and the three trees takes 8 s there, the whole test 13 s;
    at full size it would take minutes) equal the restatement's, and two default trees on the whole set keep the
    training identities."""
    from tests.test_gpu_fullsize import _shape

    _, X, y, qid, g = _shape("30k")
    names = sorted(g.queries())
    sub = g.subsample_queries(names[::10])
    ids, fids, edges, bins = native.hist_bins(sub, 64)
    assert len(ids) > 300_000 and len(fids) == X.shape[1]
    t0 = time.time()
    binned = hm.bin_matrix(X, ids, list(fids), 64)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(edges, binned[0]))
    assert np.array_equal(bins, binned[1])
    req = _request("ndcg@10", num_trees=3, split_candidates=64)
    trees = [m["DecisionTree"] for m in sub.train_model(req).to_dict()["Ensemble"]["models"]]
    n_total = X.shape[0]
    for t in range(3):
        prefix = fr.CModel.from_dict({"Ensemble": {"weights": [0.1] * t, "models": [{"DecisionTree": x} for x in trees[:t]]}})
        lam, wt = native.lambda_gradients(prefix, sub, "ndcg@10", 1.0, n_total=n_total)
        lam, wt = np.nan_to_num(lam), np.nan_to_num(wt)  # (ids outside the view: never read)
        exp = hm.fit_tree(X, lam, wt, ids, list(fids), 6, 10, 64, binned)
        assert trees[t] == exp, "tree %d" % t
        assert _depth(trees[t]) == 6
    print("30K-shape view: restatement of bins and 3 trees took %.0f s" % (time.time() - t0))
    model = g.train_model(_request("ndcg@10", num_trees=2, split_candidates=64))
    st = native.last_train_stats()["lambdamart"]
    _, per_q = native.evaluate_dense(model, g, "ndcg@10")
    o.set_mean_segment(o.DEVICE_MEAN_SEGMENT)  # (31 000 queries: the device's two-level summation shape)
    try:
        assert st["train_measure"][-1] == o.mean(per_q)
    finally:
        o.set_mean_segment(0)
    assert st["train_measure"][1] > st["train_measure"][0]
    assert json.dumps(g.train_model(_request("ndcg@10", num_trees=2, split_candidates=64)).to_dict()) == json.dumps(model.to_dict())
