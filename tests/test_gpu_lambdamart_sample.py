"""LambdaMART's per-tree query and feature samples on the device against the numpy restatement
(tests/lambdamart_sample_model.py, DESIGN.md section 11, "Sampling"): the sampled gradient pass, one histogram tree on a
sample from given gradients, then training stage by stage with both growers."""
import json
import os

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import native
from oracle import pyoracle as o
from tests import lambdamart_hist_model as hm
from tests import lambdamart_model as lm
from tests import lambdamart_sample_model as sm
from tests.conftest import GOLDEN, synth_dataset

pytestmark = pytest.mark.gpu

EMPTY = {"Ensemble": {"weights": [], "models": []}}


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
    X[::7, 3] = -0.0
    X[:, 9] = 2.5
    return X, y, qid, fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)


def _ensemble(trees, lr):
    return fr.CModel.from_dict({"Ensemble": {"weights": [lr] * len(trees), "models": [{"DecisionTree": x} for x in trees]}})


# --- the sampled gradient pass -------------------------------------------------------------------

def _check_sampled_gradients(g, queries, model, measure, sigma, samples):
    full_l, full_w = native.lambda_gradients(model, g, measure, sigma)
    assert np.all(np.isfinite(full_l)) and np.all(np.isfinite(full_w))
    for qsel in samples:
        qsel = np.asarray(qsel)
        lam, wt = native.lambda_gradients(model, g, measure, sigma, queries=qsel)
        inside = np.zeros(len(full_l), dtype=bool)
        inside[np.concatenate([queries[q] for q in qsel])] = True
        assert lam[inside].tobytes() == full_l[inside].tobytes(), "lambda of a sampled query differs from the full pass"
        assert wt[inside].tobytes() == full_w[inside].tobytes(), "w of a sampled query differs from the full pass"
        assert np.all(np.isnan(lam[~inside])) and np.all(np.isnan(wt[~inside]))
    # the full pass afterwards is what it was
    again_l, again_w = native.lambda_gradients(model, g, measure, sigma)
    assert again_l.tobytes() == full_l.tobytes() and again_w.tobytes() == full_w.tobytes()


def _gradient_samples(queries, seed):
    nq = len(queries)
    lens = np.array([len(ids) for ids in queries])
    longest = int(np.argmax(lens))
    out = [[longest], [q for q in range(nq) if q != longest], [0], [nq - 1], list(range(nq))]
    for t in range(3):
        out.append(sm.sample(seed, t, 1, nq, (0.5, 1.0))[1])
    out.append(sm.sample(seed, 0, 1, nq, (0.1, 1.0))[1])
    return out


@pytest.mark.parametrize("measure", ["ndcg", "ndcg@10"])
def test_sampled_gradients_trec(trec, measure):
    X, y, qid, g, c = trec
    model = fr.CModel.from_dict({"Linear": {"weights": [0.0, 0.3, -0.2, 0.5, 0.1, 0.9]}})
    queries = lm.query_lists(c)
    _check_sampled_gradients(g, queries, model, measure, 1.0, _gradient_samples(queries, 3))


def test_sampled_gradients_synthetic(synth):
    X, y, qid, g, c = synth
    w = [0.0] * X.shape[1]
    w[1], w[5] = 1.0, 2.0  # integer columns: tied scores
    model = fr.CModel.from_dict({"Linear": {"weights": w}})
    queries = lm.query_lists(c)
    _check_sampled_gradients(g, queries, model, "ndcg@10", 1.5, _gradient_samples(queries, 4))
    _check_sampled_gradients(g, queries, fr.CModel.from_dict(EMPTY), "ndcg", 1.0, _gradient_samples(queries, 5)[:3])


def test_sampled_gradients_on_queries_longer_than_lds():
    """The long-query construction of the gradient tests: 6 001, 5 000 (no positive label), 4 099 and 4 097 documents take
    the slab path, 4 096 and 4 095 the LDS path at its limit.  Samples of slab queries only, LDS queries only, one of
    each, the longest alone and all but the longest."""
    from tests.test_gpu_lambdamart import _long_query_set

    X, y, qid = _long_query_set()
    g, c = fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)
    queries = lm.query_lists(c)
    by_len = {len(ids): q for q, ids in enumerate(queries)}
    model = fr.CModel.from_dict({"Linear": {"weights": [0.25, 1.0, 0.0, 0.0, 0.5, 0.0]}})
    samples = [[by_len[6001]], [q for q in range(len(queries)) if q != by_len[6001]],
               [by_len[4097], by_len[4099]], [by_len[4097]], [by_len[5000], by_len[2]],
               [by_len[4096], by_len[4095], by_len[300]], [by_len[4097], by_len[4096], by_len[1]], [by_len[1]]]
    _check_sampled_gradients(g, queries, model, "ndcg@10", 1.5, samples)


# --- one histogram tree on a sample, from given gradients ----------------------------------------

def _one_tree(g, X, queries, feats, lam, wt, k, depth, min_leaf, qsel=None, fsel=None, binned=None):
    """feats: the view's features ascending; qsel: indices of queries, fsel: indices into feats (None: all)."""
    order_ids = np.concatenate(queries)
    binned = binned if binned is not None else hm.bin_matrix(X, order_ids, feats, k)
    q = np.arange(len(queries)) if qsel is None else np.asarray(qsel)
    f = np.arange(len(feats)) if fsel is None else np.asarray(fsel)
    # gradients outside the query sample must not be read: poison them
    lam_in, wt_in = np.array(lam, dtype=np.float64), np.array(wt, dtype=np.float64)
    if qsel is not None:
        outside = np.ones(len(lam_in), dtype=bool)
        outside[np.concatenate([queries[x] for x in q])] = False
        lam_in[outside], wt_in[outside] = np.nan, np.inf
    got = native.hist_tree(g, lam_in, wt_in, k, depth, min_leaf, queries=None if qsel is None else q,
                           features=None if fsel is None else [feats[s] for s in f]).to_dict()["DecisionTree"]
    exp = sm.hist_tree(X, lam, wt, order_ids, feats, binned, sm.instance_rows(queries, q), f, depth, min_leaf, k)
    assert got == exp, "k = %d, depth %d, min_leaf %d, %d queries, %d features" % (k, depth, min_leaf, len(q), len(f))
    return got


def _depth(node):
    if "LeafNode" in node:
        return 1
    return 1 + max(_depth(node["FeatureSplit"]["lhs"]), _depth(node["FeatureSplit"]["rhs"]))


def _fids(node):
    if "LeafNode" in node:
        return set()
    fs = node["FeatureSplit"]
    return {fs["fid"]} | _fids(fs["lhs"]) | _fids(fs["rhs"])


def _gradients_for(y, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0.0, 1.0, len(y)) + 0.5 * (y - y.mean()), rng.random(len(y))


@pytest.mark.parametrize("k", [2, 64, 256])
@pytest.mark.parametrize("depth,min_leaf", [(1, 1), (4, 1), (10, 1), (10, 25)])
def test_one_tree_on_a_sample_equals_restatement(synth, k, depth, min_leaf):
    X, y, qid, g, c = synth
    queries = lm.query_lists(c)
    feats = list(range(X.shape[1]))
    lam, wt = _gradients_for(y, 100 * k + depth)
    binned = hm.bin_matrix(X, np.concatenate(queries), feats, k)
    fsel, qsel = sm.sample(k + depth, 0, len(feats), len(queries), (0.5, 0.5))
    tree = _one_tree(g, X, queries, feats, lam, wt, k, depth, min_leaf, qsel, fsel, binned)
    assert _depth(tree) <= depth and _fids(tree) <= set(feats[s] for s in fsel)
    _one_tree(g, X, queries, feats, lam, wt, k, depth, min_leaf, qsel, None, binned)
    _one_tree(g, X, queries, feats, lam, wt, k, depth, min_leaf, None, fsel, binned)
    # without a sample afterwards: the unsampled tree, as before
    _one_tree(g, X, queries, feats, lam, wt, k, depth, min_leaf, None, None, binned)


@pytest.mark.parametrize("nf", [1, 7, 8, 9, 20])
def test_one_tree_around_the_feature_block(nf):
    """hist_build_kernel takes eight features per workgroup: samples of 1, 7, 8, 9 and all of 20 features, contiguous and
    scattered."""
    X, y, qid = synth_dataset(31, 4000, 20, 40)
    g, c = fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)
    queries = lm.query_lists(c)
    feats = list(range(20))
    lam, wt = _gradients_for(y, nf)
    binned = hm.bin_matrix(X, np.concatenate(queries), feats, 64)
    rng = np.random.default_rng(nf)
    for fsel in (np.arange(nf), np.arange(20 - nf, 20), np.sort(rng.choice(20, nf, replace=False))):
        for qsel in (None, sm.sample(nf, 1, 1, len(queries), (0.5, 1.0))[1]):
            tree = _one_tree(g, X, queries, feats, lam, wt, 64, 5, 5, qsel, fsel, binned)
            assert _fids(tree) <= set(int(s) for s in fsel)


def test_one_tree_small_samples(synth):
    X, y, qid, g, c = synth
    queries = lm.query_lists(c)
    feats = list(range(X.shape[1]))
    lam, wt = _gradients_for(y, 77)
    binned = hm.bin_matrix(X, np.concatenate(queries), feats, 16)
    shortest = int(np.argmin([len(ids) for ids in queries]))
    for q in (0, len(queries) - 1, shortest):  # a sample of one query
        _one_tree(g, X, queries, feats, lam, wt, 16, 4, 1, [q], None, binned)
    # fewer sampled instances than min_leaf_support: a single leaf, the Newton step over the sample
    n_t = len(queries[shortest])
    tree = _one_tree(g, X, queries, feats, lam, wt, 16, 6, n_t + 1, [shortest], [0, 2, 4], binned)
    assert "LeafNode" in tree and tree["LeafNode"] != 0.0
    # the sample's gradients all zero although others are not
    lam0 = lam.copy()
    lam0[queries[3]] = 0.0
    assert _one_tree(g, X, queries, feats, lam0, wt, 16, 4, 1, [3], None, binned) == {"LeafNode": 0.0}
    # the constant column alone: nothing to split on
    assert "LeafNode" in _one_tree(g, X, queries, feats, lam, wt, 16, 4, 1, None, [9], binned)


def test_one_tree_with_many_workgroups_per_histogram():
    """More than 60 000 sampled instances of 120 000: eight or more workgroups per feature block add into the root's
    histogram."""
    X, y, qid = synth_dataset(19, 120000, 12, 600)
    g, c = fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)
    queries = lm.query_lists(c)
    feats = list(range(12))
    rng = np.random.default_rng(4)
    lam = rng.normal(0.0, 1.0, len(y)) * np.exp(rng.normal(0.0, 3.0, len(y))) + 0.3 * (y - 1)
    wt = rng.random(len(y))
    fsel, qsel = sm.sample(8, 0, 12, len(queries), (0.55, 0.75))
    assert len(sm.instance_rows(queries, qsel)) >= 60000
    for k, depth, min_leaf in ((256, 6, 10), (64, 10, 1)):
        _one_tree(g, X, queries, feats, lam, wt, k, depth, min_leaf, qsel, fsel)


# --- training ------------------------------------------------------------------------------------

def _stagewise(g, X, queries, feats, measure, T, grower, rates, seed, params, c=None, present=None, n_total=None):
    """Every tree equals the restatement's fit on the restatement's sample to the device's gradients of the prefix model;
    with the oracle dataset `c` of the same rows also the running scores and the training measure."""
    req = _request(measure, grower, num_trees=T, query_sampling_rate=rates[0], feature_sampling_rate=rates[1], seed=seed, **params)
    p = req.params
    model = g.train_model(req)
    st = native.last_train_stats()["lambdamart"]
    d = model.to_dict()
    trees = [m["DecisionTree"] for m in d["Ensemble"]["models"]]
    assert d["Ensemble"]["weights"] == [p.learning_rate] * T
    order_ids = np.concatenate(queries)
    binned = hm.bin_matrix(X, order_ids, feats, p.split_candidates) if grower == "histogram" else None
    nq_t, n_t, nf_t = 0, 0, 0
    for t in range(T):
        fsel, qsel = sm.sample(seed, t, len(feats), len(queries), rates)
        hf, hq = native.lambdamart_sample(g, p, t)
        assert np.array_equal(hf, np.asarray(feats)[fsel]) and np.array_equal(hq, qsel)
        lam, wt = native.lambda_gradients(_ensemble(trees[:t], p.learning_rate), g, measure, p.sigma, n_total=n_total)
        exp = sm.tree_for(grower, X, np.nan_to_num(lam), np.nan_to_num(wt), queries, feats, binned, qsel, fsel, p.max_depth,
                          p.min_leaf_support, p.split_candidates, present)
        assert trees[t] == exp, "tree %d differs from the restatement's fit on its sample" % t
        nq_t, n_t, nf_t = nq_t + len(qsel), n_t + len(sm.instance_rows(queries, qsel)), nf_t + len(fsel)
        if c is not None:
            _, per_q = native.evaluate_dense(_ensemble(trees[:t + 1], p.learning_rate), g, measure)
            assert st["train_measure"][t] == o.mean(per_q)
            exp_q, _ = c.metric_from_scores(measure, c.score_ensemble(trees[:t + 1], [p.learning_rate] * (t + 1)))
            assert st["train_measure"][t] == o.mean(exp_q)
    if c is not None:
        assert np.array_equal(native.predict_scores_dense(model, g), c.score_ensemble(trees, d["Ensemble"]["weights"]))
    if rates[0] < 1.0 or rates[1] < 1.0:
        assert (st["query_sampling_rate"], st["feature_sampling_rate"], st["seed"]) == (rates[0], rates[1], seed)
        assert st["sample_queries"] == nq_t / T and st["sample_instances"] == n_t / T and st["sample_features"] == nf_t / T
    assert st["grower"] == grower and st["trees"] == T
    return model, st


RATES = [(0.5, 1.0), (1.0, 0.3), (0.5, 0.25)]


@pytest.mark.parametrize("rates", RATES)
@pytest.mark.parametrize("grower", ["exact", "histogram"])
def test_stagewise_identity_trec(trec, grower, rates):
    X, y, qid, g, c = trec
    _stagewise(g, X, lm.query_lists(c), list(range(X.shape[1])), "ndcg@10", 20, grower, rates, 11,
               dict(max_depth=5, min_leaf_support=5, split_candidates=16), c=c)


@pytest.mark.parametrize("rates", RATES)
@pytest.mark.parametrize("grower", ["exact", "histogram"])
def test_stagewise_identity_synthetic(synth, grower, rates):
    X, y, qid, g, c = synth
    _stagewise(g, X, lm.query_lists(c), list(range(X.shape[1])), "ndcg", 20, grower, rates, 2 ** 63 + 5,
               dict(max_depth=6, min_leaf_support=10, split_candidates=64), c=c)


def test_bins_are_built_once(trec):
    X, y, qid, g, c = trec
    g = fr.CDataset.from_numpy(X, y, qid)  # (a dataset of its own: no bins yet)
    kw = dict(num_trees=6, max_depth=4, min_leaf_support=5, split_candidates=16)
    g.train_model(_request("ndcg", **kw))
    assert native.last_train_stats()["lambdamart"]["bins_ms"] > 0.0
    ids, fids, edges, bins = native.hist_bins(g, 16)
    for rates in RATES:
        g.train_model(_request("ndcg", query_sampling_rate=rates[0], feature_sampling_rate=rates[1], seed=5, **kw))
        assert native.last_train_stats()["lambdamart"]["bins_ms"] == 0.0
        ids2, fids2, edges2, bins2 = native.hist_bins(g, 16)
        assert np.array_equal(ids, ids2) and np.array_equal(fids, fids2) and np.array_equal(bins, bins2)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(edges, edges2))
    # ... and an unsampled training after the sampled ones is what it was before them
    a = json.dumps(g.train_model(_request("ndcg", **kw)).to_dict())
    own = fr.CDataset.from_numpy(X, y, qid)
    assert a == json.dumps(own.train_model(_request("ndcg", **kw)).to_dict())
    assert native.last_train_stats()["lambdamart"]["bins_ms"] > 0.0


@pytest.mark.parametrize("grower", ["exact", "histogram"])
def test_same_request_same_model_other_seed_other_model(synth, grower):
    X, y, qid, g, c = synth
    kw = dict(num_trees=5, max_depth=4, min_leaf_support=10, split_candidates=16, query_sampling_rate=0.5, feature_sampling_rate=0.5)
    a = json.dumps(g.train_model(_request("ndcg@10", grower, seed=1, **kw)).to_dict())
    b = json.dumps(g.train_model(_request("ndcg@10", grower, seed=1, **kw)).to_dict())
    other = json.dumps(g.train_model(_request("ndcg@10", grower, seed=2, **kw)).to_dict())
    assert a == b and a != other


@pytest.mark.parametrize("grower", ["exact", "histogram"])
def test_full_rates_are_the_request_without_the_keys(trec, grower):
    X, y, qid, g, c = trec
    kw = dict(num_trees=5, max_depth=4, min_leaf_support=5, split_candidates=16)
    absent = _request("ndcg@10", grower, **kw)
    assert not set(absent.to_dict()["params"]["LambdaMART"]) & {"query_sampling_rate", "feature_sampling_rate", "seed"}
    a = json.dumps(g.train_model(absent).to_dict())
    keys = sorted(native.last_train_stats()["lambdamart"].keys())
    assert "sample_queries" not in keys and "seed" not in keys
    from fastrank_amd import clib
    for seed in (0, 1, 2 ** 64 - 1):
        wire = absent.to_dict()
        wire["params"]["LambdaMART"].update(query_sampling_rate=1.0, feature_sampling_rate=1.0, seed=seed)
        m = fr.CModel(clib._unwrap(clib._load().train_model(json.dumps(wire).encode(), g.pointer)))
        assert json.dumps(m.to_dict()) == a
        assert sorted(native.last_train_stats()["lambdamart"].keys()) == keys
    assert json.dumps(g.train_model(_request("ndcg@10", grower, seed=77, **kw)).to_dict()) == a


@pytest.mark.parametrize("grower", ["exact", "histogram"])
def test_a_sampled_view_trains_like_the_restatement(trec, grower):
    X, y, qid, g, c = trec
    names = sorted(g.queries())
    sub = g.subsample_queries(names[::2]).subsample_feature_names(sorted(g.feature_names())[1:])
    feats = sorted(sub.feature_ids())
    ids = native.hist_bins(sub, 16)[0].astype(np.int64)
    cuts = np.flatnonzero(np.diff(qid[ids]) != 0) + 1
    queries = np.split(ids, cuts)
    assert len(queries) == len(names[::2]) and all(np.all(np.diff(q) > 0) for q in queries)
    _stagewise(sub, X, queries, feats, "ndcg@10", 8, grower, (0.5, 0.6), 21, dict(max_depth=4, min_leaf_support=4, split_candidates=16),
               n_total=X.shape[0])


def test_a_file_loaded_dataset_trains_like_the_restatement(tmp_path):
    """Absent values read 0.0 in the bins; the exact grower takes a feature's range over the held values (the mask)."""
    from tests.conftest import ranksvm_presence
    from tests.test_gpu_lambdamart import _sparse_file

    path = str(tmp_path / "sparse.train")
    X, y, qid = _sparse_file(path)
    rd = fr.CDataset.open_ranksvm(path)
    c = o.Dataset(X, y, qid)
    present = ranksvm_presence(path, X.shape[1])
    feats = sorted(rd.feature_ids())
    queries = lm.query_lists(c)
    kw = dict(max_depth=4, min_leaf_support=3, split_candidates=16)
    _stagewise(rd, X, queries, feats, "ndcg@10", 6, "exact", (0.6, 0.5), 3, kw, c=c, present=present)
    _stagewise(rd, X, queries, feats, "ndcg@10", 6, "histogram", (0.6, 0.5), 3, kw, c=c)


def test_30k_shape_sampled_trees_equal_restatement():
    """The 30K shape: three default-depth histogram trees at rates (0.5, 0.5) on the view of every tenth query equal the
    restatement's, and two sampled trees on all 3.8 M documents keep the training identities."""
    from tests.test_gpu_fullsize import _shape

    _, X, y, qid, g = _shape("30k")
    names = sorted(g.queries())
    sub = g.subsample_queries(names[::10])
    ids, fids, edges, bins = native.hist_bins(sub, 64)
    ids = ids.astype(np.int64)
    feats = [int(f) for f in fids]
    queries = np.split(ids, np.flatnonzero(np.diff(qid[ids]) != 0) + 1)
    assert len(queries) == len(names[::10]) and len(ids) > 300_000
    binned = hm.bin_matrix(X, ids, feats, 64)
    req = _request("ndcg@10", num_trees=3, split_candidates=64, query_sampling_rate=0.5, feature_sampling_rate=0.5, seed=30)
    trees = [m["DecisionTree"] for m in sub.train_model(req).to_dict()["Ensemble"]["models"]]
    st = native.last_train_stats()["lambdamart"]
    assert st["sample_features"] == 68 and st["sample_queries"] == len(queries) // 2
    for t in range(3):
        fsel, qsel = sm.sample(30, t, len(feats), len(queries), (0.5, 0.5))
        lam, wt = native.lambda_gradients(_ensemble(trees[:t], 0.1), sub, "ndcg@10", 1.0, n_total=X.shape[0])
        exp = sm.hist_tree(X, np.nan_to_num(lam), np.nan_to_num(wt), ids, feats, binned, sm.instance_rows(queries, qsel), fsel, 6, 10, 64)
        assert trees[t] == exp, "tree %d" % t
        assert _fids(trees[t]) <= set(feats[s] for s in fsel)
    full = _request("ndcg@10", num_trees=2, split_candidates=64, query_sampling_rate=0.5, feature_sampling_rate=0.5, seed=30)
    model = g.train_model(full)
    st = native.last_train_stats()["lambdamart"]
    _, per_q = native.evaluate_dense(model, g, "ndcg@10")
    o.set_mean_segment(o.DEVICE_MEAN_SEGMENT)
    try:
        assert st["train_measure"][-1] == o.mean(per_q)
    finally:
        o.set_mean_segment(0)
    assert st["train_measure"][1] > st["train_measure"][0]
    assert json.dumps(g.train_model(full).to_dict()) == json.dumps(model.to_dict())
