"""The Newton split gain of LambdaMART's histogram grower on the device against the numpy restatement
(tests/lambdamart_newton_model.py, DESIGN.md section 11, "Newton split gain"), bit for bit: one tree from given gradients,
the equal-hessian identity with the variance kernels, then training stage by stage."""
import json
import os

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import clib, native
from oracle import pyoracle as o
from tests import lambdamart_hist_model as hm
from tests import lambdamart_model as lm
from tests import lambdamart_newton_model as nm
from tests import lambdamart_sample_model as sm
from tests import lambdamart_valid_model as vm
from tests.conftest import GOLDEN, synth_dataset

pytestmark = pytest.mark.gpu

NEWTON_KEYS = {"split_gain", "lambda_l2", "min_sum_hessian", "min_split_gain"}
L2S = [0.0, 2.0 ** -10, 1.0]


def _request(measure="ndcg", **kw):
    req = fr.TrainRequest.lambdamart()
    req.measure = measure
    req.params.quiet = True
    req.params.grower = "histogram"
    for k, v in kw.items():
        setattr(req.params, k, v)
    return req


def _names(qid):
    _, first = np.unique(qid, return_index=True)
    return [str(int(qid[i])) for i in np.sort(first)]


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
    c = o.Dataset(X, y, qid)
    ids = np.concatenate(lm.query_lists(c))
    return X, y, qid, fr.CDataset.from_numpy(X, y, qid), c, ids, {}


@pytest.fixture(scope="module")
def big():
    """60 000 instances: eight workgroups per feature block add into the root's histogram (HIST_CHUNK is 8 192)."""
    X, y, qid = synth_dataset(19, 60000, 12, 300)
    c = o.Dataset(X, y, qid)
    ids = np.concatenate(lm.query_lists(c))
    return X, y, qid, fr.CDataset.from_numpy(X, y, qid), c, ids, {}


def _binned(case, k):
    X, ids, cache = case[0], case[5], case[6]
    if k not in cache:
        cache[k] = hm.bin_matrix(X, ids, list(range(X.shape[1])), k)
    return cache[k]


def _gradients(y, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0.0, 1.0, len(y)) + 0.5 * (y - y.mean()), rng.random(len(y))


def _one_tree(case, lam, wt, k, depth, min_leaf, **newton):
    X, g, ids = case[0], case[3], case[5]
    got = native.hist_tree(g, lam, wt, k, depth, min_leaf, split_gain="newton", **newton).to_dict()["DecisionTree"]
    exp = nm.fit_tree(X, lam, wt, ids, range(X.shape[1]), depth, min_leaf, k, _binned(case, k), **newton)
    assert got == exp, "k = %d, depth %d, min_leaf %d, %r" % (k, depth, min_leaf, newton)
    return got


def _depth(node):
    if "LeafNode" in node:
        return 1
    return 1 + max(_depth(node["FeatureSplit"]["lhs"]), _depth(node["FeatureSplit"]["rhs"]))


def _leaves(node):
    if "LeafNode" in node:
        return 1
    return _leaves(node["FeatureSplit"]["lhs"]) + _leaves(node["FeatureSplit"]["rhs"])


# --- one tree from given gradients ---------------------------------------------------------------

@pytest.mark.parametrize("k", [2, 16, 64, 256])
@pytest.mark.parametrize("depth,min_leaf", [(1, 1), (4, 1), (4, 400), (10, 1), (10, 25)])
def test_one_tree_equals_restatement(synth, k, depth, min_leaf):
    lam, wt = _gradients(synth[1], 100 * k + depth)
    for l2 in L2S:
        tree = _one_tree(synth, lam, wt, k, depth, min_leaf, lambda_l2=l2)
        assert _depth(tree) <= depth
        if depth > 1:
            assert "FeatureSplit" in tree


def test_min_sum_hessian_invalidates_some_candidates_of_the_root(synth):
    X, y, ids = synth[0], synth[1], synth[5]
    lam, wt = _gradients(y, 31)
    k = 64
    edges, xbin = _binned(synth, k)
    Q, S, W, Sw = nm.quantise_pair(lam[ids], wt[ids], len(ids))
    rows = np.arange(len(ids))
    free, _ = nm.candidates(xbin, edges, Q, W, rows, 1, S, Sw, 1.0, 0.0)
    low = np.concatenate([np.minimum(nm.hess(wL, Sw), nm.hess(int(W.sum()) - wL, Sw)) for _, _, _, wL, _, _ in free])
    floor = float(np.median(low))
    held, _ = nm.candidates(xbin, edges, Q, W, rows, 1, S, Sw, 1.0, floor)
    n_ok = sum(int(ok.sum()) for *_, ok, _ in held)
    assert 0 < n_ok < sum(int(ok.sum()) for *_, ok, _ in free)
    a = _one_tree(synth, lam, wt, k, 6, 1, lambda_l2=1.0, min_sum_hessian=floor)
    assert "FeatureSplit" in a and a != _one_tree(synth, lam, wt, k, 6, 1, lambda_l2=1.0)
    # a floor no child can reach: one leaf
    root_h = float(nm.hess(int(W.sum()), Sw))
    assert list(_one_tree(synth, lam, wt, k, 6, 1, lambda_l2=1.0, min_sum_hessian=root_h).keys()) == ["LeafNode"]


def test_min_split_gain_stops_nodes_below_the_root(synth):
    X, y, ids = synth[0], synth[1], synth[5]
    lam, wt = _gradients(y, 32)
    k, l2 = 16, 2.0 ** -10
    edges, xbin = _binned(synth, k)
    Q, S, W, Sw = nm.quantise_pair(lam[ids], wt[ids], len(ids))

    def gain(rows):
        best, node = nm.best_split(xbin, edges, Q, W, rows, 10, S, Sw, l2, 0.0)
        return float(np.float64(best[0]) - nm.term(node[1], node[2], S, Sw, l2)), best

    rows = np.arange(len(ids))
    g0, best = gain(rows)
    left = xbin[best[1]][rows] <= best[2]
    g1, g2 = gain(rows[left])[0], gain(rows[~left])[0]
    floor = (g1 + g2) / 2
    assert min(g1, g2) < floor < max(g1, g2) and floor < g0
    tree = _one_tree(synth, lam, wt, k, 5, 10, lambda_l2=l2, min_split_gain=floor)
    sides = [tree["FeatureSplit"]["lhs"], tree["FeatureSplit"]["rhs"]]
    assert sorted("LeafNode" in s for s in sides) == [False, True]
    assert _leaves(tree) < _leaves(_one_tree(synth, lam, wt, k, 5, 10, lambda_l2=l2))
    # the comparison is strict: a floor equal to the root's gain stops the root, the next smaller double does not
    assert list(_one_tree(synth, lam, wt, k, 5, 10, lambda_l2=l2, min_split_gain=g0).keys()) == ["LeafNode"]
    assert "FeatureSplit" in _one_tree(synth, lam, wt, k, 5, 10, lambda_l2=l2, min_split_gain=float(np.nextafter(g0, 0.0)))


def test_one_tree_special_gradients(synth):
    X, y, g, ids = synth[0], synth[1], synth[3], synth[5]
    n = len(y)
    rng = np.random.default_rng(8)
    lam, wt = _gradients(y, 33)
    for l2 in L2S:
        assert native.hist_tree(g, np.zeros(n), wt, 16, 4, 1, split_gain="newton", lambda_l2=l2).to_dict() == {"DecisionTree": {"LeafNode": 0.0}}
    # min_leaf_support larger than the tree's list: the root is not searched
    assert list(_one_tree(synth, lam, wt, 16, 4, n + 1, lambda_l2=1.0).keys()) == ["LeafNode"]
    # every w zero: no valid candidate without an L2 term (one leaf of 0.0), a tree on G alone with one
    assert _one_tree(synth, lam, np.zeros(n), 16, 4, 10) == {"LeafNode": 0.0}
    assert "FeatureSplit" in _one_tree(synth, lam, np.zeros(n), 16, 4, 10, lambda_l2=1.0)
    # w zero in whole bins of a feature, lambda_l2 = 0: the H + lambda_l2 > 0 rule decides at its low and its high edges
    wz = wt.copy()
    wz[(X[:, 0] <= np.quantile(X[:, 0], 0.3)) | (X[:, 2] >= np.quantile(X[:, 2], 0.6))] = 0.0
    for l2 in L2S:
        _one_tree(synth, lam, wz, 64, 6, 1, lambda_l2=l2)
    # every w zero but in one bin of feature 1
    vals, counts = np.unique(X[:, 1], return_counts=True)
    w1 = np.where(X[:, 1] == vals[counts.argmax()], wt, 0.0)
    assert w1.any() and not w1.all()
    _one_tree(synth, lam, w1, 64, 4, 1)
    # largest magnitudes powers of two
    lam2 = rng.integers(-8, 9, n) / 8.0
    lam2[5] = -4.0
    wt2 = rng.integers(0, 9, n) / 16.0
    wt2[11] = 0.5
    for l2 in L2S:
        _one_tree(synth, lam2, wt2, 16, 5, 10, lambda_l2=l2)
    # tiny magnitudes: G * G underflows to 0 for every candidate, no gain above 0 (one leaf); huge ones
    assert list(_one_tree(synth, lam * 1e-300, wt * 1e-12, 64, 4, 10).keys()) == ["LeafNode"]
    _one_tree(synth, lam * 1e100, wt * 1e100, 64, 4, 10, lambda_l2=1.0)
    # gradients equal inside every bin of every feature: ties between candidates, the last one wins
    _one_tree(synth, np.where(X[:, 1] > 2, 1.0, -1.0), np.ones(n), 64, 3, 1)


def _sampled_tree(case, lam, wt, k, depth, min_leaf, qsel, fids, **newton):
    X, g, c, ids = case[0], case[3], case[4], case[5]
    feats = list(range(X.shape[1]))
    got = native.hist_tree(g, lam, wt, k, depth, min_leaf, queries=qsel, features=fids, split_gain="newton", **newton).to_dict()["DecisionTree"]
    queries = lm.query_lists(c)
    rows = np.arange(len(ids)) if qsel is None else sm.instance_rows(queries, qsel)
    fsel = feats if fids is None else sorted(int(f) for f in fids)
    exp = nm.tree_on_sample(X, lam, wt, ids, feats, _binned(case, k), rows, fsel, depth, min_leaf, k, **newton)
    assert got == exp, "k = %d, depth %d, queries %r, features %r, %r" % (k, depth, None if qsel is None else len(qsel), fids, newton)
    return got


@pytest.mark.parametrize("ft", [1, 3, 4, 5, 7, 8, 9, 11])
def test_feature_sample_around_the_build_kernels_block(big, ft):
    """F_t one below, at and one above the build kernel's features per workgroup (8; 4 was the other candidate), and 1."""
    X, y = big[0], big[1]
    lam, wt = _gradients(y, 40 + ft)
    fids = sorted(np.random.default_rng(ft).permutation(X.shape[1])[:ft].tolist())
    _sampled_tree(big, lam, wt, 64, 5, 10, None, fids, lambda_l2=1.0, min_sum_hessian=2.0 ** -6)


def test_query_samples(synth):
    X, y, c = synth[0], synth[1], synth[4]
    lam, wt = _gradients(y, 50)
    nq = len(lm.query_lists(c))
    half = sorted(np.random.default_rng(2).permutation(nq)[:nq // 2].tolist())
    for l2 in L2S:
        _sampled_tree(synth, lam, wt, 64, 6, 5, half, None, lambda_l2=l2)
    _sampled_tree(synth, lam, wt, 16, 6, 5, half, [0, 2, 5, 8], lambda_l2=1.0, min_split_gain=2.0 ** -20)
    t = _sampled_tree(synth, lam, wt, 16, 4, 1, [7], None, lambda_l2=2.0 ** -10)  # a single query
    assert "FeatureSplit" in t
    assert list(_sampled_tree(synth, lam, wt, 16, 4, 1000, [7], None, lambda_l2=1.0).keys()) == ["LeafNode"]  # n_t < min_leaf_support
    # values outside the query sample are not read
    rows = sm.instance_rows(lm.query_lists(c), half)
    lam2, wt2 = np.full(len(y), np.nan), np.full(len(y), np.nan)
    lam2[synth[5][rows]], wt2[synth[5][rows]] = lam[synth[5][rows]], wt[synth[5][rows]]
    a = native.hist_tree(synth[3], lam2, wt2, 64, 6, 5, queries=half, split_gain="newton", lambda_l2=1.0).to_dict()
    assert a == native.hist_tree(synth[3], lam, wt, 64, 6, 5, queries=half, split_gain="newton", lambda_l2=1.0).to_dict()


def test_one_tree_with_many_workgroups_per_histogram(big):
    X, y, ids = big[0], big[1], big[5]
    rng = np.random.default_rng(4)
    lam = rng.normal(0.0, 1.0, len(y)) * np.exp(rng.normal(0.0, 3.0, len(y))) + 0.3 * (y - 1)
    wt = rng.random(len(y))
    assert len(ids) >= 60000
    _one_tree(big, lam, wt, 64, 10, 1, lambda_l2=2.0 ** -10)
    _one_tree(big, lam, wt, 256, 6, 10, lambda_l2=1.0, min_sum_hessian=2.0 ** -6, min_split_gain=2.0 ** -20)
    nq = len(lm.query_lists(big[4]))
    _sampled_tree(big, lam, wt, 64, 6, 10, list(range(0, nq, 2)) + [1], [0, 1, 2, 3, 4, 5, 6, 7, 9], lambda_l2=1.0)


# --- the equal-hessian identity on the device -----------------------------------------------------

def _identity(g, n, seed, cases):
    rng = np.random.default_rng(seed)
    lam = rng.normal(0.0, 1.0, n)
    wt = np.full(n, 0.25)
    for k, depth, min_leaf in cases:
        a = native.hist_tree(g, lam, wt, k, depth, min_leaf, split_gain="newton").to_dict()
        b = native.hist_tree(g, lam, wt, k, depth, min_leaf).to_dict()
        assert json.dumps(a) == json.dumps(b), "k = %d, depth %d, min_leaf %d" % (k, depth, min_leaf)
        assert "FeatureSplit" in a["DecisionTree"]


def test_equal_hessians_give_the_variance_kernels_tree_trec(trec):
    """w = 0.25 everywhere, lambda_l2 = 0: term is the variance term scaled by a power of two, so the new build, subtract
    and scan kernels must give what the ones already tested give, byte for byte."""
    X, y, qid, g, c = trec
    _identity(g, len(y), 1, [(2, 3, 1), (16, 6, 5), (64, 8, 5), (256, 5, 2)])


def test_equal_hessians_give_the_variance_kernels_tree_many_workgroups(big):
    _identity(big[3], len(big[1]), 2, [(64, 8, 10), (256, 6, 1)])
    nq = len(lm.query_lists(big[4]))
    lam, wt = np.random.default_rng(3).normal(0.0, 1.0, len(big[1])), np.full(len(big[1]), 0.25)
    kw = dict(queries=list(range(0, nq, 3)), features=[1, 2, 3, 5, 7, 8, 9, 10, 11])
    assert json.dumps(native.hist_tree(big[3], lam, wt, 64, 7, 10, split_gain="newton", **kw).to_dict()) == json.dumps(
        native.hist_tree(big[3], lam, wt, 64, 7, 10, **kw).to_dict())


# --- training ------------------------------------------------------------------------------------

NEWTON = dict(split_gain="newton", lambda_l2=1.0, min_sum_hessian=2.0 ** -6, min_split_gain=2.0 ** -20)


def _ensemble(trees, lr):
    return fr.CModel.from_dict({"Ensemble": {"weights": [lr] * len(trees), "models": [{"DecisionTree": x} for x in trees]}})


def _stagewise(g, c, X, qid, measure, T, params, rates=(1.0, 1.0), seed=0, held=(), rounds=0):
    """Every tree of the model equals the restatement's fit, on the restatement's sample, to the device's gradients of the
    prefix model; the running scores are `predict` of the model; the measures after every tree are the oracle's."""
    req = _request(measure, num_trees=T, query_sampling_rate=rates[0], feature_sampling_rate=rates[1], seed=seed,
                   validation_queries=list(held), early_stopping_rounds=rounds, **dict(NEWTON, **params))
    p = req.params
    model = g.train_model(req)
    st = native.last_train_stats()["lambdamart"]
    d = model.to_dict()
    trees = [m["DecisionTree"] for m in d["Ensemble"]["models"]]
    assert {k: st[k] for k in NEWTON_KEYS} == NEWTON and st["grower"] == "histogram"
    queries, names = lm.query_lists(c), _names(qid)
    order_ids = np.concatenate(queries)
    feats = list(range(X.shape[1]))
    binned = hm.bin_matrix(X, order_ids, feats, p.split_candidates)
    Tq, Hq = vm.split(names, held) if held else (np.arange(len(names)), np.zeros(0, dtype=np.int64))
    if held:
        best, trained, stopped, kept = vm.stopping(st["valid_measure"] + [0.0] * (T - len(st["valid_measure"])), rounds, T)
        assert (st["best_iteration"], st["trees"], st["stopped_early"], len(trees)) == (best, trained, stopped, kept)
    else:
        assert st["trees"] == T and len(trees) == T
    assert d["Ensemble"]["weights"] == [p.learning_rate] * len(trees)
    newton = {k: v for k, v in NEWTON.items() if k != "split_gain"}
    for t in range(len(trees)):
        fsel, qsel = vm.sample(seed, t, len(feats), Tq, rates)
        lam, wt = native.lambda_gradients(_ensemble(trees[:t], p.learning_rate), g, measure, p.sigma)
        exp = nm.tree_on_sample(X, lam, wt, order_ids, feats, binned, sm.instance_rows(queries, qsel), fsel, p.max_depth,
                                p.min_leaf_support, p.split_candidates, **newton)
        assert trees[t] == exp, "tree %d differs from the restatement's fit" % t
        exp_q, _ = c.metric_from_scores(measure, c.score_ensemble(trees[:t + 1], [p.learning_rate] * (t + 1)))
        if held:
            assert st["train_measure"][t] == vm.subset_mean(exp_q, Tq) and st["valid_measure"][t] == vm.subset_mean(exp_q, Hq)
        else:
            assert st["train_measure"][t] == o.mean(exp_q)
    assert np.array_equal(native.predict_scores_dense(model, g), c.score_ensemble(trees, d["Ensemble"]["weights"]))
    return model, st, trees


MODES = ["plain", "sampled", "held_out"]


def _mode(mode, names):
    if mode == "sampled":
        return dict(rates=(0.5, 0.5), seed=1)
    if mode == "held_out":
        return dict(held=names[3::10], rounds=3)
    return dict()


@pytest.mark.parametrize("mode", MODES)
def test_stagewise_identity_trec(trec, mode):
    X, y, qid, g, c = trec
    _, st, trees = _stagewise(g, c, X, qid, "ndcg@10", 20, dict(max_depth=5, min_leaf_support=5, split_candidates=16), **_mode(mode, _names(qid)))
    assert any("FeatureSplit" in t for t in trees)


@pytest.mark.parametrize("mode", MODES)
def test_stagewise_identity_synthetic(synth, mode):
    X, y, qid, g, c = synth[:5]
    _, st, trees = _stagewise(g, c, X, qid, "ndcg", 20, dict(max_depth=6, min_leaf_support=10, split_candidates=64), **_mode(mode, _names(qid)))
    assert any("FeatureSplit" in t for t in trees)
    if mode == "plain":
        assert st["train_measure"][-1] > st["train_measure"][0]


def test_deterministic(trec):
    X, y, qid, g, c = trec
    req = _request("ndcg@10", num_trees=6, max_depth=5, min_leaf_support=5, split_candidates=16, **NEWTON)
    a = json.dumps(g.train_model(req).to_dict())
    assert a == json.dumps(g.train_model(req).to_dict())
    assert a == json.dumps(fr.CDataset.from_numpy(X, y, qid).train_model(req).to_dict())


def test_variance_spelled_out_is_the_request_without_the_key_and_bins_are_shared(trec):
    X, y, qid, g, c = trec
    g = fr.CDataset.from_numpy(X, y, qid)  # (a dataset of its own: no bins yet)
    kw = dict(num_trees=5, max_depth=4, min_leaf_support=5, split_candidates=16)
    absent = _request("ndcg@10", **kw)
    assert not NEWTON_KEYS & set(absent.to_dict()["params"]["LambdaMART"])
    a = json.dumps(g.train_model(absent).to_dict())
    st = native.last_train_stats()["lambdamart"]
    assert st["bins_ms"] > 0.0 and not NEWTON_KEYS & set(st)
    wire = absent.to_dict()
    wire["params"]["LambdaMART"].update(split_gain="variance", lambda_l2=0.0, min_sum_hessian=0.0, min_split_gain=0.0)
    m = fr.CModel(clib._unwrap(clib._load().train_model(json.dumps(wire).encode(), g.pointer)))
    assert json.dumps(m.to_dict()) == a
    assert not NEWTON_KEYS & set(native.last_train_stats()["lambdamart"])
    # the same view's bins serve a Newton training, and a variance training after it is what it was
    newton = json.dumps(g.train_model(_request("ndcg@10", **dict(kw, **NEWTON))).to_dict())
    st = native.last_train_stats()["lambdamart"]
    assert st["bins_ms"] == 0.0 and st["split_gain"] == "newton" and newton != a
    assert json.dumps(g.train_model(absent).to_dict()) == a
    assert native.last_train_stats()["lambdamart"]["bins_ms"] == 0.0
