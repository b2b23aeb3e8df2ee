"""LambdaMART's symmetric trees on the device against the numpy restatement (tests/lambdamart_symmetric_model.py, DESIGN.md
section 11, "Symmetric trees"): one tree from given gradients, then training stage by stage, alone and composed with the keys
that sit upstream of the grower.  Every tree must equal the restatement's bit for bit."""
import json
import os

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import native
from oracle import pyoracle as o
from tests import lambdamart_composed_model as cmod
from tests import lambdamart_dart_model as dm
from tests import lambdamart_goss_model as gm
from tests import lambdamart_hist_model as hm
from tests import lambdamart_model as lm
from tests import lambdamart_newton_model as nm
from tests import lambdamart_sample_model as sm
from tests import lambdamart_symmetric_model as sy
from tests import lambdamart_xendcg_model as xm
from tests.conftest import GOLDEN, synth_dataset
from tests.test_lambdamart_symmetric_host import assert_symmetric, level_splits

pytestmark = pytest.mark.gpu

EMPTY = {"Ensemble": {"weights": [], "models": []}}
VARIANCE = dict()
NEWTON = dict(split_gain="newton", lambda_l2=0.5, min_sum_hessian=2.0 ** -6, min_split_gain=2.0 ** -10)
GAINS = {"variance": VARIANCE, "newton": NEWTON}
SYM_STATS = {"symmetric_trees", "levels"}


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


@pytest.fixture(scope="module")
def synth_binned(synth):
    """(edges, bins) of the synthetic set's full lists per k: made once, shared, never changed."""
    X, y, qid, g, c = synth
    ids = np.concatenate(lm.query_lists(c))
    return {k: hm.bin_matrix(X, ids, list(range(X.shape[1])), k) for k in (2, 64, 256)}


def _gradients(y, seed):
    rng = np.random.default_rng(seed)
    lam = rng.normal(0.0, 1.0, len(y)) + 0.5 * (y - y.mean())
    return lam, rng.random(len(y)) + 2.0 ** -8


def _one_tree(g, X, order_ids, lam, wt, k, depth, min_leaf, gain, binned=None, feats=None):
    """The device's symmetric tree for given gradients = the restatement's; returns (tree, levels that split, the most open
    nodes of a level searched)."""
    all_feats = list(range(X.shape[1]))
    levels, opened = [], []
    if feats is None:
        exp = sy.fit_tree(X, lam, wt, order_ids, all_feats, depth, min_leaf, k, binned, levels_out=levels, open_out=opened, **gain)
    else:
        binned = hm.bin_matrix(X, order_ids, all_feats, k) if binned is None else binned
        exp = sy.tree_on_sample(X, lam, wt, order_ids, all_feats, binned, np.arange(len(order_ids)), [all_feats.index(f) for f in feats],
                                depth, min_leaf, k, levels_out=levels, open_out=opened, **gain)
    got = native.hist_tree(g, lam, wt, k, depth, min_leaf, features=feats, symmetric=True, **gain).to_dict()["DecisionTree"]
    assert got == exp, "k = %d, depth %d, min_leaf %d, %s" % (k, depth, min_leaf, gain.get("split_gain", "variance"))
    assert assert_symmetric(got) == levels[0] <= max(depth - 1, 0)
    return got, levels[0], max(opened, default=0)


# --- one tree from given gradients ---------------------------------------------------------------

@pytest.mark.parametrize("gain", list(GAINS))
@pytest.mark.parametrize("k", [2, 64, 256])
@pytest.mark.parametrize("depth,min_leaf", [(1, 1), (4, 1), (4, 400), (10, 1), (10, 25)])
def test_one_tree_equals_restatement(synth, synth_binned, gain, k, depth, min_leaf):
    X, y, qid, g, c = synth
    lam, wt = _gradients(y, 100 * k + depth)
    tree, levels, opened = _one_tree(g, X, np.concatenate(lm.query_lists(c)), lam, wt, k, depth, min_leaf, GAINS[gain], synth_binned[k])
    if depth > 1:
        assert "FeatureSplit" in tree
    if depth == 10 and min_leaf == 1 and k == 2:  # levels wider than the scan kernel's node tile, and than two of them
        assert opened >= 33 and levels == 9


@pytest.mark.parametrize("gain", list(GAINS))
def test_the_root_and_depth_one_are_the_plain_growers(synth, synth_binned, gain):
    X, y, qid, g, c = synth
    lam, wt = _gradients(y, 5)
    ids = np.concatenate(lm.query_lists(c))
    numbers = {key: v for key, v in GAINS[gain].items() if key != "split_gain"}
    for depth in (1, 2):
        got, _, _ = _one_tree(g, X, ids, lam, wt, 64, depth, 10, GAINS[gain], synth_binned[64])
        plain = native.hist_tree(g, lam, wt, 64, depth, 10, **GAINS[gain]).to_dict()["DecisionTree"]
        exp = (nm if gain == "newton" else hm).fit_tree(X, lam, wt, ids, range(X.shape[1]), depth, 10, 64, synth_binned[64], **numbers)
        assert json.dumps(got) == json.dumps(plain) == json.dumps(exp)


@pytest.mark.parametrize("gain", list(GAINS))
@pytest.mark.parametrize("feats", [[4], [0, 3, 9], [0, 1, 2, 3, 4, 5, 6, 7, 8]], ids=["1", "3", "9"])
def test_one_tree_on_a_feature_list(synth, synth_binned, gain, feats):
    X, y, qid, g, c = synth
    lam, wt = _gradients(y, len(feats))
    tree = _one_tree(g, X, np.concatenate(lm.query_lists(c)), lam, wt, 64, 6, 10, GAINS[gain], synth_binned[64], feats=feats)[0]
    used = {fid for lvl in level_splits(tree)[0] for fid, _ in lvl}
    assert used and used <= set(feats) - {9}


@pytest.mark.parametrize("gain", list(GAINS))
def test_one_tree_special_gradients(synth, synth_binned, gain):
    X, y, qid, g, c = synth
    n = len(y)
    ids = np.concatenate(lm.query_lists(c))
    rng = np.random.default_rng(8)
    wt = rng.random(n)
    kw = GAINS[gain]
    assert native.hist_tree(g, np.zeros(n), wt, 64, 4, 1, symmetric=True, **kw).to_dict() == {"DecisionTree": {"LeafNode": 0.0}}
    lam = rng.integers(-8, 9, n) / 8.0
    lam[5] = -4.0
    _one_tree(g, X, ids, lam, wt, 64, 5, 10, kw, synth_binned[64])
    # every weight zero; documents without gradient or weight in whole bins (an open node whose sums are all zero)
    _one_tree(g, X, ids, lam, np.zeros(n), 64, 4, 10, kw, synth_binned[64])
    dead = X[:, 1] > 2
    _one_tree(g, X, ids, np.where(dead, 0.0, lam), np.where(dead, 0.0, wt), 64, 6, 1, kw, synth_binned[64])
    _one_tree(g, X, ids, lam * 1e-300, wt * 1e-12, 64, 4, 10, kw, synth_binned[64])
    _one_tree(g, X, ids, lam * 1e200, wt * 1e100, 64, 4, 10, kw, synth_binned[64])
    # gradients equal inside every bin of every feature: ties between candidates, the last one wins
    _one_tree(g, X, ids, np.where(X[:, 1] > 2, 1.0, -1.0), np.ones(n), 64, 4, 1, kw, synth_binned[64])


def _additive_gradients(X, seed):
    """Gradients that follow several features at once, each through its median: one split pays off in every node of a level,
    so the levels stay full and grow wide."""
    rng = np.random.default_rng(seed)
    lam = sum((1.0 + f / 16.0) * np.where(X[:, f] > np.median(X[:, f]), 1.0, -1.0) for f in (0, 2, 4, 5, 6, 7))
    return lam + rng.normal(0.0, 0.05, len(X)), rng.random(len(X)) + 0.5


@pytest.mark.parametrize("gain", list(GAINS))
@pytest.mark.parametrize("k", [64, 256])
def test_a_level_wider_than_two_node_tiles(synth, synth_binned, gain, k):
    """33 or more open nodes in one level: the scan kernel's LDS tile of nodes is refilled, at one and at four bins per lane."""
    X, y, qid, g, c = synth
    lam, wt = _additive_gradients(X, k)
    tree, levels, opened = _one_tree(g, X, np.concatenate(lm.query_lists(c)), lam, wt, k, 8, 1, GAINS[gain], synth_binned[k])
    assert opened >= 33 and levels == 7


def test_the_newton_numbers_bind_and_a_floor_refuses_the_root(synth, synth_binned):
    X, y, qid, g, c = synth
    lam, wt = _gradients(y, 33)
    ids = np.concatenate(lm.query_lists(c))
    base = dict(split_gain="newton", lambda_l2=0.0, min_sum_hessian=0.0, min_split_gain=0.0)
    free = _one_tree(g, X, ids, lam, wt, 64, 6, 1, base, synth_binned[64])[0]
    for key, value in (("lambda_l2", 64.0), ("min_sum_hessian", 40.0), ("min_split_gain", 2.0)):
        bound = _one_tree(g, X, ids, lam, wt, 64, 6, 1, dict(base, **{key: value}), synth_binned[64])[0]
        assert bound != free and "FeatureSplit" in bound, key
    for key, value in (("min_split_gain", 1e30), ("min_sum_hessian", 1e30)):
        tree, levels, _ = _one_tree(g, X, ids, lam, wt, 64, 6, 1, dict(base, **{key: value}), synth_binned[64])
        assert list(tree) == ["LeafNode"] and tree["LeafNode"] != 0.0 and levels == 0


@pytest.mark.parametrize("gain", list(GAINS))
def test_one_tree_over_sixty_thousand_instances(gain):
    X, y, qid = synth_dataset(19, 60000, 12, 300)
    g, c = fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)
    rng = np.random.default_rng(4)
    lam = rng.normal(0.0, 1.0, len(y)) * np.exp(rng.normal(0.0, 3.0, len(y))) + 0.3 * (y - 1)
    wt = rng.random(len(y))
    tree, levels, _ = _one_tree(g, X, np.concatenate(lm.query_lists(c)), lam, wt, 256, 7, 10, GAINS[gain])
    assert levels == 6


# --- training ------------------------------------------------------------------------------------

def _ensemble(trees, weights):
    if not trees:
        return fr.CModel.from_dict(EMPTY)
    return fr.CModel.from_dict({"Ensemble": {"weights": [float(w) for w in weights], "models": [{"DecisionTree": x} for x in trees]}})


def _trees(model):
    return [m["DecisionTree"] for m in model.to_dict()["Ensemble"]["models"]]


def _stagewise(g, c, X, y, measure, params, names=None, symmetric=True):
    """Trains and holds every stage to the restatements: tree t is the symmetric restatement's fit (symmetric = False: the
    plain restatements') to the DEVICE's gradients of the ensemble the tree is fitted to (the prefix; under DART without the
    dropped trees), over the tree's query and feature sample (under GOSS: over the GOSS list, amplified); the running measures
    are the oracle's of the oracle's ensemble scores, the prediction is the oracle's."""
    params = dict(params, symmetric_trees=True) if symmetric else dict(params)
    req = cmod._request(measure, "histogram", **params)
    p = req.params
    cm = cmod.Composed(X, y, c, measure, dict(fr.LambdaMARTParams().to_dict(), **dict(params, grower="histogram")), names=names)
    model = g.train_model(req)
    st = native.last_train_stats()["lambdamart"]
    d = model.to_dict()
    got = _trees(model)
    T = st["trees"]
    trees = got
    if p.early_stopping_rounds > 0:  # the trees the stats speak of: those of a run without the rule
        free = {k: v for k, v in params.items() if k != "early_stopping_rounds"}
        trees = _trees(g.train_model(cmod._request(measure, "histogram", **dict(free, num_trees=T))))
        assert len(trees) == T and got == trees[:st["best_iteration"]]
        best, n_trained, stopped, kept = cm.stopping(st["valid_measure"])
        assert (st["best_iteration"], T, st["stopped_early"], len(got)) == (best, n_trained, stopped, kept)
    else:
        assert len(got) == T == p.num_trees
    if symmetric:
        assert SYM_STATS <= set(st) and st["symmetric_trees"] is True and len(st["levels"]) == T
    else:
        assert not (SYM_STATS & set(st))
    goss = p.goss_top_rate > 0.0
    keys, xkeys = gm.keys(p.seed, T), xm.keys(p.seed, T)
    plan = dm.plan(p.seed, p.drop_rate, p.max_drop, p.skip_drop, T, p.learning_rate) if p.drop_rate > 0 else None
    if plan is not None:
        assert st["dropped"] == [len(D) for D, _, _ in plan] and any(st["dropped"])
        assert np.asarray(d["Ensemble"]["weights"], dtype=np.float64).tobytes() == plan[-1][2].tobytes()
    else:
        assert d["Ensemble"]["weights"] == [p.learning_rate] * len(got)
    gain = dict(split_gain=p.split_gain, **cm.newton())
    for t in range(T):
        fsel, qsel = cm.sample(t)
        if plan is not None:
            D, before, after = plan[t]
            keep = dm.kept(t, D)
            fitted_to = _ensemble([trees[i] for i in keep], before[keep])
        else:
            after = [p.learning_rate] * (t + 1)
            fitted_to = _ensemble(trees[:t], after[:t])
        lam, wt = native.lambda_gradients(fitted_to, g, measure, p.sigma, queries=qsel if cm.subset(qsel) else None,
                                          truncation_level=p.truncation_level, lambda_norm=p.lambda_norm, objective=p.objective,
                                          xe_key=xkeys[t])
        lam, wt = np.nan_to_num(lam), np.nan_to_num(wt)
        rows = sm.instance_rows(cm.queries, qsel)
        if not symmetric:
            exp = cm.tree(lam, wt, fsel, qsel)
        else:
            if goss:
                rows, top, _, amp = gm.goss_list(lam, rows, cm.order_ids, p.goss_top_rate, p.goss_other_rate, keys[t])
                lam, wt = gm.amplified(lam, wt, cm.order_ids, rows, top, amp)
                assert st["goss_instances"][t] == len(rows)
            levels = []
            exp = sy.tree_on_sample(X, lam, wt, cm.order_ids, cm.feats, cm.binned, rows, list(fsel), p.max_depth, p.min_leaf_support,
                                    p.split_candidates, levels_out=levels, **gain)
            assert st["levels"][t] == levels[0] == assert_symmetric(trees[t]), "tree %d" % t
        assert trees[t] == exp, "tree %d differs from the restatement's fit" % t
        tr, va, err = cm.measures(c.score_ensemble(trees[:t + 1], after))
        assert err == 0
        assert st["train_measure"][t] == tr, "train_measure[%d]" % t
        if va is not None:
            assert st["valid_measure"][t] == va, "valid_measure[%d]" % t
    assert np.array_equal(native.predict_scores_dense(model, g), c.score_ensemble(got, d["Ensemble"]["weights"]))
    assert any("FeatureSplit" in t for t in trees)
    return model, st


def _shape(data):
    if data == "trec":
        return dict(max_depth=5, min_leaf_support=5, split_candidates=16)
    return dict(max_depth=6, min_leaf_support=10, split_candidates=64)


@pytest.mark.parametrize("gain", list(GAINS))
@pytest.mark.parametrize("data", ["trec", "synth"])
def test_stagewise_identity(request, data, gain):
    X, y, qid, g, c = request.getfixturevalue(data)
    kw = dict(num_trees=10, **_shape(data), **GAINS[gain])
    model, st = _stagewise(g, c, X, y, "ndcg@10", kw)
    assert max(st["levels"]) >= 3
    # deterministic; and the key reaches the grower: the plain request gives other trees
    assert json.dumps(g.train_model(cmod._request("ndcg@10", "histogram", symmetric_trees=True, **kw)).to_dict()) == json.dumps(model.to_dict())
    assert json.dumps(g.train_model(cmod._request("ndcg@10", "histogram", **kw)).to_dict()) != json.dumps(model.to_dict())


SMALL = dict(num_trees=6, seed=3, max_depth=5, min_leaf_support=5, split_candidates=16)


@pytest.mark.parametrize("extra", [
    dict(query_sampling_rate=0.5, feature_sampling_rate=0.5),
    dict(validation_queries="every fifth", early_stopping_rounds=2, num_trees=12, learning_rate=0.5, **NEWTON),
    dict(truncation_level=3),
    dict(objective="map", **NEWTON),
    dict(objective="xendcg"),
    dict(drop_rate=0.5, skip_drop=0.25, max_drop=3),
    dict(goss_top_rate=0.2, goss_other_rate=0.1, **NEWTON),
], ids=["samples", "holdout+stopping", "truncation", "map", "xendcg", "dart", "goss"])
def test_symmetric_trees_compose_with_the_other_keys(synth, extra):
    X, y, qid, g, c = synth
    names = cmod._names(qid)
    extra = dict(extra)
    if extra.get("validation_queries"):
        extra["validation_queries"] = names[::5]
    _stagewise(g, c, X, y, "ndcg@10", dict(SMALL, **extra), names=names)


@pytest.mark.parametrize("gain", list(GAINS))
def test_without_the_key_the_request_is_the_plain_one(synth, gain):
    X, y, qid, g, c = synth
    kw = dict(num_trees=5, max_depth=5, min_leaf_support=10, split_candidates=16, **GAINS[gain])
    absent = cmod._request("ndcg@7", "histogram", **kw)
    spelled = cmod._request("ndcg@7", "histogram", symmetric_trees=False, **kw)
    assert "symmetric_trees" not in absent.to_dict()["params"]["LambdaMART"] and absent.to_dict() == spelled.to_dict()
    a = json.dumps(g.train_model(absent).to_dict())
    wire = absent.to_dict()
    wire["params"]["LambdaMART"]["symmetric_trees"] = False  # (the key on the wire, as another client may send it)
    from fastrank_amd import clib
    m = fr.CModel(clib._unwrap(clib._load().train_model(json.dumps(wire).encode(), g.pointer)))
    assert json.dumps(m.to_dict()) == a
    assert not (SYM_STATS & set(native.last_train_stats()["lambdamart"]))
    # ... and what both give is the plain restatements' model, stage by stage, as before
    model, _ = _stagewise(g, c, X, y, "ndcg@7", kw, symmetric=False)
    assert json.dumps(model.to_dict()) == a


def test_explanation_of_a_symmetric_model(trec):
    from tests.test_gpu_explain import _check, _some_rows

    X, y, qid, g, c = trec
    model = g.train_model(cmod._request("ndcg@10", "histogram", symmetric_trees=True, num_trees=10, max_depth=6, min_leaf_support=5,
                                        split_candidates=16))
    trees = _trees(model)
    assert len(trees) == 10 and max(assert_symmetric(t) for t in trees) >= 3
    _check(model, g, X, rows=_some_rows(len(X)))
