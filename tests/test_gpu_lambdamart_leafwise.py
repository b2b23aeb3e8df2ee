"""Leaf-wise growth of LambdaMART's histogram grower on the device against the numpy restatement
(tests/lambdamart_leafwise_model.py, DESIGN.md section 11, "Leaf-wise growth"), bit for bit: one tree from given gradients
under both split gains, the level-wise identity, then training stage by stage."""
import json
import os

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import native
from oracle import pyoracle as o
from tests import lambdamart_hist_model as hm
from tests import lambdamart_leafwise_model as lw
from tests import lambdamart_model as lm
from tests import lambdamart_newton_model as nm
from tests import lambdamart_sample_model as sm
from tests import lambdamart_valid_model as vm
from tests.conftest import GOLDEN, synth_dataset

pytestmark = pytest.mark.gpu

NEWTON = dict(split_gain="newton", lambda_l2=2.0 ** -10, min_sum_hessian=2.0 ** -6, min_split_gain=2.0 ** -20)
GAINS = {"variance": dict(), "newton": NEWTON}


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


def _case(X, y, qid):
    c = o.Dataset(X, y, qid)
    return X, y, qid, fr.CDataset.from_numpy(X, y, qid), c, np.concatenate(lm.query_lists(c)), {}


@pytest.fixture(scope="module")
def trec():
    d = np.load(os.path.join(GOLDEN, "trec_news_2018.npz"))
    return _case(d["train_X"], d["train_y"], d["train_qid"])


@pytest.fixture(scope="module")
def synth():
    X, y, qid = synth_dataset(7, 5000, 10, 50)
    X = X.copy()
    X[::7, 3] = -0.0  # signed zeros in a sparse column
    X[:, 9] = 2.5     # a constant column: no edge, never split on
    return _case(X, y, qid)


@pytest.fixture(scope="module")
def small():
    return _case(*synth_dataset(23, 2000, 8, 40))


@pytest.fixture(scope="module")
def thousand():
    return _case(*synth_dataset(29, 1000, 6, 20))


@pytest.fixture(scope="module")
def big():
    """60 000 instances: eight workgroups per feature block add into a histogram (HIST_CHUNK is 8 192), and the partition of
    the root's stretch takes 235 workgroups."""
    return _case(*synth_dataset(19, 60000, 8, 300))


def _binned(case, k):
    X, ids, cache = case[0], case[5], case[6]
    if k not in cache:
        cache[k] = hm.bin_matrix(X, ids, list(range(X.shape[1])), k)
    return cache[k]


def _gradients(y, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0.0, 1.0, len(y)) + 0.5 * (y - y.mean()), rng.random(len(y))


def _level_tree(case, lam, wt, k, depth, min_leaf, gain):
    X, ids = case[0], case[5]
    if gain:
        newton = {key: v for key, v in gain.items() if key != "split_gain"}
        return nm.fit_tree(X, lam, wt, ids, range(X.shape[1]), depth, min_leaf, k, _binned(case, k), **newton)
    return hm.fit_tree(X, lam, wt, ids, range(X.shape[1]), depth, min_leaf, k, _binned(case, k))


def _one_tree(case, lam, wt, k, depth, min_leaf, max_leaves, gain):
    X, g, ids = case[0], case[3], case[5]
    got = native.hist_tree(g, lam, wt, k, depth, min_leaf, max_leaves=max_leaves, **gain).to_dict()["DecisionTree"]
    exp = lw.fit_tree(X, lam, wt, ids, range(X.shape[1]), depth, min_leaf, k, max_leaves, _binned(case, k), **gain)
    assert got == exp, "k = %d, depth %d, min_leaf %d, max_leaves %d, %r" % (k, depth, min_leaf, max_leaves, gain)
    assert lw.n_leaves(got) <= max_leaves and lw.depth(got) <= depth
    return got


# --- one tree from given gradients ---------------------------------------------------------------

@pytest.mark.parametrize("gain", sorted(GAINS))
@pytest.mark.parametrize("k", [2, 64, 256])
def test_budget_binds_in_the_middle_of_a_level(small, k, gain):
    """The leaf count is the restatement's and within the budget, where the level-wise tree of the same depth has more
    leaves than the budget (without leaf-wise growth the key would be ignored and that tree returned)."""
    lam, wt = _gradients(small[1], 7 * k)
    level = _level_tree(small, lam, wt, k, 12, 1, GAINS[gain])
    assert lw.n_leaves(level) > 5
    if k > 2:
        assert lw.n_leaves(level) > 31
    for max_leaves in (2, 3, 5, 31):
        tree = _one_tree(small, lam, wt, k, 12, 1, max_leaves, GAINS[gain])
        if k > 2:
            assert lw.n_leaves(tree) == max_leaves
        assert tree != level


@pytest.mark.parametrize("gain", sorted(GAINS))
def test_budget_binds_through_train_model(small, gain):
    X, y, qid, g, c = small[:5]
    _, st, trees = _stagewise(small, "ndcg", 2, dict(max_depth=12, min_leaf_support=1, split_candidates=64, max_leaves=5, **GAINS[gain]))
    assert [lw.n_leaves(t) for t in trees] == [5, 5] and st["mean_leaves"] == 5.0
    assert st["pool_bytes"] == 5 * 8 * 64 * (20 if gain == "newton" else 12)
    level = g.train_model(_request("ndcg", num_trees=1, max_depth=12, min_leaf_support=1, split_candidates=64, **GAINS[gain]))
    assert lw.n_leaves(level.to_dict()["Ensemble"]["models"][0]["DecisionTree"]) > 5
    assert "max_leaves" not in native.last_train_stats()["lambdamart"] and "mean_leaves" not in native.last_train_stats()["lambdamart"]


@pytest.mark.parametrize("gain", sorted(GAINS))
def test_chain(gain):
    """One side carries all the gain: 16 groups of feature 0 whose gradients grow threefold from group to group, and no
    feature varies inside a group.  The tree peels one group off per split, so the larger child takes over its parent's
    histogram and the smaller one is built, 15 times in a row."""
    rng = np.random.default_rng(12)
    n, groups = 4000, 16
    grp = np.repeat(np.arange(groups), n // groups)
    X = np.stack([grp, grp % 4, grp // 4, grp // 2], axis=1).astype(np.float32)
    lam = 3.0 ** grp * (1.0 + 0.01 * rng.normal(0.0, 1.0, n))
    wt = rng.random(n) + 0.5
    perm = rng.permutation(n)
    X, lam, wt = X[perm], lam[perm], wt[perm]
    case = _case(X, np.zeros(n), np.repeat(np.arange(1, 41), n // 40))
    tree = _one_tree(case, lam, wt, 64, 16, 1, 16, GAINS[gain])
    assert lw.n_leaves(tree) == 16 and lw.depth(tree) == 16
    node, splits = tree, 0
    while "FeatureSplit" in node:
        sides = [node["FeatureSplit"]["lhs"], node["FeatureSplit"]["rhs"]]
        assert any("LeafNode" in s for s in sides)
        node, splits = sides[0] if "FeatureSplit" in sides[0] else sides[1], splits + 1
    assert splits == 15


@pytest.mark.parametrize("gain", sorted(GAINS))
def test_equal_gains_split_the_lhs(gain):
    X, lam, wt = lw.mirrored_halves(3, 256)
    case = _case(X, np.zeros(512), np.repeat(np.arange(1, 9), 64))
    trace = []
    lw.fit_tree(X, lam, wt, case[5], [0, 1], 6, 1, 16, 3, trace=trace, **GAINS[gain])
    assert [i for i, _ in trace[1]["open"]] == [1, 2] and trace[1]["open"][0][1]["gain"] == trace[1]["open"][1][1]["gain"]
    tree = _one_tree(case, lam, wt, 16, 6, 1, 3, GAINS[gain])
    assert "FeatureSplit" in tree["FeatureSplit"]["lhs"] and "LeafNode" in tree["FeatureSplit"]["rhs"]
    _one_tree(case, lam, wt, 16, 6, 1, 4, GAINS[gain])


def test_equal_gains_with_identical_histograms_split_the_lhs():
    X, lam, wt = lw.copied_halves(4, 256)
    case = _case(X, np.zeros(512), np.repeat(np.arange(1, 9), 64))
    tree = _one_tree(case, lam, wt, 16, 6, 1, 3, dict())
    assert tree["FeatureSplit"]["fid"] == 1
    assert "FeatureSplit" in tree["FeatureSplit"]["lhs"] and "LeafNode" in tree["FeatureSplit"]["rhs"]


@pytest.mark.parametrize("gain", sorted(GAINS))
@pytest.mark.parametrize("nf", [3, 70])
def test_identical_columns_the_later_feature_wins(gain, nf):
    """Every feature gives the same record: the pick over the features must keep the last one (70 features: more than one per
    lane of the picking wave)."""
    rng = np.random.default_rng(9)
    col = rng.integers(0, 20, 512).astype(np.float32)
    X = np.repeat(col[:, None], nf, axis=1)
    lam, wt = rng.normal(0.0, 1.0, 512) + 0.2 * col, rng.random(512) + 0.5
    case = _case(X, np.zeros(512), np.repeat(np.arange(1, 9), 64))
    tree = _one_tree(case, lam, wt, 64, 8, 5, 7, GAINS[gain])

    def fids(node):
        return [] if "LeafNode" in node else [node["FeatureSplit"]["fid"]] + fids(node["FeatureSplit"]["lhs"]) + fids(node["FeatureSplit"]["rhs"])

    assert fids(tree) == [nf - 1] * 6


def test_children_that_are_not_enterable(thousand):
    X, y, g = thousand[0], thousand[1], thousand[3]
    n = len(y)
    lam, wt = _gradients(y, 61)
    for gain in GAINS.values():
        # most children are below min_leaf_support: they get no histogram and no scan
        t = _one_tree(thousand, lam, wt, 64, 12, 300, 64, gain)
        assert 2 <= lw.n_leaves(t) <= 3
        _one_tree(thousand, lam, wt, 64, 12, 120, 64, gain)
        # a budget nothing can reach: min_leaf_support bounds the leaves, then max_depth does
        t = _one_tree(thousand, lam, wt, 16, 12, 50, 255, gain)
        assert lw.n_leaves(t) <= n // 50
        assert _one_tree(thousand, lam, wt, 16, 3, 1, 255, gain) == _level_tree(thousand, lam, wt, 16, 3, 1, gain)
        assert list(_one_tree(thousand, lam, wt, 16, 12, n + 1, 8, gain).keys()) == ["LeafNode"]  # the root is not searched
        assert list(_one_tree(thousand, lam, wt, 16, 1, 1, 8, gain).keys()) == ["LeafNode"]
        assert native.hist_tree(g, np.zeros(n), wt, 16, 6, 1, max_leaves=8, **gain).to_dict() == {"DecisionTree": {"LeafNode": 0.0}}
    # every w zero under the Newton gain without an L2 term: no valid candidate, one leaf of 0.0; a tree with one
    assert _one_tree(thousand, lam, np.zeros(n), 16, 6, 10, 8, dict(split_gain="newton")) == {"LeafNode": 0.0}
    assert "FeatureSplit" in _one_tree(thousand, lam, np.zeros(n), 16, 6, 10, 8, dict(split_gain="newton", lambda_l2=1.0))
    _one_tree(thousand, lam, np.zeros(n), 16, 6, 10, 8, dict())


@pytest.mark.parametrize("gain", sorted(GAINS))
@pytest.mark.parametrize("depth,min_leaf", [(1, 1), (6, 1001)])
def test_a_root_that_is_not_searched_as_the_first_tree_of_a_dataset(thousand, gain, depth, min_leaf):
    """The single leaf's sums run over the device's index list, which no earlier tree of this dataset object has made."""
    X, y, qid = thousand[:3]
    lam, wt = _gradients(y, 71)
    fresh = _case(X, y, qid)
    tree = _one_tree(fresh, lam, wt, 16, depth, min_leaf, 2, GAINS[gain])
    assert list(tree.keys()) == ["LeafNode"] and tree["LeafNode"] != 0.0
    # ... and after a tree on one query sample the single leaf of another sample is summed over its own instances
    queries = lm.query_lists(fresh[4])
    a, b = list(range(0, len(queries), 2)), list(range(1, len(queries), 3))
    feats = list(range(X.shape[1]))
    native.hist_tree(fresh[3], lam, wt, 16, 6, 5, queries=a, max_leaves=6, **GAINS[gain])
    got = native.hist_tree(fresh[3], lam, wt, 16, depth, min_leaf, queries=b, max_leaves=2, **GAINS[gain]).to_dict()["DecisionTree"]
    exp = lw.tree_on_sample(X, lam, wt, fresh[5], feats, _binned(fresh, 16), sm.instance_rows(queries, b), feats, depth, min_leaf, 16, 2,
                            **GAINS[gain])
    assert got == exp and list(got.keys()) == ["LeafNode"]


@pytest.mark.parametrize("gain", sorted(GAINS))
@pytest.mark.parametrize("params", [dict(max_depth=1, min_leaf_support=1), dict(max_depth=6, min_leaf_support=1001)])
def test_training_single_leaf_trees_under_query_samples_on_a_fresh_dataset(thousand, gain, params):
    """No tree of the training searches its root, and every tree has another query sample: each leaf value is the
    restatement's over that tree's own instances."""
    X, y, qid = thousand[:3]
    _, st, trees = _stagewise(_case(X, y, qid), "ndcg", 4, dict(split_candidates=16, max_leaves=4, **dict(params, **GAINS[gain])),
                              rates=(0.5, 1.0), seed=3)
    assert all(list(t.keys()) == ["LeafNode"] for t in trees) and len({t["LeafNode"] for t in trees}) > 1
    assert st["mean_leaves"] == 1.0


@pytest.mark.parametrize("gain", sorted(GAINS))
def test_several_workgroups_per_stretch(big, gain):
    y = big[1]
    rng = np.random.default_rng(4)
    lam = rng.normal(0.0, 1.0, len(y)) * np.exp(rng.normal(0.0, 3.0, len(y))) + 0.3 * (y - 1)
    wt = rng.random(len(y))
    assert len(big[5]) >= 60000
    tree = _one_tree(big, lam, wt, 64 if gain == "variance" else 256, 12, 10, 8, GAINS[gain])
    assert lw.n_leaves(tree) == 8


def test_a_sampled_tree(synth):
    X, y, g, c, ids = synth[0], synth[1], synth[3], synth[4], synth[5]
    lam, wt = _gradients(y, 50)
    queries = lm.query_lists(c)
    half = sorted(np.random.default_rng(2).permutation(len(queries))[:len(queries) // 2].tolist())
    fids = [0, 2, 5, 8, 9]
    for gain in GAINS.values():
        got = native.hist_tree(g, lam, wt, 64, 10, 5, queries=half, features=fids, max_leaves=12, **gain).to_dict()["DecisionTree"]
        exp = lw.tree_on_sample(X, lam, wt, ids, list(range(X.shape[1])), _binned(synth, 64), sm.instance_rows(queries, half), fids, 10, 5, 64,
                                12, **gain)
        assert got == exp and lw.n_leaves(got) == 12


# --- training ------------------------------------------------------------------------------------

def _ensemble(trees, lr):
    return fr.CModel.from_dict({"Ensemble": {"weights": [lr] * len(trees), "models": [{"DecisionTree": x} for x in trees]}})


def _stagewise(case, measure, T, params, rates=(1.0, 1.0), seed=0, held=(), rounds=0):
    """Every tree of the model equals the restatement's fit, on the restatement's sample, to the device's gradients of the
    prefix model; the running scores are `predict` of the model; the measures after every tree are the oracle's."""
    X, y, qid, g, c = case[:5]
    req = _request(measure, num_trees=T, query_sampling_rate=rates[0], feature_sampling_rate=rates[1], seed=seed,
                   validation_queries=list(held), early_stopping_rounds=rounds, **params)
    p = req.params
    model = g.train_model(req)
    st = native.last_train_stats()["lambdamart"]
    d = model.to_dict()
    trees = [m["DecisionTree"] for m in d["Ensemble"]["models"]]
    assert st["max_leaves"] == p.max_leaves and st["grower"] == "histogram"
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
    gain = {k: getattr(p, k) for k in ("split_gain", "lambda_l2", "min_sum_hessian", "min_split_gain")}
    for t in range(len(trees)):
        fsel, qsel = vm.sample(seed, t, len(feats), Tq, rates)
        lam, wt = native.lambda_gradients(_ensemble(trees[:t], p.learning_rate), g, measure, p.sigma)
        exp = lw.tree_on_sample(X, np.nan_to_num(lam), np.nan_to_num(wt), order_ids, feats, binned, sm.instance_rows(queries, qsel), fsel,
                                p.max_depth, p.min_leaf_support, p.split_candidates, p.max_leaves, **gain)
        assert trees[t] == exp, "tree %d differs from the restatement's fit" % t
        exp_q, _ = c.metric_from_scores(measure, c.score_ensemble(trees[:t + 1], [p.learning_rate] * (t + 1)))
        if held:
            assert st["train_measure"][t] == vm.subset_mean(exp_q, Tq) and st["valid_measure"][t] == vm.subset_mean(exp_q, Hq)
        else:
            assert st["train_measure"][t] == o.mean(exp_q)
    if st["trees"] == len(trees):
        assert st["mean_leaves"] == sum(lw.n_leaves(t) for t in trees) / len(trees)
    assert st["pool_bytes"] <= p.max_leaves * len(feats) * p.split_candidates * (20 if p.split_gain == "newton" else 12)
    assert np.array_equal(native.predict_scores_dense(model, g), c.score_ensemble(trees, d["Ensemble"]["weights"]))
    return model, st, trees


@pytest.mark.parametrize("gain", sorted(GAINS))
def test_composition_stage_by_stage(synth, gain):
    """Leaf-wise trees under per-tree query and feature samples and a held-out split."""
    names = _names(synth[2])
    _, st, trees = _stagewise(synth, "ndcg", 10, dict(max_depth=10, min_leaf_support=10, split_candidates=64, max_leaves=12, **GAINS[gain]),
                              rates=(0.5, 0.5), seed=1, held=names[3::10])
    assert any(lw.n_leaves(t) == 12 for t in trees) and any(lw.depth(t) > 5 for t in trees)


@pytest.mark.parametrize("gain", sorted(GAINS))
@pytest.mark.parametrize("data", ["trec", "synth"])
def test_level_wise_identity(request, data, gain):
    """A budget of 2^(max_depth - 1) leaves, or 255, gives the bytes of the request without the key."""
    case = request.getfixturevalue(data)
    g = case[3]
    measure = "ndcg@10" if data == "trec" else "ndcg"
    for depth in (1, 4, 6):
        kw = dict(num_trees=3, max_depth=depth, min_leaf_support=5, split_candidates=16 if data == "trec" else 64, **GAINS[gain])
        absent = _request(measure, **kw)
        assert "max_leaves" not in absent.to_dict()["params"]["LambdaMART"]
        a = json.dumps(g.train_model(absent).to_dict())
        assert depth == 1 or "FeatureSplit" in a
        for budget in (max(2, 2 ** (depth - 1)), 255):
            assert json.dumps(g.train_model(_request(measure, max_leaves=budget, **kw)).to_dict()) == a, "depth %d, budget %d" % (depth, budget)
            assert native.last_train_stats()["lambdamart"]["max_leaves"] == budget


def test_deterministic_and_the_level_arrays_are_left_alone(synth):
    X, y, qid, g = synth[:4]
    g = fr.CDataset.from_numpy(X, y, qid)  # (a dataset of its own: no bins yet)
    kw = dict(num_trees=5, max_depth=8, min_leaf_support=10, split_candidates=64)
    absent = _request("ndcg", **kw)
    a = json.dumps(g.train_model(absent).to_dict())
    assert native.last_train_stats()["lambdamart"]["bins_ms"] > 0.0
    for gain in GAINS.values():
        leafwise = _request("ndcg", max_leaves=9, **dict(kw, **gain))
        b = json.dumps(g.train_model(leafwise).to_dict())
        st = native.last_train_stats()["lambdamart"]
        assert st["bins_ms"] == 0.0 and st["max_leaves"] == 9 and st["mean_leaves"] <= 9.0 and b != a
        assert json.dumps(g.train_model(leafwise).to_dict()) == b
        assert json.dumps(fr.CDataset.from_numpy(X, y, qid).train_model(leafwise).to_dict()) == b
        # a request without the key after a leaf-wise one gives the bytes it gave
        assert json.dumps(g.train_model(absent).to_dict()) == a
        assert native.last_train_stats()["lambdamart"]["bins_ms"] == 0.0
