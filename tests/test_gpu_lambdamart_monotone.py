"""Monotone constraints of LambdaMART's histogram grower on the device ("Monotone constraints"): the
monotone scan kernels against the Newton ones where no bound binds, one tree from given gradients against the numpy
restatement (tests/lambdamart_monotone_model.py) bit for bit, a constraint that binds, the property itself on trained models
(the scores never move against a feature's sign, with no tolerance), training stage by stage, and a request without the key."""
import json
import os

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import clib, native
from oracle import pyoracle as o
from tests import lambdamart_hist_model as hm
from tests import lambdamart_leafwise_model as lw
from tests import lambdamart_model as lm
from tests import lambdamart_monotone_model as mm
from tests import lambdamart_sample_model as sm
from tests.conftest import GOLDEN, synth_dataset

pytestmark = pytest.mark.gpu

L2S = [0.0, 2.0 ** -10, 1.0]
SIGNS = [{0: 1, 1: 1}, {0: -1, 1: -1}, {0: 1, 1: -1, 3: 1, 2: 0}]
MONO_KEYS = {"monotone_constraints", "monotone_clamped_leaves"}


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
    c = o.Dataset(X, y, qid)
    return X, y, qid, fr.CDataset.from_numpy(X, y, qid), c, np.concatenate(lm.query_lists(c)), {}


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


def _gradients(X, y, seed):
    """Gradients that rise and fall along the first features, so that either sign of a constraint has something to forbid."""
    rng = np.random.default_rng(seed)
    lam = rng.normal(0.0, 1.0, len(y)) + 0.5 * (y - y.mean()) + 2.0 * np.sin(7.0 * X[:, 0]) + np.cos(1.3 * X[:, 1]) + np.sin(2.0 * X[:, 3])
    return lam, rng.random(len(y))


def _one_tree(case, lam, wt, k, depth, min_leaf, monotone, max_leaves=0, **newton):
    """The device's tree and clamped count equal the restatement's; returns both."""
    X, g, ids = case[0], case[3], case[5]
    count = []
    got = native.hist_tree(g, lam, wt, k, depth, min_leaf, split_gain="newton", max_leaves=max_leaves, monotone=monotone, clamped_out=count,
                           **newton).to_dict()["DecisionTree"]
    exp, clamped = mm.fit_tree(X, lam, wt, ids, range(X.shape[1]), depth, min_leaf, k, monotone, max_leaves, _binned(case, k), **newton)
    what = "k = %d, depth %d, min_leaf %d, max_leaves %d, %r, %r" % (k, depth, min_leaf, max_leaves, monotone, newton)
    assert got == exp, what
    assert count == [clamped], what
    return got, clamped


def _grid(X, fid, points=40):
    """About `points` ascending f32 values of a feature: quantiles of its column, and the extremes of f32."""
    big = np.finfo(np.float32).max
    qs = np.quantile(X[:, fid].astype(np.float64), np.linspace(0.0, 1.0, points - 2)).astype(np.float32)
    return np.unique(np.concatenate([qs, np.asarray([-big, big], dtype=np.float32)]))


def _probe(X, fid, grid, rows=200):
    """rows x len(grid) instances: every one of the first `rows` training rows at every grid value of feature fid."""
    P = np.repeat(np.asarray(X[:rows], dtype=np.float32), len(grid), axis=0)
    P[:, fid] = np.tile(grid, rows)
    return P, np.repeat(np.arange(1, rows + 1, dtype=np.int64), len(grid))


def _against(S, sign):
    """The number of adjacent grid pairs at which a row's score moves against the sign (exact comparisons)."""
    return int(np.sum(S[:, 1:] < S[:, :-1])) if sign > 0 else int(np.sum(S[:, 1:] > S[:, :-1]))


# --- 1. kernel against kernel ---------------------------------------------------------------------

@pytest.mark.parametrize("k", [2, 16, 64, 256])
def test_constraints_on_the_constant_column_alone_give_the_newton_kernels_tree(synth, k):
    """Feature 9 has no edge: no interval is ever cut, nothing clamps, and the monotone scan kernels (level-wise and leaf-wise)
    must return the Newton kernels' tree byte for byte."""
    X, y, g = synth[0], synth[1], synth[3]
    lam, wt = _gradients(X, y, 10 + k)
    for sign in (1, -1):
        for depth, min_leaf, l2 in ((1, 1, 0.0), (4, 1, 2.0 ** -10), (10, 1, 1.0), (10, 25, 0.0)):
            count = []
            a = native.hist_tree(g, lam, wt, k, depth, min_leaf, split_gain="newton", lambda_l2=l2, monotone={9: sign}, clamped_out=count).to_dict()
            b = native.hist_tree(g, lam, wt, k, depth, min_leaf, split_gain="newton", lambda_l2=l2).to_dict()
            assert json.dumps(a) == json.dumps(b) and count == [0], "k = %d, depth %d, min_leaf %d" % (k, depth, min_leaf)
            assert depth == 1 or "FeatureSplit" in a["DecisionTree"]
        for budget in (2, 31, 255):
            count = []
            a = native.hist_tree(g, lam, wt, k, 12, 2, split_gain="newton", lambda_l2=1.0, max_leaves=budget, monotone={9: sign}, clamped_out=count).to_dict()
            b = native.hist_tree(g, lam, wt, k, 12, 2, split_gain="newton", lambda_l2=1.0, max_leaves=budget).to_dict()
            assert json.dumps(a) == json.dumps(b) and count == [0], "k = %d, max_leaves %d" % (k, budget)
            assert "FeatureSplit" in a["DecisionTree"]


# --- 2. one tree from given gradients --------------------------------------------------------------

@pytest.mark.parametrize("k", [2, 16, 64, 256])
@pytest.mark.parametrize("depth,min_leaf", [(1, 1), (4, 1), (4, 400), (10, 1), (10, 25)])
def test_one_tree_equals_restatement(synth, k, depth, min_leaf):
    """Every lambda_l2 with every set of signs over the grid: a case takes them three at a time."""
    X, y = synth[0], synth[1]
    lam, wt = _gradients(X, y, 100 * k + depth)
    turn = [2, 16, 64, 256].index(k) + depth + min_leaf
    for i, l2 in enumerate(L2S):
        tree, _ = _one_tree(synth, lam, wt, k, depth, min_leaf, SIGNS[(i + turn) % 3], lambda_l2=l2)
        assert lw.depth(tree) <= depth


@pytest.mark.parametrize("k", [2, 16, 64, 256])
@pytest.mark.parametrize("budget,depth,min_leaf", [(2, 6, 1), (31, 12, 1), (31, 5, 25), (255, 16, 2)])
def test_one_leaf_wise_tree_equals_restatement(synth, k, budget, depth, min_leaf):
    X, y = synth[0], synth[1]
    lam, wt = _gradients(X, y, 100 * k + budget)
    turn = [2, 16, 64, 256].index(k) + budget + depth
    for i, l2 in enumerate(L2S):
        tree, _ = _one_tree(synth, lam, wt, k, depth, min_leaf, SIGNS[(i + turn) % 3], max_leaves=budget, lambda_l2=l2)
        assert lw.n_leaves(tree) <= budget and lw.depth(tree) <= depth


def test_bounds_clamp_leaves_in_both_growth_modes(synth):
    """(the cases above are not all unclamped trees)"""
    X, y = synth[0], synth[1]
    lam, wt = _gradients(X, y, 7)
    assert _one_tree(synth, lam, wt, 64, 8, 5, SIGNS[2], lambda_l2=2.0 ** -10)[1] > 0
    assert _one_tree(synth, lam, wt, 64, 12, 5, SIGNS[2], max_leaves=31, lambda_l2=2.0 ** -10)[1] > 0
    # with the floors of the Newton gain, and on a sample of the queries and the features
    floors = dict(lambda_l2=1.0, min_sum_hessian=2.0 ** -6, min_split_gain=2.0 ** -20)
    _one_tree(synth, lam, wt, 64, 8, 5, SIGNS[0], **floors)
    _one_tree(synth, lam, wt, 16, 10, 5, SIGNS[1], max_leaves=20, **floors)
    g, c, ids = synth[3], synth[4], synth[5]
    queries = lm.query_lists(c)
    half = sorted(np.random.default_rng(2).permutation(len(queries))[:len(queries) // 2].tolist())
    fids = [0, 2, 3, 5, 8]  # (feature 1 is constrained and not in the sample: its sign is not read)
    feats = list(range(X.shape[1]))
    for budget in (0, 12):
        count = []
        got = native.hist_tree(g, lam, wt, 64, 8, 5, queries=half, features=fids, split_gain="newton", max_leaves=budget, monotone=SIGNS[2],
                               clamped_out=count, **floors).to_dict()["DecisionTree"]
        exp, clamped = mm.tree_on_sample(X, lam, wt, ids, feats, _binned(synth, 64), sm.instance_rows(queries, half), fids, 8, 5, 64, SIGNS[2],
                                         budget, **floors)
        assert got == exp and count == [clamped], "max_leaves %d" % budget


def test_one_tree_with_many_workgroups_per_histogram(big):
    X, y, ids = big[0], big[1], big[5]
    rng = np.random.default_rng(4)
    lam = rng.normal(0.0, 1.0, len(y)) * np.exp(rng.normal(0.0, 3.0, len(y))) + 0.3 * (y - 1) + np.sin(7.0 * X[:, 0])
    wt = rng.random(len(y))
    assert len(ids) >= 60000
    _one_tree(big, lam, wt, 256, 6, 10, SIGNS[2], lambda_l2=1.0, min_sum_hessian=2.0 ** -6, min_split_gain=2.0 ** -20)
    _one_tree(big, lam, wt, 64, 12, 10, SIGNS[2], max_leaves=16, lambda_l2=2.0 ** -10)


# --- 3. the constraint binds ------------------------------------------------------------------------

def test_a_constraint_against_the_gradients_binds(synth):
    """Gradients that fall along feature 4 under a constraint that the score must not: the tree differs from the plain one,
    a bound moved a leaf, the tree is monotone and the plain one is not (the seed was chosen on the CPU restatement for the
    four of them)."""
    X, y, g = synth[0], synth[1], synth[3]
    fid = 4
    rng = np.random.default_rng(7)
    lam = -(X[:, fid] - X[:, fid].mean()) + rng.normal(0.0, 1.0, len(y))
    wt = rng.random(len(y))
    tree, clamped = _one_tree(synth, lam, wt, 64, 10, 2, {fid: 1}, lambda_l2=1.0)
    plain = native.hist_tree(g, lam, wt, 64, 10, 2, split_gain="newton", lambda_l2=1.0).to_dict()["DecisionTree"]
    assert tree != plain and clamped >= 1
    grid = mm.probe_grid(_binned(synth, 64)[0][fid])
    assert mm.violations(lambda P: mm.predict(tree, P), X[:200], fid, grid, 1) == 0
    assert mm.violations(lambda P: mm.predict(plain, P), X[:200], fid, grid, 1) > 0


# --- 4. the property on trained models ----------------------------------------------------------------

CONSTRAINTS = {"0": 1, "1": -1}
VARIANTS = {
    "plain": dict(num_trees=20),
    "leaf_wise": dict(num_trees=10, max_leaves=31, max_depth=12),
    "sampled": dict(num_trees=10, query_sampling_rate=0.5, feature_sampling_rate=0.5, seed=1),
    "held_out": dict(num_trees=10, validation_queries="names"),
    "truncated": dict(num_trees=10, truncation_level=10, lambda_norm=True),
    "map": dict(num_trees=10, objective="map"),
    "dart": dict(num_trees=10, drop_rate=0.3, seed=2),
}


@pytest.fixture(scope="module")
def probes(synth):
    """Per constrained feature: the grid's length, the probe as a device dataset and as the oracle's."""
    X = synth[0]
    out = {}
    for name in CONSTRAINTS:
        grid = _grid(X, int(name))
        P, qid = _probe(X, int(name), grid)
        zeros = np.zeros(len(P))
        out[name] = (len(grid), fr.CDataset.from_numpy(P, zeros, qid), o.Dataset(P, zeros, qid))
    return out


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_trained_models_are_monotone(synth, probes, variant):
    X, y, qid, g = synth[:4]
    kw = dict(max_depth=6, min_leaf_support=10, split_candidates=64, split_gain="newton", lambda_l2=1.0)
    kw.update(VARIANTS[variant])
    if kw.get("validation_queries") == "names":
        kw["validation_queries"] = _names(qid)[3::10]
    models = {}
    for constrained in (True, False):
        req = _request("ndcg@10", **dict(kw, monotone_constraints=dict(CONSTRAINTS) if constrained else {}))
        models[constrained] = g.train_model(req)
        st = native.last_train_stats()["lambdamart"]
        if constrained:
            assert st["monotone_constraints"] == CONSTRAINTS and len(st["monotone_clamped_leaves"]) == st["trees"] == kw["num_trees"]
        else:
            assert not MONO_KEYS & set(st)
    broken = 0
    for name, sign in CONSTRAINTS.items():
        G, gp, cp = probes[name]
        for constrained, model in models.items():
            d = model.to_dict()["Ensemble"]
            scores = native.predict_scores_dense(model, gp)
            assert np.array_equal(scores, cp.score_ensemble([m["DecisionTree"] for m in d["models"]], d["weights"]))
            against = _against(scores.reshape(-1, G), sign)
            if constrained:
                assert against == 0, "feature %s: the score moves against its sign at %d grid steps" % (name, against)
            else:
                broken += against
    assert broken > 0  # the same request without the key is not monotone: the property above is not vacuous
    assert json.dumps(models[True].to_dict()) != json.dumps(models[False].to_dict())


# --- 5. stage by stage ----------------------------------------------------------------------------

def _ensemble(trees, lr):
    return fr.CModel.from_dict({"Ensemble": {"weights": [lr] * len(trees), "models": [{"DecisionTree": x} for x in trees]}})


@pytest.mark.parametrize("max_leaves", [0, 12])
@pytest.mark.parametrize("data", ["trec", "synth"])
def test_stage_by_stage(request, data, max_leaves):
    """Every tree equals the restatement's fit to the device's gradients of the prefix model, and the stats' clamped leaves are
    the restatement's counts."""
    case = request.getfixturevalue(data)
    X, y, qid, g, c, order_ids = case[:6]
    measure = "ndcg@10" if data == "trec" else "ndcg"
    T = 10
    constraints = {"0": 1, "1": -1} if data == "synth" else {"3": -1, "5": 1}
    newton = dict(lambda_l2=1.0, min_sum_hessian=2.0 ** -6, min_split_gain=2.0 ** -20)
    req = _request(measure, num_trees=T, max_depth=10 if max_leaves else 5, min_leaf_support=5, split_candidates=16 if data == "trec" else 64,
                   split_gain="newton", max_leaves=max_leaves, monotone_constraints=constraints, **newton)
    p = req.params
    model = g.train_model(req)
    st = native.last_train_stats()["lambdamart"]
    d = model.to_dict()
    trees = [m["DecisionTree"] for m in d["Ensemble"]["models"]]
    assert st["trees"] == T and len(trees) == T and st["monotone_constraints"] == constraints
    feats = list(range(X.shape[1]))
    binned = _binned(case, p.split_candidates)
    monotone = {int(k): v for k, v in constraints.items()}
    counts = []
    for t in range(T):
        lam, wt = native.lambda_gradients(_ensemble(trees[:t], p.learning_rate), g, measure, p.sigma)
        exp, clamped = mm.fit_tree(X, np.nan_to_num(lam), np.nan_to_num(wt), order_ids, feats, p.max_depth, p.min_leaf_support,
                                   p.split_candidates, monotone, max_leaves, binned, **newton)
        assert trees[t] == exp, "tree %d differs from the restatement's fit" % t
        counts.append(clamped)
        exp_q, _ = c.metric_from_scores(measure, c.score_ensemble(trees[:t + 1], [p.learning_rate] * (t + 1)))
        assert st["train_measure"][t] == o.mean(exp_q)
    print("clamped leaves per tree (%s, max_leaves %d): %r" % (data, max_leaves, counts))
    assert st["monotone_clamped_leaves"] == counts
    assert any("FeatureSplit" in t for t in trees)
    assert np.array_equal(native.predict_scores_dense(model, g), c.score_ensemble(trees, d["Ensemble"]["weights"]))


# --- 6. a request without the key ---------------------------------------------------------------------

@pytest.mark.parametrize("others", [dict(split_gain="newton", lambda_l2=1.0), dict(split_gain="newton", max_leaves=9, max_depth=10), dict(),
                                    dict(grower="exact")])
def test_zero_entries_are_the_request_without_the_key(trec, others):
    X, y, qid, g = trec[:4]
    kw = dict(num_trees=4, max_depth=4, min_leaf_support=5, split_candidates=16)
    absent = _request("ndcg@10", **dict(kw, **others))
    assert "monotone_constraints" not in absent.to_dict()["params"]["LambdaMART"]
    a = json.dumps(g.train_model(absent).to_dict())
    keys = list(native.last_train_stats()["lambdamart"])
    assert not MONO_KEYS & set(keys)
    wire = absent.to_dict()
    wire["params"]["LambdaMART"]["monotone_constraints"] = {"0": 0, "3": 0}
    m = fr.CModel(clib._unwrap(clib._load().train_model(json.dumps(wire).encode(), g.pointer)))
    assert json.dumps(m.to_dict()) == a
    assert list(native.last_train_stats()["lambdamart"]) == keys
    if others.get("split_gain") == "newton":  # a constrained training in between leaves the plain one what it was
        b = json.dumps(g.train_model(_request("ndcg@10", **dict(kw, monotone_constraints={"3": 1, "4": -1}, **others))).to_dict())
        assert b != a and MONO_KEYS <= set(native.last_train_stats()["lambdamart"])
        assert json.dumps(g.train_model(absent).to_dict()) == a
        assert list(native.last_train_stats()["lambdamart"]) == keys
