"""LambdaMART's gradient-based one-side sampling on the device (kernels_goss.inc; DESIGN.md section 11, "GOSS") against the
numpy restatement (tests/lambdamart_goss_model.py), bit for bit.

Selection: native.goss_select -- the radix select, the tie scan, the Bernoulli flags, the list -- gives the restatement's list,
top flags and tau.  One tree: native.hist_tree(goss=...) is the Newton / leaf-wise / monotone restatement run on the
restatement's list with amplified gradients.  Training: every tree equals that fit to the DEVICE's gradients of the ensemble the
tree is fitted to, under the tree's key; scores, prediction and measures are the oracle's.
"""
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
from tests import lambdamart_sample_model as sm
from tests import lambdamart_valid_model as vm
from tests import lambdamart_xendcg_model as xm
from tests.conftest import GOLDEN, synth_dataset

pytestmark = pytest.mark.gpu

EMPTY = {"Ensemble": {"weights": [], "models": []}}
SHARE = 4096  # GOSS_SHARE: the entries of the list one workgroup of goss_hist_kernel counts
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, SHARE + 1, 60000]
GOSS_STATS = {"goss_top_rate", "goss_other_rate", "goss_ms", "goss_instances", "goss_top"}


# --- selection -----------------------------------------------------------------------------------

class Listed:
    """A dataset of n documents in queries of at most 40, with its full instance list."""

    def __init__(self, n, seed=0):
        rng = np.random.default_rng(1000 + n + seed)
        qid = (np.arange(n) // 40 + 1).astype(np.int64)
        self.X = rng.random((n, 2)).astype(np.float32)
        self.y = rng.integers(0, 3, n).astype(np.float64)
        self.qid, self.n = qid, n
        self.g, self.c = fr.CDataset.from_numpy(self.X, self.y, qid), o.Dataset(self.X, self.y, qid)
        self.queries = lm.query_lists(self.c)
        self.order_ids = np.concatenate(self.queries)


_listed = {}


def listed(n):
    if n not in _listed:
        _listed[n] = Listed(n)
    return _listed[n]


def _same_selection(ds, lam, a, b, seed, tree, qsel=None, g=None, order_ids=None, queries=None):
    """The device's selection is the restatement's; returns it."""
    order_ids = ds.order_ids if order_ids is None else order_ids
    queries = ds.queries if queries is None else queries
    L = np.arange(len(order_ids)) if qsel is None else sm.instance_rows(queries, qsel)
    key = gm.keys(seed, tree + 1)[tree]
    exp_rows, exp_top, exp_tau, _ = gm.goss_list(lam, L, order_ids, a, b, key)
    rows, top, tau = native.goss_select(ds.g if g is None else g, lam, a, b, seed, tree, queries=qsel)
    assert tau == exp_tau, "tau %016x, not %016x" % (tau, exp_tau)
    assert np.array_equal(rows, exp_rows), "the list differs (%d entries, %d expected)" % (len(rows), len(exp_rows))
    assert np.array_equal(top, exp_top), "the top flags differ"
    return rows, top, tau


def _rates(n):
    """(a, b): the usual rates, n_top = 1, n_top = n - 1 (n * a = n - 0.5), and everything kept."""
    out = [(0.2, 0.1), (1e-9, 0.3), (0.5, 0.5)]
    if n >= 2:
        a = (n - 0.5) / n
        out.append((a, min(0.1, (1.0 - a) * 0.8)))
        assert gm.plan(n, *out[-1])[0] == n - 1 and a + out[-1][1] <= 1.0
    assert gm.plan(n, *out[1])[0] == 1
    return out


@pytest.mark.parametrize("n", SIZES)
def test_select_is_the_restatements(n):
    ds = listed(n)
    rng = np.random.default_rng(n)
    lam = rng.standard_normal(n) * np.exp(rng.standard_normal(n) * 3.0)
    for i, (a, b) in enumerate(_rates(n)):
        rows, top, _ = _same_selection(ds, lam, a, b, seed=7 + i, tree=i)
        n_top, p, _ = gm.plan(n, a, b)
        assert int(top.sum()) == n_top and (p < 1.0 or len(rows) == n)
    if n >= 1000:  # (the Bernoulli part did something)
        rows, top, _ = _same_selection(ds, lam, 0.2, 0.1, seed=1, tree=0)
        assert n // 5 < len(rows) < n // 2


def _designed(n, rng):
    i = np.arange(n)
    sign = np.where(i % 2 == 0, 1.0, -1.0)
    one = np.float64(1.0).view(np.uint64)
    ulps = (one + np.uint64(1) * (rng.permutation(n) % 7).astype(np.uint64)).view(np.float64)  # 1.0 .. 1.0 + 6 ulp
    exps = np.ldexp(1.0, ((rng.permutation(n) % 5) * 400 - 1000).astype(np.int64))            # 2^-1000 .. 2^600: the first digit decides
    ties = rng.standard_normal(n)
    ties[np.abs(ties) < 0.25] *= 0.1
    ties[rng.permutation(n)[: n // 2]] = 0.25  # half of the keys equal (hundreds at n = 2500); with a = 0.5 tau falls among them
    return {"equal": np.full(n, -0.375), "zero": np.zeros(n), "signed zeros": np.where(i % 3 == 0, -0.0, 0.0),
            "lowest mantissa bit": ulps * sign, "highest exponent bits": exps * sign,
            "denormals": ((rng.permutation(n) % 9) + 1) * 5e-324 * sign, "denormals and zeros": (rng.permutation(n) % 3) * 5e-324,
            "a tie group across tau": ties * sign}


@pytest.mark.parametrize("n", [257, 2500])
def test_select_on_designed_gradients(n):
    ds = listed(n)
    for name, lam in _designed(n, np.random.default_rng(n + 1)).items():
        for a, b in ((0.2, 0.1), (0.5, 0.25), (1e-9, 0.3)):
            try:
                rows, top, tau = _same_selection(ds, lam, a, b, seed=3, tree=2)
            except AssertionError as e:
                raise AssertionError("%s, (a, b) = (%g, %g): %s" % (name, a, b, e))
            if name == "a tie group across tau" and a == 0.5:
                k = gm.bit_keys(lam)[ds.order_ids]
                tied = np.flatnonzero(k == tau)
                taken = np.isin(tied, rows[top])
                assert len(tied) == n // 2 and 0 < taken.sum() < len(tied) and np.all(taken[: taken.sum()])  # the tie rule decided


def test_select_over_a_query_sample_and_twice():
    ds = listed(2500)
    lam = np.random.default_rng(5).standard_normal(2500)
    nq = len(ds.queries)
    for qsel in (np.arange(0, nq, 2), np.array([nq - 1]), np.arange(3, nq - 4)):
        rows, _, _ = _same_selection(ds, lam, 0.2, 0.3, seed=11, tree=1, qsel=qsel)
        assert np.all(np.isin(rows, sm.instance_rows(ds.queries, qsel)))
    first = native.goss_select(ds.g, lam, 0.2, 0.3, 11, 1)
    again = native.goss_select(ds.g, lam, 0.2, 0.3, 11, 1)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes() and first[2] == again[2]
    other_tree = native.goss_select(ds.g, lam, 0.2, 0.3, 11, 2)
    other_seed = native.goss_select(ds.g, lam, 0.2, 0.3, 12, 1)
    assert first[0].tobytes() != other_tree[0].tobytes() and first[0].tobytes() != other_seed[0].tobytes()
    assert first[2] == other_tree[2] == other_seed[2]  # (tau is the gradients' alone)


def test_a_sampled_view_draws_its_parents_uniforms():
    ds = listed(2500)
    lam = np.random.default_rng(6).standard_normal(2500)
    names = cmod._names(ds.qid)
    pick = names[1::3]
    view = ds.g.subsample_queries(pick)
    qsel = np.asarray([names.index(x) for x in pick])
    vq = [ds.queries[q] for q in qsel]
    v_ids = np.concatenate(vq)
    # the view's own list: its selection is the restatement's under the ORIGINAL instance ids
    rows, top, _ = _same_selection(ds, lam, 0.2, 0.3, seed=4, tree=0, g=view, order_ids=v_ids, queries=vq)
    # ... and equals the parent's selection over the same queries as a query sample (same list, same ids, same key)
    prow, ptop, _ = native.goss_select(ds.g, lam, 0.2, 0.3, 4, 0, queries=qsel)
    assert np.array_equal(ds.order_ids[prow], v_ids[rows]) and np.array_equal(ptop, top)


# --- one tree ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def synth():
    X, y, qid = synth_dataset(7, 5000, 10, 50)
    return X, y, qid, fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)


@pytest.fixture(scope="module")
def trec():
    d = np.load(os.path.join(GOLDEN, "trec_news_2018.npz"))
    X, y, qid = d["train_X"], d["train_y"], d["train_qid"]
    return X, y, qid, fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)


def _gradients(n, seed):
    rng = np.random.default_rng(seed)
    lam = rng.standard_normal(n) * np.exp(rng.standard_normal(n))
    lam[rng.random(n) < 0.3] = 0.0
    return lam, rng.random(n) * np.abs(lam) + 1e-3


def _one_tree(X, g, c, lam, wt, k, depth, min_leaf, a, b, seed, tree, qsel=None, fsel=None, binned=None, **kw):
    queries = lm.query_lists(c)
    order_ids = np.concatenate(queries)
    feats = list(range(X.shape[1]))
    binned = hm.bin_matrix(X, order_ids, feats, k) if binned is None else binned
    L = np.arange(len(order_ids)) if qsel is None else sm.instance_rows(queries, qsel)
    fs = list(range(len(feats))) if fsel is None else list(fsel)
    key = gm.keys(seed, tree + 1)[tree]
    exp, rows, top = gm.tree(X, lam, wt, order_ids, feats, binned, L, fs, depth, min_leaf, k, a, b, key, **kw)
    got = native.hist_tree(g, lam, wt, k, depth, min_leaf, queries=qsel, features=None if fsel is None else [feats[s] for s in fsel],
                           split_gain="newton", goss=(a, b, seed, tree), **kw).to_dict()["DecisionTree"]
    assert got == exp
    return got, rows, top


@pytest.mark.parametrize("k,depth", [(2, 1), (2, 4), (64, 4), (64, 10), (256, 4), (256, 10)])
def test_one_goss_tree_is_the_newton_restatement_on_the_list(synth, k, depth):
    X, y, qid, g, c = synth
    lam, wt = _gradients(len(y), k + depth)
    tree, rows, top = _one_tree(X, g, c, lam, wt, k, depth, 10, 0.2, 0.1, seed=9, tree=3, lambda_l2=0.5, min_sum_hessian=2.0 ** -8)
    assert ("FeatureSplit" in tree) == (depth > 1) and 1000 < len(rows) < 2500
    # amplification reaches the tree: the same list with the others' gradients as they were is another tree
    if depth > 1:
        plain = native.hist_tree(g, lam, wt, k, depth, 10, split_gain="newton", lambda_l2=0.5, min_sum_hessian=2.0 ** -8).to_dict()["DecisionTree"]
        assert plain != tree


def test_goss_tree_on_samples_leafwise_and_monotone(synth):
    X, y, qid, g, c = synth
    lam, wt = _gradients(len(y), 77)
    nq = len(lm.query_lists(c))
    binned = hm.bin_matrix(X, np.concatenate(lm.query_lists(c)), list(range(X.shape[1])), 32)
    common = dict(binned=binned, lambda_l2=1.0)
    _one_tree(X, g, c, lam, wt, 32, 6, 5, 0.3, 0.2, 2, 0, qsel=np.arange(0, nq, 2), fsel=[0, 3, 4, 8], **common)
    for max_leaves in (2, 31):
        tree, _, _ = _one_tree(X, g, c, lam, wt, 32, 12, 5, 0.2, 0.1, 2, 1, max_leaves=max_leaves, **common)
        assert json.dumps(tree).count("LeafNode") == max_leaves
    for max_leaves in (0, 8):
        _one_tree(X, g, c, lam, wt, 32, 5, 5, 0.2, 0.1, 2, 2, max_leaves=max_leaves, monotone={0: 1, 1: -1}, **common)
    # fewer kept instances than min_leaf_support: one leaf, the Newton value of the list's own sums
    tree, rows, _ = _one_tree(X, g, c, lam, wt, 32, 6, 4000, 0.2, 0.1, 2, 3, **common)
    assert len(rows) < 4000 and list(tree) == ["LeafNode"] and tree["LeafNode"] != 0.0
    # every gradient zero: LeafNode(0.0)
    zero, _, _ = _one_tree(X, g, c, np.zeros(len(y)), wt, 32, 6, 5, 0.2, 0.1, 2, 4, **common)
    assert zero == {"LeafNode": 0.0}


def test_goss_tree_over_sixty_thousand_kept_instances():
    X, y, qid = synth_dataset(11, 70000, 6, 600)
    g, c = fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)
    lam, wt = _gradients(len(y), 5)
    tree, rows, top = _one_tree(X, g, c, lam, wt, 16, 4, 10, 0.6, 0.35, seed=1, tree=0)
    assert len(rows) >= 60000 and int(top.sum()) == gm.plan(len(y), 0.6, 0.35)[0] >= 41999 and "FeatureSplit" in tree


# --- training ------------------------------------------------------------------------------------

def _ensemble(trees, weights):
    if not trees:
        return fr.CModel.from_dict(EMPTY)
    return fr.CModel.from_dict({"Ensemble": {"weights": [float(w) for w in weights], "models": [{"DecisionTree": x} for x in trees]}})


def _trees(model):
    return [m["DecisionTree"] for m in model.to_dict()["Ensemble"]["models"]]


def _stagewise(g, c, X, y, measure, params, names=None, binned=None, strict=True):
    """Trains under GOSS and holds every stage to the restatements: tree t is the GOSS restatement's fit -- list, amplified
    gradients, then the Newton / leaf-wise / monotone restatement -- to the DEVICE's gradients of the ensemble the tree is
    fitted to (the prefix; under DART without the dropped trees), over the tree's query and feature sample, under the key K_t;
    the running measures are the oracle's of the oracle's ensemble scores, the prediction is the oracle's.  strict: the case
    was designed, so its trees split, its plan drops and its lists shrink (a drawn case may do none of these)."""
    params = dict(params, split_gain="newton")
    req = cmod._request(measure, "histogram", **params)
    p = req.params
    a, b = p.goss_top_rate, p.goss_other_rate
    cm = cmod.Composed(X, y, c, measure, dict(fr.LambdaMARTParams().to_dict(), **dict(params, grower="histogram")), names=names, binned=binned)
    model = g.train_model(req)
    st = native.last_train_stats()["lambdamart"]
    assert GOSS_STATS <= set(st) and st["goss_top_rate"] == a and st["goss_other_rate"] == b and st["goss_ms"] > 0.0
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
    assert len(st["goss_instances"]) == T == len(st["goss_top"])
    keys, xkeys = gm.keys(p.seed, T), xm.keys(p.seed, T)
    plan = dm.plan(p.seed, p.drop_rate, p.max_drop, p.skip_drop, T, p.learning_rate) if p.drop_rate > 0 else None
    if plan is not None:
        assert st["dropped"] == [len(D) for D, _, _ in plan] and (any(st["dropped"]) or not strict)
        assert np.asarray(d["Ensemble"]["weights"], dtype=np.float64).tobytes() == plan[-1][2].tobytes()
    else:
        assert d["Ensemble"]["weights"] == [p.learning_rate] * len(got)
    mono = {int(k): int(v) for k, v in p.monotone_constraints.items()}
    shrunk = 0
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
        L = sm.instance_rows(cm.queries, qsel)
        exp, rows, top = gm.tree(X, lam, wt, cm.order_ids, cm.feats, cm.binned, L, list(fsel), p.max_depth, p.min_leaf_support,
                                 p.split_candidates, a, b, keys[t], max_leaves=p.max_leaves, monotone=mono, **cm.newton())
        assert st["goss_instances"][t] == len(rows) and st["goss_top"][t] == int(top.sum()) == gm.plan(len(L), a, b)[0], "tree %d" % t
        assert trees[t] == exp, "tree %d differs from the restatement's fit" % t
        shrunk += len(rows) < len(L)
        tr, va, err = cm.measures(c.score_ensemble(trees[:t + 1], after))
        assert err == 0
        assert st["train_measure"][t] == tr, "train_measure[%d]" % t
        if va is not None:
            assert st["valid_measure"][t] == va, "valid_measure[%d]" % t
    assert shrunk == T or a + b == 1.0 or not strict
    assert np.array_equal(native.predict_scores_dense(model, g), c.score_ensemble(got, d["Ensemble"]["weights"]))
    assert any("FeatureSplit" in t for t in trees) or not strict
    return model, st


def _shape(data):
    if data == "trec":
        return dict(max_depth=5, min_leaf_support=5, split_candidates=16)
    return dict(max_depth=4, min_leaf_support=10, split_candidates=12)


@pytest.mark.parametrize("rates", [(0.2, 0.1), (0.5, 0.25)])
@pytest.mark.parametrize("data", ["trec", "synth"])
def test_stagewise_identity(request, data, rates):
    X, y, qid, g, c = request.getfixturevalue(data)
    kw = dict(num_trees=10, seed=11, goss_top_rate=rates[0], goss_other_rate=rates[1], **_shape(data))
    model, st = _stagewise(g, c, X, y, "ndcg@7", kw)
    got = json.dumps(model.to_dict())
    # determinism, and the seed reaches the selection
    assert json.dumps(g.train_model(cmod._request("ndcg@7", "histogram", split_gain="newton", **kw)).to_dict()) == got
    assert json.dumps(g.train_model(cmod._request("ndcg@7", "histogram", split_gain="newton", **dict(kw, seed=12))).to_dict()) != got


SMALL = dict(num_trees=6, seed=3, max_depth=4, min_leaf_support=5, split_candidates=16, goss_top_rate=0.2, goss_other_rate=0.1)


@pytest.mark.parametrize("extra", [
    dict(query_sampling_rate=0.5, feature_sampling_rate=0.5),
    dict(validation_queries="every fifth", early_stopping_rounds=2, num_trees=12, learning_rate=0.5),
    dict(validation_queries="every fifth", feature_sampling_rate=0.5),  # (a fixed split: the query sample's list is made once)
    dict(drop_rate=0.1, num_trees=10, seed=1),  # (the defaults of the two other keys; under seed 1 five of the ten trees drop)
    dict(drop_rate=0.5, skip_drop=0.25, max_drop=3),
    dict(objective="xendcg"),
    dict(objective="map"),
    dict(truncation_level=3),
    dict(max_leaves=6, max_depth=10, lambda_l2=0.5, min_sum_hessian=2.0 ** -6),
    dict(monotone_constraints={"0": 1, "1": -1}, lambda_l2=1.0),
], ids=["samples", "holdout+stopping", "holdout+features", "dart-0.1", "dart", "xendcg", "map", "truncation", "leafwise", "monotone"])
def test_goss_composes_with_the_other_keys(synth, extra):
    X, y, qid, g, c = synth
    names = cmod._names(qid)
    extra = dict(extra)
    if extra.get("validation_queries"):
        extra["validation_queries"] = names[::5]
    _stagewise(g, c, X, y, "ndcg@10", dict(SMALL, **extra), names=names)


def test_truncation_leaves_exact_zeros_for_the_tie_rule(synth):
    """Under truncation_level 3 about half of the documents have lambda exactly 0: with a = 0.6 tau is 0 and the top set is
    filled with zero-gradient documents in list order."""
    X, y, qid, g, c = synth
    lam, _ = native.lambda_gradients(_ensemble([], []), g, "ndcg@10", 1.0, truncation_level=3)
    assert len(lam) // 4 < np.count_nonzero(lam) < gm.plan(len(lam), 0.6, 0.25)[0]
    order_ids = np.concatenate(lm.query_lists(c))
    rows, top, tau = native.goss_select(g, lam, 0.6, 0.25, 3, 0)
    assert tau == 0 and np.count_nonzero(lam[order_ids][rows[top]]) == np.count_nonzero(lam)
    _stagewise(g, c, X, y, "ndcg@10", dict(SMALL, goss_top_rate=0.6, goss_other_rate=0.25, truncation_level=3, num_trees=3))


def test_rates_that_sum_to_one_and_absent_keys_are_the_plain_request(synth):
    X, y, qid, g, c = synth
    kw = dict(num_trees=5, seed=2, max_depth=4, min_leaf_support=10, split_candidates=12, split_gain="newton", lambda_l2=0.25)
    plain = g.train_model(cmod._request("ndcg@7", "histogram", **kw))
    st_plain = native.last_train_stats()["lambdamart"]
    assert not (GOSS_STATS & set(st_plain)) and "goss_top_rate" not in cmod._request("ndcg@7", "histogram", **kw).to_dict()["params"]["LambdaMART"]
    whole = g.train_model(cmod._request("ndcg@7", "histogram", goss_top_rate=0.5, goss_other_rate=0.5, **kw))
    st = native.last_train_stats()["lambdamart"]
    n = len(y)
    assert st["goss_instances"] == [n] * 5 and st["goss_top"] == [n // 2] * 5  # (everything kept, nothing amplified)
    assert json.dumps(whole.to_dict()) == json.dumps(plain.to_dict())
    assert set(st) - GOSS_STATS == set(st_plain) and st["train_measure"] == st_plain["train_measure"]
    # the plain request is still the Newton restatement's, stage by stage
    cm = cmod.Composed(X, y, c, "ndcg@7", dict(fr.LambdaMARTParams().to_dict(), **dict(kw, grower="histogram")))
    trees = _trees(plain)
    for t in range(len(trees)):
        lam, wt = native.lambda_gradients(_ensemble(trees[:t], [0.1] * t), g, "ndcg@7", 1.0)
        assert trees[t] == cm.tree(lam, wt, *cm.sample(t))


# --- small soak ----------------------------------------------------------------------------------

def _soak_case(i):
    """Case i of the soak: a small random set and the two rates drawn with the other keys of the histogram grower, from a
    generator of its own."""
    rng = np.random.default_rng([20171204, i])
    n, d, q = int(rng.integers(300, 1500)), int(rng.integers(3, 8)), int(rng.integers(8, 40))
    X, y, qid = synth_dataset(int(rng.integers(1, 10 ** 6)), n, d, q)
    a = float(rng.choice([0.05, 0.1, 0.2, 0.35, 0.5, 0.75]))
    b = float(rng.choice([x for x in (0.05, 0.1, 0.25, 0.5) if a + x <= 1.0]))
    p = dict(num_trees=4, seed=int(rng.integers(0, 2 ** 63)), goss_top_rate=a, goss_other_rate=b, max_depth=int(rng.integers(2, 7)),
             min_leaf_support=int(rng.integers(1, 20)), split_candidates=int(rng.choice([2, 5, 16, 64, 256])),
             learning_rate=float(rng.choice([0.1, 0.3])), lambda_l2=float(rng.choice([0.0, 0.5])))
    if rng.random() < 0.5:
        p["max_leaves"] = int(rng.integers(2, 12))
        p["max_depth"] = int(rng.integers(3, 12))
    if rng.random() < 0.5:
        p["query_sampling_rate"] = float(rng.choice([0.3, 0.7]))
    if rng.random() < 0.5:
        p["feature_sampling_rate"] = float(rng.choice([0.4, 0.8]))
    names = cmod._names(qid)
    if rng.random() < 0.4:
        p["validation_queries"] = names[int(rng.integers(0, 3))::4]
    p["objective"] = str(rng.choice(["ndcg", "ndcg", "map", "xendcg"]))
    if p["objective"] == "ndcg" and rng.random() < 0.5:
        p["truncation_level"] = int(rng.integers(1, 6))
    if rng.random() < 0.3:
        p.update(drop_rate=0.5, skip_drop=0.0)
    if rng.random() < 0.3:
        p["monotone_constraints"] = {"0": int(rng.choice([-1, 1]))}
    return X, y, qid, names, p


@pytest.mark.parametrize("i", range(8))
def test_soak(i):
    X, y, qid, names, p = _soak_case(i)
    g, c = fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)
    try:
        _stagewise(g, c, X, y, "ndcg@5", p, names=names, strict=False)
    except AssertionError as e:
        raise AssertionError("case %d %r: %s" % (i, {k: v for k, v in p.items() if k != "validation_queries"}, e))
