"""LambdaMART's DART boosting on the device ("DART") against the numpy restatement
(tests/lambdamart_dart_model.py): dart_rescore_kernel on its own over random forests, then training stage by stage with
both growers, composed with the other keys, and the identities that need no restatement.  Every sum is held bit for bit:
the arithmetic is defined operation by operation."""
import json
import os

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import clib, native
from oracle import pyoracle as o
from tests import lambdamart_composed_model as cmod
from tests import lambdamart_dart_model as dm
from tests import lambdamart_hist_model as hm
from tests import lambdamart_sample_model as sm
from tests import lambdamart_valid_model as vm
from tests.conftest import GOLDEN, synth_dataset

pytestmark = pytest.mark.gpu

EMPTY = {"Ensemble": {"weights": [], "models": []}}
TILE = 1024  # documents per workgroup of dart_rescore_kernel (256 lanes x 4)
DART = dict(drop_rate=0.5, skip_drop=0.25, max_drop=3)
DART_STATS = {"drop_rate", "max_drop", "skip_drop", "dropped", "dart_ms", "dart_cache_bytes"}


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


def _ensemble(trees, weights):
    return fr.CModel.from_dict({"Ensemble": {"weights": [float(w) for w in weights], "models": [{"DecisionTree": x} for x in trees]}})


def _request(measure, grower, **kw):
    req = fr.TrainRequest.lambdamart()
    req.measure = measure
    req.params.quiet = True
    req.params.grower = grower
    for k, v in kw.items():
        setattr(req.params, k, v)
    return req


# --- the kernel alone ----------------------------------------------------------------------------

SPECIAL = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, 1e-310, 1.0, -1.0, 3.0])


def _forest(rng, X, count, deep=0):
    """`count` random trees made as tools/fuzz_trees.py makes them (thresholds that are data values, their neighbours, shared
    across trees, quantiles; leaves that end early), of which the last `deep` are full trees of depth 10 (1024 leaves: the
    second byte of a cache entry) and the first, of a forest of more than one tree, is a bare leaf; leaf values and weights
    include -0.0 and denormals."""
    n, d = X.shape
    shared = [float(v) for v in rng.normal(0, 1, 4)]

    def threshold(f):
        col = X[:, f]
        k = rng.integers(0, 5)
        if k == 0:
            return float(col[rng.integers(0, n)])
        if k == 1:
            return float(np.nextafter(np.float64(col[rng.integers(0, n)]), rng.choice([-np.inf, np.inf])))
        if k == 2:
            return shared[int(rng.integers(0, len(shared)))]
        if k == 3:
            return float(rng.choice([0.0, -0.0, 0.1, 1e-46]))
        return float(np.quantile(col.astype(np.float64), rng.random()))

    def leaf():
        return {"LeafNode": float(rng.choice([rng.uniform(-2, 4), rng.normal() * 1e-310, float(rng.choice(SPECIAL)), float(rng.integers(-3, 4))]))}

    def grow(dd, p_leaf):
        if dd == 0 or rng.random() < p_leaf:
            return leaf()
        f = int(rng.integers(0, d))
        return {"FeatureSplit": {"fid": f, "split": threshold(f), "lhs": grow(dd - 1, p_leaf), "rhs": grow(dd - 1, p_leaf)}}

    trees = []
    for t in range(count):
        if t >= count - deep:
            trees.append(grow(10, 0.0))
        elif t == 0 and count > 1:
            trees.append(leaf())
        else:
            trees.append(grow(int(rng.choice([1, 2, 3, 5])), float(rng.choice([0.0, 0.05, 0.2]))))
    weights = rng.uniform(-1, 1, count)
    pick = rng.random(count) < 0.3
    weights[pick] = rng.choice(SPECIAL, int(pick.sum()))
    return trees, weights


def _n_leaves(tree):
    if "LeafNode" in tree:
        return 1
    return _n_leaves(tree["FeatureSplit"]["lhs"]) + _n_leaves(tree["FeatureSplit"]["rhs"])


def _includes(count):
    out = [[], list(range(count)), [count // 2], list(range(0, count, 2))]
    if count > 2:
        out.append(list(range(1, count, 2)))
    return out


def _check_kernel(g, c, rows, trees, weights, n_total=None):
    """rows: the instance ids of the dataset `g`, which are also the rows of the oracle dataset `c` they are scored in."""
    leafs = [dm.leaf_numbers(t, c)[0] for t in trees]
    for include in _includes(len(trees)):
        got, cache = native.dart_scores(g, _ensemble(trees, weights), weights, include, n_total=n_total)
        kept_trees, kept_w = [trees[i] for i in include], [weights[i] for i in include]
        exp = c.score_ensemble(kept_trees, kept_w) if include else np.zeros(c.n)
        assert got[rows].tobytes() == exp[rows].tobytes(), "include %r: the kernel differs from the oracle" % (include[:4],)
        assert exp[rows].tobytes() == dm.scores(trees, weights, include, c)[rows].tobytes()
        # ... and from the re-traversal path, an independent device route
        walked = native.predict_scores_dense(_ensemble(kept_trees, kept_w) if include else fr.CModel.from_dict(EMPTY), g, n_total=n_total)
        assert got[rows].tobytes() == walked[rows].tobytes(), "include %r: the kernel differs from score_trees" % (include[:4],)
        outside = np.ones(len(got), dtype=bool)
        outside[rows] = False
        assert np.all(np.isnan(got[outside])) and np.all(cache[:, outside] == 0xFFFF)
        for t in range(len(trees)):
            assert np.array_equal(cache[t, rows], leafs[t][rows]), "cache row %d" % t


# (tree count, full depth-10 trees among them): 33 trees keep the leaf values in LDS, 130 with ten deep trees (more than
# 8192 values) take the global-memory path
FORESTS = [(1, 0), (1, 1), (2, 0), (33, 1), (130, 10)]


@pytest.mark.parametrize("count,deep", FORESTS)
def test_kernel_equals_oracle_trec(trec, count, deep):
    X, y, qid, g, c = trec
    trees, weights = _forest(np.random.default_rng(100 + count + deep), X, count, deep)
    assert (sum(_n_leaves(t) for t in trees) > 8192) == (count == 130)
    assert deep == 0 or _n_leaves(trees[-1]) == 1024
    _check_kernel(g, c, np.arange(X.shape[0]), trees, weights)


@pytest.mark.parametrize("count,deep", FORESTS)
def test_kernel_equals_oracle_synthetic(synth, count, deep):
    X, y, qid, g, c = synth
    trees, weights = _forest(np.random.default_rng(200 + count + deep), X, count, deep)
    assert native.device_form(g)["np"] > TILE  # more than one workgroup
    _check_kernel(g, c, np.arange(X.shape[0]), trees, weights)


def test_kernel_on_a_sampled_view(synth):
    """The cache is indexed by the view's own tiles: a view of every third query, and one of a single query (a few tiles of
    64: the one workgroup's tile of 1024 documents is partial)."""
    X, y, qid, g, c = synth
    names = sorted(g.queries())
    trees, weights = _forest(np.random.default_rng(5), X, 33, 1)
    for pick in (names[::3], names[1:2]):
        sub = g.subsample_queries(pick)
        f = native.device_form(sub)
        assert f["nvtiles"] > 0 and (len(pick) > 1 or f["nvtiles"] * 64 < TILE)
        rows = np.sort(np.concatenate([np.asarray(ids) for ids in sub.instances_by_query().values()])).astype(np.int64)
        _check_kernel(sub, c, rows, trees, weights, n_total=X.shape[0])


def test_kernel_on_a_file_loaded_dataset(tmp_path):
    from tests.test_gpu_lambdamart import _sparse_file

    path = str(tmp_path / "sparse.train")
    X, y, qid = _sparse_file(path)
    rd = fr.CDataset.open_ranksvm(path)
    c = o.Dataset(X, y, qid)
    feats = sorted(rd.feature_ids())
    trees, weights = _forest(np.random.default_rng(6), X[:, feats], 33, 1)

    def remap(node):
        if "FeatureSplit" in node:
            fs = node["FeatureSplit"]
            fs["fid"] = int(feats[fs["fid"]])
            remap(fs["lhs"]), remap(fs["rhs"])

    for t in trees:
        remap(t)
    _check_kernel(rd, c, np.arange(X.shape[0]), trees, weights)


# --- training, stage by stage --------------------------------------------------------------------

def _plan_events(seed, T, drop_rate, max_drop, skip_drop):
    """(some tree drops, some tree skips, some tree is cut by the cap, some tree draws an empty set without skipping)"""
    draws = dm.rand_floats(seed, T * (T + 1) // 2)
    drops = skips = capped = empty = False
    for t in range(1, T):
        at = t * (t + 1) // 2 - 1
        u, k = draws[at], int(np.sum(draws[at + 1:at + 1 + t] < drop_rate))
        if u < skip_drop:
            skips = True
            continue
        drops, capped, empty = drops or k > 0, capped or (max_drop > 0 and k > max_drop), empty or k == 0
    return drops, skips, capped, empty


def _stagewise(g, c, X, y, measure, params, names=None, n_total=None, rows=None, present=None):
    """Every tree equals the restatement's fit (tests/lambdamart_composed_model.py dispatches to the restatement of the case's
    keys) to the DEVICE's gradients of the dropped ensemble; the reported measures are those of the re-weighted ensemble,
    from the device and from the oracle; the weights are the plan's."""
    req = _request(measure, params.get("grower", "exact"), **{k: v for k, v in params.items() if k != "grower"})
    p = req.params
    cm = cmod.Composed(X, y, c, measure, dict(fr.LambdaMARTParams().to_dict(), **dict(params, grower=p.grower)), present=present, names=names)
    model = g.train_model(req)
    st = native.last_train_stats()["lambdamart"]
    d = model.to_dict()
    trees = [m["DecisionTree"] for m in d["Ensemble"]["models"]]
    T = p.num_trees
    plan = dm.plan(p.seed, p.drop_rate, p.max_drop, p.skip_drop, T, p.learning_rate)
    assert len(trees) == T and st["trees"] == T
    assert st["dropped"] == [len(D) for D, _, _ in plan]
    assert np.asarray(d["Ensemble"]["weights"], dtype=np.float64).tobytes() == plan[-1][2].tobytes()
    assert DART_STATS <= set(st) and (st["drop_rate"], st["max_drop"], st["skip_drop"]) == (p.drop_rate, p.max_drop, p.skip_drop)
    assert st["dart_ms"] > 0.0 and st["dart_cache_bytes"] >= 2 * T * X.shape[0]
    options = dict(truncation_level=p.truncation_level, lambda_norm=p.lambda_norm, objective=p.objective)
    for t in range(T):
        D, before, after = plan[t]
        keep = dm.kept(t, D)
        fsel, qsel = cm.sample(t)
        hf, hq = native.lambdamart_sample(g, p, t)
        assert np.array_equal(hf, np.asarray(cm.feats)[fsel]) and np.array_equal(hq, qsel)
        dropped_model = _ensemble([trees[i] for i in keep], before[keep]) if keep else fr.CModel.from_dict(EMPTY)
        lam, wt = native.lambda_gradients(dropped_model, g, measure, p.sigma, **options)
        exp = cm.tree(np.nan_to_num(lam), np.nan_to_num(wt), fsel, qsel)
        assert trees[t] == exp, "tree %d (fitted without %r) differs from the restatement's fit" % (t, D)
        _, per_q = native.evaluate_dense(_ensemble(trees[:t + 1], after), g, cm.reported)
        tr, va, err = cm.measures(c.score_ensemble(trees[:t + 1], after))
        assert err == 0
        if len(cm.H):
            assert st["train_measure"][t] == vm.subset_mean(per_q, cm.T) == tr, "train_measure[%d]" % t
            assert st["valid_measure"][t] == vm.subset_mean(per_q, cm.H) == va, "valid_measure[%d]" % t
        else:
            assert st["train_measure"][t] == o.mean(per_q) == tr, "train_measure[%d]" % t
    assert np.array_equal(native.predict_scores_dense(model, g), c.score_ensemble(trees, plan[-1][2]))
    return model, st, plan


@pytest.mark.parametrize("grower", ["exact", "histogram"])
def test_stagewise_identity_trec(trec, grower):
    X, y, qid, g, c = trec
    assert all(_plan_events(11, 12, **DART)[:3]), "the plan must drop, skip and hit the cap within 12 trees"
    _stagewise(g, c, X, y, "ndcg@10", dict(grower=grower, num_trees=12, seed=11, max_depth=5, min_leaf_support=5, split_candidates=16, **DART))


@pytest.mark.parametrize("grower", ["exact", "histogram"])
def test_stagewise_identity_synthetic(synth, grower):
    X, y, qid, g, c = synth
    seed = 2 ** 63 + 5
    assert all(_plan_events(seed, 10, **DART)[:3]), "the plan must drop, skip and hit the cap within ten trees"
    _stagewise(g, c, X, y, "ndcg", dict(grower=grower, num_trees=10, seed=seed, max_depth=6, min_leaf_support=10, split_candidates=64, **DART))


# --- composed with the other keys ----------------------------------------------------------------

SMALL = dict(num_trees=8, seed=3, max_depth=4, min_leaf_support=5, split_candidates=16)


@pytest.mark.parametrize("extra", [
    dict(grower="histogram", query_sampling_rate=0.5, feature_sampling_rate=0.25, validation_queries="every fifth"),
    dict(grower="exact", query_sampling_rate=0.5, feature_sampling_rate=0.25, validation_queries="every fifth"),
    dict(grower="histogram", max_leaves=6, split_gain="newton", lambda_l2=0.5),
    dict(grower="exact", objective="map"),
    dict(grower="histogram", truncation_level=5, lambda_norm=True),
], ids=["samples+holdout-hist", "samples+holdout-exact", "leafwise+newton", "map", "trunc+norm"])
def test_dart_composes_with_the_other_keys(synth, extra):
    X, y, qid, g, c = synth
    assert all(_plan_events(SMALL["seed"], SMALL["num_trees"], **DART)[:2])
    names = cmod._names(qid)
    extra = dict(extra)
    if extra.get("validation_queries"):
        extra["validation_queries"] = names[::5]
    model, st, plan = _stagewise(g, c, X, y, "ndcg@10", dict(SMALL, **DART, **extra), names=names)
    if "query_sampling_rate" in extra:
        # the drop stream is a stream of its own: without the hold-out the hook gives lambdamart_sample_model.sample's lists
        wire = _request("ndcg@10", extra["grower"], **dict(SMALL, **DART, query_sampling_rate=0.5, feature_sampling_rate=0.25)).params
        for t in range(SMALL["num_trees"]):
            fsel, qsel = sm.sample(SMALL["seed"], t, X.shape[1], len(names), (0.5, 0.25))
            hf, hq = native.lambdamart_sample(g, wire, t)
            assert np.array_equal(hf, fsel) and np.array_equal(hq, qsel)
        assert len(st["valid_measure"]) == SMALL["num_trees"] and 1 <= st["best_iteration"] <= SMALL["num_trees"]


@pytest.mark.parametrize("grower", ["exact", "histogram"])
def test_dart_on_a_sampled_view(trec, grower):
    """A view of every other query and all but one feature: its trees are the restatement's on the view's lists, its running
    scores the oracle's over the view's rows."""
    X, y, qid, g, c = trec
    names = sorted(g.queries())
    sub = g.subsample_queries(names[::2]).subsample_feature_names(sorted(g.feature_names())[1:])
    feats = sorted(sub.feature_ids())
    ids = native.hist_bins(sub, 16)[0].astype(np.int64)
    queries = np.split(ids, np.flatnonzero(np.diff(qid[ids]) != 0) + 1)
    T, seed, kw = 8, 3, dict(max_depth=4, min_leaf_support=4, split_candidates=16)
    req = _request("ndcg@10", grower, num_trees=T, seed=seed, **kw, **DART)
    model = sub.train_model(req)
    st = native.last_train_stats()["lambdamart"]
    d = model.to_dict()
    trees = [m["DecisionTree"] for m in d["Ensemble"]["models"]]
    plan = dm.plan(seed, DART["drop_rate"], DART["max_drop"], DART["skip_drop"], T, req.params.learning_rate)
    assert st["dropped"] == [len(D) for D, _, _ in plan] and any(st["dropped"])
    assert np.asarray(d["Ensemble"]["weights"]).tobytes() == plan[-1][2].tobytes()
    binned = hm.bin_matrix(X, ids, feats, 16) if grower == "histogram" else None
    everything = (np.arange(len(feats)), np.arange(len(queries)))
    for t in range(T):
        D, before, after = plan[t]
        keep = dm.kept(t, D)
        dropped_model = _ensemble([trees[i] for i in keep], before[keep]) if keep else fr.CModel.from_dict(EMPTY)
        lam, wt = native.lambda_gradients(dropped_model, sub, "ndcg@10", 1.0, n_total=X.shape[0])
        exp = sm.tree_for(grower, X, np.nan_to_num(lam), np.nan_to_num(wt), queries, feats, binned, everything[1], everything[0], 4, 4, 16)
        assert trees[t] == exp, "tree %d" % t
        _, per_q = native.evaluate_dense(_ensemble(trees[:t + 1], after), sub, "ndcg@10")
        assert st["train_measure"][t] == o.mean(per_q)
    got = native.predict_scores_dense(model, sub, n_total=X.shape[0])
    assert got[ids].tobytes() == c.score_ensemble(trees, plan[-1][2])[ids].tobytes()


# --- identities that need no restatement ---------------------------------------------------------

KW = dict(num_trees=6, max_depth=4, min_leaf_support=5, split_candidates=16)


@pytest.mark.parametrize("grower", ["exact", "histogram"])
def test_skip_drop_one_is_the_plain_model(trec, grower):
    X, y, qid, g, c = trec
    plain = g.train_model(_request("ndcg@10", grower, **KW))
    keys = set(native.last_train_stats()["lambdamart"])
    dart = g.train_model(_request("ndcg@10", grower, drop_rate=0.9, skip_drop=1.0, seed=4, **KW))
    st = native.last_train_stats()["lambdamart"]
    assert json.dumps(dart.to_dict()) == json.dumps(plain.to_dict())
    assert st["dropped"] == [0] * KW["num_trees"] and set(st) == keys | DART_STATS


@pytest.mark.parametrize("grower", ["exact", "histogram"])
def test_dropping_everything_repeats_the_first_tree(synth, grower):
    """drop_rate 1, no skips, no cap, no samples: every tree is fitted at scores 0.0, so every tree is tree 0."""
    X, y, qid, g, c = synth
    T = KW["num_trees"]
    model = g.train_model(_request("ndcg", grower, drop_rate=1.0, skip_drop=0.0, max_drop=0, learning_rate=0.3, **KW))
    st = native.last_train_stats()["lambdamart"]
    d = model.to_dict()["Ensemble"]
    first = g.train_model(_request("ndcg", grower, learning_rate=0.3, **dict(KW, num_trees=1))).to_dict()["Ensemble"]["models"][0]
    assert "FeatureSplit" in first["DecisionTree"] and all(m == first for m in d["models"])
    plan = dm.plan(0, 1.0, 0, 0.0, T, 0.3)
    assert st["dropped"] == list(range(T)) and np.asarray(d["weights"]).tobytes() == plan[-1][2].tobytes()
    assert np.array_equal(native.predict_scores_dense(model, g), c.score_ensemble([m["DecisionTree"] for m in d["models"]], d["weights"]))


@pytest.mark.parametrize("grower", ["exact", "histogram"])
def test_a_second_run_gives_the_same_bytes(synth, grower):
    X, y, qid, g, c = synth
    req = _request("ndcg@10", grower, seed=9, query_sampling_rate=0.5, **KW, **DART)
    a = json.dumps(g.train_model(req).to_dict())
    sa = native.last_train_stats()["lambdamart"]
    b = json.dumps(g.train_model(req).to_dict())
    sb = native.last_train_stats()["lambdamart"]
    assert a == b and sa["dropped"] == sb["dropped"] and sa["train_measure"] == sb["train_measure"] and any(sa["dropped"])
    other = json.dumps(g.train_model(_request("ndcg@10", grower, seed=10, query_sampling_rate=0.5, **KW, **DART)).to_dict())
    assert other != a


@pytest.mark.parametrize("grower", ["exact", "histogram"])
def test_no_keys_is_the_request_it_was(trec, grower):
    """Without the keys, and with them spelled at their defaults, the model bytes and the stats' key set are what they
    are without DART; the weights stay uniform."""
    X, y, qid, g, c = trec
    absent = _request("ndcg@10", grower, **KW)
    assert not set(absent.to_dict()["params"]["LambdaMART"]) & {"drop_rate", "max_drop", "skip_drop"}
    a = g.train_model(absent)
    keys = set(native.last_train_stats()["lambdamart"])
    base = {"trees", "seconds", "gradient_ms", "grow_ms", "leaves_ms", "update_ms", "grower", "bins_ms", "train_measure"}
    assert keys == base | ({"bins"} if grower == "histogram" else set()) and not keys & DART_STATS
    assert a.to_dict()["Ensemble"]["weights"] == [absent.params.learning_rate] * KW["num_trees"]
    for spelled in (dict(drop_rate=0.0), dict(drop_rate=0, max_drop=50, skip_drop=0.5)):
        wire = absent.to_dict()
        wire["params"]["LambdaMART"].update(spelled)
        m = fr.CModel(clib._unwrap(clib._load().train_model(json.dumps(wire).encode(), g.pointer)))
        assert json.dumps(m.to_dict()) == json.dumps(a.to_dict())
        assert set(native.last_train_stats()["lambdamart"]) == keys


def test_a_tree_of_65536_leaves_fits_the_cache_and_one_more_is_refused(synth):
    """A cache entry is 16 bits: the full tree of depth 16 is the largest that fits, with one leaf more the fill is a plain error."""
    X, y, qid, g, c = synth
    cuts = np.quantile(X[:, 0].astype(np.float64), np.linspace(0.0, 1.0, 2 ** 16 + 1)[1:-1])

    def grow(lo, hi):  # leaves lo .. hi - 1, split at the quantile between the halves: the documents spread over all of them
        if hi - lo == 1:
            return {"LeafNode": float(lo) * 0.5}
        mid = (lo + hi) // 2
        return {"FeatureSplit": {"fid": 0, "split": float(cuts[mid - 1]), "lhs": grow(lo, mid), "rhs": grow(mid, hi)}}

    full = grow(0, 2 ** 16)
    got, cache = native.dart_scores(g, _ensemble([full], [1.0]), [2.0], [0])
    assert got.tobytes() == c.score_ensemble([full], [2.0]).tobytes()
    assert np.array_equal(cache[0], dm.leaf_numbers(full, c)[0]) and cache[0].max() > 60000
    node = full
    while "FeatureSplit" in node["FeatureSplit"]["rhs"]:
        node = node["FeatureSplit"]["rhs"]
    node["FeatureSplit"]["rhs"] = {"FeatureSplit": {"fid": 1, "split": 0.0, "lhs": {"LeafNode": 1.0}, "rhs": {"LeafNode": 2.0}}}
    with pytest.raises(Exception, match="65537 leaves does not fit the leaf cache"):
        native.dart_scores(g, _ensemble([full], [1.0]), [2.0], [0])


# --- the 30K shape -------------------------------------------------------------------------------

def test_30k_shape_view_running_scores_equal_prediction_and_oracle():
    """The 30K shape on a view of every tenth query (about 380 000 documents, several hundred workgroups of the kernel): five
    default histogram trees under DART; the reported measure is the prediction's, the prediction is the oracle's."""
    from tests.test_gpu_fullsize import _shape

    _, X, y, qid, g = _shape("30k")
    names = sorted(g.queries())
    sub = g.subsample_queries(names[::10])
    ids = np.sort(np.concatenate([np.asarray(v) for v in sub.instances_by_query().values()])).astype(np.int64)
    assert len(ids) > 300_000
    seed = 2
    assert all(_plan_events(seed, 5, 0.5, 3, 0.0)[:1])
    req = _request("ndcg@10", "histogram", num_trees=5, split_candidates=64, seed=seed, drop_rate=0.5, skip_drop=0.0, max_drop=3)
    model = sub.train_model(req)
    st = native.last_train_stats()["lambdamart"]
    d = model.to_dict()["Ensemble"]
    trees = [m["DecisionTree"] for m in d["models"]]
    plan = dm.plan(seed, 0.5, 3, 0.0, 5, req.params.learning_rate)
    assert st["dropped"] == [len(D) for D, _, _ in plan] and any(st["dropped"])
    assert np.asarray(d["weights"]).tobytes() == plan[-1][2].tobytes()
    assert st["dart_cache_bytes"] >= 2 * 5 * len(ids)
    c = o.Dataset(X[ids], y[ids], qid[ids])
    got = native.predict_scores_dense(model, sub, n_total=X.shape[0])
    assert got[ids].tobytes() == c.score_ensemble(trees, d["weights"]).tobytes()
    o.set_mean_segment(o.DEVICE_MEAN_SEGMENT)
    try:
        for t in (0, 4):
            _, per_q = native.evaluate_dense(_ensemble(trees[:t + 1], plan[t][2]), sub, "ndcg@10")
            assert st["train_measure"][t] == o.mean(per_q)
    finally:
        o.set_mean_segment(0)
