"""LambdaMART's per-tree query and feature samples without a GPU ("Sampling"): the three optional
wire keys and their validation (every request here fails or is only parsed before any device work), the samples the
trainer would draw (native.lambdamart_sample) against the restatement (tests/lambdamart_sample_model.py), and the
restatement's own properties."""
import json

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import clib, native
from fastrank_amd.training import LambdaMARTParams, TrainRequest
from oracle import pyoracle as o
from tests import lambdamart_model as lm
from tests import lambdamart_sample_model as sm
from tests.conftest import synth_dataset

KEYS = ["num_trees", "learning_rate", "max_depth", "min_leaf_support", "split_candidates", "sigma", "quiet"]
NEW = ["query_sampling_rate", "feature_sampling_rate", "seed"]
DEFAULTS_TEXT = ('{"measure": "ndcg", "params": {"LambdaMART": {"num_trees": 100, "learning_rate": 0.1, "max_depth": 6, '
                 '"min_leaf_support": 10, "split_candidates": 64, "sigma": 1.0, "quiet": false}}, "judgments": null}')


def _dataset():
    X = np.arange(24, dtype=np.float32).reshape(8, 3)
    y = np.array([0, 1, 2, 0, 1, 0, 0, 1], dtype=np.float64)
    qid = np.array([1, 1, 1, 1, 2, 2, 2, 2], dtype=np.int64)
    return fr.CDataset.from_numpy(X, y, qid)


def _train_raw(params, measure="ndcg"):
    ds = _dataset()
    text = json.dumps({"measure": measure, "params": {"LambdaMART": params}, "judgments": None}).encode()
    return clib._unwrap(clib._load().train_model(text, ds.pointer))


def _params(**kw):
    p = LambdaMARTParams().to_dict()
    p.update(kw)
    return p


# --- wire form ---------------------------------------------------------------------------------

def test_defaults_and_existing_wire_forms_keep_their_bytes():
    assert json.dumps(clib.query_json("lambdamart_defaults")) == DEFAULTS_TEXT
    assert json.dumps(TrainRequest.lambdamart().to_dict()) == DEFAULTS_TEXT
    assert list(LambdaMARTParams().to_dict().keys()) == KEYS
    assert list(LambdaMARTParams(grower="histogram").to_dict().keys()) == KEYS + ["grower"]
    p = LambdaMARTParams()
    assert (p.query_sampling_rate, p.feature_sampling_rate, p.seed) == (1.0, 1.0, 0)
    # explicit defaults are not written either
    assert list(LambdaMARTParams(query_sampling_rate=1.0, feature_sampling_rate=1.0, seed=0).to_dict().keys()) == KEYS


@pytest.mark.parametrize("kw", [dict(query_sampling_rate=0.5), dict(feature_sampling_rate=0.25), dict(seed=2 ** 64 - 1),
                                dict(query_sampling_rate=0.5, feature_sampling_rate=0.3, seed=7, grower="histogram")])
def test_the_three_keys_round_trip_and_are_absent_at_their_defaults(kw):
    req = TrainRequest.lambdamart()
    for k, v in kw.items():
        setattr(req.params, k, v)
    d = req.to_dict()
    wire = d["params"]["LambdaMART"]
    order = [k for k in ["grower"] + NEW if k in kw]
    assert list(wire.keys()) == KEYS + order
    for k, v in kw.items():
        assert wire[k] == v
    back = TrainRequest.from_dict(json.loads(json.dumps(d)))
    assert back == req and back.to_dict() == d
    c = req.clone()
    assert c == req and c.params is not req.params and c != TrainRequest.lambdamart()


def test_explicit_defaults_on_the_wire_read_back_as_defaults():
    d = TrainRequest.lambdamart().to_dict()
    d["params"]["LambdaMART"].update(query_sampling_rate=1.0, feature_sampling_rate=1.0, seed=0)
    assert TrainRequest.from_dict(d) == TrainRequest.lambdamart()
    assert json.dumps(TrainRequest.from_dict(d).to_dict()) == DEFAULTS_TEXT


@pytest.mark.parametrize("key", ["query_sampling_rate", "feature_sampling_rate"])
@pytest.mark.parametrize("value", [0, 0.0, -0.5, 1.5, 1.0000001, -1e-300])
def test_rate_out_of_range_is_rejected(key, value):
    with pytest.raises(Exception, match="invalid value") as e:
        _train_raw(_params(**{key: value}))
    assert key + " must be greater than 0 and at most 1" in str(e.value)


@pytest.mark.parametrize("key", ["query_sampling_rate", "feature_sampling_rate"])
@pytest.mark.parametrize("value", ["0.5", None, True, [0.5], {"rate": 0.5}])
def test_rate_of_the_wrong_type_is_rejected(key, value):
    with pytest.raises(Exception, match="invalid type") as e:
        _train_raw(_params(**{key: value}))
    assert "expected f64 for " + key in str(e.value)


@pytest.mark.parametrize("key", ["query_sampling_rate", "feature_sampling_rate"])
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
def test_rate_not_finite_is_rejected(key, value):
    """JSON has no spelling for NaN or an infinity: Python writes NaN / Infinity, which the parser refuses for any key (so
    this holds without the feature as well; the literals JSON does have are the two tests below)."""
    with pytest.raises(Exception, match="Error"):
        _train_raw(_params(**{key: value}))


def _train_literal(key, literal):
    """The request with `literal` as the text of `key`'s value (written by hand: json.dumps has no such literals)."""
    text = json.dumps({"measure": "ndcg", "params": {"LambdaMART": _params(**{key: 0.123456})}, "judgments": None})
    assert text.count("0.123456") == 1
    ds = _dataset()
    return clib._unwrap(clib._load().train_model(text.replace("0.123456", literal).encode(), ds.pointer))


@pytest.mark.parametrize("key", ["query_sampling_rate", "feature_sampling_rate"])
@pytest.mark.parametrize("literal", ["1.7976931348623157e308", "-1.7976931348623157e308", "1e-999", "-0.0", "2"])
def test_rate_literal_outside_the_range_is_rejected(key, literal):
    """What JSON can spell and f64 can hold: the largest finite numbers, a literal too small for f64 (reads as zero), a
    negative zero, an integer: all fail the range check with the `invalid value` envelope."""
    with pytest.raises(Exception, match="invalid value") as e:
        _train_literal(key, literal)
    assert key + " must be greater than 0 and at most 1" in str(e.value)


@pytest.mark.parametrize("key", ["query_sampling_rate", "feature_sampling_rate"])
@pytest.mark.parametrize("literal", ["1e999", "-1e999"])
def test_rate_literal_too_large_for_f64_never_becomes_an_infinity(key, literal):
    """The request parser refuses a number that f64 cannot hold (`number out of range`, as for every other key), so no
    infinity can reach the range check."""
    with pytest.raises(Exception, match="number out of range"):
        _train_literal(key, literal)


@pytest.mark.parametrize("value", [-1, 1.5, 0.0, "3", None, True, 2 ** 64])
def test_bad_seed_is_rejected(value):
    with pytest.raises(Exception, match="invalid type") as e:
        _train_raw(_params(seed=value))
    assert "expected unsigned integer for seed" in str(e.value)


def test_valid_keys_reach_the_later_checks():
    ok = dict(query_sampling_rate=0.5, feature_sampling_rate=1, seed=2 ** 64 - 1)
    with pytest.raises(Exception, match=r"supported: ndcg, ndcg@k"):
        _train_raw(_params(**ok), "map")
    with pytest.raises(Exception, match="num_trees must be at least 1"):
        _train_raw(_params(num_trees=0, **ok))
    for key in KEYS:  # the seven keys stay required
        p = _params(**ok)
        del p[key]
        with pytest.raises(Exception, match="missing field `%s`" % key):
            _train_raw(p)


# --- the samples the trainer draws --------------------------------------------------------------

def _sized(nF, nQ):
    rng = np.random.default_rng(nF * 100 + nQ)
    lens = rng.integers(1, 6, nQ)
    qid = np.repeat(np.arange(10, 10 + nQ, dtype=np.int64), lens)
    n = len(qid)
    X = rng.random((n, nF)).astype(np.float32)
    y = rng.integers(0, 3, n).astype(np.float64)
    return fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)


@pytest.fixture(scope="module", params=[(nF, nQ) for nF in (1, 3, 136) for nQ in (1, 2, 50)], ids=lambda p: "F%d-Q%d" % p)
def sized(request):
    nF, nQ = request.param
    return (nF, nQ) + _sized(nF, nQ)


RATES = [(1.0, 1.0), (0.5, 1.0), (1.0, 0.3), (0.5, 0.25), (0.01, 0.01), (0.99, 0.99)]


@pytest.mark.parametrize("seed", [0, 7, 2 ** 64 - 1])
@pytest.mark.parametrize("rates", RATES)
def test_sample_hook_equals_restatement(sized, seed, rates):
    nF, nQ, g, c = sized
    p = LambdaMARTParams(query_sampling_rate=rates[0], feature_sampling_rate=rates[1], seed=seed)
    feats = np.array(sorted(g.feature_ids()))
    for t in (0, 1, 5):
        f, q = native.lambdamart_sample(g, p, t)
        ef, eq = sm.sample(seed, t, nF, nQ, rates)
        assert np.array_equal(f, feats[ef]) and np.array_equal(q, eq)
        assert len(f) == sm.count(nF, rates[1]) and len(q) == sm.count(nQ, rates[0])
        assert np.all(np.diff(f.astype(np.int64)) > 0) and np.all(np.diff(q.astype(np.int64)) > 0)
        if rates[1] == 1.0:
            assert np.array_equal(f, feats)
        if rates[0] == 1.0:
            assert np.array_equal(q, np.arange(nQ))


def test_count_is_the_random_forest_rule():
    for n, r, exp in ((136, 0.25, 34), (136, 0.5, 68), (3, 0.3, 1), (3, 0.99, 2), (1, 0.01, 1), (50, 0.5, 25), (50, 0.01, 1),
                      (50, 1.0, 50), (7, 0.999999, 6), (10, 0.3, 3), (2, 0.5, 1)):
        assert sm.count(n, r) == exp, (n, r)


def test_query_sample_does_not_depend_on_the_feature_rate(sized):
    nF, nQ, g, c = sized
    for t in range(4):
        a = native.lambdamart_sample(g, LambdaMARTParams(query_sampling_rate=0.5, feature_sampling_rate=1.0, seed=11), t)[1]
        b = native.lambdamart_sample(g, LambdaMARTParams(query_sampling_rate=0.5, feature_sampling_rate=0.3, seed=11), t)[1]
        assert np.array_equal(a, b)
        fa = native.lambdamart_sample(g, LambdaMARTParams(query_sampling_rate=1.0, feature_sampling_rate=0.3, seed=11), t)[0]
        fb = native.lambdamart_sample(g, LambdaMARTParams(query_sampling_rate=0.5, feature_sampling_rate=0.3, seed=11), t)[0]
        assert np.array_equal(fa, fb)


def test_trees_and_seeds_differ():
    g, c = _sized(136, 50)
    p = LambdaMARTParams(query_sampling_rate=0.5, feature_sampling_rate=0.25, seed=3)
    per_tree = [native.lambdamart_sample(g, p, t) for t in range(6)]
    for a in range(6):
        for b in range(a + 1, 6):
            assert not np.array_equal(per_tree[a][0], per_tree[b][0])
            assert not np.array_equal(per_tree[a][1], per_tree[b][1])
    other = native.lambdamart_sample(g, LambdaMARTParams(query_sampling_rate=0.5, feature_sampling_rate=0.25, seed=4), 0)
    assert not np.array_equal(other[0], per_tree[0][0]) and not np.array_equal(other[1], per_tree[0][1])
    # a feature sample and the query sample of one tree come from different seeds
    g2, _ = _sized(50, 50)
    f, q = native.lambdamart_sample(g2, LambdaMARTParams(query_sampling_rate=0.5, feature_sampling_rate=0.5, seed=3), 0)
    assert not np.array_equal(f, q)


def test_sample_of_a_view_indexes_the_views_lists():
    g, c = _sized(136, 50)
    names = sorted(g.queries())
    sub = g.subsample_queries(names[::2]).subsample_feature_names(sorted(g.feature_names())[1::2])
    p = LambdaMARTParams(query_sampling_rate=0.5, feature_sampling_rate=0.5, seed=9)
    f, q = native.lambdamart_sample(sub, p, 2)
    feats = np.array(sorted(sub.feature_ids()))
    ef, eq = sm.sample(9, 2, len(feats), len(names[::2]), (0.5, 0.5))
    assert np.array_equal(f, feats[ef]) and np.array_equal(q, eq)


def test_sample_hook_validates_like_a_request():
    g, _ = _sized(3, 2)
    with pytest.raises(Exception, match="invalid value"):
        native.lambdamart_sample(g, _params(query_sampling_rate=0.0), 0)
    with pytest.raises(Exception, match="missing field `learning_rate`"):
        native.lambdamart_sample(g, {"num_trees": 1}, 0)


# --- the restatement's own properties ----------------------------------------------------------

def test_sampled_instance_list_is_a_subsequence_of_the_full_one():
    X, y, qid = synth_dataset(3, 600, 5, 30)
    c = o.Dataset(X, y, qid)
    queries = lm.query_lists(c)
    full = np.concatenate(queries)
    for t in range(5):
        _, qsel = sm.sample(5, t, 5, len(queries), (0.4, 1.0))
        rows = sm.instance_rows(queries, qsel)
        assert np.all(np.diff(rows) > 0) and len(rows) == sum(len(queries[q]) for q in qsel)
        assert np.array_equal(full[rows], np.concatenate([queries[q] for q in qsel]))


@pytest.mark.parametrize("grower", ["exact", "histogram"])
def test_restatement_with_full_rates_is_the_unsampled_restatement(grower):
    from tests import lambdamart_hist_model as hm

    X, y, qid = synth_dataset(4, 300, 4, 12)
    c = o.Dataset(X, y, qid)
    kw = dict(measure="ndcg@5", num_trees=3, max_depth=3, min_leaf_support=5, split_candidates=8)
    model, s, _, samples = sm.train(X, y, c, grower=grower, rates=(1.0, 1.0), seed=99, **kw)
    ref = (hm if grower == "histogram" else lm).train(X, y, c, **kw)
    assert model == ref[0] and np.array_equal(s, ref[1])
    assert all(len(f) == 4 and len(q) == 12 for f, q in samples)


@pytest.mark.parametrize("grower", ["exact", "histogram"])
def test_restatement_trees_use_only_their_sample(grower):
    X, y, qid = synth_dataset(6, 800, 8, 40)
    c = o.Dataset(X, y, qid)
    model, s, measures, samples = sm.train(X, y, c, grower=grower, measure="ndcg@10", num_trees=4, max_depth=4, min_leaf_support=5,
                                           split_candidates=16, rates=(0.5, 0.25), seed=1)

    def fids(node):
        if "LeafNode" in node:
            return set()
        fs = node["FeatureSplit"]
        return {fs["fid"]} | fids(fs["lhs"]) | fids(fs["rhs"])

    for m, (fsel, qsel) in zip(model["Ensemble"]["models"], samples):
        assert fids(m["DecisionTree"]) <= set(int(f) for f in fsel)
        assert len(fsel) == 2 and len(qsel) == 20
    assert any(fids(m["DecisionTree"]) for m in model["Ensemble"]["models"])
    assert np.array_equal(s, c.score_ensemble([m["DecisionTree"] for m in model["Ensemble"]["models"]], model["Ensemble"]["weights"]))
    other = sm.train(X, y, c, grower=grower, measure="ndcg@10", num_trees=4, max_depth=4, min_leaf_support=5,
                     split_candidates=16, rates=(0.5, 0.25), seed=2)[0]
    assert other != model
