"""LambdaMART's held-out validation queries and early stopping without a GPU ("Validation and early
stopping"): the two optional wire keys and their validation (every request here fails or is only parsed before any device
work), the samples the trainer would draw from the training queries, the split helper, and the restatement's own properties
(tests/lambdamart_valid_model.py)."""
import json

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import clib, native
from fastrank_amd.training import LambdaMARTParams, TrainRequest, hold_out_queries
from oracle import pyoracle as o
from tests import lambdamart_sample_model as sm
from tests import lambdamart_valid_model as vm
from tests.conftest import synth_dataset

KEYS = ["num_trees", "learning_rate", "max_depth", "min_leaf_support", "split_candidates", "sigma", "quiet"]
DEFAULTS_TEXT = ('{"measure": "ndcg", "params": {"LambdaMART": {"num_trees": 100, "learning_rate": 0.1, "max_depth": 6, '
                 '"min_leaf_support": 10, "split_candidates": 64, "sigma": 1.0, "quiet": false}}, "judgments": null}')


def _dataset():
    X = np.arange(36, dtype=np.float32).reshape(12, 3)
    y = np.array([0, 1, 2, 0, 1, 0, 0, 1, 2, 1, 0, 0], dtype=np.float64)
    qid = np.array([7, 7, 7, 7, 3, 3, 3, 3, 11, 11, 11, 11], dtype=np.int64)
    return fr.CDataset.from_numpy(X, y, qid)


def _train_raw(params, measure="ndcg", ds=None):
    ds = ds if ds is not None else _dataset()
    text = json.dumps({"measure": measure, "params": {"LambdaMART": params}, "judgments": None}).encode()
    return clib._unwrap(clib._load().train_model(text, ds.pointer))


def _params(**kw):
    p = LambdaMARTParams().to_dict()
    p.update(kw)
    return p


# --- wire form ---------------------------------------------------------------------------------

def test_keys_are_absent_at_their_defaults_and_existing_wire_forms_keep_their_bytes():
    assert json.dumps(clib.query_json("lambdamart_defaults")) == DEFAULTS_TEXT
    assert json.dumps(TrainRequest.lambdamart().to_dict()) == DEFAULTS_TEXT
    assert list(LambdaMARTParams().to_dict().keys()) == KEYS
    p = LambdaMARTParams()
    assert p.validation_queries == [] and p.early_stopping_rounds == 0
    assert list(LambdaMARTParams(validation_queries=[], early_stopping_rounds=0).to_dict().keys()) == KEYS
    assert list(LambdaMARTParams(grower="histogram", seed=3).to_dict().keys()) == KEYS + ["grower", "seed"]
    # the default list is not shared between instances
    p.validation_queries.append("1")
    assert LambdaMARTParams().validation_queries == []


@pytest.mark.parametrize("kw", [dict(validation_queries=["3"]), dict(validation_queries=["11", "7"], early_stopping_rounds=5),
                                dict(validation_queries=["3"], early_stopping_rounds=2 ** 32 - 1, grower="histogram",
                                     query_sampling_rate=0.5, seed=9)])
def test_the_keys_round_trip_and_clone(kw):
    req = TrainRequest.lambdamart()
    for k, v in kw.items():
        setattr(req.params, k, v)
    d = req.to_dict()
    wire = d["params"]["LambdaMART"]
    order = [k for k in ["grower", "query_sampling_rate", "feature_sampling_rate", "seed", "validation_queries", "early_stopping_rounds"] if k in kw]
    assert list(wire.keys()) == KEYS + order
    for k, v in kw.items():
        assert wire[k] == v
    back = TrainRequest.from_dict(json.loads(json.dumps(d)))
    assert back == req and back.to_dict() == d
    c = req.clone()
    assert c == req and c.params is not req.params and c != TrainRequest.lambdamart()
    assert c.params.validation_queries is not req.params.validation_queries


def test_explicit_defaults_on_the_wire_read_back_as_defaults():
    d = TrainRequest.lambdamart().to_dict()
    d["params"]["LambdaMART"].update(validation_queries=[], early_stopping_rounds=0)
    assert TrainRequest.from_dict(d) == TrainRequest.lambdamart()
    assert json.dumps(TrainRequest.from_dict(d).to_dict()) == DEFAULTS_TEXT


def test_the_native_side_writes_the_keys_only_when_set():
    """The sample hook parses the payload with the request's parser: what it accepts is what train_model accepts."""
    g = _dataset()
    f, q = native.lambdamart_sample(g, _params(validation_queries=["3"], early_stopping_rounds=4), 0)
    assert list(q) == [0, 2]  # (the view's order is 7, 3, 11: query 1 is held out)


# --- errors, all before any device work ----------------------------------------------------------

@pytest.mark.parametrize("value", ["3", 3, None, True, {"3": 1}, 0.5])
def test_validation_queries_of_the_wrong_type_is_rejected(value):
    with pytest.raises(Exception, match="invalid type") as e:
        _train_raw(_params(validation_queries=value))
    assert "expected an array of strings for validation_queries" in str(e.value)


@pytest.mark.parametrize("value", [[3], ["3", 7], [None], [["3"]], [True], [1.5]])
def test_a_non_string_entry_is_rejected(value):
    with pytest.raises(Exception, match="invalid type") as e:
        _train_raw(_params(validation_queries=value))
    assert "expected a string for every entry of validation_queries" in str(e.value)


@pytest.mark.parametrize("bad", ["4", "03", " 3", "", "seven"])
def test_an_id_that_is_not_a_query_is_rejected_by_name(bad):
    with pytest.raises(Exception, match="invalid value") as e:
        _train_raw(_params(validation_queries=["3", bad]))
    assert "validation_queries names `%s`, which is not a query of the dataset" % bad in str(e.value)


def test_an_id_outside_a_sampled_view_is_rejected():
    g = _dataset()
    sub = g.subsample_queries(["7", "11"])
    with pytest.raises(Exception, match="validation_queries names `3`, which is not a query of the dataset"):
        _train_raw(_params(validation_queries=["3"]), ds=sub)
    f, q = native.lambdamart_sample(sub, _params(validation_queries=["11"]), 0)
    assert list(q) == [0]


def test_a_repeated_id_is_rejected():
    with pytest.raises(Exception, match="invalid value") as e:
        _train_raw(_params(validation_queries=["3", "7", "3"]))
    assert "validation_queries names query `3` more than once" in str(e.value)


def test_holding_out_every_query_is_rejected():
    with pytest.raises(Exception, match="invalid value") as e:
        _train_raw(_params(validation_queries=["3", "7", "11"]))
    assert "no training query left" in str(e.value)
    one = fr.CDataset.from_numpy(np.ones((2, 1), dtype=np.float32), np.array([0.0, 1.0]), np.array([5, 5], dtype=np.int64))
    with pytest.raises(Exception, match="no training query left"):
        _train_raw(_params(validation_queries=["5"]), ds=one)


@pytest.mark.parametrize("r", [1, 10, 2 ** 32 - 1])
def test_early_stopping_without_a_validation_query_is_rejected(r):
    for extra in ({}, {"validation_queries": []}):
        with pytest.raises(Exception, match="invalid value") as e:
            _train_raw(_params(early_stopping_rounds=r, **extra))
        assert "early_stopping_rounds needs at least one validation query" in str(e.value)


@pytest.mark.parametrize("value", [-1, 1.5, "3", None, True, 2 ** 32, [1]])
def test_bad_early_stopping_rounds_is_rejected(value):
    # (the parser's own words for a u32: a value that does not fit is an `invalid value`, any other kind an `invalid type`)
    with pytest.raises(Exception, match="invalid value" if value == 2 ** 32 else "invalid type") as e:
        _train_raw(_params(validation_queries=["3"], early_stopping_rounds=value))
    assert "u32" in str(e.value) or "early_stopping_rounds" in str(e.value)


def test_valid_keys_reach_the_later_checks():
    ok = dict(validation_queries=["3", "11"], early_stopping_rounds=3)
    with pytest.raises(Exception, match=r"supported: ndcg, ndcg@k"):
        _train_raw(_params(**ok), "map")
    with pytest.raises(Exception, match="num_trees must be at least 1"):
        _train_raw(_params(num_trees=0, **ok))
    with pytest.raises(Exception, match="query_sampling_rate must be greater than 0 and at most 1"):
        _train_raw(_params(query_sampling_rate=0.0, **ok))
    for key in KEYS:  # the seven keys stay required
        p = _params(**ok)
        del p[key]
        with pytest.raises(Exception, match="missing field `%s`" % key):
            _train_raw(p)


# --- the samples the trainer draws from the training queries ---------------------------------------

def _sized(nF, nQ):
    rng = np.random.default_rng(nF * 100 + nQ)
    lens = rng.integers(1, 6, nQ)
    # ids in no numeric order: the view's order is first appearance
    ids = rng.permutation(np.arange(100, 100 + nQ, dtype=np.int64))
    qid = np.repeat(ids, lens)
    n = len(qid)
    X = rng.random((n, nF)).astype(np.float32)
    y = rng.integers(0, 3, n).astype(np.float64)
    return fr.CDataset.from_numpy(X, y, qid), [str(int(i)) for i in ids]


@pytest.mark.parametrize("rates", [(1.0, 1.0), (0.5, 1.0), (1.0, 0.3), (0.5, 0.25), (0.01, 0.5)])
@pytest.mark.parametrize("nQ,step", [(2, 2), (50, 2), (50, 7), (51, 50)])
def test_sample_hook_draws_from_the_training_queries(rates, nQ, step):
    g, names = _sized(5, nQ)
    assert set(g.queries()) == set(names)  # (spelling; the view's order is first appearance)
    held = names[1::step]
    T, H = vm.split(names, held)
    assert len(T) + len(H) == nQ and len(H) == len(held)
    feats = np.array(sorted(g.feature_ids()))
    # the order in which the ids are given does not matter
    p = LambdaMARTParams(query_sampling_rate=rates[0], feature_sampling_rate=rates[1], seed=17, validation_queries=held[::-1])
    without = LambdaMARTParams(query_sampling_rate=rates[0], feature_sampling_rate=rates[1], seed=17)
    for t in (0, 1, 4):
        f, q = native.lambdamart_sample(g, p, t)
        ef, eq = vm.sample(17, t, 5, T, rates)
        assert np.array_equal(f, feats[ef]) and np.array_equal(q, eq)
        assert not set(q.tolist()) & set(H.tolist()) and np.all(np.diff(q.astype(np.int64)) > 0)
        assert len(q) == sm.count(len(T), rates[0])
        # the feature sample is the one of the request without a hold-out: the master generator hands out the same seeds
        assert np.array_equal(f, native.lambdamart_sample(g, without, t)[0])
        if rates[0] == 1.0:
            assert np.array_equal(q, T)


# --- hold_out_queries ----------------------------------------------------------------------------

def test_hold_out_queries_bounds_determinism_and_order():
    names = [str(x) for x in np.random.default_rng(1).permutation(1000)]
    for rate, n in ((0.1, 100), (0.5, 500), (0.0005, 1), (0.9999, 999), (0.25, 250)):
        a = hold_out_queries(names, rate, 7)
        assert len(a) == n and len(set(a)) == n and set(a) <= set(names)
        pos = [names.index(q) for q in a]
        assert pos == sorted(pos), "the result keeps the given order"
        assert a == hold_out_queries(names, rate, 7) == hold_out_queries(tuple(names), rate, 7)
    assert hold_out_queries(names, 0.1, 7) != hold_out_queries(names, 0.1, 8)
    assert hold_out_queries(["a", "b"], 0.01) in (["a"], ["b"]) and hold_out_queries(["a", "b"], 0.99) in (["a"], ["b"])
    assert len(hold_out_queries(["a", "b", "c"], 0.99)) == 2
    assert hold_out_queries(names, 0.1) == hold_out_queries(names, 0.1, 0)
    # a set has no order of its own (CDataset.queries() is one): it is sorted first, so the split is still a function of the arguments
    assert hold_out_queries(set(names), 0.1, 7) == hold_out_queries(sorted(names), 0.1, 7)
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            hold_out_queries(names, bad)
    for few in ([], ["a"]):
        with pytest.raises(ValueError):
            hold_out_queries(few, 0.5)
    # what it returns is a request the library accepts as far as a CPU can tell
    g, ids = _sized(3, 20)
    held = hold_out_queries(g.queries(), 0.3, 1)
    assert len(held) == 6
    assert len(native.lambdamart_sample(g, LambdaMARTParams(validation_queries=held), 0)[1]) == 14


# --- the restatement's own properties ----------------------------------------------------------

@pytest.mark.parametrize("rates", [(1.0, 1.0), (0.5, 0.5)])
@pytest.mark.parametrize("grower", ["exact", "histogram"])
def test_restatement_without_held_out_queries_is_the_sampled_restatement(grower, rates):
    X, y, qid = synth_dataset(4, 300, 4, 12)
    c = o.Dataset(X, y, qid)
    kw = dict(measure="ndcg@5", num_trees=3, max_depth=3, min_leaf_support=5, split_candidates=8, grower=grower, rates=rates, seed=99)
    r = vm.train(X, y, c, (), **kw)
    model, s, measures, samples = sm.train(X, y, c, **kw)
    assert r["model"] == model and np.array_equal(r["scores"], s)
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(r["samples"], samples))
    # (sm.train reports numpy's pairwise mean, this one the project's sequential one: 12 values in [0, 1])
    assert np.allclose(r["train_measure"], measures, rtol=0, atol=12 * 2.0 ** -52)
    assert r["valid_measure"] == [] and r["trees"] == 3 and not r["stopped_early"]


@pytest.mark.parametrize("grower", ["exact", "histogram"])
def test_restatement_trees_do_not_depend_on_held_out_labels(grower):
    X, y, qid = synth_dataset(6, 800, 6, 40)
    c = o.Dataset(X, y, qid)
    H = list(range(0, 40, 3))
    kw = dict(measure="ndcg@10", num_trees=4, max_depth=4, min_leaf_support=5, split_candidates=16, grower=grower)
    a = vm.train(X, y, c, H, **kw)
    y2 = y.copy()
    rows = np.isin(qid, np.unique(qid)[H]) if np.all(np.diff(qid) >= 0) else None
    assert rows is not None
    y2[rows] = (y2[rows] + 1) % 3
    b = vm.train(X, y2, o.Dataset(X, y2, qid), H, **kw)
    assert a["model"] == b["model"] and a["train_measure"] == b["train_measure"]
    assert a["valid_measure"] != b["valid_measure"]
    for fsel, qsel in a["samples"]:
        assert not set(qsel.tolist()) & set(H)
    # the truncated model is the model of the shorter training
    full = vm.train(X, y, c, H, early_stopping_rounds=1, **kw)
    short = vm.train(X, y, c, H, **dict(kw, num_trees=full["best_iteration"]))
    assert full["model"] == short["model"] and np.array_equal(full["scores"], short["scores"])


def test_subset_means_have_the_compacted_two_level_shape():
    rng = np.random.default_rng(3)
    per_q = rng.random(700)
    H = np.sort(rng.choice(700, 300, replace=False))
    T = np.setdiff1d(np.arange(700), H)

    def two_level(v):
        parts = []
        for b in range(0, len(v), 256):
            s = 0.0
            for x in v[b:b + 256]:
                s = s + x
            parts.append(s)
        tot = 0.0
        for p in parts:
            tot = tot + p
        return tot / len(v)

    o.set_mean_segment(o.DEVICE_MEAN_SEGMENT)
    try:
        assert vm.subset_mean(per_q, T) == two_level(per_q[T]) and vm.subset_mean(per_q, H) == two_level(per_q[H])
        # not the full mean's segments: segment 0 of T holds T's first 256 queries, not the queries below 256
        assert vm.subset_mean(per_q, np.arange(700)) == two_level(per_q)
    finally:
        o.set_mean_segment(0)


def test_stopping_rule_on_hand_made_sequences():
    # (best_iteration, trees trained, stopped_early, trees in the model)
    # the first maximum on ties
    assert vm.stopping([0.5, 0.7, 0.7, 0.6, 0.7], 0) == (2, 5, False, 5)
    assert vm.stopping([0.5, 0.7, 0.7, 0.6, 0.7, 0.1, 0.1], 3) == (2, 5, True, 2)
    assert vm.stopping([0.3, 0.3, 0.3, 0.3], 2) == (1, 3, True, 1)
    # a stop exactly at r: tree t = best + r is the last one trained
    assert vm.stopping([0.1, 0.2, 0.9, 0.8, 0.7, 0.95, 0.99], 2) == (3, 5, True, 3)
    assert vm.stopping([0.1, 0.2, 0.9, 0.8, 0.91, 0.7, 0.6, 0.5], 2) == (5, 7, True, 5)
    assert vm.stopping([0.9, 0.1], 1) == (1, 2, False, 1)  # the rule fires at the last tree: nothing was saved
    assert vm.stopping([0.9, 0.1, 0.1], 1) == (1, 2, True, 1)
    # never while the measure keeps improving
    up = [0.01 * t for t in range(1, 60)]
    assert vm.stopping(up, 1) == (59, 59, False, 59)
    # ran out of trees before r rounds passed: still the trees up to the best
    assert vm.stopping([0.1, 0.5, 0.4, 0.3], 10) == (2, 4, False, 2)
    # r = 0: everything is trained and kept, the best is only reported
    assert vm.stopping([0.1, 0.5, 0.4, 0.3], 0) == (2, 4, False, 4)
    # a measure of 0.0 throughout: tree 1 is the first maximum
    assert vm.stopping([0.0, 0.0, 0.0], 1) == (1, 2, True, 1)
    # the sequence is read only as far as training goes
    assert vm.stopping([0.5, 0.4, 0.3, 0.99], 2, num_trees=4) == (1, 3, True, 1)


def test_restatement_stops_early_on_the_trec_golden():
    """The fixture of the device test (tests/test_gpu_lambdamart_valid.py): every second query held out, learning rate 0.3."""
    import os

    from tests.conftest import GOLDEN

    d = np.load(os.path.join(GOLDEN, "trec_news_2018.npz"))
    X, y, qid = d["train_X"], d["train_y"], d["train_qid"]
    c = o.Dataset(X, y, qid)
    nq = len(np.unique(qid))
    for grower, best in (("exact", 5), ("histogram", 8)):
        r = vm.train(X, y, c, range(1, nq, 2), grower=grower, measure="ndcg@10", num_trees=30, learning_rate=0.3, max_depth=4,
                     min_leaf_support=5, split_candidates=16, early_stopping_rounds=3)
        assert (r["best_iteration"], r["trees"], r["stopped_early"]) == (best, best + 3, True)
        assert len(r["model"]["Ensemble"]["models"]) == best and best + 3 < 30
        assert r["valid_measure"][best - 1] == max(r["valid_measure"]) and r["valid_measure"].index(max(r["valid_measure"])) == best - 1
