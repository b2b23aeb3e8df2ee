"""LambdaMART's wire form, defaults and request validation (no GPU: every request here fails or is only parsed before any
device work)."""
import json

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import clib
from fastrank_amd.training import LambdaMARTParams, TrainRequest

KEYS = ["num_trees", "learning_rate", "max_depth", "min_leaf_support", "split_candidates", "sigma", "quiet"]


def _dataset():
    X = np.arange(24, dtype=np.float32).reshape(8, 3)
    y = np.array([0, 1, 2, 0, 1, 0, 0, 1], dtype=np.float64)
    qid = np.array([1, 1, 1, 1, 2, 2, 2, 2], dtype=np.int64)
    return fr.CDataset.from_numpy(X, y, qid)


def _train_raw(params, measure="ndcg"):
    ds = _dataset()
    text = json.dumps({"measure": measure, "params": {"LambdaMART": params}, "judgments": None}).encode()
    return clib._unwrap(clib._load().train_model(text, ds.pointer))


def test_defaults_equal_the_native_defaults():
    req = TrainRequest.lambdamart()
    assert req.measure == "ndcg" and req.judgments is None
    assert req.params == LambdaMARTParams()
    assert isinstance(req.params, LambdaMARTParams)
    assert clib.query_json("lambdamart_defaults") == {
        "measure": "ndcg",
        "params": {"LambdaMART": {"num_trees": 100, "learning_rate": 0.1, "max_depth": 6, "min_leaf_support": 10,
                                  "split_candidates": 64, "sigma": 1.0, "quiet": False}},
        "judgments": None,
    }


def test_round_trips():
    req = TrainRequest.lambdamart()
    req.measure = "ndcg@10"
    req.params.num_trees = 7
    req.params.sigma = 2.5
    d = req.to_dict()
    assert list(d["params"]["LambdaMART"].keys()) == KEYS
    back = TrainRequest.from_dict(d)
    assert back == req
    c = req.clone()
    assert c == req and c is not req and c.params is not req.params


def test_unknown_query_still_unknown():
    with pytest.raises(Exception, match="unknown_query_str"):
        clib.query_json("lambdamart_whatever")


@pytest.mark.parametrize("key", KEYS)
def test_each_missing_key_is_rejected(key):
    p = LambdaMARTParams().to_dict()
    del p[key]
    with pytest.raises(Exception, match="missing field `%s`" % key):
        _train_raw(p)


@pytest.mark.parametrize("key,value,what", [
    ("num_trees", "ten", "expected unsigned integer for num_trees"),
    ("num_trees", -1, "expected unsigned integer for num_trees"),
    ("learning_rate", "fast", "expected f64 for learning_rate"),
    ("max_depth", 2.5, "expected unsigned integer for max_depth"),
    ("min_leaf_support", None, "expected unsigned integer for min_leaf_support"),
    ("split_candidates", [], "expected unsigned integer for split_candidates"),
    ("sigma", True, "expected f64 for sigma"),
    ("quiet", 1, "quiet"),
])
def test_wrong_types_are_rejected(key, value, what):
    p = LambdaMARTParams().to_dict()
    p[key] = value
    with pytest.raises(Exception, match="invalid type") as e:
        _train_raw(p)
    assert what in str(e.value)


@pytest.mark.parametrize("key,value,what", [
    ("num_trees", 0, "num_trees must be at least 1"),
    ("learning_rate", 0.0, "learning_rate must be finite and greater than 0"),
    ("learning_rate", -0.1, "learning_rate must be finite and greater than 0"),
    ("max_depth", 0, "max_depth must be at least 1"),
    ("sigma", 0.0, "sigma must be finite and greater than 0"),
    ("sigma", -1.0, "sigma must be finite and greater than 0"),
    ("num_trees", 2 ** 32, "expected u32"),
])
def test_out_of_range_values_are_rejected(key, value, what):
    p = LambdaMARTParams().to_dict()
    p[key] = value
    with pytest.raises(Exception) as e:
        _train_raw(p)
    assert what in str(e.value)


@pytest.mark.parametrize("measure", ["map", "ap", "mrr", "rr", "MAP@5"])
def test_measures_without_gradients_are_rejected(measure):
    with pytest.raises(Exception, match=r"supported: ndcg, ndcg@k"):
        _train_raw(LambdaMARTParams().to_dict(), measure)
    req = TrainRequest.lambdamart()
    req.measure = measure
    with pytest.raises(Exception, match=r"supported: ndcg, ndcg@k"):
        _dataset().train_model(req)


def test_unknown_variant_lists_three():
    ds = _dataset()
    text = json.dumps({"measure": "ndcg", "params": {"GBDT": {}}, "judgments": None}).encode()
    with pytest.raises(Exception, match="unknown variant `GBDT`, expected one of `CoordinateAscent`, `RandomForest`, `LambdaMART`"):
        clib._unwrap(clib._load().train_model(text, ds.pointer))


def test_shard_and_step_entry_points_stay_coordinate_ascent_only():
    from fastrank_amd import native

    ds = _dataset()
    req = TrainRequest.lambdamart()
    with pytest.raises(Exception, match="only CoordinateAscent"):
        native.train_model_shard(ds, req, 0, 1)
    with pytest.raises(Exception):
        native.CoordinateAscentRun(ds, req)


def test_gradient_hook_rejects_other_measures():
    from fastrank_amd import native

    ds = _dataset()
    m = fr.CModel.from_dict({"Linear": {"weights": [0.0, 0.0, 0.0]}})
    with pytest.raises(Exception, match="supported: ndcg, ndcg@k"):
        native.lambda_gradients(m, ds, "map")
