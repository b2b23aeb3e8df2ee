"""LambdaMART with a validation dataset of its own and with an init model, without a GPU ("Validation
dataset" and "Continued training"): the binding and the symbol, every refusal (all raised before any device work), and the
restatement's own properties (tests/lambdamart_validset_model.py)."""
import inspect
import json
import os
import re

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import clib
from fastrank_amd.training import LambdaMARTParams
from oracle import pyoracle as o
from tests import lambdamart_hist_model as hm
from tests import lambdamart_model as lm
from tests import lambdamart_valid_model as vm
from tests import lambdamart_validset_model as vs
from tests.conftest import ROOT

LEAF = {"LeafNode": 0.5}


def _tree(fid=0, split=10.0, lo=-1.0, hi=1.0):
    return {"FeatureSplit": {"fid": fid, "split": split, "lhs": {"LeafNode": lo}, "rhs": {"LeafNode": hi}}}


def _dataset(d=3, qids=(7, 3, 11)):
    n = 4 * len(qids)
    X = np.arange(n * d, dtype=np.float32).reshape(n, d)
    y = np.array(([0, 1, 2, 0, 1, 0, 0, 1, 2, 1, 0, 0] * len(qids))[:n], dtype=np.float64)
    qid = np.repeat(np.array(qids, dtype=np.int64), 4)
    return fr.CDataset.from_numpy(X, y, qid)


def _request(**kw):
    req = fr.TrainRequest.lambdamart()
    req.params.quiet = True
    req.params.num_trees = 2
    for k, v in kw.items():
        setattr(req.params, k, v)
    return req


def _ensemble(trees, weights=None):
    return fr.CModel.from_dict({"Ensemble": {"weights": [1.0] * len(trees) if weights is None else weights,
                                             "models": [{"DecisionTree": t} for t in trees]}})


# --- the binding and the symbol -------------------------------------------------------------------

def test_the_binding_takes_the_two_optional_arguments():
    sig = inspect.signature(fr.CDataset.train_model)
    assert list(sig.parameters) == ["self", "train_req", "valid", "init_model"]
    assert sig.parameters["valid"].default is None and sig.parameters["init_model"].default is None


def test_without_the_new_arguments_the_binding_issues_the_call_it_issued(monkeypatch):
    calls = []

    class Recorder:
        def train_model(self, request, dataset):
            calls.append(("train_model", request, dataset))

        def fr_train_model_with(self, request, dataset, valid, init):
            calls.append(("fr_train_model_with", request, dataset, valid, init))

    a, b, m = _dataset(), _dataset(qids=(1, 2)), _ensemble([_tree()])
    req = _request()
    text = json.dumps(req.to_dict()).encode("utf-8")
    monkeypatch.setattr(clib, "_load", lambda: Recorder())
    for kw in ({}, dict(valid=None, init_model=None), dict(valid=b), dict(init_model=m), dict(valid=b, init_model=m)):
        with pytest.raises(ValueError, match="CResult should not be NULL"):  # (the recorder returns nothing)
            a.train_model(req, **kw)
    assert calls == [("train_model", text, a.pointer)] * 2 + [("fr_train_model_with", text, a.pointer, b.pointer, None),
                                                             ("fr_train_model_with", text, a.pointer, None, m.pointer),
                                                             ("fr_train_model_with", text, a.pointer, b.pointer, m.pointer)]


def test_the_symbol_is_exported_declared_and_bound():
    lib = clib._load()
    assert hasattr(lib, "fr_train_model_with") and lib.fr_train_model_with.argtypes is not None and len(lib.fr_train_model_with.argtypes) == 4
    with open(os.path.join(ROOT, "include", "fastrank.h")) as fh:
        header = fh.read()
    assert re.search(r"const CResult \*fr_train_model_with\(const void \*train_request_json, const CDataset \*dataset,\s+"
                     r"const CDataset \*valid_dataset_or_null,\s+const CModel \*init_model_or_null\);", header)
    # train_model itself is declared as it was
    assert "const CResult *train_model(void *train_request_json, void *dataset);" in header


def test_a_null_dataset_and_a_bad_request_fail_as_in_train_model():
    lib = clib._load()
    v = _dataset()
    with pytest.raises(Exception, match="Dataset pointer is null!"):
        clib._unwrap(lib.fr_train_model_with(b"{}", None, v.pointer, None))
    with pytest.raises(Exception, match="Dataset pointer is null!"):
        clib._unwrap(lib.fr_train_model_with(b"{}", None, None, None))
    with pytest.raises(Exception, match="missing field"):
        clib._unwrap(lib.fr_train_model_with(b"{}", v.pointer, v.pointer, None))


# --- refusals, all before any device work -----------------------------------------------------------

@pytest.mark.parametrize("make,name", [(fr.TrainRequest.coordinate_ascent, "CoordinateAscent"), (fr.TrainRequest.random_forest, "RandomForest")])
def test_the_other_learners_refuse_either_argument(make, name):
    a, b = _dataset(), _dataset(qids=(1, 2))
    with pytest.raises(Exception, match="the request's learner is %s" % name):
        a.train_model(make(), valid=b)
    with pytest.raises(Exception, match="the request's learner is %s" % name):
        a.train_model(make(), init_model=_ensemble([_tree()]))


def test_valid_with_validation_queries_is_refused():
    a, b = _dataset(), _dataset(qids=(1, 2))
    with pytest.raises(Exception, match="invalid value") as e:
        a.train_model(_request(validation_queries=["3"]), valid=b)
    assert "validation_queries cannot be combined with a validation dataset (there is one source of the held-out measure)" in str(e.value)


def test_valid_being_the_trained_view_is_refused():
    a = _dataset()
    for same in (a, a.subsample_feature_names(sorted(a.feature_names())[:2])):
        with pytest.raises(Exception, match="invalid value") as e:
            a.train_model(_request(), valid=same)
        assert "the validation dataset is the dataset being trained on (hold queries of it out with validation_queries)" in str(e.value)


def test_a_feature_the_validation_dataset_lacks_is_named():
    a = _dataset(d=4)
    with pytest.raises(Exception, match="the validation dataset does not hold feature `3` of the training dataset"):
        a.train_model(_request(), valid=_dataset(d=3, qids=(1, 2)))
    sib = a.subsample_queries(["7"]).subsample_feature_names(["0", "2", "3"])
    with pytest.raises(Exception, match="the validation dataset does not hold feature `1` of the training dataset"):
        a.subsample_queries(["3", "11"]).train_model(_request(), valid=sib)


def test_early_stopping_needs_a_source_and_stays_refused_under_dart():
    a, b = _dataset(), _dataset(qids=(1, 2))
    with pytest.raises(Exception, match="early_stopping_rounds needs at least one validation query"):
        a.train_model(_request(early_stopping_rounds=2))
    with pytest.raises(Exception, match="early_stopping_rounds needs at least one validation query"):
        a.train_model(_request(early_stopping_rounds=2), init_model=_ensemble([_tree()]))
    with pytest.raises(Exception, match="early_stopping_rounds cannot be combined with drop_rate greater than 0"):
        a.train_model(_request(early_stopping_rounds=2, drop_rate=0.5), valid=b)


@pytest.mark.parametrize("model,what", [
    ({"Linear": {"weights": [1.0, 2.0, 3.0]}}, "not a Linear model"),
    ({"SingleFeature": {"fid": 0, "dir": 1.0}}, "not a SingleFeature model"),
    ({"DecisionTree": _tree()}, "not a bare DecisionTree"),
    ({"Ensemble": {"weights": [1.0, 1.0], "models": [{"DecisionTree": _tree()}, {"Ensemble": {"weights": [1.0], "models": [{"DecisionTree": _tree()}]}}]}},
     r"a nested Ensemble \(member 1\)"),
    ({"Ensemble": {"weights": [1.0, 1.0], "models": [{"DecisionTree": _tree()}, {"Linear": {"weights": [1.0]}}]}}, r"a Linear member \(member 1\)"),
    ({"Ensemble": {"weights": [1.0, 1.0], "models": [{"SingleFeature": {"fid": 0, "dir": 1.0}}, {"DecisionTree": _tree()}]}},
     r"a SingleFeature member \(member 0\)"),
    ({"Ensemble": {"weights": [1.0], "models": [{"DecisionTree": _tree()}, {"DecisionTree": _tree()}]}}, "1 weights for 2 models"),
])
def test_an_init_model_that_is_no_forest_is_refused_by_name(model, what):
    with pytest.raises(Exception, match=what) as e:
        _dataset().train_model(_request(), init_model=fr.CModel.from_dict(model))
    assert "init_model" in str(e.value)


def test_a_non_finite_number_cannot_reach_the_trainer():
    """A model comes into being through model_from_json (CModel.from_dict) or a trainer.  JSON has no spelling for a
    non-finite number: the parser refuses an overflowing literal and the words Python writes for inf and nan, for a weight, a
    leaf and a split alike, so no handle to such a model exists to be given as init_model.  (The trainer's own isfinite
    refusal in lambdamart_check_init stands behind this for models a later loader might make.)"""
    lib = clib._load()
    tree = json.dumps({"DecisionTree": _tree()})
    assert tree.count("-1.0") == 1 and tree.count("10.0") == 1
    for bad, message in (("1e999", "number out of range"), ("-1e999", "number out of range"), ("Infinity", None), ("NaN", None)):
        for text in ('{"Ensemble": {"weights": [%s], "models": [%s]}}' % (bad, tree),
                     '{"Ensemble": {"weights": [1.0], "models": [%s]}}' % tree.replace("-1.0", bad),
                     '{"Ensemble": {"weights": [1.0], "models": [%s]}}' % tree.replace("10.0", bad)):
            with pytest.raises(Exception, match=message) as e:
                clib._unwrap(lib.model_from_json(text.encode()))
            assert str(e.value).startswith("error: "), "not the library's error envelope"
    for value in (float("inf"), float("-inf"), float("nan")):
        with pytest.raises(Exception, match="error: "):
            _ensemble([_tree()], [value])
        with pytest.raises(Exception, match="error: "):
            _ensemble([_tree(lo=value)])
        with pytest.raises(Exception, match="error: "):
            _ensemble([_tree(split=value)])
    # the largest finite numbers are numbers: they pass the parser and the trainer's number checks, which come before the
    # last refusal of lambdamart_check_init (nothing here reaches the device)
    big = _ensemble([_tree(split=1.7976931348623157e308, lo=-1.7976931348623157e308)], [1.7976931348623157e308])
    with pytest.raises(Exception, match="init_model cannot be combined with drop_rate greater than 0"):
        _dataset().train_model(_request(drop_rate=0.3), init_model=big)


def test_an_init_model_under_dart_is_refused():
    with pytest.raises(Exception, match="invalid value") as e:
        _dataset().train_model(_request(drop_rate=0.3), init_model=_ensemble([_tree()]))
    assert "init_model cannot be combined with drop_rate greater than 0" in str(e.value) and "changes a model the caller owns" in str(e.value)


# --- the restatement's own properties ---------------------------------------------------------------

def _trec(trec):
    XA, yA, qA = trec["train_X"], trec["train_y"], trec["train_qid"]
    XB, yB, qB = trec["test_X"], trec["test_y"], trec["test_qid"]
    return (XA, yA, qA, o.Dataset(XA, yA, qA)), (XB, yB, qB, o.Dataset(XB, yB, qB))


KW = dict(measure="ndcg@10", learning_rate=0.1, max_depth=5, min_leaf_support=5, split_candidates=16)


@pytest.mark.parametrize("grower", ["exact", "histogram"])
def test_b_reaches_no_tree(trec, grower):
    """The restatement on train || test with the five test queries held out gives the trees of the restatement on train
    alone: for the exact grower as it is, for the histogram grower once the bins are those of train alone."""
    (XA, yA, qA, cA), (XB, yB, qB, cB) = _trec(trec)
    assert len(set(qA.tolist())) == 45 and len(set(qB.tolist())) == 5 and not set(qA.tolist()) & set(qB.tolist())
    X, y, qid = np.concatenate([XA, XB]), np.concatenate([yA, yB]), np.concatenate([qA, qB])
    c = o.Dataset(X, y, qid)
    held = list(range(45, 50))
    alone = vs.train(XA, yA, cA, B=(XB, yB, cB), grower=grower, num_trees=4, **KW)
    if grower == "exact":
        both = vm.train(X, y, c, held, grower=grower, num_trees=4, **KW)
        assert both["model"] == alone["model"]
        assert both["train_measure"] == alone["train_measure"] and both["valid_measure"] == alone["valid_measure"]
    else:
        edges, bins = hm.bin_matrix(XA, np.concatenate(lm.query_lists(cA)), list(range(6)), 16)
        padded = (edges, np.concatenate([bins, np.zeros((bins.shape[0], len(yB)), dtype=bins.dtype)], axis=1))  # (held-out rows are never read)
        both = vs.train(X, y, c, held_idx=held, grower=grower, num_trees=4, binned=padded, **KW)
        assert both["model"] == alone["model"]
        assert both["train_measure"] == alone["train_measure"] and both["valid_measure"] == alone["valid_measure"]
        # ... and with the bins over the full list the held-out documents do shape the edges
        full = hm.bin_matrix(X, np.concatenate(lm.query_lists(c)), list(range(6)), 16)
        assert any(a.tobytes() != b.tobytes() for a, b in zip(full[0], edges))


def test_the_stopping_rule_with_a_baseline():
    # T0 = 0 is the existing rule
    for valid, r in ([0.1, 0.3, 0.3, 0.2, 0.5], 0), ([0.1, 0.3, 0.3, 0.2, 0.5], 2), ([0.5, 0.5, 0.5], 1), ([0.0, 0.0], 0):
        assert vs.stopping(valid, r) == vm.stopping(valid, r)
    # no new tree beats the baseline: best stays T0 (ties do not take over), training ends after r trees, T0 trees come back
    assert vs.stopping([0.4, 0.5, 0.5, 0.9], 3, T0=10, init_valid=0.5) == (10, 3, True, 10)
    assert vs.stopping([0.4, 0.5], 3, T0=10, init_valid=0.5) == (10, 2, False, 10)
    # a new tree beats it strictly; the first maximum wins among ties
    assert vs.stopping([0.4, 0.6, 0.6, 0.6, 0.1], 3, T0=10, init_valid=0.5) == (12, 5, False, 12)
    assert vs.stopping([0.4, 0.6, 0.6, 0.6, 0.1, 0.9], 3, T0=10, init_valid=0.5) == (12, 5, True, 12)
    assert vs.stopping([0.6, 0.7], 1, T0=2, init_valid=0.5) == (4, 2, False, 4)
    # r = 0: every new tree is kept, the best is still reported
    assert vs.stopping([0.4, 0.6, 0.2], 0, T0=3, init_valid=0.5) == (5, 3, False, 6)
    assert vs.stopping([0.4, 0.5, 0.2], 0, T0=3, init_valid=0.5) == (3, 3, False, 6)
    # a baseline of 0.0 is a baseline, not "none yet"
    assert vs.stopping([0.0, 0.0], 2, T0=1, init_valid=0.0) == (1, 2, False, 1)


def test_the_early_stopping_fixture_is_not_trivial(trec):
    """trec train with trec test as the validation dataset, exact grower: the held-out curve peaks at tree 4 and r = 3 stops
    after tree 7; the curve has exact ties, so the first-maximum rule is exercised."""
    (XA, yA, qA, cA), (XB, yB, qB, cB) = _trec(trec)
    got = vs.train(XA, yA, cA, B=(XB, yB, cB), grower="exact", num_trees=20, early_stopping_rounds=3, **KW)
    v = got["valid_measure"]
    assert (got["best_iteration"], got["trees_trained"], got["stopped_early"]) == (4, 7, True)
    assert len(got["model"]["Ensemble"]["models"]) == 4 and len(v) == 7
    assert v[3] == max(v) and all(x < v[3] for x in v[:3])
    assert len(set(v)) < len(v), "the curve has no exact tie"
    assert vs.stopping(v + [0.0] * 13, 3, 20) == (4, 7, True, 4)


def test_the_restatement_splits(trec):
    """a trees, then b more from them, are a + b trees, with samples (the restatement's own split identity)."""
    (XA, yA, qA, cA), (XB, yB, qB, cB) = _trec(trec)
    kw = dict(KW, grower="histogram", rates=(0.5, 0.5), seed=9, B=(XB, yB, cB))
    long = vs.train(XA, yA, cA, num_trees=3, **kw)
    first = vs.train(XA, yA, cA, num_trees=1, **kw)
    init = (first["model"]["Ensemble"]["weights"], [m["DecisionTree"] for m in first["model"]["Ensemble"]["models"]])
    second = vs.train(XA, yA, cA, num_trees=2, init=init, **kw)
    assert second["model"] == long["model"]
    assert second["train_measure"] == long["train_measure"][1:] and second["valid_measure"] == long["valid_measure"][1:]
    assert second["init_train_measure"] == long["train_measure"][0] and second["init_valid_measure"] == long["valid_measure"][0]
    assert LambdaMARTParams().early_stopping_rounds == 0
