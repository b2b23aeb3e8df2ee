"""Random-forest TRAINING on the device on +inf, -inf and NaN feature values (csrc/rf_train.hpp, kernels_rf.inc) against the
oracle, whose own outcomes on these cases tests/test_rf_nonfinite_host.py derives by hand from the reference
(tests/rf_nonfinite_cases.py states the rule).  Where the reference grows a forest the device grows the same one, node by
node and bit by bit; where the reference panics, train_model raises a plain error naming the cause and returns nothing --
and the dataset object trains on as if nothing had happened.  No tolerances."""
import json

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import clib, native
from oracle import pyoracle as o
from tests import rf_nonfinite_cases as nf
from tests.conftest import ranksvm_presence

pytestmark = pytest.mark.gpu

INF = float("inf")
NAN_WORDS = "NaN found!"                 # Scored::new, src/core.rs:53
POSITION_WORDS = "split position is NaN"  # NotNan::new(..).unwrap(), src/random_forest.rs:238
WORDS = {"minus_inf": POSITION_WORDS, "both_inf": POSITION_WORDS, "nan": NAN_WORDS, "nan_sign_bit": NAN_WORDS}


def _request(params, measure="ndcg"):
    req = fr.TrainRequest.random_forest()
    req.measure = measure
    req.params.quiet = True
    for k, v in params.items():
        setattr(req.params, k, {v: []} if k == "split_method" else v)
    return req


def _oracle(c, req, fids=None):
    trees, w, _ = c.rf_learn(req.measure, req.params.to_dict(), fids=fids)
    return trees, w


def _same_forest(model, trees, w):
    """The device's forest is the oracle's: weights, then every node's fid and the f64 bits of its split or leaf value, where
    a non-finite split is JSON's null (what serde_json writes for it, and the only thing a dict can show)."""
    got = model.to_dict()["Ensemble"]
    assert got["weights"] == list(w)
    assert len(got["models"]) == len(trees)
    for t, (m, e) in enumerate(zip(got["models"], trees)):
        assert nf.flat_nodes(m["DecisionTree"]) == nf.flat_nodes(nf.as_json_tree(e)), "tree %d" % t


def _check(g, c, req, fids=None, infinite=None):
    """train_model against the oracle; the scores of the IN-MEMORY model against the oracle's scoring of its own trees (null
    hides which non-finite value a split holds; the scores do not: finite rows go left of +inf and right of NaN).
    infinite: whether the forest must / must not carry a +inf split (None: not asked)."""
    model = g.train_model(req)
    trees, w = _oracle(c, req, fids)
    _same_forest(model, trees, w)
    assert np.array_equal(native.predict_scores_dense(model, g), c.score_ensemble(trees, w))
    n_inf = sum(s == INF for t in trees for s in nf.splits(t))
    assert not any(np.isnan(s) or s == -INF for t in trees for s in nf.splits(t))
    if infinite is not None:
        assert (n_inf > 0) == infinite, "the case must%s contain an infinite split" % ("" if infinite else " not")
    # the text the library writes for the model: the reference's serde_json writes a non-finite f64 as null
    text = clib._take_str(clib._load().model_query_json(model.pointer, b"to_json")).replace(" ", "")
    assert text.count('"split":null') == n_inf and "inf" not in text.lower() and "nan" not in text.lower()
    return model, trees


def _raises(g, req, words):
    with pytest.raises(Exception, match=words) as ei:
        g.train_model(req)
    assert "random forest: feature " in str(ei.value)
    return str(ei.value)


# --- +inf with a finite minimum: a forest with split = +inf ---------------------------------------------------------------

@pytest.mark.parametrize("method", nf.METHODS)
def test_plus_inf_rows_grow_the_oracles_forest(method):
    X, y, qid = nf.two_hundred()
    X = nf.edit_column(X, "plus_inf")
    _check(fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid), _request(nf.two_hundred_params(method)), infinite=True)


@pytest.mark.parametrize("method", nf.METHODS[:3])
def test_ten_instances_one_plus_inf(method):
    """test_rf_nonfinite_host.py::test_one_plus_inf_splits_the_root_at_plus_inf, on the device."""
    X, y, qid = nf.ten()
    X[9, 0] = nf.INF
    model, trees = _check(fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid), _request(nf.ten_params(method)), infinite=True)
    assert trees[0]["FeatureSplit"]["split"] == INF
    root = model.to_dict()["Ensemble"]["models"][0]["DecisionTree"]["FeatureSplit"]
    assert root["split"] is None and root["rhs"] == {"LeafNode": 12.0}


def test_plus_inf_through_the_three_block_candidate_loop():
    """split_candidates = 130: 129 candidates, three trips of the eval kernel's 64-lane candidate loop."""
    X, y, qid = nf.two_hundred()
    X = nf.edit_column(X, "plus_inf")
    _check(fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid), _request(nf.two_hundred_params(split_candidates=130)), infinite=True)


def test_plus_inf_cut_into_batches(monkeypatch):
    monkeypatch.setenv("FR_RF_BATCH_BYTES", "1")  # (below one tree's size: every tree is a batch of its own)
    X, y, qid = nf.four_hundred()
    X = nf.edit_column(X, "plus_inf")
    _check(fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid), _request(nf.two_hundred_params(num_trees=16)), infinite=True)
    assert native.last_train_stats()["groups"] >= 2, "batches"


@pytest.mark.parametrize("env", ["FR_RF_PARTITION=0", "FR_RF_RESORT=1"])
def test_plus_inf_under_the_other_level_formulations(env, monkeypatch):
    monkeypatch.setenv(*env.split("="))
    X, y, qid = nf.two_hundred()
    X = nf.edit_column(X, "plus_inf")
    _check(fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid), _request(nf.two_hundred_params()), infinite=True)


# --- nothing but +inf: no panic in the reference (the minimum stays f64::MAX) ----------------------------------------------------

@pytest.mark.parametrize("method", nf.METHODS)
def test_all_plus_inf_column_is_no_error(method):
    """test_rf_nonfinite_host.py::test_all_plus_inf_is_a_leaf_not_a_panic and ::test_two_hundred_documents_all_plus_inf_column_
    is_silently_unused, on the device: the column yields no candidate under min_leaf_support >= 1."""
    X, y, qid = nf.ten()
    X[:, 0] = nf.INF
    model, _ = _check(fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid), _request(nf.ten_params(method)), infinite=False)
    assert model.to_dict()["Ensemble"]["models"] == [{"DecisionTree": {"LeafNode": 7.0}}]
    X, y, qid = nf.two_hundred()
    X = nf.edit_column(X, "all_plus_inf")
    _check(fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid), _request(nf.two_hundred_params(method)), infinite=False)


def test_all_plus_inf_with_no_leaf_support_splits_off_an_empty_side():
    """::test_all_plus_inf_with_no_leaf_support_splits_off_an_empty_side on the device: min = f64::MAX makes the position
    +inf, not NaN, and min_leaf_support = 0 lets the candidate with an empty left side through."""
    X, y, qid = nf.ten()
    X[:, 0] = nf.INF
    _, trees = _check(fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid), _request(nf.ten_params(min_leaf_support=0, max_depth=3)),
                      infinite=True)
    assert trees[0]["FeatureSplit"]["lhs"] == {"LeafNode": 0.0}


# --- the reference's panics: a plain error, and a dataset that trains on --------------------------------------------------------

@pytest.mark.parametrize("method", nf.METHODS)
@pytest.mark.parametrize("kind", ["minus_inf", "both_inf", "nan", "nan_sign_bit"])
def test_reached_bad_values_are_a_plain_error_and_leave_nothing_behind(kind, method):
    X, y, qid = nf.two_hundred()
    Xe = nf.edit_column(X, kind)
    g = fr.CDataset.from_numpy(Xe, y, qid)
    req = _request(nf.two_hundred_params(method))
    with pytest.raises(RuntimeError, match="error 2"):  # (the oracle agrees that this is a panic)
        _oracle(o.Dataset(Xe, y, qid), req)
    assert "feature 1:" in _raises(g, req, WORDS[kind])
    # the same dataset object, through a view without the bad column: the oracle's forest over features 0, 2, 3
    names = g.feature_index_to_name()
    view = g.subsample_feature_names([names[f] for f in (0, 2, 3)])
    _check(view, o.Dataset(Xe, y, qid), req, fids=[0, 2, 3])
    _raises(g, req, WORDS[kind])  # (and the whole dataset is refused again)
    # ... and a second, finite dataset right after the failure
    _check(fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid), req, infinite=False)


@pytest.mark.parametrize("kind,words", [("minus_inf", POSITION_WORDS), ("nan", NAN_WORDS), ("nan_sign_bit", NAN_WORDS)])
def test_ten_instances_error_cases(kind, words):
    """::test_one_minus_inf_is_the_position_panic and ::test_one_nan_is_the_scored_new_panic on the device, the NaN also with
    split_candidates = 1, where no kernel runs."""
    X, y, qid = nf.ten()
    X[3, 0] = {"minus_inf": -nf.INF, "nan": nf.NAN_POS, "nan_sign_bit": nf.NAN_NEG}[kind]
    g = fr.CDataset.from_numpy(X, y, qid)
    for method in nf.METHODS:
        _raises(g, _request(nf.ten_params(method)), words)
        if kind != "minus_inf":
            _raises(g, _request(nf.ten_params(method, split_candidates=1)), words)


def test_a_later_tree_or_a_deeper_node_is_enough():
    """The bad rows sit in one query only and trees sample half the queries: some trees never see them, and the call fails
    all the same (src/random_forest.rs:305: a panic in any tree).  The oracle says which requests reach them."""
    X, y, qid = nf.two_hundred()
    X[40:60:3, 1] = -nf.INF  # query 3
    g, c = fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)
    outcomes = set()
    for seed in range(6):
        req = _request(nf.two_hundred_params(seed=seed, num_trees=2, instance_sampling_rate=0.5))
        try:
            trees, w = _oracle(c, req)
        except RuntimeError:
            _raises(g, req, POSITION_WORDS)
            outcomes.add("error")
        else:
            _same_forest(g.train_model(req), trees, w)
            outcomes.add("forest")
    assert outcomes == {"error", "forest"}, "both outcomes must occur among the seeds"


# --- bad values no node reaches: silence, and the oracle's forest -----------------------------------------------------------------

@pytest.mark.parametrize("kind", ["minus_inf", "nan"])
@pytest.mark.parametrize("why", ["labels_equal", "max_depth_1", "support_above_n", "query_view", "feature_view"])
def test_unreached_bad_values_stay_silent(why, kind):
    X, y, qid = nf.two_hundred()
    bad = -nf.INF if kind == "minus_inf" else nf.NAN_POS
    X[40:60:3, 1] = bad  # rows of query 3 only
    assert not np.isfinite(X[:, 1]).all(), "the parent data must hold the bad value"
    params, fids, rows = nf.two_hundred_params(), None, np.ones(200, dtype=bool)
    if why == "labels_equal":
        y = np.full_like(y, 2.0)
    elif why == "max_depth_1":
        params["max_depth"] = 1
    elif why == "support_above_n":
        params["min_leaf_support"] = 201
    g = fr.CDataset.from_numpy(X, y, qid)
    view = g
    if why == "query_view":
        view = g.subsample_queries([q for q in sorted(g.queries()) if q != "3"])
        rows = qid != 3
        assert np.isfinite(X[rows]).all() and not np.isfinite(X[~rows]).all()
    elif why == "feature_view":
        names = g.feature_index_to_name()
        view, fids = g.subsample_feature_names([names[f] for f in (0, 2, 3)]), [0, 2, 3]
    c = o.Dataset(np.ascontiguousarray(X[rows]), np.ascontiguousarray(y[rows]), np.ascontiguousarray(qid[rows]))
    req = _request(params)
    model = view.train_model(req)
    trees, w = _oracle(c, req, fids)
    _same_forest(model, trees, w)
    leaves_only = why in ("labels_equal", "max_depth_1", "support_above_n")
    assert all(("LeafNode" in t) == leaves_only for t in trees)


# --- file-loaded datasets: values a row does not hold --------------------------------------------------------------------------

@pytest.mark.parametrize("token", ["inf", "-inf", "NaN", "+Infinity"])
def test_ranksvm_file_with_absent_values_and_non_finite_tokens(tmp_path, token):
    """The reference reads a feature value with fast_float::parse (src/libsvm.rs:88), which -- by that crate's documentation;
    its source is not part of the reference -- accepts "inf", "infinity" and "nan" in any case, with a sign: the file loads
    and the instance HOLDS the non-finite value (src/instance.rs:104-130).  The loader here takes them alike.  Then the
    rule is the one above over the HELD values (src/normalizers.rs:23-27), an absent value sorting as 0.0
    (src/random_forest.rs:228): checked against the oracle with the file's presence table."""
    path = str(tmp_path / "nonfinite.train")
    X, y, qid = nf.write_ranksvm(path, token)
    rd = fr.CDataset.open_ranksvm(path)
    present = ranksvm_presence(path, 4)
    assert int((~present[:, 3]).sum()) == 12 and not X[~present].any() and not np.isfinite(X[present]).all()
    c = o.Dataset(X, y, qid)
    c.set_presence(present)
    for method in ("SquaredError", "TrueVarianceReduction"):
        req = _request(nf.two_hundred_params(method, num_trees=4))
        if token in ("inf", "+Infinity"):
            _check(rd, c, req, infinite=True)
        else:
            with pytest.raises(RuntimeError, match="error 2"):
                _oracle(c, req)
            assert "feature 3:" in _raises(rd, req, NAN_WORDS if token == "NaN" else POSITION_WORDS)
    if token == "NaN":
        # a NaN that is the ONLY value a node holds of the feature has no stats (src/stats.rs:98-100) and stays silent
        only = np.zeros_like(present)
        only[:, :3] = True
        only[7, 3] = True
        lines = open(path).read().splitlines()
        kept = [ln if i == 7 else " ".join(t for t in ln.split() if not t.startswith("3:")) for i, ln in enumerate(lines)]
        lone = str(tmp_path / "lone.train")
        open(lone, "w").write("\n".join(kept) + "\n")
        assert np.array_equal(ranksvm_presence(lone, 4), only) and np.isnan(X[7, 3])
        X1 = X.copy()
        X1[~only] = 0.0
        c1 = o.Dataset(X1, y, qid)
        c1.set_presence(only)
        req = _request(nf.two_hundred_params(num_trees=4))
        model = fr.CDataset.open_ranksvm(lone).train_model(req)
        _same_forest(model, *_oracle(c1, req))
