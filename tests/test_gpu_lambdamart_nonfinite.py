"""LambdaMART on +inf, -inf and NaN feature values ("Non-finite feature values").  The invariant: whatever
train_model returns for a LambdaMART request can be written down -- it survives to_dict -> from_dict byte for byte, is accepted
as init_model and by explain.  A split at +-inf cannot (JSON writes null), so a request that may READ a column holding +-inf or
NaN is refused up front, by both growers, with one plain error naming the feature; a column a feature view leaves out, and a
validation dataset no tree reads, are fine.  No tolerances: errors, bytes, and the restatements' trees."""
import json

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import native
from oracle import pyoracle as o
from tests import lambdamart_hist_model as hm
from tests import lambdamart_model as lm
from tests import rf_nonfinite_cases as nf
from tests.conftest import synth_dataset
from tests.lambdamart_composed_model import _request

pytestmark = pytest.mark.gpu

SMALL = dict(max_depth=4, min_leaf_support=5, split_candidates=16)
# exact and histogram growers; the histogram grower level-wise and leaf-wise, under the variance and the Newton gain
GROWERS = {"exact": ("exact", {}), "histogram": ("histogram", {}), "histogram-newton": ("histogram", dict(split_gain="newton")),
           "histogram-leafwise": ("histogram", dict(max_leaves=6)), "histogram-newton-leafwise": ("histogram", dict(split_gain="newton", max_leaves=6))}
BAD = {"plus_inf": nf.INF, "minus_inf": -nf.INF, "nan": nf.NAN_POS, "nan_sign_bit": nf.NAN_NEG}
COL = 2


@pytest.fixture(scope="module")
def data():
    X, y, qid = synth_dataset(11, 300, 5, 12, max_len=60)
    return X, y, qid


def _stats():
    return native.last_train_stats()["lambdamart"]


@pytest.mark.parametrize("grower", sorted(GROWERS))
@pytest.mark.parametrize("kind", sorted(BAD))
def test_a_readable_non_finite_column_is_refused(data, kind, grower):
    X, y, qid = data
    X = X.copy()
    X[17, COL] = BAD[kind]
    g = fr.CDataset.from_numpy(X, y, qid)
    name, extra = GROWERS[grower]
    # (the histogram grower meets a NaN while binning, with the message it always had; everything else is the new refusal)
    words = "a feature value is NaN" if name == "histogram" and kind.startswith("nan") else "feature %d holds an inf or NaN value" % COL
    with pytest.raises(Exception, match=words):
        g.train_model(_request("ndcg@10", name, num_trees=2, **SMALL, **extra))
    # the dataset is not spoilt: a view without the column trains, twice to the same bytes
    names = g.feature_index_to_name()
    view = g.subsample_feature_names([names[f] for f in range(X.shape[1]) if f != COL])
    req = _request("ndcg@10", name, num_trees=2, **SMALL, **extra)
    assert json.dumps(view.train_model(req).to_dict()) == json.dumps(view.train_model(req).to_dict())


def test_a_query_view_is_refused_by_its_parents_column(data):
    """The decision is read from the device form's per-column max |x|, which a query view inherits from the dataset it was
    sampled from (tests/test_gpu_device_form.py): a view whose own rows are finite is refused all the same, and says so."""
    X, y, qid = data
    X = X.copy()
    rows = np.flatnonzero(qid == qid[0])
    X[rows[0], COL] = nf.INF
    g = fr.CDataset.from_numpy(X, y, qid)
    view = g.subsample_queries([q for q in sorted(g.queries()) if q != str(int(qid[0]))])
    for grower in ("exact", "histogram"):
        with pytest.raises(Exception, match="or in the dataset it is a query view of"):
            view.train_model(_request("ndcg@10", grower, num_trees=2, **SMALL))


@pytest.mark.parametrize("grower", ["exact", "histogram"])
@pytest.mark.parametrize("kind", ["minus_inf", "nan"])
def test_a_column_left_out_by_a_feature_view_trains_to_the_restatements_trees(data, kind, grower):
    """No LambdaMART key fixes a feature sample (feature_sampling_rate draws one per tree); a feature view does.  Stage by
    stage, as tests/test_gpu_lambdamart.py::_stagewise: every tree is the restatement's fit to the device's gradients of the
    trees before it, over the view's features.  The model then keeps the invariant."""
    X, y, qid = data
    X = X.copy()
    X[17::40, COL] = BAD[kind]
    assert not np.isfinite(X[:, COL]).all(), "the parent data must hold the bad value"
    g, c = fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)
    feats = [f for f in range(X.shape[1]) if f != COL]
    names = g.feature_index_to_name()
    view = g.subsample_feature_names([names[f] for f in feats])
    T, lr = 3, 0.1
    req = _request("ndcg@10", grower, num_trees=T, learning_rate=lr, **SMALL)
    model = view.train_model(req)
    d = model.to_dict()
    trees = [m["DecisionTree"] for m in d["Ensemble"]["models"]]
    assert d["Ensemble"]["weights"] == [lr] * T
    order_ids = np.concatenate(lm.query_lists(c))
    fit = hm.fit_tree if grower == "histogram" else lm.fit_tree
    for t in range(T):
        prefix = fr.CModel.from_dict({"Ensemble": {"weights": [lr] * t, "models": [{"DecisionTree": x} for x in trees[:t]]}})
        lam, wt = native.lambda_gradients(prefix, view, "ndcg@10", req.params.sigma)
        assert trees[t] == fit(X, lam, wt, order_ids, feats, SMALL["max_depth"], SMALL["min_leaf_support"], SMALL["split_candidates"]), "tree %d" % t
    assert any("FeatureSplit" in t for t in trees)
    # the invariant: written down and read back byte for byte, continued, explained
    text = json.dumps(d)
    again = fr.CModel.from_dict(json.loads(text))
    assert json.dumps(again.to_dict()) == text
    more = view.train_model(_request("ndcg@10", grower, num_trees=1, learning_rate=lr, **SMALL), init_model=again)
    assert [m["DecisionTree"] for m in more.to_dict()["Ensemble"]["models"]][:T] == trees
    Xf = X.copy()
    Xf[:, COL] = 0.0
    ex = model.explain(fr.CDataset.from_numpy(Xf, y, qid))
    assert np.isfinite(ex.values).all() and not ex.values[:, COL].any()


@pytest.mark.parametrize("grower", ["exact", "histogram"])
def test_a_validation_dataset_may_hold_anything(data, grower):
    """No tree is fitted to the validation dataset: 300 documents holding NaN (both signs), +inf and -inf only change where its
    documents are routed.  valid_measure[j] is the oracle's evaluation of the first j + 1 trees on it, bit for bit, and the
    model is the one trained without it."""
    X, y, qid = data
    XB, yB, qB = synth_dataset(12, 300, 5, 10, max_len=60)
    XB = XB.copy()
    for j, v in enumerate(BAD.values()):
        XB[j::13, j] = v
    XB[5::17, 4] = nf.NAN_POS
    assert sum(int((~np.isfinite(XB[:, f])).any()) for f in range(5)) == 5
    gA, gB, cB = fr.CDataset.from_numpy(X, y, qid), fr.CDataset.from_numpy(XB, yB, qB), o.Dataset(XB, yB, qB)
    T, lr = 5, 0.1
    req = _request("ndcg@10", grower, num_trees=T, learning_rate=lr, **SMALL)
    model = gA.train_model(req, valid=gB)
    st = _stats()
    assert json.dumps(model.to_dict()) == json.dumps(gA.train_model(req).to_dict())
    trees = [m["DecisionTree"] for m in model.to_dict()["Ensemble"]["models"]]
    used = set()
    for t in trees:
        for fid, _ in nf.flat_nodes(t):
            used.add(fid)
    assert len(used - {-1}) >= 2, "the trees must read columns that are not finite in the validation dataset"
    assert len(st["valid_measure"]) == T
    for j in range(T):
        per_q, err = cB.metric_from_scores("ndcg@10", cB.score_ensemble(trees[:j + 1], [lr] * (j + 1)))
        assert err == 0 and st["valid_measure"][j] == o.mean(per_q), "valid_measure[%d]" % j
