"""LambdaMART's MAP and MRR objectives on the device (lambda_grad_kernel / lambda_grad_trunc_kernel instantiated for the
objective) against the numpy restatement (tests/lambdamart_objective_model.py, DESIGN.md section 11, "Objectives").

Gradients: rtol 1e-12 with exact zeros, the figure of tests/test_gpu_lambdamart.py: delta is built from correctly rounded
basic operations only and both sides perform them identically, so `exp` remains the only library call.  Under lambda_norm
the derived tolerance of tests/test_gpu_lambdamart_trunc.py (`_norm_rtol`, its derivation is there).
Training: every tree equals the restatement's fit to the DEVICE's gradients of the prefix model, bit for bit.
"""
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
from tests import lambdamart_objective_model as om
from tests import lambdamart_trunc_model as tm
from tests import lambdamart_valid_model as vm
from tests.lambdamart_composed_model import _ensemble, _names, _request
from tests.conftest import GOLDEN, synth_dataset
from tests.test_gpu_lambdamart_trunc import _norm_rtol

pytestmark = pytest.mark.gpu

MEASURE_OF = {"map": "ap", "mrr": "rr"}


def _edge_set():
    """Stored order = row order, integer scores in column 0 (many ties).  By query id:
    1..5: 1, 2, 4, 5 and 6 documents; 6: no relevant document; 7: every document relevant; 8: exactly one relevant document
    (no f2); 9: the first relevant document at rank 0; 10: the only relevant documents at the last ranks; 11: two
    non-relevant documents on top, then a score tie of three non-relevant and two relevant documents (gain ascending puts the
    non-relevant ones first: f = 5), the rest below; 12: grades {0, 1, 2, 3}; 13, 14, 15: 300 (more than one document per
    thread), 1 300 and 4 100 documents (the slab path)."""
    rng = np.random.default_rng(91)
    lens = {1: 1, 2: 2, 3: 4, 4: 5, 5: 6, 6: 10, 7: 10, 8: 12, 9: 8, 10: 8, 11: 12, 12: 30, 13: 300, 14: 1300, 15: 4100}
    qid = np.concatenate([np.full(n, q, dtype=np.int64) for q, n in lens.items()])
    n = len(qid)
    y = rng.choice(4, size=n, p=[0.6, 0.25, 0.1, 0.05]).astype(np.float64)
    s = np.floor(rng.exponential(3.0, n))
    y[qid == 1] = [1.0]
    y[qid == 2], s[qid == 2] = [2.0, 0.0], [1.0, 3.0]
    y[qid == 3] = [0.0, 1.0, 0.0, 3.0]
    y[qid == 4] = [1.0, 0.0, 0.0, 2.0, 0.0]
    y[qid == 5] = [0.0, 0.0, 1.0, 0.0, 1.0, 0.0]
    y[qid == 6] = 0.0
    y[qid == 7] = rng.choice([1.0, 2.0, 3.0], size=10)
    y8 = np.zeros(12)
    y8[7] = 2.0
    y[qid == 8] = y8
    s9, y9 = rng.permutation(8).astype(np.float64), rng.choice([0.0, 1.0], size=8)
    y9[np.argmax(s9)] = 3.0
    s[qid == 9], y[qid == 9] = s9, y9
    s10, y10 = np.array([5.0, 7.0, 1.0, 3.0, 1.0, 9.0, 4.0, 6.0]), np.zeros(8)
    y10[[2, 4]] = [1.0, 2.0]  # the tie at the lowest score: ranks 6 and 7
    s[qid == 10], y[qid == 10] = s10, y10
    s[qid == 11] = [9.0, 5.0, 5.0, 2.0, 5.0, 9.0, 5.0, 1.0, 5.0, 0.0, 2.0, 1.0]
    y[qid == 11] = [0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 2.0, 0.0, 0.0, 3.0, 0.0, 0.0]
    y[qid == 12] = rng.permutation(np.arange(30) % 4).astype(np.float64)
    X = np.zeros((n, 3), dtype=np.float32)
    X[:, 0] = s
    X[:, 1] = rng.random(n)
    X[:, 2] = rng.integers(0, 4, n)
    return X, y, qid


def _edge_qrel(y, qid):
    """Judgments that know more relevant documents than the lists of queries 4, 11 and 13 hold (and none at all for query
    5: its count falls back to the list's own)."""
    qrel = {}
    for q, extra in ((4, 3), (11, 1), (13, 40)):
        count = int((y[qid == q] > 0).sum()) + extra
        qrel[str(q)] = {"%d.%d" % (q, i): 1.0 for i in range(count)}
    qrel["5"] = {"5.0": 0.0}
    return qrel


@pytest.fixture(scope="module")
def edge():
    X, y, qid = _edge_set()
    g, c = fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)
    model = fr.CModel.from_dict({"Linear": {"weights": [1.0, 0.0, 0.0]}})
    return X, y, qid, g, c, model, lm.query_lists(c), {}


@pytest.fixture(scope="module")
def trec():
    d = np.load(os.path.join(GOLDEN, "trec_news_2018.npz"))
    X, y, qid = d["train_X"], d["train_y"], d["train_qid"]
    return X, y, qid, fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)


@pytest.fixture(scope="module")
def synth():
    """Labels thresholded (0 and 1 -> 0; 2, 3, 4 -> 0, 1, 2) so that relevant and non-relevant documents are mixed."""
    X, y, qid = synth_dataset(7, 5000, 10, 50)
    y = np.maximum(y - 1.0, 0.0)
    assert 0.1 < (y > 0).mean() < 0.9
    return X, y, qid, fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)


def _compare(lam, wt, exp, queries, lambda_norm):
    elam, ewt, _, S, _ = exp
    assert np.all(np.isfinite(lam)) and np.all(np.isfinite(wt))
    worst = 0.0
    for q, ids in enumerate(queries):
        rtol = _norm_rtol(float(S[q])) if lambda_norm and S[q] > 0.0 else 1e-12
        for got, want in ((lam[ids], elam[ids]), (wt[ids], ewt[ids])):
            zero = want == 0.0
            assert np.array_equal(got[zero], want[zero]), q
            rel = np.abs(got[~zero] - want[~zero]) / np.abs(want[~zero])
            if rel.size:
                worst = max(worst, float(rel.max()))
                assert rel.max() <= rtol, "query %d: relative error %.3e > %.3e" % (q, rel.max(), rtol)
    print("worst relative error %.3e" % worst)


def _expected(edge, objective, sigma, T, norm, norms=None, tag=None):
    X, y, qid, g, c, model, queries, cache = edge
    key = (objective, sigma, T, norm, tag)
    if key not in cache:
        scores = native.predict_scores_dense(model, g)
        if norms is None:
            norms = c.default_norms(MEASURE_OF[objective])
        cache[key] = om.gradients(scores, y, queries, norms, objective, sigma, T, norm, parts=True)
    return cache[key]


def test_the_edge_set_is_what_its_docstring_says(edge):
    X, y, qid, g, c, model, queries, _ = edge
    s = X[:, 0].astype(np.float64)

    def ranked_rel(q):
        ids = queries[q - 1]
        r = tm.ranks(s[ids], y[ids].astype(np.float32), ids)
        out = np.empty(len(ids), dtype=bool)
        out[r] = y[ids] > 0
        return out

    assert [len(x) for x in queries] == [1, 2, 4, 5, 6, 10, 10, 12, 8, 8, 12, 30, 300, 1300, 4100]
    assert not ranked_rel(6).any() and ranked_rel(7).all() and ranked_rel(8).sum() == 1
    assert ranked_rel(9)[0] and np.flatnonzero(ranked_rel(10)).tolist() == [6, 7]
    F, T = False, True
    assert ranked_rel(11).tolist() == [F, F, F, F, F, T, T, F, T, F, F, T]
    assert np.sum(s[qid == 11] == 5.0) == 5 and sorted(y[(qid == 11) & (s == 5.0)]) == [0.0, 0.0, 0.0, 1.0, 2.0]
    assert set(y[qid == 12]) == {0.0, 1.0, 2.0, 3.0}
    for q in (13, 14, 15):
        assert 0 < ranked_rel(q).sum() < len(queries[q - 1])
        assert len(np.unique(s[qid == q])) < len(queries[q - 1]) // 4  # ties are many


# every sigma with every level (none, 5, beyond the longest query); normalisation on top of two of them
CASES = [(sigma, T, False) for sigma in (0.3, 1.0, 1.5) for T in (0, 5, 5000)] + [(0.3, 5, True), (1.5, 0, True)]


@pytest.mark.parametrize("sigma,T,norm", CASES)
@pytest.mark.parametrize("objective", om.OBJECTIVES)
def test_gradients_match_the_restatement(edge, objective, sigma, T, norm):
    X, y, qid, g, c, model, queries, _ = edge
    exp = _expected(edge, objective, sigma, T, norm)
    lam, wt = native.lambda_gradients(model, g, "ndcg", sigma, truncation_level=T, lambda_norm=norm, objective=objective)
    _compare(lam, wt, exp, queries, norm)
    for q in (1, 6, 7):  # one document, no relevant document, every document relevant
        assert not lam[qid == q].any() and not wt[qid == q].any()
    for q in (2, 3, 4, 5, 8, 9, 10, 11, 12, 13, 14, 15):
        assert lam[qid == q].any(), q
    # a second call gives the same bytes
    lam2, wt2 = native.lambda_gradients(model, g, "ndcg", sigma, truncation_level=T, lambda_norm=norm, objective=objective)
    assert lam2.tobytes() == lam.tobytes() and wt2.tobytes() == wt.tobytes()
    # the measure's depth is read for nothing
    lam3, wt3 = native.lambda_gradients(model, g, "ndcg@3", sigma, truncation_level=T, lambda_norm=norm, objective=objective)
    assert lam3.tobytes() == lam.tobytes() and wt3.tobytes() == wt.tobytes()


@pytest.mark.parametrize("objective", om.OBJECTIVES)
def test_judgments_that_know_more_relevant_documents_than_the_list(edge, objective):
    """R_q is the evaluator's norm: the judged count where the judgments know the query, the list's own count where they
    know no relevant document.  mrr does not read it."""
    X, y, qid, g, c, model, queries, _ = edge
    qrel_dict = _edge_qrel(y, qid)
    qrel = fr.CQRel.from_dict(qrel_dict)
    norms = c.qrel_norms(MEASURE_OF[objective], qrel_dict)
    if objective == "map":
        own = c.default_norms("ap")
        assert [norms[q - 1] - own[q - 1] for q in (4, 11, 13)] == [3.0, 1.0, 40.0] and norms[4] == own[4]
    for sigma, T, norm in ((1.0, 0, False), (1.5, 5, True)):
        exp = _expected(edge, objective, sigma, T, norm, norms, tag="qrel")
        lam, wt = native.lambda_gradients(model, g, "ndcg", sigma, qrel, truncation_level=T, lambda_norm=norm, objective=objective)
        _compare(lam, wt, exp, queries, norm)
        plain = native.lambda_gradients(model, g, "ndcg", sigma, truncation_level=T, lambda_norm=norm, objective=objective)[0]
        for q in (4, 11, 13):
            assert (plain[qid == q].tobytes() != lam[qid == q].tobytes()) == (objective == "map"), q


def test_a_query_sample_leaves_the_other_queries_alone(edge):
    X, y, qid, g, c, model, queries, _ = edge
    for objective, kw in (("map", dict()), ("mrr", dict(truncation_level=5, lambda_norm=True))):
        full_l, full_w = native.lambda_gradients(model, g, "ndcg", 1.5, objective=objective, **kw)
        for qsel in ([14], [1, 3, 12, 13]):
            lam, wt = native.lambda_gradients(model, g, "ndcg", 1.5, queries=np.asarray(qsel), objective=objective, **kw)
            inside = np.zeros(len(full_l), dtype=bool)
            inside[np.concatenate([queries[q] for q in qsel])] = True
            assert lam[inside].tobytes() == full_l[inside].tobytes() and wt[inside].tobytes() == full_w[inside].tobytes()
            assert np.all(np.isnan(lam[~inside])) and np.all(np.isnan(wt[~inside]))


def test_objective_ndcg_and_the_key_absent_give_the_same_gradient_bytes(edge):
    X, y, qid, g, c, model, queries, _ = edge
    for measure, kw in (("ndcg", dict()), ("ndcg@10", dict()), ("ndcg", dict(truncation_level=5, lambda_norm=True))):
        a = native.lambda_gradients(model, g, measure, 1.5, **kw)
        b = native.lambda_gradients(model, g, measure, 1.5, objective="ndcg", **kw)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        # ... also when the options object spells the default out
        out_l, out_w = np.full(len(y), np.nan), np.full(len(y), np.nan)
        opts = dict(objective="ndcg", **kw)
        native._status(native._load().fr_debug_lambda_gradients_opts(model.pointer, g.pointer, None, measure.encode(), 1.5, None, 0,
                                                                   json.dumps(opts).encode(), out_l.ctypes.data, out_w.ctypes.data, len(y)))
        assert out_l.tobytes() == a[0].tobytes() and out_w.tobytes() == a[1].tobytes()
        for objective in om.OBJECTIVES:
            assert native.lambda_gradients(model, g, measure, 1.5, objective=objective, **kw)[0].tobytes() != a[0].tobytes()


# --- training ------------------------------------------------------------------------------------

def _stagewise(case, grower, objective, params, trees_n=10, leafwise=None):
    X, y, qid, g, c = case
    req = _request("ndcg@7", grower, num_trees=trees_n, objective=objective, **params)
    p = req.params
    model = g.train_model(req)
    st = native.last_train_stats()["lambdamart"]
    assert st["objective"] == objective
    d = model.to_dict()
    trees = [m["DecisionTree"] for m in d["Ensemble"]["models"]]
    assert len(trees) == trees_n and d["Ensemble"]["weights"] == [p.learning_rate] * trees_n
    queries = lm.query_lists(c)
    order_ids = np.concatenate(queries)
    feats = list(range(X.shape[1]))
    binned = hm.bin_matrix(X, order_ids, feats, p.split_candidates) if grower == "histogram" else None
    for t in range(trees_n):
        lam, wt = native.lambda_gradients(_ensemble(trees[:t], p.learning_rate), g, "ndcg", p.sigma, objective=objective)
        if t == 0:  # the device's gradients are the restatement's (not NDCG's)
            exp_l, _ = om.gradients(np.zeros(len(y)), y, queries, c.default_norms(MEASURE_OF[objective]), objective, p.sigma)
            assert np.allclose(lam, exp_l, rtol=1e-12, atol=0.0)
        if leafwise is not None:
            exp = lw.tree_on_sample(X, lam, wt, order_ids, feats, binned, np.arange(len(order_ids)), np.arange(len(feats)), p.max_depth,
                                    p.min_leaf_support, p.split_candidates, p.max_leaves, **leafwise)
        elif grower == "histogram":
            exp = hm.fit_tree(X, lam, wt, order_ids, feats, p.max_depth, p.min_leaf_support, p.split_candidates, binned)
        else:
            exp = lm.fit_tree(X, lam, wt, order_ids, feats, p.max_depth, p.min_leaf_support, p.split_candidates)
        assert trees[t] == exp, "tree %d differs from the restatement's fit" % t
        exp_q, _ = c.metric_from_scores(MEASURE_OF[objective], c.score_ensemble(trees[:t + 1], [p.learning_rate] * (t + 1)))
        assert st["train_measure"][t] == o.mean(exp_q)
    assert np.array_equal(native.predict_scores_dense(model, g), c.score_ensemble(trees, d["Ensemble"]["weights"]))
    return json.dumps(d)


@pytest.mark.parametrize("objective", om.OBJECTIVES)
@pytest.mark.parametrize("grower", ["exact", "histogram"])
@pytest.mark.parametrize("data", ["trec", "synth"])
def test_stagewise_identity(request, data, grower, objective):
    """Fails where the key is ignored: the trees are then fitted to NDCG gradients."""
    case = request.getfixturevalue(data)
    params = dict(max_depth=5, min_leaf_support=5, split_candidates=16) if data == "trec" else dict(max_depth=4, min_leaf_support=10, split_candidates=12)
    got = _stagewise(case, grower, objective, params)
    plain = json.dumps(case[3].train_model(_request("ndcg@7", grower, num_trees=10, **params)).to_dict())
    assert got != plain


@pytest.mark.parametrize("objective", om.OBJECTIVES)
def test_stagewise_identity_leafwise_newton(synth, objective):
    gain = dict(split_gain="newton", lambda_l2=2.0 ** -10, min_sum_hessian=2.0 ** -6, min_split_gain=2.0 ** -20)
    params = dict(max_depth=10, min_leaf_support=10, split_candidates=64, max_leaves=12, **gain)
    _stagewise(synth, "histogram", objective, params, leafwise=gain)


@pytest.mark.parametrize("objective", om.OBJECTIVES)
def test_validation_and_early_stopping_follow_the_objective(synth, objective):
    X, y, qid, g, c = synth
    names = _names(qid)
    held = names[3::10]
    Tq, Hq = vm.split(names, held)
    rounds, T = 3, 25
    req = _request("ndcg@5", "histogram", num_trees=T, objective=objective, validation_queries=held, early_stopping_rounds=rounds,
                   max_depth=4, min_leaf_support=10, split_candidates=12, learning_rate=0.5)
    model = g.train_model(req)
    st = native.last_train_stats()["lambdamart"]
    assert st["objective"] == objective
    n = st["trees"]
    assert len(st["train_measure"]) == n == len(st["valid_measure"])
    # the trees the stats speak of: the returned ones are the first best_iteration of them, so retrain without the rule
    full = g.train_model(_request("ndcg@5", "histogram", num_trees=n, objective=objective, validation_queries=held,
                                  max_depth=4, min_leaf_support=10, split_candidates=12, learning_rate=0.5))
    trees = [m["DecisionTree"] for m in full.to_dict()["Ensemble"]["models"]]
    for t in range(n):
        exp_q, _ = c.metric_from_scores(MEASURE_OF[objective], c.score_ensemble(trees[:t + 1], [0.5] * (t + 1)))
        assert st["train_measure"][t] == vm.subset_mean(exp_q, Tq) and st["valid_measure"][t] == vm.subset_mean(exp_q, Hq)
    valid = st["valid_measure"]
    best = 1 + int(np.argmax(valid))  # the FIRST maximum
    assert st["best_iteration"] == best and st["best_valid_measure"] == valid[best - 1]
    assert n == min(T, best + rounds) and st["stopped_early"] == (n < T)
    got = [m["DecisionTree"] for m in model.to_dict()["Ensemble"]["models"]]
    assert got == trees[:best]


@pytest.mark.parametrize("grower", ["exact", "histogram"])
def test_objective_ndcg_is_the_key_absent(synth, grower):
    X, y, qid, g, c = synth
    kw = dict(num_trees=4, max_depth=4, min_leaf_support=10, split_candidates=12)
    plain = _request("ndcg", grower, **kw)
    assert "objective" not in plain.to_dict()["params"]["LambdaMART"]
    a = json.dumps(g.train_model(plain).to_dict())
    stats = native.last_train_stats()["lambdamart"]
    keys = set(stats)
    wire = plain.to_dict()
    wire["params"]["LambdaMART"]["objective"] = "ndcg"
    b = clib._unwrap(clib._load().train_model(json.dumps(wire).encode(), g.pointer))
    again = native.last_train_stats()["lambdamart"]
    assert set(again) == keys and "objective" not in keys and again["train_measure"] == stats["train_measure"]
    assert json.dumps(fr.CModel(b).to_dict()) == a
