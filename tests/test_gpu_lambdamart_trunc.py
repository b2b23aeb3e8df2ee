"""LambdaRank truncation level and per-query normalisation on the device (lambda_grad_trunc_kernel) against the numpy
restatement (tests/lambdamart_trunc_model.py, DESIGN.md section 11, "Truncation and normalisation").

Gradients: rtol 1e-12 with exact zeros, the figure of tests/test_gpu_lambdamart.py (the operations are the same, over fewer
partners).  Under lambda_norm the scale f = log2(1 + S) / S is a further library call on a sum that differs between the
two sides, so the tolerance is derived (`_norm_rtol`), from the method of tests/lambdamart_bound.py (u = 2^-53, a library
result within 2 ulp = 4u relative):
  * A_p is a sum of terms >= 0 that each lie within 1e-12 (the unnormalised property), so S lies within 1e-12 relative;
  * x = fl(1 + S) then differs by at most 1e-12 S + 2u (1 + S) between the two sides, log2(x) by that over x ln(1 + S) plus
    the two library errors 8u; S / ((1 + S) ln(1 + S)) <= 1, so log2 differs by at most 1e-12 + 2u / ln(1 + S) + 8u relative;
  * the division by S adds 1e-12 + 2u, the product with lambda (itself within 1e-12) 1e-12 + 2u:
    rtol = 3e-12 + 2u / ln(1 + S) + 12u.  For S >= 1e-3 that is below 3.3e-12.
Training: every tree equals the restatement's fit to the DEVICE's gradients of the prefix model, bit for bit.
"""
import json
import math
import os

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import native
from oracle import pyoracle as o
from tests import lambdamart_hist_model as hm
from tests import lambdamart_leafwise_model as lw
from tests import lambdamart_model as lm
from tests import lambdamart_sample_model as sm
from tests import lambdamart_trunc_model as tm
from tests import lambdamart_valid_model as vm
from tests.lambdamart_composed_model import _ensemble, _names, _request
from tests.conftest import GOLDEN, synth_dataset

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
_LABEL_P = [0.515, 0.324, 0.134, 0.019, 0.008]
T0 = 5  # the truncation level the edge set is built around


def _norm_rtol(S):
    return 3e-12 + 2.0 * U / math.log1p(S) + 12.0 * U


def _edge_set():
    """Queries (stored order = row order) built around T0 = 5: 1, 2, T0 - 1, T0, T0 + 1 documents; 300 (more than one
    document per thread) and 1 300; a score tie straddling ranks T0 - 1 | T0 whose members differ in label and id; a query
    whose top T0 all carry one label; all labels equal; no positive label.  Column 0 is the score (integers: many ties)."""
    rng = np.random.default_rng(77)
    lens = {1: 1, 2: 2, 3: T0 - 1, 4: T0, 5: T0 + 1, 6: 300, 7: 1300, 8: 40, 9: 40, 10: 25, 11: 25, 12: 120}
    qid = np.concatenate([np.full(n, q, dtype=np.int64) for q, n in lens.items()])
    n = len(qid)
    y = rng.choice(5, size=n, p=_LABEL_P).astype(np.float64)
    s = np.floor(rng.exponential(3.0, n))
    y[qid == 2] = [2.0, 0.0]
    for q in (3, 4, 5):
        y[qid == q] = rng.permutation(np.arange(lens[q]) % 3).astype(np.float64)
    # query 8: three documents above, then a tie group of 30 at score 5 holding ranks 3..32 (T0 - 1 = 4 and T0 = 5 among them)
    s8 = np.full(40, 1.0)
    s8[[7, 19, 33]] = 9.0
    s8[rng.permutation(np.setdiff1d(np.arange(40), [7, 19, 33]))[:30]] = 5.0
    s[qid == 8] = s8
    y[qid == 8] = rng.choice(3, size=40).astype(np.float64)
    # query 9: the T0 best scores all carry label 2
    s9 = rng.permutation(40).astype(np.float64)
    y9 = rng.choice([0.0, 1.0, 3.0], size=40)
    y9[np.argsort(-s9)[:T0]] = 2.0
    s[qid == 9], y[qid == 9] = s9, y9
    y[qid == 10] = 2.0
    y[qid == 11] = 0.0
    X = np.zeros((n, 3), dtype=np.float32)
    X[:, 0] = s
    X[:, 1] = rng.random(n)
    X[:, 2] = rng.integers(0, 4, n)
    return X, y, qid


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
    X, y, qid = synth_dataset(7, 5000, 10, 50)
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


def _expected(edge, measure, sigma, T, norm):
    X, y, qid, g, c, model, queries, cache = edge
    key = (measure, sigma, T, norm)
    if key not in cache:
        scores = native.predict_scores_dense(model, g)
        cache[key] = tm.gradients(scores, y, queries, c.default_norms(measure), lm.depth_of(measure), sigma, T, norm, parts=True)
    return cache[key]


@pytest.mark.parametrize("measure,sigma,T,norm", [
    ("ndcg", 1.5, T0, False), ("ndcg", 0.3, T0, True), ("ndcg", 1.5, 1, False), ("ndcg", 0.3, 1, True),
    ("ndcg@10", 1.5, 30, True), ("ndcg@3", 0.3, T0, False), ("ndcg", 1.5, 0, True), ("ndcg", 0.3, 100, False)])
def test_gradients_match_the_restatement(edge, measure, sigma, T, norm):
    X, y, qid, g, c, model, queries, _ = edge
    exp = _expected(edge, measure, sigma, T, norm)
    lam, wt = native.lambda_gradients(model, g, measure, sigma, truncation_level=T, lambda_norm=norm)
    _compare(lam, wt, exp, queries, norm)
    for q in (1, 10, 11):  # one document, all labels equal, no positive label
        assert not lam[qid == q].any() and not wt[qid == q].any()
    for q in (2, 3, 4, 5, 6, 7, 8, 9):
        assert lam[qid == q].any(), q
    if T == T0:  # the edge set is what its docstring says
        scores = X[:, 0].astype(np.float64)
        ids8 = queries[7]
        r8 = tm.ranks(scores[ids8], y[ids8].astype(np.float32), ids8)
        a, b = ids8[r8 == T0 - 1][0], ids8[r8 == T0][0]
        assert scores[a] == scores[b] == 5.0
        ids9 = queries[8]
        r9 = tm.ranks(scores[ids9], y[ids9].astype(np.float32), ids9)
        assert set(y[ids9][r9 < T0]) == {2.0}
        if not norm:  # a top document there meets no other top document: its lambda is the untruncated one
            full = native.lambda_gradients(model, g, measure, sigma)[0]
            assert np.array_equal(lam[ids9][r9 < T0], full[ids9][r9 < T0])
            if measure == "ndcg":  # (under ndcg@3 the pairs T0 = 5 cuts have delta = 0)
                assert not np.array_equal(lam[ids9][r9 >= T0], full[ids9][r9 >= T0])
    # a second call gives the same bytes
    lam2, wt2 = native.lambda_gradients(model, g, measure, sigma, truncation_level=T, lambda_norm=norm)
    assert lam2.tobytes() == lam.tobytes() and wt2.tobytes() == wt.tobytes()


@pytest.mark.parametrize("measure,levels", [("ndcg", [1300, 5000, 2 ** 32 - 1]), ("ndcg@3", [1300]), ("ndcg@10", [10, 30, 1300])])
def test_levels_that_cut_nothing_give_the_untruncated_bytes(edge, measure, levels):
    """(a) T at least the longest query; (b) under ndcg@k any T >= k: the skipped pairs have delta = 0 exactly."""
    X, y, qid, g, c, model, queries, _ = edge
    for sigma in (0.3, 1.5):
        lam, wt = native.lambda_gradients(model, g, measure, sigma)
        for T in levels:
            tl, tw = native.lambda_gradients(model, g, measure, sigma, truncation_level=T)
            assert tl.tobytes() == lam.tobytes() and tw.tobytes() == wt.tobytes(), (measure, sigma, T)
    if measure == "ndcg@10":  # ... and a level below k does cut
        tl, _ = native.lambda_gradients(model, g, measure, 1.5, truncation_level=9)
        assert tl.tobytes() != lam.tobytes()


def test_slab_and_lds_limit():
    """4 096 documents (the LDS limit: the staging plus the kernel's own tile) and 4 097 (the global slab), next to short
    queries, under T = 30 with normalisation."""
    rng = np.random.default_rng(43)
    lens = [300, 4097, 1, 4096, 2]
    qid = np.repeat(np.arange(1, len(lens) + 1, dtype=np.int64), lens)
    n = len(qid)
    y = rng.choice(5, size=n, p=_LABEL_P).astype(np.float64)
    X = np.empty((n, 2), dtype=np.float32)
    X[:, 0] = rng.random(n) + 0.3 * y
    X[:, 1] = np.floor(rng.exponential(2.0, n))
    g, c = fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)
    model = fr.CModel.from_dict({"Linear": {"weights": [0.25, 1.0]}})
    queries = lm.query_lists(c)
    scores = native.predict_scores_dense(model, g)
    exp = tm.gradients(scores, y, queries, c.default_norms("ndcg"), None, 1.5, 30, True, parts=True)
    lam, wt = native.lambda_gradients(model, g, "ndcg", 1.5, truncation_level=30, lambda_norm=True)
    _compare(lam, wt, exp, queries, True)
    for q in (1, 2, 4):
        assert lam[qid == q].any(), q
    full_l, full_w = native.lambda_gradients(model, g, "ndcg", 1.5)
    tl, tw = native.lambda_gradients(model, g, "ndcg", 1.5, truncation_level=4097)
    assert tl.tobytes() == full_l.tobytes() and tw.tobytes() == full_w.tobytes()


def test_qrel_norms(trec):
    X, y, qid, g, c = trec
    with open(os.path.join(GOLDEN, "newsir18_entity_qrel.json")) as fh:
        qrel_dict = json.load(fh)
    qrel = fr.CQRel.from_dict(qrel_dict)
    model = fr.CModel.from_dict({"Linear": {"weights": [0.0, 0.3, -0.2, 0.5, 0.1, 0.9]}})
    queries = lm.query_lists(c)
    scores = native.predict_scores_dense(model, g)
    for measure, T, norm in (("ndcg", 5, True), ("ndcg@5", 3, False)):
        exp = tm.gradients(scores, y, queries, c.qrel_norms(measure, qrel_dict), lm.depth_of(measure), 1.0, T, norm, parts=True)
        lam, wt = native.lambda_gradients(model, g, measure, 1.0, qrel, truncation_level=T, lambda_norm=norm)
        _compare(lam, wt, exp, queries, norm)


def test_a_query_sample_leaves_the_other_queries_alone(edge):
    X, y, qid, g, c, model, queries, _ = edge
    kw = dict(truncation_level=T0, lambda_norm=True)
    full_l, full_w = native.lambda_gradients(model, g, "ndcg", 1.5, **kw)
    for qsel in ([6], [0, 3, 7], [1, 2, 4, 5, 8, 9, 10, 11]):
        lam, wt = native.lambda_gradients(model, g, "ndcg", 1.5, queries=np.asarray(qsel), **kw)
        inside = np.zeros(len(full_l), dtype=bool)
        inside[np.concatenate([queries[q] for q in qsel])] = True
        assert lam[inside].tobytes() == full_l[inside].tobytes() and wt[inside].tobytes() == full_w[inside].tobytes()
        assert np.all(np.isnan(lam[~inside])) and np.all(np.isnan(wt[~inside]))
    again_l, again_w = native.lambda_gradients(model, g, "ndcg", 1.5, **kw)
    assert again_l.tobytes() == full_l.tobytes() and again_w.tobytes() == full_w.tobytes()


# --- training ------------------------------------------------------------------------------------

def _stagewise(case, grower, measure, T, norm, params, trees_n=10):
    X, y, qid, g, c = case
    req = _request(measure, grower, num_trees=trees_n, truncation_level=T, lambda_norm=norm, **params)
    p = req.params
    model = g.train_model(req)
    st = native.last_train_stats()["lambdamart"]
    assert st.get("truncation_level", 0) == T and st.get("lambda_norm", False) == norm
    assert ("truncation_level" in st) == (T != 0) and ("lambda_norm" in st) == norm
    d = model.to_dict()
    trees = [m["DecisionTree"] for m in d["Ensemble"]["models"]]
    assert len(trees) == trees_n and d["Ensemble"]["weights"] == [p.learning_rate] * trees_n
    order_ids = np.concatenate(lm.query_lists(c))
    feats = list(range(X.shape[1]))
    binned = hm.bin_matrix(X, order_ids, feats, p.split_candidates) if grower == "histogram" else None
    for t in range(trees_n):
        lam, wt = native.lambda_gradients(_ensemble(trees[:t], p.learning_rate), g, measure, p.sigma, truncation_level=T, lambda_norm=norm)
        if grower == "histogram":
            exp = hm.fit_tree(X, lam, wt, order_ids, feats, p.max_depth, p.min_leaf_support, p.split_candidates, binned)
        else:
            exp = lm.fit_tree(X, lam, wt, order_ids, feats, p.max_depth, p.min_leaf_support, p.split_candidates)
        assert trees[t] == exp, "tree %d differs from the restatement's fit" % t
        exp_q, _ = c.metric_from_scores(measure, c.score_ensemble(trees[:t + 1], [p.learning_rate] * (t + 1)))
        assert st["train_measure"][t] == o.mean(exp_q)
    assert np.array_equal(native.predict_scores_dense(model, g), c.score_ensemble(trees, d["Ensemble"]["weights"]))
    return json.dumps(d)


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("grower", ["exact", "histogram"])
@pytest.mark.parametrize("data", ["trec", "synth"])
def test_stagewise_identity(request, data, grower, norm):
    case = request.getfixturevalue(data)
    params = dict(max_depth=5, min_leaf_support=5, split_candidates=16) if data == "trec" else dict(max_depth=4, min_leaf_support=10, split_candidates=12)
    got = _stagewise(case, grower, "ndcg", 30, norm, params)
    plain = json.dumps(case[3].train_model(_request("ndcg", grower, num_trees=10, **params)).to_dict())
    assert got != plain  # (T = 30 cuts pairs on both sets: the options are not a no-op here)


def test_stagewise_identity_composed(synth):
    """T = 30 and normalisation under the Newton gain, a leaf budget, per-tree samples and held-out queries."""
    X, y, qid, g, c = synth
    names = _names(qid)
    held, rates, seed, T = names[3::10], (0.5, 0.5), 1, 10
    gain = dict(split_gain="newton", lambda_l2=2.0 ** -10, min_sum_hessian=2.0 ** -6, min_split_gain=2.0 ** -20)
    req = _request("ndcg", "histogram", num_trees=T, truncation_level=30, lambda_norm=True, max_depth=10, min_leaf_support=10, split_candidates=64,
                   max_leaves=12, query_sampling_rate=rates[0], feature_sampling_rate=rates[1], seed=seed, validation_queries=held, **gain)
    p = req.params
    model = g.train_model(req)
    st = native.last_train_stats()["lambdamart"]
    assert st["truncation_level"] == 30 and st["lambda_norm"] is True and st["max_leaves"] == 12 and st["split_gain"] == "newton"
    trees = [m["DecisionTree"] for m in model.to_dict()["Ensemble"]["models"]]
    assert len(trees) == T
    queries = lm.query_lists(c)
    order_ids = np.concatenate(queries)
    feats = list(range(X.shape[1]))
    binned = hm.bin_matrix(X, order_ids, feats, p.split_candidates)
    Tq, Hq = vm.split(names, held)
    for t in range(T):
        fsel, qsel = vm.sample(seed, t, len(feats), Tq, rates)
        lam, wt = native.lambda_gradients(_ensemble(trees[:t], p.learning_rate), g, "ndcg", p.sigma, truncation_level=30, lambda_norm=True)
        exp = lw.tree_on_sample(X, lam, wt, order_ids, feats, binned, sm.instance_rows(queries, qsel), fsel, p.max_depth, p.min_leaf_support,
                                p.split_candidates, p.max_leaves, **gain)
        assert trees[t] == exp, "tree %d differs from the restatement's fit" % t
        exp_q, _ = c.metric_from_scores("ndcg", c.score_ensemble(trees[:t + 1], [p.learning_rate] * (t + 1)))
        assert st["train_measure"][t] == vm.subset_mean(exp_q, Tq) and st["valid_measure"][t] == vm.subset_mean(exp_q, Hq)
    assert np.array_equal(native.predict_scores_dense(model, g), c.score_ensemble(trees, [p.learning_rate] * T))


@pytest.mark.parametrize("grower", ["exact", "histogram"])
def test_keys_at_their_defaults_give_the_plain_model(synth, grower):
    X, y, qid, g, c = synth
    kw = dict(num_trees=4, max_depth=4, min_leaf_support=10, split_candidates=12)
    plain = _request("ndcg", grower, **kw)
    assert "truncation_level" not in plain.to_dict()["params"]["LambdaMART"] and "lambda_norm" not in plain.to_dict()["params"]["LambdaMART"]
    a = json.dumps(g.train_model(plain).to_dict())
    keys = set(native.last_train_stats()["lambdamart"])
    wire = plain.to_dict()
    wire["params"]["LambdaMART"].update(truncation_level=0, lambda_norm=False)
    from fastrank_amd import clib

    b = clib._unwrap(clib._load().train_model(json.dumps(wire).encode(), g.pointer))
    assert set(native.last_train_stats()["lambdamart"]) == keys and "truncation_level" not in keys and "lambda_norm" not in keys
    assert json.dumps(fr.CModel(b).to_dict()) == a
    # ... and a level no query reaches, through the other kernel, gives those bytes too
    assert json.dumps(g.train_model(_request("ndcg", grower, truncation_level=10 ** 6, **kw)).to_dict()) == a
