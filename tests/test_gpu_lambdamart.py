"""LambdaMART on the device against the numpy restatement (tests/lambdamart_model.py)."""
import json
import os

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import native
from oracle import pyoracle as o
from tests import lambdamart_model as lm
from tests import lambdamart_bound as hx
from tests.conftest import GOLDEN, ranksvm_presence, synth_dataset

pytestmark = pytest.mark.gpu


def _request(measure="ndcg", **kw):
    req = fr.TrainRequest.lambdamart()
    req.measure = measure
    req.params.quiet = True
    for k, v in kw.items():
        setattr(req.params, k, v)
    return req


@pytest.fixture(scope="module")
def trec():
    d = np.load(os.path.join(GOLDEN, "trec_news_2018.npz"))
    X, y, qid = d["train_X"], d["train_y"], d["train_qid"]
    return X, y, qid, fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)


@pytest.fixture(scope="module")
def qrel_dict():
    with open(os.path.join(GOLDEN, "newsir18_entity_qrel.json")) as fh:
        return json.load(fh)


def _tied_set():
    """Queries of 1, 2 and up to 1 300 documents; one query without a positive label, one whose labels are all equal."""
    X, y, qid = synth_dataset(21, 6000, 8, 40, max_len=1300)
    qid = qid.copy()
    qid[-1300:] = 2000  # one query of 1 300 documents
    # query 1 -> one document, query 2 -> two documents (moved to fresh qids 1001 / 1002)
    first = np.flatnonzero(qid == 1)
    qid[first[0]] = 1001
    second = np.flatnonzero(qid == 2)
    qid[second[:2]] = 1002
    y = y.copy()
    y[qid == 3] = 0.0  # no positive label
    y[qid == 4] = 2.0  # all labels equal
    return X, y, qid


def _check_gradients(g, c, X, y, model, measure, norms, qrel=None, sigma=1.0):
    scores = native.predict_scores_dense(model, g)
    lam, wt = native.lambda_gradients(model, g, measure, sigma, qrel)
    queries = lm.query_lists(c)
    elam, ewt = lm.gradients(scores, y, queries, norms, lm.depth_of(measure), sigma)
    assert np.all(np.isfinite(lam)) and np.all(np.isfinite(wt))
    for got, exp in ((lam, elam), (wt, ewt)):
        zero = exp == 0.0
        assert np.array_equal(got[zero], exp[zero])
        np.testing.assert_allclose(got, exp, rtol=1e-12, atol=0.0)
    for ids in queries:
        assert abs(lam[ids].sum()) <= 1e-9 * max(1.0, np.abs(lam[ids]).sum())
    return lam, wt


@pytest.mark.parametrize("measure", ["ndcg", "ndcg@1", "ndcg@10", "ndcg@5000"])
def test_gradient_kernel_matches_restatement(measure):
    X, y, qid = _tied_set()
    g, c = fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)
    # a linear model on the integer columns: many tied scores
    w = [0.0] * X.shape[1]
    w[1], w[5] = 1.0, 2.0
    model = fr.CModel.from_dict({"Linear": {"weights": w}})
    lam, wt = _check_gradients(g, c, X, y, model, measure, c.default_norms(measure), sigma=1.5)
    assert np.all(lam[qid == 3] == 0.0) and np.all(wt[qid == 3] == 0.0)
    assert np.all(lam[qid == 4] == 0.0) and np.all(wt[qid == 4] == 0.0)
    assert np.all(lam[qid == 1001] == 0.0)
    assert np.any(lam[qid == 1002] != 0.0) or len(set(y[qid == 1002])) == 1


def test_gradient_kernel_with_qrel_norms(trec, qrel_dict):
    X, y, qid, g, c = trec
    qrel = fr.CQRel.from_dict(qrel_dict)
    model = fr.CModel.from_dict({"Linear": {"weights": [0.0, 0.3, -0.2, 0.5, 0.1, 0.9]}})
    for measure in ("ndcg", "ndcg@5"):
        _check_gradients(g, c, X, y, model, measure, c.qrel_norms(measure, qrel_dict), qrel=qrel)


def _stagewise(g, c, X, y, measure, T, params):
    req = _request(measure, num_trees=T, **params)
    model = g.train_model(req)
    d = model.to_dict()
    trees = [m["DecisionTree"] for m in d["Ensemble"]["models"]]
    assert d["Ensemble"]["weights"] == [req.params.learning_rate] * T
    queries = lm.query_lists(c)
    order_ids = np.concatenate(queries)
    for t in range(T):
        prefix = fr.CModel.from_dict({"Ensemble": {"weights": [req.params.learning_rate] * t,
                                                   "models": [{"DecisionTree": x} for x in trees[:t]]}})
        lam, wt = native.lambda_gradients(prefix, g, measure, req.params.sigma)
        exp = lm.fit_tree(X, lam, wt, order_ids, range(X.shape[1]), req.params.max_depth, req.params.min_leaf_support,
                          req.params.split_candidates)
        assert trees[t] == exp, "tree %d differs from the restatement's fit" % t
    return model, req


def test_stagewise_identity_trec(trec):
    X, y, qid, g, c = trec
    _stagewise(g, c, X, y, "ndcg@10", 20, dict(max_depth=5, min_leaf_support=5, split_candidates=16, learning_rate=0.1))


_LABEL_P = [0.515, 0.324, 0.134, 0.019, 0.008]


def _long_query_set():
    """Queries beyond the LDS budget of lambda_grad_kernel (LM_LDS_MAX: 4 096 documents) take a per-block global slab.
    Here 4 095 and 4 096 documents (LDS, the second at its limit), 4 097, 4 099 and 6 001 (slab), 5 000 without a positive
    label (slab, the zero branch), and 1, 2 and 300.  Slab launch order (longest first): 6 001, 5 000, 4 099, 4 097.  A slab
    block holds 36 * max_len bytes and max_len = 6 001 is odd, so the f64 arrays of block 3 (the 4 097-document query)
    start 4 bytes off 8-byte alignment."""
    rng = np.random.default_rng(43)
    lens = [300, 4097, 1, 6001, 4095, 5000, 2, 4099, 4096]
    qid = np.repeat(np.arange(1, len(lens) + 1, dtype=np.int64), lens)
    n = len(qid)
    y = rng.choice(5, size=n, p=_LABEL_P).astype(np.float64)
    y[qid == 6] = 0.0
    X = np.empty((n, 6), dtype=np.float32)
    X[:, 0] = rng.random(n) + 0.3 * y
    X[:, 1] = np.floor(rng.exponential(2.0, n))  # integer columns: tied scores
    X[:, 2] = rng.lognormal(0.0, 2.0, n)
    X[:, 3] = np.where(rng.random(n) < 0.7, 0.0, rng.random(n))
    X[:, 4] = rng.integers(0, 5, n)
    X[:, 5] = rng.normal(0.0, 1.0, n)
    return X, y, qid


@pytest.mark.parametrize("measure", ["ndcg", "ndcg@10", "ndcg@5000"])
def test_gradient_kernel_on_queries_longer_than_lds(measure):
    X, y, qid = _long_query_set()
    g, c = fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)
    model = fr.CModel.from_dict({"Linear": {"weights": [0.25, 1.0, 0.0, 0.0, 0.5, 0.0]}})
    lam, wt = _check_gradients(g, c, X, y, model, measure, c.default_norms(measure), sigma=1.5)
    assert np.all(lam[qid == 6] == 0.0) and np.all(wt[qid == 6] == 0.0)
    assert np.all(lam[qid == 3] == 0.0) and np.all(wt[qid == 3] == 0.0)
    for q in (1, 2, 4, 5, 8, 9):
        assert np.any(lam[qid == q] != 0.0), q


def test_stagewise_identity_on_queries_longer_than_lds():
    X, y, qid = _long_query_set()
    g, c = fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)
    _stagewise(g, c, X, y, "ndcg@10", 3, dict(max_depth=3, min_leaf_support=20, split_candidates=8, learning_rate=0.1))


def test_gradient_kernel_on_more_slab_queries_than_one_launch_takes():
    """1 030 queries of 4 097 - 4 099 documents: all in the slab, launched LM_SLAB_BLOCKS = 1 024 at a time, so a second
    launch starts at q_first = 1 024 (max_len 4 099: every odd block misaligned).  Launch order is longest first and
    stable; the queries at launch order 0, 1 023 (the first launch's last block), 1 024 (the second launch's first) and
    1 029 (the last) are restated, every query's gradients are finite and sum to ~0."""
    rng = np.random.default_rng(47)
    nq = 1030
    lens = rng.integers(4097, 4100, nq)
    lens[517] = 4099
    qid = np.repeat(np.arange(1, nq + 1, dtype=np.int64), lens)
    n = len(qid)
    y = rng.choice(5, size=n, p=_LABEL_P).astype(np.float64)
    X = np.stack([rng.random(n) + 0.3 * y, np.floor(rng.exponential(2.0, n))], axis=1).astype(np.float32)
    g, c = fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)
    model = fr.CModel.from_dict({"Linear": {"weights": [1.0, 0.5]}})
    measure = "ndcg@10"
    lam, wt = native.lambda_gradients(model, g, measure, 1.0)
    assert np.all(np.isfinite(lam)) and np.all(np.isfinite(wt))
    queries = lm.query_lists(c)
    qlen = [len(ids) for ids in queries]
    order = sorted(range(nq), key=lambda q: -qlen[q])  # (stable, as the launch order)
    pick = [order[0], order[1023], order[1024], order[-1]]
    norms = c.default_norms(measure)
    scores = native.predict_scores_dense(model, g)
    elam, ewt = lm.gradients(scores, y, [queries[q] for q in pick], norms[pick], lm.depth_of(measure), 1.0)
    for q in pick:
        ids = queries[q]
        for got, exp in ((lam[ids], elam[ids]), (wt[ids], ewt[ids])):
            zero = exp == 0.0
            assert np.array_equal(got[zero], exp[zero]), q
            np.testing.assert_allclose(got, exp, rtol=1e-12, atol=0.0)
        assert np.any(lam[ids] != 0.0), q
    for ids in queries:
        assert abs(lam[ids].sum()) <= 1e-9 * max(1.0, np.abs(lam[ids]).sum())


def test_stagewise_identity_synthetic():
    X, y, qid = synth_dataset(7, 5000, 10, 50)
    g, c = fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)
    _stagewise(g, c, X, y, "ndcg", 20, dict(max_depth=4, min_leaf_support=10, split_candidates=12, sigma=1.0))


def _train_stats(g, req):
    model = g.train_model(req)
    st = native.last_train_stats()
    assert st["path"] == "lambdamart"
    return model, st["lambdamart"]


@pytest.mark.parametrize("measure", ["ndcg", "ndcg@10"])
def test_running_scores_equal_prediction(trec, measure):
    X, y, qid, g, c = trec
    model, st = _train_stats(g, _request(measure, num_trees=12, max_depth=4, min_leaf_support=5, split_candidates=16))
    assert st["trees"] == 12 and len(st["train_measure"]) == 12
    for key in ("seconds", "gradient_ms", "grow_ms", "leaves_ms", "update_ms"):
        assert st[key] >= 0.0
    _, per_q = native.evaluate_dense(model, g, measure)
    assert st["train_measure"][-1] == o.mean(per_q)
    d = model.to_dict()["Ensemble"]
    exp = c.score_ensemble([m["DecisionTree"] for m in d["models"]], d["weights"])
    assert np.array_equal(native.predict_scores_dense(model, g), exp)


def test_learning_happens():
    X, y, qid = synth_dataset(3, 5000, 16, 60)
    g, c = fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)
    model, st = _train_stats(g, _request("ndcg@10", num_trees=50, split_candidates=32))
    assert st["train_measure"][-1] > st["train_measure"][0]
    zero = fr.CModel.from_dict({"Linear": {"weights": [0.0] * X.shape[1]}})
    _, base = native.evaluate_dense(zero, g, "ndcg@10")
    _, mine = native.evaluate_dense(model, g, "ndcg@10")
    assert np.nanmean(mine) > np.nanmean(base) + 0.05


def test_full_restatement_small(trec):
    """The whole loop on the CPU gives the device's model (the exp of the two sides may differ in the last bit, so the
    CPU's own gradients can in principle pick another split: a tiny dataset and few trees)."""
    X, y, qid, g, c = trec
    req = _request("ndcg@5", num_trees=3, max_depth=3, min_leaf_support=5, split_candidates=8)
    model = g.train_model(req)
    exp, s = lm.train(X, y, c, "ndcg@5", num_trees=3, learning_rate=0.1, max_depth=3, min_leaf_support=5,
                      split_candidates=8)
    got = model.to_dict()
    assert [m["DecisionTree"] for m in got["Ensemble"]["models"]] == [m["DecisionTree"] for m in exp["Ensemble"]["models"]] or \
        np.allclose(native.predict_scores_dense(model, g), s, rtol=1e-9, atol=1e-12)


def test_query_subsample_trains_like_its_own_rows(trec):
    X, y, qid, g, c = trec
    names = sorted(g.queries())
    sub_q = names[::2]
    sub = g.subsample_queries(sub_q)
    rows = np.isin(np.array([str(int(q)) for q in qid]), sub_q)
    own = fr.CDataset.from_numpy(np.ascontiguousarray(X[rows]), np.ascontiguousarray(y[rows]), np.ascontiguousarray(qid[rows]))
    req = _request("ndcg@10", num_trees=8, max_depth=4, min_leaf_support=4, split_candidates=16)
    assert sub.train_model(req).to_dict() == own.train_model(req).to_dict()


def _fids(node, out):
    if "FeatureSplit" in node:
        out.add(node["FeatureSplit"]["fid"])
        _fids(node["FeatureSplit"]["lhs"], out)
        _fids(node["FeatureSplit"]["rhs"], out)
    return out


def test_feature_subsample_uses_only_its_features(trec):
    X, y, qid, g, c = trec
    names = sorted(g.feature_names())
    keep = names[1::2]
    sub = g.subsample_feature_names(keep)
    allowed = set(sub.feature_ids())
    model = sub.train_model(_request("ndcg", num_trees=10, max_depth=4, min_leaf_support=4, split_candidates=16))
    used = set()
    for m in model.to_dict()["Ensemble"]["models"]:
        _fids(m["DecisionTree"], used)
    assert used and used <= allowed


def test_ranksvm_dataset_trains():
    rd = fr.CDataset.open_ranksvm(os.path.join(GOLDEN, "data", "trec_news_2018.train"))
    model = rd.train_model(_request("ndcg@5", num_trees=5, max_depth=3, min_leaf_support=5, split_candidates=8))
    assert len(model.to_dict()["Ensemble"]["models"]) == 5
    vals = rd.evaluate(model, "ndcg@5")
    assert all(np.isfinite(v) for v in vals.values())


def test_deterministic_and_single_device(trec, monkeypatch):
    X, y, qid, g, c = trec
    req = _request("ndcg", num_trees=6, max_depth=4, min_leaf_support=5, split_candidates=16)
    a = json.dumps(g.train_model(req).to_dict())
    b = json.dumps(g.train_model(req).to_dict())
    assert a == b
    monkeypatch.setenv("FR_DEVICES", "0,0")
    g2 = fr.CDataset.from_numpy(X, y, qid)
    assert json.dumps(g2.train_model(req).to_dict()) == a
    assert native.last_train_stats()["devices"] == 1


def test_quiet_false_prints_one_line_per_tree(trec, capfd):
    X, y, qid, g, c = trec
    req = _request("ndcg", num_trees=3, max_depth=3, min_leaf_support=5, split_candidates=8)
    req.params.quiet = False
    g.train_model(req)
    out = capfd.readouterr().out
    rows = [l for l in out.splitlines() if l.startswith("|") and l.strip("|").split("|")[0].strip().isdigit()]
    assert len(rows) == 3


# --- the kernel against exact arithmetic (tests/lambdamart_exact.py; the bound: tests/test_lambdamart_exact_host.py) -------

def _designed_dataset():
    queries = hx.designed_queries() + hx.random_queries(3, 12)
    X, y, qid = hx.as_dataset(queries)
    return X, y, qid, fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)


@pytest.mark.parametrize("sigma", hx.SIGMAS)
def test_gradient_kernel_within_bound_of_exact_on_designed_queries(sigma):
    """Equal scores, saturated gaps both ways, labels 0.5 / -1 / 30, one positive label, random queries of 2..400
    documents, as one dataset of short queries; depths none / 1 / 10 / beyond the query.  Every document's lambda and w lie
    within the derived bound of the exact value (the same constants as on the CPU side, the 2 ulp assumed for exp among
    them).  One designed input does not carry over: the scores must come from `predict_scores_dense`, and a linear
    model's sum turns -0.0 into +0.0, so the "signed zeros" query reaches the kernel as all +0.0 (one more all-equal
    query); the -0.0 / +0.0 mix is held on the CPU side only."""
    X, y, qid, g, c = _designed_dataset()
    model = fr.CModel.from_dict({"Linear": {"weights": hx.WEIGHTS}})
    scores = native.predict_scores_dense(model, g)
    worst = 0.0
    for measure in hx.MEASURES:
        norms = c.default_norms(measure)
        lam, wt = native.lambda_gradients(model, g, measure, sigma)
        worst = max(worst, hx.check_dataset(c, scores, y, lam, wt, measure, sigma, norms))
    print("kernel, designed queries, sigma %s: worst error / bound = %.4f" % (sigma, worst))


_CONTINUOUS = [0.25, 1.0, 0.0, 0.0, 0.5, 0.0]  # the model of the rtol tests above: column 0 is continuous, ties are rare
_INTEGER = [0.0, 1.0, 0.0, 0.0, 0.5, 0.0]      # the integer columns only: a few dozen scores, tie groups of hundreds


@pytest.mark.parametrize("weights,measure,sigma", [(_CONTINUOUS, "ndcg", 0.3), (_CONTINUOUS, "ndcg@10", 1.0), (_CONTINUOUS, "ndcg@5000", 1.5),
                                                   (_INTEGER, "ndcg@10", 1.5), (_INTEGER, "ndcg", 1.0)],
                         ids=["continuous-ndcg-0.3", "continuous-ndcg@10-1.0", "continuous-ndcg@5000-1.5", "tied-ndcg@10-1.5", "tied-ndcg-1.0"])
def test_gradient_kernel_within_bound_of_exact_on_long_queries(weights, measure, sigma):
    """The LDS path at its limit (4 096 documents) and the slab path (4 097: the misaligned block; 6 001), with 300 and 2:
    about 50 chosen documents of each -- the first and last stored, both sides of the cut, the best and worst ranked,
    members of tie groups, a spread of the rest.  Under the continuous model two documents hardly ever share a score, so
    the integer model is there for the rank count's gain / id branch: with it the chosen documents of every query of 300
    documents and more must hold a tie group with different labels (and, under any model, both sides of the cut), or the
    test fails rather than pass without them."""
    X, y, qid = _long_query_set()
    g, c = fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)
    model = fr.CModel.from_dict({"Linear": {"weights": weights}})
    scores = native.predict_scores_dense(model, g)
    lam, wt = native.lambda_gradients(model, g, measure, sigma)
    only = {k for k, ids in enumerate(lm.query_lists(c)) if len(ids) in (2, 300, 4096, 4097, 6001)}
    assert len(only) == 5
    worst = hx.check_dataset(c, scores, y, lam, wt, measure, sigma, c.default_norms(measure), limit=50, only=only,
                             demand_ties_from=300 if weights is _INTEGER else None)
    print("kernel, long queries, %s model, %s, sigma %s: worst error / bound = %.4f" % (
        "integer" if weights is _INTEGER else "continuous", measure, sigma, worst))


def _leaf_values(node, out):
    if "LeafNode" in node:
        out.append(node["LeafNode"])
    else:
        _leaf_values(node["FeatureSplit"]["lhs"], out)
        _leaf_values(node["FeatureSplit"]["rhs"], out)
    return out


@pytest.mark.parametrize("grower", ["exact", "histogram"])
def test_training_through_saturation_stays_finite(grower):
    """Five trees with a learning rate that drives sigma (s_h - s_l) beyond +-745 after the first: every gradient, leaf value
    and running score is finite, and train_measure is the oracle evaluator's mean of the prediction (a Newton step of
    1e15 from a saturated leaf would at least show)."""
    X, y, qid, g, c = _designed_dataset()
    measure, T = "ndcg@10", 5
    req = _request(measure, num_trees=T, max_depth=4, min_leaf_support=1, split_candidates=16, sigma=1.5, learning_rate=2000.0)
    req.params.grower = grower
    model = g.train_model(req)
    st = native.last_train_stats()["lambdamart"]
    trees = [m["DecisionTree"] for m in model.to_dict()["Ensemble"]["models"]]
    norms = c.default_norms(measure)
    queries = lm.query_lists(c)
    saturated = False
    for t in range(T + 1):
        prefix = fr.CModel.from_dict({"Ensemble": {"weights": [2000.0] * t, "models": [{"DecisionTree": x} for x in trees[:t]]}})
        s = native.predict_scores_dense(prefix, g)
        assert np.all(np.isfinite(s)), t
        saturated = saturated or any(1.5 * (s[ids].max() - s[ids].min()) > 745.0 for ids in queries)
        if t > 0:
            assert np.all(np.isfinite(_leaf_values(trees[t - 1], []))), t
            per_q, err = c.metric_from_scores(measure, s, norms)
            assert err == 0 and st["train_measure"][t - 1] == o.mean(per_q), t
        lam, wt = native.lambda_gradients(prefix, g, measure, 1.5)
        assert np.all(np.isfinite(lam)) and np.all(np.isfinite(wt)), t
    assert saturated, "the case must reach saturation, or it tests nothing"


def test_randomised_lambdamart_soak():
    """tools/fuzz_lambdamart.py: random small datasets (1..40 features, constant / signed-zero / denormal / huge columns,
    scattered queries, odd label sets, sampled views, file-loaded sparse rows) and random parameters, both growers; every
    stage of every case must equal the restatement's."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_lambdamart.py"), "--iters", "30", "--seed", "5"],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    last = out.stdout.strip().splitlines()[-1]
    assert out.returncode == 0, out.stdout[-2000:]
    res = json.loads(last)
    assert res["mismatches"] == 0 and res["both_error"] * 10 <= res["iters"]


def _sparse_file(path):
    """A small ranksvm file whose feature values all lie in 4 .. 6 and a third of whose rows list only three of their
    nine features: an absent value reads 0.0, far outside the range of the held ones, so a grower that took a feature's range
    over all the values it reads would place other thresholds.  Returns (X with the unlisted column 0, y, qid)."""
    rng = np.random.default_rng(31)
    n, d = 160, 9
    qid = np.repeat(np.arange(1, 9, dtype=np.int64), 20)
    y = rng.choice(5, n).astype(np.float64)
    X = np.zeros((n, d + 1), dtype=np.float32)
    X[:, 1:] = 4.0 + rng.integers(0, 17, (n, d)) / 8.0
    X[:, 2] += (0.125 * y).astype(np.float32)
    with open(path, "w") as fh:
        for i in range(n):
            if rng.random() < 0.35:  # three of nine, the last among them: under half of 1 .. 9, so the row holds only these
                drop = np.ones(d, dtype=bool)
                drop[rng.choice(d - 1, 2, replace=False)] = False
                drop[d - 1] = False
                X[i, 1:][drop] = 0.0
            fh.write("%d qid:%d %s # doc%d\n" % (int(y[i]), int(qid[i]), " ".join("%d:%r" % (j, float(X[i, j])) for j in range(1, d + 1) if X[i, j] != 0.0), i))
    return X, y, qid


def test_stagewise_identity_file_loaded_with_absent_values(tmp_path):
    """The exact grower on a file-loaded dataset: a feature's range is taken over the values the node's instances HOLD
    (the RF grower's FeatureStats rule, restated in lm.fit_tree's `present`; the mask comes from conftest's reading of the
    file, not from the loader).  Every tree equals the restatement's with the mask, and the mask matters here."""
    path = str(tmp_path / "sparse.train")
    X, y, qid = _sparse_file(path)
    rd = fr.CDataset.open_ranksvm(path)
    c = o.Dataset(X, y, qid)
    present = ranksvm_presence(path, X.shape[1])
    assert not present[:, 1:].all() and present[:, 1:].any(axis=0).all()
    feats = sorted(rd.feature_ids())
    assert feats == list(range(10))  # (0 too: a row that lists most of 1 .. max is held densely from index 0, which reads 0.0)
    T, lr = 6, 0.1
    req = _request("ndcg@10", num_trees=T, max_depth=4, min_leaf_support=3, split_candidates=16, learning_rate=lr)
    trees = [m["DecisionTree"] for m in rd.train_model(req).to_dict()["Ensemble"]["models"]]
    order_ids = np.concatenate(lm.query_lists(c))
    mask_matters = False
    for t in range(T):
        prefix = fr.CModel.from_dict({"Ensemble": {"weights": [lr] * t, "models": [{"DecisionTree": x} for x in trees[:t]]}})
        lam, wt = native.lambda_gradients(prefix, rd, "ndcg@10", 1.0)
        assert trees[t] == lm.fit_tree(X, lam, wt, order_ids, feats, 4, 3, 16, present), "tree %d" % t
        mask_matters = mask_matters or trees[t] != lm.fit_tree(X, lam, wt, order_ids, feats, 4, 3, 16, None)
    assert mask_matters
    exp = c.score_ensemble(trees, [lr] * T)
    assert np.array_equal(native.predict_scores_dense(fr.CModel.from_dict({"Ensemble": {"weights": [lr] * T, "models": [{"DecisionTree": x} for x in trees]}}), rd), exp)
