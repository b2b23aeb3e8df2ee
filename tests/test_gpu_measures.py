"""DCG, precision, recall, success and ERR on the device against the numpy restatement
(tests/measures_model.py), bit for bit, through both metric kernels: metric_sort_kernel and the selection kernel
metric_topk_kernel (FR_METRIC_KERNEL forces one; native.last_metric_plan says which ran).

The dataset: 20 queries of 1 .. 200 documents and one of 8193 (beyond the LDS sort), rows interleaved, D = 4 columns of small
integers (scores tie all the time; the tie-break decides), labels 0 .. 4, one query without a relevant document, both signs of
zero among the scores, and an all-zero model under which every score ties."""
import functools
import json
import math

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import native
from tests import measures_model as mm
from tests import permute_model as pm
from tests import resample_model as rm

pytestmark = pytest.mark.gpu

QLENS = [1, 2, 3, 63, 64, 65, 127, 128, 129, 200, 8193, 1, 64, 65, 3, 128, 200, 2, 129, 63]  # query ids 1 .. 20
NO_RELEVANT = 4   # the query id (63 documents) whose labels are all 0
TOP_GAIN_QUERY = 10  # the only query that holds a label 4 (200 documents): a view without it must still divide by 2^4
KS = (1, 2, 10, 63, 64, 65, 300)
EVALUATORS = ["%s@%d" % (n, k) for n in mm.NAMES for k in KS] + ["dcg", "recall", "err"]
MODELS = {
    "linear": {"Linear": {"weights": [-0.7, -1.0 / 3.0, 0.0, 0.45]}},
    "single": {"SingleFeature": {"fid": 0, "dir": -1.5}},  # -1.5 * +0.0 = -0.0 and -1.5 * -0.0 = +0.0
    "zero": {"Linear": {"weights": [0.0, 0.0, 0.0, 0.0]}},
}


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _same(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


@functools.lru_cache(maxsize=None)
def _data():
    rng = np.random.default_rng(17)
    n = sum(QLENS)
    qid = np.repeat(np.arange(1, len(QLENS) + 1, dtype=np.int64), QLENS)[rng.permutation(n)]
    y = rng.integers(0, 4, size=n).astype(np.float64)
    y[qid == NO_RELEVANT] = 0.0
    y[np.flatnonzero(qid == TOP_GAIN_QUERY)[::9]] = 4.0
    X = rng.integers(-3, 4, size=(n, 4)).astype(np.float32)
    zeros = np.flatnonzero(X[:, 0] == 0)
    X[zeros[::2], 0] = -0.0
    return X, y, qid


@functools.lru_cache(maxsize=None)
def _dataset():
    return fr.CDataset.from_numpy(*_data())


@functools.lru_cache(maxsize=None)
def _model(name):
    return fr.CModel.from_dict(MODELS[name])


@functools.lru_cache(maxsize=None)
def _ranked(name):
    """the restatement's ranked lists under a model, from the library's scores (held to the oracle elsewhere)"""
    X, y, qid = _data()
    scores = native.predict_scores_dense(_model(name), _dataset())
    return mm.ranked_lists(scores, y, qid)


JUDGED = {
    "3": {"doc%d" % k: 1.0 for k in range(9)},                 # 9 relevant judged, the dataset holds 3 documents
    "7": {"doc%d" % k: float(k % 3) for k in range(200)},       # more relevant documents than the dataset's
    "9": {"a": 6.0, "b": 0.0},                                  # a gain above the dataset's 4: den = 2^6
    "12": {"a": 0.0, "b": -1.0},                                # judged, nothing relevant: the list's own count
    "99": {"a": 5.0},                                           # a query the dataset lacks
}


def _expected(evaluator, model, judged=None, queries=None):
    ranked = _ranked(model)
    if queries is not None:
        ranked = {q: ranked[q] for q in queries}
    return mm.per_query(evaluator, ranked, _data()[1], judged)


def _plan_kernels():
    return {c["kernel"] for c in native.last_metric_plan()["classes"]}


def _check_all(monkeypatch, model, dataset, judged=None, queries=None):
    qrel = fr.CQRel.from_dict(judged) if judged is not None else None
    for kernel in ("topk", "sort"):
        monkeypatch.setenv("FR_METRIC_KERNEL", kernel)
        for evaluator in EVALUATORS:
            names, got = native.evaluate_dense(_model(model), dataset, evaluator, qrel)
            want = _expected(evaluator, model, judged, queries)
            want = np.array([want[int(q)] for q in names])
            bad = np.flatnonzero(_bits(got) != _bits(want))
            print(model, kernel, evaluator, "queries that differ:", [(names[i], got[i], want[i]) for i in bad[:4]])
            assert len(bad) == 0 and len(names) == len(queries if queries is not None else QLENS)
            _, depth = mm.parse(evaluator)
            selects = kernel == "topk" and depth is not None and 1 <= depth <= 64
            plan = native.last_metric_plan()
            assert _plan_kernels() == {"topk" if selects else "sort"}, (evaluator, plan)
            assert plan["measure"] == mm.parse(evaluator)[0] and plan["depth"] == depth and plan["slots"] == 1
            assert sum(c["queries"] for c in plan["classes"]) == len(names)


# ---- 1: per-query values, both kernels ---------------------------------------------------------------------------------


@pytest.mark.parametrize("model", list(MODELS))
def test_every_measure_and_depth_equals_the_restatement_under_both_kernels(monkeypatch, model):
    if model == "single":
        zero = native.predict_scores_dense(_model(model), _dataset())
        zero = zero[zero == 0.0]
        assert np.signbit(zero).any() and not np.signbit(zero).all()  # both signs of zero tie
    _check_all(monkeypatch, model, _dataset())


def test_with_judgments_that_move_recalls_norm_and_errs_denominator(monkeypatch):
    _check_all(monkeypatch, "linear", _dataset(), judged=JUDGED)
    # they did move them
    plain, judged = _expected("recall@10", "linear"), _expected("recall@10", "linear", JUDGED)
    assert plain[7] != judged[7] and plain[12] == judged[12] and plain[5] == judged[5]
    e_plain, e_judged = _expected("err@10", "linear"), _expected("err@10", "linear", JUDGED)
    assert e_plain[1] == 4.0 * e_judged[1] and e_plain != e_judged  # den 16 -> 64; query 1 is one document


def test_a_query_sampled_view_gives_its_parents_values(monkeypatch):
    chosen = [1, 3, 4, 6, 9, 11, 14, 20]  # lengths 1, 3, 63 (nothing relevant), 65, 129, 8193, 65, 63: not the query of the top gain
    view = _dataset().subsample_queries([str(q) for q in chosen])
    _check_all(monkeypatch, "linear", view, queries=chosen)
    _check_all(monkeypatch, "single", view, judged=JUDGED, queries=chosen)


def test_without_a_forced_kernel_the_rule_routes_each_class(monkeypatch):
    monkeypatch.delenv("FR_METRIC_KERNEL", raising=False)
    for evaluator in ("dcg@1", "err@10", "recall@64", "precision@20"):
        names, got = native.evaluate_dense(_model("linear"), _dataset(), evaluator)
        want = _expected(evaluator, "linear")
        assert _same(got, [want[int(q)] for q in names])
        depth = mm.parse(evaluator)[1]
        for c in native.last_metric_plan()["classes"]:
            assert c["kernel"] == ("topk" if native.metric_topk_pays(depth, c["npad"]) else "sort"), (evaluator, c)
    assert {c["npad"]: c["kernel"] for c in native.last_metric_plan()["classes"]}[16384] == "topk"  # the 8193 documents: no scratch slab


# ---- 2: ties to the measures that were there ---------------------------------------------------------------------------------


@pytest.mark.parametrize("kernel", ["topk", "sort"])
def test_ties_to_ndcg_and_mrr(monkeypatch, kernel):
    monkeypatch.setenv("FR_METRIC_KERNEL", kernel)
    X, y, qid = _data()
    m, ds = _model("linear"), _dataset()
    names, mrr = native.evaluate_dense(m, ds, "mrr")
    for k in KS:
        _, ndcg = native.evaluate_dense(m, ds, "ndcg@%d" % k)
        _, dcg = native.evaluate_dense(m, ds, "dcg@%d" % k)
        _, success = native.evaluate_dense(m, ds, "success@%d" % k)
        for i, q in enumerate(names):
            gains = np.sort(y[qid == int(q)].astype(np.float32))[::-1]
            ideal = mm.dcg(gains, k)
            assert _same(ndcg[i], dcg[i] / ideal if (gains > 0).any() else 0.0), (k, q)
            assert success[i] == (1.0 if mrr[i] >= 1.0 / k else 0.0), (k, q)
    _, recall = native.evaluate_dense(m, ds, "recall")
    assert set(recall) == {0.0, 1.0} and [float(v) for q, v in zip(names, recall) if int(q) == NO_RELEVANT] == [0.0]


# ---- 3: several slots at once ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kernel", ["topk", "sort"])
def test_line_search_candidates_equal_single_slot_calls(monkeypatch, kernel):
    monkeypatch.setenv("FR_METRIC_KERNEL", kernel)
    ds = _dataset()
    base = np.array([[-0.7, -1.0 / 3.0, 0.0, 0.45], [0.25, 0.0, -0.5, 0.125]])
    feats, cands = [1, 3], [[-1.0, 0.0, 0.5, 2.0 / 3.0], [0.125, -0.25, 0.0]]
    for evaluator in ("err@10", "recall@2", "dcg@64", "precision@65"):
        means, pq = native.evaluate_candidates(ds, evaluator, feats, base, cands, per_query=True)
        assert native.last_metric_plan()["slots"] >= 7
        assert _plan_kernels() == {"topk" if kernel == "topk" and mm.parse(evaluator)[1] <= 64 else "sort"}
        for g in range(2):
            for ci, cand in enumerate(cands[g]):
                w = base[g].copy()
                w[feats[g]] = cand
                _, one = native.evaluate_dense(fr.CModel.from_dict({"Linear": {"weights": w.tolist()}}), ds, evaluator)
                assert _same(pq[:, g * 64 + ci], one), (evaluator, g, ci)
                assert _same(means[g][ci], rm.means(one[:, None])[0])


@pytest.mark.parametrize("kernel, evaluator", [("topk", "recall@10"), ("sort", "err@10"), ("topk", "err@3")])
def test_permutation_importance_equals_the_exact_path_on_permuted_matrices(monkeypatch, kernel, evaluator):
    monkeypatch.setenv("FR_METRIC_KERNEL", kernel)
    X, y, qid = _data()
    ids = np.arange(len(y))
    model, feats, R, seed = _model("linear"), [0, 3, 1], 2, 5
    rep, values, pq = native.permutation_importance_dense(model, _dataset(), evaluator, repeats=R, seed=seed, features=feats)
    assert _plan_kernels() == {kernel}
    names, base = native.evaluate_dense(model, _dataset(), evaluator)
    assert _same(pq[-1], base) and pq.shape == (len(feats) * R + 1, len(names))
    moved = 0
    for fi, f in enumerate(feats):
        for r in range(R):
            src = pm.sources(ids, seed, r, "dataset", qid[ids])
            other = fr.CDataset.from_numpy(np.ascontiguousarray(pm.permuted_matrix(X, ids, src, f)), y, qid)
            other_names, want = native.evaluate_dense(model, other, evaluator)
            want = dict(zip(other_names, want))
            want = np.array([want[q] for q in names])
            assert _same(pq[fi * R + r], want), (f, r)
            assert _same(values[fi, r], rm.means(want[:, None])[0])
            moved += int((_bits(want) != _bits(base)).sum())
    assert moved > 0


# ---- 4: training -------------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _binary(one_relevant):
    rng = np.random.default_rng(23 + one_relevant)
    lens = rng.integers(2, 40, size=24)
    n = int(lens.sum())
    qid = np.repeat(np.arange(1, 25, dtype=np.int64), lens)
    y = np.zeros(n) if one_relevant else (rng.random(n) < 0.3).astype(np.float64)
    for q in range(1, 25):  # at least one relevant document in every query (exactly one, if asked for)
        rows = np.flatnonzero(qid == q)
        if one_relevant or y[rows].sum() == 0:
            y[rng.choice(rows)] = 1.0
    X = (rng.integers(-3, 4, size=(n, 4)) + 0.5 * y[:, None] * (rng.random((n, 4)) < 0.5)).astype(np.float32)
    return X, y, qid


def _ca(measure):
    req = fr.TrainRequest.coordinate_ascent()
    req.measure = measure
    req.params.num_restarts, req.params.num_max_iterations, req.params.quiet, req.params.seed = 2, 3, True, 42
    return req


def test_coordinate_ascent_on_binary_labels_is_the_ndcg_at_1_run(monkeypatch):
    monkeypatch.delenv("FR_METRIC_KERNEL", raising=False)
    ds = fr.CDataset.from_numpy(*_binary(0))
    models, paths = {}, {}
    for measure in ("ndcg@1", "dcg@1", "precision@1", "success@1"):
        models[measure] = json.dumps(ds.train_model(_ca(measure)).to_dict(), sort_keys=True)
        paths[measure] = native.last_train_stats()["path"]
    assert paths == {"ndcg@1": "fused_linesearch", "dcg@1": "generic_sort", "precision@1": "generic_sort", "success@1": "generic_sort"}
    assert len(set(models.values())) == 1, models
    assert any(w != 0.0 for w in json.loads(models["ndcg@1"])["Linear"]["weights"])
    one = fr.CDataset.from_numpy(*_binary(1))
    assert json.dumps(one.train_model(_ca("recall@1")).to_dict(), sort_keys=True) == json.dumps(one.train_model(_ca("ndcg@1")).to_dict(), sort_keys=True)
    # the random forest's trees do not look at the measure; its report goes through the general evaluator
    forests = []
    for measure in ("ndcg@1", "precision@1"):
        rf = fr.TrainRequest.random_forest()
        rf.measure = measure
        rf.params.quiet, rf.params.num_trees, rf.params.seed = True, 2, 7
        forests.append(json.dumps(ds.train_model(rf).to_dict(), sort_keys=True))
    assert forests[0] == forests[1]


@pytest.mark.parametrize("kernel", ["topk", "sort"])
def test_a_stepped_run_under_err_reports_the_mean_of_evaluate(monkeypatch, kernel):
    monkeypatch.setenv("FR_METRIC_KERNEL", kernel)
    X, y, qid = _data()
    keep = qid != 11  # (without the 8193 documents: a training tick evaluates every candidate of every restart)
    ds = fr.CDataset.from_numpy(np.ascontiguousarray(X[keep]), y[keep], qid[keep])
    run = native.CoordinateAscentRun(ds, _ca("err@10"))
    run.step(4)
    assert _plan_kernels() == {kernel}
    state = run.state()
    run.close()
    assert len(state["restarts"]) == 2
    for r in state["restarts"]:
        _, vals = native.evaluate_dense(fr.CModel.from_dict({"Linear": {"weights": list(r["weights"])}}), ds, "err@10")
        assert _same(r["score"], rm.means(vals[:, None])[0])
    model = ds.train_model(_ca("err@10"))
    assert native.last_train_stats()["path"] == "generic_sort"
    mean = rm.means(native.evaluate_dense(model, ds, "err@10")[1][:, None])[0]
    assert 0.0 < mean < 1.0 and math.isclose(sum(ds.evaluate(model, "err@10").values()) / 19, mean, rel_tol=1e-12)


# ---- 5: refusals that need the device, and the old measures' plan -------------------------------------------------------------


def test_a_nan_score_is_refused_by_both_kernels_and_the_old_measures_sort(monkeypatch):
    ds = _dataset()
    nan = fr.CModel.from_dict({"Linear": {"weights": [1e308, -1e308, 0.0, 0.0]}})  # (no NaN weight in the model format: +inf - inf)
    for kernel in ("topk", "sort"):
        monkeypatch.setenv("FR_METRIC_KERNEL", kernel)
        for evaluator in ("dcg@10", "recall@64", "err@1"):
            with pytest.raises(Exception, match="Model.predict -> NaN"):
                native.evaluate_dense(nan, ds, evaluator)
            assert _plan_kernels() == {kernel}
        for evaluator in ("ndcg@10", "map", "mrr", "ndcg"):
            native.evaluate_dense(_model("linear"), ds, evaluator)
            assert _plan_kernels() == {"sort"}, evaluator
    monkeypatch.delenv("FR_METRIC_KERNEL")
    for evaluator in ("ndcg@10", "map", "mrr"):
        native.evaluate_dense(_model("linear"), ds, evaluator)
        assert _plan_kernels() == {"sort"} and native.last_metric_plan()["measure"] == evaluator.split("@")[0]


# ---- 6: compare_models and bootstrap_eval on the bundled example ----------------------------------------------------------------


def test_compare_models_and_bootstrap_eval_under_precision_at_10(trec):
    X, y, qid = trec["train_X"], trec["train_y"], trec["train_qid"]
    ds = fr.CDataset.from_numpy(X, y, qid)
    models = {}
    for name, f in (("pagerank", 4), ("para-fraction", 5)):
        w = [0.0] * 6
        w[f] = 1.0
        models[name] = fr.CModel.from_dict({"Linear": {"weights": w}})
    names, _ = native.evaluate_dense(models["pagerank"], ds, "precision@10")
    cols = []
    for m in models.values():
        want = mm.per_query("precision@10", mm.ranked_lists(native.predict_scores_dense(m, ds), y, qid), y)
        cols.append([want[int(q)] for q in names])
    V = np.array(cols).T
    assert 0.0 < V.mean() < 1.0
    got = fr.compare_models(ds, models, "Precision@10", trials=300, seed=3)
    rep, _, _ = native.resample(V, 300, 3)
    want = fr.compare.named_report(rep, list(models))
    for key in ("systems", "means", "intervals", "summary", "pairs", "trials", "seed", "alpha"):
        assert got[key] == want[key], key
    boot = ds.bootstrap_eval(models["para-fraction"], "prec@10", trials=200)
    rep1, _, _ = native.resample(V[:, 1:2], 200, 0, perm=False)
    assert boot == {"mean": rep1["means"][0], "summary": rep1["summary"][0], "interval": rep1["intervals"][0]}
