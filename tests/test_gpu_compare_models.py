"""compare_models and CDataset.bootstrap_eval on the reference's bundled example (782 rows, 45 queries,
6 features): the report equals the numpy restatement (tests/resample_model.py) run on the per-query values
native.evaluate_dense returns."""
import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import native
from tests import resample_model as rm

pytestmark = pytest.mark.gpu

MEASURE = "ndcg@5"


def _linear(f, d=6):
    """the single-feature linear model of feature f"""
    w = [0.0] * d
    w[f] = 1.0
    return fr.CModel.from_dict({"Linear": {"weights": w}})


@pytest.fixture(scope="module")
def example(trec):
    ds = fr.CDataset.from_numpy(trec["train_X"], trec["train_y"], trec["train_qid"])
    models = {"pagerank": _linear(4), "para-fraction": _linear(5), "caption_count": _linear(1)}
    return ds, models


def _table(ds, models):
    cols, names = [], None
    for m in models.values():
        got_names, vals = native.evaluate_dense(m, ds, MEASURE)
        assert names is None or names == got_names
        names = got_names
        cols.append(vals)
    return np.stack(cols, axis=1)


def _want(V, names, trials, seed, alpha=0.05):
    M = V.shape[1]
    rep = rm.report(V, alpha, rm.boot(V, trials, seed), rm.perm(V, trials, seed) if M > 1 else None)
    rep.update(trials=trials, seed=seed, alpha=alpha, boot_path="", boot_ms=0, perm_ms=0, upload_ms=0, download_ms=0, device_call_ms=0, report_ms=0)
    return fr.compare.named_report(rep, list(names))


def _same(got, want):
    for key in ("systems", "means", "intervals", "summary", "pairs", "trials", "seed", "alpha"):
        assert got[key] == want[key], key


def test_two_models_equal_the_restatement_on_the_evaluated_values(example, known):
    ds, models = example
    two = {k: models[k] for k in ("pagerank", "para-fraction")}
    V = _table(ds, two)
    assert V.shape == (len(known["expected_queries"]), 2)
    got = fr.compare_models(ds, two, MEASURE, trials=1000, seed=3)
    _same(got, _want(V, two, 1000, 3))
    assert got["queries"] == len(known["expected_queries"]) and got["stats"]["boot_path"] in ("lds", "global")
    [pair] = got["pairs"]
    assert (pair["a"], pair["b"]) == ("pagerank", "para-fraction")
    assert pair["wins"] + pair["losses"] + pair["ties"] == V.shape[0]
    assert pair["diff"] == got["means"]["pagerank"] - got["means"]["para-fraction"]
    assert pair["diff_interval"][0] <= pair["diff"] <= pair["diff_interval"][1]
    # the means are CDataset.evaluate's values in the fixed-shape sum, and the reference's pinned ones for these models
    assert got["means"]["pagerank"] == float(rm.means(V)[0])
    for name in two:
        assert got["means"][name] == pytest.approx(known["single_feature_ndcg5"][name], abs=5e-8)
    # the same call again gives the same report
    _same(fr.compare_models(ds, two, MEASURE, trials=1000, seed=3), got)


def test_a_model_against_itself(example):
    ds, models = example
    got = fr.compare_models(ds, {"a": models["pagerank"], "b": models["pagerank"]}, MEASURE, trials=200, seed=1)
    [pair] = got["pairs"]
    assert pair["diff"] == 0.0 and pair["p"] == 1.0 and pair["diff_interval"] == [0.0, 0.0]
    assert (pair["wins"], pair["losses"], pair["ties"]) == (0, 0, got["queries"])


def test_a_query_view_gives_the_report_of_its_rows(example):
    ds, models = example
    two = {k: models[k] for k in ("pagerank", "para-fraction")}
    names, _ = native.evaluate_dense(models["pagerank"], ds, MEASURE)
    view = ds.subsample_queries(names[3:25:2])
    V = _table(view, two)
    assert V.shape == (11, 2)
    got = fr.compare_models(view, two, MEASURE, trials=130, seed=9, alpha=0.1)
    _same(got, _want(V, two, 130, 9, 0.1))
    assert got["queries"] == 11


def test_bootstrap_eval_is_the_restatements_percentiles(example):
    ds, models = example
    V = _table(ds, {"m": models["para-fraction"]})
    got = ds.bootstrap_eval(models["para-fraction"], MEASURE, trials=200)
    b = np.sort(rm.boot(V, 200, 0)[:, 0])
    assert got["mean"] == float(rm.means(V)[0])
    assert set(got["summary"]) == {"p5", "p25", "p50", "p75", "p95"}
    for name, at in (("p5", 0.05), ("p25", 0.25), ("p50", 0.5), ("p75", 0.75), ("p95", 0.95)):
        assert float.hex(got["summary"][name]) == float.hex(rm.percentile(b, at)), name
    assert got["interval"] == rm.interval(b, 0.05)
    assert got["summary"]["p5"] <= got["summary"]["p50"] <= got["summary"]["p95"]


def test_three_models_give_three_pairs_from_one_set_of_trials(example):
    ds, models = example
    V = _table(ds, models)
    got = fr.compare_models(ds, models, MEASURE, trials=500, seed=2)
    _same(got, _want(V, models, 500, 2))
    assert [(p["a"], p["b"]) for p in got["pairs"]] == [("pagerank", "para-fraction"), ("pagerank", "caption_count"), ("para-fraction", "caption_count")]
    # one set of trials: the first two models' bootstrap intervals are those of the two-model call (the draws are shared by
    # every column), while their p-value may only grow under the range statistic of three
    two = fr.compare_models(ds, {k: models[k] for k in ("pagerank", "para-fraction")}, MEASURE, trials=500, seed=2)
    assert two["intervals"]["pagerank"] == got["intervals"]["pagerank"] and two["pairs"][0]["diff_interval"] == got["pairs"][0]["diff_interval"]


def test_refusals(example):
    ds, models = example
    with pytest.raises(Exception, match="between 1 and 8 systems, not 0"):
        fr.compare_models(ds, {}, MEASURE)
    with pytest.raises(Exception, match="between 1 and 8 systems, not 9"):
        fr.compare_models(ds, {str(i): models["pagerank"] for i in range(9)}, MEASURE)
    with pytest.raises(Exception, match="trials must be between 1 and 1048576, not 0"):
        fr.compare_models(ds, models, MEASURE, trials=0)
    with pytest.raises(Exception):
        fr.compare_models(ds, models, "no-such-measure")
