"""The linear LambdaRank trainer on the device: every iteration restated stage by stage through the
hooks, the returned model, a sampled view, repeatability, and that it learns."""
import json
import os

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import native
from oracle import pyoracle as o
from tests.conftest import GOLDEN, synth_dataset

pytestmark = pytest.mark.gpu


def _request(measure="ndcg@10", **kw):
    req = fr.TrainRequest.linear_lambdarank()
    req.measure = measure
    req.params.quiet = True
    for k, v in kw.items():
        setattr(req.params, k, v)
    return req


def _train(ds, req):
    model = ds.train_model(req)
    return model, native.last_train_stats()["linear_lambdarank"]


def _linear(w):
    return fr.CModel.from_dict({"Linear": {"weights": [float(v) for v in w]}})


@pytest.fixture(scope="module")
def sets():
    d = np.load(os.path.join(GOLDEN, "trec_news_2018.npz"))
    X, y, qid = synth_dataset(11, 3000, 17, 40)
    return {"trec": fr.CDataset.from_numpy(d["train_X"], d["train_y"], d["train_qid"]), "synth": fr.CDataset.from_numpy(X, y, qid)}


@pytest.mark.parametrize("options", [{}, {"objective": "map"}, {"objective": "xendcg"}, {"truncation_level": 5, "lambda_norm": True}],
                         ids=["ndcg", "map", "xendcg", "trunc_norm"])
@pytest.mark.parametrize("which", ["trec", "synth"])
def test_every_iteration_is_its_stages(sets, which, options):
    ds = sets[which]
    measure, lr, l2, sigma = "ndcg@10", 0.5, 0.125, 1.5
    model, st = _train(ds, _request(measure, num_iterations=3, learning_rate=lr, lambda_l2=l2, sigma=sigma, **options))
    role = {"map": "map", "mrr": "mrr"}.get(options.get("objective"), measure)  # the measure that is reported
    W = [np.zeros(len(st["weights"][0]))] + [np.asarray(w) for w in st["weights"]]
    assert st["iterations"] == 3 and len(W) == 4
    for t in range(3):
        lam, wt = native.lambda_gradients(_linear(W[t]), ds, measure, sigma, truncation_level=options.get("truncation_level", 0),
                                          lambda_norm=options.get("lambda_norm", False), objective=options.get("objective", "ndcg"))
        H, g = native.weighted_gram(ds, lam, wt)
        delta = native.newton_step(H, g, l2)
        assert np.array_equal(W[t] + lr * delta, W[t + 1]), t
        _, per_q = native.evaluate_dense(_linear(W[t + 1]), ds, role)
        assert st["train_measure"][t] == o.mean(per_q), t
    assert model.to_dict() == {"Linear": {"weights": st["weights"][st["best_iteration"] - 1]}}


def test_model_and_behaviour(sets):
    ds = sets["synth"]
    req = _request(num_iterations=6, lambda_l2=0.01)
    model, st = _train(ds, req)
    tm = st["train_measure"]
    best = st["best_iteration"]
    assert tm[best - 1] == max(tm) and all(v < tm[best - 1] for v in tm[: best - 1])
    # learning: the returned model beats all-zero weights on the data it was trained on
    _, zero_q = native.evaluate_dense(_linear(np.zeros(17)), ds, "ndcg@10")
    assert st["zero_measure"] == o.mean(zero_q) and tm[best - 1] > st["zero_measure"]
    # the model is an ordinary Linear one: the JSON round trip, evaluate, permutation_importance
    again = fr.CModel.from_dict(json.loads(json.dumps(model.to_dict())))
    _, per_q = native.evaluate_dense(again, ds, "ndcg@10")
    assert o.mean(per_q) == tm[best - 1] and len(ds.evaluate(model, "ndcg@10")) == len(ds.queries())
    imp = fr.permutation_importance(ds, model, "ndcg@10", repeats=2, seed=1)
    assert imp["baseline"] == tm[best - 1] and len(imp["ranking"]) == 17
    assert all(st[key] >= 0.0 for key in ("score_ms", "gradient_ms", "gram_ms", "solve_ms", "measure_ms"))
    # the same request twice: the same bytes
    model2, st2 = _train(ds, req)
    assert model2.to_dict() == model.to_dict() and st2["weights"] == st["weights"] and st2["train_measure"] == tm
    # a sampled view trains on its own queries only: its first iteration restated over the view's documents alone (the hooks
    # hand back NaN for every other document, and the Gram hook never reads those)
    view = ds.subsample_queries(sorted(ds.queries())[::3])
    mv, sv = _train(view, req)
    lam, wt = native.lambda_gradients(_linear(np.zeros(17)), view, "ndcg@10", 1.0)
    assert np.isnan(lam).any()
    H, g = native.weighted_gram(view, lam, wt)
    assert np.array_equal(1.0 * native.newton_step(H, g, 0.01), np.asarray(sv["weights"][0]))
    assert sv["weights"][0] != st["weights"][0]
