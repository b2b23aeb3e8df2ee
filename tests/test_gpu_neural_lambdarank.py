"""The neural LambdaRank trainer and the NeuralNet model on the device: every iteration restated through
the hooks, the returned model, the model's other callers, repeatability, and that it learns what no linear model can."""
import json
import os

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import native
from oracle import pyoracle as o
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu


def _request(kind="neural_lambdarank", measure="ndcg@10", **kw):
    req = getattr(fr.TrainRequest, kind)()
    req.measure = measure
    req.params.quiet = True
    for k, v in kw.items():
        setattr(req.params, k, v)
    return req


def _train(ds, req):
    return ds.train_model(req), native.last_train_stats()[{"NeuralLambdaRank": "neural_lambdarank"}.get(req.params.VARIANT, "linear_lambdarank")]


def _flat(net):
    n = net["NeuralNet"]
    return np.concatenate([np.asarray(n["hidden_weights"]).ravel(), n["hidden_bias"], n["output_weights"], [n["output_bias"]]])


@pytest.fixture(scope="module")
def sets():
    d = np.load(os.path.join(GOLDEN, "trec_news_2018.npz"))
    raw = fr.CDataset.from_numpy(d["train_X"], d["train_y"], d["train_qid"])
    # labels that are a sum of ReLUs of two features, |x0| + |x1|: symmetric in both, so no linear model orders them
    rng = np.random.default_rng(4)
    X = rng.normal(0.0, 1.0, (1500, 8)).astype(np.float32)
    y = np.floor(np.minimum(3.0, np.abs(X[:, 0]) + np.abs(X[:, 1]))).astype(np.float64)
    qid = np.repeat(np.arange(1, 31, dtype=np.int64), 50)
    return {"trec": fr.Normalizer.fit(raw, "zscore").apply(raw), "synth": fr.CDataset.from_numpy(X, y, qid)}


@pytest.mark.parametrize("options", [{}, {"objective": "map"}, {"objective": "xendcg"}, {"truncation_level": 5, "lambda_norm": True}],
                         ids=["ndcg", "map", "xendcg", "trunc_norm"])
@pytest.mark.parametrize("which", ["trec", "synth"])
def test_every_iteration_is_its_stages(sets, which, options):
    ds = sets[which]
    measure, h, lr, l2, sigma, T = "ndcg@10", 5, 0.05, 0.125, 1.5, 3
    model, st = _train(ds, _request(measure=measure, hidden=h, num_iterations=T, learning_rate=lr, lambda_l2=l2, sigma=sigma, seed=3, trace=True, **options))
    role = {"map": "map", "mrr": "mrr"}.get(options.get("objective"), measure)  # the measure that is reported
    nets = [st["initial"]] + st["iterates"]
    assert st["iterations"] == T and len(nets) == T + 1
    d = len(nets[0]["NeuralNet"]["hidden_weights"][0])
    decays = np.concatenate([np.ones(h * d), np.zeros(h), np.ones(h), [0]])
    theta, m, v = _flat(nets[0]), np.zeros(h * d + 2 * h + 1), np.zeros(h * d + 2 * h + 1)
    for t in range(T):
        net = fr.CModel.from_dict(nets[t])
        lam, _ = native.lambda_gradients(net, ds, measure, sigma, truncation_level=options.get("truncation_level", 0),
                                         lambda_norm=options.get("lambda_norm", False), objective=options.get("objective", "ndcg"))
        g = native.mlp_gradients(ds, net, lam)
        grad = np.concatenate([g["hidden_weights"].ravel(), g["hidden_bias"], g["output_weights"], [g["output_bias"]]])
        theta, m, v = native.adam_step(theta, grad, m, v, t + 1, lr, l2, decays)
        assert np.array_equal(theta, _flat(nets[t + 1])), t
        _, per_q = native.evaluate_dense(fr.CModel.from_dict(nets[t + 1]), ds, role)
        assert st["train_measure"][t] == o.mean(per_q), t
    tm, best = st["train_measure"], st["best_iteration"]
    beats = [t for t in range(T) if tm[t] > st["initial_measure"]]
    assert best == (1 + tm.index(max(tm[t] for t in beats)) if beats else 1)
    assert model.to_dict() == nets[best]


def test_the_model_with_its_other_callers(sets):
    ds = sets["synth"]
    req = _request(hidden=8, num_iterations=4, learning_rate=0.05, seed=1)
    model, st = _train(ds, req)
    assert "iterates" not in st and st["score_plan"]["resident"] and st["backprop_plan"]["workgroups"] == st["backprop_plan"]["tiles"]
    assert all(st[key] >= 0.0 for key in ("score_ms", "gradient_ms", "backprop_ms", "adam_ms", "measure_ms"))
    scores = native.predict_scores_dense(model, ds)
    again = fr.CModel.from_dict(json.loads(json.dumps(model.to_dict())))
    assert np.array_equal(native.predict_scores_dense(again, ds), scores) and not np.isnan(scores).any()
    assert len(ds.evaluate(model, "ndcg@10")) == len(ds.queries())
    # an Ensemble with a Linear member: s = (0 + w_a s_net) + w_b s_lin, products and sums rounded separately
    lin = fr.CModel.from_dict({"Linear": {"weights": [0.25, -1.0, 0.5, 0.0, 0.0, 2.0, 0.0, -0.125]}})
    ens = fr.CModel.from_dict({"Ensemble": {"weights": [0.3, -1.7], "models": [model.to_dict(), lin.to_dict()]}})
    assert np.array_equal(native.predict_scores_dense(ens, ds), (0.0 + 0.3 * scores) + -1.7 * native.predict_scores_dense(lin, ds))
    rep = fr.compare_models(ds, {"net": model, "lin": lin}, "ndcg@10", trials=200, seed=2)
    assert rep["systems"] == ["net", "lin"] and rep["queries"] == len(ds.queries())
    with pytest.raises(Exception, match="permutation importance does not take a NeuralNet model"):
        fr.permutation_importance(ds, model, "ndcg@10", repeats=2, seed=1)
    with pytest.raises(Exception, match="explain: a NeuralNet model has no trees to explain"):
        model.explain(ds)
    # the same request twice: the same bytes; another seed: other ones
    model2, st2 = _train(ds, req)
    assert model2.to_dict() == model.to_dict() and st2["train_measure"] == st["train_measure"]
    other, _ = _train(ds, _request(hidden=8, num_iterations=4, learning_rate=0.05, seed=2))
    assert other.to_dict() != model.to_dict()


def test_a_non_finite_feature_value_is_refused_before_the_first_iteration():
    X = np.arange(40, dtype=np.float32).reshape(10, 4)
    X[7, 2] = np.inf
    ds = fr.CDataset.from_numpy(X, np.arange(10) % 3.0, np.repeat(np.arange(1, 3, dtype=np.int64), 5))
    with pytest.raises(Exception, match="NeuralLambdaRank: feature 2 holds an inf or NaN value"):
        ds.train_model(_request(hidden=2, num_iterations=1))


def test_the_net_learns_what_no_linear_model_orders(sets):
    ds = sets["synth"]
    _, lin = _train(ds, _request("linear_lambdarank", measure="ndcg", num_iterations=10))
    _, net = _train(ds, _request(measure="ndcg", hidden=16, num_iterations=60, learning_rate=0.05, seed=0))
    assert net["train_measure"][-1] > max(lin["train_measure"])
