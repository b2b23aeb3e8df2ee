"""The neural LambdaRank trainer under objective "approxndcg" ("ApproxNDCG objective"; section 19):
every iterate is the hook's gradient, back-propagation and the Adam step; the training measure stays the request's NDCG; and
the ascent raises the objective it states."""
import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import native
from oracle import pyoracle as o
from tests import lambdamart_approx_model as am
from tests import lambdamart_model as lm
from tests.lambdamart_xendcg_model import gains

pytestmark = pytest.mark.gpu

PARTS = ("hidden_weights", "hidden_bias", "hidden2_weights", "hidden2_bias", "output_weights")


@pytest.fixture(scope="module")
def synth():
    """30 queries of 50 documents; labels that are a sum of ReLUs of two features, |x0| + |x1|."""
    rng = np.random.default_rng(4)
    X = rng.normal(0.0, 1.0, (1500, 8)).astype(np.float32)
    y = np.floor(np.minimum(3.0, np.abs(X[:, 0]) + np.abs(X[:, 1]))).astype(np.float64)
    qid = np.repeat(np.arange(1, 31, dtype=np.int64), 50)
    return fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid), y


def _train(ds, measure, **kw):
    req = fr.TrainRequest.neural_lambdarank()
    req.measure, req.params.quiet, req.params.objective = measure, True, "approxndcg"
    for k, v in kw.items():
        setattr(req.params, k, v)
    return ds.train_model(req), native.last_train_stats()["neural_lambdarank"]


def _flat(net):
    n = net["NeuralNet"]
    return np.concatenate([np.asarray(n[k], dtype=np.float64).ravel() for k in PARTS if k in n] + [[n["output_bias"]]])


@pytest.mark.parametrize("h2", [None, 3], ids=["one_layer", "hidden2"])
def test_every_iteration_is_its_stages(synth, h2):
    ds = synth[0]
    measure, h, lr, l2, sigma, T = "ndcg@10", 5, 0.05, 0.125, 1.5, 3
    model, st = _train(ds, measure, hidden=h, hidden2=h2, num_iterations=T, learning_rate=lr, lambda_l2=l2, sigma=sigma, seed=3, trace=True)
    assert st["request"]["objective"] == "approxndcg"
    nets = [st["initial"]] + st["iterates"]
    assert st["iterations"] == T and len(nets) == T + 1
    d = len(nets[0]["NeuralNet"]["hidden_weights"][0])
    decays = np.concatenate([np.ones(h * d), np.zeros(h)] + ([np.ones(h2 * h), np.zeros(h2), np.ones(h2)] if h2 else [np.ones(h)]) + [[0]])
    theta, m, v = _flat(nets[0]), np.zeros(len(decays)), np.zeros(len(decays))
    for t in range(T):
        net = fr.CModel.from_dict(nets[t])
        lam, wt = native.lambda_gradients(net, ds, measure, sigma, objective="approxndcg")
        assert lam.any() and not wt.any()
        g = native.mlp2_gradients(ds, net, lam) if h2 else native.mlp_gradients(ds, net, lam)
        theta, m, v = native.adam_step(theta, _flat({"NeuralNet": g}), m, v, t + 1, lr, l2, decays)
        assert np.array_equal(theta, _flat(nets[t + 1])), t
        _, per_q = native.evaluate_dense(fr.CModel.from_dict(nets[t + 1]), ds, measure)
        assert st["train_measure"][t] == o.mean(per_q), t
    tm, best = st["train_measure"], st["best_iteration"]
    beats = [t for t in range(T) if tm[t] > st["initial_measure"]]
    assert best == (1 + tm.index(max(tm[t] for t in beats)) if beats else 1) and model.to_dict() == nets[best]


def test_thirty_iterations_raise_the_objective(synth):
    ds, c, y = synth
    queries, norms, G = lm.query_lists(c), c.default_norms("ndcg"), gains(y)
    _, st = _train(ds, "ndcg", hidden=8, num_iterations=30, learning_rate=0.03, sigma=1.0, seed=1, trace=True)
    A = [am.gradients(native.predict_scores_dense(fr.CModel.from_dict(net), ds), G, queries, norms, 1.0)[1] for net in (st["initial"], st["iterates"][-1])]
    print("mean ApproxNDCG: %.6f initially, %.6f after 30 iterations" % (A[0], A[1]))
    assert A[1] > A[0]
