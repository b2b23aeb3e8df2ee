"""The neural LambdaRank trainer with `hidden2` ("Two hidden layers"): every iteration restated through the
hooks, the initialiser, the returned model, repeatability, and that the second layer fits what one layer fits badly."""
import json
import os

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import native
from oracle import pyoracle as o
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

PARTS = ("hidden_weights", "hidden_bias", "hidden2_weights", "hidden2_bias", "output_weights")


def _train(ds, measure="ndcg@10", **kw):
    req = fr.TrainRequest.neural_lambdarank()
    req.measure, req.params.quiet = measure, True
    for k, v in kw.items():
        setattr(req.params, k, v)
    return ds.train_model(req), native.last_train_stats()["neural_lambdarank"]


def _flat(net):
    n = net["NeuralNet"]
    return np.concatenate([np.asarray(n[k], dtype=np.float64).ravel() for k in PARTS if k in n] + [[n["output_bias"]]])


def _draw(seed, c, fan):
    """csrc/neural_lambda.hpp's initialiser: parameter number c under the scale sqrt(6 / fan)."""
    M, G = 2 ** 64 - 1, 0x9E3779B97F4A7C15

    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    return (2.0 * ((mix((mix((seed + 4 * G) & M) + c) & M) >> 11) * 2.0 ** -53) - 1.0) * np.sqrt(6.0 / fan)


@pytest.fixture(scope="module")
def sets():
    d = np.load(os.path.join(GOLDEN, "trec_news_2018.npz"))
    raw = fr.CDataset.from_numpy(d["train_X"], d["train_y"], d["train_qid"])
    # labels that need a product of two hidden features: |x0 + x1| |x2|
    rng = np.random.default_rng(4)
    X = rng.normal(0.0, 1.0, (1500, 8)).astype(np.float32)
    y = np.floor(np.minimum(3.0, np.abs(X[:, 0] + X[:, 1]) * np.abs(X[:, 2]))).astype(np.float64)
    return {"trec": fr.Normalizer.fit(raw, "zscore").apply(raw), "synth": fr.CDataset.from_numpy(X, y, np.repeat(np.arange(1, 31, dtype=np.int64), 50))}


def test_every_iteration_is_its_stages(sets):
    ds, measure, h, h2, lr, l2, sigma, T, seed = sets["trec"], "ndcg@10", 5, 3, 0.05, 0.125, 1.5, 3, 3
    kw = dict(measure=measure, hidden=h, num_iterations=T, learning_rate=lr, lambda_l2=l2, sigma=sigma, seed=seed, trace=True)
    model, st = _train(ds, hidden2=h2, **kw)
    nets = [st["initial"]] + st["iterates"]
    assert st["iterations"] == T and len(nets) == T + 1 and st["score_plan"]["hidden2"] == st["backprop_plan"]["hidden2"] == h2
    # the initial net: W1 is the one-layer request's bit for bit, W2 / w3 are the header's draws, the biases 0
    first, d = nets[0]["NeuralNet"], len(nets[0]["NeuralNet"]["hidden_weights"][0])
    assert first["hidden_weights"] == _train(ds, **kw)[1]["initial"]["NeuralNet"]["hidden_weights"]
    cw2 = h * d + h
    assert first["hidden2_weights"] == [[_draw(seed, cw2 + k * h + j, h + h2) for j in range(h)] for k in range(h2)]
    assert first["output_weights"] == [_draw(seed, cw2 + h2 * h + h2 + k, h2 + 1) for k in range(h2)]
    assert first["hidden_bias"] == [0.0] * h and first["hidden2_bias"] == [0.0] * h2 and first["output_bias"] == 0.0
    decays = np.concatenate([np.ones(h * d), np.zeros(h), np.ones(h2 * h), np.zeros(h2), np.ones(h2), [0]])
    theta, m, v = _flat(nets[0]), np.zeros(len(decays)), np.zeros(len(decays))
    for t in range(T):
        net = fr.CModel.from_dict(nets[t])
        lam, _ = native.lambda_gradients(net, ds, measure, sigma)
        g = native.mlp2_gradients(ds, net, lam)
        theta, m, v = native.adam_step(theta, _flat({"NeuralNet": g}), m, v, t + 1, lr, l2, decays)
        assert np.array_equal(theta, _flat(nets[t + 1])), t
        _, per_q = native.evaluate_dense(fr.CModel.from_dict(nets[t + 1]), ds, measure)
        assert st["train_measure"][t] == o.mean(per_q), t
    tm, best = st["train_measure"], st["best_iteration"]
    beats = [t for t in range(T) if tm[t] > st["initial_measure"]]
    assert best == (1 + tm.index(max(tm[t] for t in beats)) if beats else 1) and model.to_dict() == nets[best]
    # the JSON round trip scores the same bytes; the same request twice gives the same model
    again = fr.CModel.from_dict(json.loads(json.dumps(model.to_dict())))
    assert np.array_equal(native.predict_scores_dense(again, ds), native.predict_scores_dense(model, ds))
    assert _train(ds, hidden2=h2, **kw)[0].to_dict() == model.to_dict()


@pytest.mark.parametrize("hidden2", [0, 65])
def test_hidden2_outside_its_range_is_refused(sets, hidden2):
    with pytest.raises(Exception, match="hidden2 must be between 1 and 64"):
        _train(sets["synth"], hidden=4, num_iterations=1, hidden2=hidden2)


def test_the_second_layer_fits_what_one_layer_fits_badly(sets):
    """Seed 0: 0.9597 against 0.9976 after 60 iterations; seeds 1 to 3 leave 0.010 to 0.028 between the two."""
    kw = dict(measure="ndcg", hidden=16, num_iterations=60, learning_rate=0.05, seed=0)
    one, two = _train(sets["synth"], **kw)[1], _train(sets["synth"], hidden2=16, **kw)[1]
    print("one layer %.6f, two layers %.6f" % (one["train_measure"][-1], two["train_measure"][-1]))
    assert two["train_measure"][-1] > one["train_measure"][-1]
