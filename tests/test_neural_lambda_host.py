"""The NeuralNet model and the neural LambdaRank trainer without a device: wire forms, refusals, the
initialiser and native.adam_step against restatements, csrc/neural_lambda.hpp under the sanitizers."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import clib, native
from fastrank_amd.training import NeuralLambdaRankParams, TrainRequest

KEYS = ["hidden", "num_iterations", "learning_rate", "lambda_l2", "sigma", "seed", "quiet"]
NET = {"NeuralNet": {"activation": "relu", "hidden_weights": [[0.5, -1.0, 0.0], [2.0, 0.25, -0.125]], "hidden_bias": [0.0, -1.5],
                     "output_weights": [1.0, -2.0], "output_bias": 0.75}}


def _dataset():
    X = np.arange(24, dtype=np.float32).reshape(8, 3)
    y = np.array([0, 1, 2, 0, 1, 0, 0, 1], dtype=np.float64)
    qid = np.array([1, 1, 1, 1, 2, 2, 2, 2], dtype=np.int64)
    return fr.CDataset.from_numpy(X, y, qid)


def _train_raw(params, measure="ndcg", variant="NeuralLambdaRank"):
    text = json.dumps({"measure": measure, "params": {variant: params}, "judgments": None}).encode()
    ds = _dataset()  # (kept alive over the call: a request that passes the parser reads it)
    return clib._unwrap(clib._load().train_model(text, ds.pointer))


def _params(**kw):
    p = NeuralLambdaRankParams(quiet=True, num_iterations=2).to_dict()
    p.update(kw)
    return p


def test_model_wire_form_round_trips():
    assert fr.CModel.from_dict(NET).to_dict() == NET
    ens = {"Ensemble": {"weights": [0.5, 2.0], "models": [NET, {"Linear": {"weights": [1.0]}}]}}
    assert fr.CModel.from_dict(ens).to_dict() == ens


@pytest.mark.parametrize("change,text", [
    ({"hidden_weights": [], "hidden_bias": [], "output_weights": []}, "at least one hidden unit"),
    ({"hidden_weights": [[0.5, -1.0, 0.0], [2.0, 0.25]]}, "rows of hidden_weights must have one length"),
    ({"hidden_bias": [0.0]}, "one number per row of hidden_weights"),
    ({"activation": "tanh"}, 'activation must be \\\\"relu\\\\"'),
    ({"output_bias": 1e999}, "number out of range"),  # (the JSON reader's own words: no number it accepts is non-finite)
    ({"hidden_weights": [[0.5, -1e999, 0.0], [2.0, 0.25, 1.0]]}, "number out of range"),
])
def test_model_refusals(change, text):
    with pytest.raises(Exception, match=text):
        clib._unwrap(clib._load().model_from_json(json.dumps({"NeuralNet": {**NET["NeuralNet"], **change}}).replace("Infinity", "1e999").encode()))


def test_unknown_variant_messages_begin_as_they_did():
    with pytest.raises(Exception, match="unknown variant `MLP`, expected one of `SingleFeature`, `Linear`, `DecisionTree`, `Ensemble`, `NeuralNet`"):
        clib._unwrap(clib._load().model_from_json(json.dumps({"MLP": {}}).encode()))
    with pytest.raises(Exception, match="unknown variant `GBDT`, expected one of `CoordinateAscent`, `RandomForest`, `LambdaMART`, `LinearLambdaRank`, `NeuralLambdaRank`"):
        _train_raw(_params(), variant="GBDT")


def test_request_defaults_and_round_trip():
    wire = fr.query_json("neural_lambdarank_defaults")
    assert wire["measure"] == "ndcg" and list(wire["params"]["NeuralLambdaRank"]) == KEYS
    req = TrainRequest.neural_lambdarank()
    assert req.params == NeuralLambdaRankParams() and req.to_dict() == wire
    req.params = NeuralLambdaRankParams(hidden=4, seed=2 ** 63 + 5, objective="ap", truncation_level=5, lambda_norm=True, trace=True)
    wire = req.to_dict()["params"]["NeuralLambdaRank"]
    assert list(wire) == KEYS + ["objective", "truncation_level", "lambda_norm", "trace"] and wire["objective"] == "map"
    assert TrainRequest.from_dict(json.loads(json.dumps(req.to_dict()))) == req and req.clone() == req


@pytest.mark.parametrize("change,text", [
    ({"validation_queries": ["1"]}, "held-out queries are not supported by NeuralLambdaRank"),
    ({"early_stopping_rounds": 3}, "held-out queries are not supported by NeuralLambdaRank"),
    ({"init_model": None}, "init_model is not supported by NeuralLambdaRank"),
    ({"validation_dataset": None}, "a validation dataset is not supported by NeuralLambdaRank"),
    ({"valid": None}, "a validation dataset is not supported by NeuralLambdaRank"),
    ({"num_trees": 5}, "unknown field `num_trees` of NeuralLambdaRankParams"),
    ({"hidden": 0}, "hidden must be between 1 and 1024"),
    ({"num_iterations": 0}, "num_iterations must be at least 1"),
    ({"learning_rate": 0.0}, "learning_rate must be finite and greater than 0"),
    ({"lambda_l2": -0.5}, "lambda_l2 must be finite and at least 0"),
    ({"sigma": 0.0}, "sigma must be finite and greater than 0"),
    ({"objective": "xendcg", "truncation_level": 2}, "truncation_level cannot be combined with objective `xendcg`"),
])
def test_request_refusals(change, text):
    with pytest.raises(Exception, match=text):
        _train_raw(_params(**change))


def test_the_measure_and_a_validation_dataset_or_init_model_are_refused():
    with pytest.raises(Exception, match="unsupported training measure"):
        _train_raw(_params(), "map")
    text = json.dumps({"measure": "ndcg", "params": {"NeuralLambdaRank": _params()}, "judgments": None}).encode()
    ds, model = _dataset(), fr.CModel.from_dict(NET)
    with pytest.raises(Exception, match="a validation dataset and an init model are not supported by NeuralLambdaRank"):
        clib._unwrap(clib._load().fr_train_model_with(text, ds.pointer, None, model.pointer))


def test_adam_step_is_its_operations():
    """Three steps against the header's recurrence written operation by operation (numpy rounds every one separately)."""
    rng = np.random.default_rng(3)
    n, lr, l2 = 37, 0.05, 0.25
    theta, m, v = rng.normal(0, 1, n), np.zeros(n), np.zeros(n)
    decays = rng.random(n) < 0.5
    et, em, evv, p1, p2 = theta.copy(), m.copy(), v.copy(), 1.0, 1.0
    for t in (1, 2, 3):
        g = rng.normal(0, 1, n) * 10.0 ** rng.integers(-6, 3, n)
        theta, m, v = native.adam_step(theta, g, m, v, t, lr, l2, decays)
        p1, p2 = p1 * 0.9, p2 * 0.999
        gp = np.where(decays, g - l2 * et, g)
        em = 0.9 * em + (1.0 - 0.9) * gp
        evv = 0.999 * evv + (1.0 - 0.999) * (gp * gp)
        et = et + (lr * (em / (1.0 - p1))) / (np.sqrt(evv / (1.0 - p2)) + 1e-8)
        assert np.array_equal(theta, et) and np.array_equal(m, em) and np.array_equal(v, evv), t


def test_host_header_under_address_and_undefined_sanitizers(tmp_path):
    """tests/neural_lambda_sanitize.cpp: a program of its own over csrc/neural_lambda.hpp, built with -fsanitize=address,undefined
    and run directly.  It prints the initial net of seed 7, which is held here to a restatement of the initialiser."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "neural_lambda_sanitize")
    build = subprocess.run([cxx, "-std=c++17", "-O0", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                            "-I", os.path.join(here, "..", "fastrank_amd", "csrc"), os.path.join(here, "neural_lambda_sanitize.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "neural_lambda ok" in run.stdout, run.stdout
    net = json.loads(next(ln for ln in run.stdout.splitlines() if ln.startswith("{")))["NeuralNet"]
    # the initialiser for seed 7, h = 3, d = 5, the view holding columns 1, 2 and 4
    M, G, h, d, held = 2 ** 64 - 1, 0x9E3779B97F4A7C15, 3, 5, [1, 2, 4]

    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    draw = lambda c, fan: (2.0 * ((mix((mix((7 + 4 * G) & M) + c) & M) >> 11) * 2.0 ** -53) - 1.0) * np.sqrt(6.0 / fan)  # noqa: E731
    assert net["hidden_weights"] == [[draw(j * d + i, len(held) + h) if i in held else 0.0 for i in range(d)] for j in range(h)]
    assert net["output_weights"] == [draw(h * d + h + j, h + 1) for j in range(h)]
    assert net["hidden_bias"] == [0.0] * h and net["output_bias"] == 0.0
