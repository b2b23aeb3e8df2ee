"""The ApproxNDCG objective without a device ("ApproxNDCG objective"): the exact statement is the
gradient of the stated function, the numpy restatement lies within the derived bound of it, and the request's plumbing."""
import decimal
import json
from decimal import Decimal

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import clib
from fastrank_amd.training import LambdaMARTParams, LinearLambdaRankParams, NeuralLambdaRankParams, TrainRequest
from tests import lambdamart_approx_model as am
from tests import lambdamart_exact as ex


def _query(n, seed, spread=3.0):
    rng = np.random.default_rng(seed)
    s = (rng.standard_normal(n) * spread).astype(np.float32).astype(np.float64)
    G = 2.0 ** rng.choice(5, n).astype(np.float64) - 1.0
    G[0] = 3.0
    return s, G, float(np.sum(np.sort(G)[::-1] / np.log2(np.arange(n) + 2.0)))


@pytest.mark.parametrize("n, alpha", [(2, 1.0), (7, 2.5), (19, 0.5)])
def test_the_exact_gradient_is_the_finite_difference_of_the_exact_objective(n, alpha):
    s, G, N = _query(n, n)
    e = am.ExactApprox(s, G, N, alpha)
    h = Decimal(10) ** -20  # (truncation ~ h^2 = 1e-40, the 60-digit roundings ~ 1e-60 / h = 1e-40)
    with decimal.localcontext(am.CTX):
        assert abs(e.A - am.exact_objective(e.s, e.G, e.N, e.alpha)) <= Decimal(10) ** -55  # (two routes through 60-digit roundings)
        for k in range(n):
            up, dn = list(e.s), list(e.s)
            up[k], dn[k] = e.s[k] + h, e.s[k] - h
            fd = (am.exact_objective(up, e.G, e.N, e.alpha) - am.exact_objective(dn, e.G, e.N, e.alpha)) / (2 * h)
            assert abs(fd - e.lam[k]) <= Decimal(10) ** -34, (k, fd, e.lam[k])
        assert any(v != 0 for v in e.lam) and abs(sum(e.lam)) <= Decimal(10) ** -50  # (a shift of every score changes nothing)


@pytest.mark.parametrize("n, alpha, spread", [(2, 1.0, 3.0), (65, 1.5, 3.0), (40, 10.0, 5.0)])
def test_the_numpy_restatement_lies_within_the_bound(n, alpha, spread):
    s, G, N = _query(n, 100 + n, spread)
    lam, A = am.query_gradients(s, G, N, alpha)
    e = am.ExactApprox(s, G, N, alpha)
    print("numpy, n = %d: worst error / bound %.3f" % (n, am.worst_ratio(e, lam)))
    assert abs(ex.dec(A) - e.A) <= Decimal(10) ** -12 and 0.0 < A <= 1.0


def _train_raw(variant, params):
    X = np.arange(24, dtype=np.float32).reshape(8, 3)
    ds = fr.CDataset.from_numpy(X, np.array([0, 1, 2, 0, 1, 0, 0, 1], dtype=np.float64), np.array([1] * 4 + [2] * 4, dtype=np.int64))
    text = json.dumps({"measure": "ndcg", "params": {variant: params}, "judgments": None}).encode()
    return clib._unwrap(clib._load().train_model(text, ds.pointer))


@pytest.mark.parametrize("variant, params, text", [
    ("LambdaMART", LambdaMARTParams(quiet=True, objective="approxndcg").to_dict(), "objective `approxndcg` is not supported by LambdaMART"),
    ("LinearLambdaRank", LinearLambdaRankParams(quiet=True, objective="approxndcg").to_dict(), "objective `approxndcg` is not supported by LinearLambdaRank"),
    ("NeuralLambdaRank", NeuralLambdaRankParams(quiet=True, objective="approxndcg", truncation_level=2).to_dict(),
     "truncation_level cannot be combined with objective `approxndcg`"),
    ("NeuralLambdaRank", NeuralLambdaRankParams(quiet=True, objective="approxndcg", lambda_norm=True).to_dict(),
     "lambda_norm cannot be combined with objective `approxndcg`"),
])
def test_refusals(variant, params, text):
    with pytest.raises(Exception, match=text):
        _train_raw(variant, params)


def test_the_request_round_trips():
    req = TrainRequest(measure="ndcg@10", params=NeuralLambdaRankParams(objective="approxndcg", sigma=10.0, hidden2=3))
    wire = req.to_dict()
    assert wire["params"]["NeuralLambdaRank"]["objective"] == "approxndcg"
    assert TrainRequest.from_dict(wire).to_dict() == wire
    assert "objective" not in TrainRequest(params=NeuralLambdaRankParams()).to_dict()["params"]["NeuralLambdaRank"]
