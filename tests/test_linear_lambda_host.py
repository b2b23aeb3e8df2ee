"""The linear LambdaRank trainer without a device: the variant's wire form and refusals, the host solver
(native.newton_step) against exact rational arithmetic, and csrc/linear_lambda.hpp under the sanitizers."""
import json
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import clib, native
from fastrank_amd.training import LinearLambdaRankParams, TrainRequest

KEYS = ["num_iterations", "learning_rate", "lambda_l2", "sigma", "quiet"]


def _dataset():
    X = np.arange(24, dtype=np.float32).reshape(8, 3)
    y = np.array([0, 1, 2, 0, 1, 0, 0, 1], dtype=np.float64)
    qid = np.array([1, 1, 1, 1, 2, 2, 2, 2], dtype=np.int64)
    return fr.CDataset.from_numpy(X, y, qid)


def _train_raw(params, measure="ndcg", variant="LinearLambdaRank"):
    text = json.dumps({"measure": measure, "params": {variant: params}, "judgments": None}).encode()
    ds = _dataset()  # (kept alive over the call: a request that passes the parser reads it)
    return clib._unwrap(clib._load().train_model(text, ds.pointer))


def _params(**kw):
    p = LinearLambdaRankParams(quiet=True, num_iterations=2).to_dict()
    p.update(kw)
    return p


def test_defaults_and_round_trip():
    assert fr.query_json("linear_lambdarank_defaults") == {
        "measure": "ndcg", "judgments": None,
        "params": {"LinearLambdaRank": {"num_iterations": 20, "learning_rate": 1.0, "lambda_l2": 1.0, "sigma": 1.0, "quiet": False}}}
    req = TrainRequest.linear_lambdarank()
    assert req.params == LinearLambdaRankParams() and list(req.to_dict()["params"]["LinearLambdaRank"]) == KEYS
    req.params = LinearLambdaRankParams(num_iterations=3, lambda_l2=0.5, objective="ap", truncation_level=5, lambda_norm=True)
    wire = req.to_dict()["params"]["LinearLambdaRank"]
    assert list(wire) == KEYS + ["objective", "truncation_level", "lambda_norm"] and wire["objective"] == "map"
    assert TrainRequest.from_dict(json.loads(json.dumps(req.to_dict()))) == req and req.clone() == req


@pytest.mark.parametrize("change,text", [
    ({"validation_queries": ["1"]}, "held-out queries are not supported by LinearLambdaRank"),
    ({"early_stopping_rounds": 3}, "held-out queries are not supported by LinearLambdaRank"),
    ({"init_model": None}, "init_model is not supported by LinearLambdaRank"),
    ({"validation_dataset": None}, "a validation dataset is not supported by LinearLambdaRank"),
    ({"valid": None}, "a validation dataset is not supported by LinearLambdaRank"),
    ({"num_trees": 5}, "unknown field `num_trees` of LinearLambdaRankParams"),
    ({"num_iterations": 0}, "num_iterations must be at least 1"),
    ({"learning_rate": 0.0}, "learning_rate must be finite and greater than 0"),
    ({"lambda_l2": -0.5}, "lambda_l2 must be finite and at least 0"),
    ({"sigma": 0.0}, "sigma must be finite and greater than 0"),
    ({"objective": "auc"}, "objective must be `ndcg`, `map` or `mrr`, not `auc`"),
    ({"objective": "xendcg", "truncation_level": 2}, "truncation_level cannot be combined with objective `xendcg`"),
    ({"objective": "xendcg", "lambda_norm": True}, "lambda_norm cannot be combined with objective `xendcg`"),
])
def test_refusals(change, text):
    with pytest.raises(Exception, match=text):
        _train_raw(_params(**change))


def test_refusals_of_the_request():
    with pytest.raises(Exception, match="missing field `lambda_l2`"):
        _train_raw({k: v for k, v in _params().items() if k != "lambda_l2"})
    with pytest.raises(Exception, match="unsupported training measure"):
        _train_raw(_params(), "map")
    with pytest.raises(Exception, match="unknown variant `GBDT`, expected one of `CoordinateAscent`, `RandomForest`, `LambdaMART`, `LinearLambdaRank`"):
        _train_raw(_params(), variant="GBDT")
    ds, req = _dataset(), TrainRequest.linear_lambdarank()
    zero = fr.CModel.from_dict({"Linear": {"weights": [0.0, 0.0, 0.0]}})
    with pytest.raises(Exception, match="are not supported by LinearLambdaRank"):
        ds.train_model(req, valid=_dataset())
    with pytest.raises(Exception, match="are not supported by LinearLambdaRank"):
        ds.train_model(req, init_model=zero)


def _designed(n, ill, seed):
    """An exactly representable symmetric positive definite A = L D L^T: L unit lower bidiagonal with +-1 below the diagonal,
    D all 1, or when `ill` a descending run of powers of two from 2^0 to 2^-40 (condition number beyond 10^12 from n = 2 on)."""
    rng = np.random.default_rng(seed)
    L = np.eye(n, dtype=np.int64) + np.diag(rng.choice([-1, 1], max(n - 1, 0)), -1)[:n, :n]
    D = [Fraction(1, 2 ** ((40 * k) // max(n - 1, 1))) if ill else Fraction(1) for k in range(n)]
    A = [[sum(int(L[i, k]) * D[k] * int(L[j, k]) for k in range(min(i, j) + 1)) for j in range(n)] for i in range(n)]
    Af = np.array([[float(v) for v in row] for row in A])
    assert all(Fraction(Af[i, j]) == A[i][j] for i in range(n) for j in range(n))
    return A, Af


@pytest.mark.parametrize("ill", [False, True])
@pytest.mark.parametrize("n", [1, 2, 17, 136])
def test_newton_step_residual_within_choleskys_backward_error(n, ill):
    """The computed delta solves (A + dA) delta = g with |dA| <= gamma_(3n+1) |R^T| |R| (Higham, Accuracy and Stability of
    Numerical Algorithms, 2nd ed., Thm 10.4), and || |R^T| |R| ||_2 <= n (1 - n gamma_(n+1))^-1 ||A||_2 (eq. 10.7, from Thm
    10.3).  The solver also rounds A_jj = fl(H_jj + lambda_l2) once, a relative perturbation u of the diagonal: one more u in
    the constant.  With ||A||_2 <= ||A||_F the exact residual obeys
        || g - A delta ||_2  <=  gamma_(3n+2) * n / (1 - n gamma_(n+1)) * ||A||_F * ||delta||_2,   gamma_k = k u / (1 - k u), u = 2^-53.
    The derived constant is c(n) = n gamma_(3n+2) / (1 - n gamma_(n+1)) (about 3 n^2 u: 6.2e-12 at n = 136); both sides are
    compared squared, in exact rational arithmetic.  The ill-conditioned systems are solved under lambda_l2 = 2^-60, far below
    D's smallest entry, so that the system solved keeps A's condition number."""
    A, Af = _designed(n, ill, 10 * n + ill)
    l2 = 2.0 ** -60 if ill else 0.25
    assert not (ill and n > 1) or np.linalg.cond(Af + l2 * np.eye(n)) > 1e12
    rng = np.random.default_rng(n)
    g = rng.normal(0.0, 1.0, n)
    delta = native.newton_step(Af, g, l2)
    u = Fraction(1, 2 ** 53)
    gamma = lambda k: k * u / (1 - k * u)  # noqa: E731
    c = n * gamma(3 * n + 2) / (1 - n * gamma(n + 1))
    df = [Fraction(float(v)) for v in delta]
    Al = [[A[i][j] + (Fraction(l2) if i == j else 0) for j in range(n)] for i in range(n)]
    res = [Fraction(float(g[i])) - sum(Al[i][j] * df[j] for j in range(n)) for i in range(n)]
    lhs = sum(r * r for r in res)
    rhs = c * c * sum(v * v for row in Al for v in row) * sum(v * v for v in df)
    assert lhs <= rhs, (float(lhs) ** 0.5, float(rhs) ** 0.5)
    assert np.array_equal(delta, native.newton_step(Af, g, l2))


def test_a_pivot_that_is_not_positive_is_a_plain_error():
    A = np.array([[1.0, 2.0], [2.0, 1.0]])
    with pytest.raises(Exception, match=r"not positive definite at feature 1 \(pivot -3 under lambda_l2 = 0\); try a larger lambda_l2"):
        native.newton_step(A, np.ones(2), 0.0)
    assert np.allclose(native.newton_step(A, np.array([4.0, 5.0]), 3.0), np.linalg.solve(A + 3.0 * np.eye(2), [4.0, 5.0]), rtol=1e-14)
    with pytest.raises(Exception, match="not positive definite at feature 0"):
        native.newton_step(np.zeros((3, 3)), np.ones(3), 0.0)


def test_host_header_under_address_and_undefined_sanitizers(tmp_path):
    """tests/linear_lambda_sanitize.cpp: a program of its own over csrc/linear_lambda.hpp, built with
    -fsanitize=address,undefined and run directly."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "linear_lambda_sanitize")
    build = subprocess.run([cxx, "-std=c++17", "-O0", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                            "-I", os.path.join(here, "..", "fastrank_amd", "csrc"), os.path.join(here, "linear_lambda_sanitize.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "linear_lambda ok" in run.stdout, run.stdout
