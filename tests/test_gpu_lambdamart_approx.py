"""The ApproxNDCG objective on the device (lambda_grad_approx_kernel and its wave kernel; DESIGN.md section 11, "ApproxNDCG
objective") through native.lambda_gradients, against the exact statement and the numpy restatement
(tests/lambdamart_approx_model.py).  Query lengths: one document, the wave kernel up to its limit of 64, the staged workgroup
path up to its limit of 256, and 257 documents (five blocks, fifteen tiles) on the path that stages nothing."""
import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import native
from oracle import pyoracle as o
from tests import lambdamart_approx_model as am
from tests import lambdamart_model as lm
from tests.lambdamart_xendcg_model import gains

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 63, 64, 65, 256, 257]
TIED = [5, 13, 61, 125]  # 1 + r = (n + 3) / 2 is a power of two
ALPHA = 1.5


@pytest.fixture(scope="module")
def data():
    """Query q + 1 has LENGTHS[q] documents with continuous scores; then the TIED lengths with equal scores; then ten
    documents without a positive label.  The score is column 0; stored order is row order."""
    rng = np.random.default_rng(2010)
    lens = LENGTHS + TIED + [10]
    qid = np.concatenate([np.full(n, q + 1, dtype=np.int64) for q, n in enumerate(lens)])
    y = rng.choice(5, size=len(qid), p=[0.5, 0.2, 0.15, 0.1, 0.05]).astype(np.float64)
    y[np.flatnonzero(np.diff(qid, prepend=0))] = 2.0  # (a positive label in every query)
    X = np.zeros((len(qid), 2), dtype=np.float32)
    X[:, 0] = rng.standard_normal(len(qid)) * 3.0
    for q in range(len(LENGTHS), len(lens) - 1):
        X[qid == q + 1, 0] = 0.25 * (q - 8)
        y[qid == q + 1] = np.arange(lens[q]) % 5
    y[qid == len(lens)] = 0.0
    g, c = fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)
    model = fr.CModel.from_dict({"Linear": {"weights": [1.0, 0.0]}})
    scores = native.predict_scores_dense(model, g)
    assert np.array_equal(scores, X[:, 0].astype(np.float64))
    queries, norms = lm.query_lists(c), c.default_norms("ndcg")
    assert [len(ids) for ids in queries] == lens and np.isnan(norms[-1])
    lam, wt = native.lambda_gradients(model, g, "ndcg", ALPHA, objective="approxndcg")
    return g, model, scores, gains(y), queries, norms, lam, wt, c.default_norms("ndcg@3")


@pytest.mark.parametrize("q", range(len(LENGTHS)), ids=["n=%d" % n for n in LENGTHS])
def test_continuous_scores_lie_within_the_bound_of_the_exact_statement(data, q):
    g, model, scores, G, queries, norms, lam, wt, norms3 = data
    ids = queries[q]
    assert not wt[ids].any()
    if len(ids) == 1:
        assert lam[ids].tobytes() == np.zeros(1).tobytes()
        return
    ratio = am.worst_ratio(am.ExactApprox(scores[ids], G[ids], norms[q], ALPHA), lam[ids])
    print("device, n = %d: worst error / bound %.3f" % (len(ids), ratio))
    assert lam[ids].any()
    # the query alone (first in its launch, whatever kernel the others go to) gets the bits it has among the others
    alone = native.lambda_gradients(model, g, "ndcg", ALPHA, objective="approxndcg", queries=np.asarray([q]))
    assert alone[0][ids].tobytes() == lam[ids].tobytes() and not alone[1][ids].any()
    rest = np.ones(len(lam), dtype=bool)
    rest[ids] = False
    assert np.all(np.isnan(alone[0][rest]))


def test_the_same_call_gives_the_same_bytes_and_a_view_its_parents_bits(data):
    g, model, scores, G, queries, norms, lam, wt, norms3 = data
    again = native.lambda_gradients(model, g, "ndcg", ALPHA, objective="approxndcg")
    assert again[0].tobytes() == lam.tobytes() and again[1].tobytes() == wt.tobytes()
    names = ["3", "5", "7"]  # 63, 65 and 257 documents: one of each path, first in their launches
    view = native.lambda_gradients(model, g.subsample_queries(names), "ndcg", ALPHA, objective="approxndcg", n_total=len(lam))
    inside = np.concatenate([queries[int(x) - 1] for x in names])
    assert view[0][inside].tobytes() == lam[inside].tobytes()
    # the depth reaches the norm and nothing else: the gradient scales by the ratio of the norms
    deep = native.lambda_gradients(model, g, "ndcg@3", ALPHA, objective="approxndcg")
    ids = queries[4]
    assert norms3[4] < norms[4]
    assert np.allclose(deep[0][ids], lam[ids] * (norms[4] / norms3[4]), rtol=0.0, atol=1e-12 * np.abs(lam[ids]).max())


def test_tied_scores_are_the_restatements_bits(data):
    g, model, scores, G, queries, norms, lam, wt, norms3 = data
    for q in range(len(LENGTHS), len(LENGTHS) + len(TIED)):
        ids = queries[q]
        exp, _ = am.query_gradients(scores[ids], G[ids], norms[q], ALPHA)
        assert exp.any() and lam[ids].tobytes() == exp.tobytes(), "query of %d tied documents" % len(ids)
        assert not wt[ids].any()


def test_a_query_without_a_positive_norm_gets_zeros(data):
    g, model, scores, G, queries, norms, lam, wt, norms3 = data
    ids = queries[-1]
    assert lam[ids].tobytes() == np.zeros(len(ids)).tobytes() and wt[ids].tobytes() == np.zeros(len(ids)).tobytes()
