"""LambdaMART's histogram grower without a GPU: the `grower` wire key and its validation (every request here fails or is
only parsed before any device work), and self-checks of the numpy restatement (tests/lambdamart_hist_model.py) that
the GPU tests hold the device to."""
import json

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import clib
from fastrank_amd.training import LambdaMARTParams, TrainRequest
from oracle import pyoracle as o
from tests import lambdamart_hist_model as hm
from tests import lambdamart_model as lm
from tests.conftest import synth_dataset

KEYS = ["num_trees", "learning_rate", "max_depth", "min_leaf_support", "split_candidates", "sigma", "quiet"]


def _dataset():
    X = np.arange(24, dtype=np.float32).reshape(8, 3)
    y = np.array([0, 1, 2, 0, 1, 0, 0, 1], dtype=np.float64)
    qid = np.array([1, 1, 1, 1, 2, 2, 2, 2], dtype=np.int64)
    return fr.CDataset.from_numpy(X, y, qid)


def _train_raw(params, measure="ndcg"):
    ds = _dataset()
    text = json.dumps({"measure": measure, "params": {"LambdaMART": params}, "judgments": None}).encode()
    return clib._unwrap(clib._load().train_model(text, ds.pointer))


def _params(**kw):
    p = LambdaMARTParams().to_dict()
    p.update(kw)
    return p


# --- wire form ---------------------------------------------------------------------------------

@pytest.mark.parametrize("value", ["hist", "Histogram", "", "EXACT"])
def test_bad_grower_value_is_rejected(value):
    with pytest.raises(Exception, match="invalid value") as e:
        _train_raw(_params(grower=value))
    assert "`exact`" in str(e.value) and "`histogram`" in str(e.value)


@pytest.mark.parametrize("value", [1, None, True, ["histogram"], {"histogram": []}])
def test_bad_grower_type_is_rejected(value):
    with pytest.raises(Exception, match="invalid type") as e:
        _train_raw(_params(grower=value))
    assert "expected a string for grower" in str(e.value)


@pytest.mark.parametrize("k", [0, 1, 257, 1000])
def test_histogram_needs_2_to_256_candidates(k):
    with pytest.raises(Exception, match="invalid value") as e:
        _train_raw(_params(grower="histogram", split_candidates=k))
    assert "split_candidates must be between 2 and 256 for the histogram grower" in str(e.value)


@pytest.mark.parametrize("grower", ["exact", "histogram"])
def test_accepted_spellings_reach_the_later_checks(grower):
    """A valid `grower` passes the parser: the request then fails on what is checked after the parameters (the measure)."""
    with pytest.raises(Exception, match=r"supported: ndcg, ndcg@k"):
        _train_raw(_params(grower=grower), "map")
    with pytest.raises(Exception, match="num_trees must be at least 1"):
        _train_raw(_params(grower=grower, num_trees=0))


def test_the_seven_keys_stay_required_with_grower():
    for key in KEYS:
        p = _params(grower="histogram")
        del p[key]
        with pytest.raises(Exception, match="missing field `%s`" % key):
            _train_raw(p)


def test_defaults_keep_their_seven_keys():
    assert list(clib.query_json("lambdamart_defaults")["params"]["LambdaMART"].keys()) == KEYS
    assert list(LambdaMARTParams().to_dict().keys()) == KEYS
    assert LambdaMARTParams().grower == "exact"
    assert list(LambdaMARTParams(grower="exact").to_dict().keys()) == KEYS


def test_histogram_request_round_trips():
    req = TrainRequest.lambdamart()
    assert req.params.grower == "exact"
    req.params.grower = "histogram"
    req.params.split_candidates = 32
    d = req.to_dict()
    assert list(d["params"]["LambdaMART"].keys()) == KEYS + ["grower"]
    assert d["params"]["LambdaMART"]["grower"] == "histogram"
    back = TrainRequest.from_dict(d)
    assert back == req and back.params.grower == "histogram"
    c = req.clone()
    assert c == req and c is not req and c.params is not req.params
    assert c != TrainRequest.lambdamart()
    # an explicit "exact" on the wire reads back as the default
    d["params"]["LambdaMART"]["grower"] = "exact"
    assert TrainRequest.from_dict(d).params.grower == "exact"


# --- the restatement's own properties ----------------------------------------------------------

def _columns():
    rng = np.random.default_rng(5)
    n = 3000
    cols = {
        "uniform": rng.random(n),
        "integers": np.floor(rng.exponential(2.0, n)),
        "sparse": np.where(rng.random(n) < 0.7, 0.0, rng.random(n)),
        "constant": np.full(n, 3.5),
        "signed_zero": np.where(rng.random(n) < 0.5, -0.0, 0.0),
        "signed_zero_mix": np.where(rng.random(n) < 0.3, -0.0, rng.integers(-2, 3, n).astype(np.float64)),
        "five_values": rng.integers(0, 5, n).astype(np.float64),
        "heavy_tail": rng.lognormal(0.0, 2.0, n),
        "mostly_max": np.where(rng.random(n) < 0.9, 7.0, rng.random(n)),
        "two": np.array([1.0, 2.0]),
        "one": np.array([4.0]),
    }
    return {k: v.astype(np.float32) for k, v in cols.items()}


@pytest.mark.parametrize("k", [2, 3, 16, 64, 256])
def test_bins_are_the_scoring_partition(k):
    for name, col in _columns().items():
        e = hm.bin_edges(col, k)
        b = hm.bin_column(col, e)
        assert len(e) <= k - 1, name
        assert np.all(np.diff(e) > 0), name
        assert int(b.max()) <= len(e), name
        distinct = np.unique(hm.canon(col))
        if len(distinct) <= k:
            assert np.array_equal(e, distinct[:-1]), name
        if len(distinct) == 1:
            assert len(e) == 0 and not b.any(), name
        for j in range(len(e)):
            left = b <= j
            assert np.array_equal(left, col.astype(np.float64) <= float(e[j])), (name, j)
            assert left.any() and not left.all(), (name, j)
        assert not np.any(np.signbit(e)[e == 0.0]), name  # a zero edge is +0.0


def test_nan_is_refused_by_the_restatement():
    with pytest.raises(ValueError):
        hm.bin_edges(np.array([1.0, np.nan, 2.0], dtype=np.float32), 4)


@pytest.mark.parametrize("col", [[-np.inf, -np.inf, 1, 2, 3, 4, np.inf], [1, 2, np.inf], [-np.inf, 1, 2]])
def test_infinite_values_are_refused_by_the_restatement(col):
    """Every distinct value but the largest is an edge, so -inf would become a split: a tree that cannot be written down
    (JSON has null for it), continued or explained.  Training refuses +-inf like NaN, and so does the restatement."""
    with pytest.raises(ValueError, match="infinite feature value"):
        hm.bin_edges(np.array(col, dtype=np.float32), 4)
    assert len(hm.bin_edges(np.array([1, 2, 3.4e38], dtype=np.float32), 4)) == 2  # (the largest finite float is a value like any)


def test_fixed_point_sums_do_not_depend_on_order():
    rng = np.random.default_rng(9)
    n = 100_000
    lam = rng.normal(0.0, 1.0, n) * 10.0 ** rng.integers(-8, 3, n)
    Q, S = hm.quantise(lam, n)
    c = n.bit_length()
    assert c == int(np.ceil(np.log2(n + 1)))
    assert int(np.abs(Q).max()) <= 2 ** (61 - c)
    assert int(np.abs(Q).max()) > 2 ** (59 - c)
    total = int(Q.sum())
    assert total == sum(int(x) for x in Q)  # no int64 wrap
    for _ in range(3):
        assert int(Q[rng.permutation(n)].sum()) == total
    # parent minus child is exact
    part = rng.random(n) < 0.3
    assert int(Q[part].sum()) + int(Q[~part].sum()) == total
    np.testing.assert_allclose(np.ldexp(Q.astype(np.float64), -S), lam, rtol=0, atol=np.ldexp(0.5, -S))
    # a power of two as the largest magnitude sits on the bound, not beyond it
    Q2, S2 = hm.quantise(np.array([0.25, -0.5, 0.125]), 3)
    assert S2 == 61 - 0 - 2 and list(Q2) == [2 ** 57, -(2 ** 58), 2 ** 56]
    Qz, Sz = hm.quantise(np.zeros(5), 5)
    assert Sz is None and not Qz.any()


def test_limb_histogram_equals_integer_adds():
    rng = np.random.default_rng(11)
    n = 20_000
    Q, _ = hm.quantise(rng.normal(0, 1, n), n)
    b = rng.integers(0, 37, n)
    exp = np.zeros(40, dtype=np.int64)
    np.add.at(exp, b, Q)
    assert np.array_equal(hm.int_hist(b, Q, 40), exp)


@pytest.mark.parametrize("k,min_leaf", [(4, 1), (16, 10), (64, 1), (64, 200)])
def test_chosen_split_equals_brute_force(k, min_leaf):
    X, y, qid = synth_dataset(13, 1500, 7, 20)
    rng = np.random.default_rng(k)
    lam = rng.normal(0, 1, len(y))
    ids = np.arange(len(y))
    feats = list(range(X.shape[1]))
    edges, xbin = hm.bin_matrix(X, ids, feats, k)
    Q, S = hm.quantise(lam, len(y))
    rows = np.flatnonzero(rng.random(len(y)) < 0.6)
    got = hm.best_split(xbin, edges, Q, rows, min_leaf)
    best = None
    qtot = sum(int(q) for q in Q[rows])
    for slot, f in enumerate(feats):
        x = X[rows, f].astype(np.float64)
        for j, e in enumerate(edges[slot]):
            left = x <= float(e)
            nl, nr = int(left.sum()), int((~left).sum())
            if nl < max(min_leaf, 1) or nr < max(min_leaf, 1):
                continue
            ql = sum(int(q) for q in Q[rows][left])
            imp = (float(ql) * float(ql)) / float(nl) + (float(qtot - ql) * float(qtot - ql)) / float(nr)
            if best is None or imp >= best[0]:
                best = (imp, slot, j, nl, ql)
    assert got == best
    if min_leaf == 200:
        assert got is None or (got[3] >= 200 and len(rows) - got[3] >= 200)


def test_fit_tree_leaves_are_newton_steps_of_their_partition():
    X, y, qid = synth_dataset(17, 1200, 6, 15)
    rng = np.random.default_rng(2)
    lam, wt = rng.normal(0, 1, len(y)), rng.random(len(y))
    ids = np.arange(len(y))
    tree = hm.fit_tree(X, lam, wt, ids, range(X.shape[1]), 4, 20, 16)
    assert "FeatureSplit" in tree
    reached = lm.route(tree, X, ids)
    n = len(y)
    Q, S = hm.quantise(lam, n)
    W, Sw = hm.quantise(wt, n)
    leaves = {id(r): r for r in reached}
    assert 2 <= len(leaves) <= 8
    for key, leaf in leaves.items():
        sel = np.array([id(r) == key for r in reached])
        assert sel.sum() >= 20
        exp = np.ldexp(float(Q[sel].sum()), -S) / np.ldexp(float(W[sel].sum()), -Sw)
        assert leaf["LeafNode"] == exp
        assert abs(exp - lam[sel].sum() / wt[sel].sum()) <= 1e-9 * abs(exp) + 1e-12
    assert hm.fit_tree(X, np.zeros(n), wt, ids, range(X.shape[1]), 4, 20, 16) == {"LeafNode": 0.0}


# seed, size and tree count chosen on the CPU so that this holds for the restatement alone
LEARNING_CASE = dict(seed=3, n=1500, d=8, q=25, measure="ndcg@10", num_trees=12, max_depth=4, min_leaf_support=10,
                     split_candidates=16)


def test_restatement_learns():
    k = LEARNING_CASE
    X, y, qid = synth_dataset(k["seed"], k["n"], k["d"], k["q"])
    c = o.Dataset(X, y, qid)
    _, _, measures = hm.train(X, y, c, k["measure"], num_trees=k["num_trees"], max_depth=k["max_depth"],
                              min_leaf_support=k["min_leaf_support"], split_candidates=k["split_candidates"])
    assert len(measures) == k["num_trees"]
    assert measures[-1] > measures[0] + 0.02
