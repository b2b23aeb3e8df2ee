"""The Newton split gain of LambdaMART's histogram grower without a GPU: the four wire keys and their validation (every
request here fails or is only parsed before any device work), and self-checks of the numpy restatement
(tests/lambdamart_newton_model.py) that the GPU tests hold the device to."""
import json
import math
from fractions import Fraction

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import clib
from fastrank_amd.training import LambdaMARTParams, TrainRequest
from tests import lambdamart_hist_model as hm
from tests import lambdamart_newton_model as nm
from tests.conftest import synth_dataset

KEYS = ["num_trees", "learning_rate", "max_depth", "min_leaf_support", "split_candidates", "sigma", "quiet"]
NUMBERS = ["lambda_l2", "min_sum_hessian", "min_split_gain"]
DEFAULTS_TEXT = ('{"measure":"ndcg","params":{"LambdaMART":{"num_trees":100,"learning_rate":0.1,"max_depth":6,"min_leaf_support":10,'
                 '"split_candidates":64,"sigma":1.0,"quiet":false}},"judgments":null}')


def _dataset():
    X = np.arange(24, dtype=np.float32).reshape(8, 3)
    y = np.array([0, 1, 2, 0, 1, 0, 0, 1], dtype=np.float64)
    qid = np.array([1, 1, 1, 1, 2, 2, 2, 2], dtype=np.int64)
    return fr.CDataset.from_numpy(X, y, qid)


def _train_raw(params, measure="ndcg"):
    ds = _dataset()
    text = json.dumps({"measure": measure, "params": {"LambdaMART": params}, "judgments": None}).encode()
    return clib._unwrap(clib._load().train_model(text, ds.pointer))


def _train_python(**kw):
    req = TrainRequest.lambdamart()
    req.params.quiet = True
    for k, v in kw.items():
        setattr(req.params, k, v)
    return _dataset().train_model(req)


def _params(**kw):
    p = LambdaMARTParams().to_dict()
    p.update(kw)
    return p


def _both(match, **kw):
    """The request fails the same way as a raw JSON request and through the Python classes; returns the two messages."""
    out = []
    for call in (lambda: _train_raw(_params(**kw)), lambda: _train_python(**kw)):
        with pytest.raises(Exception, match=match) as e:
            call()
        out.append(str(e.value))
    return out


# --- wire form ---------------------------------------------------------------------------------------

def test_keys_are_absent_at_their_defaults():
    assert list(LambdaMARTParams().to_dict().keys()) == KEYS
    assert list(LambdaMARTParams(split_gain="variance", lambda_l2=0.0, min_sum_hessian=0.0, min_split_gain=0.0).to_dict().keys()) == KEYS
    p = LambdaMARTParams()
    assert (p.split_gain, p.lambda_l2, p.min_sum_hessian, p.min_split_gain) == ("variance", 0.0, 0.0, 0.0)
    assert list(TrainRequest.lambdamart().to_dict()["params"]["LambdaMART"].keys()) == KEYS


def test_defaults_text_is_unchanged():
    """The text the library answers `lambdamart_defaults` with, to the byte."""
    assert clib._take_str(clib._load().query_json(b"lambdamart_defaults")) == DEFAULTS_TEXT
    assert list(clib.query_json("lambdamart_defaults")["params"]["LambdaMART"].keys()) == KEYS


def test_keys_round_trip():
    req = TrainRequest.lambdamart()
    req.params.grower = "histogram"
    req.params.split_gain = "newton"
    req.params.lambda_l2, req.params.min_sum_hessian, req.params.min_split_gain = 1.0, 2.0 ** -6, 2.0 ** -20
    d = req.to_dict()
    wire = d["params"]["LambdaMART"]
    assert list(wire.keys()) == KEYS + ["grower", "split_gain"] + NUMBERS
    assert (wire["split_gain"], wire["lambda_l2"], wire["min_sum_hessian"], wire["min_split_gain"]) == ("newton", 1.0, 2.0 ** -6, 2.0 ** -20)
    back = TrainRequest.from_dict(json.loads(json.dumps(d)))
    assert back == req and back.params.split_gain == "newton" and back.params.min_split_gain == 2.0 ** -20
    c = req.clone()
    assert c == req and c.params is not req.params and c != TrainRequest.lambdamart()
    # only the keys that differ from their defaults are written
    req.params.min_sum_hessian = 0.0
    assert list(req.to_dict()["params"]["LambdaMART"].keys()) == KEYS + ["grower", "split_gain", "lambda_l2", "min_split_gain"]
    # an explicit "variance" on the wire reads back as the default
    d["params"]["LambdaMART"] = _params(split_gain="variance")
    assert TrainRequest.from_dict(d).params == LambdaMARTParams()


def test_native_parser_writes_the_keys_back():
    """The native side parses, validates and writes the keys: the per-tree sample hook parses a whole parameter object."""
    from fastrank_amd import native

    ok = LambdaMARTParams(grower="histogram", split_gain="newton", lambda_l2=0.5)
    native.lambdamart_sample(_dataset(), ok, 0)
    with pytest.raises(Exception, match="split_gain must be `variance` or `newton`"):
        native.lambdamart_sample(_dataset(), LambdaMARTParams(grower="histogram", split_gain="gain"), 0)


# --- errors ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("value", ["Newton", "gain", "", "hessian"])
def test_bad_split_gain_value_is_rejected(value):
    for msg in _both("invalid value", grower="histogram", split_gain=value):
        assert "split_gain must be `variance` or `newton`, not `%s`" % value in msg


@pytest.mark.parametrize("value", [1, None, True, ["newton"], {"newton": []}])
def test_bad_split_gain_type_is_rejected(value):
    for msg in _both("invalid type", grower="histogram", split_gain=value):
        assert "expected a string for split_gain" in msg


@pytest.mark.parametrize("grower", [None, "exact"])
def test_newton_needs_the_histogram_grower(grower):
    kw = dict(split_gain="newton") if grower is None else dict(split_gain="newton", grower=grower)
    for msg in _both("invalid value", **kw):
        assert "needs grower: \\\"histogram\\\"" in msg or 'needs grower: "histogram"' in msg


@pytest.mark.parametrize("key", NUMBERS)
@pytest.mark.parametrize("value", [-1.0, -1e-300, -0.5])
def test_negative_number_is_rejected(key, value):
    for msg in _both("invalid value", grower="histogram", split_gain="newton", **{key: value}):
        assert key + " must be finite and at least 0" in msg


@pytest.mark.parametrize("key", NUMBERS)
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
def test_number_not_finite_is_rejected(key, value):
    """JSON has no spelling for NaN or an infinity: Python writes NaN / Infinity, which the request parser refuses for any
    key; a literal f64 cannot hold is `number out of range`.  No non-finite value reaches the range check."""
    _both("Error", grower="histogram", split_gain="newton", **{key: value})
    text = json.dumps({"measure": "ndcg", "params": {"LambdaMART": _params(grower="histogram", split_gain="newton", **{key: 12345.5})},
                       "judgments": None}).replace("12345.5", "1e999")
    with pytest.raises(Exception, match="number out of range"):
        clib._unwrap(clib._load().train_model(text.encode(), _dataset().pointer))


@pytest.mark.parametrize("key", NUMBERS)
@pytest.mark.parametrize("value", ["1", None, True, [1.0]])
def test_number_of_another_type_is_rejected(key, value):
    for msg in _both("invalid type", grower="histogram", split_gain="newton", **{key: value}):
        assert "expected f64 for " + key in msg


@pytest.mark.parametrize("key", NUMBERS)
@pytest.mark.parametrize("others", [dict(), dict(grower="histogram"), dict(grower="histogram", split_gain="variance")])
def test_a_number_without_newton_is_rejected(key, others):
    for msg in _both("invalid value", **dict(others, **{key: 0.5})):
        assert key + " needs split_gain: " in msg and "newton" in msg


@pytest.mark.parametrize("params", [dict(grower="histogram", split_gain="newton", lambda_l2=1.0, min_sum_hessian=0.25, min_split_gain=1e-6),
                                    dict(grower="histogram", split_gain="newton"), dict(split_gain="variance"),
                                    dict(grower="histogram", split_gain="variance", lambda_l2=0.0)])
def test_accepted_requests_reach_the_later_checks(params):
    """Valid keys pass the parser: the request then fails on what is checked after the parameters (the measure)."""
    with pytest.raises(Exception, match=r"supported: ndcg, ndcg@k"):
        _train_raw(_params(**params), "map")
    with pytest.raises(Exception, match="num_trees must be at least 1"):
        _train_raw(_params(num_trees=0, **params))


@pytest.mark.parametrize("key", NUMBERS)
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf"), -1.0])
def test_debug_hook_rejects_a_number_that_is_not_finite_or_negative(key, value):
    """The one entry point a non-finite number can reach as a double: fr_debug_hist_tree's options refuse it before it looks at
    the dataset."""
    from fastrank_amd import native

    lam = np.ones(8)
    with pytest.raises(Exception, match="lambda_l2, min_sum_hessian and min_split_gain must be finite and at least 0"):
        native.hist_tree(_dataset(), lam, lam, 4, 2, 1, split_gain="newton", **{key: value})


def test_hist_tree_rejects_bad_arguments_before_any_call():
    from fastrank_amd import native

    lam = np.zeros(8)
    with pytest.raises(ValueError, match="split_gain"):
        native.hist_tree(_dataset(), lam, lam, 4, 2, 1, split_gain="gain")
    with pytest.raises(ValueError, match="need split_gain='newton'"):
        native.hist_tree(_dataset(), lam, lam, 4, 2, 1, lambda_l2=1.0)


# --- the restatement's own properties ---------------------------------------------------------------

def _case(seed, n=3000, d=6, q=30):
    X, y, qid = synth_dataset(seed, n, d, q)
    rng = np.random.default_rng(seed)
    lam = rng.normal(0.0, 1.0, n) + 0.5 * (y - y.mean())
    wt = rng.random(n)
    return X, lam, wt, np.arange(n)


@pytest.mark.parametrize("k,depth,min_leaf", [(2, 3, 1), (16, 6, 1), (64, 8, 5), (256, 5, 25)])
def test_equal_hessians_give_the_variance_tree(k, depth, min_leaf):
    """w = 0.25 everywhere and lambda_l2 = 0: H is a power of two times the count, term the variance term scaled exactly, so
    argmax, tie order and leaf values are those of the variance restatement, byte for byte."""
    X, lam, _, ids = _case(k)
    wt = np.full(len(lam), 0.25)
    feats = range(X.shape[1])
    a = nm.fit_tree(X, lam, wt, ids, feats, depth, min_leaf, k)
    b = hm.fit_tree(X, lam, wt, ids, feats, depth, min_leaf, k)
    assert json.dumps(a) == json.dumps(b)
    assert "FeatureSplit" in a


def _exact_terms(q, w, S, Sw, l2):
    return Fraction(int(q), 1) ** 2 / Fraction(2) ** (2 * S) / (Fraction(int(w), 1) / Fraction(2) ** Sw + Fraction(l2))


@pytest.mark.parametrize("seed", range(12))
def test_choice_against_exact_arithmetic(seed):
    """Every valid candidate's importance recomputed in fractions.Fraction from the integer sums: the restatement's choice
    is valid by the exact rules and within a relative 2^-48 of the exact maximum (seven roundings of 2^-53 each per
    importance -- two conversions, a square, a sum and a quotient per side, counted with the square's doubling, and the
    final sum -- with slack)."""
    rng = np.random.default_rng(1000 + seed)
    n, d, k = int(rng.integers(20, 201)), int(rng.integers(1, 6)), int(rng.integers(2, 9))
    X = rng.integers(0, 12, (n, d)).astype(np.float32) if seed % 2 else rng.normal(0, 1, (n, d)).astype(np.float32)
    lam = rng.normal(0, 1, n) * np.exp(rng.normal(0, 2, n))
    wt = rng.random(n) * (rng.random(n) < 0.8)
    l2 = [0.0, 2.0 ** -10, 1.0, 0.3][seed % 4]
    min_hess = [0.0, 0.5, 2.0][seed % 3]
    min_leaf = [1, 3][seed % 2]
    ids = np.arange(n)
    edges, xbin = hm.bin_matrix(X, ids, list(range(d)), k)
    Q, S, W, Sw = nm.quantise_pair(lam, wt, n)
    best, node = nm.best_split(xbin, edges, Q, W, ids, min_leaf, S, Sw, l2, min_hess)
    cands, _ = nm.candidates(xbin, edges, Q, W, ids, min_leaf, S, Sw, l2, min_hess)
    fl2, fmh = Fraction(l2), Fraction(min_hess)
    exact = {}
    for slot, nL, qL, wL, ok, imp in cands:
        for j in range(len(nL)):
            nl, nr = int(nL[j]), n - int(nL[j])
            hl, hr = Fraction(int(wL[j])) / Fraction(2) ** Sw, Fraction(node[2] - int(wL[j])) / Fraction(2) ** Sw
            if nl > 0 and nr > 0 and nl >= min_leaf and nr >= min_leaf and hl >= fmh and hr >= fmh and hl + fl2 > 0 and hr + fl2 > 0:
                exact[(slot, j)] = _exact_terms(qL[j], wL[j], S, Sw, l2) + _exact_terms(node[1] - int(qL[j]), node[2] - int(wL[j]), S, Sw, l2)
    if best is None:
        assert not exact
        return
    assert (best[1], best[2]) in exact, "the chosen candidate is not valid by the exact rules"
    top = max(exact.values())
    assert exact[(best[1], best[2])] >= top * (1 - Fraction(1, 2 ** 48))
    assert abs(Fraction(best[0]) - exact[(best[1], best[2])]) <= top * Fraction(1, 2 ** 48)


def _leaves(node):
    if "LeafNode" in node:
        return [node["LeafNode"]]
    return _leaves(node["FeatureSplit"]["lhs"]) + _leaves(node["FeatureSplit"]["rhs"])


def test_lambda_l2_shrinks_every_leaf_of_a_fixed_structure():
    X, lam, wt, ids = _case(3)
    k = 16
    edges, xbin = hm.bin_matrix(X, ids, list(range(X.shape[1])), k)
    Q, S, W, Sw = nm.quantise_pair(lam, wt, len(ids))
    # a fixed partition: the bins of feature 0 crossed with those of feature 1
    cell = xbin[0].astype(np.int64) * 256 + xbin[1]
    sums = [(int(Q[cell == c].sum()), int(W[cell == c].sum())) for c in np.unique(cell)]
    prev = None
    for l2 in [0.0, 2.0 ** -10, 0.01, 0.5, 1.0, 7.0, 1e6]:
        vals = np.array([nm.leaf_value(q, w, S, Sw, l2) for q, w in sums])
        if prev is not None:
            assert np.all(np.abs(vals) <= np.abs(prev)) and np.all(np.sign(vals) * np.sign(prev) >= 0)
        prev = vals
    # with lambda_l2 = 0 a leaf is the variance grower's
    assert [nm.leaf_value(q, w, S, Sw, 0.0) for q, w in sums] == [math.ldexp(float(q), -S) / math.ldexp(float(w), -Sw) for q, w in sums]
    # ... and the depth-1 tree is that leaf
    assert nm.fit_tree(X, lam, wt, ids, range(X.shape[1]), 1, 1, k, lambda_l2=1.0) == {
        "LeafNode": nm.leaf_value(int(Q.sum()), int(W.sum()), S, Sw, 1.0)}


def test_min_sum_hessian_and_min_split_gain_stop_the_root():
    X, lam, wt, ids = _case(4)
    k, feats = 16, list(range(X.shape[1]))
    binned = hm.bin_matrix(X, ids, feats, k)
    Q, S, W, Sw = nm.quantise_pair(lam, wt, len(ids))
    l2 = 0.5
    root_h = float(nm.hess(int(W.sum()), Sw))
    one = nm.fit_tree(X, lam, wt, ids, feats, 6, 1, k, binned, lambda_l2=l2, min_sum_hessian=root_h * 1.001)
    assert one == {"LeafNode": nm.leaf_value(int(Q.sum()), int(W.sum()), S, Sw, l2)}
    assert "FeatureSplit" in nm.fit_tree(X, lam, wt, ids, feats, 6, 1, k, binned, lambda_l2=l2, min_sum_hessian=root_h / 4)
    best, node = nm.best_split(binned[1], binned[0], Q, W, ids, 1, S, Sw, l2, 0.0)
    gain = float(np.float64(best[0]) - nm.term(node[1], node[2], S, Sw, l2))
    assert gain > 0.0
    assert nm.fit_tree(X, lam, wt, ids, feats, 6, 1, k, binned, lambda_l2=l2, min_split_gain=gain) == one  # (strict)
    assert nm.fit_tree(X, lam, wt, ids, feats, 6, 1, k, binned, lambda_l2=l2, min_split_gain=gain * 1.5) == one
    below = nm.fit_tree(X, lam, wt, ids, feats, 6, 1, k, binned, lambda_l2=l2, min_split_gain=float(np.nextafter(gain, 0.0)))
    assert "FeatureSplit" in below
    # the floor applies at every node: fewer leaves than without it, never more
    free = nm.fit_tree(X, lam, wt, ids, feats, 6, 1, k, binned, lambda_l2=l2)
    some = nm.fit_tree(X, lam, wt, ids, feats, 6, 1, k, binned, lambda_l2=l2, min_split_gain=gain / 50)
    assert 1 < len(_leaves(some)) < len(_leaves(free))


def test_zero_gradients_and_zero_hessians():
    X, lam, wt, ids = _case(6)
    feats = range(X.shape[1])
    assert nm.fit_tree(X, np.zeros(len(lam)), wt, ids, feats, 5, 1, 16, lambda_l2=1.0) == {"LeafNode": 0.0}
    # all-zero w: no candidate has H + 0 > 0, a single leaf of 0.0; with an L2 term the tree grows on G alone
    assert nm.fit_tree(X, lam, np.zeros(len(lam)), ids, feats, 5, 1, 16) == {"LeafNode": 0.0}
    assert "FeatureSplit" in nm.fit_tree(X, lam, np.zeros(len(lam)), ids, feats, 5, 1, 16, lambda_l2=1.0)
    # G * G underflows to 0 for every candidate: the gain is 0, which is not above min_split_gain = 0
    tiny = nm.fit_tree(X, lam * 1e-300, wt, ids, feats, 5, 1, 16)
    assert list(tiny.keys()) == ["LeafNode"] and tiny["LeafNode"] != 0.0
