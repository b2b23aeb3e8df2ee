"""Monotone constraints of LambdaMART's histogram grower without a GPU: the wire key `monotone_constraints` and its validation
(every request here fails or is only parsed before any device work), and self-checks of the numpy restatement
(tests/lambdamart_monotone_model.py) that the GPU tests hold the device to: the trees it grows are monotone, and where no
bound binds they are the plain Newton grower's."""
import itertools
import json
from fractions import Fraction

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import clib
from fastrank_amd.training import LambdaMARTParams, TrainRequest
from tests import lambdamart_hist_model as hm
from tests import lambdamart_leafwise_model as lw
from tests import lambdamart_monotone_model as mm
from tests import lambdamart_newton_model as nm

KEYS = ["num_trees", "learning_rate", "max_depth", "min_leaf_support", "split_candidates", "sigma", "quiet"]
HIST = dict(grower="histogram", split_gain="newton")


def _dataset():
    X = np.arange(24, dtype=np.float32).reshape(8, 3)
    y = np.array([0, 1, 2, 0, 1, 0, 0, 1], dtype=np.float64)
    qid = np.array([1, 1, 1, 1, 2, 2, 2, 2], dtype=np.int64)
    return fr.CDataset.from_numpy(X, y, qid)


def _train_raw(params, measure="ndcg"):
    text = json.dumps({"measure": measure, "params": {"LambdaMART": params}, "judgments": None}).encode()
    dataset = _dataset()  # (kept alive over the call: the feature names are looked up in it)
    return clib._unwrap(clib._load().train_model(text, dataset.pointer))


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
    out = []
    for call in (lambda: _train_raw(_params(**kw)), lambda: _train_python(**kw)):
        with pytest.raises(Exception, match=match) as e:
            call()
        out.append(str(e.value))
    return out


# --- wire form ---------------------------------------------------------------------------------------

def test_key_is_absent_at_its_default():
    assert LambdaMARTParams().monotone_constraints == {}
    assert list(LambdaMARTParams().to_dict().keys()) == KEYS
    assert list(LambdaMARTParams(monotone_constraints={}).to_dict().keys()) == KEYS
    assert list(TrainRequest.lambdamart().to_dict()["params"]["LambdaMART"].keys()) == KEYS
    assert list(clib.query_json("lambdamart_defaults")["params"]["LambdaMART"].keys()) == KEYS


def test_key_comes_after_every_other_key():
    p = LambdaMARTParams(grower="histogram", query_sampling_rate=0.5, feature_sampling_rate=0.5, seed=3, validation_queries=["2"],
                         early_stopping_rounds=2, split_gain="newton", lambda_l2=1.0, min_sum_hessian=0.5, min_split_gain=0.25,
                         max_leaves=7, truncation_level=5, lambda_norm=True, objective="map", monotone_constraints={"1": -1})
    keys = list(p.to_dict().keys())
    assert keys[:len(KEYS)] == KEYS and keys[-1] == "monotone_constraints" and len(keys) == len(KEYS) + 15
    q = LambdaMARTParams(drop_rate=0.25, max_drop=3, skip_drop=0.25, monotone_constraints={"0": 1}, **HIST)
    assert list(q.to_dict().keys()) == KEYS + ["grower", "split_gain", "drop_rate", "max_drop", "skip_drop", "monotone_constraints"]


def test_key_round_trips_and_zero_entries_are_dropped():
    req = TrainRequest.lambdamart()
    req.params.grower, req.params.split_gain = "histogram", "newton"
    req.params.monotone_constraints = {"2": 1, "0": -1}
    d = req.to_dict()
    wire = d["params"]["LambdaMART"]
    assert list(wire.keys()) == KEYS + ["grower", "split_gain", "monotone_constraints"]
    assert wire["monotone_constraints"] == {"2": 1, "0": -1} and list(wire["monotone_constraints"]) == ["2", "0"]
    back = TrainRequest.from_dict(json.loads(json.dumps(d)))
    assert back == req and back.params.monotone_constraints == {"2": 1, "0": -1}
    assert req.clone() == req and req.clone() != TrainRequest.lambdamart()
    req.params.monotone_constraints = {"2": 1, "1": 0, "0": -1}
    assert req.to_dict() == d and req.clone() == back
    req.params.monotone_constraints = {"1": 0, "2": 0}  # only zero entries: the default wire form
    assert list(req.to_dict()["params"]["LambdaMART"].keys()) == KEYS + ["grower", "split_gain"]
    assert list(LambdaMARTParams(monotone_constraints={"1": 0}).to_dict().keys()) == KEYS


def test_native_parser_accepts_writes_and_refuses_the_key():
    """The native side parses and validates the key wherever it parses a whole parameter object: the per-tree sample hook."""
    from fastrank_amd import native

    native.lambdamart_sample(_dataset(), LambdaMARTParams(monotone_constraints={"0": 1, "2": -1, "1": 0}, **HIST), 0)
    native.lambdamart_sample(_dataset(), LambdaMARTParams(monotone_constraints={"1": 0}), 0)  # zero entries need nothing
    with pytest.raises(Exception, match="to -1, 0 or 1"):
        native.lambdamart_sample(_dataset(), LambdaMARTParams(monotone_constraints={"0": 2}, **HIST), 0)


# --- errors ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("value", ["1", None, True, [1], 1.5, 3])
def test_a_value_that_is_not_an_object_is_rejected(value):
    for msg in _both("invalid type", monotone_constraints=value, **HIST):
        assert "expected an object from feature name to -1, 0 or 1 for monotone_constraints" in msg


@pytest.mark.parametrize("value", ["1", None, True, [1], 1.0, 0.5, {"a": 1}])
def test_an_entry_that_is_not_an_integer_is_rejected(value):
    for msg in _both("invalid type", monotone_constraints={"0": value}, **HIST):
        assert "expected an integer for every entry of monotone_constraints" in msg


@pytest.mark.parametrize("value", [2, -2, 100, -2 ** 40, 2 ** 63])
def test_an_entry_outside_the_three_signs_is_rejected(value):
    for msg in _both("invalid value", monotone_constraints={"1": 1, "0": value}, **HIST):
        assert "monotone_constraints must map feature `0` to -1, 0 or 1" in msg


@pytest.mark.parametrize("grower", [None, "exact"])
@pytest.mark.parametrize("sign", [1, -1])
def test_a_constraint_needs_the_histogram_grower(grower, sign):
    kw = dict(monotone_constraints={"0": sign})
    if grower is not None:
        kw["grower"] = grower
    for msg in _both("invalid value", **kw):
        assert "monotone_constraints needs grower: \\\"histogram\\\"" in msg or 'monotone_constraints needs grower: "histogram"' in msg


@pytest.mark.parametrize("gain", [None, "variance"])
@pytest.mark.parametrize("others", [dict(), dict(max_leaves=8)])
def test_a_constraint_needs_the_newton_gain(gain, others):
    kw = dict(grower="histogram", monotone_constraints={"2": -1, "0": 0}, **others)
    if gain is not None:
        kw["split_gain"] = gain
    for msg in _both("invalid value", **kw):
        assert "monotone_constraints needs split_gain: \\\"newton\\\"" in msg or 'monotone_constraints needs split_gain: "newton"' in msg


@pytest.mark.parametrize("params", [dict(monotone_constraints={"0": 0}), dict(grower="exact", monotone_constraints={"0": 0, "9": 0}),
                                    dict(grower="histogram", monotone_constraints={}),
                                    dict(monotone_constraints={"0": 1, "1": -1, "2": 0}, **HIST),
                                    dict(monotone_constraints={"2": -1}, max_leaves=4, drop_rate=0.5, feature_sampling_rate=0.5, **HIST)])
def test_accepted_requests_reach_the_later_checks(params):
    """Valid keys pass the parser (zero entries ask for nothing, under any grower): the request then fails on what is checked
    after the parameters (the measure)."""
    with pytest.raises(Exception, match=r"supported: ndcg, ndcg@k"):
        _train_raw(_params(**params), "map")


@pytest.mark.parametrize("name", ["3", "bm25", " 0", ""])
def test_a_view_without_the_feature_is_refused(name):
    for msg in _both("invalid value", monotone_constraints={"1": 1, name: -1}, **HIST):
        assert "monotone_constraints names `%s`, which is not a feature of the dataset" % name in msg


def test_hist_tree_rejects_constraints_without_the_newton_gain_before_any_call():
    from fastrank_amd import native

    lam = np.zeros(8)
    with pytest.raises(ValueError, match="need split_gain='newton'"):
        native.hist_tree(_dataset(), lam, lam, 4, 2, 1, monotone={0: 1})
    with pytest.raises(ValueError, match="max_leaves"):
        native.hist_tree(_dataset(), lam, lam, 4, 2, 1, split_gain="newton", max_leaves=1, monotone={0: 1})


# --- the restatement: every tree is monotone ---------------------------------------------------------

N, F, K = 1200, 5, 32


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(17)
    X = rng.normal(0.0, 1.0, (N, F)).astype(np.float32)
    X[:, 1] = np.round(X[:, 1] * 3.0) / 3.0  # few distinct values
    # gradients that rise and fall along every feature: each sign of a constraint has something to forbid
    lam = np.sin(2.5 * X[:, 0]) - np.cos(2.0 * X[:, 1]) + np.cos(2.5 * X[:, 2]) + np.sin(3.0 * X[:, 3]) + rng.normal(0.0, 0.5, N)
    wt = rng.random(N) + 0.05
    ids = np.arange(N)
    return X, lam, wt, ids, hm.bin_matrix(X, ids, list(range(F)), K)


GROWTH = [dict(max_leaves=0, depth=7), dict(max_leaves=24, depth=12)]


def _fit(case, monotone, growth, min_leaf=3, l2=2.0 ** -10):
    X, lam, wt, ids, binned = case
    return mm.fit_tree(X, lam, wt, ids, range(F), growth["depth"], min_leaf, K, monotone, growth["max_leaves"], binned, lambda_l2=l2)


def _plain(case, growth, min_leaf=3, l2=2.0 ** -10):
    X, lam, wt, ids, binned = case
    if growth["max_leaves"]:
        return lw.fit_tree(X, lam, wt, ids, range(F), growth["depth"], min_leaf, K, growth["max_leaves"], binned, split_gain="newton", lambda_l2=l2)
    return nm.fit_tree(X, lam, wt, ids, range(F), growth["depth"], min_leaf, K, binned, lambda_l2=l2)


def _violations(case, tree, fid, sign, rows=300):
    X, binned = case[0], case[4]
    grid = mm.probe_grid(binned[0][fid])  # every edge of the feature, its neighbours of one ulp, and the extremes
    return mm.violations(lambda P: mm.predict(tree, P), X[:rows], fid, grid, sign)


@pytest.mark.parametrize("growth", GROWTH)
@pytest.mark.parametrize("pair", [(0, 3), (1, 2)])
def test_every_tree_is_monotone_along_every_constrained_feature(case, growth, pair):
    bound = 0
    for signs in itertools.product((-1, 0, 1), repeat=2):
        if signs == (0, 0):
            continue
        monotone = dict(zip(pair, signs))
        tree, clamped = _fit(case, monotone, growth)
        assert "FeatureSplit" in tree
        for fid, sign in monotone.items():
            if sign != 0:
                assert _violations(case, tree, fid, sign) == 0, "signs %r, feature %d" % (monotone, fid)
        bound += clamped
    assert bound > 0  # (some bound moved some leaf: the clamp was exercised)
    # the property is not vacuous: the plain tree breaks it along these features in both directions
    plain = _plain(case, growth)
    for fid in pair:
        assert _violations(case, plain, fid, 1) > 0 and _violations(case, plain, fid, -1) > 0


@pytest.mark.parametrize("growth", GROWTH)
def test_no_constraint_gives_the_plain_newton_tree(case, growth):
    """Nothing clamps under (-inf, +inf): the two-case term is Newton's bit for bit, with signs of 0 or none at all."""
    plain = _plain(case, growth)
    for monotone in (dict(), {0: 0, 3: 0}):
        assert _fit(case, monotone, growth) == (plain, 0)


@pytest.mark.parametrize("growth", GROWTH)
@pytest.mark.parametrize("sign", [1, -1])
def test_constraints_on_a_constant_column_alone_give_the_plain_newton_tree(growth, sign):
    rng = np.random.default_rng(23)
    X = rng.normal(0.0, 1.0, (800, 4)).astype(np.float32)
    X[:, 2] = 2.5
    lam, wt, ids = rng.normal(0.0, 1.0, 800) + X[:, 0], rng.random(800), np.arange(800)
    binned = hm.bin_matrix(X, ids, list(range(4)), 16)
    assert len(binned[0][2]) == 0  # no edge: never split on, so no interval is ever cut
    for l2 in (0.0, 2.0 ** -10, 1.0):
        got = mm.fit_tree(X, lam, wt, ids, range(4), growth["depth"], 2, 16, {2: sign}, growth["max_leaves"], binned, lambda_l2=l2)
        if growth["max_leaves"]:
            exp = lw.fit_tree(X, lam, wt, ids, range(4), growth["depth"], 2, 16, growth["max_leaves"], binned, split_gain="newton", lambda_l2=l2)
        else:
            exp = nm.fit_tree(X, lam, wt, ids, range(4), growth["depth"], 2, 16, binned, lambda_l2=l2)
        assert got == (exp, 0) and "FeatureSplit" in exp


def test_the_clamped_term_never_exceeds_the_newton_term():
    """In exact arithmetic 2 G v - (H + l) v^2 <= G^2 / (H + l), with equality only at v = G / (H + l): the clamped term has the
    Newton term's sign and scale, so importances of clamped and unclamped candidates compare."""
    rng = np.random.default_rng(5)
    for _ in range(300):
        G = Fraction(int(rng.integers(-10 ** 6, 10 ** 6)), int(rng.integers(1, 10 ** 4)))
        D = Fraction(int(rng.integers(1, 10 ** 6)), int(rng.integers(1, 10 ** 4)))  # H + lambda_l2 > 0
        best = G / D
        assert 2 * G * best - D * best * best == G * G / D
        for v in (Fraction(int(rng.integers(-10 ** 6, 10 ** 6)), int(rng.integers(1, 10 ** 4))), best + Fraction(1, 10 ** 12), best - Fraction(1, 10 ** 12)):
            if v != best:
                assert 2 * G * v - D * v * v < G * G / D
    # and the restatement's f64 term is that expression: at an interval that clamps, and at one that does not
    S, Sw, l2 = 20, 18, 0.5
    for q, w, lo, hi in ((3 << 20, 5 << 18, -1.0, 0.25), (3 << 20, 5 << 18, 1.0, 2.0), (-(7 << 19), 1 << 18, -1.0, 1.0)):
        t, v = mm.term(q, w, S, Sw, l2, lo, hi)
        G, D = Fraction(q, 1 << S), Fraction(w, 1 << Sw) + Fraction(l2)
        out = G / D
        assert Fraction(float(v)) == min(max(out, Fraction(lo)), Fraction(hi)) and Fraction(float(v)) != out
        assert Fraction(float(t)) == 2 * G * Fraction(float(v)) - D * Fraction(float(v)) ** 2  # (dyadic numbers: no rounding)
    t, v = mm.term(3 << 20, 5 << 18, S, Sw, l2, -1.0, 1.0)
    assert float(v) == 3.0 / 5.5 and float(t) == float(nm.term(3 << 20, 5 << 18, S, Sw, l2))


def test_clamped_leaves_are_counted(case):
    for growth in GROWTH:
        tree, clamped = _fit(case, {0: 1, 3: -1}, growth)
        assert 0 < clamped <= lw.n_leaves(tree) and tree != _plain(case, growth)
