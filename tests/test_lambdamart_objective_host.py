"""LambdaMART's MAP and MRR objectives on the CPU ("Objectives"): the key's wire form and errors, the
restatement's pair weights (tests/lambdamart_objective_model.py) against exact rationals and against the evaluator, and the
gradients' sign and scale.  The bound of the evaluator comparison is derived in tests/lambdamart_objective_bound.py.
"""
import json
from fractions import Fraction

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import clib, native
from fastrank_amd.training import LambdaMARTParams, TrainRequest
from oracle import pyoracle as o
from tests import lambdamart_objective_bound as ob
from tests import lambdamart_objective_model as om

KEYS = ["num_trees", "learning_rate", "max_depth", "min_leaf_support", "split_candidates", "sigma", "quiet"]


def _dataset():
    X = np.arange(24, dtype=np.float32).reshape(8, 3)
    y = np.array([0, 1, 2, 0, 1, 0, 0, 1], dtype=np.float64)
    qid = np.array([1, 1, 1, 1, 2, 2, 2, 2], dtype=np.int64)
    return fr.CDataset.from_numpy(X, y, qid)


def _params(**kw):
    p = LambdaMARTParams().to_dict()
    p.update(kw)
    return p


def _train_raw(params, measure="ndcg"):
    text = json.dumps({"measure": measure, "params": {"LambdaMART": params}, "judgments": None}).encode()
    return clib._unwrap(clib._load().train_model(text, _dataset().pointer))


def _train_python(**kw):
    req = TrainRequest.lambdamart()
    req.params.quiet = True
    for k, v in kw.items():
        setattr(req.params, k, v)
    return _dataset().train_model(req)


# --- wire form ---------------------------------------------------------------------------------------

def test_the_key_is_absent_at_its_default():
    p = LambdaMARTParams()
    assert p.objective == "ndcg"
    assert list(p.to_dict().keys()) == KEYS
    assert list(LambdaMARTParams(objective="ndcg").to_dict().keys()) == KEYS
    assert list(TrainRequest.lambdamart().to_dict()["params"]["LambdaMART"].keys()) == KEYS
    assert list(clib.query_json("lambdamart_defaults")["params"]["LambdaMART"].keys()) == KEYS


@pytest.mark.parametrize("spelling,stored", [("map", "map"), ("ap", "map"), ("mrr", "mrr"), ("rr", "mrr")])
def test_the_key_round_trips(spelling, stored):
    req = TrainRequest.lambdamart()
    req.params = LambdaMARTParams(objective=spelling)
    d = req.to_dict()
    wire = d["params"]["LambdaMART"]
    assert list(wire.keys()) == KEYS + ["objective"] and wire["objective"] == stored
    back = TrainRequest.from_dict(json.loads(json.dumps(d)))
    assert back == req and back.params.objective == stored
    assert req.clone() == req and req.clone() != TrainRequest.lambdamart()
    d["params"]["LambdaMART"] = _params(objective="ndcg")  # the explicit default reads back as the default
    assert TrainRequest.from_dict(d).params == LambdaMARTParams()


@pytest.mark.parametrize("spelling,stored", [("map", "map"), ("ap", "map"), ("mrr", "mrr"), ("rr", "mrr"), ("ndcg", None)])
def test_the_native_parser_accepts_every_spelling(spelling, stored):
    """The per-tree sample hook parses the variant's payload with LambdaMARTParams::from_json, and a training request is
    refused for its measure only AFTER its parameters were accepted.  (What the parser stored is seen on the device: the
    training stats report the canonical spelling.)"""
    native.lambdamart_sample(_dataset(), _params(objective=spelling), 0)
    with pytest.raises(Exception, match=r"supported: ndcg, ndcg@k"):
        _train_raw(_params(objective=spelling), "map")


@pytest.mark.parametrize("extra", [dict(), dict(grower="histogram"), dict(truncation_level=3, lambda_norm=True),
                                   dict(grower="histogram", split_gain="newton", lambda_l2=1.0, max_leaves=8, query_sampling_rate=0.5,
                                        validation_queries=["2"], truncation_level=30)])
@pytest.mark.parametrize("objective", ["map", "mrr"])
def test_measure_map_is_still_refused_with_the_key_set(objective, extra):
    for measure in ("map", "mrr", "ap", "rr", "map@10"):
        with pytest.raises(Exception, match=r"supported: ndcg, ndcg@k"):
            _train_raw(_params(objective=objective, **extra), measure)
    req = TrainRequest.lambdamart()
    req.measure = "map"
    req.params.objective = objective
    with pytest.raises(Exception, match=r"supported: ndcg, ndcg@k"):
        _dataset().train_model(req)


@pytest.mark.parametrize("value", ["NDCG", "MAP", "Mrr", "", "err", "ndcg@10", "map@5", "precision", " map"])
def test_an_unknown_objective_is_rejected(value):
    for call in (lambda: _train_raw(_params(objective=value)), lambda: _train_python(objective=value)):
        with pytest.raises(Exception, match="invalid value") as e:
            call()
        assert "objective must be `ndcg`, `map` or `mrr`, not `%s`" % value in str(e.value)
        assert "line: 0, column: 0" in str(e.value)


@pytest.mark.parametrize("value", [None, 1, True, ["map"], 2.5, {"name": "map"}])
def test_an_objective_that_is_not_a_string_is_rejected(value):
    for call in (lambda: _train_raw(_params(objective=value)), lambda: _train_python(objective=value)):
        with pytest.raises(Exception, match="invalid type") as e:
            call()
        assert "expected a string for objective" in str(e.value)


def _opts_call(options, measure="ndcg"):
    ds = _dataset()
    m = fr.CModel.from_dict({"Linear": {"weights": [0.0, 0.0, 1.0]}})
    out = np.zeros(8)
    native._status(native._load().fr_debug_lambda_gradients_opts(m.pointer, ds.pointer, None, measure.encode(), 1.0, None, 0,
                                                               json.dumps(options).encode(), out.ctypes.data, out.ctypes.data, 8))


@pytest.mark.parametrize("options,text", [({"objective": "MAP"}, "objective must be `ndcg`, `map` or `mrr`, not `MAP`"),
                                          ({"objective": 1}, "expected a string for objective"),
                                          ({"objective": "map", "lambda_norm": 1}, "expected a boolean for lambda_norm")])
def test_the_debug_entry_point_checks_the_objective_before_any_device_work(options, text):
    with pytest.raises(Exception) as e:
        _opts_call(options)
    assert text in str(e.value)
    for objective in ("map", "mrr", "ndcg"):  # the measure must name NDCG whatever the objective
        with pytest.raises(Exception, match=r"supported: ndcg, ndcg@k"):
            _opts_call({"objective": objective}, "map")
    m, ds = fr.CModel.from_dict({"Linear": {"weights": [0.0, 0.0, 1.0]}}), _dataset()
    with pytest.raises(Exception, match=r"supported: ndcg, ndcg@k"):
        native.lambda_gradients(m, ds, "map", objective="map")


def test_default_identity():
    """`"objective": "ndcg"` is the key absent: the same parameters, the same wire form, the same per-tree samples."""
    assert LambdaMARTParams(objective="ndcg") == LambdaMARTParams()
    assert LambdaMARTParams.from_dict(_params(objective="ndcg")).to_dict() == LambdaMARTParams().to_dict()
    kw = dict(query_sampling_rate=0.5, feature_sampling_rate=0.5, seed=7)
    for tree in (0, 3):
        a = native.lambdamart_sample(_dataset(), _params(**kw), tree)
        b = native.lambdamart_sample(_dataset(), _params(objective="ndcg", **kw), tree)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    for measure in ("map", "err@3"):  # ... and is refused for the same reasons
        errs = []
        for params in (_params(), _params(objective="ndcg")):
            with pytest.raises(Exception) as e:
                _train_raw(params, measure)
            errs.append(str(e.value))
        assert errs[0] == errs[1]


# --- delta -------------------------------------------------------------------------------------------

def _designed_lists():
    """(relevance flags by rank, norm) of designed lists: no / one / every relevant document, the first relevant one first
    and last, a judged count above the list's own."""
    out = []
    for flags in ([1], [0], [1, 0], [0, 1], [0, 0, 0, 0], [1, 1, 1, 1], [0, 0, 0, 1], [1, 0, 0, 0], [0, 1, 0, 0, 0], [0, 1, 1, 0, 1, 0],
                  [0, 0, 1, 0, 1, 1, 0, 0, 1], [1, 1, 0, 0, 1, 0, 1, 0, 0, 0, 1, 1, 0]):
        out.append((flags, 0))
        out.append((flags, sum(flags) + 3))
    return out


def _random_lists(seed, count):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        m = int(rng.integers(2, 14))
        flags = (rng.random(m) < rng.choice([0.15, 0.5, 0.8])).astype(int).tolist()
        out.append((flags, int(rng.choice([0, sum(flags), sum(flags) + 2]))))
    return out


def _scatter(flags, seed):
    """The list in a shuffled stored order: (rank, rel) by stored position."""
    rank = np.random.default_rng(seed).permutation(len(flags))
    return rank, np.asarray(flags, dtype=bool)[rank]


@pytest.mark.parametrize("objective", om.OBJECTIVES)
def test_delta_is_the_swap_difference_in_exact_rationals(objective):
    """The restatement's f64 table against |metric swapped - metric| in exact rationals, for every (relevant, non-relevant)
    pair of the designed and random lists, within the derived bound (whose closed-form part is what applies here; the
    evaluator's part only widens it)."""
    pairs = 0
    for k, (flags, norm) in enumerate(_designed_lists() + _random_lists(11, 320)):
        rank, rel = _scatter(flags, k)
        table = om.delta_table(rank, rel, float(norm), objective)
        live = any(flags) if objective == "mrr" else (norm or sum(flags)) != 0
        if not live:
            assert table is None
            continue
        m = len(flags)
        for i in range(m):
            for j in range(m):
                if rel[i] == rel[j]:
                    assert table[i, j] == 0.0
                    continue
                exact = ob.swap_delta(rank, rel, i, j, norm, objective)
                assert abs(Fraction(float(table[i, j])) - exact) <= ob.oracle_bound(rank, rel, i, j, norm, objective), (flags, norm, i, j)
                assert (table[i, j] == 0.0) == (exact == 0)
                assert table[i, j] == table[j, i]
                pairs += 1
    assert pairs > 6000


@pytest.mark.parametrize("objective", om.OBJECTIVES)
def test_the_closed_forms_are_exact_identities(objective):
    """The closed form itself, evaluated in rationals, against the swap: no tolerance at all."""
    for k, (flags, norm) in enumerate(_designed_lists() + _random_lists(5, 120)):
        m = len(flags)
        c = np.cumsum(flags)
        P = [sum((Fraction(1, r + 1) for r in range(x + 1) if flags[r]), Fraction(0)) for x in range(m)]
        rank, rel = np.arange(m), np.asarray(flags, dtype=bool)
        R = norm or int(sum(flags))
        rel_at = [r for r in range(m) if flags[r]]
        for rh in rel_at:
            for rl in range(m):
                if flags[rl]:
                    continue
                if objective == "map":
                    a, b, up = min(rh, rl), max(rh, rl), int(rl < rh)
                    closed = abs(Fraction(int(c[a]) + up, a + 1) - Fraction(int(c[b]), b + 1) + (P[b - 1] - P[a])) / R
                else:
                    f = rel_at[0]
                    f2 = rel_at[1] if len(rel_at) > 1 else None
                    if rl < f:
                        closed = Fraction(1, rl + 1) - Fraction(1, f + 1)
                    elif rh == f:
                        closed = Fraction(1, f + 1) - Fraction(1, (rl if f2 is None else min(f2, rl)) + 1)
                    else:
                        closed = Fraction(0)
                assert closed == ob.swap_delta(rank, rel, rh, rl, norm, objective), (flags, norm, rh, rl)


@pytest.mark.parametrize("objective", om.OBJECTIVES)
def test_delta_is_the_evaluators(objective):
    """The table against the C oracle's metric_from_scores with the two documents' places exchanged (scores = -rank, all
    different, so exchanging two scores exchanges exactly two places), within the derived bound."""
    lists = _designed_lists() + _random_lists(23, 40)
    lists = [(f, n) for f, n in lists if len(f) >= 2]
    worst = 0.0
    for k, (flags, norm) in enumerate(lists):
        rank, rel = _scatter(flags, 100 + k)
        m = len(flags)
        table = om.delta_table(rank, rel, float(norm), objective)
        if table is None:
            continue
        X = np.zeros((m, 1), dtype=np.float32)
        c = o.Dataset(X, rel.astype(np.float64), np.ones(m, dtype=np.int64))
        norms = np.array([float(norm)]) if objective == "map" else None
        scores = -rank.astype(np.float64)
        base = c.metric_from_scores(objective, scores, norms)[0][0]
        assert Fraction(float(base)) != 0 or not any(flags)
        for i in range(m):
            for j in range(i + 1, m):
                if rel[i] == rel[j]:
                    continue
                sw = scores.copy()
                sw[i], sw[j] = scores[j], scores[i]
                moved = c.metric_from_scores(objective, sw, norms)[0][0]
                err = abs(Fraction(float(table[i, j])) - abs(Fraction(float(moved)) - Fraction(float(base))))
                bound = ob.oracle_bound(rank, rel, i, j, norm, objective)
                assert err <= bound, (flags, norm, i, j, float(err), float(bound))
                worst = max(worst, float(err / bound))
    print("worst error / bound against the evaluator (%s): %.3f" % (objective, worst))
    if objective == "map":
        assert any(n > sum(f) for f, n in lists)  # a judged count above the list's own was among them


# --- sign and scale ------------------------------------------------------------------------------------

@pytest.mark.parametrize("objective", om.OBJECTIVES)
@pytest.mark.parametrize("sigma", [0.3, 1.0, 1.5])
def test_sign_and_scale(objective, sigma):
    """With delta frozen at the current ranks, lambda = -dC/ds and w = d2C/ds2 of C = sum over pairs of
    delta_hl log(1 + exp(-sigma (s_h - s_l))).  Central differences of C in long double, step h = 1e-4: the truncation
    error is at most h^2 sigma^3 D for the first and h^2 sigma^4 D for the second derivative (D = the document's summed
    delta; the logistic's derivatives are below 1), the rounding error about 4 eps C / h^2 <= 1e-7 C even where long double
    is double.  A wrong sign or a missing factor sigma is an error of order sigma D."""
    rng = np.random.default_rng(8)
    m = 12
    s = rng.normal(0.0, 1.0, m)
    y = rng.choice([0.0, 0.0, 1.0, 2.0], m)
    ids = [np.arange(m)]
    norms = [float((y > 0).sum())]
    lam, wt = om.gradients(s, y, ids, norms, objective, sigma)
    g = y.astype(np.float32)
    from tests import lambdamart_trunc_model as tm

    table = om.delta_table(tm.ranks(s, g, ids[0]), g > 0, norms[0], objective)
    rel = y > 0

    def cost(v):
        v = v.astype(np.longdouble)
        total = np.longdouble(0.0)
        for h in np.flatnonzero(rel):
            for l in np.flatnonzero(~rel):
                total += np.longdouble(table[h, l]) * np.log1p(np.exp(-np.longdouble(sigma) * (v[h] - v[l])))
        return total

    h = 1e-4
    assert np.any(lam != 0.0)
    for i in range(m):
        e = np.zeros(m)
        e[i] = h
        up, mid, down = cost(s + e), cost(s), cost(s - e)
        d1 = float((up - down) / (2 * h))
        d2 = float((up - 2 * mid + down) / (h * h))
        D = float(table[i].sum())
        tol = h * h * (sigma ** 3 + sigma ** 4) * D + 1e-7 * float(mid) + 1e-12
        assert abs(lam[i] + d1) <= tol and abs(wt[i] - d2) <= tol, (i, lam[i], -d1, wt[i], d2, tol)
        assert (lam[i] >= 0.0) == bool(rel[i]) or lam[i] == 0.0  # a relevant document is pushed up, the others down
        assert wt[i] >= 0.0
    assert abs(lam.sum()) <= 1e-12 * np.abs(lam).sum()  # every pair's two terms cancel
