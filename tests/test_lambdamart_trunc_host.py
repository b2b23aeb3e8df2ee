"""LambdaRank truncation level and per-query normalisation on the CPU ("Truncation and
normalisation"): the two keys' wire form and errors, the restatement's identities (tests/lambdamart_trunc_model.py), and
the restatement held to exact arithmetic (tests/lambdamart_exact.py restricted to the qualifying pairs).

The normalised values' bound (`_scaled_bound`), by the method of tests/lambdamart_bound.py (u = 2^-53, a library result
within K = 2 ulp = 4u relative, second-order terms under its SLACK):
  * A_p adds the same terms t_pq >= 0 as lambda_p adds with signs, so |A_p - exact| <= the lambda bound b_p of that document;
  * S = the A_p added one after the other: |S - exact| <= e_S = sum_p b_p + gamma_n S;
  * f = fl(fl(log2(fl(1 + S))) / S): x = 1 + S carries e_S / x + u relative, log2(x) that divided by ln(x) plus 4u, the
    division by S adds e_S / S + u:  e_f = (e_S / (1 + S) + u) / ln(1 + S) + e_S / S + 5u;
  * lambda_p f: |. - exact| <= f b_p + |lambda_p| f (e_f + u), and the same for w_p with its own bound.
"""
import decimal
import json
from decimal import Decimal

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import clib, native
from fastrank_amd.training import LambdaMARTParams, TrainRequest
from oracle import pyoracle as o
from tests import lambdamart_exact as ex
from tests import lambdamart_model as lm
from tests import lambdamart_trunc_model as tm
from tests.lambdamart_bound import C, MEASURES, SLACK, U, WEIGHTS, as_dataset, designed_queries, gradient_bound, random_queries, worst_ratio

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


def _both(match, **kw):
    out = []
    for call in (lambda: _train_raw(_params(**kw)), lambda: _train_python(**kw)):
        with pytest.raises(Exception, match=match) as e:
            call()
        out.append(str(e.value))
    return out


# --- wire form ---------------------------------------------------------------------------------------

def test_keys_are_absent_at_their_defaults():
    p = LambdaMARTParams()
    assert p.truncation_level == 0 and p.lambda_norm is False
    assert list(p.to_dict().keys()) == KEYS
    assert list(LambdaMARTParams(truncation_level=0, lambda_norm=False).to_dict().keys()) == KEYS
    assert list(TrainRequest.lambdamart().to_dict()["params"]["LambdaMART"].keys()) == KEYS
    assert list(clib.query_json("lambdamart_defaults")["params"]["LambdaMART"].keys()) == KEYS


def test_keys_round_trip():
    req = TrainRequest.lambdamart()
    req.params.truncation_level = 30
    req.params.lambda_norm = True
    d = req.to_dict()
    wire = d["params"]["LambdaMART"]
    assert list(wire.keys()) == KEYS + ["truncation_level", "lambda_norm"] and wire["truncation_level"] == 30 and wire["lambda_norm"] is True
    back = TrainRequest.from_dict(json.loads(json.dumps(d)))
    assert back == req and back.params.truncation_level == 30 and back.params.lambda_norm is True
    assert req.clone() == req and req.clone() != TrainRequest.lambdamart()
    only_norm = LambdaMARTParams(lambda_norm=True).to_dict()
    assert list(only_norm.keys()) == KEYS + ["lambda_norm"]
    d["params"]["LambdaMART"] = _params(truncation_level=0, lambda_norm=False)  # explicit defaults read back as the defaults
    assert TrainRequest.from_dict(d).params == LambdaMARTParams()


@pytest.mark.parametrize("params", [dict(truncation_level=1), dict(truncation_level=2 ** 32 - 1, lambda_norm=True), dict(lambda_norm=True),
                                    dict(truncation_level=0, lambda_norm=False), dict(grower="histogram", truncation_level=30, lambda_norm=True),
                                    dict(grower="histogram", truncation_level=30, split_gain="newton", lambda_l2=1.0, max_leaves=8,
                                         query_sampling_rate=0.5, validation_queries=["2"])])
def test_accepted_requests_reach_the_later_checks(params):
    """Valid keys, on both growers and next to every other optional group, pass the native parser: the request then fails on
    what is checked after the parameters (the measure), and the per-tree sample hook parses the same object."""
    with pytest.raises(Exception, match=r"supported: ndcg, ndcg@k"):
        _train_raw(_params(**params), "map")
    native.lambdamart_sample(_dataset(), _params(**params), 0)


# --- errors ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("value", ["30", None, True, [30], 2.5, -1, {"level": 30}])
def test_truncation_level_that_is_not_an_unsigned_integer_is_rejected(value):
    for msg in _both("invalid type", truncation_level=value):
        assert "expected unsigned integer for truncation_level" in msg


def test_truncation_level_that_does_not_fit_u32_is_rejected():
    for msg in _both("invalid value", truncation_level=2 ** 32):
        assert "expected u32" in msg


@pytest.mark.parametrize("value", ["true", None, 1, [True], 1.0, {"on": True}])
def test_lambda_norm_that_is_not_a_boolean_is_rejected(value):
    for msg in _both("invalid type", lambda_norm=value):
        assert "expected a boolean for lambda_norm" in msg


def _opts_call(options, measure="ndcg"):
    ds = _dataset()
    m = fr.CModel.from_dict({"Linear": {"weights": [0.0, 0.0, 1.0]}})
    out = np.zeros(8)
    text = options if isinstance(options, bytes) else json.dumps(options).encode()
    native._status(native._load().fr_debug_lambda_gradients_opts(m.pointer, ds.pointer, None, measure.encode(), 1.0, None, 0, text,
                                                               out.ctypes.data, out.ctypes.data, 8))


@pytest.mark.parametrize("options,text", [
    ({"truncation_level": "3"}, "expected unsigned integer for truncation_level"), ({"truncation_level": -2}, "expected unsigned integer for truncation_level"),
    ({"truncation_level": 2 ** 32}, "expected u32"), ({"lambda_norm": 1}, "expected a boolean for lambda_norm"),
    ({"truncation": 3}, "unknown field `truncation`, expected `truncation_level` or `lambda_norm`"), ([3, True], "expected a map of gradient options")])
def test_the_debug_entry_point_checks_its_options_before_any_device_work(options, text):
    with pytest.raises(Exception) as e:
        _opts_call(options)
    assert text in str(e.value)
    with pytest.raises(Exception, match=r"supported: ndcg, ndcg@k"):
        _opts_call({"truncation_level": 3}, "map")


# --- identities of the restatement -------------------------------------------------------------------

@pytest.fixture(scope="module")
def data():
    """The designed and some random queries of tests/lambdamart_bound.py as one dataset, scored by its linear model."""
    queries = designed_queries() + random_queries(3, 10)
    X, y, qid = as_dataset(queries)
    c = o.Dataset(X, y, qid)
    return X, y, c, c.score_linear(WEIGHTS), lm.query_lists(c)


@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("sigma", [0.3, 1.5])
def test_a_level_of_at_least_the_query_length_changes_no_byte(data, measure, sigma):
    X, y, c, scores, queries = data
    norms = c.default_norms(measure)
    with np.errstate(over="ignore"):
        lam, wt = lm.gradients(scores, y, queries, norms, lm.depth_of(measure), sigma)
    longest = max(len(ids) for ids in queries)
    for T in (0, longest, longest + 1, 2 ** 32 - 1):
        tl, tw = tm.gradients(scores, y, queries, norms, lm.depth_of(measure), sigma, T)
        assert tl.tobytes() == lam.tobytes() and tw.tobytes() == wt.tobytes(), T
    tl, _ = tm.gradients(scores, y, queries, norms, lm.depth_of(measure), sigma, 1)
    assert measure == "ndcg@1" or tl.tobytes() != lam.tobytes()


@pytest.mark.parametrize("k", [1, 3, 10])
def test_under_ndcg_at_k_a_level_of_at_least_k_changes_no_byte(data, k):
    X, y, c, scores, queries = data
    measure = "ndcg@%d" % k
    norms = c.default_norms(measure)
    for sigma in (0.3, 1.5):
        with np.errstate(over="ignore"):
            lam, wt = lm.gradients(scores, y, queries, norms, k, sigma)
        for T in (k, k + 1, 30):
            tl, tw = tm.gradients(scores, y, queries, norms, k, sigma, T)
            assert tl.tobytes() == lam.tobytes() and tw.tobytes() == wt.tobytes(), (sigma, T)
    if k > 1:
        assert tm.gradients(scores, y, queries, norms, k, 1.5, k - 1)[0].tobytes() != lam.tobytes()


def test_the_level_cuts_pairs_only(data):
    """(c): D and Z are those of the untruncated pass: a kept pair's term is the untruncated pass's term.  With one label
    above all others (one document of label 4 over labels 0), the top document's lambda is untouched by any T >= 1 when it
    ranks first."""
    scores = np.array([5.0, 4.0, 3.0, 2.0, 1.0, 0.0])
    y = np.array([4.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    ids = [np.arange(6)]
    z = [float(ex.ExactQuery(scores, y, ids[0]).Z)]
    lam, wt = lm.gradients(scores, y, ids, z)
    for T in (1, 2, 5):
        tl, tw = tm.gradients(scores, y, ids, z, None, 1.0, T)
        assert tl.tobytes() == lam.tobytes() and tw.tobytes() == wt.tobytes()
    # the same labels with the label-4 document ranked last: only pairs with a top-T partner remain
    tl, _ = tm.gradients(scores[::-1].copy(), y, ids, z, None, 1.0, 2)
    full, _ = lm.gradients(scores[::-1].copy(), y, ids, z)
    assert tl[5] == full[5] and tl[4] == full[4] and tl[1] == 0.0 and full[1] != 0.0
    assert tl[0] == -(tl[5] + tl[4])


# --- exact arithmetic --------------------------------------------------------------------------------

class TruncQuery(ex.ExactQuery):
    """ExactQuery restricted to the pairs a truncation level keeps: min(r_i, r_j) < T."""

    def __init__(self, *a, level=0, **kw):
        super().__init__(*a, **kw)
        self.level = level

    def keeps(self, i, j):
        return self.level == 0 or min(self.rank[i], self.rank[j]) < self.level

    def pairs(self, i):
        for p in super().pairs(i):
            if self.keeps(i, p.j):
                yield p

    def cost(self, scores=None):
        s = self.s if scores is None else scores
        c = ex.ZERO
        for h in range(self.m):
            for l in range(self.m):
                if self.live and self.g[h] > self.g[l] and self.D[h] != self.D[l] and self.keeps(h, l):
                    x = ex.CTX.multiply(self.sigma, ex.CTX.subtract(s[h], s[l]))
                    c = ex.SUM.add(c, ex.CTX.multiply(self.delta(h, l), ex.CTX.ln(ex.CTX.add(ex.ONE, ex.CTX.exp(x.copy_negate())))))
        return c


@pytest.mark.parametrize("measure,sigma,T", [("ndcg", 1.0, 1), ("ndcg", 1.5, 5), ("ndcg@10", 0.3, 3), ("ndcg", 0.3, 30), ("ndcg@5000", 1.5, 5)])
def test_restatement_within_bound_of_exact_over_the_qualifying_pairs(data, measure, sigma, T):
    """The bound of tests/lambdamart_bound.py evaluated over the kept pairs only: the same operations over fewer partners."""
    X, y, c, scores, queries = data
    norms = c.default_norms(measure)
    lam, wt = tm.gradients(scores, y, queries, norms, lm.depth_of(measure), sigma, T)
    worst = 0.0
    for k, ids in enumerate(queries):
        if len(ids) > 70:
            continue
        q = TruncQuery(scores[ids], y[ids], ids, lm.depth_of(measure), sigma, norms[k], level=T)
        if not q.live:
            assert not lam[ids].any() and not wt[ids].any()
            continue
        worst = max(worst, worst_ratio(q, range(q.m), lam[ids], wt[ids]))
    print("%s sigma %s T %d: worst error / bound = %.4f" % (measure, sigma, T, worst))


@pytest.mark.parametrize("T", [1, 2, 4])
@pytest.mark.parametrize("depth", [None, 3])
def test_lambda_is_the_negative_gradient_of_the_cost_over_the_qualifying_pairs(T, depth):
    """lambda_p = -dC/ds_p, w_p = d2C/ds_p2 of C summed over the kept pairs only, delta frozen: symmetric differences at 60
    digits, step and tolerance of tests/test_lambdamart_exact_host.py."""
    rng = np.random.default_rng(5)
    m, sigma = 7, 1.5
    scores = np.round(rng.normal(0, 2, m), 1)
    scores[3] = scores[4]
    y = np.array([0, 2, 1, 0.5, 3, 0, 1], dtype=np.float64)
    q = TruncQuery(scores, y, np.arange(m), depth, sigma, level=T)
    h = Decimal("1e-12")
    total = sum(q.delta(a, b) for a in range(m) for b in range(m) if q.g[a] > q.g[b])
    tol = Decimal("1e-20") * (q.sigma + q.sigma ** 4 + 1) * total
    c0 = q.cost()
    full = ex.ExactQuery(scores, y, np.arange(m), depth, sigma).cost()
    assert c0 < full or (depth is not None and T >= depth and c0 == full)  # (T >= k cuts pairs of delta = 0 only)
    with decimal.localcontext(C):
        for p in range(m):
            up, dn = list(q.s), list(q.s)
            up[p], dn[p] = q.s[p] + h, q.s[p] - h
            cu, cd = q.cost(up), q.cost(dn)
            lam, w = q.document(p)
            assert abs(lam - (-(cu - cd) / (2 * h))) <= tol, p
            assert abs(w - (cu - 2 * c0 + cd) / (h * h)) <= tol, p
    lam64, w64 = tm.gradients(scores, y, [np.arange(m)], [float(q.Z)], depth, sigma, T)
    for p in range(m):
        lam, w = q.document(p)
        assert abs(ex.dec(lam64[p]) - lam) <= Decimal("1e-12") * (abs(lam) + 1) and abs(ex.dec(w64[p]) - w) <= Decimal("1e-12") * (w + 1)


# --- normalisation -----------------------------------------------------------------------------------

def _scaled_bound(q, lam, wt):
    """Exact f, and for every document (exact lambda f, exact w f, bound, bound): see the module docstring."""
    with decimal.localcontext(C):
        rows = [gradient_bound(q, i) for i in range(q.m)]
        S = sum((sum((C.multiply(C.multiply(q.sigma, p.rho), p.delta) for p in q.pairs(i)), Decimal(0)) for i in range(q.m)), Decimal(0))
        if S == 0:
            return None, S, rows
        gamma = q.m * U / (1 - q.m * U)
        e_S = sum(r[2] for r in rows) + gamma * S
        ln1p = C.ln(1 + S)
        f = ln1p / C.ln(Decimal(2)) / S
        e_f = (e_S / (1 + S) + U) / ln1p + e_S / S + 5 * U
        out = []
        for el, ew, bl, bw in rows:
            out.append((el * f, ew * f, SLACK * (f * bl + abs(el) * f * (e_f + U)), SLACK * (f * bw + abs(ew) * f * (e_f + U))))
        return f, S, out


@pytest.mark.parametrize("measure,sigma,T", [("ndcg", 1.0, 0), ("ndcg", 1.5, 5), ("ndcg@10", 0.3, 30), ("ndcg", 0.3, 1)])
def test_normalised_restatement_within_bound_of_exact(data, measure, sigma, T):
    X, y, c, scores, queries = data
    norms = c.default_norms(measure)
    raw_l, raw_w, A, S64, f64 = tm.gradients(scores, y, queries, norms, lm.depth_of(measure), sigma, T, False, parts=True)
    lam, wt, A2, S2, f2 = tm.gradients(scores, y, queries, norms, lm.depth_of(measure), sigma, T, True, parts=True)
    assert A2.tobytes() == A.tobytes() and S2.tobytes() == S64.tobytes() and np.all(f64 == 1.0)
    scaled = 0
    for k, ids in enumerate(queries):
        assert S64[k] == lm.seq_sum(A[ids]) and np.all(A[ids] >= 0.0)
        if len(ids) > 70:
            continue
        q = TruncQuery(scores[ids], y[ids], ids, lm.depth_of(measure), sigma, norms[k], level=T)
        if S64[k] == 0.0:  # nothing to scale: the raw values, zeros where the query has no pair mass at all
            assert f2[k] == 1.0 and lam[ids].tobytes() == raw_l[ids].tobytes() and wt[ids].tobytes() == raw_w[ids].tobytes()
            assert not lam[ids].any()
            continue
        assert q.live
        f, S, rows = _scaled_bound(q, lam[ids], wt[ids])
        assert f is not None
        # the scale itself is the f64 statement of the definition, and every value is its raw value times it
        assert f2[k] == tm.scale(float(S64[k])) and lam[ids].tobytes() == (raw_l[ids] * f2[k]).tobytes()
        assert wt[ids].tobytes() == (raw_w[ids] * f2[k]).tobytes()
        for i, (el, ew, bl, bw) in enumerate(rows):
            assert abs(ex.dec(lam[ids][i]) - el) <= bl, (k, i, float(lam[ids][i]), float(el), float(bl))
            assert abs(ex.dec(wt[ids][i]) - ew) <= bw, (k, i, float(wt[ids][i]), float(ew), float(bw))
        scaled += 1
    assert scaled >= 10


def test_scaling_one_query_does_not_touch_another(data):
    X, y, c, scores, queries = data
    norms = c.default_norms("ndcg")
    lam, wt = tm.gradients(scores, y, queries, norms, None, 1.0, 5, True)
    for k in (0, 4, len(queries) - 1):
        one_l, one_w = tm.gradients(scores, y, [queries[k]], [norms[k]], None, 1.0, 5, True)
        ids = queries[k]
        assert one_l[ids].tobytes() == lam[ids].tobytes() and one_w[ids].tobytes() == wt[ids].tobytes()
    # ... and a query's scale moves with its own scores only
    moved = scores.copy()
    moved[queries[0]] = moved[queries[0]][::-1]
    lam2, _ = tm.gradients(moved, y, queries, norms, None, 1.0, 5, True)
    rest = np.concatenate(queries[1:])
    assert lam2[rest].tobytes() == lam[rest].tobytes()


def test_a_query_without_pair_mass_is_left_alone():
    """S = 0: no pair, or every kept pair saturated to rho = 0 (exp overflow): zeros stay zeros, nothing divides by S."""
    ids = [np.arange(3), np.arange(3, 5), np.arange(5, 8)]
    y = np.array([1.0, 1.0, 1.0, 2.0, 0.0, 0.0, 0.0, 0.0])
    scores = np.array([0.0, 1.0, 2.0, 2000.0, 0.0, 1.0, 2.0, 3.0])
    lam, wt, A, S, f = tm.gradients(scores, y, ids, [1.0, 1.0, float("nan")], None, 1.0, 2, True, parts=True)
    assert not lam.any() and not wt.any() and not S.any() and np.all(f == 1.0)
    assert np.all(np.isfinite(lam)) and np.all(np.isfinite(wt))
