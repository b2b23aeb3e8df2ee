"""LambdaMART's leaf regularisation without a GPU ("Leaf regularisation"): the three wire keys and their
refusals (every request here fails or is only parsed before any device work), the numpy restatement
(tests/lambdamart_reg_model.py) against rational arithmetic and against the restatements it generalises, the host header's
arithmetic (`native.hist_reg_term`) against the restatement bit for bit, and the header on its own under the address and
undefined-behaviour sanitizers (tests/lambdamart_reg_sanitize.cpp)."""
import json
import math
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import clib, native
from fastrank_amd.training import LambdaMARTParams, TrainRequest
from tests import lambdamart_hist_model as hm
from tests import lambdamart_leafwise_model as lw
from tests import lambdamart_monotone_model as mm
from tests import lambdamart_newton_model as nm
from tests import lambdamart_reg_model as rm
from tests import lambdamart_symmetric_model as sy
from tests.conftest import synth_dataset

KEYS = ["num_trees", "learning_rate", "max_depth", "min_leaf_support", "split_candidates", "sigma", "quiet"]
NUMBERS = ["lambda_l1", "max_delta_step", "path_smooth"]
INF = float("inf")


def _dataset():
    X = np.arange(24, dtype=np.float32).reshape(8, 3)
    y = np.array([0, 1, 2, 0, 1, 0, 0, 1], dtype=np.float64)
    qid = np.array([1, 1, 1, 1, 2, 2, 2, 2], dtype=np.int64)
    return fr.CDataset.from_numpy(X, y, qid)


def _train_raw(params, measure="ndcg"):
    text = json.dumps({"measure": measure, "params": {"LambdaMART": params}, "judgments": None}).encode()
    return clib._unwrap(clib._load().train_model(text, _dataset().pointer))


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


NEWTON = dict(grower="histogram", split_gain="newton")


# --- wire form ---------------------------------------------------------------------------------------

def test_keys_are_absent_at_their_defaults():
    assert list(LambdaMARTParams().to_dict().keys()) == KEYS
    p = LambdaMARTParams()
    assert (p.lambda_l1, p.max_delta_step, p.path_smooth) == (0.0, 0.0, 0.0)
    # a key of 0.0 given explicitly is not written
    assert list(LambdaMARTParams(lambda_l1=0.0, max_delta_step=0.0, path_smooth=0.0).to_dict().keys()) == KEYS
    assert list(LambdaMARTParams(lambda_l1=0.0, max_delta_step=2.0, **NEWTON).to_dict().keys()) == KEYS + ["grower", "split_gain", "max_delta_step"]
    assert list(clib.query_json("lambdamart_defaults")["params"]["LambdaMART"].keys()) == KEYS


def test_keys_round_trip():
    req = TrainRequest.lambdamart()
    req.params.grower, req.params.split_gain = "histogram", "newton"
    req.params.lambda_l1, req.params.max_delta_step, req.params.path_smooth = 2.0 ** -7, 1e300, 3.5
    d = req.to_dict()
    wire = d["params"]["LambdaMART"]
    assert list(wire.keys()) == KEYS + ["grower", "split_gain"] + NUMBERS
    assert [wire[k] for k in NUMBERS] == [2.0 ** -7, 1e300, 3.5]
    back = TrainRequest.from_dict(json.loads(json.dumps(d)))
    assert back == req and back.params.max_delta_step == 1e300
    c = req.clone()
    assert c == req and c.params is not req.params and c != TrainRequest.lambdamart()
    req.params.max_delta_step = 0.0
    assert list(req.to_dict()["params"]["LambdaMART"].keys()) == KEYS + ["grower", "split_gain", "lambda_l1", "path_smooth"]
    assert LambdaMARTParams.from_dict(dict(lambda_l1=0.5, **NEWTON)).lambda_l1 == 0.5


def test_native_parser_reads_the_keys():
    """The native side parses and validates the keys: the per-tree sample hook parses a whole parameter object."""
    native.lambdamart_sample(_dataset(), LambdaMARTParams(lambda_l1=0.5, max_delta_step=2.0, path_smooth=1.0, **NEWTON), 0)
    native.lambdamart_sample(_dataset(), LambdaMARTParams(lambda_l1=0.5, max_delta_step=2.0, symmetric_trees=True, **NEWTON), 0)
    with pytest.raises(Exception, match="path_smooth must be finite and at least 0"):
        native.lambdamart_sample(_dataset(), LambdaMARTParams(path_smooth=-1.0, **NEWTON), 0)


@pytest.mark.parametrize("key", NUMBERS)
@pytest.mark.parametrize("value", [-1.0, -1e-300])
def test_negative_number_is_rejected(key, value):
    for msg in _both("invalid value", **dict(NEWTON, **{key: value})):
        assert key + " must be finite and at least 0" in msg


@pytest.mark.parametrize("key", NUMBERS)
@pytest.mark.parametrize("value", [float("nan"), float("inf")])
def test_number_not_finite_is_rejected(key, value):
    _both("Error", **dict(NEWTON, **{key: value}))
    text = json.dumps({"measure": "ndcg", "params": {"LambdaMART": _params(**dict(NEWTON, **{key: 12345.5}))}, "judgments": None})
    with pytest.raises(Exception, match="number out of range"):
        clib._unwrap(clib._load().train_model(text.replace("12345.5", "1e999").encode(), _dataset().pointer))


@pytest.mark.parametrize("key", NUMBERS)
@pytest.mark.parametrize("value", ["1", None, True, [1.0]])
def test_number_of_another_type_is_rejected(key, value):
    for msg in _both("invalid type", **dict(NEWTON, **{key: value})):
        assert "expected f64 for " + key in msg


@pytest.mark.parametrize("key", NUMBERS)
def test_a_key_needs_the_histogram_grower_and_the_newton_gain(key):
    for others in (dict(), dict(grower="exact")):
        for msg in _both("invalid value", **dict(others, **{key: 0.5})):
            assert key + " needs grower: " in msg and "histogram" in msg
    for others in (dict(grower="histogram"), dict(grower="histogram", split_gain="variance")):
        for msg in _both("invalid value", **dict(others, **{key: 0.5})):
            assert key + " needs split_gain: " in msg and "newton" in msg


def test_path_smooth_is_refused_with_symmetric_trees():
    for msg in _both("invalid value", symmetric_trees=True, path_smooth=1.0, **NEWTON):
        assert "path_smooth cannot be combined with symmetric_trees" in msg


@pytest.mark.parametrize("params", [dict(lambda_l1=0.5, max_delta_step=1.0, path_smooth=2.0), dict(lambda_l1=1.0, symmetric_trees=True),
                                    dict(max_delta_step=1e300, max_leaves=8), dict(path_smooth=1.0, monotone_constraints={"0": 1}),
                                    dict(path_smooth=1.0, goss_top_rate=0.2, drop_rate=0.1, objective="xendcg"),
                                    dict(lambda_l1=0.0, max_delta_step=0.0, path_smooth=0.0)])
def test_accepted_requests_reach_the_later_checks(params):
    """Valid keys pass the parser: the request then fails on what is checked after the parameters."""
    with pytest.raises(Exception, match="num_trees must be at least 1"):
        _train_raw(_params(num_trees=0, **dict(NEWTON, **params)))


def test_hist_tree_rejects_bad_arguments_before_any_call():
    lam = np.zeros(8)
    for key in NUMBERS:
        with pytest.raises(ValueError, match="need split_gain='newton'"):
            native.hist_tree(_dataset(), lam, lam, 4, 2, 1, **{key: 1.0})
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="must be finite and at least 0"):
                native.hist_tree(_dataset(), lam, lam, 4, 2, 1, split_gain="newton", **{key: bad})
    with pytest.raises(ValueError, match="symmetric trees take no path_smooth"):
        native.hist_tree(_dataset(), lam, lam, 4, 2, 1, split_gain="newton", symmetric=True, path_smooth=1.0)


def test_options_record_ends_with_the_three_doubles_and_a_fresh_one_is_off():
    names = [f[0] for f in clib.HistTreeOptions._fields_]
    assert names[-3:] == NUMBERS
    fresh = clib.HistTreeOptions()
    assert (fresh.lambda_l1, fresh.max_delta_step, fresh.path_smooth) == (0.0, 0.0, 0.0)


# --- the restatement against rational arithmetic --------------------------------------------------------

def _exact_side(q, w, n, S, Sw, l1, l2, mds, smooth, parent, lo, hi):
    """The definition with every operation carried out exactly on its (already rounded) inputs and then rounded once to
    nearest even: float(Fraction) is the correctly rounded quotient of two integers.  A restatement whose every operation
    lies within half an ulp of the exact one gives these very bits."""
    F = Fraction
    rnd = float
    G = rnd(F(q) / F(2) ** S)
    den = rnd(rnd(F(w) / F(2) ** Sw) + F(l2))
    T = rnd(F(G) - F(l1)) if G > l1 else (rnd(F(G) + F(l1)) if G < -l1 else 0.0)
    q0 = rnd(F(T) / F(den)) if den != 0.0 else 0.0
    o = q0
    if mds > 0.0:
        o = mds if o > mds else o
        o = -mds if o < -mds else o
    if smooth > 0.0 and parent is not None:
        r = rnd(F(rnd(F(n))) / F(smooth))
        r1 = rnd(F(r) + 1)
        o = rnd(F(rnd(F(rnd(F(o) * F(r))) / F(r1))) + F(rnd(F(parent) / F(r1))))
    v = lo if o < lo else o
    v = hi if v > hi else v
    if v == q0:
        term = rnd(F(rnd(F(T) * F(T))) / F(den))
    else:
        term = rnd(F(rnd(F(rnd(F(2) * F(T))) * F(v))) - F(rnd(F(rnd(F(den) * F(v))) * F(v))))
    return v, term


def _random_case(rng):
    S, Sw = int(rng.integers(20, 50)), int(rng.integers(20, 50))
    q = int(rng.integers(-2 ** 58, 2 ** 58)) >> int(rng.integers(0, 50))
    w = int(rng.integers(1, 2 ** 58)) >> int(rng.integers(0, 50))
    n = int(rng.integers(1, 5000))
    dy = lambda: float(rng.integers(0, 2 ** 20)) * 2.0 ** -int(rng.integers(0, 30))  # noqa: E731 (a dyadic parameter)
    l1, mds, smooth = (dy() if rng.random() < 0.7 else 0.0 for _ in range(3))
    l2 = dy() if rng.random() < 0.5 else 0.0
    parent = None if rng.random() < 0.2 else float(rng.normal()) * 4.0
    lo, hi = (-INF, INF) if rng.random() < 0.5 else sorted(float(x) for x in rng.normal(size=2) * 2.0)
    return q, w, n, S, Sw, l1, l2, mds, smooth, parent, lo, hi


def _restated(q, w, n, S, Sw, l1, l2, mds, smooth, parent, lo, hi):
    term, v = rm.side(q, w, n, S, Sw, l2, (l1, mds, smooth), parent, lo, hi)
    return float(v), float(term)


def _bits(pair):
    return np.asarray(pair, dtype=np.float64).tobytes()


def test_restatement_against_exact_arithmetic():
    rng = np.random.default_rng(20240611)
    moved = 0
    for _ in range(1500):
        case = _random_case(rng)
        if math.ldexp(float(case[1]), -case[4]) + case[6] == 0.0:
            continue
        got, exact = _restated(*case), _exact_side(*case)
        assert _bits(got) == _bits(exact), (case, got, exact)
        moved += got[0] != float(rm.sums(case[0], case[1], case[3], case[4], case[5], case[6])[2])
    assert 300 < moved < 1400  # both forms of the term were exercised


# --- the host header against the restatement ---------------------------------------------------------

def _designed_cases():
    """(q, w, n, S, Sw, l1, l2, mds, smooth, parent, lo, hi) with G = q / 16, H = w / 16."""
    base = dict(q=48, w=32, n=4, S=4, Sw=4, l1=0.0, l2=1.0, mds=0.0, smooth=0.0, parent=None, lo=-INF, hi=INF)
    out = []

    def case(**kw):
        c = dict(base, **kw)
        out.append(tuple(c[k] for k in ("q", "w", "n", "S", "Sw", "l1", "l2", "mds", "smooth", "parent", "lo", "hi")))

    case()
    for q in (48, -48, 47, -47, 49, -49, 0):  # |G| == l1 exactly, just inside, just outside, G = 0
        case(q=q, l1=3.0)
    case(q=0, l1=0.0)
    case(w=0, l2=0.0), case(w=0, l2=0.0, mds=2.0, smooth=1.0, parent=0.5)  # den == 0
    for q in (48, -48, 49, -49, 47):  # an output exactly at +-mds, beyond it and inside it
        case(q=q, mds=1.0)
    case(q=2 ** 62, w=1, S=-900, Sw=1000, l2=0.0, mds=1.0)  # the quotient overflows
    case(smooth=4.0), case(smooth=4.0, parent=-2.0), case(smooth=4.0, parent=-2.0, n=1), case(smooth=4.0, parent=-2.0, n=4999)
    case(smooth=2.0 ** 60, parent=-2.0, n=1)  # r + 1.0 rounds to 1.0
    case(smooth=2.0 ** -900, parent=-2.0, n=2 ** 32 - 1)  # r is huge
    case(smooth=2.0 ** -1000, parent=-2.0, n=2 ** 32 - 1)  # r overflows: the definition's NaN
    case(hi=0.5), case(hi=0.5, smooth=4.0, parent=-2.0)  # a bound that binds before smoothing and not after
    case(lo=0.0), case(lo=0.0, smooth=4.0, parent=-2.0)  # ... and one that binds only after it
    case(lo=1.0, hi=1.0), case(lo=-1.0, hi=1.0, mds=0.5, smooth=1.0, parent=3.0, l1=1.0)
    case(q=-(2 ** 63), w=2 ** 63 - 1, S=61, Sw=61), case(q=2 ** 63 - 1, w=-(2 ** 63), S=0, Sw=0, mds=1e300)
    return out


def _native(case):
    return native.hist_reg_term(*case)


def test_hist_reg_term_equals_the_restatement_on_the_designed_cases():
    seen_nan = False
    for case in _designed_cases():
        got, exp = _native(case), _restated(*case)
        assert _bits(got) == _bits(exp), (case, got, exp)
        seen_nan = seen_nan or got[0] != got[0]
    assert seen_nan  # (the overflowing r is among them)
    # what the designed cases were designed for
    d = {c: _native(c) for c in _designed_cases()}
    base = (48, 32, 4, 4, 4)
    assert d[base + (0.0, 1.0, 0.0, 0.0, None, -INF, INF)] == (1.0, 3.0)
    assert d[base + (3.0, 1.0, 0.0, 0.0, None, -INF, INF)] == (0.0, 0.0)
    assert d[(49, 32, 4, 4, 4, 3.0, 1.0, 0.0, 0.0, None, -INF, INF)][0] == (49 / 16 - 3.0) / 3.0
    assert d[base + (0.0, 1.0, 1.0, 0.0, None, -INF, INF)] == (1.0, 3.0)
    assert d[(49, 32, 4, 4, 4, 0.0, 1.0, 1.0, 0.0, None, -INF, INF)][0] == 1.0
    assert d[(2 ** 62, 1, 4, -900, 1000, 0.0, 0.0, 1.0, 0.0, None, -INF, INF)][0] == 1.0
    assert d[base + (0.0, 1.0, 0.0, 4.0, None, -INF, INF)][0] == 1.0  # the root is not pulled
    assert d[base + (0.0, 1.0, 0.0, 4.0, -2.0, -INF, INF)][0] == -0.5
    assert d[(48, 32, 1, 4, 4, 0.0, 1.0, 0.0, 2.0 ** 60, -2.0, -INF, INF)][0] == 2.0 ** -60 - 2.0
    assert d[(48, 32, 2 ** 32 - 1, 4, 4, 0.0, 1.0, 0.0, 2.0 ** -900, -2.0, -INF, INF)] == (1.0, 3.0)
    assert d[base + (0.0, 1.0, 0.0, 4.0, -2.0, 0.0, INF)] == (0.0, 0.0)


def test_hist_reg_term_equals_the_restatement_on_random_cases():
    rng = np.random.default_rng(77)
    for _ in range(3000):
        case = _random_case(rng)
        assert _bits(_native(case)) == _bits(_restated(*case)), case


# --- the restatement's identities -------------------------------------------------------------------

def _case(seed, n=1200, d=5, q=20):
    X, y, qid = synth_dataset(seed, n, d, q)
    rng = np.random.default_rng(seed)
    lam = rng.normal(0.0, 1.0, n) + 0.5 * (y - y.mean())
    wt = rng.random(n) * np.exp(-3.0 * rng.random(n)) + 2.0 ** -20
    return X, lam, wt, np.arange(n), list(range(d))


@pytest.mark.parametrize("reg", [(0.0, 0.0, 0.0), (0.0, 1e300, 0.0)], ids=["zeros", "mds-1e300"])
@pytest.mark.parametrize("k", [2, 16, 64])
def test_without_an_effect_it_is_the_restatements_it_generalises(reg, k):
    X, lam, wt, ids, feats = _case(k)
    binned = hm.bin_matrix(X, ids, feats, k)
    nw = dict(lambda_l2=0.5, min_sum_hessian=2.0 ** -6, min_split_gain=2.0 ** -10)
    common = (X, lam, wt, ids, feats, 6, 5, k)
    assert rm.fit_tree(*common, reg, binned=binned, **nw) == nm.fit_tree(*common, binned, **nw)
    assert rm.fit_tree(*common, reg, max_leaves=9, binned=binned, **nw) == lw.fit_tree(*common, 9, binned, split_gain="newton", **nw)
    mono = {0: 1, 2: -1}
    assert rm.fit_tree(*common, reg, monotone=mono, binned=binned, **nw) == mm.fit_tree(*common, mono, 0, binned, **nw)[0]
    assert rm.fit_tree(*common, reg, monotone=mono, max_leaves=9, binned=binned, **nw) == mm.fit_tree(*common, mono, 9, binned, **nw)[0]
    assert rm.fit_tree(*common, reg, symmetric=True, binned=binned, **nw) == sy.fit_tree(*common, binned, split_gain="newton", **nw)


def test_a_threshold_above_every_gradient_sum_gives_one_zero_leaf():
    X, lam, wt, ids, feats = _case(3)
    l1 = float(np.sum(np.abs(lam))) * 1.5  # no subset's |G| reaches it (the quantised sums are within 2^-50 of the real ones)
    for kw in (dict(), dict(max_leaves=8), dict(symmetric=True), dict(monotone={1: 1})):
        assert rm.fit_tree(X, lam, wt, ids, feats, 6, 1, 16, (l1, 0.0, 0.0), **kw) == {"LeafNode": 0.0}
    assert "FeatureSplit" in rm.fit_tree(X, lam, wt, ids, feats, 6, 1, 16, (l1 / 1e3, 0.0, 0.0))


@pytest.mark.parametrize("kw", [dict(), dict(max_leaves=12), dict(symmetric=True), dict(monotone={0: 1, 1: -1}), dict(lambda_l1=0.25)],
                         ids=["levels", "leaves", "symmetric", "monotone", "l1"])
def test_every_leaf_is_within_the_cap_without_smoothing(kw):
    X, lam, wt, ids, feats = _case(5)
    kw = dict(kw)
    l1 = kw.pop("lambda_l1", 0.0)
    free = rm.leaves_of(rm.fit_tree(X, lam, wt, ids, feats, 7, 1, 16, (l1, 0.0, 0.0), **kw))
    mds = float(np.median(np.abs(free)))
    capped = rm.leaves_of(rm.fit_tree(X, lam, wt, ids, feats, 7, 1, 16, (l1, mds, 0.0), **kw))
    assert max(abs(v) for v in free) > mds  # the cap has something to do
    assert all(abs(v) <= mds for v in capped) and any(abs(v) == mds for v in capped)


def test_smoothing_pulls_small_leaves_toward_their_parents():
    X, lam, wt, ids, feats = _case(8)
    trace = []
    tree = rm.fit_tree(X, lam, wt, ids, feats, 5, 1, 16, (0.0, 0.0, 50.0), trace=trace)
    plain = nm.fit_tree(X, lam, wt, ids, feats, 5, 1, 16)
    assert tree != plain and trace and trace[0]["parent"] is None
    assert max(abs(v) for v in rm.leaves_of(tree)) < max(abs(v) for v in rm.leaves_of(plain))


# --- the header under the sanitizers ------------------------------------------------------------------

def test_reg_header_under_address_and_undefined_sanitizers(tmp_path):
    """tests/lambdamart_reg_sanitize.cpp: a program of its own over csrc/lambdamart_reg.hpp, built with
    -fsanitize=address,undefined and run directly."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "lambdamart_reg_sanitize")
    build = subprocess.run([cxx, "-std=c++17", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                            "-I", os.path.join(here, "..", "fastrank_amd", "csrc"), os.path.join(here, "lambdamart_reg_sanitize.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "lambdamart_reg ok" in run.stdout, run.stdout
