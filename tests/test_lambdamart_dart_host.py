"""LambdaMART's DART boosting on the CPU ("DART"): the three keys' wire form and refusals, the Python
dataclass, and the drop plan of the library (native.lambdamart_dart_plan, csrc/lambdamart_dart.hpp) against the numpy
restatement (tests/lambdamart_dart_model.py), with the plan's properties; the header also runs on its own under the
address and undefined-behaviour sanitizers (tests/lambdamart_dart_sanitize.cpp).
"""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import clib, native
from fastrank_amd.training import LambdaMARTParams, TrainRequest
from tests import lambdamart_dart_model as dm

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


# --- wire form and the dataclass ---------------------------------------------------------------------

def test_the_keys_are_absent_at_their_defaults():
    p = LambdaMARTParams()
    assert (p.drop_rate, p.max_drop, p.skip_drop) == (0.0, 50, 0.5)
    assert list(p.to_dict().keys()) == KEYS
    assert list(TrainRequest.lambdamart().to_dict()["params"]["LambdaMART"].keys()) == KEYS
    assert list(clib.query_json("lambdamart_defaults")["params"]["LambdaMART"].keys()) == KEYS
    # drop_rate: 0 (and the two others at their defaults) is byte for byte the request without the keys
    explicit = LambdaMARTParams(drop_rate=0.0, max_drop=50, skip_drop=0.5)
    assert json.dumps(explicit.to_dict()) == json.dumps(p.to_dict())
    req, plain = TrainRequest.lambdamart(), TrainRequest.lambdamart()
    req.params = explicit
    assert json.dumps(req.to_dict()) == json.dumps(plain.to_dict())


@pytest.mark.parametrize("kw,written", [(dict(drop_rate=0.1), ["drop_rate"]), (dict(drop_rate=1.0, max_drop=0), ["drop_rate", "max_drop"]),
                                        (dict(drop_rate=0.25, skip_drop=0.0), ["drop_rate", "skip_drop"]),
                                        (dict(drop_rate=0.5, max_drop=3, skip_drop=0.25), ["drop_rate", "max_drop", "skip_drop"])])
def test_the_keys_round_trip(kw, written):
    req = TrainRequest.lambdamart()
    req.params = LambdaMARTParams(**kw)
    d = req.to_dict()
    wire = d["params"]["LambdaMART"]
    assert list(wire.keys()) == KEYS + written and all(wire[k] == kw[k] for k in written)
    back = TrainRequest.from_dict(json.loads(json.dumps(d)))
    assert back == req and all(getattr(back.params, k) == v for k, v in kw.items())
    assert req.clone() == req and req.clone() != TrainRequest.lambdamart()
    # the native parser takes the same payload (the plan hook parses it with LambdaMARTParams::from_json)
    assert len(native.lambdamart_dart_plan(wire, 3)) == 3
    d["params"]["LambdaMART"] = _params(drop_rate=0.0, max_drop=50, skip_drop=0.5)  # the explicit defaults read back as the defaults
    assert TrainRequest.from_dict(d).params == LambdaMARTParams()


def test_the_native_parser_takes_the_defaults_spelled_out():
    for wire in (_params(), _params(drop_rate=0), _params(drop_rate=0.0, max_drop=50, skip_drop=0.5)):
        for row in native.lambdamart_dart_plan(wire, 4):
            assert row["dropped"] == [] and np.all(row["after"] == 0.1)


# --- refusals, before any device work ----------------------------------------------------------------

def _refused(params, text):
    for call in (lambda: _train_raw(params), lambda: native.lambdamart_dart_plan(params, 2)):
        with pytest.raises(Exception, match="invalid value") as e:
            call()
        assert text in str(e.value) and "line: 0, column: 0" in str(e.value)


@pytest.mark.parametrize("value", [-0.1, 1.5, -1e-300, 2, 1e308])
def test_a_drop_rate_outside_its_range_is_refused(value):
    _refused(_params(drop_rate=value), "drop_rate must be at least 0 and at most 1")


@pytest.mark.parametrize("value", [-0.5, 1.0000001, 3])
def test_a_skip_drop_outside_its_range_is_refused(value):
    _refused(_params(drop_rate=0.5, skip_drop=value), "skip_drop must be at least 0 and at most 1")


@pytest.mark.parametrize("value", [-1, 2 ** 32, 1.5, "3", None])
def test_a_max_drop_that_is_no_u32_is_refused(value):
    with pytest.raises(Exception, match="invalid (type|value)") as e:
        _train_raw(_params(drop_rate=0.5, max_drop=value))
    assert "max_drop" in str(e.value) or "u32" in str(e.value)


@pytest.mark.parametrize("kw,key", [(dict(max_drop=3), "max_drop"), (dict(max_drop=0), "max_drop"), (dict(skip_drop=0.25), "skip_drop"),
                                    (dict(skip_drop=1.0, drop_rate=0.0), "skip_drop"), (dict(max_drop=7, drop_rate=0), "max_drop")])
def test_max_drop_and_skip_drop_need_a_drop_rate(kw, key):
    _refused(_params(**kw), key + " needs drop_rate greater than 0")
    with pytest.raises(Exception, match=key + " needs drop_rate greater than 0"):
        _train_python(**kw)


@pytest.mark.parametrize("grower", ["exact", "histogram"])
def test_early_stopping_is_refused_under_dart(grower):
    kw = dict(drop_rate=0.1, validation_queries=["2"], early_stopping_rounds=2)
    if grower == "histogram":
        kw["grower"] = "histogram"
    _refused(_params(**kw), "early_stopping_rounds cannot be combined with drop_rate greater than 0")
    with pytest.raises(Exception, match="early_stopping_rounds cannot be combined with drop_rate"):
        _train_python(**kw)
    # ... while held-out queries alone, and early stopping without DART, still parse
    assert len(native.lambdamart_dart_plan(_params(drop_rate=0.1, validation_queries=["2"]), 2)) == 2
    assert len(native.lambdamart_dart_plan(_params(validation_queries=["2"], early_stopping_rounds=2), 2)) == 2


# --- the plan ----------------------------------------------------------------------------------------

def _same_plan(got, exp):
    assert len(got) == len(exp)
    for t, (row, (dropped, before, after)) in enumerate(zip(got, exp)):
        assert row["dropped"] == dropped, "tree %d" % t
        assert row["before"].tobytes() == before.tobytes() and row["after"].tobytes() == after.tobytes(), "tree %d" % t


@pytest.mark.parametrize("seed", [0, 1, 42, 2 ** 63, 2 ** 63 + 12345, 2 ** 64 - 1])
@pytest.mark.parametrize("rates", [(0.1, 50, 0.5), (0.5, 3, 0.25), (1.0, 0, 0.0), (0.9, 1, 0.0), (0.3, 0, 1.0), (1e-3, 50, 0.0)])
def test_the_librarys_plan_is_the_restatements(seed, rates):
    drop_rate, max_drop, skip_drop = rates
    wire = _params(seed=seed, drop_rate=drop_rate, max_drop=max_drop, skip_drop=skip_drop, learning_rate=0.3)
    _same_plan(native.lambdamart_dart_plan(wire, 40), dm.plan(seed, drop_rate, max_drop, skip_drop, 40, 0.3))


def test_the_plan_reads_its_own_stream():
    """The drops come from Rand64(seed ^ DART_STREAM): the per-tree sample seeds of Rand64(seed) are the first values of
    another stream, and the sample hook answers as it did whatever the DART keys say."""
    from oracle import pyoracle as o
    from tests import lambdamart_sample_model as sm

    for seed in (0, 7, 2 ** 63 + 5):
        assert not np.array_equal(o.rand64_stream(seed, 4), o.rand64_stream(seed ^ dm.DART_STREAM, 4))
        for t in (0, 3):
            base = _params(seed=seed, query_sampling_rate=0.5, feature_sampling_rate=0.7)
            f0, q0 = native.lambdamart_sample(_dataset(), base, t)
            f1, q1 = native.lambdamart_sample(_dataset(), dict(base, drop_rate=0.5, max_drop=3, skip_drop=0.25), t)
            ef, eq = sm.sample(seed, t, 3, 2, (0.5, 0.7))
            assert np.array_equal(f0, f1) and np.array_equal(q0, q1) and np.array_equal(f0, ef) and np.array_equal(q0, eq)


def test_skip_drop_one_never_drops():
    for seed in (0, 5):
        for row in native.lambdamart_dart_plan(_params(seed=seed, drop_rate=1.0, max_drop=0, skip_drop=1.0), 60):
            assert row["dropped"] == [] and np.all(row["after"] == 0.1)


def test_full_rates_drop_every_earlier_tree():
    rows = native.lambdamart_dart_plan(_params(seed=3, drop_rate=1.0, max_drop=0, skip_drop=0.0, learning_rate=0.5), 30)
    w = np.zeros(0)
    for t, row in enumerate(rows):
        assert row["dropped"] == list(range(t))
        w = np.append(w * (np.float64(t) / np.float64(t + 1)), np.float64(0.5) / np.float64(t + 1))
        assert row["after"].tobytes() == w.tobytes()


def test_max_drop_keeps_the_smallest_indices():
    capped = native.lambdamart_dart_plan(_params(seed=9, drop_rate=0.5, max_drop=3, skip_drop=0.0), 40)
    free = native.lambdamart_dart_plan(_params(seed=9, drop_rate=0.5, max_drop=0, skip_drop=0.0), 40)
    assert any(len(r["dropped"]) > 3 for r in free)
    for a, b in zip(capped, free):
        assert a["dropped"] == b["dropped"][:3]  # (the draws are the same: the cap cuts the list, nothing else)
    one = native.lambdamart_dart_plan(_params(seed=9, drop_rate=0.5, max_drop=1, skip_drop=0.0), 40)
    assert all(r["dropped"] == f["dropped"][:1] for r, f in zip(one, free))


def test_the_stream_position_of_a_tree_does_not_depend_on_the_rates():
    """Tree t always draws 1 + t floats: what tree t drops under one setting can be read off the draws at the position
    t (t + 1) / 2 - 1 whatever the earlier trees did, skipped or capped."""
    seed, T = 21, 30
    draws = dm.rand_floats(seed, T * (T + 1) // 2)
    for drop_rate, max_drop, skip_drop in ((0.5, 3, 0.25), (0.05, 50, 0.9), (1.0, 0, 0.0), (0.7, 2, 0.5)):
        rows = native.lambdamart_dart_plan(_params(seed=seed, drop_rate=drop_rate, max_drop=max_drop, skip_drop=skip_drop), T)
        for t in range(1, T):
            at = t * (t + 1) // 2 - 1
            u, c = draws[at], draws[at + 1:at + 1 + t]
            exp = [] if u < skip_drop else [int(i) for i in np.flatnonzero(c < drop_rate)]
            assert rows[t]["dropped"] == (exp[:max_drop] if max_drop else exp), (t, drop_rate)


def test_an_empty_drop_is_an_ordinary_boosting_step():
    rows = native.lambdamart_dart_plan(_params(seed=4, drop_rate=0.3, max_drop=50, skip_drop=0.5, learning_rate=0.07), 50)
    assert any(r["dropped"] for r in rows) and any(not r["dropped"] for r in rows[1:])
    for t, row in enumerate(rows):
        k = len(row["dropped"])
        assert len(row["before"]) == t and len(row["after"]) == t + 1
        if k == 0:
            assert row["after"][:t].tobytes() == row["before"].tobytes() and row["after"][t] == 0.07
            continue
        assert row["after"][t] == 0.07 / (k + 1)
        f = np.float64(k) / np.float64(k + 1)
        for i in range(t):
            assert row["after"][i] == (row["before"][i] * f if i in row["dropped"] else row["before"][i])
        if t + 1 < len(rows):
            assert rows[t + 1]["before"].tobytes() == row["after"].tobytes()


# --- the header under the sanitizers ------------------------------------------------------------------

def test_dart_header_under_address_and_undefined_sanitizers(tmp_path):
    """tests/lambdamart_dart_sanitize.cpp: a program of its own over csrc/lambdamart_dart.hpp (plans replayed at the edges:
    1 and 300 trees, rates 0 and 1, max_drop 0 / 1 / beyond the tree count), built with -fsanitize=address,undefined and run
    directly."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "lambdamart_dart_sanitize")
    build = subprocess.run([cxx, "-std=c++17", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                            "-I", os.path.join(here, "..", "fastrank_amd", "csrc"), os.path.join(here, "lambdamart_dart_sanitize.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "lambdamart_dart ok" in run.stdout, run.stdout
