"""LambdaMART's gradient-based one-side sampling on the CPU ("GOSS"): the two keys' wire form and
refusals, the Python dataclass, and the properties of the numpy restatement (tests/lambdamart_goss_model.py) that the device
tests hold the kernels to; the host header also runs on its own under the address and undefined-behaviour sanitizers
(tests/lambdamart_goss_sanitize.cpp).
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
from tests import lambdamart_goss_model as gm
from tests import lambdamart_xendcg_model as xm

KEYS = ["num_trees", "learning_rate", "max_depth", "min_leaf_support", "split_candidates", "sigma", "quiet"]
HIST = dict(grower="histogram", split_gain="newton")


def _dataset():
    X = np.arange(24, dtype=np.float32).reshape(8, 3)
    y = np.array([0, 1, 2, 0, 1, 0, 0, 1], dtype=np.float64)
    qid = np.array([1, 1, 1, 1, 2, 2, 2, 2], dtype=np.int64)
    return fr.CDataset.from_numpy(X, y, qid)


def _params(**kw):
    p = LambdaMARTParams().to_dict()
    p.update(kw)
    return p


def _train_text(params_text):
    text = ('{"measure": "ndcg", "params": {"LambdaMART": %s}, "judgments": null}' % params_text).encode()
    ds = _dataset()  # (kept alive over the call: a request that parses goes on to read it)
    return clib._unwrap(clib._load().train_model(text, ds.pointer))


def _parses(params):
    """The request parser alone (the plan hook reads its payload with LambdaMARTParams::from_json and touches no device)."""
    return native.lambdamart_dart_plan(params, 1)


# --- wire form and the dataclass ---------------------------------------------------------------------

def test_the_keys_are_absent_at_their_defaults():
    p = LambdaMARTParams()
    assert (p.goss_top_rate, p.goss_other_rate) == (0.0, 0.1)
    assert list(p.to_dict().keys()) == KEYS
    assert list(clib.query_json("lambdamart_defaults")["params"]["LambdaMART"].keys()) == KEYS
    explicit = LambdaMARTParams(goss_top_rate=0.0, goss_other_rate=0.1)
    assert json.dumps(explicit.to_dict()) == json.dumps(p.to_dict())
    assert len(_parses(_params(goss_top_rate=0.0, goss_other_rate=0.1))) == 1  # (the defaults spelled out parse, on any grower)


@pytest.mark.parametrize("kw,written", [(dict(goss_top_rate=0.2), ["goss_top_rate"]),
                                        (dict(goss_top_rate=0.2, goss_other_rate=0.1), ["goss_top_rate"]),
                                        (dict(goss_top_rate=0.5, goss_other_rate=0.25), ["goss_top_rate", "goss_other_rate"]),
                                        (dict(goss_top_rate=0.5, goss_other_rate=0.5), ["goss_top_rate", "goss_other_rate"])])
def test_the_keys_round_trip(kw, written):
    req = TrainRequest.lambdamart()
    req.params = LambdaMARTParams(grower="histogram", split_gain="newton", **kw)
    d = req.to_dict()
    wire = d["params"]["LambdaMART"]
    assert list(wire.keys()) == KEYS + ["grower", "split_gain"] + written and all(wire[k] == kw[k] for k in written)
    back = TrainRequest.from_dict(json.loads(json.dumps(d)))
    assert back == req and all(getattr(back.params, k) == v for k, v in kw.items())
    assert req.clone() == req and req.clone() != TrainRequest.lambdamart()
    assert len(_parses(wire)) == 1  # the native parser takes the same payload


# --- refusals, before any device work ----------------------------------------------------------------

def _refused(params, text):
    for call in (lambda: _train_text(json.dumps(params)), lambda: _parses(params)):
        with pytest.raises(Exception, match="invalid value") as e:
            call()
        assert text in str(e.value) and "line: 0, column: 0" in str(e.value)


@pytest.mark.parametrize("value", [-0.1, -1e-300, 1.0, 1.5, 2, 1e308])
def test_a_top_rate_outside_its_range_is_refused(value):
    _refused(_params(goss_top_rate=value, **HIST), "goss_top_rate must be finite, at least 0 and less than 1")


@pytest.mark.parametrize("value", [0.0, 0, -0.1, 1.0000001, 3, 1e308])
def test_an_other_rate_outside_its_range_is_refused(value):
    _refused(_params(goss_top_rate=0.2, goss_other_rate=value, **HIST), "goss_other_rate must be finite, greater than 0 and at most 1")


@pytest.mark.parametrize("key", ["goss_top_rate", "goss_other_rate"])
@pytest.mark.parametrize("token", ["1e999", "-1e999", "NaN", "Infinity", "null", '"0.2"'])
def test_a_rate_that_is_no_finite_number_is_refused(key, token):
    """The JSON reader lets no infinity or NaN through (its own error points at the token); what it does let through and is
    no number is refused by name."""
    p = _params(goss_top_rate=0.2, **HIST)
    p.pop(key, None)
    text = json.dumps(p)[:-1] + ', "%s": %s}' % (key, token)
    with pytest.raises(Exception) as e:
        _train_text(text)
    assert key in str(e.value) or "line: 1" in str(e.value), str(e.value)


@pytest.mark.parametrize("a,b", [(float("nan"), 0.1), (float("inf"), 0.1), (0.2, float("nan")), (0.2, float("inf")), (0.0, 0.1), (1.0, 0.1),
                                 (0.2, 0.0), (0.6, 0.5)])
def test_the_debug_hooks_refuse_rates_that_reach_them_as_doubles(a, b):
    """The one way a non-finite rate can arrive: the hooks take doubles.  Refused before any device work."""
    ds = _dataset()
    with pytest.raises(Exception, match="top_rate must lie in"):
        native.goss_select(ds, np.zeros(8), a, b, 0, 0)
    with pytest.raises(Exception, match="top_rate must lie in"):
        native.hist_tree(ds, np.zeros(8), np.zeros(8), 4, 3, 1, split_gain="newton", goss=(a, b, 0, 0))


@pytest.mark.parametrize("a,b", [(0.5, 0.6), (0.9, 0.2), (0.99, 1.0), (0.2, 0.8000000000000002)])
def test_rates_that_sum_past_one_are_refused(a, b):
    assert not (np.float64(a) + np.float64(b) <= 1.0)
    _refused(_params(goss_top_rate=a, goss_other_rate=b, **HIST), "goss_top_rate + goss_other_rate must be at most 1")


def test_the_sum_is_taken_in_f64():
    for a, b in ((0.5, 0.5), (0.9, 0.1), (0.7, 0.3), (0.2, 0.8)):
        assert np.float64(a) + np.float64(b) <= 1.0
        assert len(_parses(_params(goss_top_rate=a, goss_other_rate=b, **HIST))) == 1


@pytest.mark.parametrize("kw", [dict(goss_other_rate=0.2), dict(goss_other_rate=0.5, goss_top_rate=0.0), dict(goss_other_rate=1.0, **HIST)])
def test_an_other_rate_needs_a_top_rate(kw):
    _refused(_params(**kw), "goss_other_rate needs goss_top_rate greater than 0")
    req = TrainRequest.lambdamart()
    for k, v in kw.items():
        setattr(req.params, k, v)
    with pytest.raises(Exception, match="goss_other_rate needs goss_top_rate greater than 0"):
        _dataset().train_model(req)


def test_goss_needs_the_histogram_grower_under_the_newton_gain():
    _refused(_params(goss_top_rate=0.2), "goss_top_rate needs grower: \"histogram\"")
    _refused(_params(goss_top_rate=0.2, split_gain="newton"), "split_gain `newton` needs grower")  # (the older rule speaks first)
    _refused(_params(goss_top_rate=0.2, grower="histogram"), "goss_top_rate needs split_gain: \"newton\"")
    _refused(_params(goss_top_rate=0.2, grower="histogram", split_gain="variance"), "goss_top_rate needs split_gain: \"newton\"")
    assert len(_parses(_params(goss_top_rate=0.2, **HIST))) == 1


def test_every_other_key_parses_with_goss():
    for extra in (dict(query_sampling_rate=0.5, feature_sampling_rate=0.5, seed=9), dict(validation_queries=["2"], early_stopping_rounds=2),
                  dict(max_leaves=31), dict(monotone_constraints={"0": 1}), dict(truncation_level=3, lambda_norm=True),
                  dict(objective="map"), dict(objective="mrr"), dict(objective="xendcg"), dict(drop_rate=0.1)):
        assert len(_parses(_params(goss_top_rate=0.2, goss_other_rate=0.3, **HIST, **extra))) == 1


# --- the key stream ----------------------------------------------------------------------------------

def test_the_key_stream_is_its_own():
    assert gm.GOSS_STREAM == int.from_bytes(b"GOSSGOSS", "big")
    assert len({gm.GOSS_STREAM, xm.XENDCG_STREAM, dm.DART_STREAM}) == 3
    from oracle import pyoracle as o
    for seed in (0, 1, 42, 2 ** 63, 2 ** 64 - 1):
        k = gm.keys(seed, 4)
        assert k != xm.keys(seed, 4) and k != [int(x) for x in o.rand64_stream(seed, 4)]
        assert k == gm.keys(seed, 6)[:4]


# --- properties of the restatement -------------------------------------------------------------------

def _designed(n, rng):
    """name -> lambda of n entries."""
    out = {"equal": np.full(n, 0.375), "zero": np.zeros(n), "signed zeros": np.where(np.arange(n) % 2 == 0, 0.0, -0.0),
           "opposite signs": np.where(np.arange(n) % 2 == 0, 1.5, -1.5) * np.where(np.arange(n) % 3 == 0, 2.0, 1.0),
           "denormals": (np.arange(n) % 5 + 1) * 5e-324 * np.where(np.arange(n) % 2 == 0, 1.0, -1.0),
           "continuous": rng.standard_normal(n)}
    half = rng.standard_normal(n)
    half[rng.random(n) < 0.5] = 0.0
    out["half zero"] = half
    return out


@pytest.mark.parametrize("n", [1, 2, 7, 1000])
@pytest.mark.parametrize("seed", [0, 5, 2 ** 64 - 1])
def test_the_top_set_is_exact_and_ties_enter_in_list_order(n, seed):
    rng = np.random.default_rng(n)
    ids = np.sort(rng.choice(4 * n + 8, size=n, replace=False))
    key = gm.keys(seed, 3)[2]
    for name, lam in _designed(n, rng).items():
        for a, b in ((0.2, 0.1), (0.5, 0.25), (1e-9, 0.5), (0.99, 0.01)):
            kept, top, tau, amp = gm.select(lam, ids, a, b, key)
            n_top, p, amp2 = gm.plan(n, a, b)
            k = gm.bit_keys(lam)
            assert amp == amp2 == (1.0 - a) / b and 1 <= n_top <= n and n_top == min(n, max(1, int(n * a)))
            assert int(top.sum()) == n_top, (name, a)
            assert np.all(np.diff(kept) > 0)
            in_top = np.zeros(n, dtype=bool)
            in_top[kept[top]] = True
            assert k[in_top].min() == tau and (n_top == n or k[~in_top].max() <= tau)  # every top key >= every other key
            ties = np.flatnonzero(k == tau)
            taken = in_top[ties]
            assert taken.any() and np.all(taken[: int(taken.sum())])  # the ties taken are the first ones of the list
            assert np.all(in_top[k > tau])
            # the others: exactly those with u < p, whatever their key
            u = gm.uniform(key, ids)
            assert np.array_equal(np.flatnonzero(in_top | (u < p)), kept)


def test_signed_zeros_and_opposite_signs_are_one_key():
    assert gm.bit_keys([0.0, -0.0, 1.5, -1.5]).tolist() == [0, 0, gm.bit_keys([1.5])[0], gm.bit_keys([1.5])[0]]
    lam = np.array([-2.0, 2.0, -2.0, 2.0, 1.0])
    kept, top, tau, _ = gm.select(lam, np.arange(5), 0.5, 0.5, 1)  # n_top = 2: the first two of the four tied entries
    assert tau == gm.bit_keys([2.0])[0] and kept[top].tolist() == [0, 1]


@pytest.mark.parametrize("a,b", [(0.5, 0.5), (0.25, 0.75), (0.75, 0.25)])
def test_rates_that_sum_to_one_keep_everything_unamplified(a, b):
    rng = np.random.default_rng(3)
    for n in (1, 2, 7, 1000):
        lam = rng.standard_normal(n)
        kept, top, _, amp = gm.select(lam, np.arange(n), a, b, gm.keys(n, 1)[0])
        assert gm.plan(n, a, b)[1:] == (1.0, 1.0) and amp == 1.0
        assert np.array_equal(kept, np.arange(n)) and int(top.sum()) == gm.plan(n, a, b)[0]
        lam2, wt2 = gm.amplified(lam, np.abs(lam), np.arange(n), kept, top, amp)
        assert lam2.tobytes() == lam.tobytes()


def test_a_document_has_one_uniform_whatever_list_it_is_in():
    """u hangs on the original instance id: a sampled view, whose lists are shorter, gives every document its parent's u."""
    key = gm.keys(17, 5)[4]
    parent_ids = np.arange(1000)
    view_ids = parent_ids[(parent_ids // 25) % 3 == 0]
    u_parent, u_view = gm.uniform(key, parent_ids), gm.uniform(key, view_ids)
    assert u_view.tobytes() == u_parent[view_ids].tobytes()
    assert np.all((u_parent >= 0.0) & (u_parent < 1.0)) and len(np.unique(u_parent)) == 1000
    rng = np.random.default_rng(8)
    lam = rng.standard_normal(1000)
    lam[view_ids] *= 1e-3  # (all of the view's documents are others of the parent's list too)
    kp, tp, _, _ = gm.select(lam, parent_ids, 0.2, 0.1, key)
    kv, tv, _, _ = gm.select(lam[view_ids], view_ids, 0.2, 0.1, key)
    parent_others, view_others = set(parent_ids[kp[~tp]].tolist()), set(view_ids[kv[~tv]].tolist())
    view_top = set(view_ids[kv[tv]].tolist())
    assert view_others == (parent_others & set(view_ids.tolist())) - view_top


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("a,b", [(0.2, 0.1), (0.1, 0.1), (0.5, 0.25)])
def test_the_kept_others_are_a_bernoulli_sample(seed, a, b):
    """Fixed seeds, for which the restatement satisfies the bound (a 5 sigma bound fails one seed in about two million)."""
    n = 20000
    lam = np.random.default_rng(seed).standard_normal(n)
    kept, top, _, _ = gm.select(lam, np.arange(n), a, b, gm.keys(seed, 1)[0])
    n_top, p, _ = gm.plan(n, a, b)
    others = n - n_top
    got = len(kept) - n_top
    assert abs(got - others * p) <= 5.0 * np.sqrt(others * p * (1.0 - p)), (got, others * p)


@pytest.mark.parametrize("a,b", [(0.2, 0.1), (0.5, 0.25)])
def test_the_amplified_sum_is_unbiased(a, b):
    """Sum of lambda' over the GOSS list against the sum of lambda over L, over 200 seeds at n_t = 1000: the mean difference
    lies within 5 s / sqrt(200) of zero, s the differences' own standard deviation.  An amplification of the wrong direction
    (b / (1 - a)) or scale (1 / b) misses this by tens of s / sqrt(200): the others' sum would be off by a factor."""
    n = 1000
    rng = np.random.default_rng(2024)
    lam = rng.standard_normal(n) + 0.5  # (a non-zero mean: a wrong scale moves the sum)
    ids = np.arange(n)
    full = float(np.sum(lam))
    diffs = []
    for seed in range(200):
        kept, top, _, amp = gm.select(lam, ids, a, b, gm.keys(seed, 1)[0])
        lam2, _ = gm.amplified(lam, lam, ids, kept, top, amp)
        diffs.append(float(np.sum(lam2[kept])) - full)
    diffs = np.asarray(diffs)
    s = float(np.std(diffs, ddof=1))
    assert s > 0.0 and abs(float(np.mean(diffs))) <= 5.0 * s / np.sqrt(200.0), (float(np.mean(diffs)), s)
    # ... and the check has teeth: the same lists amplified by 1 / b miss it
    wrong = []
    for seed in range(200):
        kept, top, _, _ = gm.select(lam, ids, a, b, gm.keys(seed, 1)[0])
        lam2, _ = gm.amplified(lam, lam, ids, kept, top, 1.0 / b)
        wrong.append(float(np.sum(lam2[kept])) - full)
    assert abs(float(np.mean(wrong))) > 5.0 * float(np.std(wrong, ddof=1)) / np.sqrt(200.0)


# --- the header under the sanitizers ------------------------------------------------------------------

def test_goss_header_under_address_and_undefined_sanitizers(tmp_path):
    """tests/lambdamart_goss_sanitize.cpp: a program of its own over csrc/lambdamart_goss.hpp, built with
    -fsanitize=address,undefined and run directly."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "lambdamart_goss_sanitize")
    build = subprocess.run([cxx, "-std=c++17", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                            "-I", os.path.join(here, "..", "fastrank_amd", "csrc"), os.path.join(here, "lambdamart_goss_sanitize.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "lambdamart_goss ok" in run.stdout, run.stdout
