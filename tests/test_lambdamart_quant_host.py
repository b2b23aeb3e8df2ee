"""LambdaMART's quantised gradients on the CPU ("Quantised gradients"): the key's wire form and
refusals, the Python dataclass, the key stream, and the properties of the numpy restatement
(tests/lambdamart_quant_model.py) that the device tests hold the kernels to; the host header also runs on its own under the
address and undefined-behaviour sanitizers (tests/lambdamart_quant_sanitize.cpp).
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
from oracle import pyoracle as o
from tests import lambdamart_dart_model as dm
from tests import lambdamart_goss_model as gm
from tests import lambdamart_quant_model as qm
from tests import lambdamart_xendcg_model as xm

KEYS = ["num_trees", "learning_rate", "max_depth", "min_leaf_support", "split_candidates", "sigma", "quiet"]
HIST = dict(grower="histogram", split_gain="newton")
UNDECIDED = "it is not decided whether those would read the quantised sums or the full-precision ones"


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

def test_the_key_is_absent_at_its_default():
    p = LambdaMARTParams()
    assert p.grad_quant_bits == 0
    assert list(p.to_dict().keys()) == KEYS
    assert list(clib.query_json("lambdamart_defaults")["params"]["LambdaMART"].keys()) == KEYS
    assert json.dumps(LambdaMARTParams(grad_quant_bits=0).to_dict()) == json.dumps(p.to_dict())
    assert len(_parses(_params(grad_quant_bits=0))) == 1  # (the default spelled out parses, on any grower)


@pytest.mark.parametrize("bits", [2, 3, 4, 5, 6, 7, 8])
def test_the_key_round_trips(bits):
    req = TrainRequest.lambdamart()
    req.params = LambdaMARTParams(grower="histogram", split_gain="newton", grad_quant_bits=bits)
    d = req.to_dict()
    wire = d["params"]["LambdaMART"]
    assert list(wire.keys()) == KEYS + ["grower", "split_gain", "grad_quant_bits"] and wire["grad_quant_bits"] == bits
    back = TrainRequest.from_dict(json.loads(json.dumps(d)))
    assert back == req and back.params.grad_quant_bits == bits
    assert req.clone() == req and req.clone() != TrainRequest.lambdamart()
    assert len(_parses(wire)) == 1  # the native parser takes the same payload


# --- refusals, before any device work ----------------------------------------------------------------

def _refused(params, text):
    for call in (lambda: _train_text(json.dumps(params)), lambda: _parses(params)):
        with pytest.raises(Exception, match="invalid value") as e:
            call()
        assert text in str(e.value) and "grad_quant_bits" in str(e.value) and "line: 0, column: 0" in str(e.value)


@pytest.mark.parametrize("value", [1, 9, 16, 64, 2 ** 32 - 1])
def test_a_width_outside_its_range_is_refused(value):
    _refused(_params(grad_quant_bits=value, **HIST), "grad_quant_bits must be 0 (off) or between 2 and 8")


@pytest.mark.parametrize("token", ["-1", "2.5", "1e999", "null", '"4"', "true", str(2 ** 32)])
def test_a_width_that_is_no_u32_is_refused(token):
    """What is no u32 never becomes a width: the JSON reader's or the u32 reader's own error (the one every u32 key gets)."""
    text = json.dumps(_params(**HIST))[:-1] + ', "grad_quant_bits": %s}' % token
    with pytest.raises(Exception) as e:
        _train_text(text)
    assert "grad_quant_bits" in str(e.value) or "line: 1" in str(e.value) or "expected u32" in str(e.value), str(e.value)


def test_the_key_needs_the_histogram_grower_under_the_newton_gain():
    _refused(_params(grad_quant_bits=4), "grad_quant_bits needs grower: \"histogram\"")
    _refused(_params(grad_quant_bits=4, grower="exact"), "grad_quant_bits needs grower: \"histogram\"")
    _refused(_params(grad_quant_bits=4, grower="histogram"), "grad_quant_bits needs split_gain: \"newton\"")
    _refused(_params(grad_quant_bits=4, grower="histogram", split_gain="variance"), "grad_quant_bits needs split_gain: \"newton\"")
    assert len(_parses(_params(grad_quant_bits=4, **HIST))) == 1


@pytest.mark.parametrize("extra,key", [(dict(monotone_constraints={"0": 1}), "monotone_constraints"), (dict(lambda_l1=0.5), "lambda_l1"),
                                       (dict(max_delta_step=1.0), "max_delta_step"), (dict(path_smooth=2.0), "path_smooth")])
def test_the_keys_whose_nodes_carry_outputs_are_refused(extra, key):
    _refused(_params(grad_quant_bits=4, **HIST, **extra), "grad_quant_bits cannot be combined with " + key)
    _refused(_params(grad_quant_bits=4, **HIST, **extra), UNDECIDED)
    assert len(_parses(_params(**HIST, **extra))) == 1 and len(_parses(_params(grad_quant_bits=0, **HIST, **extra))) == 1


def test_the_dataclass_request_is_refused_like_the_text():
    req = TrainRequest.lambdamart()
    req.params.grad_quant_bits = 4
    with pytest.raises(Exception, match="grad_quant_bits needs grower"):
        _dataset().train_model(req)


def test_every_other_key_parses_with_the_key():
    for extra in (dict(query_sampling_rate=0.5, feature_sampling_rate=0.5, seed=9), dict(validation_queries=["2"], early_stopping_rounds=2),
                  dict(max_leaves=31), dict(symmetric_trees=True), dict(truncation_level=3, lambda_norm=True), dict(objective="map"),
                  dict(objective="mrr"), dict(objective="xendcg"), dict(drop_rate=0.1), dict(goss_top_rate=0.2, goss_other_rate=0.3),
                  dict(lambda_l2=0.5, min_sum_hessian=0.25, min_split_gain=0.125)):
        assert len(_parses(_params(grad_quant_bits=3, **HIST, **extra))) == 1


def test_the_debug_hooks_refuse_what_reaches_them():
    ds = _dataset()
    one = np.ones(8)
    for bits in (0, 1, 9):
        with pytest.raises(Exception, match="between 2 and 8"):
            native.hist_tree(ds, one, one, 4, 3, 1, split_gain="newton", quant=(bits, 0, 0))
        with pytest.raises(Exception, match="between 2 and 8"):
            native.hist_quantise(ds, one, one, bits, 0, 0)
    with pytest.raises(Exception, match="between 2 and 8"):
        native.hist_root_histogram(ds, one, one, 4, quant=(9, 0, 0))
    with pytest.raises(ValueError, match="quant needs split_gain='newton'"):
        native.hist_tree(ds, one, one, 4, 3, 1, quant=(4, 0, 0))
    with pytest.raises(ValueError, match="quant needs split_gain='newton'"):
        native.hist_tree(ds, one, one, 4, 3, 1, split_gain="newton", lambda_l1=0.5, quant=(4, 0, 0))
    opt = clib.HistTreeOptions(split_candidates=4, max_depth=3, min_leaf_support=1, quant_bits=4)  # (past the Python checks)
    with pytest.raises(Exception, match="quantised gradients need the Newton gain"):
        clib._unwrap(clib._load().fr_debug_hist_tree(ds.pointer, opt, one.ctypes.data, one.ctypes.data, 8, None))


# --- the key stream ----------------------------------------------------------------------------------

def test_the_key_stream_is_its_own():
    assert qm.QUANT_STREAM == int.from_bytes(b"QUANTGRD", "big")
    assert len({qm.QUANT_STREAM, gm.GOSS_STREAM, xm.XENDCG_STREAM, dm.DART_STREAM}) == 4
    for seed in (0, 1, 42, 2 ** 63, 2 ** 64 - 1):
        k = qm.keys(seed, 4)
        assert k not in (gm.keys(seed, 4), xm.keys(seed, 4), [int(x) for x in o.rand64_stream(seed, 4)])
        assert k not in ([int(x) for x in o.rand64_stream((seed ^ dm.DART_STREAM) & qm.MASK, 4)],)
        assert k == qm.keys(seed, 6)[:4]


def test_the_other_streams_stay_where_they_were():
    """The sample, the DART plan, the listwise keys and the GOSS keys of a request are those of the request without the key."""
    base = _params(num_trees=6, seed=77, query_sampling_rate=0.5, feature_sampling_rate=0.5, drop_rate=0.5, skip_drop=0.0, **HIST)
    with_key = dict(base, grad_quant_bits=4)
    assert repr(native.lambdamart_dart_plan(with_key, 6)) == repr(native.lambdamart_dart_plan(base, 6))
    ds = _dataset()
    for t in range(6):
        assert repr(native.lambdamart_sample(ds, with_key, t)) == repr(native.lambdamart_sample(ds, base, t))
    assert gm.keys(77, 6) == [int(x) for x in o.rand64_stream(77 ^ gm.GOSS_STREAM, 6)]
    assert xm.keys(77, 6) == [int(x) for x in o.rand64_stream(77 ^ xm.XENDCG_STREAM, 6)]


# --- properties of the restatement -------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 4, 255, 256, 2 ** 13 - 1, 2 ** 13, 2 ** 22 - 1, 2 ** 22, 2 ** 31 - 1])
def test_the_shifts(n):
    c = 1 if n == 1 else int(np.floor(np.log2(n))) + 1
    assert n.bit_length() == c
    for b in range(2, 9):
        d, dw = qm.shifts(n, b)
        assert (d, dw) == (62 - c - b, 61 - c - b) and dw >= 22 and d <= 59


def _extremes(n, b):
    c = n.bit_length()
    return 1 << (61 - c), 1 << (b - 1), 1 << b


@pytest.mark.parametrize("b", [2, 4, 8])
@pytest.mark.parametrize("n", [1, 2, 1000, 3800000])
def test_ranges_extremes_multiples_and_zeros(n, b):
    top, qmax, wmax = _extremes(n, b)
    d, dw = qm.shifts(n, b)
    rng = np.random.default_rng(n + b)
    m = 400
    ids = rng.integers(0, 2 ** 32, m)
    for key in qm.keys(n + b, 3) + [0, qm.MASK]:
        # shifts are a function of the list's length: fake a list of n entries by its length alone
        def quant(Q, W):
            q = [(int(v) + r) >> d for v, r in zip(Q, qm.offsets(key, ids, 1, d))]
            w = [(int(v) + r) >> dw for v, r in zip(W, qm.offsets(key, ids, 2, dw))]
            return np.asarray(q), np.asarray(w)
        assert all(0 <= r < 2 ** d for r in qm.offsets(key, ids, 1, d)) and all(0 <= r < 2 ** dw for r in qm.offsets(key, ids, 2, dw))
        Q = [int(x) for x in rng.integers(-top, top + 1, m)]
        W = [int(x) for x in rng.integers(0, top + 1, m)]
        q, w = quant(Q, W)
        assert q.min() >= -qmax and q.max() <= qmax and w.min() >= 0 and w.max() <= wmax
        # both extremes, whatever the key
        q, w = quant([top] * m, [top] * m)
        assert np.all(q == qmax) and np.all(w == wmax)
        q, w = quant([-top] * m, [0] * m)
        assert np.all(q == -qmax) and np.all(w == 0)  # (all-zero w stays all zero)
        # a multiple of 2^d is Q >> d for every key
        mult = [int(x) << d for x in rng.integers(-qmax, qmax + 1, m)]
        multw = [int(x) << dw for x in rng.integers(0, wmax + 1, m)]
        q, w = quant(mult, multw)
        assert q.tolist() == [x >> d for x in mult] and w.tolist() == [x >> dw for x in multw]


def test_quantise_reads_the_lists_length_and_the_original_ids():
    n = 1000
    rng = np.random.default_rng(4)
    Q = rng.integers(-2 ** 40, 2 ** 40, n)
    W = rng.integers(0, 2 ** 40, n)
    parent_ids = np.arange(n)
    key = qm.keys(17, 5)[4]
    q, w, d, dw = qm.quantise(Q, W, parent_ids, 4, key)
    assert (d, dw) == qm.shifts(n, 4)
    # a document's offsets hang on its original id alone: a sub-list of 512..1023 entries (the same c) gets its parent's values
    keep = np.flatnonzero(rng.random(n) < 0.7)
    assert len(keep).bit_length() == n.bit_length()
    q2, w2, _, _ = qm.quantise(Q[keep], W[keep], parent_ids[keep], 4, key)
    assert np.array_equal(q2, q[keep]) and np.array_equal(w2, w[keep])
    # another key, another tree: other values
    q3, _, _, _ = qm.quantise(Q, W, parent_ids, 4, qm.keys(17, 6)[5])
    assert not np.array_equal(q3, q)


@pytest.mark.parametrize("b", [2, 4, 8])
def test_the_mean_over_keys_is_unbiased(b):
    """200 keys: the mean of q lies within 5 sigma of Q / 2^d, sigma^2 = f (1 - f) / 200 for the fraction f.  Rounding to
    nearest, or truncation, misses this for f = 0.25 by tens of sigma."""
    n = 3800000
    d, dw = qm.shifts(n, b)
    ks = qm.keys(b, 200)
    for frac in (-0.75, 0.25, 0.5, 1.0 - 2.0 ** -20):
        Q = int(frac * 2 ** d)
        W = int(abs(frac) * 2 ** dw)
        for doc in (0, 12345, 2 ** 32 - 1):
            qs = [(Q + qm.offsets(k, [doc], 1, d)[0]) >> d for k in ks]
            ws = [(W + qm.offsets(k, [doc], 2, dw)[0]) >> dw for k in ks]
            for got, want in ((np.mean(qs), Q / 2 ** d), (np.mean(ws), W / 2 ** dw)):
                f = want - np.floor(want)
                assert abs(got - want) <= 5.0 * np.sqrt(f * (1.0 - f) / 200.0) + 1e-12, (frac, doc, got, want)
    # the issue's figure: 20 000 ids of Q = -0.75 2^d at n = 3.8 M
    Q = int(-0.75 * 2 ** d)
    mean = np.mean([(Q + r) >> d for r in qm.offsets(ks[0], range(20000), 1, d)])
    assert abs(mean + 0.75) <= 5.0 * np.sqrt(0.25 * 0.75 / 20000.0)


def test_renewed_leaves_are_the_full_precision_formula():
    rng = np.random.default_rng(9)
    n = 600
    X = rng.random((n, 3)).astype(np.float32)
    lam = rng.standard_normal(n)
    wt = rng.random(n) + 0.01
    ids = np.arange(n)
    t = qm.fit_tree(X, lam, wt, ids, [0, 1, 2], 4, 5, 16, 3, qm.keys(1, 1)[0], lambda_l2=0.5)
    from tests import lambdamart_newton_model as nm
    plain = nm.fit_tree(X, lam, wt, ids, [0, 1, 2], 4, 5, 16, lambda_l2=0.5)
    assert "FeatureSplit" in t and t != plain
    Q, S, W, Sw = nm.quantise_pair(lam, wt, n)

    def walk(node, at):
        if "LeafNode" in node:
            assert node["LeafNode"] == nm.leaf_value(int(Q[at].sum()), int(W[at].sum()), S, Sw, 0.5)
            return 1
        sp = node["FeatureSplit"]
        left = X[at, sp["fid"]] <= np.float32(sp["split"])
        assert left.any() and (~left).any()
        return walk(sp["lhs"], at[left]) + walk(sp["rhs"], at[~left])
    assert walk(t, ids) >= 2
    # with enough bits the shape is the unquantised tree's on this small list, and the leaves are then the same numbers
    wide = qm.fit_tree(X, lam, wt, ids, [0, 1, 2], 2, 5, 16, 8, qm.keys(1, 1)[0], lambda_l2=0.5)
    narrow = nm.fit_tree(X, lam, wt, ids, [0, 1, 2], 2, 5, 16, lambda_l2=0.5)
    if wide["FeatureSplit"]["fid"] == narrow["FeatureSplit"]["fid"] and wide["FeatureSplit"]["split"] == narrow["FeatureSplit"]["split"]:
        assert wide == narrow
    assert qm.fit_tree(X, np.zeros(n), wt, ids, [0, 1, 2], 4, 5, 16, 3, 1) == {"LeafNode": 0.0}


# --- the header under the sanitizers ------------------------------------------------------------------

def test_quant_header_under_address_and_undefined_sanitizers(tmp_path):
    """tests/lambdamart_quant_sanitize.cpp: a program of its own over csrc/lambdamart_quant.hpp -- the arithmetic, the packed
    cell at 8 192 entries of each extreme for 2 and 8 bits, the key stream -- built with -fsanitize=address,undefined and run
    directly."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "lambdamart_quant_sanitize")
    build = subprocess.run([cxx, "-std=c++17", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                            "-I", os.path.join(here, "..", "fastrank_amd", "csrc"), os.path.join(here, "lambdamart_quant_sanitize.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "lambdamart_quant ok" in run.stdout, run.stdout
