"""Feature normalisation without a device: the numpy restatement (tests/normalize_model.py) against the
reference's known answer, against the plain sequential loop, and against exact rationals under a bound derived from its own
operations; the wire form; the calls' behaviour without a device; csrc/normalize_host.hpp under the sanitizers."""
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import native
from tests import normalize_model as nm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_DEVICE = "no MI355X/HIP device available"


def _column(kind, m, seed):
    rng = np.random.default_rng(seed)
    if kind == "normal":
        x = rng.normal(size=m)
    elif kind == "near_1e6":
        x = 1e6 + 0.0625 * rng.integers(-3, 4, size=m)  # (0.0625 = one unit in the last place of an f32 there)
    elif kind == "counts":
        x = np.round(rng.exponential(size=m) * 3)
    else:
        x = np.full(m, 7.25)
    return x.astype(np.float32), rng.random(m) < 0.7


def test_reference_known_answer():
    """src/stats.rs:178-190"""
    st = nm.finish(nm.sequential([0, 1, 1, 0]))
    assert st["mean"] == 0.5 and st["max"] == 1.0 and st["min"] == 0.0 and st["total"] == 2.0 and st["num_elements"] == 4
    assert abs(st["variance"] - 0.33333) < 1e-5 and abs(np.sqrt(st["variance"]) - 0.57735) < 1e-5
    assert st["variance"] == 1.0 / 3.0
    assert nm.finish(nm.sequential([3.0])) is None and nm.finish(nm.sequential([])) is None


@pytest.mark.parametrize("m", [1, 2, 255, 256])
@pytest.mark.parametrize("kind", ["normal", "near_1e6", "counts", "constant"])
def test_one_chunk_is_the_sequential_loop(kind, m):
    x, held = _column(kind, m, 100 + m)
    want = nm.sequential([v for v, h in zip(x, held) if h])
    assert nm.chunked(list(x), list(held)) == want
    rec = nm.dataset_records(x.reshape(m, 1), held.reshape(m, 1))
    got = [int(rec["n"][0])] + [float(rec[k][0]) for k in ("mean", "s", "max", "min", "total")]
    assert [float.hex(float(v)) for v in got] == [float.hex(float(v)) for v in want]


def test_vectorised_form_is_the_scalar_form():
    rng = np.random.default_rng(5)
    X = rng.normal(size=(700, 6)).astype(np.float32)
    H = rng.random((700, 6)) < 0.6
    H[256:512, 2] = False   # absent from one whole chunk
    H[:, 3] = False          # held nowhere
    H[:, 4] = False
    H[600, 4] = True         # held once
    rec = nm.dataset_records(X, H)
    for f in range(6):
        want = nm.chunked(list(X[:, f]), list(H[:, f]))
        got = [int(rec["n"][f])] + [float(rec[k][f]) for k in ("mean", "s", "max", "min", "total")]
        assert got == want
    st = nm.fit(X, H, np.arange(700), range(6))
    assert sorted(st) == [0, 1, 2, 5]


_WORST = {}


@pytest.mark.parametrize("m", [257, 513, 20000])
@pytest.mark.parametrize("kind", ["normal", "near_1e6", "counts", "constant"])
def test_mean_and_variance_within_the_derived_bound(kind, m):
    x, held = _column(kind, m, 7 * m + len(kind))
    rec, em, ev = nm.bounded_column(list(x), list(held))
    assert rec == nm.chunked(list(x), list(held))  # (the bounded walk computes the restatement's own floats)
    mu, var = nm.exact_column(list(x), list(held))
    err_m = abs(Fraction(rec[1]) - mu)
    err_v = abs(Fraction(rec[2] / float(rec[0] - 1)) - var)
    rm = float(err_m / em) if em else 0.0
    rv = float(err_v / ev) if ev else 0.0
    rel_v = float(err_v / var) if var else float(err_v)
    print("%s m=%d held=%d: mean error %.3e (bound %.3e), variance error %.3e (bound %.3e, relative error %.3e)"
          % (kind, m, rec[0], float(err_m), float(em), float(err_v), float(ev), rel_v))
    _WORST[(kind, m)] = (rm, rv, rel_v)
    assert err_m <= em and err_v <= ev
    if kind == "constant":
        assert rec[2] == 0.0 and err_m == 0


def test_constant_column_maps_to_zero():
    x = np.full((600, 1), 7.25, dtype=np.float32)
    H = np.ones((600, 1), dtype=bool)
    st = nm.fit(x, H, np.arange(600), [0])
    assert st[0]["variance"] == 0.0 and st[0]["max"] == st[0]["min"] == 7.25
    for method in ("zscore", "maxmin"):
        out = nm.apply(x, H, st, method)
        assert out.dtype == np.float32 and not out.any() and not np.signbit(out).any()
    assert not nm.per_query(x, H, np.arange(600) // 7, "zscore").any()


def test_per_value_functions():
    X = np.array([[1.0, 3e38, 5.0], [3.0, -3e38, 5.0], [np.inf, 0.0, 6.0]], dtype=np.float32)
    H = np.ones(X.shape, dtype=bool)
    H[2, 2] = False
    st = {0: {"mean": 2.0, "variance": 2.0, "max": 3.0, "min": 1.0}, 1: {"mean": 0.0, "variance": 1.0, "max": 3e38, "min": -3e38}}
    out = nm.apply(X, H, st, "maxmin")
    assert out[0, 0] == 0.0 and out[1, 0] == 1.0 and out[2, 0] == np.inf      # inf passes through the arithmetic
    assert np.isnan(out[0, 1]) and nm.first_nan(out, H) == (0, 1)            # the range overflows f32: inf / inf
    assert out[0, 2] == 5.0 and out[2, 2] == 0.0                              # no record: unchanged; absent: 0.0
    z = nm.apply(X, H, st, "zscore")
    assert z[0, 0] == (np.float32(1.0) - np.float32(2.0)) / np.float32(np.sqrt(2.0))
    assert nm.sigmoid_value(0.0) == 0.5 and nm.sigmoid_value(np.inf) == 1.0 and nm.sigmoid_value(-np.inf) == 0.0
    # (exp(-103) = 1.9e-45 rounds to the smallest f32 denormal, exp(-104) = 6.8e-46 lies below half of it)
    assert nm.sigmoid_value(-103.0) > 0.0 and nm.sigmoid_value(-104.0) == 0.0 and nm.sigmoid_value(88.0) == 1.0 and np.isnan(nm.sigmoid_value(np.nan))


def test_wire_form_round_trips_bit_for_bit():
    awkward = [5e-324, 2.2250738585072014e-308, 1.0 / 3.0, 0.1, 1e22, 1.7976931348623157e308, -0.0, 123456789.12345679, 2.0 ** -30]
    stats = {}
    for i, v in enumerate(awkward):
        stats[str(i * 7)] = {"num_elements": 2 + i, "mean": v, "variance": abs(v), "max": v, "min": -v, "total": v * 3 if np.isfinite(v * 3) else v}
    for name in ("ZScoreNormalizer", "MaxMinNormalizer"):
        n = fr.Normalizer.from_dict({name: {"feature_stats": stats}})
        back = fr.Normalizer.from_dict(n.to_dict()).to_dict()
        assert list(back) == [name]
        for fid, rec in stats.items():
            for key in nm.KEYS[1:]:
                assert float.hex(back[name]["feature_stats"][fid][key]) == float.hex(float(rec[key]))
            assert back[name]["feature_stats"][fid]["num_elements"] == rec["num_elements"]
        assert n.feature_stats()[7]["mean"] == awkward[1]
    assert fr.Normalizer.sigmoid().to_dict() == {"SigmoidNormalizer": []}
    assert fr.Normalizer.per_query("zscore").to_dict() == {"PerQuery": "zscore"}
    assert fr.Normalizer.per_query("linear").to_dict() == {"PerQuery": "maxmin"}
    assert fr.Normalizer.from_dict({"PerQuery": "linear"}).to_dict() == {"PerQuery": "maxmin"}
    assert fr.Normalizer.sigmoid().feature_stats() == {}


def test_wire_form_refusals():
    good = {"num_elements": 3, "mean": 1.0, "variance": 1.0, "max": 2.0, "min": 0.0, "total": 3.0}
    for key in nm.KEYS[1:]:
        for bad in (float("nan"), float("inf"), -float("inf"), None, "1.0"):
            rec = dict(good)
            rec[key] = bad
            with pytest.raises(Exception, match="no finite number for " + key):
                fr.Normalizer.from_dict({"ZScoreNormalizer": {"feature_stats": {"4": rec}}})
    with pytest.raises(Exception, match="Unsupported Normalizer: RobustNormalizer"):
        fr.Normalizer.from_dict({"RobustNormalizer": {"feature_stats": {}}})
    with pytest.raises(Exception, match="Unsupported Normalizer: robust"):
        fr.Normalizer.from_dict({"PerQuery": "robust"})
    with pytest.raises(Exception, match="Unsupported Normalizer: robust"):
        fr.Normalizer.per_query("robust")
    with pytest.raises(Exception, match="Unsupported Normalizer: sigmoid"):
        fr.Normalizer.per_query("sigmoid")
    with pytest.raises(Exception, match="feature_stats"):
        fr.Normalizer.from_dict({"MaxMinNormalizer": {}})
    with pytest.raises(Exception, match="Unsupported Normalizer"):
        fr.Normalizer.from_dict({"ZScoreNormalizer": {"feature_stats": {}}, "MaxMinNormalizer": {"feature_stats": {}}})


def _small():
    rng = np.random.default_rng(3)
    X = rng.normal(size=(12, 3)).astype(np.float32)
    return fr.CDataset.from_numpy(X, rng.integers(0, 3, size=12).astype(np.float64), (np.arange(12) // 4).astype(np.int64))


def test_library_refuses_before_any_device():
    """what the library decides from its arguments alone: the method, the normaliser's JSON, a view, a null handle"""
    ds = _small()
    lib = native._load()
    with pytest.raises(Exception, match="Unsupported Normalizer: robust"):
        native._json_reply(lib.fr_fit_normalizer(ds.pointer, b"robust"))
    with pytest.raises(Exception, match="Dataset pointer is null"):
        native._json_reply(lib.fr_fit_normalizer(None, b"zscore"))
    assert native._json_reply(lib.fr_fit_normalizer(ds.pointer, b"sigmoid")) == {"SigmoidNormalizer": []}
    for text, needle in ((b'{"RobustNormalizer": {}}', "Unsupported Normalizer: RobustNormalizer"), (b'{"PerQuery": "robust"}', "Unsupported Normalizer: robust"),
                         (b'{"ZScoreNormalizer": {"feature_stats": {"1": {"num_elements": 2, "mean": null}}}}', "no finite number for mean"),
                         (b'{"ZScoreNormalizer": ', "EOF")):
        with pytest.raises(Exception, match=needle):
            fr.clib._unwrap(lib.fr_normalize_dataset(ds.pointer, text))
    view = ds.subsample_queries(["0", "2"])
    with pytest.raises(Exception, match="normalise the whole dataset, then sample it"):
        fr.Normalizer.sigmoid().apply(view)
    with pytest.raises(Exception, match="normalise the whole dataset, then sample it"):
        fr.Normalizer.per_query("zscore").apply(ds.subsample_feature_names(["0", "1"]))
    assert ds.normalization() is None and view.normalization() is None


@pytest.mark.skipif(native.device_count() > 0, reason="checks the no-GPU failure mode")
def test_fit_and_apply_without_gpu_fail_loudly():
    ds = _small()
    for call in (lambda: fr.Normalizer.fit(ds, "zscore"), lambda: fr.Normalizer.fit(ds, "linear"), lambda: ds.feature_stats(),
                 lambda: fr.Normalizer.sigmoid().apply(ds), lambda: fr.Normalizer.per_query("maxmin").apply(ds),
                 lambda: fr.Normalizer.from_dict({"ZScoreNormalizer": {"feature_stats": {}}}).apply(ds)):
        with pytest.raises(Exception, match=NO_DEVICE):
            call()


def test_host_header_under_address_and_undefined_sanitizers(tmp_path):
    """tests/normalize_host_sanitize.cpp: a program of its own over csrc/normalize_host.hpp (empty chunks, a feature held
    nowhere, a fold of one record, malformed JSON), built with -fsanitize=address,undefined and run directly."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "normalize_host_sanitize")
    build = subprocess.run([cxx, "-std=c++17", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                            "-I", os.path.join(here, "..", "fastrank_amd", "csrc"), os.path.join(here, "normalize_host_sanitize.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "normalize_host ok" in run.stdout, run.stdout


def test_recorded_error_figures_are_current():
    """profiles/normalize_stats_error.txt holds the largest error / bound of the bound test's cases; rewritten with
    FR_WRITE_PROFILES=1 after that test ran in this process, otherwise only read."""
    path = os.path.join(ROOT, "profiles", "normalize_stats_error.txt")
    if os.environ.get("FR_WRITE_PROFILES") and len(_WORST) == 12:
        with open(path, "w") as fh:
            fh.write("Chunked statistics (256-instance chunks folded in order, tests/normalize_model.py) against exact rationals:\n")
            fh.write("error / derived bound (tests/test_normalize_host.py::test_mean_and_variance_within_the_derived_bound), 70 % held.\n")
            fh.write("kind m mean_error/bound variance_error/bound variance_relative_error\n")
            for (kind, m), (rm, rv, rel) in sorted(_WORST.items()):
                fh.write("%s %d %.3e %.3e %.3e\n" % (kind, m, rm, rv, rel))
            fh.write("largest mean_error/bound %.3e, largest variance_error/bound %.3e\n" % (max(v[0] for v in _WORST.values()), max(v[1] for v in _WORST.values())))
    text = open(path).read()
    assert "largest mean_error/bound" in text
    largest = [float(w) for w in text.strip().splitlines()[-1].replace(",", " ").split() if w[0].isdigit()]
    assert len(largest) == 2 and all(0.0 <= v <= 1.0 for v in largest)
