"""The device text parser without a device ("Text loading"): the Python restatement of its grammar and value rule
(tests/ranksvm_text_cases.py) against numpy's correctly rounded parse, the library's host compile of the same rule against the
restatement, the parser switch of open_ranksvm, and the host merge header under ASan + UBSan."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import native
from tests import ranksvm_text_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_TRAIN = os.path.join(ROOT, "tests", "golden", "data", "trec_news_2018.train")
NO_DEVICE = "no MI355X/HIP device available"


def _tokens():
    rng = np.random.default_rng(20261020)
    return tc.random_tokens(rng, 42000) + tc.midpoints(rng, 9, 500) + tc.midpoints(rng, 17, 500) + tc.EDGE_VALUES


@pytest.fixture(scope="module")
def restated():
    toks = _tokens()
    return toks, [tc.fast_number(t.encode()) for t in toks]


def test_every_unflagged_token_has_the_bits_of_the_correctly_rounded_parse(restated):
    toks, got = restated
    kept = [(t, v) for t, (r, v) in zip(toks, got) if r == "none"]
    assert len(kept) > len(toks) // 2, len(kept)   # (the rule is of use: most tokens stay on the device)
    for t, v in kept:
        assert np.float32(v).tobytes() == tc.exact_f32_bytes(t), (t, v)                # strtof's value (-0 included)
        assert np.float32(v).tobytes() == np.float32(np.float64(t)).tobytes(), (t, v)  # and (float)strtod, as the label is read
    reasons = {r for r, _ in got}
    assert {"none", "number", "range", "near_tie"} <= reasons
    by_tok = dict(zip(toks, (r for r, _ in got)))
    assert by_tok["16777217"] == "near_tie" and by_tok["12345678901234567890"] == "number" and by_tok["1e-40"] == "range"
    assert by_tok["1e39"] == "range" and by_tok["inf"] == by_tok["nan"] == by_tok["0x1p3"] == "number"
    assert [by_tok[t] for t in ("+1", "-0", ".5", "5.", "1e5")] == ["none"] * 5
    for digits in (9, 17):   # an exact f32 midpoint is never kept
        assert all(tc.fast_number(t.encode())[0] == "near_tie" for t in tc.exact_midpoints(np.random.default_rng(digits), digits, 200))


def test_the_librarys_host_compile_of_the_rule_is_the_restatement(restated):
    toks, got = restated
    names, v64, v32 = native.text_numbers(toks)
    assert names == [r for r, _ in got]
    keep = np.array([r == "none" for r, _ in got])
    want = np.array([v if v is not None else 0.0 for _, v in got], dtype=np.float64)
    assert v64[keep].tobytes() == want[keep].tobytes()
    assert v32[keep].tobytes() == want[keep].astype(np.float32).tobytes()


def test_the_golden_file_stays_inside_the_fast_grammar():
    text = open(GOLDEN_TRAIN, "rb").read()
    stats_limit = native.last_load_stats()["stage_limit"]
    reasons = tc.text_reasons(text, stats_limit)
    assert len(reasons) == 782 and reasons.count("none") == 782, {r: reasons.count(r) for r in set(reasons)}


def _same_arrays(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
        else:
            assert a[k] == b[k], k


def test_parser_host_is_the_default_on_the_golden_file():
    default = native.loaded_arrays(fr.CDataset.open_ranksvm(GOLDEN_TRAIN))
    assert native.last_load_stats()["parser"] == "host"   # (far below the threshold, with or without a device)
    host = native.loaded_arrays(fr.CDataset.open_ranksvm(GOLDEN_TRAIN, parser="host"))
    st = native.last_load_stats()
    assert st["parser"] == "host" and st["lines"] == 782 and st["host_lines"] == 0 and st["auto_threshold"] >= 32 << 20
    _same_arrays(default, host)
    assert host["x"].shape == (782, host["d"]) and len(host["qnames"]) == len(set(host["qnames"])) == 45


def test_an_unknown_parser_word_is_refused():
    with pytest.raises(Exception, match="auto.*host.*device"):
        fr.CDataset.open_ranksvm(GOLDEN_TRAIN, parser="gpu")
    L = fr.clib._load()
    with pytest.raises(Exception, match="unknown parser .*gpu.*: expected one of .*auto.*host.*device"):
        fr.clib._unwrap(L.fr_load_ranksvm(GOLDEN_TRAIN.encode(), None, b"gpu"))


def test_parser_device_without_a_device_fails_loudly():
    if native.device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(Exception, match=NO_DEVICE):
        fr.CDataset.open_ranksvm(GOLDEN_TRAIN, parser="device")


def test_merge_header_under_address_and_undefined_sanitizers(tmp_path):
    """tests/ranksvm_merge_sanitize.cpp: a program of its own over csrc/text_merge.hpp alone, fed hand-made pass-1 records,
    built with -fsanitize=address,undefined and run directly."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "ranksvm_merge_sanitize")
    build = subprocess.run([cxx, "-std=c++17", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                            "-I", os.path.join(here, "..", "fastrank_amd", "csrc"), os.path.join(here, "ranksvm_merge_sanitize.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "ranksvm_merge ok" in run.stdout, run.stdout
