"""The evaluation measures without a device: the numpy restatement (tests/measures_model.py) against its
own term-by-term form and against exact statements, the library's scalar definitions (csrc/measures_host.hpp through
fr_debug_measure_ranked) against hand-derived values and the restatement, every refusal that needs no device, the list of
measures, the routing rule at its edges, and the header under the sanitizers."""
import math
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import native
from tests import measures_model as mm


def _bits(v):
    return np.float64(v).view(np.uint64)


def _forms(name, depth, gains, norm):
    """the vectorised form, the term-by-term form and the library's scalar form of one value"""
    evaluator = name if depth is None else "%s@%d" % (name, depth)
    lib_norm = float(depth) if name == "precision" else float(norm)
    return mm.value(name, depth, gains, norm), mm.value(name, depth, gains, norm, scalar=True), native.measure_ranked(evaluator, gains, lib_norm)


@pytest.mark.parametrize("n", [1, 2, 7, 64, 65, 300])
def test_the_two_forms_and_the_library_agree_bit_for_bit_on_random_lists(n):
    rng = np.random.default_rng(n)
    for trial in range(6):
        gains = rng.integers(0, 5, size=n).astype(np.float32)
        if trial == 0:
            gains[:] = 0
        if trial == 1:
            gains = (gains - 2).astype(np.float32)  # negative gains: not relevant, a negative DCG term
        for depth in (None, 1, 2, 10, 64, 65, 1000):
            for name in mm.NAMES:
                if depth is None and name in mm.NEEDS_DEPTH:
                    continue
                norms = {"recall": (0, 3, n + 5), "err": (16.0, 1024.0)}.get(name, (0,))
                for norm in norms:
                    a, b, c = _forms(name, depth, gains, norm)
                    assert _bits(a) == _bits(b) == _bits(c), (name, depth, norm, a, b, c)


def test_err_and_dcg_equal_exact_statements_rounded_once():
    # ERR: relevant documents at ranks 1, 2, 4, 8 only (divisions by powers of two), gains <= 3 under den = 16: every product
    # and quotient is a dyadic fraction of few bits, so the float form makes no rounding at all
    gains = np.zeros(12, dtype=np.float32)
    gains[[0, 1, 3, 7]] = [1, 3, 2, 3]
    for depth in (None, 1, 2, 3, 4, 8, 12, 40):
        exact = mm.err_exact(gains, depth, 16)
        assert mm.err(gains, depth, 16.0) == float(exact) and Fraction(mm.err_scalar(gains, depth, 16.0)) == exact
        assert native.measure_ranked("err" if depth is None else "err@%d" % depth, gains, 16.0) == float(exact)
    assert mm.err_exact(gains, 2, 16) == Fraction(1, 16) + Fraction(15, 16) * Fraction(7, 16) / 2
    # DCG: gains at ranks 1, 3, 7 (discounts 1, 2, 3); 2^2 - 1 = 3 over 3 is exact
    gains = np.zeros(9, dtype=np.float32)
    gains[[0, 2, 6]] = [3, 1, 2]
    for depth in (None, 1, 3, 6, 7, 9, 100):
        exact = mm.dcg_exact(gains, depth)
        assert mm.dcg(gains, depth) == float(exact) and Fraction(mm.dcg_scalar(gains, depth)) == exact
        assert native.measure_ranked("dcg" if depth is None else "dcg@%d" % depth, gains) == float(exact)
    assert mm.dcg_exact(gains, None) == 7 + Fraction(1, 2) + 1


def _all(evaluator, gains, norm=0.0):
    name, depth = mm.parse(evaluator)
    a, b, c = _forms(name, depth, np.asarray(gains, dtype=np.float32), norm)
    assert _bits(a) == _bits(b) == _bits(c), (evaluator, a, b, c)
    return a


def test_hand_derived_values_on_designed_lists():
    none, one, every = [0, 0, 0, 0], [0, 0, 1, 0], [1, 2, 1, 1]
    # no relevant document
    for ev in ("dcg", "dcg@2", "precision@2", "recall", "recall@2", "success@3", "err", "err@2"):
        assert _all(ev, none, 4.0 if ev.startswith("err") else 0.0) == 0.0
    # one, at rank 3
    assert _all("dcg", one) == 0.5 and _all("dcg@2", one) == 0.0 and _all("dcg@3", one) == 0.5
    assert _all("precision@2", one) == 0.0 and _all("precision@3", one) == 1.0 / 3.0 and _all("precision@4", one) == 0.25
    assert _all("recall@2", one) == 0.0 and _all("recall@3", one) == 1.0 and _all("recall", one) == 1.0
    assert _all("success@2", one) == 0.0 and _all("success@3", one) == 1.0
    assert _all("err@2", one, 2.0) == 0.0 and _all("err", one, 2.0) == 0.5 / 3.0 and _all("err", one, 4.0) == 0.25 / 3.0
    # every one: gains 1 2 1 1, den 4: R = 1/4, 3/4, 1/4, 1/4
    assert _all("precision@2", every) == 1.0 and _all("recall@2", every) == 0.5 and _all("success@1", every) == 1.0
    assert _all("dcg@2", every) == 1.0 + 3.0 / math.log2(3.0)
    assert _all("err@2", every, 4.0) == 0.25 + (0.75 * 0.75) / 2.0
    assert _all("err@3", every, 4.0) == (0.25 + (0.75 * 0.75) / 2.0) + ((0.75 * 0.25) * 0.25) / 3.0
    # a relevant document first, and the next one at rank k + 1 = 4
    first = [2, 0, 0, 1, 0]
    assert _all("success@1", first) == 1.0 and _all("precision@3", first) == 1.0 / 3.0 and _all("precision@4", first) == 0.5
    assert _all("recall@3", first) == 0.5 and _all("recall@4", first) == 1.0
    assert _all("dcg@3", first) == 3.0 and _all("dcg@4", first) == 3.0 + 1.0 / math.log2(5.0)
    assert _all("err@3", first, 4.0) == 0.75 and _all("err@4", first, 4.0) == 0.75 + (0.25 * 0.25) / 4.0
    # k larger than the list: precision divides by k all the same
    assert _all("precision@10", every) == 0.4 and _all("recall@10", every) == 1.0 and _all("dcg@10", every) == _all("dcg", every)
    assert _all("err@10", every, 4.0) == _all("err", every, 4.0) and _all("success@10", none) == 0.0
    # a judged count above the list's own, and one below it (a value above 1: the judgments' business)
    assert _all("recall", every, 16) == 0.25 and _all("recall@2", every, 16) == 0.125 and _all("recall", every, 2) == 2.0
    # the list of one document
    assert _all("precision@1", [3]) == 1.0 and _all("err", [3], 8.0) == 0.875 and _all("dcg@1", [3]) == 7.0 and _all("recall@1", [0]) == 0.0


def test_rank_order_is_score_descending_then_gain_ascending_then_id_ascending():
    scores = [1.0, 2.0, 1.0, 1.0, -0.0, 0.0]
    gains = [1, 0, 0, 0, 2, 1]
    assert list(mm.rank_order(scores, gains, np.arange(6))) == [1, 2, 3, 0, 5, 4]
    assert list(mm.rank_order(scores, gains, [5, 4, 3, 2, 1, 0])) == [1, 3, 2, 0, 5, 4]


def _small():
    X = np.arange(12, dtype=np.float32).reshape(6, 2)
    return X, np.array([0, 1, 2, 0, 1, 0], dtype=np.float64), np.array([1, 1, 1, 2, 2, 2], dtype=np.int64)


def test_refusals_that_need_no_device():
    X, y, qid = _small()
    ds = fr.CDataset.from_numpy(X, y, qid)
    m = fr.CModel.from_dict({"Linear": {"weights": [1.0, 0.0]}})
    for name in ("precision", "prec", "Precision", "success"):
        with pytest.raises(Exception, match="%s needs a cut-off: write" % ("Success" if name == "success" else "Precision")):
            ds.evaluate(m, name)
    for name in ("precision@0", "prec@0", "success@0", "SUCCESS@00"):
        with pytest.raises(Exception, match="needs a cut-off of at least 1"):
            ds.evaluate(m, name)
    with pytest.raises(Exception, match='Invalid training measure: \\\\"p@5\\\\"'):
        ds.evaluate(m, "p@5")
    for name in ("p", "r@5", "errr", "dcg2", "recal@3"):
        with pytest.raises(Exception, match="Invalid training measure"):
            ds.evaluate(m, name)
    with pytest.raises(Exception, match="Couldn't parse after the @"):
        ds.evaluate(m, "precision@x")
    # a gain whose 2^gain is not finite: ERR has nothing to divide by (the other measures do not look)
    big = fr.CDataset.from_numpy(X, np.array([0, 1, 2000, 0, 1, 0], dtype=np.float64), qid)
    with pytest.raises(Exception, match="no finite 2\\^gain"):
        big.evaluate(m, "err@10")
    qrel = fr.CQRel.from_dict({"7": {"d": 1500.0}})  # ... in a judgment of a query the dataset does not even hold
    with pytest.raises(Exception, match="no finite 2\\^gain"):
        ds.evaluate(m, "err", qrel)
    # the trainers refuse the same way, before any device work
    req = fr.TrainRequest.coordinate_ascent()
    req.measure = "success"
    with pytest.raises(Exception, match="Success needs a cut-off"):
        ds.train_model(req)
    lm = fr.TrainRequest.lambdamart()
    lm.measure = "precision@5"
    with pytest.raises(Exception, match="LambdaMART: unsupported training measure"):
        ds.train_model(lm)
    with pytest.raises(Exception, match="not one of dcg, precision, recall, success, err"):
        native.measure_ranked("ndcg@3", [1, 0])


def test_the_list_of_measures():
    rows = fr.measures()
    assert rows == fr.query_json("measures")
    assert [r["name"] for r in rows] == ["ndcg", "map", "mrr", "dcg", "precision", "recall", "success", "err"]
    by = {r["name"]: r for r in rows}
    assert by["map"]["aliases"] == ["ap"] and by["mrr"]["aliases"] == ["rr"] and by["precision"]["aliases"] == ["prec"]
    assert all(by[n]["aliases"] == [] for n in ("ndcg", "dcg", "recall", "success", "err"))
    assert {n: by[n]["cutoff"] for n in by} == {"ndcg": "optional", "map": "ignored", "mrr": "ignored", "dcg": "optional", "precision": "required",
                                                  "recall": "optional", "success": "required", "err": "optional"}
    assert [r["display"] for r in rows] == ["NDCG", "AP", "RR", "DCG", "Precision", "Recall", "Success", "ERR"]
    assert not any("p" in [r["name"]] + r["aliases"] for r in rows)
    assert native.last_metric_plan()["measure"] is None or "classes" in native.last_metric_plan()


def test_the_routing_rule_at_its_edges():
    pays = native.metric_topk_pays
    for npad in (64, 128, 8192, 16384, 1 << 20):
        assert not pays(0, npad) and not pays(-1, npad) and not pays(65, npad) and not pays(1 << 40, npad)
    assert not pays(10, 0)
    # classes that would sort in the global scratch slab (more than 8192 documents) always select
    for depth in (1, 10, 64):
        assert pays(depth, 16384) and pays(depth, 1 << 20)
    # the depths the 30K table set
    assert pays(10, 64) and not pays(11, 64) and pays(10, 128) and not pays(20, 128)
    assert pays(20, 256) and pays(20, 512) and not pays(21, 256) and not pays(64, 512)
    assert pays(10, 1024) and not pays(20, 1024) and pays(10, 8192) and not pays(11, 8192)
    # monotone in the depth for every class: a deeper cut-off never pays where a shallower one does not
    for lg in range(6, 21):
        row = [pays(d, 1 << lg) for d in range(1, 65)]
        assert row == sorted(row, reverse=True), lg


def test_host_header_under_address_and_undefined_sanitizers(tmp_path):
    """tests/measures_host_sanitize.cpp: a program of its own over csrc/measures_host.hpp, built with
    -fsanitize=address,undefined and run directly."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "measures_host_sanitize")
    build = subprocess.run([cxx, "-std=c++17", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(here, "..", "fastrank_amd", "csrc"), os.path.join(here, "measures_host_sanitize.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "measures_host ok" in run.stdout, run.stdout
