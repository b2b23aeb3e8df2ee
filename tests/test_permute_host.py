"""Permutation importance without a device: the numpy restatement (tests/permute_model.py) against its
own term-by-term form, the library's sources against the restatement on datasets and views, the uniformity of the stream, the
refusals that need no device, and csrc/permute_host.hpp under the sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import native
from tests import permute_model as pm

NO_DEVICE = "no MI355X/HIP device available"
NONE = 0xFFFFFFFF
CHI2_23_999 = 49.73   # the 99.9 % point of chi-square with 23 degrees of freedom
CHI2_256_999 = 330.5  # ... with 256


def _dataset(qid, d=3, seed=0):
    qid = np.asarray(qid, dtype=np.int64)
    rng = np.random.default_rng(seed)
    X = rng.integers(-3, 4, size=(len(qid), d)).astype(np.float32)
    y = rng.integers(0, 3, size=len(qid)).astype(np.float64)
    return fr.CDataset.from_numpy(X, y, qid)


def _interleaved(n, nq, seed):
    return np.random.default_rng(seed).integers(0, nq, size=n).astype(np.int64) + 10


@pytest.mark.parametrize("n", [1, 2, 5, 257])
def test_vectorised_restatement_equals_the_term_by_term_one(n):
    ids = np.arange(n) * 3 + 1  # (gapped ids: the list index, not the id, enters the stream)
    query_of = list(_interleaved(n, 4, n))
    for seed in (0, 0xFFFFFFFFFFFFFFFF, 12345):
        for r in (0, 63):
            assert list(pm.sources(ids, seed, r)) == pm.sources_scalar(ids, seed, r)
            assert list(pm.sources(ids, seed, r, "query", query_of)) == pm.sources_scalar(ids, seed, r, "query", query_of)
    rng = np.random.default_rng(n)
    for R in (1, 2, 5, 64):
        values = rng.random(R)
        a, b = pm.report(0.625, values), pm.report_scalar(0.625, values)
        assert np.array_equal(np.array(a).view(np.uint64), np.array(b).view(np.uint64))
    assert pm.report(0.75, [0.25]) == (0.5, 0.0)
    assert pm.report(0.75, [0.5, 0.25, 0.75]) == (0.25, 0.25)  # d = 0.25, 0.5, 0; squares 0, 1/16, 1/16


def test_the_stream_key_is_the_next_free_multiple():
    from tests import resample_model as rm

    assert pm.stream_key(0) == rm.mix_int(3 * pm.G)
    assert len({pm.stream_key(0), rm.boot_key(0), rm.perm_key(0)}) == 3


@pytest.mark.parametrize("n", [1, 2, 257])
def test_library_sources_equal_the_restatement(n):
    qid = _interleaved(n, 5, n)
    ds = _dataset(qid)
    ids = np.arange(n)
    for seed, r in ((0, 0), (7, 3), (0xFFFFFFFFFFFFFFFF, 63)):
        assert np.array_equal(native.permutation_sources(ds, seed, r), pm.sources(ids, seed, r))
        got = native.permutation_sources(ds, seed, r, "query")
        assert np.array_equal(got, pm.sources(ids, seed, r, "query", qid))
        assert np.array_equal(qid[got], qid)  # never crosses a query
        assert np.array_equal(np.sort(got), ids)


def test_interleaved_queries_and_a_one_document_query():
    qid = np.array([4, 9, 4, 7, 9, 4, 9, 4, 4, 9], dtype=np.int64)  # query 7 holds one document
    ds = _dataset(qid)
    moved = 0
    for r in range(8):
        got = native.permutation_sources(ds, 3, r, "query")
        assert np.array_equal(got, pm.sources(np.arange(10), 3, r, "query", qid))
        assert got[3] == 3 and np.array_equal(qid[got], qid)
        moved += int((got != np.arange(10)).sum())
    assert moved > 0


def test_a_query_views_sources_never_leave_the_view():
    qid = _interleaved(300, 6, 1)
    ds = _dataset(qid)
    view = ds.subsample_queries(["11", "14", "15"])
    ids = np.nonzero(np.isin(qid, [11, 14, 15]))[0]
    for scope in ("dataset", "query"):
        got = native.permutation_sources(view, 5, 1, scope, n_total=300)
        want = np.full(300, NONE, dtype=np.int64)
        want[ids] = pm.sources(ids, 5, 1, scope, qid[ids])
        assert np.array_equal(got, want)
        assert np.array_equal(np.sort(got[ids]), ids)
    # the list index enters the stream, not the id: the view's permutation is not the parent's restricted to it
    assert not np.array_equal(native.permutation_sources(ds, 5, 1)[ids], native.permutation_sources(view, 5, 1, n_total=300)[ids])


def test_a_feature_view_has_its_parents_sources():
    qid = _interleaved(100, 3, 2)
    ds = _dataset(qid, d=4)
    view = ds.subsample_feature_names(["0", "2"])
    for scope in ("dataset", "query"):
        assert np.array_equal(native.permutation_sources(view, 9, 2, scope), native.permutation_sources(ds, 9, 2, scope))
        assert np.array_equal(native.permutation_sources(view, 9, 2, scope), pm.sources(np.arange(100), 9, 2, scope, qid))


def test_repeat_r_is_the_same_whatever_the_number_of_repeats():
    """The stream of repeat r takes (seed, r, n) and nothing else: the sources of r = 0 .. 8 are the restatement's one by one
    (there is no count to pass), differ from each other, and differ between seeds."""
    qid = _interleaved(64, 3, 3)
    ds = _dataset(qid)
    rows = [native.permutation_sources(ds, 2, r) for r in range(9)]
    for r, row in enumerate(rows):
        assert np.array_equal(row, pm.sources(np.arange(64), 2, r))
    assert len({row.tobytes() for row in rows}) == 9
    assert not np.array_equal(native.permutation_sources(ds, 3, 0), rows[0])


def test_all_24_orders_of_four_documents_are_equally_likely_over_seeds():
    """n = 4, repeat 0, seeds 0 .. 47 999: chi-square over the 24 permutations 12.87 (23 degrees of freedom; cap: the 99.9 % point)."""
    T = 48000
    which = pm.permutation_index(pm.order_of(pm.keys_many(range(T), [0] * T, 4)))
    chi = pm.chi_square(np.bincount(which, minlength=24), T / 24)
    print("chi-square", chi)
    assert chi <= CHI2_23_999


def test_all_24_orders_are_equally_likely_over_the_repeats_of_one_seed():
    """n = 4, seed 0, repeats 0 .. 47 999 (the stream has no cap of its own; the call's is 64): chi-square 20.06."""
    T = 48000
    which = pm.permutation_index(pm.order_of(pm.keys_many([0] * T, range(T), 4)))
    chi = pm.chi_square(np.bincount(which, minlength=24), T / 24)
    print("chi-square", chi)
    assert chi <= CHI2_23_999


def test_where_one_document_of_257_lands_is_uniform():
    """n = 257, seeds 0 .. 19 999: the place document 0 takes, chi-square 254.4 (256 degrees of freedom)."""
    T = 20000
    order = pm.order_of(pm.keys_many(range(T), [0] * T, 257))
    chi = pm.chi_square(np.bincount(np.argmax(order == 0, axis=1), minlength=257), T / 257)
    print("chi-square", chi)
    assert chi <= CHI2_256_999


def test_a_four_document_query_inside_a_larger_dataset_takes_all_24_orders_equally():
    """Scope "query": the four documents of one query, scattered over a dataset of 40, over seeds 0 .. 23 999 through the
    restatement (held to the library above and, for 200 of the seeds, here)."""
    n, T = 40, 24000
    qid = np.array([1] * 10 + [2] * 26 + [3] * 4, dtype=np.int64)
    qid = qid[np.random.default_rng(4).permutation(n)]
    members = np.nonzero(qid == 3)[0]
    u = pm.keys_many(range(T), [0] * T, n)[:, members]
    which = pm.permutation_index(pm.order_of(u))
    chi = pm.chi_square(np.bincount(which, minlength=24), T / 24)
    print("chi-square", chi)
    assert chi <= CHI2_23_999
    ds = _dataset(qid)
    for seed in range(200):
        got = native.permutation_sources(ds, seed, 0, "query")
        assert np.array_equal(got[members], members[pm.order_of(u[seed])])


def _linear(d=3):
    return fr.CModel.from_dict({"Linear": {"weights": [1.0] * d}})


def _leaf(v):
    return {"LeafNode": v}


def test_refusals_come_before_the_device_is_touched():
    """Every one of these is raised on a machine with no device: the device is asked for after them."""
    ds = _dataset(_interleaved(20, 3, 0))
    m = _linear()
    call = native.permutation_importance_dense
    with pytest.raises(Exception, match="repeats must be between 1 and 64, not 0"):
        call(m, ds, "ndcg", repeats=0)
    with pytest.raises(Exception, match="repeats must be between 1 and 64, not 65"):
        call(m, ds, "ndcg", repeats=65)
    with pytest.raises(Exception, match="scope must be .*dataset.* or .*query.*, not .*document"):
        call(m, ds, "ndcg", scope="document")
    with pytest.raises(Exception, match="feature 3 is not one of the dataset's features"):
        call(m, ds, "ndcg", features=[0, 3])
    with pytest.raises(Exception, match="feature 1 is listed twice"):
        call(m, ds, "ndcg", features=[1, 0, 1])
    view = ds.subsample_feature_names(["0", "2"])
    with pytest.raises(Exception, match="feature 1 is not one of the dataset's features"):
        call(m, view, "ndcg", features=[1])
    with pytest.raises(Exception, match="max_slots must be at least 1"):
        call(m, ds, "ndcg", max_slots=0)
    tree = {"DecisionTree": {"FeatureSplit": {"fid": 0, "split": 0.5, "lhs": _leaf(0.0), "rhs": _leaf(1.0)}}}
    mixed = fr.CModel.from_dict({"Ensemble": {"weights": [1.0, 1.0], "models": [{"Linear": {"weights": [1.0, 0.0, 0.0]}}, tree]}})
    with pytest.raises(Exception, match=r"not Ensemble\[Linear, DecisionTree\]"):
        call(mixed, ds, "ndcg")
    nested = fr.CModel.from_dict({"Ensemble": {"weights": [1.0], "models": [{"Ensemble": {"weights": [1.0], "models": [tree]}}]}})
    with pytest.raises(Exception, match=r"not Ensemble\[Ensemble\[DecisionTree\]\]"):
        call(nested, ds, "ndcg")
    reply = fr.clib._json_reply
    with pytest.raises(Exception, match="unknown field `repeat`, expected one of `repeats`, `seed`, `scope`, `features`, `skip_unused`, `max_slots`"):
        reply(fr.clib._load().fr_permutation_importance(m.pointer, ds.pointer, None, b"ndcg", b'{"repeat": 2}', None, 0, None))
    with pytest.raises(Exception, match="output buffer too small"):
        reply(fr.clib._load().fr_permutation_importance(m.pointer, ds.pointer, None, b"ndcg", b"{}", np.zeros(14).ctypes.data, 14, None))
    with pytest.raises(Exception, match="scope must be"):
        native.permutation_sources(ds, 0, 0, "list")
    with pytest.raises(ValueError, match="no feature named 'nine'"):
        fr.permutation_importance(ds, m, "ndcg", features=["nine"])
    with pytest.raises(Exception, match="repeats must be between 1 and 64, not 0"):
        m.permutation_importance(ds, "ndcg", repeats=0)


def test_an_empty_view_is_refused_before_the_device():
    ds = _dataset(_interleaved(20, 3, 0))
    empty = ds.subsample_queries([])
    assert empty.num_instances() == 0
    with pytest.raises(Exception, match="needs at least one document"):
        native.permutation_importance_dense(_linear(), empty, "ndcg")
    assert len(native.permutation_sources(empty, 0, 0)) == 0


@pytest.mark.skipif(native.device_count() > 0, reason="checks the no-GPU failure mode")
def test_without_gpu_a_good_call_fails_loudly():
    ds = _dataset(_interleaved(20, 3, 0))
    with pytest.raises(Exception, match=NO_DEVICE):
        native.permutation_importance_dense(_linear(), ds, "ndcg")


def test_host_header_under_address_and_undefined_sanitizers(tmp_path):
    """tests/permute_host_sanitize.cpp: a program of its own over csrc/permute_host.hpp (no documents and one, equal keys
    through the tie rule, the positions, the report at one repeat, every refusal), built with -fsanitize=address,undefined and
    run directly."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "permute_host_sanitize")
    build = subprocess.run([cxx, "-std=c++17", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                            "-I", os.path.join(here, "..", "fastrank_amd", "csrc"), os.path.join(here, "permute_host_sanitize.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "permute_host ok" in run.stdout, run.stdout
