"""The forest packers (csrc/forest_pack.hpp) on the CPU: every forest of tests/test_gpu_tree_scoring.py is packed through
fr_debug_forest_pack (no device), decoded by the numpy restatements of the kernels' walks (tests/forest_pack_model.py) and
held to tests/tree_shapes.score bit for bit; the admissions, batches and block shapes are the ones the device tests assert
by path; the header also runs on its own under the address and undefined-behaviour sanitizers
(tests/forest_pack_sanitize.cpp)."""
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import native
from tests import forest_pack_model as fpm
from tests import test_gpu_tree_scoring as cases

ALL_SHAPES = sorted(cases.lds_shape_table()[0])
ORDER_MULTI = cases.lds_shape_table()[1]


def order_single():
    """The shapes a bare tree tries (its leaf comes back as it is, which only one-part blocks do), read from the packer."""
    src = open(os.path.join(cases.ROOT, "fastrank_amd", "csrc", "forest_pack.hpp")).read()
    body = re.search(r"TREE_ORDER_SINGLE\[\]\[2\] = \{(.*?)\};", src, re.S).group(1)
    order = [(int(a), int(b)) for a, b in re.findall(r"\{(\d+), (\d+)\}", body)]
    assert len(order) == 3 and all(s in ALL_SHAPES and s[1] == 1 for s in order)
    return order


ORDER_SINGLE = order_single()


@functools.lru_cache(maxsize=None)
def packed(name, encoding):
    mname, _, _, model, _, _ = cases.built(name)
    return native.forest_pack(fr.CModel.from_dict(model), cases.MATRICES[mname][1], encoding)


def lds_name(shape):
    return "lds:%d,%d" % shape


def first_admitting_shape(name):
    bare = cases.FORESTS[name][2]
    for shape in (ORDER_SINGLE if bare else ORDER_MULTI):
        if packed(name, lds_name(shape))["admitted"]:
            return shape
    return None


def same_bits(got, name):
    mname, _, _, _, _, restated = cases.built(name)
    assert got.dtype == np.float64 and np.array_equal(got, restated, equal_nan=True) and (np.signbit(got) == np.signbit(restated)).all(), name


def decode_lds(name, shape):
    mname, _, _, _, _, _ = cases.built(name)
    rep = packed(name, lds_name(shape))
    assert rep["admitted"], (name, shape)
    same_bits(fpm.score_lds(cases.matrix(mname)[0], shape[0], shape[1], rep["tables"], cases.FORESTS[name][2]), name)


@pytest.mark.parametrize("name", sorted(cases.FORESTS))
def test_every_encoding_that_admits_a_forest_decodes_to_its_scores(name):
    mname, _, _, _, _, _ = cases.built(name)
    X, bare = cases.matrix(mname)[0], cases.FORESTS[name][2]
    rank = packed(name, "rank")
    if rank["admitted"]:
        same_bits(fpm.score_rank(X, rank["tables"], rank["nslots"]), name)
        assert rank["nrounds"] == len(rank["tables"]["rdesc"]) // 32
    else:
        assert rank["tables"] == {} and "batches" not in rank
    shape = first_admitting_shape(name)
    if shape is not None:
        decode_lds(name, shape)
    same_bits(fpm.score_l2(X, packed(name, "l2")["tables"], bare), name)
    assert packed(name, "l2")["admitted"] is True


# (a bare tree is walked by one-part blocks only)
@pytest.mark.parametrize("name,shape", [("leafwise_32", s) for s in ALL_SHAPES] + [("bare_chain_12_left", s) for s in ALL_SHAPES if s[1] == 1])
def test_every_block_shape_of_the_lds_walk(name, shape):
    decode_lds(name, shape)
    rep = packed(name, lds_name(shape))
    fixed = (shape[0] * (24 + 1) * 4 + 15) // 16 * 16 + (shape[0] * 8 if shape[1] > 1 else 0)
    cap = min(cases.lds_shape_table()[0][shape] * 16 * shape[0] * shape[1], (160 * 1024 - fixed) // 16 * 16) // 8
    assert rep["lds_bytes"] == fixed + cap * 8


def test_admissions_are_the_ones_the_device_tests_assert_by_path():
    rank = lambda name: packed(name, "rank")["admitted"]
    lds = lambda name: [s for s in ORDER_MULTI if packed(name, lds_name(s))["admitted"]]
    assert rank("thr_1023") and not rank("thr_1024")
    assert rank("slots_170") and not rank("slots_171")
    assert [rank("slots_%d" % k) for k in cases.RANK_FEATURE_COUNTS] == [True] * 4 + [False] * 2
    assert all(rank("thr_%d" % n) for n in cases.RANK_THRESHOLD_COUNTS[:-1])
    assert not rank("chain_11_ensemble") and lds("chain_11_ensemble")
    assert all(not rank(n) for n in cases.FORESTS if cases.FORESTS[n][2]), "a bare tree is never ranked"
    for name in ("complete_8", "comb_admitted", "comb_left_admitted"):
        assert lds(name)[0] == ORDER_MULTI[0], name
    for name in ("complete_8_plus_one", "complete_9", "comb_refused", "comb_left_refused", "cache_c_l2"):
        assert not any(packed(name, lds_name(s))["admitted"] for s in ALL_SHAPES), name
    assert lds("word_cap_under")[0] == ORDER_MULTI[0]
    over = lds("word_cap_over")
    assert over and over[0] != ORDER_MULTI[0] and over[0] == cases.first_lds_shape(fpm_nodes("word_cap_over"), 24)
    for m in cases.WIDE:
        exp = cases.wide_expectation(cases.MATRICES[m][1])
        got = first_admitting_shape("wide_" + m)
        assert got == ((exp["docs"], exp["parts"]) if exp["path"] == "lds" else None), (m, got, exp)
        assert rank("wide_" + m)


def fpm_nodes(name):
    """Nodes of the forest's first tree, counted from its adjacent-children layout."""
    t = packed(name, "l2")["tables"]
    return int(t["roots"][1]) if len(t["roots"]) > 1 else len(t["nodes"])


def test_batches_are_the_ones_the_device_tests_assert():
    batches = lambda name, enc="rank": packed(name, enc)["batches"]
    assert batches("chains_10") == [[1, 10]] * 3
    assert batches("chain_10_alone") == [[1, 10]]
    assert batches("walks_by_count") == [[8, 1], [4, 1], [2, 1], [1, 10]]
    assert batches("walks_by_depth") == [[8, 7], [4, 8], [4, 8], [2, 9], [2, 9], [1, 10]]
    assert batches("tail_of_two") == [[8, 1], [1, 2]]
    assert batches("all_leaves") == [[1, 1], [1, 1]] and packed("all_leaves", "rank")["nslots"] == 0
    assert packed("absent_features", "rank")["nslots"] == 0
    first = lds_name(ORDER_MULTI[0])
    assert batches("complete_8", first) == [[1, 8], [1, 1]]
    for name, comb in (("comb_admitted", cases.COMB_ADMITTED), ("comb_left_admitted", cases.COMB_LEFT_ADMITTED)):
        assert batches(name, first) == [[1, comb[0] + comb[1]]]
    assert batches("bare_chain_12_left", "lds:256,1") == [[1, 12]] and batches("batched_chain_12_left", first) == [[2, 12], [1, 1]]
    assert batches("word_cap_under", first)[0][0] == 1
    base = packed("chunk_min", "rank")
    assert base["nslots"] == 4
    for exact, more in (("chunk_1024_512", "chunk_1024_512_256"), ("chunk_512_512_512", "chunk_512_512_512_256"), ("chunk_1024_512", "chunk_1024_512_2")):
        assert packed(exact, "rank")["nrounds"] == base["nrounds"] and packed(more, "rank")["nrounds"] == base["nrounds"] + 1


def test_forest_hash_covers_every_bit_of_a_weight():
    _, trees, weights, model, _, _ = cases.built("cache_a")
    changed = list(weights)
    changed[17] = float(np.nextafter(changed[17], np.inf))
    other = {"Ensemble": {"weights": changed, "models": [{"DecisionTree": t} for t in trees]}}
    a, b = packed("cache_a", "rank")["hash"], native.forest_pack(fr.CModel.from_dict(other), 24, "rank")["hash"]
    assert len(a) == 16 and int(a, 16) != 0 and a != b
    assert a == native.forest_pack(fr.CModel.from_dict(model), 24, "l2")["hash"], "the hash is the forest's, whatever the encoding"


def test_the_hook_refuses_what_it_cannot_pack():
    linear = fr.CModel.from_dict({"Linear": {"weights": [1.0, 2.0]}})
    with pytest.raises(Exception, match="neither a DecisionTree"):
        native.forest_pack(linear, 24, "rank")
    tree = fr.CModel.from_dict(cases.built("cache_a")[3])
    with pytest.raises(Exception, match="no block shape"):
        native.forest_pack(tree, 24, "lds:100,3")
    with pytest.raises(Exception, match="encoding is"):
        native.forest_pack(tree, 24, "heap")


def test_forest_pack_header_under_address_and_undefined_sanitizers(tmp_path):
    """tests/forest_pack_sanitize.cpp: a program of its own over csrc/forest_pack.hpp (forests at the packers' limits, every
    block shape), built with -fsanitize=address,undefined and run directly."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "forest_pack_sanitize")
    build = subprocess.run([cxx, "-std=c++17", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                            "-I", os.path.join(here, "..", "fastrank_amd", "csrc"), os.path.join(here, "forest_pack_sanitize.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "forest_pack ok" in run.stdout, run.stdout
