"""Forest scoring at the limits of its three encodings: the threshold-rank walk, the f32 LDS walk and
the L2 walk, each held to the oracle AND to the numpy restatement of tests/tree_shapes.py bit for bit, with
native.last_tree_plan() asserting that the intended path, block shape and batch sizes really ran.

Every forest is registered in FORESTS (name -> matrix, builder); tests/test_tree_shapes_host.py walks the same registry on
the CPU and holds the restatement to the oracle on every one of them, so the references are themselves checked.

Where a limit is a number in the packer the tests stand on both sides of it and assert that the two sides took different
paths; the scores must be exact on both.
"""
import functools
import os
import re

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import native
from oracle import pyoracle as o
from tests import tree_shapes as ts

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_DOCS = 449  # ragged for blocks of 64, 128, 192 and 256 documents

# f32 values thresholds and documents are drawn from (no zero among them)
GRID = ((np.arange(1100) - 550 + 0.25) * 0.37).astype(np.float32)
FLT_MAX = np.float32(3.4028235e38)
SPECIALS = np.float32([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, np.inf, -np.inf, np.nan, FLT_MAX, -FLT_MAX])

MATRICES = {"d24": (N_DOCS, 24), "n1": (1, 24), "d176": (N_DOCS, 176), "d200": (N_DOCS, 200), "d320": (N_DOCS, 320),
            "d600": (N_DOCS, 600), "d604": (N_DOCS, 604), "d608": (N_DOCS, 608), "d700": (N_DOCS, 700)}


@functools.lru_cache(maxsize=None)
def matrix(name):
    """Every column holds grid values (= thresholds), their f32 neighbours on either side, +-0.0, denormals, +-inf, NaN and
    +-FLT_MAX, in an order of its own; half of the grid draws come from the grid's first 300 values, where the small
    threshold sets live.  Nine queries (one for the one-document matrix)."""
    n, d = MATRICES[name]
    rng = np.random.default_rng(1000 + d + n)
    X = np.empty((n, d), dtype=np.float32)
    for j in range(d):
        idx = np.where(rng.random(n) < 0.5, rng.integers(0, 300, n), rng.integers(0, len(GRID), n))
        col = GRID[idx]
        kind = rng.integers(0, 3, n)
        col = np.where(kind == 1, np.nextafter(col, np.float32(np.inf)), col)
        col = np.where(kind == 2, np.nextafter(col, np.float32(-np.inf)), col).astype(np.float32)
        if n >= 64:
            col[rng.choice(n, len(SPECIALS), replace=False)] = SPECIALS
        X[:, j] = col
    y = rng.integers(0, 5, n).astype(np.float64)
    qid = np.sort(rng.integers(0, 9, n)).astype(np.int64)
    return X, y, qid


@functools.lru_cache(maxsize=None)
def oracle_dataset(name):
    return o.Dataset(*matrix(name))


@functools.lru_cache(maxsize=None)
def device_dataset(name):
    return fr.CDataset.from_numpy(*matrix(name))


def weights_for(count, seed):
    """Both signs, twelve orders of magnitude: the order of the f64 sum shows in its bits."""
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], count) * 10.0 ** rng.uniform(-6.0, 6.0, count)).tolist()


def threshold_set(distinct):
    """f64 splits that the rank encoding counts as `distinct` thresholds: grid values, doubles that floor onto a grid value
    already there, -0.0 beside 0.0, -1e300 (floors to -inf) and 1e300 (floors to FLT_MAX)."""
    if distinct == 1:
        return [float(GRID[5]), float(GRID[5]) + 1e-9]
    if distinct == 2:
        return [0.0, -0.0, float(GRID[5]), float(GRID[5]) + 1e-9]
    grid = [float(v) for v in GRID[:distinct - 3]]
    return [-1e300, 1e300, 0.0, -0.0] + grid + [v + 1e-9 for v in grid[::7]]


ALL_THRESHOLDS = [float(v) for v in GRID[:300]] + [0.0, -0.0, 1e300, -1e300, float(GRID[7]) + 1e-9]


def picker(seed, feats, thresholds=None):
    return ts.Picker(seed, feats, ALL_THRESHOLDS if thresholds is None else thresholds)


# ---------------------------------------------------------------------------------------------- the forests
FORESTS = {}


def forest(name, matrix_name="d24", bare=False):
    def reg(fn):
        FORESTS[name] = (matrix_name, fn, bare)
        return fn
    return reg


RANK_THRESHOLD_COUNTS = (1, 2, 255, 256, 511, 512, 1023, 1024)
for _n in RANK_THRESHOLD_COUNTS:
    def _thr_forest(n=_n):
        p = picker(n, [0, 1, 2, 5, 23])
        trees = ts.stumps_with_thresholds(3, threshold_set(n), p) + [ts.complete(3, p) for _ in range(3)]
        return trees, weights_for(len(trees), n)
    forest("thr_%d" % _n)(_thr_forest)
forest("thr_255_one_document", "n1")(FORESTS["thr_255"][1])


def _group_forest(counts, seed):
    """Stumps on the features of float4 group 1 (features 4..7): counts[c] distinct thresholds on feature 4 + c."""
    p = picker(seed, [0])
    trees = []
    for c, count in enumerate(counts):
        if count:
            trees += ts.stumps_with_thresholds(4 + c, [float(v) for v in GRID[c:c + count]], p)
    order = np.random.default_rng(seed).permutation(len(trees))
    trees = [trees[i] for i in order]
    return trees, weights_for(len(trees), seed)


# table sizes: 2^k > count.  600 -> 1024 floats, 300 -> 512, 200 -> 256, 1 -> 2
forest("chunk_1024_512")(lambda: _group_forest((600, 300, 0, 0), 31))
forest("chunk_1024_512_256")(lambda: _group_forest((600, 300, 200, 0), 32))
forest("chunk_512_512_512")(lambda: _group_forest((300, 300, 300, 0), 33))
forest("chunk_512_512_512_256")(lambda: _group_forest((300, 300, 300, 200), 34))
forest("chunk_1024_512_2")(lambda: _group_forest((600, 300, 0, 1), 38))  # the smallest table there is: two floats over the chunk
forest("chunk_min")(lambda: _group_forest((1, 1, 1, 1), 35))
forest("chunk_depths_10_1_1_1")(lambda: _group_forest((1000, 1, 1, 1), 36))
forest("chunk_depths_1_1_1_10")(lambda: _group_forest((1, 1, 1, 1000), 37))

RANK_FEATURE_COUNTS = (167, 168, 169, 170, 171, 172)
for _k in RANK_FEATURE_COUNTS:
    def _slots_forest(k=_k):
        feats = [int(f) for f in np.random.default_rng(k).permutation(176)[:k]]
        p = picker(k, feats)
        trees = [t for f in feats for t in ts.stumps_with_thresholds(f, [p.node()[1]], p)]
        trees += [ts.complete(4, p) for _ in range(9)]
        return trees, weights_for(len(trees), k)
    forest("slots_%d" % _k, "d176")(_slots_forest)


# Random splits leave the deep end of a chain, or the last node of a wide level, without a document.  The trees whose far
# end is the point of a case get a spine the documents walk (tree_shapes.set_spine); SPINES lists them, and the host test
# holds that a good share of the documents reaches every spine's end.
SPINE_VALUES = [float(v) for v in GRID[:300]]
SPINES = {}


def walked(name, tree, side, fid):
    SPINES.setdefault(name, []).append((tree, side))
    return ts.set_spine(tree, side, fid, SPINE_VALUES)


def _chains(name, depths_sides, seed, feats=(0, 3, 7, 8, 22)):
    p = picker(seed, feats)
    trees = [ts.chain(d, s, p) for d, s in depths_sides]
    for i, (tree, (d, s)) in enumerate(zip(trees, depths_sides)):
        if d >= 2:
            walked(name, tree, s, feats[i % len(feats)])
    return trees, weights_for(len(trees), seed)


for _name, _spec, _seed in (
        ("chains_10", [(10, s) for s in ts.SIDES] * 3, 41),
        ("chain_10_alone", [(10, "zigzag")], 42),
        ("chain_11_ensemble", [(11, "left")], 43),
        # 32 + 16 + 8 stumps, a depth-10 chain, 3 stumps
        ("walks_by_count", [(1, "left")] * 56 + [(10, "right")] + [(1, "left")] * 3, 44),
        ("walks_by_depth", [(7, "left")] * 32 + [(8, "zigzag")] * 32 + [(9, "right")] * 16 + [(10, "left")] * 4, 45),
        ("tail_of_two", [(1, "left")] * 33 + [(2, "right")], 46),
        ("cache_b_lds", [(12, "left"), (3, "right"), (1, "left")], 102)):
    forest(_name)(lambda name=_name, spec=_spec, seed=_seed: _chains(name, spec, seed))


@forest("all_leaves")
def _all_leaves():
    p = picker(47, [0])
    trees = [ts.leaf_only(p) for _ in range(5)]
    return trees, weights_for(5, 47)


@forest("absent_features")
def _absent():
    p = picker(48, [24, 25, 1000], [-1.5, -0.0, 0.0, 2.5, 1e-46, -1e-46, -1e300, 1e300])
    trees = [ts.complete(3, p) for _ in range(13)]
    return trees, weights_for(13, 48)


# ---- the f32 LDS walk
@forest("complete_8")
def _complete8():
    p = picker(51, range(24))
    # the node with the largest child offset is the last one of level 7: the right spine ends there
    return [walked("complete_8", ts.complete(8, p), "right", 6)] + [ts.chain(1, "left", p) for _ in range(4)], weights_for(5, 51)


@forest("complete_8_plus_one")
def _complete8_plus_one():
    """complete(8) with one leaf of its last level split: that node's child offset is 256, the first value the 8 bits lack."""
    p = picker(57, range(24))
    tree = walked("complete_8_plus_one", ts.split_leftmost_leaf(ts.complete(8, p), p), "left", 6)
    return [tree] + [ts.chain(1, "left", p) for _ in range(4)], weights_for(5, 57)


@forest("complete_9")
def _complete9():
    p = picker(52, range(24))
    return [ts.complete(9, p)] + [ts.chain(1, "left", p) for _ in range(4)], weights_for(5, 52)


# the off-path subtrees hang on the left of a chain that runs right: the widest level of comb(12, 7) puts the largest child
# offset at exactly 255.  With the chain on the left the same limit lies one subtree level lower.
COMB_ADMITTED, COMB_REFUSED = (12, 7, "right"), (12, 8, "right")
COMB_LEFT_ADMITTED, COMB_LEFT_REFUSED = (12, 6, "left"), (12, 7, "left")
for _name, _comb, _seed in (("comb_admitted", COMB_ADMITTED, 53), ("comb_refused", COMB_REFUSED, 54),
                            ("comb_left_admitted", COMB_LEFT_ADMITTED, 55), ("comb_left_refused", COMB_LEFT_REFUSED, 56)):
    def _comb_forest(name=_name, comb=_comb, seed=_seed):
        p = picker(seed, range(24))
        tree = walked(name, ts.comb(comb[0], comb[1], p, comb[2]), comb[2], 11)
        return [tree, ts.chain(1, "left", p), ts.chain(1, "right", p)], weights_for(3, seed)
    forest(_name)(_comb_forest)


@functools.lru_cache(maxsize=None)
def deepest_chain(bare):
    """The deepest chain the model format admits (the parser stops at 128 nested containers), as a bare DecisionTree or as a
    member of an Ensemble."""
    for depth in range(70, 40, -1):
        t = ts.chain(depth, "left", picker(0, [0]))
        model = {"DecisionTree": t} if bare else {"Ensemble": {"weights": [1.0], "models": [{"DecisionTree": t}]}}
        try:
            fr.CModel.from_dict(model)
        except Exception:
            continue
        return depth
    raise AssertionError("no chain of 41..70 levels parses")


CHAIN_DEPTHS = ("11", "12", "33", "deepest")
for _d in CHAIN_DEPTHS:
    for _side in ts.SIDES:
        def _bare_chain(d=_d, side=_side):
            depth = deepest_chain(True) if d == "deepest" else int(d)
            return walked("bare_chain_%s_%s" % (d, side), ts.chain(depth, side, picker(60 + depth, [1, 4, 9, 23])), side, 4), None
        forest("bare_chain_%s_%s" % (_d, _side), bare=True)(_bare_chain)

        def _batched_chain(d=_d, side=_side):
            depth = deepest_chain(False) if d == "deepest" else int(d)
            p = picker(70 + depth, [1, 4, 9, 23])
            deep = walked("batched_chain_%s_%s" % (d, side), ts.chain(depth, side, p), side, 9)
            trees = [ts.chain(1, "left", p) for _ in range(5)] + [deep] + [ts.chain(1, "right", p) for _ in range(6)]
            return trees, weights_for(len(trees), 70 + depth)
        forest("batched_chain_%s_%s" % (_d, _side))(_batched_chain)

for _leaves in (255, 32):
    def _leafwise(leaves=_leaves):
        p = picker(80 + leaves, range(24))
        return [ts.leafwise(leaves, p) for _ in range(33)], weights_for(33, 80 + leaves)
    forest("leafwise_%d" % _leaves)(_leafwise)


# ---- the shape table and the per-shape word cap, from the packer's source
@functools.lru_cache(maxsize=None)
def lds_shape_table():
    """(TREE_SHAPES as {(docs, parts): prefetch words}, the order multi-tree forests try them in), read from the packer."""
    src = open(os.path.join(ROOT, "fastrank_amd", "csrc", "forest_pack.hpp")).read()
    table = re.search(r"TREE_SHAPES\[\] = \{(.*?)\};", src, re.S).group(1)
    shapes = {(int(a), int(b)): int(c) for a, b, c, _ in re.findall(r"\{(\d+), (\d+), (\d+), (\d+)\}", table)}
    order = re.search(r"TREE_ORDER_MULTI\[\]\[2\] = \{(.*?)\};", src, re.S).group(1)
    order = [(int(a), int(b)) for a, b in re.findall(r"\{(\d+), (\d+)\}", order)]
    assert len(shapes) == 10 and len(order) == 7 and all(s in shapes for s in order)
    return shapes, order


def lds_max_nodes(shape, d):
    """Nodes of the largest tree block shape `shape` takes on a d-feature matrix (None: the feature columns alone do not fit):
    the tree's words and its header word must fit beside parts - 1 two-word padding trees, in what is smaller of the shape's
    prefetch capacity (pf 16-byte words per thread) and the LDS the feature columns leave of 160 KB."""
    shapes, _ = lds_shape_table()
    docs, parts = shape
    dq = (d + 3) // 4
    fixed = (docs * (dq * 4 + 1) * 4 + 15) // 16 * 16 + (docs * 8 if parts > 1 else 0)
    if fixed + 8 * 1024 > 160 * 1024:
        return None
    words_cap = min(shapes[shape] * 16 * docs * parts, (160 * 1024 - fixed) // 16 * 16) // 8
    return words_cap - 1 - (parts - 1) * 2


def first_lds_shape(nodes, d):
    _, order = lds_shape_table()
    for shape in order:
        cap = lds_max_nodes(shape, d)
        if cap is not None and nodes <= cap:
            return shape
    return None


BAND_WIDTH = 64


def word_cap_leaves():
    """Leaves of the largest tree the first shape tried takes on the 24-feature matrix (a tree of L leaves has 2L - 1 nodes)."""
    _, order = lds_shape_table()
    return (lds_max_nodes(order[0], 24) + 1) // 2


for _name, _extra, _seed in (("word_cap_under", 0, 91), ("word_cap_over", 1, 92)):
    def _word_cap(name=_name, extra=_extra, seed=_seed):
        p = picker(seed, range(24))
        # the left spine runs down the first node of every level to the tree's last level
        big = walked(name, ts.banded(word_cap_leaves() + extra, BAND_WIDTH, p), "left", 13)
        return [big] + [ts.chain(1, "left", p) for _ in range(5)], weights_for(6, seed)
    forest(_name)(_word_cap)

WIDE = ("d200", "d320", "d600", "d604", "d608", "d700")
for _m in WIDE:
    def _wide(m=_m):
        d = MATRICES[m][1]
        p = picker(d, [0, 3, d // 2, d - 2, d - 1, d + 5])
        trees = [ts.complete(5, p) for _ in range(9)] + [walked("wide_" + m, ts.chain(7, "zigzag", p), "zigzag", d - 1), ts.leafwise(20, p)]
        return trees, weights_for(len(trees), d)
    forest("wide_%s" % _m, _m)(_wide)

# ---- the cache
forest("cache_a")(lambda: ([ts.complete(4, picker(101, range(24))) for _ in range(37)], weights_for(37, 101)))
forest("cache_c_l2")(lambda: ([walked("cache_c_l2", ts.comb(COMB_REFUSED[0], COMB_REFUSED[1], picker(103, range(24)), COMB_REFUSED[2]), COMB_REFUSED[2], 2),
                               ts.chain(2, "left", picker(104, [0]))], weights_for(2, 103)))


@functools.lru_cache(maxsize=None)
def built(name):
    """(matrix name, trees, weights or None for a bare tree, the model's dict, oracle scores, restated scores)."""
    mname, fn, bare = FORESTS[name]
    trees, weights = fn()
    X = matrix(mname)[0]
    if bare:
        model = {"DecisionTree": trees}
        oracle = oracle_dataset(mname).score_ensemble([trees], [1.0])
        restated = ts.score(X, trees, None)
    else:
        model = {"Ensemble": {"weights": list(weights), "models": [{"DecisionTree": t} for t in trees]}}
        oracle = oracle_dataset(mname).score_ensemble(trees, weights)
        restated = ts.score(X, trees, weights)
    oracle.setflags(write=False), restated.setflags(write=False)
    return mname, trees, weights, model, oracle, restated


def run(name, dataset=None, rows=None):
    """Scores forest `name` on its matrix (or on `dataset`, a view holding documents `rows` of it) and returns the plan, after
    holding every score to the oracle and to the restatement."""
    mname, _, _, model, oracle, restated = built(name)
    n = len(oracle)
    got = native.predict_scores_dense(fr.CModel.from_dict(model), device_dataset(mname) if dataset is None else dataset, n)
    plan = native.last_tree_plan()
    rows = np.arange(n) if rows is None else rows
    assert not np.isnan(oracle).any()
    assert np.array_equal(got[rows], oracle[rows], equal_nan=True), (name, plan, "differs from the oracle")
    assert np.array_equal(got[rows], restated[rows], equal_nan=True), (name, plan, "differs from the restatement")
    return plan


@pytest.fixture(autouse=True)
def default_paths(monkeypatch):
    monkeypatch.delenv("FR_TREE_RANK", raising=False)
    monkeypatch.delenv("FR_TREE_SHAPE", raising=False)


# ---------------------------------------------------------------------------------------------- threshold-rank walk

@pytest.mark.parametrize("count", RANK_THRESHOLD_COUNTS)
def test_rank_distinct_thresholds(count):
    """1 .. 1023 distinct thresholds on one feature are ranked; 1024 are refused.  Thresholds that collapse after flooring
    to f32, -0.0 beside 0.0, -1e300 (-inf) and 1e300 (FLT_MAX) are among them and count once."""
    name = "thr_%d" % count
    assert ts.distinct_thresholds(built(name)[1], 3) == count
    plan = run(name)
    if count <= 1023:
        assert plan["path"] == "rank" and not plan["cache_hit"], plan
        assert plan["nslots"] == len(ts.features_used(built(name)[1], 24)), plan
    else:
        assert plan["path"] != "rank", plan


def test_rank_one_document():
    plan = run("thr_255_one_document")
    assert plan["path"] == "rank", plan


def test_rank_table_chunks():
    """A float4 group whose tables fill one chunk exactly (1024 + 512 floats, 512 + 512 + 512) takes no more rounds than the
    same group with one threshold per feature; one more table of 256 floats takes one round more.  Table depths 10, 1, 1, 1
    in one round, in both feature orders."""
    base = run("chunk_min")
    assert base["path"] == "rank" and base["nslots"] == 4, base
    for exact, more in (("chunk_1024_512", "chunk_1024_512_256"), ("chunk_512_512_512", "chunk_512_512_512_256"),
                        ("chunk_1024_512", "chunk_1024_512_2")):
        pe, pm = run(exact), run(more)
        assert pe["path"] == "rank" and pm["path"] == "rank", (pe, pm)
        assert pe["nrounds"] == base["nrounds"], (exact, pe, base)
        assert pm["nrounds"] == pe["nrounds"] + 1, (more, pm, pe)
    for name in ("chunk_depths_10_1_1_1", "chunk_depths_1_1_1_10"):
        plan = run(name)
        assert plan["path"] == "rank" and plan["nslots"] == 4 and plan["nrounds"] == base["nrounds"], (name, plan)


def test_rank_features_in_use():
    """Slot offsets ride in 16 bits: up to 170 features in use are ranked, 171 are not (odd and even counts on either side);
    all score exactly.  The two neighbours of the limit take different paths, and there is one limit."""
    plans = {}
    for k in RANK_FEATURE_COUNTS:
        assert len(ts.features_used(built("slots_%d" % k)[1], 176)) == k
        plans[k] = run("slots_%d" % k)
        if plans[k]["path"] == "rank":
            assert plans[k]["nslots"] == k, plans[k]
    is_rank = [plans[k]["path"] == "rank" for k in RANK_FEATURE_COUNTS]
    assert is_rank[0] and not is_rank[-1], plans
    assert sum(a != b for a, b in zip(is_rank, is_rank[1:])) == 1, plans
    assert plans[170]["path"] != plans[171]["path"], plans


def test_rank_depth_limit_and_batches():
    """A leaf exactly 10 levels deep is walked one tree per part; 11 levels are refused.  The walks per thread follow
    4 * n * (6 << L) <= 24576 bytes and the number of trees left: 8, 4, 2, 1."""
    plan = run("chains_10")
    assert plan["path"] == "rank" and plan["batches"] == [[1, 10]] * 3, plan  # 4 + 4 + 1 (three padding trees)
    plan = run("chain_10_alone")
    assert plan["path"] == "rank" and plan["batches"] == [[1, 10]], plan
    plan = run("chain_11_ensemble")
    assert plan["path"] == "lds", plan
    # 60 trees: 32 stumps (8 walks), 16 (4: fewer than 32 left), 8 (2: fewer than 16 left), the depth-10 chain with 3 stumps
    plan = run("walks_by_count")
    assert plan["path"] == "rank" and plan["batches"] == [[8, 1], [4, 1], [2, 1], [1, 10]], plan
    # depth 7: 32 * 768 B fit; depth 8: 16 * 1536 B; depth 9: 8 * 3072 B; depth 10: 4 * 6144 B
    plan = run("walks_by_depth")
    assert plan["path"] == "rank" and plan["batches"] == [[8, 7], [4, 8], [4, 8], [2, 9], [2, 9], [1, 10]], plan
    # 34 trees: the last two share a batch with two padding trees and take the depth of the deeper
    plan = run("tail_of_two")
    assert plan["path"] == "rank" and plan["batches"] == [[8, 1], [1, 2]], plan


def test_rank_all_leaf_forest_and_absent_features():
    plan = run("all_leaves")
    assert plan["path"] == "rank" and plan["nslots"] == 0 and plan["batches"] == [[1, 1], [1, 1]], plan
    plan = run("absent_features")  # every node reads 0.0: splits either side of it, +-0.0, +-1e-46
    assert plan["path"] == "rank" and plan["nslots"] == 0, plan


# ---------------------------------------------------------------------------------------------- f32 LDS walk

def test_lds_child_offset_limit(monkeypatch):
    """complete(8) has its largest child offset at exactly 255 and is walked in LDS; complete(9) is not.  A comb whose levels
    stay under the offset limit is admitted, one level wider is refused.  Both refused forests take the L2 walk with rows
    staged in LDS."""
    monkeypatch.setenv("FR_TREE_RANK", "0")
    assert ts.lds_layout(built("complete_8")[1][0])[1] == 255
    plan = run("complete_8")
    assert plan["path"] == "lds" and plan["batches"] == [[1, 8], [1, 1]], plan
    assert ts.lds_layout(built("complete_8_plus_one")[1][0])[1] == 256
    for name in ("complete_8_plus_one", "complete_9"):
        plan = run(name)
        assert plan["path"] == "l2" and plan["rows_in_lds"] is True, (name, plan)
    for admitted, refused, comb in (("comb_admitted", "comb_refused", COMB_ADMITTED), ("comb_left_admitted", "comb_left_refused", COMB_LEFT_ADMITTED)):
        plan = run(admitted)
        assert plan["path"] == "lds" and plan["batches"] == [[1, comb[0] + comb[1]]], plan
        plan = run(refused)
        assert plan["path"] == "l2" and plan["rows_in_lds"] is True, plan


@pytest.mark.parametrize("side", ts.SIDES)
@pytest.mark.parametrize("depth", CHAIN_DEPTHS)
def test_lds_chains(depth, side):
    """Chains of 11, 12, 33 levels and the deepest the model format admits, alone as a bare tree (one-part blocks) and in a
    batch with stumps, whose leaves stay put while the chain is walked."""
    levels = deepest_chain(True) if depth == "deepest" else int(depth)
    plan = run("bare_chain_%s_%s" % (depth, side))
    assert plan["path"] == "lds" and plan["parts"] == 1 and plan["batches"] == [[1, levels]], plan
    levels = deepest_chain(False) if depth == "deepest" else int(depth)
    plan = run("batched_chain_%s_%s" % (depth, side))
    # 12 trees in four parts: eight (the chain among them) two per part, then four stumps
    assert plan["path"] == "lds" and plan["parts"] == 4 and plan["batches"] == [[2, levels], [1, 1]], plan


@pytest.mark.parametrize("leaves", (255, 32))
def test_lds_leafwise_forests(leaves, monkeypatch):
    monkeypatch.setenv("FR_TREE_RANK", "0")
    plan = run("leafwise_%d" % leaves)
    assert plan["path"] == "lds", plan
    assert max(b[1] for b in plan["batches"]) == max(ts.rank_depth(t) for t in built("leafwise_%d" % leaves)[1]), plan


def test_lds_word_cap(monkeypatch):
    """The largest tree the first block shape takes, and the tree one split larger: the first is walked by that shape, the
    second by a later one; the caps come from the packer's shape table."""
    monkeypatch.setenv("FR_TREE_RANK", "0")
    _, order = lds_shape_table()
    under, over = (ts.lds_layout(built(n)[1][0])[0] for n in ("word_cap_under", "word_cap_over"))
    assert over == under + 2 and first_lds_shape(under, 24) == order[0]
    later = first_lds_shape(over, 24)
    assert later is not None and later != order[0]
    pu, po = run("word_cap_under"), run("word_cap_over")
    assert pu["path"] == "lds" and (pu["docs"], pu["parts"]) == order[0], pu
    assert po["path"] == "lds" and (po["docs"], po["parts"]) == later, po
    # the big tree walks beside padding trees; the stumps follow in a batch of their own
    assert pu["batches"][0][0] == 1 and po["batches"][0][0] == 1, (pu, po)


def wide_expectation(d):
    """What the packer's own numbers say a d-feature matrix gets with the rank walk off: the first block shape whose feature
    columns leave 8 KB of the 160 KB of LDS (the test forests' trees are small), else the L2 walk, whose 64 rows of
    4 * ceil(d / 4) + 1 floats are staged in LDS when they fit 150 KB."""
    fits = [s for s in lds_shape_table()[1] if lds_max_nodes(s, d) is not None]
    if fits:
        return {"path": "lds", "docs": fits[0][0], "parts": fits[0][1]}
    return {"path": "l2", "rows_in_lds": 64 * ((d + 3) // 4 * 4 + 1) * 4 <= 150 * 1024}


@pytest.mark.parametrize("name", WIDE)
def test_wide_matrices(name, monkeypatch):
    """Feature columns that leave no room for 192 or 256 documents per block (d = 200, 320) fall through to the 128- and
    64-document shapes.  The 64-document shapes hold up to 604 features (d = 600 is still theirs); from 605 on no shape fits
    and 64 rows do not fit LDS either: at d = 608 and 700 the L2 walk reads global memory.  The threshold-rank walk does not
    depend on d."""
    d = MATRICES[name][1]
    plan = run("wide_" + name)
    assert plan["path"] == "rank", plan
    monkeypatch.setenv("FR_TREE_RANK", "0")
    plan = run("wide_" + name)
    exp = wide_expectation(d)
    assert {k: plan[k] for k in exp} == exp, (plan, exp)
    if d in (200, 320):
        assert plan["path"] == "lds" and plan["docs"] == (128 if d == 200 else 64), plan
    if d == 700:
        assert plan["path"] == "l2" and plan["rows_in_lds"] is False, plan


def test_wide_matrix_limit_of_the_lds_walk(monkeypatch):
    """Either side of the widest matrix a block shape holds: d = 604 and d = 608 take different paths, both exact."""
    monkeypatch.setenv("FR_TREE_RANK", "0")
    below, above = run("wide_d604"), run("wide_d608")
    assert below["path"] != above["path"] and {below["path"], above["path"]} == {"lds", "l2"}, (below, above)
    assert wide_expectation(604)["path"] == below["path"] and wide_expectation(608) == {"path": "l2", "rows_in_lds": False}
    assert above["rows_in_lds"] is False, above


# ---------------------------------------------------------------------------------------------- the packed-forest cache

def test_rank_cache_interleaved_with_other_paths():
    """A second call with the same forest launches from the kept buffers; the LDS walk overwrites them (no hit afterwards),
    the L2 walk leaves them alone (a hit afterwards).  Every call's scores are checked."""
    g = fr.CDataset.from_numpy(*matrix("d24"))  # a dataset of this test's own: its cache starts empty
    steps = [("cache_a", "rank", False), ("cache_a", "rank", True), ("cache_b_lds", "lds", False), ("cache_a", "rank", False),
             ("cache_a", "rank", True), ("cache_c_l2", "l2", False), ("cache_a", "rank", True)]
    first = None
    for i, (name, path, hit) in enumerate(steps):
        plan = run(name, dataset=g)
        assert plan["path"] == path and plan["cache_hit"] is hit, (i, name, plan)
        if name == "cache_a":
            first = first or plan
            assert {k: plan[k] for k in ("nslots", "nrounds", "batches")} == {k: first[k] for k in ("nslots", "nrounds", "batches")}


def test_rank_cache_parent_view_and_changed_weight():
    """The same forest on a parent, on a query view of it and on the parent again: the view packs for itself and the parent
    still hits.  One changed weight is another forest."""
    X, y, qid = matrix("d24")
    g = fr.CDataset.from_numpy(X, y, qid)
    queries = sorted(set(qid.tolist()))[1::2]
    view = g.subsample_queries([str(q) for q in queries])
    rows = np.flatnonzero(np.isin(qid, queries))
    assert 0 < len(rows) < len(qid)
    plan = run("cache_a", dataset=g)
    assert plan["path"] == "rank" and plan["cache_hit"] is False, plan
    plan = run("cache_a", dataset=view, rows=rows)
    assert plan["path"] == "rank" and plan["cache_hit"] is False, plan
    plan = run("cache_a", dataset=g)
    assert plan["path"] == "rank" and plan["cache_hit"] is True, plan
    _, trees, weights, _, _, _ = built("cache_a")
    changed = list(weights)
    changed[17] = np.nextafter(changed[17], np.inf)
    model = fr.CModel.from_dict({"Ensemble": {"weights": changed, "models": [{"DecisionTree": t} for t in trees]}})
    got = native.predict_scores_dense(model, g)
    plan = native.last_tree_plan()
    assert plan["path"] == "rank" and plan["cache_hit"] is False, plan
    assert np.array_equal(got, oracle_dataset("d24").score_ensemble(trees, changed), equal_nan=True)
    assert np.array_equal(got, ts.score(X, trees, changed), equal_nan=True)
