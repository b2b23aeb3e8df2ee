"""The references of tests/test_gpu_tree_scoring.py, checked on the CPU: the numpy restatement of forest scoring
(tests/tree_shapes.py) equals the oracle's score_ensemble bit for bit on every forest the device tests use, the builders
have the shapes the device tests rely on, and the test matrices hold the values the boundary cases need."""
import numpy as np
import pytest

import fastrank_amd as fr
from tests import test_gpu_tree_scoring as cases
from tests import tree_shapes as ts


@pytest.mark.parametrize("name", sorted(cases.FORESTS))
def test_restatement_equals_the_oracle_bit_for_bit(name):
    _, trees, weights, _, oracle, restated = cases.built(name)
    assert oracle.dtype == restated.dtype == np.float64 and oracle.shape == restated.shape
    assert not np.isnan(oracle).any()
    assert oracle.tobytes() == restated.tobytes()
    assert len(set(oracle.tolist())) > 1 or len(oracle) == 1 or name in ("all_leaves", "absent_features")


def test_documents_walk_the_spines_to_their_ends():
    """The deep end of every chain, the last node of complete(8)'s widest level, the last level of the trees at the word
    cap: a good share of the 449 documents gets there, so a slip in those nodes shows in the scores."""
    for name in sorted(cases.FORESTS):
        mname = cases.built(name)[0]
        for tree, side in cases.SPINES.get(name, []):
            assert ts.reach_spine_end(cases.matrix(mname)[0], tree, side) >= 40, (name, side)
    for name in ("chains_10", "complete_8", "word_cap_under", "word_cap_over", "comb_admitted", "bare_chain_deepest_zigzag", "wide_d700"):
        assert cases.SPINES[name], name
    # the spine of the trees at the word cap ends on their last level
    big = cases.built("word_cap_under")[1][0]
    assert len(ts._spine(big, "left")) == ts.rank_depth(big)


def test_restatement_by_hand():
    X = np.float32([[1.0, np.nan], [2.0, -0.0], [np.float32(0.1), np.inf]])
    leaf = lambda v: {"LeafNode": v}
    split = lambda f, s, l, r: {"FeatureSplit": {"fid": f, "split": s, "lhs": l, "rhs": r}}
    # float64(x) <= split: f32 0.1 is above the double 0.1
    assert ts.score(X, split(0, 0.1, leaf(1.0), leaf(2.0)), None).tolist() == [2.0, 2.0, 2.0]
    assert ts.score(X, split(0, float(np.float32(0.1)), leaf(1.0), leaf(2.0)), None).tolist() == [2.0, 2.0, 1.0]
    # NaN goes right; -0.0 <= 0.0; an absent feature reads 0.0
    assert ts.score(X, split(1, 0.0, leaf(1.0), leaf(2.0)), None).tolist() == [2.0, 1.0, 2.0]
    assert ts.score(X, split(9, -1e-300, leaf(1.0), leaf(2.0)), None).tolist() == [2.0, 2.0, 2.0]
    assert ts.score(X, split(9, 0.0, leaf(1.0), leaf(2.0)), None).tolist() == [1.0, 1.0, 1.0]
    # a bare tree returns the leaf itself (-0.0 stays -0.0); an ensemble starts from +0.0 and adds w * leaf in tree order
    assert np.signbit(ts.score(X, leaf(-0.0), None)).all()
    assert not np.signbit(ts.score(X, [leaf(-0.0)], [1.0])).any()
    big = ts.score(X, [leaf(1.0), leaf(1.0), leaf(1.0)], [1e16, 1.0, -1e16])
    assert big.tolist() == [0.0, 0.0, 0.0] and ts.score(X, [leaf(1.0)] * 3, [1e16, -1e16, 1.0]).tolist() == [1.0] * 3
    # zip stops at the shorter side
    assert ts.score(X, [leaf(1.0), leaf(5.0)], [2.0]).tolist() == [2.0, 2.0, 2.0]


def test_builders_have_their_shapes():
    p = cases.picker(1, range(24))
    for depth in (0, 1, 5):
        t = ts.complete(depth, p)
        assert ts.lds_layout(t)[0] == 2 ** (depth + 1) - 1 and ts.rank_depth(t) == depth
    for side in ts.SIDES:
        t = ts.chain(9, side, p)
        nodes, rel, levels = ts.lds_layout(t)
        assert (nodes, levels) == (19, 9) and rel <= 2
    node, went = ts.chain(6, "zigzag", p), []
    while "FeatureSplit" in node:
        fs = node["FeatureSplit"]
        went.append("FeatureSplit" in fs["lhs"])
        node = fs["lhs"] if "FeatureSplit" in fs["lhs"] else fs["rhs"]
    assert went[:5] == [True, False, True, False, True]
    t = ts.comb(5, 3, p, "right")
    assert ts.rank_depth(t) == 8 and ts.lds_layout(t)[0] == 2 * (5 * 8 + 1) - 1
    for leaves in (1, 2, 32, 255):
        assert (ts.lds_layout(ts.leafwise(leaves, p))[0] + 1) // 2 == leaves
        assert (ts.lds_layout(ts.banded(leaves, 4, p))[0] + 1) // 2 == leaves
    assert ts.leafwise(40, cases.picker(5, [1, 2])) == ts.leafwise(40, cases.picker(5, [1, 2]))
    stumps = ts.stumps_with_thresholds(3, [1.5, 2.5], p)
    assert [s["FeatureSplit"]["split"] for s in stumps] == [1.5, 2.5] and all(s["FeatureSplit"]["fid"] == 3 for s in stumps)


def test_floor_and_threshold_counts():
    assert ts.floor_f32(1e300) == cases.FLT_MAX and ts.floor_f32(-1e300) == np.float32(-np.inf)
    assert ts.floor_f32(0.1) == np.nextafter(np.float32(0.1), np.float32(-1)) and ts.floor_f32(0.5) == np.float32(0.5)
    assert ts.floor_f32(-1e-46) == np.float32(-1e-45) and ts.floor_f32(1e-46) == 0 and not np.signbit(ts.floor_f32(1e-46))
    for count in cases.RANK_THRESHOLD_COUNTS:
        values = cases.threshold_set(count)
        assert ts.distinct_thresholds(cases.built("thr_%d" % count)[1], 3) == count
        assert len(set(values)) > count or count == 1  # some collapse
    big = cases.threshold_set(1023)
    assert -1e300 in big and 1e300 in big and any(np.signbit(v) and v == 0 for v in big) and any(not np.signbit(v) and v == 0 for v in big)


def test_lds_layout_limits_of_the_shapes_used():
    """The child offset of the breadth-first layout is 8 bits: which of the device tests' trees stay under it."""
    assert ts.lds_layout(cases.built("complete_8")[1][0])[1] == 255
    assert ts.lds_layout(cases.built("complete_8_plus_one")[1][0])[1] == 256
    assert ts.lds_layout(cases.built("complete_9")[1][0])[1] > 255
    assert ts.lds_layout(cases.built("comb_admitted")[1][0])[1] == 255 < ts.lds_layout(cases.built("comb_refused")[1][0])[1]
    assert ts.lds_layout(cases.built("comb_left_admitted")[1][0])[1] <= 255 < ts.lds_layout(cases.built("comb_left_refused")[1][0])[1]
    for a, r in ((cases.COMB_ADMITTED, cases.COMB_REFUSED), (cases.COMB_LEFT_ADMITTED, cases.COMB_LEFT_REFUSED)):
        assert r == (a[0], a[1] + 1, a[2])  # one subtree level wider
    assert ts.lds_layout(cases.built("cache_c_l2")[1][0])[1] > 255 and ts.rank_depth(cases.built("cache_c_l2")[1][0]) > 10
    for name in ("leafwise_255", "leafwise_32", "word_cap_under", "word_cap_over"):
        assert max(ts.lds_layout(t)[1] for t in cases.built(name)[1]) <= 255, name
    assert max(ts.rank_depth(t) for t in cases.built("leafwise_255")[1]) > 10
    # the word cap of the first shape tried lies between the two trees
    _, order = cases.lds_shape_table()
    cap = cases.lds_max_nodes(order[0], 24)
    under, over = (ts.lds_layout(cases.built(n)[1][0])[0] for n in ("word_cap_under", "word_cap_over"))
    assert under <= cap < over == under + 2
    assert cases.first_lds_shape(over, 24) not in (None, order[0])


def test_deepest_chain_the_model_format_admits():
    """The parser stops at 128 nested containers: a bare chain may be about 60 levels deep, one inside an ensemble a little less."""
    bare, member = cases.deepest_chain(True), cases.deepest_chain(False)
    assert 55 <= member <= bare <= 64
    t = ts.chain(bare + 1, "left", cases.picker(0, [0]))
    with pytest.raises(Exception, match="recursion limit exceeded"):
        fr.CModel.from_dict({"DecisionTree": t})


def test_matrices_hold_the_boundary_values():
    grid = set(cases.GRID.tolist())
    above = set(np.nextafter(cases.GRID, np.float32(np.inf)).tolist())
    below = set(np.nextafter(cases.GRID, np.float32(-np.inf)).tolist())
    for name, (n, d) in cases.MATRICES.items():
        X, y, qid = cases.matrix(name)
        assert X.shape == (n, d) and X.dtype == np.float32
        if n == 1:
            continue
        assert n == 449 and len(set(qid.tolist())) > 3
        for j in range(d):
            col = X[:, j]
            vals = set(col[np.isfinite(col)].tolist())
            assert vals & grid and vals & above and vals & below, (name, j)
            assert np.isnan(col).any() and np.isposinf(col).any() and np.isneginf(col).any(), (name, j)
            zeros = col[col == 0]
            assert np.signbit(zeros).any() and not np.signbit(zeros).all(), (name, j)
            assert ((col != 0) & (np.abs(col) < np.float32(1.1754944e-38))).sum() >= 4, (name, j)
    w = np.asarray(cases.weights_for(40, 3))
    assert (w > 0).any() and (w < 0).any() and np.abs(w).max() / np.abs(w).min() > 1e8
