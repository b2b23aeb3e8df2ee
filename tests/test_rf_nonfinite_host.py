"""The oracle's random-forest trainer (oracle/fastrank_oracle.c, rf_learn_recursive) on +inf, -inf and NaN feature values,
against outcomes derived BY HAND from the reference's source -- the oracle is the thing under test here, and the reference
cannot be run.  tests/rf_nonfinite_cases.py states the rule with its line numbers; every docstring below applies it to one
case.  No tolerances: a forest is compared as values, an error is an exception."""
import numpy as np
import pytest

from oracle import pyoracle as o
from tests import rf_nonfinite_cases as nf

INF = float("inf")


def _learn(X, y, qid, params, present=None):
    c = o.Dataset(X, y, qid)
    if present is not None:
        c.set_presence(present)
    trees, w, _ = c.rf_learn("ndcg", params)
    return c, trees, w


def _panics(X, y, qid, params, present=None):
    with pytest.raises(RuntimeError, match="error 2"):
        _learn(X, y, qid, params, present)


# --- one feature, ten instances ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("method", nf.METHODS[:3])
def test_one_plus_inf_splits_the_root_at_plus_inf(method):
    """Row 9 holds +inf.  Root: min = 1, max = +inf (stats.rs:74-79), range = +inf, so each of the 31 positions is
    f * inf + 1 = +inf (random_forest.rs:236-239); the nine finite values are below it, ids_i = 9 for every position and
    :249-253 keeps one candidate; 9 and 1 instances pass min_leaf_support = 1 (:262-266).  It is the only candidate of the
    only feature: split = +inf, the finite rows on the left, row 9 alone on the right -- a leaf of its label 12
    (label_stats of one instance is None, :218).  SquaredError then fits the finite rows exactly, as in the reference's
    own test (:465-506)."""
    X, y, qid = nf.ten()
    X[9, 0] = nf.INF
    c, trees, _ = _learn(X, y, qid, nf.ten_params(method))
    root = trees[0]["FeatureSplit"]
    assert root["fid"] == 0 and root["split"] == INF
    assert root["rhs"] == {"LeafNode": 12.0}
    assert all(np.isfinite(s) for s in nf.splits(root["lhs"])), "below the root only finite rows are left"
    scores = c.score_ensemble(trees, [1.0])
    if method == "SquaredError":
        assert np.array_equal(scores, y)
    else:  # (every label is positive: Gini and entropy are 0 everywhere and pick among ties; the root has no choice)
        assert scores[9] == 12.0


def test_one_plus_inf_true_variance_reduction():
    """TrueVarianceReduction needs min_leaf_support >= 2 or label_stats(..).unwrap() fails on a side of one (:119-120).
    With ONE +inf row the root's only candidate has a right side of 1 < 2 and is dropped at :262-266 before any importance
    is computed: no candidate, the tree is the leaf of the mean, 70 / 10.  With TWO (rows 8 and 9) the sides are 8 and 2:
    split = +inf, and the right side -- both labels 12, label_stats.max == min (:219) -- is a leaf."""
    X, y, qid = nf.ten()
    X[9, 0] = nf.INF
    _, trees, _ = _learn(X, y, qid, nf.ten_params("TrueVarianceReduction"))
    assert trees == [{"LeafNode": 7.0}]
    X[8, 0] = nf.INF
    _, trees, _ = _learn(X, y, qid, nf.ten_params("TrueVarianceReduction"))
    root = trees[0]["FeatureSplit"]
    assert root["split"] == INF and root["rhs"] == {"LeafNode": 12.0} and "FeatureSplit" in root["lhs"]


@pytest.mark.parametrize("method", nf.METHODS)
def test_one_minus_inf_is_the_position_panic(method):
    """Row 0 holds -inf.  Root: labels differ, min = -inf, max = 9, range = +inf; the first position is
    (1/32) * inf + -inf = NaN and NotNan::new(..).unwrap() panics (random_forest.rs:238) -- before any importance, so for
    every split method."""
    X, y, qid = nf.ten()
    X[0, 0] = -nf.INF
    _panics(X, y, qid, nf.ten_params(method))


@pytest.mark.parametrize("method", nf.METHODS)
def test_all_plus_inf_is_a_leaf_not_a_panic(method):
    """Every row holds +inf.  max becomes +inf, but `self.min > x` (stats.rs:77) is false for min = f64::MAX and x = +inf:
    the minimum STAYS f64::MAX (stats.rs:47), it is not +inf.  range = inf - f64::MAX = +inf, every position is
    f * inf + f64::MAX = +inf -- not NaN, no panic at :238.  No value is below +inf: ids_i = 0, one candidate with an empty
    left side, dropped by min_leaf_support >= 1 (:262-266).  No candidate: the tree is the leaf of the mean.
    (Were both ends read off the data, min = max = +inf would give range = NaN; the reference does not do that.)"""
    X, y, qid = nf.ten()
    X[:, 0] = nf.INF
    _, trees, _ = _learn(X, y, qid, nf.ten_params(method))
    assert trees == [{"LeafNode": 7.0}]


def test_all_plus_inf_with_no_leaf_support_splits_off_an_empty_side():
    """The same column with min_leaf_support = 0 (SquaredError): the candidate at ids_i = 0 passes :262-266, its importance
    is -(0 + the node's squared error) (compute_output of no instance is 0.0, :33-35), and it is chosen: split = +inf, the
    left child -- no instance, StepDone -- is the leaf 0.0, the right child holds all ten rows again, one level deeper.
    max_depth = 3 stops that at the third level (:371)."""
    X, y, qid = nf.ten()
    X[:, 0] = nf.INF
    _, trees, _ = _learn(X, y, qid, nf.ten_params(min_leaf_support=0, max_depth=3))
    leaf0, mean = {"LeafNode": 0.0}, {"LeafNode": 7.0}
    inner = {"FeatureSplit": {"fid": 0, "split": INF, "lhs": leaf0, "rhs": mean}}
    assert trees == [{"FeatureSplit": {"fid": 0, "split": INF, "lhs": leaf0, "rhs": inner}}]


@pytest.mark.parametrize("nan", [nf.NAN_POS, nf.NAN_NEG], ids=["nan", "nan_sign_bit"])
@pytest.mark.parametrize("method", nf.METHODS)
def test_one_nan_is_the_scored_new_panic(method, nan):
    """Row 3 holds NaN.  The root's stats count ten elements (the NaN is pushed, stats.rs:70, and changes neither end), so
    the feature has stats; the labels differ; Scored::new(NaN, 3) panics at random_forest.rs:228 ("NaN found!",
    core.rs:53) -- whatever the NaN's sign bit, and also with split_candidates = 1, where `(1..k)` is empty but the values
    are wrapped first."""
    X, y, qid = nf.ten()
    X[3, 0] = nan
    _panics(X, y, qid, nf.ten_params(method))
    _panics(X, y, qid, nf.ten_params(method, split_candidates=1))


@pytest.mark.parametrize("method", nf.METHODS)
def test_one_nan_with_equal_labels_is_never_looked_at(method):
    """Row 3 holds NaN and every label is 7: label_stats.max == label_stats.min, generate_split_candidate returns None at
    random_forest.rs:219-221, before :228.  No candidate: a leaf of 7."""
    X, y, qid = nf.ten()
    X[3, 0] = nf.NAN_POS
    y[:] = 7.0
    _, trees, _ = _learn(X, y, qid, nf.ten_params(method))
    assert trees == [{"LeafNode": 7.0}]


@pytest.mark.parametrize("method", nf.METHODS)
def test_one_nan_with_max_depth_one_is_never_looked_at(method):
    """Row 3 holds NaN and max_depth = 1: learn_recursive returns DepthExceeded at random_forest.rs:371-373 (current_depth
    starts at 1, :345), before FeatureStats is computed.  A leaf of the mean, 70 / 10.  The same for a -inf row."""
    X, y, qid = nf.ten()
    X[3, 0] = nf.NAN_POS
    X[0, 0] = -nf.INF
    _, trees, _ = _learn(X, y, qid, nf.ten_params(method, max_depth=1))
    assert trees == [{"LeafNode": 7.0}]


def test_a_nan_the_node_does_not_hold_reads_zero():
    """File-loaded data: an instance that does not HOLD the feature reads 0.0 in the sort (`unwrap_or(0.0)`,
    random_forest.rs:228) and is skipped by the stats (normalizers.rs:23-27).  So what the matrix carries at an absent
    position is never seen -- here it is 0.0, as the loader leaves it -- and a HELD NaN is the panic only when the feature
    has stats at all: with one held value besides absent ones there are none (stats.rs:98-100) and the NaN stays silent."""
    X, y, qid = nf.ten()
    present = np.zeros((10, 1), dtype=bool)
    present[3, 0] = True
    X[:, 0] = 0.0
    X[3, 0] = nf.NAN_POS
    _, trees, _ = _learn(X, y, qid, nf.ten_params(), present)
    assert trees == [{"LeafNode": 7.0}]
    present[4, 0] = True  # two held values, one of them NaN: stats exist, Scored::new panics
    _panics(X, y, qid, nf.ten_params(), present)
    # two held finite values, and a NaN in the matrix where the instance holds nothing: read as 0.0, never seen
    X[:, 0] = [0, 0, 0, 5, 9, 0, 0, 0, 0, 0]
    _, want, _ = _learn(X, y, qid, nf.ten_params(), present)
    X[0, 0] = nf.NAN_POS
    _, got, _ = _learn(X, y, qid, nf.ten_params(), present)
    assert got == want and "FeatureSplit" in want[0]


# --- 200 documents x 4 features -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("method", nf.METHODS)
@pytest.mark.parametrize("kind", ["minus_inf", "both_inf", "nan", "nan_sign_bit"])
def test_two_hundred_documents_reach_the_panic(kind, method):
    """Both sampling rates are 1.0: every tree's root holds all 200 rows and all four features, its labels differ, and
    column 1 has stats.  -inf rows (alone or beside +inf rows) make the root's minimum -inf: the position panic (:238).
    A NaN row is the Scored::new panic (:228).  Either ends the call (:305)."""
    X, y, qid = nf.two_hundred()
    _panics(nf.edit_column(X, kind), y, qid, nf.two_hundred_params(method))


@pytest.mark.parametrize("method", nf.METHODS)
def test_two_hundred_documents_with_plus_inf_rows_carry_an_infinite_split(method):
    """+inf in 23 rows of column 1, minimum finite: no panic; column 1's one candidate at a root is (177 finite | 23 +inf)
    with split = +inf, and competes with the other columns' candidates by importance.  The case is only worth something
    if such a split is really chosen somewhere: asserted.  Finite rows go left of it, the +inf rows right."""
    X, y, qid = nf.two_hundred()
    Xe = nf.edit_column(X, "plus_inf")
    c, trees, w = _learn(Xe, y, qid, nf.two_hundred_params(method))
    all_splits = [s for t in trees for s in nf.splits(t)]
    assert any(s == INF for s in all_splits), "the +inf case must contain an infinite split"
    assert not any(np.isnan(s) or s == -INF for s in all_splits)
    assert np.isfinite(c.score_ensemble(trees, w)).all()


def test_two_hundred_documents_all_plus_inf_column_is_silently_unused():
    """Column 1 all +inf: its one candidate has an empty left side and min_leaf_support = 2 drops it (see
    test_all_plus_inf_is_a_leaf_not_a_panic).  The column yields no candidate in any node, like a constant column: the
    forest is the one grown with that column constant, fid 1 never appears."""
    X, y, qid = nf.two_hundred()
    _, trees, _ = _learn(nf.edit_column(X, "all_plus_inf"), y, qid, nf.two_hundred_params())
    Xc = X.copy()
    Xc[:, 1] = 3.0
    _, const_trees, _ = _learn(Xc, y, qid, nf.two_hundred_params())
    assert trees == const_trees
    assert any("FeatureSplit" in t for t in trees) and '"fid": 1' not in __import__("json").dumps(trees)


def test_finite_data_is_untouched_by_the_checks():
    """The two checks read, they change nothing: the unedited 200 x 4 set grows real trees with finite splits only."""
    X, y, qid = nf.two_hundred()
    for method in nf.METHODS:
        _, trees, _ = _learn(X, y, qid, nf.two_hundred_params(method))
        s = [v for t in trees for v in nf.splits(t)]
        assert len(s) >= 3 and np.isfinite(s).all()
