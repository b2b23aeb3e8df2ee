"""tests/rf_level_model.py -- the restatement tests/test_gpu_rf_levels.py holds the device's level step to -- anchored to the
oracle: grown to max_depth on one-tree requests whose sample is the whole dataset in row order, it must give
oracle.Dataset.rf_learn's tree as an identical dict (structure, thresholds and leaf values bit for bit), for every split
method, label kind, candidate count and leaf support, with a file-style presence mask, a constant column and a column of
signed zeros.  No device, no tolerance."""
import numpy as np
import pytest

from oracle import pyoracle as o
from tests import rf_level_model as lm

METHODS = ("SquaredError", "BinaryGiniImpurity", "InformationGain", "TrueVarianceReduction")


def make(seed, n, labels):
    """Rows grouped by ascending qid (the tree's sample is arange(n)); a real column, an integer column (ties) and a sparse one."""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.random(n), np.floor(rng.exponential(2.0, n)), np.where(rng.random(n) < 0.6, 0.0, rng.normal(size=n))], axis=1).astype(np.float32)
    y = rng.choice(5, size=n, p=[0.5, 0.3, 0.12, 0.05, 0.03]).astype(np.float64)
    y = np.where(X[:, 0] > 0.6, np.minimum(y + 1, 4), y)
    if labels == "frac":
        y = y + np.round(rng.random(n), 3)
    elif labels == "huge":
        y = y * 3.0e6  # above 2^21
    elif labels == "negative":
        y = y - 2.0
    elif labels == "wide":  # exponents far apart: an f64 sum of these f32 values rounds, so its order shows in the leaves
        y = (y + 1.0) * rng.lognormal(0.0, 6.0, n) * np.where(rng.random(n) < 0.3, -1.0, 1.0)
    qid = np.sort(rng.integers(1, max(2, n // 20), size=n)).astype(np.int64)
    return X, y, qid


def oracle_tree(X, y, qid, k, method, min_leaf, max_depth, present=None, seed=5):
    c = o.Dataset(X, y, qid)
    if present is not None:
        c.set_presence(present)
    params = dict(seed=seed, num_trees=1, weight_trees=False, split_method=METHODS[method], instance_sampling_rate=1.0,
                  feature_sampling_rate=1.0, min_leaf_support=min_leaf, split_candidates=k, max_depth=max_depth)
    trees, _, sample = c.rf_learn("map", params)
    assert tuple(sample[0]) == (X.shape[1], len(y))
    return trees[0]


def feature_order(d, seed=5):
    """The tree's feature list: the sorted features shuffled under the tree's own seed, all of them taken (rate 1.0)."""
    return o.shuffle_with_seed(int(o.rand64_stream(seed, 1)[0]), d).astype(np.int64)


def model_tree(X, y, k, method, min_leaf, max_depth, present=None, seed=5, **kw):
    rec = lm.grow(X, present, y, [np.arange(len(y))], [feature_order(X.shape[1], seed)], k, method, min_leaf, max_depth, **kw)
    return rec["trees"][0], rec


@pytest.mark.parametrize("k", [2, 3, 32, 66, 130])
@pytest.mark.parametrize("method", [0, 1, 2, 3])
def test_restatement_grows_the_oracles_tree(method, k):
    n = 150 if (method == 3 and k >= 32) else 500
    splits = 0
    for li, labels in enumerate(("int", "frac", "huge", "negative", "wide")):
        for min_leaf in ((2, 3, 10) if method == 3 else (0, 1, 2, 10)):
            X, y, qid = make(100 * k + 10 * li + min_leaf, n + 7 * min_leaf, labels)
            want = oracle_tree(X, y, qid, k, method, min_leaf, 5)
            got, rec = model_tree(X, y, k, method, min_leaf, 5)
            assert got == want, (labels, min_leaf)
            splits += str(got).count("FeatureSplit")
            assert len(rec["levels"]) <= 4
    assert splits > 20, "real trees expected"


@pytest.mark.parametrize("method", [0, 1, 2, 3])
def test_presence_mask_moves_the_range_not_the_sort(method):
    """A file-loaded dataset: an absent value sorts as 0.0 between the negative and positive held values and is left out of the
    range the thresholds sit on."""
    X, y, qid = make(77, 600, "frac")
    X[:, 1] += np.float32(3.0)  # (its absent rows, read as 0.0, sort below every held value and outside the range)
    rng = np.random.default_rng(3)
    present = rng.random(X.shape) < 0.7
    present[:, 0] = True
    present[:300, 1] = False
    present[5, 1] = True  # a deep node may hold one value of feature 1, or none
    X = np.where(present, X, np.float32(0.0)).astype(np.float32)
    ml = 2 if method == 3 else 1
    want = oracle_tree(X, y, qid, 8, method, ml, 6, present=present)
    got, rec = model_tree(X, y, 8, method, ml, 6, present=present)
    assert got == want
    dense, drec = model_tree(X, y, 8, method, ml, 6)
    assert dense == oracle_tree(X, y, qid, 8, method, ml, 6)
    fi = list(feature_order(3)).index(1)  # the root's thresholds on feature 1 start at 3.0 with the mask and at 0.0 without
    assert rec["levels"][0]["cands"][0, fi]["position"].min() > 3.0 > drec["levels"][0]["cands"][0, fi]["position"].min()
    seg = rec["levels"][0]["sv"][fi * 600:(fi + 1) * 600]  # "not held" is -0.0 in the sorted values, and sorts first here
    assert (seg == 0).sum() == int((~present[:, 1]).sum()) and np.signbit(seg[seg == 0]).all() and (seg[:299] == 0).all()


@pytest.mark.parametrize("method", [0, 1, 2])
def test_constant_column_splits_off_an_empty_left_side(method):
    """min_leaf_support = 0: a constant column's range is 0, every position is its value, ids_i = 0 -- the first candidate is
    evaluated with an empty left side, whose output is 0.0."""
    X, y, qid = make(9, 300, "int")
    X[:, :] = np.float32(1.5)
    want = oracle_tree(X, y, qid, 3, method, 0, 3)
    got, rec = model_tree(X, y, 3, method, 0, 3)
    assert got == want and got["FeatureSplit"]["lhs"] == {"LeafNode": 0.0}
    assert int(rec["levels"][0]["splits"][0]["pos"]) == 0


@pytest.mark.parametrize("method", [0, 1, 2, 3])
def test_signed_zeros_are_one_value(method):
    X, y, qid = make(21, 400, "frac")
    rng = np.random.default_rng(8)
    X[:, 1] = np.where(rng.random(400) < 0.5, np.float32(-0.0), np.float32(0.0))
    X[:, 2] = np.where(rng.random(400) < 0.3, np.float32(-0.0), X[:, 2])
    assert np.signbit(X[:, 1]).any() and not np.signbit(X[:, 1]).all()
    ml = 2 if method == 3 else 0
    want = oracle_tree(X, y, qid, 3, method, ml, 4)
    got, _ = model_tree(X, y, 3, method, ml, 4)
    assert got == want


@pytest.mark.parametrize("min_leaf,column", [(1, "one_low"), (0, "constant")])
def test_variance_of_fewer_than_two_labels_is_the_references_panic(min_leaf, column):
    """The two error cases: TrueVarianceReduction with a one-label side (min_leaf_support = 1) and with an empty side
    (min_leaf_support = 0, a constant column).  The oracle reports the panic; the restatement raises."""
    X, y, qid = make(4, 200, "int")
    if column == "constant":
        X[:, :] = np.float32(2.0)
    else:
        X[:, :] = np.float32(1.0)
        X[17, :] = np.float32(0.0)
    with pytest.raises(RuntimeError, match="error 2"):
        oracle_tree(X, y, qid, 2, 3, min_leaf, 3)
    with pytest.raises(lm.ReferencePanic):
        model_tree(X, y, 2, 3, min_leaf, 3)


def test_a_flipped_detail_of_the_restatement_no_longer_matches_the_oracle():
    """The anchor has teeth: an unstable sort on a column of ties, or searchsorted(.., 'right'), grows another tree."""
    X, y, qid = make(1234, 900, "wide")
    X = np.floor(X * 5).astype(np.float32)  # ties in every column: their order decides the order of the sums
    want = oracle_tree(X, y, qid, 8, 0, 1, 6)
    assert model_tree(X, y, 8, 0, 1, 6)[0] == want
    assert model_tree(X, y, 8, 0, 1, 6, side="right")[0] != want
    assert model_tree(X, y, 8, 0, 1, 6, stable=False)[0] != want
