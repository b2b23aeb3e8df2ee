"""Data and requests shared by tests/test_rf_nonfinite_host.py (the oracle against outcomes derived by hand from the
reference) and tests/test_gpu_rf_nonfinite.py (the device trainer against the oracle): feature matrices that hold +inf,
-inf or NaN, for the random-forest trainer.

The reference's rule, from src/random_forest.rs:211-286 and :362-408, src/core.rs:50-55, src/stats.rs:40-104 (release build):
  * FeatureStats::compute pushes every value the node's instances HOLD.  StreamingStats starts at min = f64::MAX and
    max = f64::MIN (stats.rs:46-47) and compares with `>` and `<` (:74-79): a NaN counts as an element but never becomes
    min or max; -inf becomes the minimum, +inf the maximum -- but a column of nothing but +inf keeps min = f64::MAX
    (`f64::MAX > inf` is false), and one of nothing but -inf keeps max = f64::MIN.
  * generate_split_candidate returns None when the node's labels are all equal (:218-221).  Otherwise it wraps every
    instance's value in Scored::new (:228), which panics on NaN ("NaN found!", core.rs:53), and then builds the
    positions NotNan::new(f * range + stats.min).unwrap() (:238), which panics when that is NaN: exactly when the
    minimum is -inf (range = max - -inf = +inf, and inf + -inf is NaN).
  * min finite, max +inf: range = +inf, every position is +inf, every finite value lies below it, so the one candidate
    that survives :249-253 has the finite rows on the left and the +inf rows on the right; the tree carries
    split = +inf, which serde_json writes as null.
  * nothing but +inf: min = f64::MAX, range = +inf, every position is +inf, no value is below it: the one candidate has
    an EMPTY left side -- dropped by min_leaf_support >= 1 (:262-266), evaluated when it is 0.  No panic.
  * a panic in any tree of the par_extend (:305) ends the call.
"""
import struct

import numpy as np

METHODS = ["SquaredError", "BinaryGiniImpurity", "InformationGain", "TrueVarianceReduction"]
NAN_POS = np.frombuffer(struct.pack("<I", 0x7FC00000), dtype=np.float32)[0]
NAN_NEG = np.frombuffer(struct.pack("<I", 0xFFC00000), dtype=np.float32)[0]
INF = np.float32(np.inf)


def ten():
    """The data of test_regression_tree_known_answer_through_training (src/random_forest.rs:465-506)."""
    X = np.array([1, 1, 2, 3, 4, 5, 6, 7, 8, 9], dtype=np.float32)[:, None]
    y = np.array([7, 7, 7, 7, 2, 2, 2, 12, 12, 12], dtype=np.float64)
    qid = np.zeros(10, dtype=np.int64)
    return X, y, qid


def ten_params(method="SquaredError", **kw):
    p = dict(seed=5, num_trees=1, weight_trees=False, split_method=method, instance_sampling_rate=1.0, feature_sampling_rate=1.0,
             min_leaf_support=2 if method == "TrueVarianceReduction" else 1, split_candidates=32, max_depth=10)
    p.update(kw)
    return p


def two_hundred():
    """200 documents x 4 features in 10 queries of 20, labels 0..2.  The rows edit_column() edits (every ninth) all carry
    label 2, so that splitting them off is worth something to every split method."""
    rng = np.random.default_rng(200)
    X = rng.random((200, 4)).astype(np.float32)
    y = rng.integers(0, 3, 200).astype(np.float64)
    y[::9] = 2.0
    qid = np.repeat(np.arange(1, 11, dtype=np.int64), 20)
    return X, y, qid


def two_hundred_params(method="SquaredError", **kw):
    p = dict(seed=5, num_trees=3, weight_trees=False, split_method=method, instance_sampling_rate=1.0, feature_sampling_rate=1.0,
             min_leaf_support=2, split_candidates=8, max_depth=5)
    p.update(kw)
    return p


def four_hundred():
    """400 documents x 8 features in 20 queries of 20, labels as in two_hundred(): enough items per tree for
    FR_RF_BATCH_BYTES to cut a forest into several batches."""
    rng = np.random.default_rng(400)
    X = rng.random((400, 8)).astype(np.float32)
    y = rng.integers(0, 3, 400).astype(np.float64)
    y[::9] = 2.0
    qid = np.repeat(np.arange(1, 21, dtype=np.int64), 20)
    return X, y, qid


def write_ranksvm(path, token, seed=7):
    """A ranksvm file of 60 rows in 3 queries over features 1..3 (a dense row also holds index 0, src/instance.rs:108-115):
    every fifth row leaves feature 3 out, every seventh (other) row carries `token` ("inf", "-inf", "NaN", or a number) as
    its feature 3 and label 2.  Returns (X, y, qid) as a dense 60 x 4 matrix with 0.0 at what a row does not hold."""
    rng = np.random.default_rng(seed)
    X = np.zeros((60, 4), dtype=np.float32)
    X[:, 1:] = np.round(rng.random((60, 3)), 3).astype(np.float32)
    y = rng.integers(0, 3, 60).astype(np.float64)
    qid = np.repeat(np.arange(1, 4, dtype=np.int64), 20)
    with open(path, "w") as fh:
        for i in range(60):
            cols = ["1:%s" % repr(float(X[i, 1])), "2:%s" % repr(float(X[i, 2]))]
            if i % 5 == 0:
                X[i, 3] = 0.0
            elif i % 7 == 0:
                X[i, 3] = np.float32(float(token))
                y[i] = 2.0
                cols.append("3:%s" % token)
            else:
                cols.append("3:%s" % repr(float(X[i, 3])))
            fh.write("%d qid:%d %s\n" % (int(y[i]), int(qid[i]), " ".join(cols)))
    return X, y, qid


def edit_column(X, kind, col=1):
    """Column `col` of a copy of X with the non-finite values of case `kind`."""
    X = X.copy()
    if kind == "plus_inf":
        X[::9, col] = INF
    elif kind == "minus_inf":
        X[::9, col] = -INF
    elif kind == "both_inf":
        X[::9, col] = -INF
        X[1::9, col] = INF
    elif kind == "all_plus_inf":
        X[:, col] = INF
    elif kind == "nan":
        X[3, col] = NAN_POS
    elif kind == "nan_sign_bit":
        X[3, col] = NAN_NEG
    else:
        raise ValueError(kind)
    return X


def splits(node, out=None):
    """Every FeatureSplit threshold of a tree in the reference's JSON shape, root first."""
    out = [] if out is None else out
    if "FeatureSplit" in node:
        fs = node["FeatureSplit"]
        out.append(fs["split"])
        splits(fs["lhs"], out)
        splits(fs["rhs"], out)
    return out


def as_json_tree(node):
    """The tree as the reference's to_json shows it: serde_json writes a non-finite f64 as null."""
    if "LeafNode" in node:
        return {"LeafNode": node["LeafNode"]}
    fs = node["FeatureSplit"]
    s = fs["split"]
    return {"FeatureSplit": {"fid": fs["fid"], "split": s if np.isfinite(s) else None, "lhs": as_json_tree(fs["lhs"]), "rhs": as_json_tree(fs["rhs"])}}


def flat_nodes(node, out=None):
    """Node by node, root first: (fid, the split or the leaf value as its f64 bit pattern; None for JSON's null)."""
    out = [] if out is None else out

    def bits(v):
        return None if v is None else struct.unpack("<Q", struct.pack("<d", float(v)))[0]

    if "LeafNode" in node:
        out.append((-1, bits(node["LeafNode"])))
    else:
        fs = node["FeatureSplit"]
        out.append((int(fs["fid"]), bits(fs["split"])))
        flat_nodes(fs["lhs"], out)
        flat_nodes(fs["rhs"], out)
    return out
