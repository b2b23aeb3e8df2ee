"""Deterministic forest builders for the tree-scoring tests, and a plain numpy restatement of how a forest is scored.

The builders (complete, chain, comb, leafwise, banded, stumps_with_thresholds, ..., Picker) live in tools/forest_shapes.py,
which tools/fuzz_trees.py draws from too (a tool does not import the test tree); they are loaded from that file here and
are this module's names.  Every builder returns a tree in the reference's JSON shape ({"FeatureSplit": {"fid", "split",
"lhs", "rhs"}} | {"LeafNode": v}).

The restatement `score` follows src/model.rs:64-84,104-112: go left iff float64(x) <= split, a feature the matrix does not
hold reads 0.0, acc = acc + w * leaf in tree order from +0.0, and a bare DecisionTree returns the leaf itself.

`floor_f32`, `distinct_thresholds`, `lds_layout` and `rank_depth` restate, on the host, the quantities the device packers'
limits are stated in, so that a test can place a forest on either side of a limit by construction.
"""
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location(
    "forest_shapes", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "forest_shapes.py"))
_shapes = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_shapes)
SIDES, Picker = _shapes.SIDES, _shapes.Picker
complete, comb, chain, leafwise, banded = _shapes.complete, _shapes.comb, _shapes.chain, _shapes.leafwise, _shapes.banded
split_leftmost_leaf, stumps_with_thresholds, leaf_only = _shapes.split_leftmost_leaf, _shapes.stumps_with_thresholds, _shapes.leaf_only
_spine, set_spine = _shapes._spine, _shapes.set_spine


def reach_spine_end(X, tree, side):
    """How many rows of X walk the whole `side` spine (and so reach its last node's on-spine child)."""
    X = np.asarray(X, dtype=np.float32)
    rows = np.arange(X.shape[0])
    for fs, go_left in _spine(tree, side):
        fid = int(fs["fid"])
        x = X[rows, fid].astype(np.float64) if fid < X.shape[1] else np.zeros(len(rows))
        left = x <= np.float64(fs["split"])
        rows = rows[left] if go_left else rows[~left]
    return len(rows)


# ------------------------------------------------------------------------------------------- the restatement

def _leaf_values(X, tree):
    """The leaf every row of X reaches, as f64."""
    n, d = X.shape
    out = np.empty(n, dtype=np.float64)
    work = [(tree, np.arange(n))]
    while work:
        node, rows = work.pop()
        if "LeafNode" in node:
            out[rows] = np.float64(node["LeafNode"])
            continue
        fs = node["FeatureSplit"]
        fid = int(fs["fid"])
        x = X[rows, fid].astype(np.float64) if fid < d else np.zeros(len(rows), dtype=np.float64)
        left = x <= np.float64(fs["split"])  # NaN compares false: right
        work.append((fs["lhs"], rows[left]))
        work.append((fs["rhs"], rows[~left]))
    return out


def score(X, trees, weights=None):
    """Ensemble: trees = list, weights = one f64 per tree (zip stops at the shorter).  weights None: `trees` is one bare
    DecisionTree, whose score is the leaf itself."""
    X = np.asarray(X, dtype=np.float32)
    if weights is None:
        return _leaf_values(X, trees)
    acc = np.zeros(X.shape[0], dtype=np.float64)
    for tree, w in zip(trees, weights):
        prod = np.float64(w) * _leaf_values(X, tree)
        acc = acc + prod
    return acc


# ------------------------------------------------------------------------------------------- what the packers count

def floor_f32(split):
    """Largest f32 <= split (what a threshold becomes on the device: for every non-NaN f32 x, f64(x) <= split <=> x <= it)."""
    with np.errstate(over="ignore"):
        t = np.float32(split)
    if np.float64(t) > np.float64(split):
        t = np.nextafter(t, np.float32(-np.inf))
    return t


def distinct_thresholds(trees, fid):
    """Distinct thresholds of feature fid as the threshold-rank encoding counts them: floored to f32, -0.0 and +0.0 one."""
    seen = set()
    work = list(trees)
    while work:
        node = work.pop()
        if "LeafNode" in node:
            continue
        fs = node["FeatureSplit"]
        if int(fs["fid"]) == fid:
            t = floor_f32(fs["split"])
            if t == t:
                seen.add(np.float32(0.0).tobytes() if t == 0 else t.tobytes())
        work += [fs["lhs"], fs["rhs"]]
    return len(seen)


def features_used(trees, d):
    """Features below d that some inner node reads."""
    used = set()
    work = list(trees)
    while work:
        node = work.pop()
        if "FeatureSplit" in node:
            fs = node["FeatureSplit"]
            if int(fs["fid"]) < d:
                used.add(int(fs["fid"]))
            work += [fs["lhs"], fs["rhs"]]
    return used


def lds_layout(tree):
    """The breadth-first layout of the f32 LDS walk: (nodes, largest child offset, levels).  A node's children are adjacent
    and appended when the node is visited; the offset is the left child's index minus the node's own."""
    nodes, max_rel, levels = 1, 0, 0
    work = [(tree, 0, 0)]
    head = 0
    while head < len(work):
        node, dst, depth = work[head]
        head += 1
        levels = max(levels, depth)
        if "FeatureSplit" in node:
            fs = node["FeatureSplit"]
            max_rel = max(max_rel, nodes - dst)
            work.append((fs["lhs"], nodes, depth + 1))
            work.append((fs["rhs"], nodes + 1, depth + 1))
            nodes += 2
    return nodes, max_rel, levels


def rank_depth(tree):
    """Depth of the deepest leaf."""
    return lds_layout(tree)[2]
