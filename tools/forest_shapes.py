"""Deterministic forest shapes: builders of trees in the reference's JSON shape ({"FeatureSplit": {"fid", "split", "lhs",
"rhs"}} | {"LeafNode": v}) -- complete trees, chains, combs, leaf-wise and banded trees, stumps.  A picker hands out the
(feature, threshold) of every inner node and the value of every leaf: anything with .rng (a numpy Generator), .node() and
.leaf(); `Picker` draws them from a seeded generator, so a shape built twice from the same seed is the same tree.
Used by tools/fuzz_trees.py and, through tests/tree_shapes.py, by the tree-scoring tests."""
import numpy as np

SIDES = ("left", "right", "zigzag")


class Picker:
    """Inner nodes draw a feature from `feats` and a threshold from `thresholds` (a sequence for every feature, or a dict
    fid -> sequence); leaves are distinct-looking values in (-4, 4), so that a walk that ends on the wrong leaf shows."""

    def __init__(self, seed, feats, thresholds):
        self.rng = np.random.default_rng(seed)
        self.feats = [int(f) for f in feats]
        self.thresholds = thresholds

    def node(self):
        f = self.feats[int(self.rng.integers(0, len(self.feats)))]
        pool = self.thresholds[f] if isinstance(self.thresholds, dict) else self.thresholds
        return f, float(pool[int(self.rng.integers(0, len(pool)))])

    def leaf(self):
        return {"LeafNode": float(self.rng.uniform(-4.0, 4.0))}


def _split(pick, lhs, rhs):
    f, s = pick.node()
    return {"FeatureSplit": {"fid": f, "split": s, "lhs": lhs, "rhs": rhs}}


def complete(depth, pick):
    """Every leaf `depth` levels deep: 2^depth leaves."""
    if depth == 0:
        return pick.leaf()
    return _split(pick, complete(depth - 1, pick), complete(depth - 1, pick))


def comb(depth, k, pick, side="left"):
    """A chain of `depth` inner nodes whose off-path child is a complete subtree of depth k (k = 0: a plain chain); the
    path continues on `side` ("zigzag" alternates, starting left).  The deepest leaf is depth + k levels deep."""
    assert side in SIDES
    t = pick.leaf()
    for level in range(depth - 1, -1, -1):  # built bottom-up; `level` is the node's depth
        off = complete(k, pick)
        go_left = side == "left" or (side == "zigzag" and level % 2 == 0)
        t = _split(pick, t, off) if go_left else _split(pick, off, t)
    return t


def chain(depth, side, pick):
    """`depth` inner nodes in a line, every off-path child a leaf; the last leaf is `depth` levels deep."""
    return comb(depth, 0, pick, side)


def leafwise(leaves, pick):
    """Split a random open leaf until the tree has `leaves` leaves: the shape a leaf budget (max_leaves) produces."""
    root = pick.leaf()
    open_leaves = [root]
    while len(open_leaves) < leaves:
        node = open_leaves.pop(int(pick.rng.integers(0, len(open_leaves))))
        lhs, rhs = pick.leaf(), pick.leaf()
        f, s = pick.node()
        node.clear()
        node["FeatureSplit"] = {"fid": f, "split": s, "lhs": lhs, "rhs": rhs}
        open_leaves += [lhs, rhs]
    return root


def banded(leaves, width, pick):
    """Level by level, the first `width` nodes of a level are split until the tree has `leaves` leaves: a deep tree of any
    size whose levels stay narrow (at most 2 * width nodes)."""
    root = pick.leaf()
    level, count = [root], 1
    while count < leaves:
        nxt = []
        for node in level[:width]:
            if count == leaves:
                break
            lhs, rhs = pick.leaf(), pick.leaf()
            f, s = pick.node()
            node.clear()
            node["FeatureSplit"] = {"fid": f, "split": s, "lhs": lhs, "rhs": rhs}
            nxt += [lhs, rhs]
            count += 1
        level = nxt
    return root


def split_leftmost_leaf(tree, pick):
    """The tree with its leftmost leaf turned into a stump (in place; returned for convenience).  On complete(d) this is the
    first node of level d, whose children land one whole level further on in a breadth-first layout."""
    node = tree
    while "FeatureSplit" in node:
        node = node["FeatureSplit"]["lhs"]
    lhs, rhs = pick.leaf(), pick.leaf()
    f, s = pick.node()
    node.clear()
    node["FeatureSplit"] = {"fid": f, "split": s, "lhs": lhs, "rhs": rhs}
    return tree


def _spine(tree, side):
    """The inner nodes met from the root by always stepping to `side` (zigzag: left on even levels), with the step taken."""
    out, node, level = [], tree, 0
    while "FeatureSplit" in node:
        go_left = side == "left" or (side == "zigzag" and level % 2 == 0)
        out.append((node["FeatureSplit"], go_left))
        node = node["FeatureSplit"]["lhs" if go_left else "rhs"]
        level += 1
    return out


def set_spine(tree, side, fid, values):
    """Rewrites the splits along the tree's `side` spine so that documents peel off it a few per level and many walk it to
    its end (random splits would leave the deep end of a chain, the last nodes of a wide level, unvisited): every spine node
    reads feature fid; a left step keeps x <= hi, a right step keeps x > lo, with hi coming down and lo going up through the
    ascending `values` towards their middle.  In place; returns the tree."""
    spine = _spine(tree, side)
    values = sorted(float(v) for v in values)
    assert len(values) >= 2 * len(spine) + 2
    step = (len(values) // 2 - 1) / max(len(spine), 1)  # the two bounds never meet: half the values stay between them
    lo, hi = 0.0, float(len(values) - 1)
    for fs, go_left in spine:
        fs["fid"] = int(fid)
        if go_left:
            fs["split"] = values[int(hi)]
            hi -= step
        else:
            fs["split"] = values[int(lo)]
            lo += step
    return tree


def stumps_with_thresholds(fid, values, pick):
    """One stump per value: fid <= value ? leaf : leaf."""
    return [{"FeatureSplit": {"fid": int(fid), "split": float(v), "lhs": pick.leaf(), "rhs": pick.leaf()}} for v in values]


def leaf_only(pick):
    return pick.leaf()
