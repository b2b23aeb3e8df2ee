"""numpy restatement of LambdaMART's DART boosting ("DART"), for the tests.

The definition, restated.  The state before tree t (0-based) is the trees m_0 .. m_{t-1} with f64 weights w_0 .. w_{t-1}.
  * Drop plan: a generator of its own, Rand64(seed XOR 0x4441525444415254), read with rand_float() = (u >> 10) * 2^-54
    only.  Tree 0 draws nothing and drops nothing.  Tree t >= 1 draws exactly 1 + t floats: u, then c_0 .. c_{t-1}.
    u < skip_drop: D_t is empty.  Otherwise D_t = {i : c_i < drop_rate}, cut to its max_drop smallest indices when
    max_drop > 0.  An empty D_t is an ordinary boosting step.  k = |D_t|.
  * The tree is fitted to S(w, skip D_t): s = +0.0; for i ascending, i not in D_t: s = s + w_i * m_i(x), product and sum
    rounded separately.
  * Re-weighting: w_t = learning_rate / float(k + 1); for i in D_t: w_i = w_i * f, f = float(k) / float(k + 1).
  * The running scores after the tree are S(w', skip nothing) over all t + 1 trees.
This module holds no tree fitting: trees come from the other restatements, called with the device's gradients of the
dropped model.  The generator and the tree scoring are the oracle's (oracle.pyoracle).
"""
import numpy as np

from oracle import pyoracle as o

DART_STREAM = 0x4441525444415254


def rand_floats(seed, n):
    """The first n rand_float() values of the drop generator of `seed`."""
    u = o.rand64_stream((int(seed) ^ DART_STREAM) & (2 ** 64 - 1), n)
    return (u >> np.uint64(10)).astype(np.float64) * 2.0 ** -54


def plan(seed, drop_rate, max_drop, skip_drop, T, lr):
    """Per tree t < T: (D_t as an ascending list, the weights before the tree [t], the weights after it [t + 1])."""
    draws = rand_floats(seed, sum(1 + t for t in range(1, T)))
    at, w, out = 0, np.zeros(0, dtype=np.float64), []
    for t in range(T):
        dropped = []
        if t >= 1:
            u, c = draws[at], draws[at + 1:at + 1 + t]
            at += 1 + t
            if not u < skip_drop:
                dropped = [int(i) for i in np.flatnonzero(c < drop_rate)]
                if max_drop > 0:
                    dropped = dropped[:max_drop]
        k = len(dropped)
        before = w.copy()
        w = w.copy()
        f = np.float64(k) / np.float64(k + 1)
        for i in dropped:
            w[i] = w[i] * f
        w = np.append(w, np.float64(lr) / np.float64(k + 1))
        out.append((dropped, before, w.copy()))
    return out


def kept(t, dropped):
    """The trees 0 .. t-1 without `dropped`, ascending."""
    gone = set(dropped)
    return [i for i in range(t) if i not in gone]


def numbered(tree):
    """(a copy of the tree whose leaves hold 0, 1, 2, ... in depth-first order, lhs before rhs; the leaves' values in that order)"""
    values = []

    def copy(node):
        if "LeafNode" in node:
            values.append(float(node["LeafNode"]))
            return {"LeafNode": float(len(values) - 1)}
        fs = node["FeatureSplit"]
        lhs = copy(fs["lhs"])
        return {"FeatureSplit": {"fid": fs["fid"], "split": fs["split"], "lhs": lhs, "rhs": copy(fs["rhs"])}}

    return copy(tree), np.asarray(values, dtype=np.float64)


def leaf_numbers(tree, c):
    """(the leaf every row of the oracle dataset `c` reaches, by the oracle's tree scoring: 0.0 + 1.0 * index is exact;
    the leaves' values)"""
    routing, values = numbered(tree)
    idx = c.score_ensemble([routing], [1.0])
    assert np.all(idx == np.floor(idx)) and np.all(idx >= 0) and np.all(idx < len(values))
    return idx.astype(np.int64), values


def scores(trees, weights, include, c):
    """S(weights, only the trees `include`, ascending) for every row of the oracle dataset `c`: the sequential recurrence,
    product and sum rounded separately."""
    s = np.zeros(c.n, dtype=np.float64)
    for i in include:
        idx, values = leaf_numbers(trees[i], c)
        prod = np.float64(weights[i]) * values[idx]
        s = s + prod
    return s
