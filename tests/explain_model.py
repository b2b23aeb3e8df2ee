"""Model explanation, restated twice, independently of the library.

1. `path_table` + `restate`: the algorithm as the device runs it -- the path table the host builds from the trees and the
   background's leaf counts, then EXTEND over the other elements for every element of every leaf path -- in numpy, vectorised
   over documents, the same IEEE operations in the same order.  The device's bytes must equal its bytes.
2. `brute`: the definition -- the Shapley sum over the subsets of F of the path-dependent coalition value -- by brute force,
   in floats (`exact=False`) or in exact rationals (`exact=True`: the f64 leaves and weights and the integer covers go in
   as they are).

Trees are the wire form: {"LeafNode": v} / {"FeatureSplit": {"fid", "split", "lhs", "rhs"}}.  A feature id >= X.shape[1]
reads 0.0; (double)x <= split goes left.
"""
import itertools
from fractions import Fraction
from math import factorial

import numpy as np

NO_FEATURE = 0xFFFFFFFF
MAX_PATH = 32


def is_leaf(node):
    return "LeafNode" in node


def column(X, fid):
    """(double)x[fid] for every row; a feature the matrix does not hold reads 0.0"""
    return X[:, fid].astype(np.float64) if fid < X.shape[1] else np.zeros(len(X))


def leaves_of(tree):
    if is_leaf(tree):
        return [tree]
    s = tree["FeatureSplit"]
    return leaves_of(s["lhs"]) + leaves_of(s["rhs"])


def route(tree, X):
    """the leaf (depth-first number) every row of X reaches"""
    out = np.zeros(len(X), dtype=np.int64)
    counter = [0]

    def walk(node, rows):
        if is_leaf(node):
            out[rows] = counter[0]
            counter[0] += 1
            return
        s = node["FeatureSplit"]
        left = column(X[rows], s["fid"]) <= np.float64(s["split"])
        walk(s["lhs"], rows[left])
        walk(s["rhs"], rows[~left])

    walk(tree, np.arange(len(X)))
    return out


def leaf_counts(trees, XB):
    """documents of the background at every leaf, depth first, tree after tree"""
    out = []
    for t in trees:
        out.extend(np.bincount(route(t, XB), minlength=len(leaves_of(t))).tolist())
    return [int(c) for c in out]


def predict(trees, weights, X, single=False):
    """f(x): the sum in tree order, product and sum rounded separately; a bare DecisionTree is its leaf"""
    acc = np.zeros(len(X))
    for t, w in zip(trees, weights):
        vals = np.array([leaf["LeafNode"] for leaf in leaves_of(t)], dtype=np.float64)[route(t, X)]
        acc = vals if single else acc + np.float64(w) * vals
    return acc


def model_features(trees):
    feats = set()

    def walk(node):
        if not is_leaf(node):
            feats.add(node["FeatureSplit"]["fid"])
            walk(node["FeatureSplit"]["lhs"])
            walk(node["FeatureSplit"]["rhs"])

    for t in trees:
        walk(t)
    return sorted(feats)


def split_counts(trees):
    counts = {}

    def walk(node):
        if not is_leaf(node):
            counts[node["FeatureSplit"]["fid"]] = counts.get(node["FeatureSplit"]["fid"], 0) + 1
            walk(node["FeatureSplit"]["lhs"])
            walk(node["FeatureSplit"]["rhs"])

    for t in trees:
        walk(t)
    return counts


# --- 1. the algorithm ---------------------------------------------------------------------------------------------------

def path_table(trees, weights, counts, d):
    """The table of csrc/explain.hpp (ExTables) and the bias.  counts: leaf_counts(); d: features of the explained matrix."""
    feats = model_features(trees)
    tab = dict(features=feats, leaf0=[0], feat0=[0], weight=[], m=[], eoff=[], value=[], slot=[], lo=[], hi=[], z=[], fid=[], col=[])
    bias = np.float64(0.0)
    next_leaf = [0]

    def cover(node, at):
        if is_leaf(node):
            at[0] += 1
            return counts[at[0] - 1]
        return cover(node["FeatureSplit"]["lhs"], at) + cover(node["FeatureSplit"]["rhs"], at)

    for tree, w in zip(trees, weights):
        tree_feats, path = [], []

        def node_value(node):
            if is_leaf(node):
                tab["m"].append(len(path))
                tab["eoff"].append(len(tab["slot"]))
                tab["value"].append(np.float64(node["LeafNode"]))
                for e in path:
                    tab["slot"].append(e[0]), tab["lo"].append(e[1]), tab["hi"].append(e[2]), tab["z"].append(e[3])
                next_leaf[0] += 1
                return np.float64(node["LeafNode"])
            s = node["FeatureSplit"]
            at = [next_leaf[0]]
            cl = cover(s["lhs"], at)
            cr = cover(s["rhs"], at)
            cp = cl + cr
            rl = np.float64(cl) / np.float64(cp) if cp else np.float64(0.0)
            rr = np.float64(cr) / np.float64(cp) if cp else np.float64(0.0)
            if s["fid"] not in tree_feats:
                tree_feats.append(s["fid"])
            slot = tree_feats.index(s["fid"])
            k = next((i for i, e in enumerate(path) if e[0] == slot), None)
            fresh = k is None
            if fresh:
                if len(path) >= MAX_PATH:
                    raise ValueError("a path with more than %d distinct features" % MAX_PATH)
                path.append((slot, -np.inf, np.inf, np.float64(1.0)))
                k = len(path) - 1
            saved = path[k]
            split = np.float64(s["split"])
            path[k] = (slot, saved[1], min(saved[2], split), saved[3] * rl)
            vl = node_value(s["lhs"])
            path[k] = (slot, max(saved[1], split), saved[2], saved[3] * rr)
            vr = node_value(s["rhs"])
            if fresh:
                path.pop()
            else:
                path[k] = saved
            a, b = rl * vl, rr * vr
            return a + b

        v = node_value(tree)
        bias = bias + np.float64(w) * v
        tab["weight"].append(np.float64(w))
        for f in tree_feats:
            tab["fid"].append(f if f < d else NO_FEATURE)
            tab["col"].append(feats.index(f))
        tab["leaf0"].append(next_leaf[0])
        tab["feat0"].append(len(tab["fid"]))
    tab["bias"] = bias
    tab["max_path"] = max(tab["m"]) if tab["m"] else 0
    tab["max_tree_feats"] = max((b - a for a, b in zip(tab["feat0"], tab["feat0"][1:])), default=0)
    return tab


def restate(tab, X):
    """phi[n, len(tab['features'])]: what explain_kernel computes, lane = row of X.  The leaves of a tree that have the same
    number of elements go through the same operations, so they are stacked ([leaves, rows] arrays: every entry sees the
    operations the kernel applies to it, in the kernel's order); the accumulation then goes leaf by leaf, depth first."""
    n = len(X)
    phi = np.zeros((n, len(tab["features"])))
    zero = np.zeros(n)
    for t in range(len(tab["weight"])):
        f0, f1 = tab["feat0"][t], tab["feat0"][t + 1]
        xs = [column(X, fid) if fid != NO_FEATURE else zero for fid in tab["fid"][f0:f1]]
        C = [np.zeros(n) for _ in range(f1 - f0)]
        leaves = range(tab["leaf0"][t], tab["leaf0"][t + 1])
        adds = {}
        for m in sorted(set(tab["m"][L] for L in leaves)):
            if m == 0:
                continue
            group = [L for L in leaves if tab["m"][L] == m]
            el = np.array([[tab["eoff"][L] + e for e in range(m)] for L in group])  # [g, m] element indices
            lo, hi, z = (np.asarray(tab[key], dtype=np.float64)[el][:, :, None] for key in ("lo", "hi", "z"))
            x = np.stack([np.stack([xs[tab["slot"][e]] for e in row]) for row in el])  # [g, m, n]
            o = ((lo < x) & (x <= hi)).astype(np.float64)
            leaf = np.asarray(tab["value"], dtype=np.float64)[group][:, None]
            for k in range(m):
                W = [np.ones((len(group), n))] + [None] * m
                l = 0
                for e in range(m):
                    if e == k:
                        continue
                    l += 1
                    carry = np.zeros((len(group), n))
                    for j in range(l - 1, -1, -1):
                        w = W[j]
                        W[j + 1] = carry + (o[:, e] * w) * (np.float64(j + 1) / np.float64(l + 1))
                        carry = (z[:, e] * w) * (np.float64(l - j) / np.float64(l + 1))
                    W[0] = carry
                s = np.zeros((len(group), n))
                for j in range(m):
                    s = s + W[j]
                add = (s * (o[:, k] - z[:, k])) * leaf
                for g, L in enumerate(group):
                    adds[(L, k)] = add[g]
        for L in leaves:
            for k in range(tab["m"][L]):
                slot = tab["slot"][tab["eoff"][L] + k]
                C[slot] = C[slot] + adds[(L, k)]
        for s in range(f1 - f0):
            col = tab["col"][f0 + s]
            phi[:, col] = phi[:, col] + tab["weight"][t] * C[s]
    return phi


def explain(trees, weights, X, XB=None):
    """(phi[n, |F|], features F, bias) by the restated algorithm, covers from XB (default X)"""
    tab = path_table(trees, weights, leaf_counts(trees, X if XB is None else XB), X.shape[1])
    return restate(tab, X), tab["features"], tab["bias"]


# --- 2. the definition ---------------------------------------------------------------------------------------------------

def brute(trees, weights, X, XB=None, exact=True):
    """(phi[n][|F|], F, bias) from the definition: Shapley weights over the subsets of F, coalition value by the walk.
    exact: Fractions throughout (objects), else floats."""
    XB = X if XB is None else XB
    feats = model_features(trees)
    nF = len(feats)
    num = Fraction if exact else float
    n = len(X)
    phi = [[num(0) for _ in feats] for _ in range(n)]
    bias = num(0)
    coef = [num(Fraction(factorial(s) * factorial(nF - s - 1), factorial(nF))) for s in range(nF)] if nF else []
    for tree, w in zip(trees, weights):
        w = num(w)

        # per node: fid, split, children, the background's cover ratios; rows of X that go left
        def annotate(node, rows_b):
            if is_leaf(node):
                return {"leaf": num(node["LeafNode"]), "cover": len(rows_b)}
            s = node["FeatureSplit"]
            left_b = column(XB[rows_b], s["fid"]) <= np.float64(s["split"])
            lhs, rhs = annotate(s["lhs"], rows_b[left_b]), annotate(s["rhs"], rows_b[~left_b])
            cp = lhs["cover"] + rhs["cover"]
            ratio = (lambda c: num(Fraction(c, cp)) if cp else num(0))
            return {"fid": s["fid"], "left": column(X, s["fid"]) <= np.float64(s["split"]), "lhs": lhs, "rhs": rhs, "cover": cp,
                    "rl": ratio(lhs["cover"]), "rr": ratio(rhs["cover"])}

        root = annotate(tree, np.arange(len(XB)))

        def value(node, S, i):
            if "leaf" in node:
                return node["leaf"]
            if node["fid"] in S:
                return value(node["lhs"] if node["left"][i] else node["rhs"], S, i)
            return node["rl"] * value(node["lhs"], S, i) + node["rr"] * value(node["rhs"], S, i)

        bias += w * value(root, frozenset(), 0) if n else num(0)
        for i in range(n):
            V = {}
            for r in range(nF + 1):
                for S in itertools.combinations(feats, r):
                    V[frozenset(S)] = value(root, frozenset(S), i)
            for fi, f in enumerate(feats):
                others = [g for g in feats if g != f]
                tot = num(0)
                for r in range(nF):
                    for S in itertools.combinations(others, r):
                        S = frozenset(S)
                        tot += coef[r] * (V[S | {f}] - V[S])
                phi[i][fi] += w * tot
    return phi, feats, bias


def exact_predict(trees, weights, X):
    """f(x) in rationals (sum of w_t * leaf)"""
    out = []
    for i in range(len(X)):
        s = Fraction(0)
        for t, w in zip(trees, weights):
            s += Fraction(w) * Fraction(leaves_of(t)[int(route(t, X[i:i + 1])[0])]["LeafNode"])
        out.append(s)
    return out


def scale(trees, weights):
    """sum over the trees of |w_t| * max |leaf_t|: what the error is measured against"""
    return float(sum(abs(float(w)) * max(abs(float(leaf["LeafNode"])) for leaf in leaves_of(t)) for t, w in zip(trees, weights)))


# --- the designed models (tests/test_explain_host.py, tests/test_gpu_explain.py) -------------------------------------------

def L(v):
    return {"LeafNode": float(v)}


def S(fid, split, lhs, rhs):
    return {"FeatureSplit": {"fid": int(fid), "split": float(split), "lhs": lhs, "rhs": rhs}}


def designed_cases():
    """[(name, trees, weights, X float32, XB float32 or None, single)]: `single` = a bare DecisionTree model"""
    rng = np.random.default_rng(2024)
    X = rng.normal(0, 1, (24, 4)).astype(np.float32)
    X[:, 1] = np.floor(rng.exponential(2.0, 24)).astype(np.float32)
    cases = []
    cases.append(("single_leaf", [L(2.5)], [1.0], X, None, True))
    cases.append(("stump", [S(0, 0.1, L(-1.0), L(3.0))], [1.0], X, None, True))
    # a feature repeated on a path: twice to the same side, and to opposite sides (an interval)
    rep = S(0, 0.5, S(0, -0.25, L(1.0), S(2, 0.0, L(2.0), L(-3.0))), S(0, 1.0, S(1, 1.0, L(4.0), L(0.5)), L(7.0)))
    cases.append(("repeated_feature", [rep, S(2, 0.3, S(2, -0.4, L(1.5), L(-0.5)), L(0.25))], [0.7, -1.3], X, None, False))
    # values equal to a split, and +-0.0 on both sides of the comparison
    Xe = X.copy()
    Xe[:8, 0] = np.float32(0.25)
    Xe[8:12, 2] = np.float32(-0.0)
    Xe[12:16, 2] = np.float32(0.0)
    eq = S(0, float(np.float32(0.25)), S(2, -0.0, L(1.0), L(2.0)), S(2, 0.0, L(-1.0), S(1, 2.0, L(5.0), L(-0.0))))
    cases.append(("equal_and_zero", [eq], [1.0], Xe, None, True))
    # a feature id beyond the dataset reads 0.0 everywhere: o = z = 1 on every path through it
    beyond = S(9, -1.0, L(100.0), S(1, 1.0, S(9, 0.0, L(2.0), L(50.0)), L(-2.0)))
    cases.append(("feature_beyond", [beyond, S(3, 0.0, L(1.0), L(-1.0))], [0.5, 2.0], X, None, False))
    # a background other than the explained rows: no background row has x0 > 0 or x3 > 1, explained rows do
    XB = X.copy()
    XB[:, 0] = -np.abs(XB[:, 0]) - np.float32(0.5)
    XB[:, 3] = np.minimum(XB[:, 3], np.float32(0.5))
    zc = S(0, 0.0, S(1, 1.0, L(1.0), L(2.0)), S(3, 1.0, S(1, 0.0, L(3.0), L(-4.0)), S(2, 0.0, L(6.0), L(8.0))))
    Xz = X.copy()
    Xz[:6, 0] = np.float32(1.5)
    Xz[:3, 3] = np.float32(2.0)
    cases.append(("zero_cover_background", [zc, S(3, 1.0, L(0.5), S(0, 0.0, L(1.0), L(9.0)))], [1.0, 0.25], Xz, XB, False))
    # tiny cover ratio: one background row in 40 goes right at the root
    Xt = rng.normal(0, 1, (40, 4)).astype(np.float32)
    Xt[:, 0] = -np.abs(Xt[:, 0])
    Xt[0, 0] = np.float32(3.0)
    tiny = S(0, 2.0, S(1, 0.0, L(1.0), L(-1.0)), S(1, 0.0, S(2, 0.0, L(10.0), L(20.0)), L(-30.0)))
    cases.append(("tiny_ratio", [tiny], [1.0], Xt, None, True))
    # non-uniform weights, a leaf among the trees, signs and magnitudes apart
    cases.append(("weights", [S(0, 0.0, L(1.0), L(2.0)), L(0.75), S(1, 1.0, S(0, 0.5, L(-1.0), L(1.0)), L(3.0)), S(2, 0.0, L(1e-3), L(-1e3))],
                  [0.1, -2.0, 3.5, 1e-2], X, None, False))
    return cases


def random_forest_model(seed, d=6, trees=3, depth=6, n=16, p_leaf=0.25):
    """seeded random trees of depth <= `depth` over d features with thresholds that are data values or near them"""
    rng = np.random.default_rng(seed)
    X = rng.normal(0, 1, (n, d)).astype(np.float32)
    X[:, 1] = np.floor(rng.exponential(1.5, n)).astype(np.float32)
    X[:, 2] = np.where(rng.random(n) < 0.6, 0.0, rng.random(n)).astype(np.float32)

    def grow(dd):
        if dd == 0 or (dd < depth and rng.random() < p_leaf):
            return L(rng.choice([rng.uniform(-2, 4), float(rng.integers(-3, 4))]))
        f = int(rng.integers(0, d))
        thr = float(X[rng.integers(0, n), f]) if rng.random() < 0.5 else float(rng.normal(0, 1))
        return S(f, thr, grow(dd - 1), grow(dd - 1))

    return [grow(depth) for _ in range(trees)], [float(w) for w in rng.uniform(-1.5, 1.5, trees)], X
