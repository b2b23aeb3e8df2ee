"""A numpy restatement of the random-forest trainer's level step (csrc/rf_train.hpp, kernels_rf.inc),
written from the design, the oracle and the kernels' comments: what native.rf_levels must return, field by field and bit by bit.
tests/test_rf_level_host.py anchors it to the oracle's trees; tests/test_gpu_rf_levels.py holds the device to it.

One level, for every open node (tree, key, its instances as indices r into the tree's instance list) and feature slot:
  * sorted arrays: the node's instances by (feature value with -0.0 folded onto +0.0, r) -- a stable argsort of the r-ascending
    list; svals = r, sg = the f32 target, sv = the folded value, or -0.0 where the instance does not hold the feature (it
    sorts as 0.0);
  * range: min / max over the held values, starting from f64::MAX / f64::MIN and compared with > and < (a column of nothing but
    +inf keeps f64::MAX); fewer than two held values, or fewer than two instances: no candidate, an all-zero record;
  * candidate c = 1..k-1: position = (c / k) * range + min in f64, ids_i = searchsorted(values, position, 'left'); evaluated
    (flags bit 0) when ids_i differs from candidate c-1's and both sides hold at least min_leaf_support instances;
  * an evaluated candidate's numbers -- SquaredError: sum_l / sum_r sequential from 0.0, the means, the two squared-error sums
    sequential from 0.0, importance = -(el + er); TrueVarianceReduction: Welford per side, NaN below two labels; Gini /
    entropy: the positive counts (importance stays 0.0 in the record; the host finishes it with libm's log2).  Every other
    field of a candidate that is not evaluated is zero.
Selection: last maximum per feature, then over features.  Children: the chosen segment's sorted order cut at ids_i; their
outputs are sequential sums in that order over their sizes (0.0 for an empty side); keys are handed out in node order."""
import math

import numpy as np

CAND_DTYPE = np.dtype([("position", "<f8"), ("importance", "<f8"), ("ids_i", "<u4"), ("flags", "<u4"), ("pos_l", "<u4"), ("pos_r", "<u4"),
                       ("sum_l", "<f8"), ("sum_r", "<f8")])
ACTIVE_DTYPE = np.dtype([("tree", "<u4"), ("key", "<u4"), ("n", "<u4")])
SPLIT_DTYPE = np.dtype([("fslot", "<i4"), ("pos", "<u4"), ("left", "<u4"), ("right", "<u4")])
F64_MAX = 1.7976931348623157e308


class ReferencePanic(Exception):
    """Where the reference panics (a NaN importance: the variance of fewer than two labels)."""


def seq_sum(a):
    """0.0 + a[0] + a[1] + ... added one after the other."""
    return float(np.cumsum(np.concatenate(([0.0], np.asarray(a, dtype=np.float64))))[-1])


def welford_variance(a):
    """stats.rs:66-104; None below two elements."""
    mean, s = 0.0, 0.0
    for i, x in enumerate(a.tolist()):
        if i == 0:
            mean = x
            continue
        old = mean
        mean = old + (x - old) / float(i + 1)
        s = s + (x - old) * (x - mean)
    return None if len(a) <= 1 else s / float(len(a) - 1)


def gini(n, positive):
    if n == 0:
        return 0.0
    count, pos = float(n), float(positive)
    p_yes, p_no = pos / count, (count - pos) / count
    return p_yes * (1.0 - p_yes) + p_no * (1.0 - p_no)


def _plogp(x):
    return 0.0 if x == 0.0 else x * math.log2(x)


def entropy(n, positive):
    if n == 0:
        return 0.0
    count, pos = float(n), float(positive)
    return -_plogp(pos / count) - _plogp((count - pos) / count)


def enterable(n, depth, min_leaf, max_depth):
    return n != 0 and depth < max_depth and n >= min_leaf and n > 1


def sorted_segment(X, present, ids, rs, f, stable=True):
    """(svals, sv, sg-order) of one node and feature: rs ascending, ids = the tree's instance list."""
    rows = ids[rs]
    col = X[rows, f].astype(np.float32)
    held = np.ones(len(rs), dtype=bool) if present is None else present[rows, f].astype(bool)
    col = np.where(held, col, np.float32(0.0))       # an absent value reads 0.0
    col = np.where(col == 0, np.float32(0.0), col)    # -0.0 and +0.0 are one key
    # (stable=False, the tests' mutation check: equal values in descending r, what an unstable sort may leave)
    order = np.argsort(col, kind="stable") if stable else np.lexsort((-np.arange(len(col)), col))
    sv = col[order].astype(np.float32)
    sv[~held[order]] = np.float32(-0.0)
    return rs[order], sv, held[order]


def candidates(sv, held, g, k, method, min_leaf, side="left", tail_first=False):
    """The k-1 candidate records of one sorted segment (sv f32 with -0.0 for absent, g the f32 targets in sorted order) and the
    host's importances (None where not evaluated).  side / tail_first exist for the tests' mutation check only."""
    n = len(sv)
    out = np.zeros(max(k - 1, 0), dtype=CAND_DTYPE)
    imps = [None] * max(k - 1, 0)
    hv = sv[held].astype(np.float64)
    if n <= 1 or len(hv) <= 1 or k < 2:
        return out, imps
    fmin, fmax = F64_MAX, -F64_MAX
    if hv.min() < fmin:
        fmin = float(hv.min())
    if hv.max() > fmax:
        fmax = float(hv.max())
    rng = fmax - fmin
    v64 = sv.astype(np.float64)
    g64 = g.astype(np.float64)
    prev = None
    for c in range(1, k):
        position = (float(c) / float(k)) * rng + fmin
        ids_i = int(np.searchsorted(v64, position, side))
        rec = out[c - 1]
        rec["position"], rec["ids_i"] = position, ids_i
        fresh = prev is None or prev != ids_i
        prev = ids_i
        nl, nr = ids_i, n - ids_i
        if not (fresh and nl >= min_leaf and nr >= min_leaf):
            continue
        rec["flags"] = 1
        gl, gr = g64[:nl], g64[nl:]
        if method == 0:
            sl, sr = seq_sum(gl), seq_sum(gr)
            ml, mr = (sl / float(nl) if nl else 0.0), (sr / float(nr) if nr else 0.0)

            def sq(mean, x):
                t = (mean - x) * (mean - x)
                if tail_first and len(t) % 16:
                    cut = len(t) - len(t) % 16
                    t = np.concatenate((t[cut:], t[:cut]))
                return seq_sum(t)
            rec["sum_l"], rec["sum_r"] = sl, sr
            rec["importance"] = -(sq(ml, gl) + sq(mr, gr))
            imps[c - 1] = float(rec["importance"])
        elif method == 3:
            vl, vr = welford_variance(gl), welford_variance(gr)
            rec["importance"] = float("nan") if vl is None or vr is None else -(vl * float(nl) + vr * float(nr))
            imps[c - 1] = float(rec["importance"])
        else:
            pl, pr = int((g[:nl] > 0).sum()), int((g[nl:] > 0).sum())
            rec["pos_l"], rec["pos_r"] = pl, pr
            fn = gini if method == 1 else entropy
            imps[c - 1] = -(fn(nl, pl) * float(nl) + fn(nr, pr) * float(nr))
    return out, imps


def _leaf(value=0.0):
    return {"leaf": True, "value": value}


def _json(node):
    if node["leaf"]:
        return {"LeafNode": float(node["value"])}
    return {"FeatureSplit": {"fid": int(node["fid"]), "split": float(node["split"]), "lhs": _json(node["lhs"]), "rhs": _json(node["rhs"])}}


def grow(X, present, y, roots, feats, k, method, min_leaf, max_depth, stable=True, side="left", tail_first=False):
    """One batch of trees.  X [n, d] f32, present [n, d] bool or None, y the targets (taken as f32), roots: per tree the instance
    ids in list order, feats [T][nf].  Returns the record native.rf_levels returns (children_from left out)."""
    X = np.asarray(X, dtype=np.float32)
    y = np.asarray(y, dtype=np.float32)
    roots = [np.asarray(r, dtype=np.int64) for r in roots]
    feats = np.asarray(feats, dtype=np.int64).reshape(len(roots), -1)
    T, nf = feats.shape
    tree_nodes = [_leaf() for _ in range(T)]
    open_nodes = []
    for t in range(T):
        if enterable(len(roots[t]), 1, min_leaf, max_depth):
            open_nodes.append((t, t, np.arange(len(roots[t]), dtype=np.int64), tree_nodes[t], 1))
    next_key = T
    levels = []
    if k < 2:
        open_nodes = []
    while open_nodes:
        A = len(open_nodes)
        lv = {"active": np.zeros(A, dtype=ACTIVE_DTYPE), "depth": np.zeros(A, dtype=np.uint32), "label_minmax": np.zeros((A, 2), dtype=np.float32),
              "cands": np.zeros((A, nf, k - 1), dtype=CAND_DTYPE), "splits": np.zeros(A, dtype=SPLIT_DTYPE),
              "child_out": np.zeros((A, 2), dtype=np.float64)}
        svals, svs, sgs = [], [], []
        nxt = []
        for a, (t, key, rs, node, depth) in enumerate(open_nodes):
            n = len(rs)
            lv["active"][a] = (t, key, n)
            lv["depth"][a] = depth
            labels = y[roots[t][rs]]
            lv["label_minmax"][a] = (labels.min(), labels.max())
            lv["splits"][a] = (-1, 0, 0, 0)
            segs = []
            for fi in range(nf):
                order, sv, held = sorted_segment(X, present, roots[t], rs, int(feats[t, fi]), stable)
                g = y[roots[t][order]]
                svals.append(order), svs.append(sv), sgs.append(g)
                cd, imps = candidates(sv, held, g, k, method, min_leaf, side, tail_first)
                lv["cands"][a, fi] = cd
                segs.append((order, g, cd, imps))
            if labels.min() == labels.max():
                continue
            best = None  # (importance, fi, candidate)
            for fi, (order, g, cd, imps) in enumerate(segs):
                fbest = None
                for c, imp in enumerate(imps):
                    if imp is None:
                        continue
                    if imp != imp:
                        raise ReferencePanic("NaN importance")
                    if fbest is None or imp >= fbest[0]:
                        fbest = (imp, fi, c)
                if fbest is not None and (best is None or fbest[0] >= best[0]):
                    best = fbest
            if best is None:
                continue
            _, fi, c = best
            order, g, cd, _ = segs[fi]
            pos = int(cd[c]["ids_i"])
            lv["splits"][a] = (fi, pos, next_key, next_key + 1)
            node["leaf"], node["fid"], node["split"] = False, int(feats[t, fi]), float(cd[c]["position"])
            kids = []
            for s, (part, gp) in enumerate(((order[:pos], g[:pos]), (order[pos:], g[pos:]))):
                out = seq_sum(gp) / float(len(gp)) if len(gp) else 0.0
                lv["child_out"][a, s] = out
                kid = _leaf(out)
                kids.append(kid)
                if enterable(len(part), depth + 1, min_leaf, max_depth):
                    nxt.append((t, next_key + s, np.sort(part), kid, depth + 1))
            node["lhs"], node["rhs"] = kids
            next_key += 2
        lv["svals"] = np.concatenate(svals).astype(np.uint32)
        lv["sv"] = np.concatenate(svs).astype(np.float32)
        lv["sg"] = np.concatenate(sgs).astype(np.float32)
        levels.append(lv)
        open_nodes = nxt
    root_out = np.zeros(0)
    if any(nd["leaf"] for nd in tree_nodes):
        root_out = np.array([seq_sum(y[roots[t]]) / float(len(roots[t])) if len(roots[t]) else 0.0 for t in range(T)])
        for t in range(T):
            if tree_nodes[t]["leaf"]:
                tree_nodes[t]["value"] = root_out[t]
    return {"levels": levels, "root_out": root_out, "trees": [_json(nd) for nd in tree_nodes]}


def same_bits(a, b):
    """Equality of every byte of two arrays of one dtype and shape (structured records included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def diff(got, want):
    """The first difference between two records as a string, or None.  Every array by its bytes, except label_minmax, whose
    sign of zero fminf / fmaxf leave open: by value."""
    if len(got["levels"]) != len(want["levels"]):
        return "levels: %d != %d" % (len(got["levels"]), len(want["levels"]))
    for i, (g, w) in enumerate(zip(got["levels"], want["levels"])):
        for name in ("active", "depth", "cands", "svals", "sv", "sg", "splits", "child_out"):
            if not same_bits(g[name], w[name]):
                where = ""
                if g[name].shape == w[name].shape:
                    bad = np.nonzero(np.asarray(g[name]).reshape(-1) != np.asarray(w[name]).reshape(-1))[0][:3]
                    where = " at %s: %s != %s" % (bad.tolist(), np.asarray(g[name]).reshape(-1)[bad], np.asarray(w[name]).reshape(-1)[bad])
                return "level %d: %s%s" % (i, name, where)
        if g["label_minmax"].shape != w["label_minmax"].shape or not (g["label_minmax"] == w["label_minmax"]).all():
            return "level %d: label_minmax" % i
    if not same_bits(np.asarray(got["root_out"], dtype=np.float64), np.asarray(want["root_out"], dtype=np.float64)):
        return "root_out"
    if got["trees"] != want["trees"]:
        return "trees"
    return None
