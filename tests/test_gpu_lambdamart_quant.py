"""LambdaMART's quantised gradients on the device (kernels_histquant.inc; DESIGN.md section 11, "Quantised gradients")
against the numpy restatement (tests/lambdamart_quant_model.py), bit for bit.

Values: native.hist_quantise gives the restatement's (q, w), exponents and shifts.  Build kernel: native.hist_root_histogram
is np.add.at of the restatement's values over the restatement's bins.  One tree: native.hist_tree(quant=...) is the
restatement's tree -- the Newton / leaf-wise / symmetric shape over the quantised values, the leaves renewed from the
full-precision sums.  Training: every tree equals that fit to the DEVICE's gradients of the ensemble the tree is fitted to,
under the tree's key; scores, prediction and measures are the oracle's.
"""
import json
import os

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import native
from oracle import pyoracle as o
from tests import lambdamart_composed_model as cmod
from tests import lambdamart_dart_model as dm
from tests import lambdamart_goss_model as gm
from tests import lambdamart_hist_model as hm
from tests import lambdamart_model as lm
from tests import lambdamart_newton_model as nm
from tests import lambdamart_quant_model as qm
from tests import lambdamart_sample_model as sm
from tests import lambdamart_xendcg_model as xm
from tests.conftest import GOLDEN, synth_dataset

pytestmark = pytest.mark.gpu

EMPTY = {"Ensemble": {"weights": [], "models": []}}
QUANT_STATS = {"grad_quant_bits", "quant_ms"}
CHUNK = 8192  # HIST_CHUNK: the entries of the index list one workgroup of the build kernel adds up


# --- values --------------------------------------------------------------------------------------

class Listed:
    """A dataset of n documents in queries of at most 40 with F features of at most `distinct` values each, and its lists."""

    def __init__(self, n, F=2, distinct=0, seed=0):
        rng = np.random.default_rng(1000 + n + 31 * F + seed)
        qid = (np.arange(n) // 40 + 1).astype(np.int64)
        X = rng.random((n, F)).astype(np.float32)
        self.X = np.floor(X * distinct).astype(np.float32) if distinct else X
        self.y = rng.integers(0, 3, n).astype(np.float64)
        self.qid, self.n, self.F = qid, n, F
        self.g, self.c = fr.CDataset.from_numpy(self.X, self.y, qid), o.Dataset(self.X, self.y, qid)
        self.queries = lm.query_lists(self.c)
        self.order_ids = np.concatenate(self.queries)


_listed = {}


def listed(n, F=2, distinct=0):
    if (n, F, distinct) not in _listed:
        _listed[(n, F, distinct)] = Listed(n, F, distinct)
    return _listed[(n, F, distinct)]


def _gradients(n, seed):
    rng = np.random.default_rng(seed)
    lam = rng.standard_normal(n) * np.exp(rng.standard_normal(n))
    lam[rng.random(n) < 0.3] = 0.0
    return lam, rng.random(n) * np.abs(lam) + 1e-3


def _expected_values(lam, wt, ids, bits, key):
    """The restatement's dict for the list whose entries have the original instance ids `ids` (lam / wt by instance id)."""
    n = len(ids)
    Q, S, W, Sw = nm.quantise_pair(np.asarray(lam, dtype=np.float64)[ids], np.asarray(wt, dtype=np.float64)[ids], n)
    q, w, d, dw = qm.quantise(Q, W, ids, bits, key)
    return dict(q=q, w=w, s_l=S, s_w=Sw, search_s_l=S - d, search_s_w=Sw - dw, d=d, d_w=dw), Q, W


def _same_values(got, exp):
    for k in ("s_l", "s_w", "search_s_l", "search_s_w", "d", "d_w"):
        assert got[k] == exp[k], (k, got[k], exp[k])
    assert len(got["q"]) == len(exp["q"])
    assert np.array_equal(got["q"], exp["q"]), "q differs at %s" % np.flatnonzero(got["q"] != exp["q"])[:5]
    assert np.array_equal(got["w"], exp["w"]), "w differs at %s" % np.flatnonzero(got["w"] != exp["w"])[:5]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 8193, 60000])
def test_values_are_the_restatements(n):
    ds = listed(n)
    lam, wt = _gradients(n, n)
    lam[0] = 1.5  # (never all zero)
    for bits in (2, 4, 8):
        key = qm.keys(5 + bits, 3)[2]
        exp, _, _ = _expected_values(lam, wt, ds.order_ids, bits, key)
        got = native.hist_quantise(ds.g, lam, wt, bits, 5 + bits, 2)
        _same_values(got, exp)
        assert np.abs(got["q"]).max() <= 2 ** (bits - 1) and got["w"].min() >= 0 and got["w"].max() <= 2 ** bits
        assert (got["d"], got["d_w"]) == (62 - n.bit_length() - bits, 61 - n.bit_length() - bits)


@pytest.mark.parametrize("n", [65, 8193])
def test_values_of_designed_gradients(n):
    ds = listed(n)
    i = np.arange(n)
    sign = np.where(i % 2 == 0, 1.0, -1.0)
    below_one = 1.0 - 2.0 ** -53
    designed = {
        "powers of two": (np.ldexp(sign, -(i % 40).astype(np.int64)), np.ldexp(1.0, -(i % 37).astype(np.int64))),
        "just below powers of two": (below_one * np.ldexp(sign, (i % 9).astype(np.int64) - 8), below_one * np.ldexp(1.0, (i % 7).astype(np.int64) - 6)),
        "zeros among them": (np.where(i % 3 == 0, 0.0, sign * 0.75), np.where(i % 4 == 0, 0.0, 0.5)),
        "all w zero": (sign * (1.0 + (i % 5)), np.zeros(n)),
        "every entry at the extreme": (np.full(n, -below_one * 4.0), np.full(n, below_one * 0.125)),
    }
    for name, (lam, wt) in designed.items():
        for bits in (2, 4, 8):
            exp, Q, W = _expected_values(lam, wt, ds.order_ids, bits, qm.keys(9, 1)[0])
            try:
                _same_values(native.hist_quantise(ds.g, lam, wt, bits, 9, 0), exp)
            except AssertionError as e:
                raise AssertionError("%s, %d bits: %s" % (name, bits, e))
            if name == "all w zero":
                assert exp["s_w"] == 0 and not exp["w"].any()
            if name == "every entry at the extreme" and n >= 512:  # (61 - c < 53: the fixed-point step rounds (1 - 2^-53) m up to 2^(61 - c))
                assert np.all(exp["q"] == -2 ** (bits - 1)) and np.all(exp["w"] == 2 ** bits)
            if name == "powers of two":  # exactly representable: q = Q >> d wherever Q is a multiple of 2^d
                mult = (Q & ((1 << exp["d"]) - 1)) == 0
                assert mult.any() and np.array_equal(exp["q"][mult], Q[mult] >> exp["d"])


def test_values_over_a_query_sample_a_view_and_goss():
    n = 2500
    ds = listed(n)
    lam, wt = _gradients(n, 3)
    nq = len(ds.queries)
    names = cmod._names(ds.qid)
    key = qm.keys(21, 2)[1]
    # a query sample: the list is the sample's, c its length's
    for qsel in (np.arange(0, nq, 2), np.array([nq - 1]), np.arange(3, nq - 4)):
        ids = ds.order_ids[sm.instance_rows(ds.queries, qsel)]
        _same_values(native.hist_quantise(ds.g, lam, wt, 4, 21, 1, queries=qsel), _expected_values(lam, wt, ids, 4, key)[0])
    # a sampled view: the offsets are those of the parent's instance ids
    pick = names[1::3]
    view = ds.g.subsample_queries(pick)
    qsel = np.asarray([names.index(x) for x in pick])
    v_ids = np.concatenate([ds.queries[q] for q in qsel])
    got_view = native.hist_quantise(view, lam, wt, 4, 21, 1)
    _same_values(got_view, _expected_values(lam, wt, v_ids, 4, key)[0])
    got_parent = native.hist_quantise(ds.g, lam, wt, 4, 21, 1, queries=qsel)
    assert np.array_equal(got_view["q"], got_parent["q"]) and np.array_equal(got_view["w"], got_parent["w"])
    renumbered = _expected_values(lam[v_ids], wt[v_ids], np.arange(len(v_ids)), 4, key)[0]
    assert not np.array_equal(renumbered["q"], got_view["q"])  # (ids of the view's own would have given other bits)
    # GOSS: the list is the GOSS list, the values the amplified ones
    for a, b in ((0.2, 0.1), (0.5, 0.5)):
        rows, top, _, amp = gm.goss_list(lam, np.arange(n), ds.order_ids, a, b, gm.keys(8, 4)[3])
        lam2, wt2 = gm.amplified(lam, wt, ds.order_ids, rows, top, amp)
        got = native.hist_quantise(ds.g, lam, wt, 3, 21, 1, goss=(a, b, 8, 3))
        _same_values(got, _expected_values(lam2, wt2, ds.order_ids[rows], 3, key)[0])
        assert len(got["q"]) == len(rows) and (len(rows) < n or a + b == 1.0)
    # twice the same, another tree or seed not
    first = native.hist_quantise(ds.g, lam, wt, 4, 21, 1)
    again = native.hist_quantise(ds.g, lam, wt, 4, 21, 1)
    assert first["q"].tobytes() == again["q"].tobytes() and first["w"].tobytes() == again["w"].tobytes()
    assert first["q"].tobytes() != native.hist_quantise(ds.g, lam, wt, 4, 21, 2)["q"].tobytes()
    assert first["q"].tobytes() != native.hist_quantise(ds.g, lam, wt, 4, 22, 1)["q"].tobytes()


# --- the build kernel ----------------------------------------------------------------------------

def _expected_histogram(ds, lam, wt, k, quant, fsel=None):
    feats = list(range(ds.F))
    edges, xbin = hm.bin_matrix(ds.X, ds.order_ids, feats, k)
    Q, S, W, Sw = nm.quantise_pair(lam[ds.order_ids], wt[ds.order_ids], ds.n)
    if quant is not None:
        Q, W, _, _ = qm.quantise(Q, W, ds.order_ids, quant[0], qm.keys(quant[1], quant[2] + 1)[quant[2]])
    slots = feats if fsel is None else sorted(fsel)
    cnt, qs, ws = (np.zeros((len(slots), k), dtype=np.int64) for _ in range(3))
    for u, s in enumerate(slots):
        np.add.at(cnt[u], xbin[s], 1)
        np.add.at(qs[u], xbin[s], Q)
        np.add.at(ws[u], xbin[s], W)
    return cnt, qs, ws


def _same_histogram(ds, lam, wt, k, quant, fsel=None):
    exp = _expected_histogram(ds, lam, wt, k, quant, fsel)
    got = native.hist_root_histogram(ds.g, lam, wt, k, quant=quant, features=fsel)
    for name, g_, e_ in zip(("count", "sum q", "sum w"), got, exp):
        assert g_.shape == e_.shape and np.array_equal(g_, e_), "%s differs in %d cells" % (name, int((g_ != e_).sum()))
    assert int(got[0].sum()) == ds.n * got[0].shape[0]
    return got


@pytest.mark.parametrize("n", [1, 255, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
def test_build_over_the_piece_boundaries(n):
    ds = listed(n, 9, 64)  # (nine features: one full block and one more under eight features per workgroup)
    lam, wt = _gradients(n, n + 1)
    lam[0] = -2.0
    for bits in (2, 8):
        _same_histogram(ds, lam, wt, 64, (bits, 3, 1))
    _same_histogram(ds, lam, wt, 64, None)  # (the Newton build, by the same hook)


@pytest.mark.parametrize("F", [7, 8, 9, 15, 16, 17, 33])
def test_build_over_the_feature_blocks(F):
    """One below, at and one above 8 and 16 features per workgroup (the two block sizes that were measured), and two blocks
    plus one."""
    ds = listed(CHUNK + 1, F, 256)
    lam, wt = _gradients(ds.n, F)
    lam[0] = 3.0
    _same_histogram(ds, lam, wt, 256, (4, 1, 0))


@pytest.mark.parametrize("k", [2, 64, 256])
def test_build_over_the_bin_counts_and_a_feature_sample(k):
    ds = listed(3000, 17, k)
    lam, wt = _gradients(ds.n, k)
    lam[0] = 1.0
    got = _same_histogram(ds, lam, wt, k, (4, 2, 2))
    assert int((got[0] > 0).sum(axis=1).max()) == k  # (every bin of some feature is in use)
    for fsel in ([0], [1, 2, 5, 8, 11, 12, 13, 16], [0, 1, 2, 3, 4, 5, 6, 7, 9], list(range(17))):
        sub = _same_histogram(ds, lam, wt, k, (4, 2, 2), fsel)  # (the SEL instance)
        assert np.array_equal(sub[1], got[1][fsel])


def test_build_at_the_limit_of_the_packed_cell():
    """Eight bits, every entry in one bin with q = -2^7 and w = 2^8: the first piece adds 8 192 of them into one cell."""
    n = CHUNK + 1
    ds = listed(n, 3, 1)  # (one distinct value per feature: one bin)
    m, below_one = 4.0, 1.0 - 2.0 ** -53  # (just below a power of two: the fixed-point step rounds it up to 2^(61 - c), 61 - c = 47 < 53)
    lam, wt = np.full(n, -below_one * m), np.full(n, below_one * 0.5)
    got = _same_histogram(ds, lam, wt, 4, (8, 1, 0))
    assert np.all(got[0][:, 0] == n) and np.all(got[1][:, 0] == -128 * n) and np.all(got[2][:, 0] == 256 * n)
    lam[::2] = -lam[::2]  # (and both extremes mixed)
    got = _same_histogram(ds, lam, wt, 4, (8, 1, 0))
    assert np.all(got[1][:, 0] == 128)


def test_both_builds_agree_on_exactly_representable_inputs():
    """Gradients whose fixed-point values are multiples of 2^d: every q is Q >> d whatever the key, so the packed build's sums
    shifted back are the Newton build's."""
    n, bits = 5000, 6
    ds = listed(n, 9, 64)
    rng = np.random.default_rng(12)
    # the largest |lambda| = 1.0 = 0.5 2^1 becomes 2^(60 - c), so a multiple of 2^-4 becomes one of 2^(56 - c) = 2^d; w likewise with d_w
    lam = rng.integers(-16, 17, n) / 16.0
    lam[0] = 1.0
    wt = rng.integers(0, 33, n) / 32.0
    wt[1] = 1.0
    d, dw = qm.shifts(n, bits)
    packed = native.hist_root_histogram(ds.g, lam, wt, 64, quant=(bits, 4, 0))
    plain = native.hist_root_histogram(ds.g, lam, wt, 64)
    assert np.array_equal(packed[0], plain[0]) and np.array_equal(packed[1] << d, plain[1]) and np.array_equal(packed[2] << dw, plain[2])


# --- one tree ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def synth():
    X, y, qid = synth_dataset(7, 5000, 10, 50)
    return X, y, qid, fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)


@pytest.fixture(scope="module")
def trec():
    d = np.load(os.path.join(GOLDEN, "trec_news_2018.npz"))
    X, y, qid = d["train_X"], d["train_y"], d["train_qid"]
    return X, y, qid, fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)


def _expected_tree(X, lam, wt, order_ids, feats, binned, L, fs, depth, min_leaf, k, bits, key, goss=None, **kw):
    if goss is not None:
        a, b, gkey = goss
        return qm.goss_tree(X, lam, wt, order_ids, feats, binned, L, fs, depth, min_leaf, k, bits, key, a, b, gkey, **kw)
    return qm.tree_on_sample(X, lam, wt, order_ids, feats, binned, L, fs, depth, min_leaf, k, bits, key, **kw), L


def _one_tree(X, g, c, lam, wt, k, depth, min_leaf, bits, seed, tree, qsel=None, fsel=None, binned=None, goss=None, **kw):
    queries = lm.query_lists(c)
    order_ids = np.concatenate(queries)
    feats = list(range(X.shape[1]))
    binned = hm.bin_matrix(X, order_ids, feats, k) if binned is None else binned
    L = np.arange(len(order_ids)) if qsel is None else sm.instance_rows(queries, qsel)
    fs = list(range(len(feats))) if fsel is None else list(fsel)
    key = qm.keys(seed, tree + 1)[tree]
    gk = None if goss is None else (goss[0], goss[1], gm.keys(goss[2], goss[3] + 1)[goss[3]])
    exp, rows = _expected_tree(X, lam, wt, order_ids, feats, binned, L, fs, depth, min_leaf, k, bits, key, goss=gk, **kw)
    got = native.hist_tree(g, lam, wt, k, depth, min_leaf, queries=qsel, features=None if fsel is None else [feats[s] for s in fsel],
                           split_gain="newton", goss=goss, quant=(bits, seed, tree), **kw).to_dict()["DecisionTree"]
    assert got == exp
    return got, rows


def _leaves_are_full_precision(tree, X, lam, wt, ids, l2):
    """Every leaf of the tree is G / (H + lambda_l2) of the fixed-point sums of its own entries of the list `ids`."""
    Q, S, W, Sw = nm.quantise_pair(lam[ids], wt[ids], len(ids))

    def walk(node, at):
        if "LeafNode" in node:
            assert node["LeafNode"] == nm.leaf_value(int(Q[at].sum()), int(W[at].sum()), S, Sw, l2)
            return 1
        sp = node["FeatureSplit"]
        left = X[ids[at], sp["fid"]] <= np.float32(sp["split"])
        return walk(sp["lhs"], at[left]) + walk(sp["rhs"], at[~left])
    return walk(tree, np.arange(len(ids)))


@pytest.mark.parametrize("k,depth", [(2, 1), (2, 4), (64, 4), (64, 10), (256, 4), (256, 10)])
def test_one_tree_is_the_restatements(synth, k, depth):
    X, y, qid, g, c = synth
    lam, wt = _gradients(len(y), k + depth)
    bits = {2: 2, 64: 4, 256: 8}[k]
    tree, _ = _one_tree(X, g, c, lam, wt, k, depth, 10, bits, seed=9, tree=3, lambda_l2=0.5, min_sum_hessian=2.0 ** -8)
    assert ("FeatureSplit" in tree) == (depth > 1)
    leaves = _leaves_are_full_precision(tree, X, lam, wt, np.concatenate(lm.query_lists(c)), 0.5)
    assert leaves == json.dumps(tree).count("LeafNode")
    if depth > 1:  # the quantisation reaches the tree: the unquantised one is another, and so is another tree's key
        plain = native.hist_tree(g, lam, wt, k, depth, 10, split_gain="newton", lambda_l2=0.5, min_sum_hessian=2.0 ** -8).to_dict()["DecisionTree"]
        assert plain != tree


def test_trees_leafwise_symmetric_goss_and_on_samples(synth):
    X, y, qid, g, c = synth
    lam, wt = _gradients(len(y), 77)
    nq = len(lm.query_lists(c))
    binned = hm.bin_matrix(X, np.concatenate(lm.query_lists(c)), list(range(X.shape[1])), 32)
    common = dict(binned=binned, lambda_l2=1.0)
    _one_tree(X, g, c, lam, wt, 32, 6, 5, 4, 2, 0, qsel=np.arange(0, nq, 2), fsel=[0, 3, 4, 8], **common)
    for max_leaves in (2, 31):  # (a budget that binds: the depth limit would allow 2^11 leaves)
        tree, _ = _one_tree(X, g, c, lam, wt, 32, 12, 5, 3, 2, 1, max_leaves=max_leaves, **common)
        assert json.dumps(tree).count("LeafNode") == max_leaves
    sym, _ = _one_tree(X, g, c, lam, wt, 32, 5, 5, 4, 2, 2, symmetric=True, **common)
    assert "FeatureSplit" in sym
    _one_tree(X, g, c, lam, wt, 32, 5, 5, 4, 2, 2, symmetric=True, fsel=[1, 2, 9], min_split_gain=2.0 ** -20, **common)
    for goss in ((0.2, 0.1, 6, 1), (0.5, 0.5, 6, 1)):
        tree, rows = _one_tree(X, g, c, lam, wt, 32, 6, 5, 4, 2, 3, goss=goss, **common)
        assert (len(rows) < len(y)) == (goss[0] + goss[1] < 1.0) and "FeatureSplit" in tree
        _leaves_are_full_precision(tree, X, *gm.amplified(lam, wt, np.concatenate(lm.query_lists(c)), rows, *_top_amp(lam, c, goss)),
                                   np.concatenate(lm.query_lists(c))[rows], 1.0)
    _one_tree(X, g, c, lam, wt, 32, 8, 5, 4, 2, 4, goss=(0.2, 0.1, 6, 2), max_leaves=12, qsel=np.arange(1, nq, 2), **common)
    # min_leaf_support beyond a side, then beyond the list: fewer splits, then one leaf of the list's own full-precision sums
    tree, _ = _one_tree(X, g, c, lam, wt, 32, 6, 2400, 4, 2, 5, **common)
    assert json.dumps(tree).count("LeafNode") <= 2
    tree, _ = _one_tree(X, g, c, lam, wt, 32, 6, 6000, 4, 2, 5, **common)
    assert list(tree) == ["LeafNode"] and tree["LeafNode"] != 0.0
    # every gradient zero: LeafNode(0.0)
    zero, _ = _one_tree(X, g, c, np.zeros(len(y)), wt, 32, 6, 5, 4, 2, 6, **common)
    assert zero == {"LeafNode": 0.0}


def _top_amp(lam, c, goss):
    order_ids = np.concatenate(lm.query_lists(c))
    _, top, _, amp = gm.goss_list(lam, np.arange(len(order_ids)), order_ids, goss[0], goss[1], gm.keys(goss[2], goss[3] + 1)[goss[3]])
    return top, amp


def test_one_tree_over_sixty_six_thousand_instances():
    X, y, qid = synth_dataset(11, 66000, 6, 600)
    g, c = fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)
    lam, wt = _gradients(len(y), 5)
    tree, _ = _one_tree(X, g, c, lam, wt, 16, 4, 10, 4, seed=1, tree=0)
    assert "FeatureSplit" in tree


# --- training ------------------------------------------------------------------------------------

def _ensemble(trees, weights):
    if not trees:
        return fr.CModel.from_dict(EMPTY)
    return fr.CModel.from_dict({"Ensemble": {"weights": [float(w) for w in weights], "models": [{"DecisionTree": x} for x in trees]}})


def _trees(model):
    return [m["DecisionTree"] for m in model.to_dict()["Ensemble"]["models"]]


def _stagewise(g, c, X, y, measure, params, names=None, binned=None, strict=True):
    """Trains with the key and holds every stage to the restatements: tree t is the quantised restatement's fit (under GOSS over
    the GOSS list with amplified gradients) to the DEVICE's gradients of the ensemble the tree is fitted to (the prefix; under
    DART without the dropped trees), over the tree's query and feature sample, under the key K_t; the running measures are the
    oracle's of the oracle's ensemble scores, the prediction is the oracle's."""
    params = dict(params, split_gain="newton")
    req = cmod._request(measure, "histogram", **params)
    p = req.params
    bits = p.grad_quant_bits
    a, b = p.goss_top_rate, p.goss_other_rate
    known = {k: v for k, v in params.items() if k not in ("grad_quant_bits", "symmetric_trees", "goss_top_rate", "goss_other_rate")}
    cm = cmod.Composed(X, y, c, measure, dict(fr.LambdaMARTParams().to_dict(), **dict(known, grower="histogram")), names=names, binned=binned)
    model = g.train_model(req)
    st = native.last_train_stats()["lambdamart"]
    assert QUANT_STATS <= set(st) and st["grad_quant_bits"] == bits and 0.0 <= st["quant_ms"] < st["grow_ms"] and (st["quant_ms"] > 0.0 or not strict)
    d = model.to_dict()
    got = _trees(model)
    T = st["trees"]
    trees = got
    if p.early_stopping_rounds > 0:  # the trees the stats speak of: those of a run without the rule
        free = {k: v for k, v in params.items() if k != "early_stopping_rounds"}
        trees = _trees(g.train_model(cmod._request(measure, "histogram", **dict(free, num_trees=T))))
        assert len(trees) == T and got == trees[:st["best_iteration"]]
        best, n_trained, stopped, kept = cm.stopping(st["valid_measure"])
        assert (st["best_iteration"], T, st["stopped_early"], len(got)) == (best, n_trained, stopped, kept)
    else:
        assert len(got) == T == p.num_trees
    keys, gkeys, xkeys = qm.keys(p.seed, T), gm.keys(p.seed, T), xm.keys(p.seed, T)
    plan = dm.plan(p.seed, p.drop_rate, p.max_drop, p.skip_drop, T, p.learning_rate) if p.drop_rate > 0 else None
    if plan is not None:
        assert st["dropped"] == [len(D) for D, _, _ in plan] and (any(st["dropped"]) or not strict)
        assert np.asarray(d["Ensemble"]["weights"], dtype=np.float64).tobytes() == plan[-1][2].tobytes()
    else:
        assert d["Ensemble"]["weights"] == [p.learning_rate] * len(got)
    for t in range(T):
        fsel, qsel = cm.sample(t)
        if plan is not None:
            D, before, after = plan[t]
            keep = dm.kept(t, D)
            fitted_to = _ensemble([trees[i] for i in keep], before[keep])
        else:
            after = [p.learning_rate] * (t + 1)
            fitted_to = _ensemble(trees[:t], after[:t])
        lam, wt = native.lambda_gradients(fitted_to, g, measure, p.sigma, queries=qsel if cm.subset(qsel) else None,
                                          truncation_level=p.truncation_level, lambda_norm=p.lambda_norm, objective=p.objective,
                                          xe_key=xkeys[t])
        lam, wt = np.nan_to_num(lam), np.nan_to_num(wt)
        L = sm.instance_rows(cm.queries, qsel)
        exp, rows = _expected_tree(X, lam, wt, cm.order_ids, cm.feats, cm.binned, L, list(fsel), p.max_depth, p.min_leaf_support,
                                   p.split_candidates, bits, keys[t], goss=(a, b, gkeys[t]) if a > 0 else None, max_leaves=p.max_leaves,
                                   symmetric=p.symmetric_trees, **cm.newton())
        if a > 0:
            assert st["goss_instances"][t] == len(rows), "tree %d" % t
        assert trees[t] == exp, "tree %d differs from the restatement's fit" % t
        tr, va, err = cm.measures(c.score_ensemble(trees[:t + 1], after))
        assert err == 0
        assert st["train_measure"][t] == tr, "train_measure[%d]" % t
        if va is not None:
            assert st["valid_measure"][t] == va, "valid_measure[%d]" % t
    assert np.array_equal(native.predict_scores_dense(model, g), c.score_ensemble(got, d["Ensemble"]["weights"]))
    assert any("FeatureSplit" in t for t in trees) or not strict
    return model, st


def _shape(data):
    if data == "trec":
        return dict(max_depth=5, min_leaf_support=5, split_candidates=16)
    return dict(max_depth=4, min_leaf_support=10, split_candidates=12)


@pytest.mark.parametrize("bits", [2, 4, 8])
@pytest.mark.parametrize("data", ["trec", "synth"])
def test_stagewise_identity(request, data, bits):
    X, y, qid, g, c = request.getfixturevalue(data)
    kw = dict(num_trees=10, seed=11, grad_quant_bits=bits, **_shape(data))
    model, st = _stagewise(g, c, X, y, "ndcg@7", kw)
    got = json.dumps(model.to_dict())
    # two runs give identical bytes, and the seed reaches the rounding
    assert json.dumps(g.train_model(cmod._request("ndcg@7", "histogram", split_gain="newton", **kw)).to_dict()) == got
    assert json.dumps(g.train_model(cmod._request("ndcg@7", "histogram", split_gain="newton", **dict(kw, seed=12))).to_dict()) != got


SMALL = dict(num_trees=6, seed=3, max_depth=4, min_leaf_support=5, split_candidates=16, grad_quant_bits=4)


@pytest.mark.parametrize("extra", [
    dict(query_sampling_rate=0.5, feature_sampling_rate=0.5),
    dict(validation_queries="every fifth", early_stopping_rounds=2, num_trees=12, learning_rate=0.5),
    dict(validation_queries="every fifth", feature_sampling_rate=0.5),
    dict(drop_rate=0.5, skip_drop=0.25, max_drop=3),
    dict(objective="xendcg"),
    dict(objective="map"),
    dict(objective="mrr"),
    dict(truncation_level=3, lambda_norm=True),
    dict(max_leaves=6, max_depth=10, lambda_l2=0.5, min_sum_hessian=2.0 ** -6),
    dict(symmetric_trees=True, lambda_l2=0.5),
    dict(goss_top_rate=0.2, goss_other_rate=0.1),
    dict(goss_top_rate=0.5, goss_other_rate=0.5),
    dict(goss_top_rate=0.2, goss_other_rate=0.1, max_leaves=6, max_depth=10, query_sampling_rate=0.5),
], ids=["samples", "holdout+stopping", "holdout+features", "dart", "xendcg", "map", "mrr", "truncation+norm", "leafwise", "symmetric", "goss",
        "goss-everything-kept", "goss+leafwise+sample"])
def test_the_key_composes_with_the_other_keys(synth, extra):
    X, y, qid, g, c = synth
    names = cmod._names(qid)
    extra = dict(extra)
    if extra.get("validation_queries"):
        extra["validation_queries"] = names[::5]
    _stagewise(g, c, X, y, "ndcg@10", dict(SMALL, **extra), names=names)


def test_a_validation_dataset_and_an_init_model(synth):
    """No tree reads the validation dataset, so the trees are those of the run without it; continued training resumes the key
    stream at the model's tree count, so three trees and three more are the six of one run."""
    X, y, qid, g, c = synth
    gB = fr.CDataset.from_numpy(X[:1200], y[:1200], qid[:1200])
    kw = dict(SMALL, split_gain="newton")
    six = g.train_model(cmod._request("ndcg@10", "histogram", **kw))
    with_valid = g.train_model(cmod._request("ndcg@10", "histogram", **kw), valid=gB)
    st = native.last_train_stats()["lambdamart"]
    assert _trees(with_valid) == _trees(six) and len(st["valid_measure"]) == 6 and QUANT_STATS <= set(st)
    first = g.train_model(cmod._request("ndcg@10", "histogram", **dict(kw, num_trees=3)))
    second = g.train_model(cmod._request("ndcg@10", "histogram", **dict(kw, num_trees=3)), init_model=first)
    assert _trees(first) == _trees(six)[:3] and _trees(second) == _trees(six)
    fresh_keys = g.train_model(cmod._request("ndcg@10", "histogram", **dict(kw, num_trees=3, seed=4)), init_model=first)
    assert _trees(fresh_keys)[3:] != _trees(six)[3:]


def test_width_zero_is_the_key_absent(synth):
    X, y, qid, g, c = synth
    kw = dict(num_trees=5, seed=2, max_depth=4, min_leaf_support=10, split_candidates=12, split_gain="newton", lambda_l2=0.25)
    plain = g.train_model(cmod._request("ndcg@7", "histogram", **kw))
    st_plain = native.last_train_stats()["lambdamart"]
    assert not (QUANT_STATS & set(st_plain)) and "grad_quant_bits" not in cmod._request("ndcg@7", "histogram", **kw).to_dict()["params"]["LambdaMART"]
    zero = g.train_model(cmod._request("ndcg@7", "histogram", grad_quant_bits=0, **kw))
    st = native.last_train_stats()["lambdamart"]
    assert json.dumps(zero.to_dict()) == json.dumps(plain.to_dict())
    assert set(st) == set(st_plain) and st["train_measure"] == st_plain["train_measure"]
    # the plain request is still the Newton restatement's, stage by stage
    cm = cmod.Composed(X, y, c, "ndcg@7", dict(fr.LambdaMARTParams().to_dict(), **dict(kw, grower="histogram")))
    trees = _trees(plain)
    for t in range(len(trees)):
        lam, wt = native.lambda_gradients(_ensemble(trees[:t], [0.1] * t), g, "ndcg@7", 1.0)
        assert trees[t] == cm.tree(lam, wt, *cm.sample(t))
    # ... and with the key it is another model
    quantised = g.train_model(cmod._request("ndcg@7", "histogram", grad_quant_bits=3, **kw))
    assert json.dumps(quantised.to_dict()) != json.dumps(plain.to_dict())


# --- small soak ----------------------------------------------------------------------------------

def _soak_case(i):
    """Case i of the soak: a small random set and the width drawn with the other keys the key composes with, from a
    generator of its own."""
    rng = np.random.default_rng([20221128, i])
    n, d, q = int(rng.integers(300, 1500)), int(rng.integers(3, 8)), int(rng.integers(8, 40))
    X, y, qid = synth_dataset(int(rng.integers(1, 10 ** 6)), n, d, q)
    p = dict(num_trees=4, seed=int(rng.integers(0, 2 ** 63)), grad_quant_bits=int(rng.integers(2, 9)), max_depth=int(rng.integers(2, 7)),
             min_leaf_support=int(rng.integers(1, 20)), split_candidates=int(rng.choice([2, 5, 16, 64, 256])),
             learning_rate=float(rng.choice([0.1, 0.3])), lambda_l2=float(rng.choice([0.0, 0.5])))
    shape = rng.random()
    if shape < 0.35:
        p["max_leaves"] = int(rng.integers(2, 12))
        p["max_depth"] = int(rng.integers(3, 12))
    elif shape < 0.6:
        p["symmetric_trees"] = True
    if rng.random() < 0.5:
        p["query_sampling_rate"] = float(rng.choice([0.3, 0.7]))
    if rng.random() < 0.5:
        p["feature_sampling_rate"] = float(rng.choice([0.4, 0.8]))
    names = cmod._names(qid)
    if rng.random() < 0.4:
        p["validation_queries"] = names[int(rng.integers(0, 3))::4]
    p["objective"] = str(rng.choice(["ndcg", "ndcg", "map", "xendcg"]))
    if p["objective"] == "ndcg" and rng.random() < 0.5:
        p["truncation_level"] = int(rng.integers(1, 6))
    if rng.random() < 0.3:
        p.update(drop_rate=0.5, skip_drop=0.0)
    if rng.random() < 0.4 and not p.get("symmetric_trees"):
        a = float(rng.choice([0.1, 0.2, 0.5]))
        p.update(goss_top_rate=a, goss_other_rate=float(rng.choice([x for x in (0.1, 0.25, 0.5) if a + x <= 1.0])))
    return X, y, qid, names, p


@pytest.mark.parametrize("i", range(12))
def test_soak(i):
    X, y, qid, names, p = _soak_case(i)
    g, c = fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)
    try:
        _stagewise(g, c, X, y, "ndcg@5", p, names=names, strict=False)
    except AssertionError as e:
        raise AssertionError("soak case %d %r: %s" % (i, p, e))
