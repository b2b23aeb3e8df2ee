"""LambdaMART's leaf regularisation on the device ("Leaf regularisation"): lambda_l1, max_delta_step and
path_smooth on the histogram grower, held bit for bit to the numpy restatement (tests/lambdamart_reg_model.py).  The single
trees are grown by `native.hist_tree` from designed gradients (tests/lambdamart_reg_stages.py), so every case is designed and
not hoped for; the trainings are held stage by stage."""
import json

import numpy as np
import pytest

from fastrank_amd import native
from tests import lambdamart_composed_model as cmod
from tests import lambdamart_reg_model as rm
from tests import lambdamart_reg_stages as rs

pytestmark = pytest.mark.gpu

REGS = ["l1", "cap", "smooth", "all"]


@pytest.fixture(scope="module")
def designed():
    """Per k: the designed case, its device dataset, and the restatement's trees, computed once and left unchanged."""
    out = {}
    for k in rs.KS:
        d = rs.Designed(k)
        g, _ = rs.datasets(d.X, d.y, d.qid)
        out[k] = (d, g)
    return out


@pytest.fixture(scope="module")
def small():
    X, y, qid = rs.small_dataset(5)
    g, c = rs.datasets(X, y, qid)
    return X, y, qid, g, c


def _kernels_of(call):
    """The result of call(), and the names of the kernels it launched."""
    native.profile_enable(True)
    native.profile_reset()
    try:
        out = call()
        return out, set(native.profile_stats())
    finally:
        native.profile_enable(False)


def _search(kernels):
    """The split-search kernels among them (the first training of a dataset also bins it, once)."""
    return {n for n in kernels if "scan" in n or "sym" in n or "pick" in n}


# --- 1, 2: the scan kernels against the restatement ---------------------------------------------------

@pytest.mark.parametrize("name", REGS)
@pytest.mark.parametrize("k", rs.KS)
def test_level_wise_tree_equals_restatement(designed, k, name):
    d, g = designed[k]
    reg = d.regs()[name]
    trace = []
    exp = d.expected(reg, trace=trace, **rs.LEVELS)
    assert exp != d.expected((0.0, 0.0, 0.0), **rs.LEVELS)  # the key reaches the tree
    if k >= 64 and name in ("smooth", "all"):
        assert rs.smoothing_changes_a_winner(trace)  # at some node another candidate wins than without path_smooth
    if k >= 64 and name == "all":
        assert len(rs.parents_at(trace, 4)) >= 4  # a level of nodes with different parent outputs: the per-node record's indexing
    if name == "l1":
        assert 0.0 in rm.leaves_of(exp)
    if name == "cap":
        assert max(abs(v) for v in rm.leaves_of(exp)) == rs.CAP
    got, kernels = _kernels_of(lambda: d.grown(g, reg, **rs.LEVELS))
    assert got == exp
    assert "hist_scan_reg_kernel" in kernels and not ({"hist_scan_newton_kernel", "hist_scan_monotone_kernel"} & kernels)


@pytest.mark.parametrize("name", REGS)
@pytest.mark.parametrize("k", rs.KS)
def test_leaf_wise_tree_equals_restatement(designed, k, name):
    d, g = designed[k]
    reg = d.regs()[name]
    exp = d.expected(reg, **rs.LEAVES)
    assert exp != d.expected((0.0, 0.0, 0.0), **rs.LEAVES)
    assert json.dumps(exp).count("LeafNode") == 8 or k == 2  # (with one edge per feature the threshold may leave fewer leaves to split)
    got, kernels = _kernels_of(lambda: d.grown(g, reg, **rs.LEAVES))
    assert got == exp
    assert {"hist_leaf_scan_reg_kernel", "hist_pick_kernel"} <= kernels
    assert not ({"hist_leaf_scan_kernel<newton>", "hist_leaf_scan_monotone_kernel"} & kernels)


def test_every_feature_and_a_larger_leaf_support(designed):
    """Without a feature sample, and with min_leaf_support above 1: the other arguments of the kernels."""
    d, g = designed[64]
    for reg in d.regs().values():
        for mode in (rs.LEVELS, rs.LEAVES):
            exp = rm.fit_tree(d.X, d.lam, d.wt, d.order_ids, d.feats, mode["max_depth"], 7, 64, reg, max_leaves=mode["max_leaves"],
                              binned=d.binned, lambda_l2=rs.L2, min_sum_hessian=2.0 ** -3, min_split_gain=2.0 ** -6)
            got = native.hist_tree(g, d.lam, d.wt, 64, mode["max_depth"], 7, split_gain="newton", lambda_l2=rs.L2, min_sum_hessian=2.0 ** -3,
                                   min_split_gain=2.0 ** -6, max_leaves=mode["max_leaves"], lambda_l1=reg[0], max_delta_step=reg[1],
                                   path_smooth=reg[2]).to_dict()["DecisionTree"]
            assert got == exp


# --- 3: monotone signs with each key -------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["levels", "leaves"])
@pytest.mark.parametrize("name", REGS)
@pytest.mark.parametrize("k", [64, 256])
def test_monotone_signs_with_each_key(designed, k, name, mode):
    d, g = designed[k]
    reg = d.regs()[name]
    kw = dict(rs.LEVELS if mode == "levels" else rs.LEAVES)
    mono = {0: -1, 3: 1}  # feature 0 against the gradients' lean: the bounds bind
    exp = d.expected(reg, monotone=mono, **kw)
    assert exp != d.expected(reg, **kw) and exp != d.expected((0.0, 0.0, 0.0), monotone=mono, **kw)
    assert d.grown(g, reg, monotone=mono, **kw) == exp


# --- 4: symmetric trees ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["l1", "cap", "l1+cap"])
@pytest.mark.parametrize("k", rs.KS)
def test_symmetric_tree_equals_restatement(designed, k, name):
    d, g = designed[k]
    reg = {"l1": (d.l1, 0.0, 0.0), "cap": (0.0, rs.CAP, 0.0), "l1+cap": (d.l1 / 4.0, rs.CAP, 0.0)}[name]
    exp = d.expected(reg, symmetric=True, max_depth=5)
    assert exp != d.expected((0.0, 0.0, 0.0), symmetric=True, max_depth=5)
    got, kernels = _kernels_of(lambda: d.grown(g, reg, symmetric=True, max_depth=5))
    assert got == exp
    assert "hist_scan_sym_reg_kernel" in kernels and "hist_scan_sym_kernel" not in kernels
    with pytest.raises(ValueError, match="symmetric trees take no path_smooth"):
        d.grown(g, (0.0, 0.0, 1.0), symmetric=True, max_depth=5)


# --- 5: new kernels, old bytes -------------------------------------------------------------------------------

@pytest.mark.parametrize("k", rs.KS)
def test_a_cap_nothing_reaches_gives_the_plain_tree_from_the_new_kernels(designed, k):
    d, g = designed[k]
    off, never = (0.0, 0.0, 0.0), (0.0, 1e300, 0.0)
    for kw in (rs.LEVELS, rs.LEAVES, dict(rs.LEVELS, monotone={0: -1, 3: 1}), dict(symmetric=True, max_depth=5)):
        plain, old = _kernels_of(lambda: d.grown(g, off, **dict(kw)))
        same, new = _kernels_of(lambda: d.grown(g, never, **dict(kw)))
        assert json.dumps(same) == json.dumps(plain) and "FeatureSplit" in plain
        assert not any("_reg_kernel" in name for name in old) and any("_reg_kernel" in name for name in new)


def test_keys_at_an_explicit_zero_are_the_keyless_request(small):
    X, y, qid, g, c = small
    kw = dict(num_trees=4, max_depth=4, min_leaf_support=2, split_candidates=16, split_gain="newton", lambda_l2=0.5)
    for extra in (dict(), dict(max_leaves=6, max_depth=8), dict(symmetric_trees=True)):
        plain, old = _kernels_of(lambda: g.train_model(cmod._request("ndcg@5", "histogram", **dict(kw, **extra))))
        st_plain = native.last_train_stats()["lambdamart"]
        zero, same = _kernels_of(lambda: g.train_model(cmod._request("ndcg@5", "histogram", lambda_l1=0.0, max_delta_step=0.0, path_smooth=0.0,
                                                                      **dict(kw, **extra))))
        st = native.last_train_stats()["lambdamart"]
        assert json.dumps(zero.to_dict()) == json.dumps(plain.to_dict())
        assert _search(old) == _search(same) and _search(old) and not any("_reg_kernel" in n for n in old | same)
        assert not (rs.REG_STATS & set(st)) and set(st) == set(st_plain)
        never = g.train_model(cmod._request("ndcg@5", "histogram", max_delta_step=1e300, **dict(kw, **extra)))
        assert json.dumps(never.to_dict()) == json.dumps(plain.to_dict())
        assert native.last_train_stats()["lambdamart"]["max_delta_step"] == 1e300


# --- 6: training ---------------------------------------------------------------------------------------------

TRAIN = dict(num_trees=10, seed=4, max_depth=5, min_leaf_support=2, split_candidates=32, learning_rate=0.3, lambda_l2=2.0 ** -6,
             lambda_l1=2.0 ** -7, max_delta_step=0.75, path_smooth=8.0)


@pytest.mark.parametrize("mode", [dict(), dict(max_leaves=8, max_depth=8)], ids=["levels", "leaves"])
def test_training_stage_by_stage(small, mode):
    X, y, qid, g, c = small
    model, st, traces = rs.stagewise(g, c, X, y, "ndcg@5", dict(TRAIN, **mode))
    assert all(traces)  # every tree split
    plain = g.train_model(cmod._request("ndcg@5", "histogram", split_gain="newton",
                                        **{k: v for k, v in dict(TRAIN, **mode).items() if k not in rs.REG_STATS}))
    assert json.dumps(plain.to_dict()) != json.dumps(model.to_dict())


@pytest.mark.parametrize("extra", [
    dict(goss_top_rate=0.3, goss_other_rate=0.3),
    dict(query_sampling_rate=0.6, feature_sampling_rate=0.6),
    dict(validation_queries="every fourth"),
    dict(drop_rate=0.5, skip_drop=0.0, max_drop=3),
    dict(objective="xendcg", max_leaves=6),
    dict(monotone_constraints={"0": 1, "2": -1}, truncation_level=4),
    dict(symmetric_trees=True, path_smooth=0.0),
], ids=["goss", "samples", "holdout", "dart", "xendcg+leaves", "monotone+truncation", "symmetric"])
def test_training_composes_with_the_other_keys(small, extra):
    X, y, qid, g, c = small
    names = cmod._names(qid)
    extra = dict(extra)
    if extra.get("validation_queries"):
        extra["validation_queries"] = names[::4]
    rs.stagewise(g, c, X, y, "ndcg@5", dict(TRAIN, **extra), names=names)


def test_five_trees_and_five_more_are_the_ten(small):
    X, y, qid, g, c = small
    kw = dict(TRAIN, split_gain="newton", query_sampling_rate=0.7)
    ten = g.train_model(cmod._request("ndcg@5", "histogram", **kw))
    five = g.train_model(cmod._request("ndcg@5", "histogram", **dict(kw, num_trees=5)))
    more = g.train_model(cmod._request("ndcg@5", "histogram", **dict(kw, num_trees=5)), init_model=five)
    assert json.dumps(more.to_dict()) == json.dumps(ten.to_dict())
    st = native.last_train_stats()["lambdamart"]
    assert st["init_trees"] == 5 and (st["lambda_l1"], st["max_delta_step"], st["path_smooth"]) == (2.0 ** -7, 0.75, 8.0)


# --- 7: properties of the trained model -------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [dict(), dict(max_leaves=8, max_depth=8), dict(monotone_constraints={"0": 1})], ids=["levels", "leaves", "monotone"])
def test_every_leaf_of_a_trained_model_is_within_the_cap(small, mode):
    X, y, qid, g, c = small
    kw = dict(dict(num_trees=10, max_depth=6, min_leaf_support=1, split_candidates=64, split_gain="newton", learning_rate=0.5), **mode)
    free = [v for t in rs.trees_of(g.train_model(cmod._request("ndcg@5", "histogram", **kw))) for v in rm.leaves_of(t)]
    cap = float(np.median(np.abs(free)))
    capped = [v for t in rs.trees_of(g.train_model(cmod._request("ndcg@5", "histogram", max_delta_step=cap, **kw))) for v in rm.leaves_of(t)]
    assert max(abs(v) for v in free) > cap
    assert all(abs(v) <= cap for v in capped) and any(abs(v) == cap for v in capped)


def test_a_threshold_above_every_gradient_sum_trains_single_zero_leaves(small):
    X, y, qid, g, c = small
    lam, _ = native.lambda_gradients(rs.ensemble([], []), g, "ndcg@5", 1.0)
    l1 = 1.5 * float(np.sum(np.abs(np.nan_to_num(lam))))  # above |G| of the root and of any subset of it
    model = g.train_model(cmod._request("ndcg@5", "histogram", split_gain="newton", num_trees=10, max_depth=6, min_leaf_support=1, lambda_l1=l1))
    assert rs.trees_of(model) == [{"LeafNode": 0.0}] * 10
    assert not np.any(native.predict_scores_dense(model, g))
