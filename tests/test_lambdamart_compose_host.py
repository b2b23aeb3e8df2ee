"""The composed restatement of LambdaMART training (tests/lambdamart_composed_model.py) on the CPU: its dispatch against
each single-feature restatement, and the three soaks of tests/test_gpu_lambdamart_compose.py run with --dry, which shows
from the reference alone that their seeds draw and bind every key and keep the oracle-error share within 10 %."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyoracle as o
from tests import lambdamart_composed_model as cm
from tests import lambdamart_hist_model as hm
from tests import lambdamart_leafwise_model as lw
from tests import lambdamart_model as lm
from tests import lambdamart_newton_model as nm
from tests import lambdamart_objective_model as om
from tests import lambdamart_sample_model as sm
from tests import lambdamart_trunc_model as tm
from tests import lambdamart_valid_model as vm
from tests.conftest import synth_dataset

BASE = dict(num_trees=3, max_depth=4, min_leaf_support=5, split_candidates=8, sigma=1.5, learning_rate=0.25)
NEWTON = dict(split_gain="newton", lambda_l2=2.0 ** -10, min_sum_hessian=2.0 ** -6, min_split_gain=2.0 ** -20)
DRAWN = {"--objective": ["truncation_level", "lambda_norm"], "--rank-objective": ["objective"],
         "--compose": ["query_sampling_rate", "feature_sampling_rate", "seed", "validation_queries", "early_stopping_rounds", "split_gain",
                       "lambda_l2", "min_sum_hessian", "min_split_gain", "max_leaves"]}


@pytest.fixture(scope="module")
def data():
    X, y, qid = synth_dataset(11, 300, 6, 12)
    c = o.Dataset(X, y, qid)
    queries = lm.query_lists(c)
    rng = np.random.default_rng(3)
    return dict(X=X, y=y, qid=qid, c=c, queries=queries, ids=np.concatenate(queries), names=cm._names(qid), feats=list(range(X.shape[1])),
                lam=rng.normal(0.0, 1.0, len(y)) + 0.5 * (y - y.mean()), wt=rng.random(len(y)), s=rng.normal(0.0, 1.0, len(y)))


def _composed(data, measure="ndcg@5", **p):
    return cm.Composed(data["X"], data["y"], data["c"], measure, dict(BASE, **p), names=data["names"])


@pytest.mark.parametrize("soak", sorted(cm.SOAKS))
def test_the_soaks_draw_and_bind_every_key_on_the_reference_alone(soak):
    flags, seed, iters = cm.SOAKS[soak]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_lambdamart.py"), "--dry", "--iters", str(iters), "--seed", str(seed)] + flags,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["iters"] == iters and res["oracle_error_while_training"] * 10 <= iters
    assert res["growers"].get("exact", 0) >= 1 and res["growers"].get("histogram", 0) >= 1
    assert res["sampled_views"] >= 1 and res["file_loaded"] >= 1
    for flag, keys in DRAWN.items():
        assert all((res["drawn"].get(k, 0) >= 1) == (flag in flags) for k in keys), (flag, res["drawn"])
    assert sorted(res["bound"]) == sorted(cm.soak_bound_keys(flags))
    assert all(count >= 1 for count in res["bound"].values()), res["bound"]


@pytest.mark.parametrize("grower", ["exact", "histogram"])
def test_every_key_at_its_default_is_the_plain_restatement(data, grower):
    m = _composed(data, grower=grower)
    fsel, qsel = m.sample(2)
    assert np.array_equal(fsel, np.arange(6)) and np.array_equal(qsel, np.arange(len(data["queries"]))) and not m.subset(qsel)
    args = (data["X"], data["lam"], data["wt"], data["ids"], data["feats"], 4, 5, 8)
    plain = hm.fit_tree(*args) if grower == "histogram" else lm.fit_tree(*args)
    assert "FeatureSplit" in plain and m.tree(data["lam"], data["wt"], fsel, qsel) == plain
    lam, wt, rtol = m.gradients(data["s"])
    exp = lm.gradients(data["s"], data["y"], data["queries"], m.norms, 5, 1.5)
    assert lam.tobytes() == exp[0].tobytes() and wt.tobytes() == exp[1].tobytes() and np.all(rtol == 1e-12)
    per_q, _ = data["c"].metric_from_scores("ndcg@5", data["s"])
    assert m.measures(data["s"]) == (o.mean(per_q), None, 0)
    assert set(m.expected_stats()) == ({"bins"} if grower == "histogram" else set()) and not any(m.bound.values())
    got = m.train()
    model = hm.train(data["X"], data["y"], data["c"], "ndcg@5", **BASE)[0] if grower == "histogram" else lm.train(data["X"], data["y"], data["c"], "ndcg@5", **BASE)[0]
    assert got["model"] == model and got["trained"] == 3 and got["best_iteration"] == 0 and not got["stopped_early"] and not got["oracle_error"]


def test_the_gradients_follow_the_objective_keys(data):
    for p in (dict(truncation_level=2), dict(lambda_norm=True), dict(truncation_level=3, lambda_norm=True)):
        m = _composed(data, grower="exact", **p)
        lam, wt, rtol = m.gradients(data["s"], [1, 4])
        exp = tm.gradients(data["s"], data["y"], [data["queries"][q] for q in (1, 4)], [m.norms[q] for q in (1, 4)], 5, 1.5,
                           p.get("truncation_level", 0), p.get("lambda_norm", False), parts=True)
        assert lam.tobytes() == exp[0].tobytes() and wt.tobytes() == exp[1].tobytes()
        assert np.all(rtol > 1e-12) == bool(p.get("lambda_norm")) and np.all(rtol < 1e-11)
        outside = np.ones(len(lam), dtype=bool)
        outside[np.concatenate([data["queries"][q] for q in (1, 4)])] = False
        assert np.all(lam[outside] == 0.0) and np.any(lam[~outside] != 0.0)
    for objective, reported in (("map", "ap"), ("mrr", "rr")):
        m = _composed(data, grower="exact", objective=objective, truncation_level=4)
        assert m.reported == reported and np.array_equal(m.norms, data["c"].default_norms(reported))
        lam, wt, _ = m.gradients(data["s"])
        exp = om.gradients(data["s"], data["y"], data["queries"], m.norms, objective, 1.5, 4, False)
        assert lam.tobytes() == exp[0].tobytes() and wt.tobytes() == exp[1].tobytes()
        per_q, _ = data["c"].metric_from_scores(reported, data["s"])
        assert m.measures(data["s"])[0] == o.mean(per_q)


def test_the_tree_follows_the_grower_the_gain_the_budget_and_the_sample(data):
    X, lam, wt, ids, feats, queries = (data[k] for k in ("X", "lam", "wt", "ids", "feats", "queries"))
    binned = hm.bin_matrix(X, ids, feats, 8)
    fsel, qsel = np.array([0, 2, 5]), np.array([1, 3, 4, 8, 9, 11])
    rows = sm.instance_rows(queries, qsel)
    numbers = {k: v for k, v in NEWTON.items() if k != "split_gain"}
    for grower in ("exact", "histogram"):
        assert _composed(data, grower=grower).tree(lam, wt, fsel, qsel) == sm.tree_for(grower, X, lam, wt, queries, feats, binned, qsel, fsel, 4, 5, 8)
    assert _composed(data, grower="histogram", **NEWTON).tree(lam, wt, fsel, qsel) == \
        nm.tree_on_sample(X, lam, wt, ids, feats, binned, rows, fsel, 4, 5, 8, **numbers)
    assert _composed(data, grower="histogram", max_leaves=5).tree(lam, wt, fsel, qsel) == \
        lw.tree_on_sample(X, lam, wt, ids, feats, binned, rows, fsel, 4, 5, 8, 5)
    both = _composed(data, grower="histogram", max_leaves=5, max_depth=9, **NEWTON).tree(lam, wt, fsel, qsel)
    assert both == lw.tree_on_sample(X, lam, wt, ids, feats, binned, rows, fsel, 9, 5, 8, 5, **NEWTON) and lw.n_leaves(both) == 5
    # the four trees are four different trees: no dispatch falls through to another
    trees = [json.dumps(_composed(data, grower="histogram", **p).tree(lam, wt, fsel, qsel)) for p in (dict(), NEWTON, dict(max_leaves=5), dict(max_leaves=5, **NEWTON))]
    assert len(set(trees)) == 4
    # a present mask reaches the exact grower
    present = np.ones(X.shape, dtype=bool)
    present[::2, 2] = False
    m = cm.Composed(X, data["y"], data["c"], "ndcg", dict(BASE, grower="exact"), present=present)
    assert m.tree(lam, wt, fsel, qsel) == lm.fit_tree(X, lam, wt, ids[rows], [0, 2, 5], 4, 5, 8, present)
    with pytest.raises(ValueError):
        _composed(data, grower="exact", max_leaves=5)
    with pytest.raises(ValueError):
        _composed(data, grower="histogram", early_stopping_rounds=1)


@pytest.mark.parametrize("grower", ["exact", "histogram"])
def test_train_follows_the_samples_the_hold_out_and_the_stopping_rule(data, grower):
    names, held = data["names"], data["names"][2::5]
    T, H = vm.split(names, held)
    kw = dict(grower=grower, measure="ndcg@5", rates=(0.5, 0.5), seed=9, **BASE)
    m = _composed(data, grower=grower, query_sampling_rate=0.5, feature_sampling_rate=0.5, seed=9)
    exp = sm.train(data["X"], data["y"], data["c"], **kw)
    got = m.train()
    assert got["model"] == exp[0] and all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(got["samples"], exp[3]))
    for rounds in (0, 1):
        p = dict(kw, num_trees=6, learning_rate=2.0)
        m = _composed(data, grower=grower, query_sampling_rate=0.5, feature_sampling_rate=0.5, seed=9, validation_queries=held,
                      early_stopping_rounds=rounds, num_trees=6, learning_rate=2.0)
        assert np.array_equal(m.T, T) and np.array_equal(m.H, H)
        assert all(set(m.sample(t)[1].tolist()) <= set(T.tolist()) for t in range(6))
        exp = vm.train(data["X"], data["y"], data["c"], held_idx=H, early_stopping_rounds=rounds, **p)
        got = m.train()
        assert got["model"] == exp["model"] and np.array_equal(got["scores"], exp["scores"])
        assert got["train_measure"] == exp["train_measure"] and got["valid_measure"] == exp["valid_measure"]
        assert (got["best_iteration"], got["trained"], got["stopped_early"]) == (exp["best_iteration"], exp["trees"], exp["stopped_early"])
        assert m.stopping(got["valid_measure"]) == vm.stopping(exp["valid_measure"] + [0.0] * (6 - exp["trees"]), rounds, 6)
        assert m.bound["early_stopping_rounds"] == exp["stopped_early"]
        assert set(m.expected_stats()) == cm.SAMPLING_STATS | cm.VALID_STATS | ({"bins"} if grower == "histogram" else set())
    assert exp["stopped_early"] and len(exp["model"]["Ensemble"]["models"]) == exp["best_iteration"] < exp["trees"] < 6


@pytest.mark.parametrize("gain", [dict(), NEWTON])
def test_a_leaf_budget_the_level_wise_tree_fits_in_is_level_wise_growth(data, gain):
    level = _composed(data, grower="histogram", **gain)
    exp = level.train()
    most = max(lw.n_leaves(t) for t in exp["trees"])
    assert 2 < most <= 8
    for budget in (most, 8, 255):
        m = _composed(data, grower="histogram", max_leaves=budget, **gain)
        got = m.train(observe=True)
        assert got["model"] == exp["model"] and got["train_measure"] == exp["train_measure"] and not m.bound["max_leaves"]
    tight = _composed(data, grower="histogram", max_leaves=most - 1, **gain)
    got = tight.train(observe=True)
    assert got["model"] != exp["model"] and tight.bound["max_leaves"] and max(lw.n_leaves(t) for t in got["trees"]) == most - 1


def test_what_bound_is_noted_from_the_restatement_alone(data):
    m = _composed(data, grower="histogram", num_trees=2, truncation_level=1, lambda_norm=True, query_sampling_rate=1e-9,
                  **dict(NEWTON, min_sum_hessian=1e30))
    got = m.train(observe=True)
    assert [len(q) for _, q in got["samples"]] == [1, 1] and all(t == {"LeafNode": 0.0} or "LeafNode" in t for t in got["trees"])
    assert m.bound == dict(truncation_level=True, lambda_norm=True, max_leaves=False, min_sum_hessian=True, min_split_gain=False,
                           early_stopping_rounds=False, query_sampling_rate=True, objective=False)
    y = data["y"].copy()
    y[data["queries"][0]] = 0.0
    c = o.Dataset(data["X"], y, data["qid"])
    for held, bound in (([], True), ([data["names"][0]], False)):  # (a held-out query is no training query)
        assert cm.Composed(data["X"], y, c, "ndcg", dict(BASE, grower="exact", objective="map", validation_queries=held),
                           names=data["names"]).bound["objective"] is bound
    free = _composed(data, grower="histogram", num_trees=2, truncation_level=40)  # (no query is that long: nothing to cut)
    free.train(observe=True)
    assert not any(free.bound.values())
