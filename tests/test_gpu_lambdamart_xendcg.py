"""LambdaMART's listwise objective "xendcg" on the device (lambda_grad_xe_kernel; DESIGN.md section 11, "Listwise
objective") against the numpy restatement (tests/lambdamart_xendcg_model.py) and the exact statement
(tests/lambdamart_xendcg_exact.py).

Gradients: bit for bit wherever `exp` is exact (all scores of a query equal; one document 800 above the rest), since every
other operation is a correctly rounded basic one in a fixed order; with continuous scores within the bound derived in
tests/lambdamart_xendcg_bound.py of the exact statement.
Training: every tree equals the restatement's fit to the DEVICE's gradients of the prefix model under that tree's key.
"""
import json
import os

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import clib, native
from oracle import pyoracle as o
from tests import lambdamart_composed_model as cmod
from tests import lambdamart_dart_model as dm
from tests import lambdamart_hist_model as hm
from tests import lambdamart_model as lm
from tests import lambdamart_valid_model as vm
from tests import lambdamart_xendcg_bound as xb
from tests import lambdamart_xendcg_exact as xe
from tests import lambdamart_xendcg_model as xm
from tests.conftest import GOLDEN, synth_dataset

pytestmark = pytest.mark.gpu

EMPTY = {"Ensemble": {"weights": [], "models": []}}
LENGTHS = [1, 2, 63, 64, 65, 128, 129, 1300, 4100]  # the lane strides, the tree step, the path that keeps nothing in registers
KEYS = [0, 12345, 2 ** 64 - 1]


def _edge_set():
    """Stored order = row order, the score is column 0.  By query id: 1..9: the LENGTHS with all scores equal; 10..17: the
    LENGTHS from 2 on with one document 800 above the rest (the rest spread over [0, 1): their exp underflows to +0.0);
    18: every label 0 (norm NaN); 19: labels (2, -60 x 7), whose norm is positive while Phi = 4 - the sum of eight gammas is
    positive under some keys and not under others; 20: labels 0..4 in turn, equal scores."""
    rng = np.random.default_rng(77)
    lens = {q + 1: n for q, n in enumerate(LENGTHS)}
    lens.update({10 + q: n for q, n in enumerate(LENGTHS[1:])})
    lens.update({18: 10, 19: 8, 20: 25})
    qid = np.concatenate([np.full(n, q, dtype=np.int64) for q, n in lens.items()])
    n = len(qid)
    y = rng.choice(5, size=n, p=[0.5, 0.2, 0.15, 0.1, 0.05]).astype(np.float64)
    s = np.zeros(n)
    for q, m in lens.items():
        rows = np.flatnonzero(qid == q)
        y[rows[0]] = max(y[rows[0]], 1.0)  # (a positive label: the norm is positive)
        if q <= 9 or q == 20:
            s[rows] = float(rng.integers(-3, 4)) + 0.25
        elif q <= 17:
            s[rows] = rng.random(m)
            s[rows[int(rng.integers(0, m))]] += 800.0
    y[qid == 18] = 0.0
    y[qid == 19] = [2.0] + [-60.0] * 7
    y[qid == 20] = np.arange(25) % 5
    X = np.zeros((n, 3), dtype=np.float32)
    X[:, 0] = s
    X[:, 1] = rng.random(n)
    return X, y, qid


@pytest.fixture(scope="module")
def edge():
    X, y, qid = _edge_set()
    g, c = fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)
    model = fr.CModel.from_dict({"Linear": {"weights": [1.0, 0.0, 0.0]}})
    queries = lm.query_lists(c)
    assert [len(x) for x in queries] == LENGTHS + LENGTHS[1:] + [10, 8, 25]
    return X, y, qid, g, c, model, queries


@pytest.fixture(scope="module")
def trec():
    d = np.load(os.path.join(GOLDEN, "trec_news_2018.npz"))
    X, y, qid = d["train_X"], d["train_y"], d["train_qid"]
    return X, y, qid, fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)


@pytest.fixture(scope="module")
def synth():
    X, y, qid = synth_dataset(7, 5000, 10, 50)
    return X, y, qid, fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)


def _grad(model, g, key, measure="ndcg", **kw):
    return native.lambda_gradients(model, g, measure, 1.0, objective="xendcg", xe_key=key, **kw)


# --- gradients -----------------------------------------------------------------------------------

@pytest.mark.parametrize("key", KEYS)
def test_gradients_are_the_restatements_bits_where_exp_is_exact(edge, key):
    X, y, qid, g, c, model, queries = edge
    scores = native.predict_scores_dense(model, g)
    assert np.array_equal(scores, X[:, 0].astype(np.float64))
    norms = c.default_norms("ndcg")
    assert np.isnan(norms[17]) and norms[18] > 0.0
    exp_l, exp_w = xm.gradients(scores, y, queries, norms, key)
    lam, wt = _grad(model, g, key)
    for q, ids in enumerate(queries):
        assert lam[ids].tobytes() == exp_l[ids].tobytes(), "lambda of query %d (%d documents)" % (q + 1, len(ids))
        assert wt[ids].tobytes() == exp_w[ids].tobytes(), "w of query %d (%d documents)" % (q + 1, len(ids))
    for q in (1, 18):  # one document; no positive label: exact zeros
        assert not lam[qid == q].any() and not wt[qid == q].any() and not np.signbit(lam[qid == q]).any()
    for q in list(range(2, 18)) + [20]:
        assert lam[qid == q].any(), q
    for q in range(10, 18):  # rho = (1, 0, ...): u = 0 on top, so every w is 0 and the top document's a is +0.0
        assert not wt[qid == q].any() and lam[qid == q].any()
    # sigma and the measure's depth are read for nothing; a second call gives the same bytes
    for other in (native.lambda_gradients(model, g, "ndcg@3", 2.5, objective="xendcg", xe_key=key), _grad(model, g, key)):
        assert other[0].tobytes() == lam.tobytes() and other[1].tobytes() == wt.tobytes()


def test_the_key_moves_the_gradients_and_phi_decides_query_19(edge):
    X, y, qid, g, c, model, queries = edge
    ids = queries[18]
    G = xm.gains(y)
    dead = next(k for k in range(1, 64) if xm.query_gradients(np.zeros(8), G[ids], ids, k, parts=True)[2] is None)
    live = next(k for k in range(1, 64) if xm.query_gradients(np.zeros(8), G[ids], ids, k, parts=True)[2] is not None)
    lam_d, wt_d = _grad(model, g, dead)
    lam_l, wt_l = _grad(model, g, live)
    assert not lam_d[ids].any() and not wt_d[ids].any()  # Phi <= 0: zeros although the norm is positive
    assert lam_l[ids].any() and wt_l[ids].all()
    assert lam_d[queries[2]].tobytes() != lam_l[queries[2]].tobytes()
    # an absent key is key 0
    out_l, out_w = np.full(len(y), np.nan), np.full(len(y), np.nan)
    native._status(native._load().fr_debug_lambda_gradients_opts(model.pointer, g.pointer, None, b"ndcg", 1.0, None, 0,
                                                               json.dumps({"objective": "xendcg"}).encode(), out_l.ctypes.data,
                                                               out_w.ctypes.data, len(y)))
    zero = _grad(model, g, 0)
    assert out_l.tobytes() == zero[0].tobytes() and out_w.tobytes() == zero[1].tobytes()


def test_judgments_decide_which_queries_are_live(edge):
    """The norms are the evaluator's: judgments that know a positive gain for query 18 (every label 0) make it live, and
    nothing else of a norm is read."""
    X, y, qid, g, c, model, queries = edge
    qrel_dict = {"18": {"18.%d" % i: float(i % 3) for i in range(6)}, "3": {"3.%d" % i: 4.0 for i in range(9)}}
    norms = c.qrel_norms("ndcg", qrel_dict)
    assert norms[17] > 0.0 and norms[2] != c.default_norms("ndcg")[2]
    qrel = fr.CQRel.from_dict(qrel_dict)
    key = 5
    lam, wt = native.lambda_gradients(model, g, "ndcg", 1.0, qrel, objective="xendcg", xe_key=key)
    exp_l, exp_w = xm.gradients(X[:, 0].astype(np.float64), y, queries, norms, key)
    assert lam.tobytes() == exp_l.tobytes() and wt.tobytes() == exp_w.tobytes()
    plain = _grad(model, g, key)
    assert lam[qid == 18].any() and not plain[0][qid == 18].any()
    assert lam[qid != 18].tobytes() == plain[0][qid != 18].tobytes()


@pytest.fixture(scope="module")
def designed():
    """tests/lambdamart_xendcg_bound.py's designed queries as one dataset (the scores become the f32 the dataset stores)."""
    qs = xb.designed_queries()
    X = np.zeros((sum(len(s) for _, s, _ in qs), 2), dtype=np.float32)
    X[:, 0] = np.concatenate([s for _, s, _ in qs])
    y = np.concatenate([v for _, _, v in qs])
    qid = np.concatenate([np.full(len(s), k + 1, dtype=np.int64) for k, (_, s, _) in enumerate(qs)])
    y[np.flatnonzero(np.diff(qid, prepend=0))] = 3.0  # (a positive label in every query)
    return qs, X, y, qid, fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)


def test_gradients_lie_within_the_bound_of_the_exact_statement(designed):
    qs, X, y, qid, g, c = designed
    model = fr.CModel.from_dict({"Linear": {"weights": [1.0, 0.0]}})
    scores = native.predict_scores_dense(model, g)
    key = 0xC0FFEE
    lam, wt = _grad(model, g, key)
    worst = {}
    for (name, _, _), ids in zip(qs, lm.query_lists(c)):
        q = xe.ExactXe(scores[ids], y[ids], ids, key)
        assert q.live
        ratio, _ = xb.worst_ratio(q, lam[ids], wt[ids])
        kind = name.split(", ", 1)[1]
        worst[kind] = max(worst.get(kind, 0.0), ratio)
    for kind in sorted(worst):
        print("device, %s: worst error / bound %.3f" % (kind, worst[kind]))
    print("device: the largest error / bound over the designed queries %.3f" % max(worst.values()))


def test_a_query_sample_leaves_the_other_queries_alone(edge):
    X, y, qid, g, c, model, queries = edge
    full_l, full_w = _grad(model, g, 9)
    for qsel in ([16], [0, 2, 8, 19], [7, 8, 15, 16]):
        lam, wt = _grad(model, g, 9, queries=np.asarray(qsel))
        inside = np.zeros(len(full_l), dtype=bool)
        inside[np.concatenate([queries[q] for q in qsel])] = True
        assert lam[inside].tobytes() == full_l[inside].tobytes() and wt[inside].tobytes() == full_w[inside].tobytes()
        assert np.all(np.isnan(lam[~inside])) and np.all(np.isnan(wt[~inside]))


def test_a_sampled_view_gets_its_parents_bits(edge, synth):
    """gamma hangs on the original instance id, so a query of a view has the targets it has in the parent."""
    X, y, qid, g, c, model, queries = edge
    full_l, full_w = _grad(model, g, 31)
    names = [str(q) for q in (3, 9, 12, 17, 20)]
    sub = g.subsample_queries(names)
    lam, wt = _grad(model, sub, 31, n_total=len(y))
    inside = np.isin(qid, [int(x) for x in names])
    assert lam[inside].tobytes() == full_l[inside].tobytes() and wt[inside].tobytes() == full_w[inside].tobytes()
    assert np.all(np.isnan(lam[~inside]))
    # ... with continuous scores as well: the same library calls on the same operands
    Xs, ys, qs, gs, cs = synth
    m = fr.CModel.from_dict({"Linear": {"weights": [0.5, -1.0, 2.0] + [0.0] * 7}})
    full = _grad(m, gs, 31)
    pick = sorted(gs.queries())[::4]
    view = _grad(m, gs.subsample_queries(pick), 31, n_total=len(ys))
    inside = np.isin(qs, [int(x) for x in pick])
    assert view[0][inside].tobytes() == full[0][inside].tobytes() and view[1][inside].tobytes() == full[1][inside].tobytes()


# --- training ------------------------------------------------------------------------------------

def _ensemble(trees, weights):
    if not trees:
        return fr.CModel.from_dict(EMPTY)
    return fr.CModel.from_dict({"Ensemble": {"weights": [float(w) for w in weights], "models": [{"DecisionTree": x} for x in trees]}})


def _stagewise(g, c, X, y, measure, params, names=None):
    """Trains with objective "xendcg" and holds every stage to the restatements: tree t is the fit (by the restatement of the
    request's grower keys, tests/lambdamart_composed_model.py) to the DEVICE's gradients, under the key k_t of the
    restatement's stream, of the ensemble the tree is fitted to (the prefix, under DART without the dropped trees), over the
    tree's query sample; the reported measures are the oracle's NDCG of the oracle's ensemble scores."""
    req = cmod._request(measure, params.get("grower", "exact"), objective="xendcg", **{k: v for k, v in params.items() if k != "grower"})
    p = req.params
    cm = cmod.Composed(X, y, c, measure, dict(fr.LambdaMARTParams().to_dict(), **dict(params, grower=p.grower, objective="xendcg")), names=names)
    assert cm.reported == measure
    model = g.train_model(req)
    st = native.last_train_stats()["lambdamart"]
    assert st["objective"] == "xendcg" and "truncation_level" not in st and "lambda_norm" not in st
    d = model.to_dict()
    trees = [m["DecisionTree"] for m in d["Ensemble"]["models"]]
    T = st["trees"]
    assert len(trees) == T == p.num_trees, "(early stopping is checked by its own test)"
    keys = xm.keys(p.seed, T)
    plan = dm.plan(p.seed, p.drop_rate, p.max_drop, p.skip_drop, T, p.learning_rate) if p.drop_rate > 0 else None
    if plan is not None:
        assert st["dropped"] == [len(D) for D, _, _ in plan] and any(st["dropped"])
        assert np.asarray(d["Ensemble"]["weights"], dtype=np.float64).tobytes() == plan[-1][2].tobytes()
    else:
        assert d["Ensemble"]["weights"] == [p.learning_rate] * T
    for t in range(T):
        fsel, qsel = cm.sample(t)
        if plan is not None:
            D, before, after = plan[t]
            keep = dm.kept(t, D)
            fitted_to = _ensemble([trees[i] for i in keep], before[keep])
        else:
            after = [p.learning_rate] * (t + 1)
            fitted_to = _ensemble(trees[:t], after[:t])
        lam, wt = _grad(fitted_to, g, keys[t], measure, queries=qsel if cm.subset(qsel) else None)
        if t == 0:  # the device's gradients are the listwise ones, bit for bit: at scores 0.0 exp is exact
            qs = [cm.queries[q] for q in qsel]
            exp_l, exp_w = xm.gradients(np.zeros(len(y)), y, qs, [cm.norms[q] for q in qsel], keys[0])
            rows = np.concatenate(qs)
            assert lam[rows].tobytes() == exp_l[rows].tobytes() and wt[rows].tobytes() == exp_w[rows].tobytes()
        exp = cm.tree(np.nan_to_num(lam), np.nan_to_num(wt), fsel, qsel)
        assert trees[t] == exp, "tree %d differs from the restatement's fit" % t
        tr, va, err = cm.measures(c.score_ensemble(trees[:t + 1], after))
        assert err == 0
        assert st["train_measure"][t] == tr, "train_measure[%d]" % t
        if va is not None:
            assert st["valid_measure"][t] == va, "valid_measure[%d]" % t
    final = d["Ensemble"]["weights"]
    assert np.array_equal(native.predict_scores_dense(model, g), c.score_ensemble(trees, final))
    assert any("FeatureSplit" in t for t in trees)
    return model, st


@pytest.mark.parametrize("grower", ["exact", "histogram"])
@pytest.mark.parametrize("data", ["trec", "synth"])
def test_stagewise_identity(request, data, grower):
    """Fails where the objective or the key is ignored: the trees are then fitted to other gradients."""
    X, y, qid, g, c = request.getfixturevalue(data)
    params = dict(max_depth=5, min_leaf_support=5, split_candidates=16) if data == "trec" else dict(max_depth=4, min_leaf_support=10, split_candidates=12)
    model, _ = _stagewise(g, c, X, y, "ndcg@7", dict(grower=grower, num_trees=10, seed=11, **params))
    got = json.dumps(model.to_dict())
    plain = json.dumps(g.train_model(cmod._request("ndcg@7", grower, num_trees=10, seed=11, **params)).to_dict())
    other = json.dumps(g.train_model(cmod._request("ndcg@7", grower, num_trees=10, seed=12, objective="xendcg", **params)).to_dict())
    assert got != plain and got != other  # (the seed reaches nothing but the keys here)
    again = json.dumps(g.train_model(cmod._request("ndcg@7", grower, num_trees=10, seed=11, objective="xendcg", **params)).to_dict())
    assert again == got


SMALL = dict(num_trees=8, seed=3, max_depth=4, min_leaf_support=5, split_candidates=16)


@pytest.mark.parametrize("extra", [
    dict(grower="histogram", split_gain="newton", lambda_l2=0.5, min_sum_hessian=2.0 ** -6, max_leaves=6, max_depth=10),
    dict(grower="histogram", drop_rate=0.5, skip_drop=0.25, max_drop=3),
    dict(grower="exact", drop_rate=0.5, skip_drop=0.25, max_drop=3),
    dict(grower="histogram", query_sampling_rate=0.5, feature_sampling_rate=0.5, validation_queries="every fifth"),
    dict(grower="exact", validation_queries="every fifth"),  # (a fixed split: the filtered query list is uploaded once)
], ids=["newton+leafwise", "dart-hist", "dart-exact", "samples+holdout", "holdout-exact"])
def test_the_objective_composes_with_the_other_keys(synth, extra):
    X, y, qid, g, c = synth
    names = cmod._names(qid)
    extra = dict(extra)
    if extra.get("validation_queries"):
        extra["validation_queries"] = names[::5]
    _stagewise(g, c, X, y, "ndcg@10", dict(SMALL, **extra), names=names)


def test_early_stopping_follows_the_requests_ndcg(synth):
    X, y, qid, g, c = synth
    names = cmod._names(qid)
    held = names[3::10]
    Tq, Hq = vm.split(names, held)
    rounds, T = 3, 25
    kw = dict(objective="xendcg", validation_queries=held, query_sampling_rate=0.5, seed=5, max_depth=4, min_leaf_support=10,
              split_candidates=12, learning_rate=0.5)
    model = g.train_model(cmod._request("ndcg@5", "histogram", num_trees=T, early_stopping_rounds=rounds, **kw))
    st = native.last_train_stats()["lambdamart"]
    n = st["trees"]
    assert st["objective"] == "xendcg" and len(st["train_measure"]) == n == len(st["valid_measure"])
    # the trees the stats speak of: the returned ones are the first best_iteration of them, so retrain without the rule
    full = g.train_model(cmod._request("ndcg@5", "histogram", num_trees=n, **kw))
    trees = [m["DecisionTree"] for m in full.to_dict()["Ensemble"]["models"]]
    for t in range(n):
        exp_q, _ = c.metric_from_scores("ndcg@5", c.score_ensemble(trees[:t + 1], [0.5] * (t + 1)))
        assert st["train_measure"][t] == vm.subset_mean(exp_q, Tq) and st["valid_measure"][t] == vm.subset_mean(exp_q, Hq)
    valid = st["valid_measure"]
    best = 1 + int(np.argmax(valid))  # the FIRST maximum
    assert st["best_iteration"] == best and st["best_valid_measure"] == valid[best - 1]
    assert n == min(T, best + rounds) and st["stopped_early"] == (n < T)
    assert [m["DecisionTree"] for m in model.to_dict()["Ensemble"]["models"]] == trees[:best]


def test_a_monotone_constraint_holds_on_the_scores(synth):
    from tests.test_gpu_lambdamart_monotone import _against, _grid, _probe

    X, y, qid, g, c = synth
    constraints = {"0": 1, "1": -1}
    kw = dict(num_trees=10, max_depth=6, min_leaf_support=10, split_candidates=64, split_gain="newton", lambda_l2=1.0, objective="xendcg")
    models = {}
    for constrained in (True, False):
        models[constrained] = g.train_model(cmod._request("ndcg@10", "histogram", monotone_constraints=constraints if constrained else {}, **kw))
        st = native.last_train_stats()["lambdamart"]
        assert st["objective"] == "xendcg" and ("monotone_constraints" in st) == constrained
    broken = 0
    for name, sign in constraints.items():
        grid = _grid(X, int(name))
        P, pq = _probe(X, int(name), grid)
        gp = fr.CDataset.from_numpy(P, np.zeros(len(P)), pq)
        for constrained, model in models.items():
            against = _against(native.predict_scores_dense(model, gp).reshape(-1, len(grid)), sign)
            if constrained:
                assert against == 0, "feature %s: the score moves against its sign at %d grid steps" % (name, against)
            else:
                broken += against
    assert broken > 0  # the same request without the key is not monotone: the property is not vacuous


# --- the other objectives are what they were -----------------------------------------------------

@pytest.mark.parametrize("grower", ["exact", "histogram"])
def test_objective_ndcg_and_the_key_absent_are_the_pairwise_restatement(synth, grower):
    X, y, qid, g, c = synth
    kw = dict(num_trees=4, max_depth=4, min_leaf_support=10, split_candidates=12)
    plain = cmod._request("ndcg@7", grower, **kw)
    p = plain.params
    assert "objective" not in plain.to_dict()["params"]["LambdaMART"]
    model = g.train_model(plain)
    stats = native.last_train_stats()["lambdamart"]
    assert "objective" not in stats
    wire = plain.to_dict()
    wire["params"]["LambdaMART"]["objective"] = "ndcg"
    spelled = fr.CModel(clib._unwrap(clib._load().train_model(json.dumps(wire).encode(), g.pointer)))
    again = native.last_train_stats()["lambdamart"]
    assert set(again) == set(stats) and again["train_measure"] == stats["train_measure"]
    assert json.dumps(spelled.to_dict()) == json.dumps(model.to_dict())
    # ... and that model is the pairwise restatement's, stage by stage
    trees = [m["DecisionTree"] for m in model.to_dict()["Ensemble"]["models"]]
    queries = lm.query_lists(c)
    order_ids = np.concatenate(queries)
    feats = list(range(X.shape[1]))
    binned = hm.bin_matrix(X, order_ids, feats, p.split_candidates) if grower == "histogram" else None
    for t in range(len(trees)):
        lam, wt = native.lambda_gradients(_ensemble(trees[:t], [p.learning_rate] * t), g, "ndcg@7", p.sigma)
        if t == 0:
            exp_l, exp_w = lm.gradients(np.zeros(len(y)), y, queries, c.default_norms("ndcg@7"), 7, p.sigma)
            assert np.allclose(lam, exp_l, rtol=1e-12, atol=0.0) and np.allclose(wt, exp_w, rtol=1e-12, atol=0.0)
            listwise = _grad(_ensemble([], []), g, 0, "ndcg@7")
            assert not np.allclose(listwise[0], lam)
        if grower == "histogram":
            exp = hm.fit_tree(X, lam, wt, order_ids, feats, p.max_depth, p.min_leaf_support, p.split_candidates, binned)
        else:
            exp = lm.fit_tree(X, lam, wt, order_ids, feats, p.max_depth, p.min_leaf_support, p.split_candidates)
        assert trees[t] == exp, "tree %d differs from the restatement's fit" % t
        exp_q, _ = c.metric_from_scores("ndcg@7", c.score_ensemble(trees[:t + 1], [p.learning_rate] * (t + 1)))
        assert stats["train_measure"][t] == o.mean(exp_q)
