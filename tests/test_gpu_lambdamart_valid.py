"""LambdaMART's held-out validation queries and early stopping on the device against the numpy restatement
(tests/lambdamart_valid_model.py, DESIGN.md section 11, "Validation and early stopping"), both growers: training stage by
stage, the two subset means, the stopping rule and the truncated model."""
import json
import os

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import clib, native
from fastrank_amd.training import hold_out_queries
from oracle import pyoracle as o
from tests import lambdamart_hist_model as hm
from tests import lambdamart_model as lm
from tests import lambdamart_sample_model as sm
from tests import lambdamart_valid_model as vm
from tests.lambdamart_composed_model import _ensemble, _names, _request
from tests.conftest import GOLDEN, synth_dataset

pytestmark = pytest.mark.gpu

VALID_KEYS = {"validation_queries", "training_queries", "valid_measure", "best_iteration", "best_valid_measure", "stopped_early",
              "early_stopping_rounds"}
GROWERS = ["exact", "histogram"]


@pytest.fixture(scope="module")
def trec():
    d = np.load(os.path.join(GOLDEN, "trec_news_2018.npz"))
    X, y, qid = d["train_X"], d["train_y"], d["train_qid"]
    return X, y, qid, fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)


@pytest.fixture(scope="module")
def synth():
    X, y, qid = synth_dataset(7, 5000, 10, 50)
    X = X.copy()
    X[::7, 3] = -0.0
    X[:, 9] = 2.5
    return X, y, qid, fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)


def _trees(model):
    return [m["DecisionTree"] for m in model.to_dict()["Ensemble"]["models"]]


def _stagewise(g, X, queries, names, feats, measure, T, grower, rates, seed, held, params, c=None, present=None, n_total=None,
               qrel=None, norms=None):
    """Every tree equals the restatement's fit on the restatement's training sample to the device's gradients of the prefix
    model; the two measures after every tree are the means of the device's per-query values over T and H; with the oracle
    dataset `c` of the same rows also the oracle's measures and scores."""
    req = _request(measure, grower, num_trees=T, query_sampling_rate=rates[0], feature_sampling_rate=rates[1], seed=seed,
                   validation_queries=list(held), **params)
    req.judgments = qrel
    p = req.params
    model = g.train_model(req)
    st = native.last_train_stats()["lambdamart"]
    d = model.to_dict()
    trees = [m["DecisionTree"] for m in d["Ensemble"]["models"]]
    assert d["Ensemble"]["weights"] == [p.learning_rate] * T and len(trees) == T
    Tq, Hq = vm.split(names, held)
    assert st["training_queries"] == len(Tq) and st["validation_queries"] == len(Hq) and st["trees"] == T
    assert len(st["train_measure"]) == T and len(st["valid_measure"]) == T
    order_ids = np.concatenate(queries)
    binned = hm.bin_matrix(X, order_ids, feats, p.split_candidates) if grower == "histogram" else None  # (the FULL list)
    nq_t = 0
    for t in range(T):
        fsel, qsel = vm.sample(seed, t, len(feats), Tq, rates)
        hf, hq = native.lambdamart_sample(g, p, t)
        assert np.array_equal(hf, np.asarray(feats)[fsel]) and np.array_equal(hq, qsel)
        assert not set(hq.tolist()) & set(Hq.tolist()), "a held-out query in tree %d's sample" % t
        lam, wt = native.lambda_gradients(_ensemble(trees[:t], p.learning_rate), g, measure, p.sigma, qrel, n_total=n_total)
        exp = sm.tree_for(grower, X, np.nan_to_num(lam), np.nan_to_num(wt), queries, feats, binned, qsel, fsel, p.max_depth,
                          p.min_leaf_support, p.split_candidates, present)
        assert trees[t] == exp, "tree %d differs from the restatement's fit on its training sample" % t
        nq_t += len(qsel)
        got_names, per_q = native.evaluate_dense(_ensemble(trees[:t + 1], p.learning_rate), g, measure, qrel)
        assert got_names == list(names)
        assert st["train_measure"][t] == vm.subset_mean(per_q, Tq), "train_measure[%d]" % t
        assert st["valid_measure"][t] == vm.subset_mean(per_q, Hq), "valid_measure[%d]" % t
        if c is not None:
            exp_q, _ = c.metric_from_scores(measure, c.score_ensemble(trees[:t + 1], [p.learning_rate] * (t + 1)), norms)
            assert st["train_measure"][t] == vm.subset_mean(exp_q, Tq) and st["valid_measure"][t] == vm.subset_mean(exp_q, Hq)
    if c is not None:
        assert np.array_equal(native.predict_scores_dense(model, g), c.score_ensemble(trees, d["Ensemble"]["weights"]))
    if rates[0] < 1.0 or rates[1] < 1.0:
        assert st["sample_queries"] == nq_t / T
    best = vm.stopping(st["valid_measure"], 0)[0]
    assert st["best_iteration"] == best and st["best_valid_measure"] == st["valid_measure"][best - 1]
    assert st["stopped_early"] is False and st["early_stopping_rounds"] == 0 and st["grower"] == grower
    return model, st


RATES = [(1.0, 1.0), (0.5, 0.25), (1.0, 0.3), (0.5, 1.0)]


@pytest.mark.parametrize("rates", RATES)
@pytest.mark.parametrize("grower", GROWERS)
def test_stagewise_identity_trec(trec, grower, rates):
    X, y, qid, g, c = trec
    names = _names(qid)
    _stagewise(g, X, lm.query_lists(c), names, list(range(X.shape[1])), "ndcg@10", 12, grower, rates, 11, names[2::3],
               dict(max_depth=5, min_leaf_support=5, split_candidates=16), c=c)


@pytest.mark.parametrize("rates", RATES[:2])
@pytest.mark.parametrize("grower", GROWERS)
def test_stagewise_identity_synthetic(synth, grower, rates):
    X, y, qid, g, c = synth
    names = _names(qid)
    held = hold_out_queries(names, 0.3, 5)
    assert len(held) == 15
    _stagewise(g, X, lm.query_lists(c), names, list(range(X.shape[1])), "ndcg", 10, grower, rates, 2 ** 63 + 5, held,
               dict(max_depth=6, min_leaf_support=10, split_candidates=64), c=c)


# --- held-out labels ---------------------------------------------------------------------------------

@pytest.mark.parametrize("rates", [(1.0, 1.0), (0.5, 0.5)])
@pytest.mark.parametrize("grower", GROWERS)
def test_held_out_labels_carry_no_influence(synth, grower, rates):
    """Without judgments a query's norm is a function of its own labels, and nothing in a gradient crosses queries: other
    labels on the held-out queries leave every tree and the training measure as they were.  (With `judgments` the norms
    come from the judgments, for training queries as well: that is the one way labels outside T's documents reach a tree,
    and it does not depend on which queries are held out.)"""
    X, y, qid, g, c = synth
    names = _names(qid)
    held = names[1::4]
    kw = dict(num_trees=6, max_depth=5, min_leaf_support=10, split_candidates=32, validation_queries=held,
              query_sampling_rate=rates[0], feature_sampling_rate=rates[1], seed=3)
    a = g.train_model(_request("ndcg@10", grower, **kw))
    sa = native.last_train_stats()["lambdamart"]
    y2 = y.copy()
    rows = np.isin(qid, [int(q) for q in held])
    y2[rows] = (y2[rows] + 1 + np.arange(rows.sum()) % 3) % 5
    assert np.any(y2 != y) and np.array_equal(y2[~rows], y[~rows])
    b = fr.CDataset.from_numpy(X, y2, qid).train_model(_request("ndcg@10", grower, **kw))
    sb = native.last_train_stats()["lambdamart"]
    assert json.dumps(a.to_dict()) == json.dumps(b.to_dict())
    assert sa["train_measure"] == sb["train_measure"] and sa["valid_measure"] != sb["valid_measure"]
    # ... and the hold-out itself does change the trees
    assert json.dumps(g.train_model(_request("ndcg@10", grower, **dict(kw, validation_queries=[]))).to_dict()) != json.dumps(a.to_dict())


# --- early stopping -----------------------------------------------------------------------------------

# chosen with the restatement alone (tests/test_lambdamart_valid_host.py::test_restatement_stops_early_on_the_trec_golden):
# every second query of the trec golden held out, learning rate 0.3, r = 3, 30 trees asked for
ES = dict(num_trees=30, learning_rate=0.3, max_depth=4, min_leaf_support=5, split_candidates=16)
ES_BEST = {"exact": 5, "histogram": 8}


@pytest.mark.parametrize("grower", GROWERS)
def test_early_stopping_triggers(trec, grower):
    X, y, qid, g, c = trec
    names = _names(qid)
    held = names[1::2]
    Tq, Hq = vm.split(names, held)
    r = 3
    exp = vm.train(X, y, c, Hq, grower=grower, measure="ndcg@10", early_stopping_rounds=r, **ES)
    assert exp["best_iteration"] == ES_BEST[grower] and exp["best_iteration"] + r < ES["num_trees"]
    model = g.train_model(_request("ndcg@10", grower, validation_queries=held, early_stopping_rounds=r, **ES))
    st = native.last_train_stats()["lambdamart"]
    best = st["best_iteration"]
    assert st["stopped_early"] is True
    assert st["trees"] == best + r
    assert len(_trees(model)) == best
    # (the restatement's own gradients differ from the device's in the last bits, so its trees are compared stage by stage
    # above, not here; the fixture's best tree is the one it was chosen for)
    assert best == exp["best_iteration"]
    assert len(st["valid_measure"]) == st["trees"] == len(st["train_measure"]) and st["early_stopping_rounds"] == r
    assert (best, st["trees"], True, best) == vm.stopping(st["valid_measure"], r, ES["num_trees"])
    # the truncated model is, byte for byte, the model of the shorter training
    short = g.train_model(_request("ndcg@10", grower, validation_queries=held, **dict(ES, num_trees=best)))
    assert json.dumps(short.to_dict()) == json.dumps(model.to_dict())
    ss = native.last_train_stats()["lambdamart"]
    assert ss["trees"] == best and ss["stopped_early"] is False and ss["valid_measure"] == st["valid_measure"][:best]
    # the reported best is what evaluating the returned model on the held-out queries gives
    by_q = g.subsample_queries(held).evaluate(model, "ndcg@10")
    assert set(by_q) == set(held)
    assert o.mean(np.array([by_q[q] for q in names if q in by_q])) == st["best_valid_measure"] == st["valid_measure"][best - 1]
    assert np.array_equal(native.predict_scores_dense(model, g), c.score_ensemble(_trees(model), [ES["learning_rate"]] * best))


@pytest.mark.parametrize("grower", GROWERS)
def test_no_rounds_returns_all_trees_and_reports_the_best(trec, grower):
    X, y, qid, g, c = trec
    names = _names(qid)
    held = names[1::2]
    model = g.train_model(_request("ndcg@10", grower, validation_queries=held, **dict(ES, num_trees=12)))
    st = native.last_train_stats()["lambdamart"]
    assert len(_trees(model)) == 12 and st["trees"] == 12 and st["stopped_early"] is False and st["early_stopping_rounds"] == 0
    assert st["best_iteration"] == ES_BEST[grower] and st["best_valid_measure"] == max(st["valid_measure"])
    # rounds that never pass: training runs out of trees, the model is still the trees up to the best
    late = g.train_model(_request("ndcg@10", grower, validation_queries=held, early_stopping_rounds=50, **dict(ES, num_trees=12)))
    sl = native.last_train_stats()["lambdamart"]
    assert sl["trees"] == 12 and sl["stopped_early"] is False and sl["valid_measure"] == st["valid_measure"]
    assert late.to_dict()["Ensemble"] == {"weights": [0.3] * st["best_iteration"],
                                          "models": model.to_dict()["Ensemble"]["models"][:st["best_iteration"]]}


# --- edge cases ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("grower", GROWERS)
def test_one_held_out_query_and_one_training_query(trec, grower):
    X, y, qid, g, c = trec
    names = _names(qid)
    queries = lm.query_lists(c)
    feats = list(range(X.shape[1]))
    kw = dict(max_depth=4, min_leaf_support=2, split_candidates=16)
    longest = names[int(np.argmax([len(q) for q in queries]))]
    _stagewise(g, X, queries, names, feats, "ndcg@10", 4, grower, (1.0, 1.0), 1, [names[-1]], kw, c=c)          # |H| = 1
    _stagewise(g, X, queries, names, feats, "ndcg@10", 4, grower, (1.0, 1.0), 1, [q for q in names if q != longest], kw, c=c)  # |T| = 1
    _stagewise(g, X, queries, names, feats, "ndcg@10", 4, grower, (0.5, 0.5), 1, [q for q in names if q != longest], kw, c=c)


@pytest.mark.parametrize("grower", GROWERS)
def test_a_hold_out_across_the_mean_segments(grower):
    """|T| = 431 and |H| = 289: both above one 256-query segment and no multiple of it; the subsets' segments are cut in
    their compacted lists, not in the view's."""
    X, y, qid = synth_dataset(23, 9000, 8, 720)
    g, c = fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)
    names = _names(qid)
    assert len(names) == 720
    rng = np.random.default_rng(2)
    pick = np.sort(rng.choice(720, 289, replace=False))
    held = [names[i] for i in pick]
    o.set_mean_segment(o.DEVICE_MEAN_SEGMENT)
    try:
        model, st = _stagewise(g, X, lm.query_lists(c), names, list(range(8)), "ndcg@10", 4, grower, (1.0, 1.0), 0, held,
                               dict(max_depth=4, min_leaf_support=10, split_candidates=32), c=c)
        assert (st["training_queries"], st["validation_queries"]) == (431, 289)
        _stagewise(g, X, lm.query_lists(c), names, list(range(8)), "ndcg@10", 3, grower, (0.7, 0.5), 4, held,
                   dict(max_depth=4, min_leaf_support=10, split_candidates=32), c=c)
        # one sequential pass over a subset agrees to rounding (at most 431 values in [0, 1]: far below 1e-12)
        _, per_q = native.evaluate_dense(model, g, "ndcg@10")
        o.set_mean_segment(0)
        Tq, Hq = vm.split(names, held)
        flat = [vm.subset_mean(per_q, Tq), vm.subset_mean(per_q, Hq)]
        assert abs(flat[0] - st["train_measure"][-1]) < 1e-12 and abs(flat[1] - st["valid_measure"][-1]) < 1e-12
    finally:
        o.set_mean_segment(0)


@pytest.mark.parametrize("grower", GROWERS)
def test_a_sampled_view(trec, grower):
    X, y, qid, g, c = trec
    names = _names(qid)
    sub_names = names[::2]
    sub = g.subsample_queries(sub_names).subsample_feature_names(sorted(g.feature_names())[1:])
    feats = sorted(sub.feature_ids())
    ids = native.hist_bins(sub, 16)[0].astype(np.int64)
    queries = np.split(ids, np.flatnonzero(np.diff(qid[ids]) != 0) + 1)
    view_names = [str(int(qid[q[0]])) for q in queries]
    assert sorted(view_names) == sorted(sub_names)
    _stagewise(sub, X, queries, view_names, feats, "ndcg@10", 6, grower, (0.6, 0.6), 21, view_names[1::3],
               dict(max_depth=4, min_leaf_support=4, split_candidates=16), n_total=X.shape[0])
    with pytest.raises(Exception, match="validation_queries names `%s`, which is not a query of the dataset" % names[1]):
        sub.train_model(_request("ndcg@10", grower, num_trees=2, validation_queries=[view_names[0], names[1]]))


def test_a_file_loaded_dataset_with_qids_in_no_numeric_order(tmp_path):
    from tests.conftest import ranksvm_presence
    from tests.test_gpu_lambdamart import _sparse_file

    src = str(tmp_path / "sparse.train")
    X, y, qid = _sparse_file(src)
    # the same rows under other query ids: 30, 4, 100, 12, ... (the view's order is the file's, not the numbers')
    new_ids = {1: 30, 2: 4, 3: 100, 4: 12, 5: 7, 6: 51, 7: 2, 8: 19}
    path = str(tmp_path / "renamed.train")
    with open(src) as fin, open(path, "w") as fout:
        for line in fin:
            label, q, rest = line.split(" ", 2)
            fout.write("%s qid:%d %s" % (label, new_ids[int(q.split(":")[1])], rest))
    qid2 = np.array([new_ids[int(q)] for q in qid], dtype=np.int64)
    rd = fr.CDataset.open_ranksvm(path)
    present = ranksvm_presence(path, X.shape[1])
    feats = sorted(rd.feature_ids())
    ids = native.hist_bins(rd, 16)[0].astype(np.int64)
    queries = np.split(ids, np.flatnonzero(np.diff(qid2[ids]) != 0) + 1)
    names = [str(int(qid2[q[0]])) for q in queries]
    assert names == ["30", "4", "100", "12", "7", "51", "2", "19"]
    kw = dict(max_depth=4, min_leaf_support=3, split_candidates=16)
    held = ["100", "2", "4"]
    _stagewise(rd, X, queries, names, feats, "ndcg@10", 5, "exact", (1.0, 1.0), 3, held, kw, present=present)
    _stagewise(rd, X, queries, names, feats, "ndcg@10", 5, "exact", (0.6, 0.5), 3, held, kw, present=present)
    _stagewise(rd, X, queries, names, feats, "ndcg@10", 5, "histogram", (1.0, 1.0), 3, held, kw)
    _stagewise(rd, X, queries, names, feats, "ndcg@10", 5, "histogram", (0.6, 0.5), 3, held, kw)


@pytest.mark.parametrize("grower", GROWERS)
def test_judgments_given(trec, grower):
    X, y, qid, g, c = trec
    with open(os.path.join(GOLDEN, "newsir18_entity_qrel.json")) as fh:
        qrel_dict = json.load(fh)
    names = _names(qid)
    _stagewise(g, X, lm.query_lists(c), names, list(range(X.shape[1])), "ndcg@5", 6, grower, (1.0, 1.0), 0, names[::4],
               dict(max_depth=4, min_leaf_support=5, split_candidates=16), c=c, qrel=fr.CQRel.from_dict(qrel_dict),
               norms=c.qrel_norms("ndcg@5", qrel_dict))


def test_bins_are_built_once_with_and_without_a_hold_out(trec):
    X, y, qid, _, c = trec
    g = fr.CDataset.from_numpy(X, y, qid)  # (a dataset of its own: no bins yet)
    names = _names(qid)
    kw = dict(num_trees=4, max_depth=4, min_leaf_support=5, split_candidates=16)
    plain = g.train_model(_request("ndcg", **kw))
    assert native.last_train_stats()["lambdamart"]["bins_ms"] > 0.0
    ids, fids, edges, bins = native.hist_bins(g, 16)
    for extra in (dict(validation_queries=names[::3]), dict(validation_queries=names[1::2], query_sampling_rate=0.5, seed=2),
                  dict(validation_queries=names[:1], feature_sampling_rate=0.5, early_stopping_rounds=2), dict()):
        g.train_model(_request("ndcg", **dict(kw, **extra)))
        assert native.last_train_stats()["lambdamart"]["bins_ms"] == 0.0
        ids2, fids2, edges2, bins2 = native.hist_bins(g, 16)
        assert np.array_equal(ids, ids2) and np.array_equal(fids, fids2) and np.array_equal(bins, bins2)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(edges, edges2))
    # ... and a training without a hold-out after the ones with is what it was before them
    assert json.dumps(g.train_model(_request("ndcg", **kw)).to_dict()) == json.dumps(plain.to_dict())


# --- no keys = the behaviour without the feature --------------------------------------------------------

@pytest.mark.parametrize("grower", GROWERS)
def test_no_keys_is_the_request_with_an_empty_list(trec, grower):
    X, y, qid, g, c = trec
    kw = dict(num_trees=5, max_depth=4, min_leaf_support=5, split_candidates=16)
    absent = _request("ndcg@10", grower, **kw)
    assert not set(absent.to_dict()["params"]["LambdaMART"]) & {"validation_queries", "early_stopping_rounds"}
    a = g.train_model(absent)
    sa = native.last_train_stats()["lambdamart"]
    assert not set(sa) & VALID_KEYS
    wire = absent.to_dict()
    wire["params"]["LambdaMART"].update(validation_queries=[], early_stopping_rounds=0)
    m = fr.CModel(clib._unwrap(clib._load().train_model(json.dumps(wire).encode(), g.pointer)))
    sb = native.last_train_stats()["lambdamart"]
    assert json.dumps(m.to_dict()) == json.dumps(a.to_dict())
    assert sorted(sb) == sorted(sa) and sb["train_measure"] == sa["train_measure"] and sb["trees"] == 5
    # the training measure without a hold-out is the mean over every query, as before
    _, per_q = native.evaluate_dense(a, g, "ndcg@10")
    assert sa["train_measure"][-1] == o.mean(per_q)
    # with a hold-out the stats hold the validation fields
    g.train_model(_request("ndcg@10", grower, validation_queries=_names(qid)[:3], **kw))
    assert VALID_KEYS <= set(native.last_train_stats()["lambdamart"])


# --- the 30K shape ----------------------------------------------------------------------------------------

def test_30k_shape_with_a_tenth_held_out():
    """The 30K shape, histogram grower, a 10 % hold-out from hold_out_queries: three default-depth trees on the view of every
    tenth query equal the restatement's, and two trees on all 3.8 M documents keep the measure identities."""
    from tests.test_gpu_fullsize import _shape

    _, X, y, qid, g = _shape("30k")
    names = _names(qid)
    sub_names = names[::10]
    sub = g.subsample_queries(sub_names)
    ids, fids, edges, bins = native.hist_bins(sub, 64)
    ids = ids.astype(np.int64)
    feats = [int(f) for f in fids]
    queries = np.split(ids, np.flatnonzero(np.diff(qid[ids]) != 0) + 1)
    view_names = [str(int(qid[q[0]])) for q in queries]
    assert view_names == sub_names and len(ids) > 300_000
    held = hold_out_queries(view_names, 0.1, 30)
    assert len(held) == len(view_names) // 10
    Tq, Hq = vm.split(view_names, held)
    binned = hm.bin_matrix(X, ids, feats, 64)
    req = _request("ndcg@10", num_trees=3, split_candidates=64, validation_queries=held)
    trees = _trees(sub.train_model(req))
    st = native.last_train_stats()["lambdamart"]
    assert (st["training_queries"], st["validation_queries"]) == (len(Tq), len(Hq))
    o.set_mean_segment(o.DEVICE_MEAN_SEGMENT)
    try:
        for t in range(3):
            lam, wt = native.lambda_gradients(_ensemble(trees[:t], 0.1), sub, "ndcg@10", 1.0, n_total=X.shape[0])
            exp = sm.hist_tree(X, np.nan_to_num(lam), np.nan_to_num(wt), ids, feats, binned, sm.instance_rows(queries, Tq),
                               np.arange(len(feats)), 6, 10, 64)
            assert trees[t] == exp, "tree %d" % t
            got_names, per_q = native.evaluate_dense(_ensemble(trees[:t + 1], 0.1), sub, "ndcg@10")
            assert got_names == view_names
            assert st["train_measure"][t] == vm.subset_mean(per_q, Tq) and st["valid_measure"][t] == vm.subset_mean(per_q, Hq)
        held_full = hold_out_queries(names, 0.1, 30)
        Tf, Hf = vm.split(names, held_full)
        assert len(Hf) == len(names) // 10 and len(Hf) > 256 and len(Hf) % 256 != 0 and len(Tf) % 256 != 0
        full = _request("ndcg@10", num_trees=2, split_candidates=64, validation_queries=held_full)
        model = g.train_model(full)
        st = native.last_train_stats()["lambdamart"]
        trees = _trees(model)
        for t in range(2):
            got_names, per_q = native.evaluate_dense(_ensemble(trees[:t + 1], 0.1), g, "ndcg@10")
            assert got_names == names
            assert st["train_measure"][t] == vm.subset_mean(per_q, Tf) and st["valid_measure"][t] == vm.subset_mean(per_q, Hf)
        assert st["train_measure"][1] > st["train_measure"][0] and st["trees"] == 2 and st["best_iteration"] in (1, 2)
        assert json.dumps(g.train_model(full).to_dict()) == json.dumps(model.to_dict())
    finally:
        o.set_mean_segment(0)
