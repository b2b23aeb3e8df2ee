"""Permutation importance on the device (csrc/kernels_permute.inc) against the project's own exact path
on a physically permuted matrix: for every (feature f, repeat r) the oracle copies X, writes X'[I, f] = X[src_r(I), f] with
the restatement's sources (tests/permute_model.py), makes a dataset of the view's rows and calls native.evaluate_dense.  The
per-query values must equal row f * R + r of the call's per-query output bit for bit (matched by query id), the values and
the baseline the fixed-shape means of those rows (tests/resample_model.py: means), importance and std the restated report.

Base case: 3 001 documents in queries of 1 .. 800 documents whose rows interleave, labels 0 .. 4, columns of small integers
with duplicated rows, so that permuted scores tie and the tie-break (gain, then id; neither moves) decides."""
import functools
import json

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import native
from tests import permute_model as pm
from tests import resample_model as rm

pytestmark = pytest.mark.gpu

QLENS = [1, 2, 63, 64, 65, 127, 128, 129, 300, 800, 129, 1, 300, 64, 2, 127, 65, 63, 128, 256, 100, 87]  # 3001 documents
DIMS = [1, 3, 4, 5, 9, 136]
LISTED_136 = [0, 3, 4, 67, 132, 135]
SEED = 5
TABLES = ("xb", "xcol", "xslot", "perm", "perm_host", "gain", "gexp", "gcls", "gkey", "segtab", "wofs", "wt_start", "qstart", "qlen", "qtight",
          "run_q0", "run_q1", "run_pos", "run_docs", "run_lo", "run_order", "run_wt0", "dcgtab", "colmax")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _same(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


@functools.lru_cache(maxsize=None)
def _data(d):
    rng = np.random.default_rng(300 + d)
    n = sum(QLENS)
    qid = np.repeat(np.arange(1, len(QLENS) + 1, dtype=np.int64), QLENS)[rng.permutation(n)]
    y = rng.integers(0, 5, size=n).astype(np.float64)
    X = rng.integers(-3, 4, size=(n, d)).astype(np.float32)
    for _ in range(60):  # copies of rows inside their query
        a = int(rng.integers(0, n))
        b = int(rng.choice(np.flatnonzero(qid == qid[a])))
        X[b] = X[a]
    return X, y, qid


@functools.lru_cache(maxsize=None)
def _dataset(d):
    X, y, qid = _data(d)
    return fr.CDataset.from_numpy(X, y, qid)


def _listed(d):
    return LISTED_136 if d == 136 else list(range(d))


def _leaf(v):
    return {"LeafNode": float(v)}


def _split(fid, s, lhs, rhs):
    return {"FeatureSplit": {"fid": int(fid), "split": float(s), "lhs": lhs, "rhs": rhs}}


def _linear(d, shift=0):
    """negative weights and exact zeros (both signs of zero); the others are no dyadic fractions, so that the order of the sum
    and a fused multiply-add would show in the scores' last bits"""
    w = [(-0.7, -1.0 / 3.0, 0.0, 0.1, 0.45)[(7 * j + shift) % 5] for j in range(d)]
    if d > 3:
        w[3] = -0.0
    return {"Linear": {"weights": w}}


def _forest7(d, A, B, C, E):
    """depth <= 4, unequal weights; A in every tree, B only in the first, C only in the last; splits that equal data values
    (the columns hold -3 .. 3); a node on feature d + 3, which no row holds (reads 0.0)"""
    t = [_split(A, 1.0, _split(B, 0.0, _leaf(0.3), _leaf(-1.7)), _split(E, -1.0, _leaf(2.2), _split(d + 3, 0.5, _leaf(0.9), _leaf(-5.0))))]
    for k in range(1, 6):
        t.append(_split(A, k - 3.0, _split(E, 0.5 * k - 1.0, _leaf(0.1 * k), _split(A, -2.0, _leaf(1.0 / k), _split(E, 2.0, _leaf(-0.7), _leaf(0.37 * k)))),
                        _leaf(-0.11 * k)))
    t.append(_split(C, 0.0, _split(A, -1.0, _leaf(0.77), _leaf(-0.21)), _leaf(1.3)))
    return {"Ensemble": {"weights": [0.5, -1.25, 2.0, 0.75, 1.5, -0.3, 1.0], "models": [{"DecisionTree": x} for x in t]}}


def _random_tree(rng, feats, depth):
    if depth == 0 or rng.random() < 0.15:
        return _leaf(rng.normal())
    return _split(rng.choice(feats), float(rng.integers(-3, 4)) + (0.5 if rng.random() < 0.5 else 0.0), _random_tree(rng, feats, depth - 1),
                  _random_tree(rng, feats, depth - 1))


def _forest70(feats):
    rng = np.random.default_rng(70)
    return {"Ensemble": {"weights": [float(w) for w in rng.normal(size=70)], "models": [{"DecisionTree": _random_tree(rng, feats, 3)} for _ in range(70)]}}


_ORACLE = {}


def _oracle(key, X, y, qid, ids, model, evaluator, f, r, scope, qrel, seed=SEED):
    """{query id: value} of `model` on D_{f,r}, through from_numpy and evaluate_dense; computed once per key"""
    k = (key, evaluator, f, r, scope, seed)
    if k not in _ORACLE:
        src = pm.sources(ids, seed, r, scope, qid[ids])
        Xp = pm.permuted_matrix(X, ids, src, f)
        other = fr.CDataset.from_numpy(np.ascontiguousarray(Xp[ids]), np.ascontiguousarray(y[ids]), np.ascontiguousarray(qid[ids]))
        qids, vals = native.evaluate_dense(model, other, evaluator, qrel)
        _ORACLE[k] = dict(zip(qids, vals))
    return _ORACLE[k]


def _check(key, d, view, ids, model_json, evaluator, feats, R=2, scope="dataset", qrel=None, oracle_pairs=None, **kw):
    """Runs the call on `view` (whose instance ids are `ids`, ascending) and holds everything it returns to the oracle;
    oracle_pairs: the (index into feats, repeat) pairs to check (default: all)."""
    X, y, qid = _data(d)
    model = fr.CModel.from_dict(model_json)
    rep, values, pq = native.permutation_importance_dense(model, view, evaluator, qrel=qrel, repeats=R, seed=SEED, scope=scope, features=feats, **kw)
    qids, base = native.evaluate_dense(model, view, evaluator, qrel)
    assert rep["features"] == list(feats) and rep["repeats"] == R and rep["seed"] == SEED and rep["scope"] == scope and rep["queries"] == len(qids)
    assert values.shape == (len(feats), R) and pq.shape == (len(feats) * R + 1, len(qids))
    assert _same(pq[-1], base) and _same(rep["baseline"], rm.means(base[:, None])[0])
    pairs = oracle_pairs if oracle_pairs is not None else [(fi, r) for fi in range(len(feats)) for r in range(R)]
    for fi, r in pairs:
        want = _oracle(key, X, y, qid, ids, model, evaluator, feats[fi], r, scope, qrel)
        want = np.array([want[q] for q in qids])
        row = pq[fi * R + r]
        print(key, evaluator, scope, "feature", feats[fi], "repeat", r, "queries that differ from the oracle:", int((_bits(row) != _bits(want)).sum()),
              "that differ from the baseline:", int((_bits(row) != _bits(base)).sum()))
        assert _same(row, want)
        assert _same(values[fi, r], rm.means(want[:, None])[0])
    for fi in range(len(feats)):
        imp, std = pm.report(rep["baseline"], values[fi])
        assert _same(rep["importance"][fi], imp) and _same(rep["std"][fi], std)
        if feats[fi] in rep["skipped"]:
            assert _same(values[fi], [rep["baseline"]] * R) and _bits(rep["importance"][fi]) == 0 and _bits(rep["std"][fi]) == 0
            for r in range(R):
                assert _same(pq[fi * R + r], base)
    return rep, values, pq


def _all_ids(d):
    return np.arange(sum(QLENS))


# ---- models, measures, scopes -------------------------------------------------------------------------------------------


@pytest.mark.parametrize("d", DIMS)
def test_linear_under_ndcg_at_10(d):
    feats = _listed(d)
    rep, values, pq = _check(("linear", d), d, _dataset(d), _all_ids(d), _linear(d), "ndcg@10", feats)
    w = _linear(d)["Linear"]["weights"]
    assert rep["skipped"] == [f for f in feats if w[f] == 0.0] and rep["stats"]["gather"] == "xcol" and rep["stats"]["rows"] == "lds"
    assert rep["stats"]["launches"] == {"linear": 1, "single": 0, "trees": 0, "axpy": 0} and rep["stats"]["chunks"] == 1
    used = [fi for fi, f in enumerate(feats) if w[f] != 0.0]
    assert used and all(not _same(pq[fi * 2], pq[-1]) for fi in used)  # shuffling a used column moves some query


@pytest.mark.parametrize("scope", ["dataset", "query"])
def test_linear_under_full_ndcg_in_both_scopes(scope):
    _check(("linear", 9), 9, _dataset(9), _all_ids(9), _linear(9), "ndcg", [8, 0, 5], scope=scope)  # (features in the order asked for)


@pytest.mark.parametrize("fid, skip", [(2, True), (4, False), (11, False)])
def test_single_feature_under_map(fid, skip):
    """on a listed feature, on another one (launched for all the same with skip_unused off), and on one no row holds"""
    rep, values, pq = _check(("single", fid), 5, _dataset(5), _all_ids(5), {"SingleFeature": {"fid": fid, "dir": -1.5}}, "map", [0, 2], skip_unused=skip)
    assert rep["skipped"] == ([0] if skip else []) and rep["stats"]["launches"]["single"] == 1
    assert _same(pq[0], pq[-1]) and _same(pq[2], pq[-1]) == (fid != 2)


@pytest.mark.parametrize("scope", ["dataset", "query"])
def test_one_decision_tree_under_mrr(scope):
    tree = _split(1, 0.0, _split(0, 1.0, _leaf(0.25), _split(4, -1.0, _leaf(-3.0), _leaf(0.7))), _split(1, 2.0, _leaf(1.1), _leaf(0.4)))
    rep, _, _ = _check(("tree", 5), 5, _dataset(5), _all_ids(5), {"DecisionTree": tree}, "mrr", [0, 1, 2, 3, 4], scope=scope)
    assert rep["skipped"] == [2, 3] and rep["stats"]["launches"]["trees"] == 1


@pytest.mark.parametrize("d, roles", [(5, (0, 1, 2, 4)), (9, (7, 1, 2, 4)), (136, (0, 4, 67, 135))])
def test_seven_trees_under_full_ndcg(d, roles):
    feats = _listed(d)
    rep, values, pq = _check(("forest7", d), d, _dataset(d), _all_ids(d), _forest7(d, *roles), "ndcg", feats)
    assert rep["skipped"] == [f for f in feats if f not in roles]
    assert all(not _same(pq[feats.index(f) * 2], pq[-1]) for f in roles)


def test_seven_trees_inside_queries_under_ndcg_at_10():
    _check(("forest7", 9), 9, _dataset(9), _all_ids(9), _forest7(9, 7, 1, 2, 4), "ndcg@10", [7, 1, 2, 4], scope="query")


def test_seventy_trees():
    _check(("forest70", 9), 9, _dataset(9), _all_ids(9), _forest70([0, 2, 3, 5, 8, 12]), "ndcg@10", [0, 3, 8, 1], scope="query")


def _two_linear(d):
    return {"Ensemble": {"weights": [0.75, -1.5], "models": [_linear(d), _linear(d, 3)]}}


def test_an_ensemble_of_two_linear_models_under_mrr():
    rep, _, _ = _check(("two-linear", 9), 9, _dataset(9), _all_ids(9), _two_linear(9), "mrr", [0, 1, 3, 6])
    assert rep["stats"]["launches"] == {"linear": 2, "single": 0, "trees": 0, "axpy": 2} and rep["skipped"] == [3]


def test_an_ensemble_of_linear_and_single_feature_members():
    model = {"Ensemble": {"weights": [1.25, 0.5, 2.0], "models": [_linear(5), {"SingleFeature": {"fid": 1, "dir": -0.3}}, {"SingleFeature": {"fid": 3, "dir": 1.0}}]}}
    rep, _, _ = _check(("linear+single", 5), 5, _dataset(5), _all_ids(5), model, "ndcg@10", [1, 3, 2])
    assert rep["skipped"] == [] and rep["stats"]["launches"]["axpy"] == 3


def test_map_with_judgments_from_a_qrel():
    X, y, qid = _data(5)
    judged = {}
    for q in (3, 9, 10, 22):  # more relevant documents than the dataset holds for these queries: AP's denominators change
        judged[str(q)] = {"doc%d" % k: 1.0 + (k % 2) for k in range(int((qid == q).sum()) + 7)}
    qrel = fr.CQRel.from_dict(judged)
    model = fr.CModel.from_dict(_linear(5))
    _, plain = native.evaluate_dense(model, _dataset(5), "map")
    _, with_qrel = native.evaluate_dense(model, _dataset(5), "map", qrel)
    assert not _same(plain, with_qrel)
    _check(("linear-qrel", 5), 5, _dataset(5), _all_ids(5), _linear(5), "map", [0, 4], qrel=qrel)


# ---- views and layouts -------------------------------------------------------------------------------------------------


def test_a_query_sampled_view():
    X, y, qid = _data(9)
    chosen = [1, 4, 9, 10, 12, 20]  # lengths 1, 64, 300, 800, 1, 256
    view = _dataset(9).subsample_queries([str(q) for q in chosen])
    ids = np.flatnonzero(np.isin(qid, chosen))
    for scope in ("dataset", "query"):
        _check(("qview-linear", 9), 9, view, ids, _linear(9), "ndcg@10", [0, 5], scope=scope)
    _check(("qview-forest7", 9), 9, view, ids, _forest7(9, 7, 1, 2, 4), "map", [7, 2])
    # the parent gives afterwards what it gave before
    _check(("linear", 9), 9, _dataset(9), _all_ids(9), _linear(9), "ndcg@10", [0, 5])


def test_a_feature_sampled_view_lists_its_own_features_and_scores_all_columns():
    view = _dataset(9).subsample_feature_names(["0", "5", "7"])
    model = fr.CModel.from_dict(_linear(9))
    rep, values, pq = native.permutation_importance_dense(model, view, "ndcg@10", repeats=2, seed=SEED)
    assert rep["features"] == [0, 5, 7] and rep["names"] == ["0", "5", "7"]
    rep2, values2, pq2 = _check(("linear", 9), 9, view, _all_ids(9), _linear(9), "ndcg@10", [0, 5, 7])
    assert _same(values, values2) and _same(pq, pq2)


def test_gathering_from_the_tiles_gives_the_same_bytes(monkeypatch):
    monkeypatch.setenv("FR_XCOL", "0")
    tiles_only = {d: fr.CDataset.from_numpy(*_data(d)) for d in (5, 9)}
    for ds in tiles_only.values():
        assert native.device_form(ds)["xcol"] is None  # (the device form is built here, under the switch)
    monkeypatch.delenv("FR_XCOL")
    for key, d, model, evaluator, feats in ((("linear", 9), 9, _linear(9), "ndcg@10", [0, 5, 8]), (("forest7", 9), 9, _forest7(9, 7, 1, 2, 4), "ndcg", [7, 1, 2]),
                                            (("single", 2), 5, {"SingleFeature": {"fid": 2, "dir": -1.5}}, "map", [2])):
        rep, values, pq = _check(key, d, tiles_only[d], _all_ids(d), model, evaluator, feats)
        rep_x, values_x, pq_x = native.permutation_importance_dense(fr.CModel.from_dict(model), _dataset(d), evaluator, repeats=2, seed=SEED, features=feats)
        assert rep["stats"]["gather"] == "tiles" and rep_x["stats"]["gather"] == "xcol"
        assert _same(values, values_x) and _same(pq, pq_x)


def test_rows_too_wide_for_lds_are_read_from_the_tiles():
    """d = 640: 64 (4 * 160 + 1) 4 bytes = 164 096 do not fit; both kernels read the document's own row from global memory"""
    d = 640
    feats = [0, 5, 639]
    rep, _, _ = _check(("linear", d), d, _dataset(d), _all_ids(d), _linear(d), "ndcg@10", feats, oracle_pairs=[(0, 0), (1, 1), (2, 0), (2, 1)])
    assert rep["stats"]["rows"] == "global"
    rep, _, _ = _check(("forest7", d), d, _dataset(d), _all_ids(d), _forest7(d, 639, 5, 0, 320), "ndcg@10", feats, oracle_pairs=[(0, 1), (1, 0), (2, 0), (2, 1)])
    assert rep["stats"]["rows"] == "global" and rep["skipped"] == []


# ---- knobs -------------------------------------------------------------------------------------------------------------


MODELS_9 = [("linear", lambda: _linear(9), "ndcg@10"), ("forest7", lambda: _forest7(9, 7, 1, 2, 4), "ndcg"), ("two-linear", lambda: _two_linear(9), "mrr"),
            ("single", lambda: {"SingleFeature": {"fid": 5, "dir": 2.0}}, "map")]


def _run(model_json, evaluator, **kw):
    kw.setdefault("repeats", 2)
    kw.setdefault("features", [7, 1, 5, 3, 0])
    return native.permutation_importance_dense(fr.CModel.from_dict(model_json), _dataset(9), evaluator, seed=SEED, **kw)


@pytest.mark.parametrize("name, make, evaluator", MODELS_9)
def test_three_slots_per_launch_take_several_chunks_and_give_the_same_bytes(name, make, evaluator):
    rep, values, pq = _run(make(), evaluator, skip_unused=False)
    rep3, values3, pq3 = _run(make(), evaluator, skip_unused=False, max_slots=3)
    assert rep["stats"]["chunks"] == 1 and rep["stats"]["slots"] == 10
    assert rep3["stats"]["chunks"] == 5 and rep3["stats"]["slots"] == 2  # one feature's two repeats stay together
    assert _same(values, values3) and _same(pq, pq3)
    assert {k: v for k, v in rep.items() if k != "stats"} == {k: v for k, v in rep3.items() if k != "stats"}
    rep5, values5, pq5 = _run(make(), evaluator, skip_unused=False, max_slots=5)
    assert rep5["stats"]["chunks"] == 3 and rep5["stats"]["slots"] == 4 and _same(values, values5) and _same(pq, pq5)


@pytest.mark.parametrize("name, make, evaluator", MODELS_9)
def test_skipping_unused_features_changes_no_byte(name, make, evaluator):
    on = _run(make(), evaluator)
    off = _run(make(), evaluator, skip_unused=False)
    assert _same(on[1], off[1]) and _same(on[2], off[2]) and off[0]["skipped"] == []
    assert on[0]["importance"] == off[0]["importance"] and on[0]["std"] == off[0]["std"]
    expected = {"linear": [1, 3], "forest7": [5, 3, 0], "two-linear": [3], "single": [7, 1, 3, 0]}[name]
    assert on[0]["skipped"] == expected
    feats = [7, 1, 5, 3, 0]
    for f in expected:
        fi = feats.index(f)
        assert _bits(on[0]["importance"][fi]) == 0 and _bits(on[0]["std"][fi]) == 0 and _same(on[1][fi], [on[0]["baseline"]] * 2)


@pytest.mark.parametrize("name, make, evaluator", MODELS_9)
def test_nine_repeats_cross_the_eight_accumulators(name, make, evaluator):
    """R = 9 takes two launches per kernel; its first two repeats are the R = 2 run's, and repeat 8 -- alone in the second
    launch -- is the oracle's"""
    feats = [5, 1] if name != "forest7" else [7, 1]
    two = _run(make(), evaluator, features=feats)
    rep, values, pq = _check((name + "-r9", 9), 9, _dataset(9), _all_ids(9), make(), evaluator, feats, R=9, oracle_pairs=[(0, 8), (1, 8), (0, 7)])
    assert _same(values[:, :2], two[1])
    for fi in range(2):
        for r in range(2):
            assert _same(pq[fi * 9 + r], two[2][fi * 2 + r])
    launches = rep["stats"]["launches"]
    assert launches[{"linear": "linear", "forest7": "trees", "two-linear": "linear", "single": "single"}[name]] == {"two-linear": 4, "single": 1}.get(name, 2)
    one = _run(make(), evaluator, features=feats, repeats=1)
    assert _same(one[1][:, 0], two[1][:, 0]) and one[0]["std"] == [0.0, 0.0]


# ---- determinism and isolation ------------------------------------------------------------------------------------------


def test_the_same_call_gives_the_same_bytes_and_leaves_the_dataset_as_it_was():
    ds = _dataset(9)
    linear, forest = fr.CModel.from_dict(_linear(9)), fr.CModel.from_dict(_forest7(9, 7, 1, 2, 4))
    before = {m: native.evaluate_dense(m, ds, "ndcg@10")[1] for m in (linear, forest)}
    scores_before = native.predict_scores_dense(forest, ds)
    form_before = native.device_form(ds)
    runs = [_run(_forest7(9, 7, 1, 2, 4), "ndcg@10", repeats=3, scope="query") for _ in range(2)] + [_run(_two_linear(9), "ndcg@10") for _ in range(2)]
    for a, b in (runs[:2], runs[2:]):
        assert json.dumps({k: v for k, v in a[0].items() if k != "stats"}, sort_keys=True) == json.dumps({k: v for k, v in b[0].items() if k != "stats"}, sort_keys=True)
        assert _same(a[1], b[1]) and _same(a[2], b[2])
    for m in (linear, forest):
        assert _same(native.evaluate_dense(m, ds, "ndcg@10")[1], before[m])
    assert _same(native.predict_scores_dense(forest, ds), scores_before)
    form_after = native.device_form(ds)
    for name in TABLES:
        a, b = form_before[name], form_after[name]
        assert (a is None and b is None) or (a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()), name
    assert not _same(_run(_linear(9), "ndcg@10")[1], native.permutation_importance_dense(linear, ds, "ndcg@10", repeats=2, seed=SEED + 1, features=[7, 1, 5, 3, 0])[1])


def test_the_public_call_names_features_and_ranks_them():
    ds = _dataset(9)
    model = fr.CModel.from_dict(_linear(9))
    rep = fr.permutation_importance(ds, model, "ndcg@10", repeats=2, seed=SEED, features=["7", "1", "5", "3", "0"])
    raw, values, _ = _run(_linear(9), "ndcg@10")
    assert list(rep["features"]) == ["7", "1", "5", "3", "0"] and rep["skipped"] == ["1", "3"] and rep["baseline"] == raw["baseline"]
    for k, name in enumerate(rep["features"]):
        assert rep["features"][name] == {"importance": raw["importance"][k], "std": raw["std"][k], "values": list(values[k])}
    order = sorted(range(5), key=lambda k: (-raw["importance"][k], raw["features"][k]))
    assert rep["ranking"] == [raw["names"][k] for k in order]
    assert model.permutation_importance(ds, "ndcg@10", repeats=2, seed=SEED, features=["7", "1", "5", "3", "0"])["features"] == rep["features"]
    everything = fr.permutation_importance(ds, model, "ndcg@10", repeats=1)
    assert list(everything["features"]) == [str(j) for j in range(9)] and everything["repeats"] == 1 and everything["scope"] == "dataset"


# ---- errors and the bundled example -------------------------------------------------------------------------------------


def test_a_refused_shape_and_a_nan_score():
    ds = _dataset(5)
    tree = {"DecisionTree": _split(0, 0.5, _leaf(0.0), _leaf(1.0))}
    mixed = fr.CModel.from_dict({"Ensemble": {"weights": [1.0, 1.0], "models": [_linear(5), tree]}})
    with pytest.raises(Exception, match=r"an Ensemble of Linear / SingleFeature models, not Ensemble\[Linear, DecisionTree\]"):
        native.permutation_importance_dense(mixed, ds, "ndcg@10")
    # (the model format cannot carry a NaN weight: these two make +inf - inf)
    nan = fr.CModel.from_dict({"Linear": {"weights": [1e308, -1e308, 0.0, 0.0, 0.0]}})
    with pytest.raises(Exception, match="Model.predict -> NaN"):
        native.permutation_importance_dense(nan, ds, "ndcg@10")
    with pytest.raises(Exception, match="Invalid training measure"):
        native.permutation_importance_dense(fr.CModel.from_dict(_linear(5)), ds, "ndgc")


def test_the_bundled_example_with_a_fixed_weight_vector(trec):
    X, y, qid = trec["train_X"], trec["train_y"], trec["train_qid"]
    ds = fr.CDataset.from_numpy(X, y, qid)
    model = fr.CModel.from_dict({"Linear": {"weights": [0.5, -0.25, 0.0, 1.0, 0.125, -1.0]}})
    rep = fr.permutation_importance(ds, model, "ndcg@10", repeats=3, seed=1)
    names = list(rep["features"])
    assert len(names) == 6 and rep["skipped"] == [names[2]]
    zero = rep["features"][names[2]]
    assert _bits(zero["importance"]) == 0 and _bits(zero["std"]) == 0 and zero["values"] == [rep["baseline"]] * 3
    off, values, _ = native.permutation_importance_dense(model, ds, "ndcg@10", repeats=3, seed=1, skip_unused=False)
    assert off["skipped"] == [] and _bits(off["importance"][2]) == 0 and _same(values[2], [rep["baseline"]] * 3)
    assert [rep["features"][n]["importance"] for n in names] == off["importance"]
    assert rep["baseline"] == float(rm.means(native.evaluate_dense(model, ds, "ndcg@10")[1][:, None])[0])
