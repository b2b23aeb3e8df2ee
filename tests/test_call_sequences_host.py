"""The call catalogue (tests/call_catalogue.py) checked without a device: it imports, it holds every family the
call-sequence tests promise with the large / small variants, names are unique, every request serialises, the pair
enumeration is complete and the walks are a pure function of their seed."""
import json

import numpy as np

from tests import call_catalogue as cc


def test_the_catalogue_holds_every_family_with_its_variants():
    print("%d ops:" % len(cc.NAMES))
    for family in cc.REQUIRED:
        print("  %s: %s" % (family, ", ".join(n for n in cc.NAMES if cc.OPS[n].family == family)))
    assert len(set(cc.NAMES)) == len(cc.NAMES) == len(cc.OPS)
    assert {o.family for o in cc.OPS.values()} == set(cc.REQUIRED)
    for family, names in cc.REQUIRED.items():
        for name in names:
            assert name in cc.OPS and cc.OPS[name].family == family, (family, name)
    for large, small in cc.LARGE_SMALL:
        assert cc.OPS[large].size == "large" and cc.OPS[small].size == "small", (large, small)
        assert cc.OPS[large].handles == cc.OPS[small].handles
    for o in cc.OPS.values():
        assert o.handles and set(o.handles) <= {"parent", "qview", "fview", "sibling"}, o.name
        assert (o.family == "refusals") == o.refusal, o.name
    # the same call on the parent and on a view is two ops
    for name in ("score_forest_rank_70", "eval_ndcg@10", "lm_hist_k16", "explain", "feature_stats"):
        assert cc.OPS[name].handles == ("parent",) and cc.OPS[name + "@qview"].handles == ("qview",)
    # the forests name the path they are built for; the cache-hit forest is its first appearance's model
    assert {cc.OPS[n].plan for n in cc.NAMES if n.startswith("score_forest")} == {"rank", "lds", "l2"}
    a, b = cc.model_dict("forest_rank_70"), cc.model_dict("forest_rank_70_ulp")
    wa, wb = a["Ensemble"]["weights"], b["Ensemble"]["weights"]
    assert a["Ensemble"]["models"] == b["Ensemble"]["models"] and [i for i in range(70) if wa[i] != wb[i]] == [17]
    assert wb[17] == np.nextafter(wa[17], np.inf)
    assert len(cc.model_dict("forest_rank_2")["Ensemble"]["models"]) == 2
    # the stepped trainer's parts chain
    p = cc.STEPPED_PARTS
    assert [cc.OPS[n].after for n in p] == [None, p[0], p[1]]


def test_the_dataset_is_the_one_the_stateful_paths_need():
    X, y, qid = cc.arrays("parent")
    assert X.shape[1] == 7 and X.dtype == np.float32
    lens = np.bincount(qid)[1:]
    assert len(lens) == 40 and set(cc.SPECIAL_LENS) <= set(lens.tolist()) and lens[cc.LONG_QUERY - 1] == 8193
    assert np.any(np.diff(qid) < 0)  # rows interleaved
    zeros = X[:, 0][X[:, 0] == 0]
    assert np.signbit(zeros).any() and not np.signbit(zeros).all()
    assert set(np.unique(y)) == {0.0, 1.0, 2.0, 3.0, 4.0}
    assert len(np.unique(X[:, 6])) > len(y) // 2 and all(len(np.unique(X[:, j])) <= 8 for j in range(6))
    view = cc.view_queries()
    assert str(cc.LONG_QUERY) not in view and {"1", "2", "8"} <= set(view) and 25 < len(view) < 39
    Xs, ys, qs = cc.arrays("sibling")
    assert 500 <= len(ys) <= 700 and Xs.shape[1] == 7
    assert cc.arrays("parent")[0] is X
    held = cc.HELD_OUT
    assert len(held["a"]) == len(held["b"]) and not set(held["a"]) & set(held["b"])
    assert set(held["a"] + held["b"]) <= set(view)
    qa, qb = cc.QRELS["a"], cc.QRELS["b"]
    assert set(qa) == set(qb) and qa != qb


def test_every_request_serialises():
    count = 0
    for o in cc.OPS.values():
        if o.request is None:
            continue
        wire = o.request().to_dict()
        assert json.loads(json.dumps(wire)) == wire, o.name
        assert cc.fr.TrainRequest.from_dict(wire).to_dict() == wire, o.name
        count += 1
    assert count >= 30
    cc.model_dict("linear")
    for name in list(cc._MODELS):
        assert json.loads(json.dumps(cc.model_dict(name))) == cc.model_dict(name)


def test_canonical_bytes_tell_bits_apart():
    c = cc.canon
    assert c(0.0) != c(-0.0) and c(1) != c(1.0) and c([1, 2]) != c([12])
    assert c({"b": 1, "a": 2}) == c({"a": 2, "b": 1})
    a = np.arange(6, dtype=np.float64)
    assert c(a) != c(a.reshape(2, 3)) and c(a) != c(a.astype(np.float32)) and c(a) == c(a.copy())
    nan1 = np.array([np.nan])
    nan2 = nan1.view(np.uint64) + 1
    assert c(nan1) != c(nan2.view(np.float64))


def test_the_pair_enumeration_is_complete():
    pairs = cc.pairs()
    n = len(cc.NAMES)
    assert len(pairs) == n * n == len(set(pairs))
    assert {a for a, _ in pairs} == set(cc.NAMES) == {b for _, b in pairs}
    assert all((a, a) in set(pairs) for a in cc.NAMES)


def test_walks_are_a_pure_function_of_their_seed():
    for seed in range(8):
        w = cc.walk(seed)
        assert w == cc.walk(seed) and len(w) == 60
        assert w != cc.walk(seed + 100)
        # the stepped trainer's parts come once each, in order, with other steps between some of them
        where = [w.index(p) for p in cc.STEPPED_PARTS]
        assert where == sorted(where) and all(w.count(p) == 1 for p in cc.STEPPED_PARTS)
    assert any(cc.walk(s).index(cc.STEPPED_PARTS[2]) - cc.walk(s).index(cc.STEPPED_PARTS[0]) > 2 for s in range(8))
    steps = [s for seed in range(8) for s in cc.walk(seed)]
    assert "@remake_views" in steps and "@release_replicas" in steps
    assert all(p in steps for p in cc.STEPPED_PARTS)
    for handles in (("parent",), ("qview", "sibling"), ("fview",)):
        w = cc.walk(3, 40, handles)
        assert all(s.startswith("@") or set(cc.OPS[s].handles) <= set(handles) for s in w)
