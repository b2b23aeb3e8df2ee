"""Every value a training's line searches publish, and every resident sum they leave, against the oracle.

The resident bound-and-verify kernels (linesearch_verify_kernel<K, 1, true, XS, DUP>, the resident paths of
fullrank_verify_kernel and rr_verify_kernel) run only inside a trainer, and the training tests compare trajectories: a wrong
value on a candidate that does not win is invisible to them.  Here a CoordinateAscentRun runs with the tick capture on
(native.CoordinateAscentRun.capture) and tests/linesearch_tick_model.py rebuilds, from the oracle alone, the whole per-query
matrix, the means and the resident sums of every line search; the capture also says which instantiation ran and which
(query, group) pairs the verify kernel decided itself.

Shapes: at most 40 queries, 3000 documents, 8 features; the query lengths are the edges of the lists (1, 2, K - 1 .. K + XS
+ 1 for every depth and list length used: every length from 1 to 26), of the walk tile (127, 128, 129, 257, 300) and, for
the full-ranking kernels, of every size class that fits (16 / 17, 32 / 33, ... 256 / 257).
"""
import os

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import native
from oracle import pyoracle as o
from tests.linesearch_tick_model import TickModel, check_log

pytestmark = pytest.mark.gpu

TOPK_LENS = list(range(1, 27)) + [127, 128, 129, 257, 300]
FV_LENS = [1, 2, 20, 21, 22, 50, 51, 127, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 128, 129, 160, 161, 192, 193, 256, 257, 300]
KINDS = ("continuous", "same_label", "mixed_label")
# The queries that carry duplicated documents, by length: 7 of the 31 (29) queries.  A tie at the cut that the list length in
# use cannot decide sends the (query, group) pair to the exact kernel, and a line search with more than a quarter of a
# restart's pairs redone sends that restart's next line searches (full ranking: everybody's next 16) there whole.  With
# continuous columns hardly anything but duplicates ties, so a group seldom has more than 7 pairs redone -- 4 * 7 <= 29 --
# and the exact kernels take few line searches whole, whatever the depth, the list length and the weights are (with
# duplicates in every query the depth-1 case at K + 1 keys had 47 % of its pairs verified, under the half required).
TOPK_DUP_LENS = (300, 257, 129, 128, 127, 21, 11)
FV_DUP_LENS = (300, 257, 256, 193, 129, 22, 17)


def _verify_path_on(resident_needed=False):
    """False when the environment forces another bit-exact path (the suite is also run under FR_LS_EXACT=1 and
    FR_LS_RESIDENT=0 as an A/B check): the values must not change, only the path assertions do not apply."""
    if os.environ.get("FR_LS_EXACT"):
        return False
    if resident_needed and os.environ.get("FR_LS_RESIDENT", "1")[:1] == "0":
        return False
    return True


def _make(kind, seed, lens, d, frac=0.06, dup_lens=None):
    """Continuous columns (no coincidental ties) with label signal; `same_label`: some documents copy their predecessor's row
    and label (ties inside one gain class); `mixed_label`: non-negative columns, the row alone is copied (ties between gain
    classes, decided by the duplicate groups).  dup_lens: only queries of these lengths get copies (None: every query); the
    short ones among them at five times the rate, so that they have some."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens)[rng.permutation(len(lens))]
    n = int(lens.sum())
    qid = np.repeat(np.arange(1, len(lens) + 1, dtype=np.int64), lens)
    y = rng.choice(5, size=n, p=[0.4, 0.3, 0.2, 0.07, 0.03]).astype(np.float64)
    X = rng.normal(0.0, 1.0, (n, d))
    X[:, 1] = rng.lognormal(0.0, 1.0, n)
    X[:, 0] += 0.5 * y
    X[:, 3] -= 0.3 * y
    if kind == "mixed_label":
        X = np.abs(X)
    X = X.astype(np.float32)
    if kind != "continuous":
        qlen = lens[qid - 1]
        rate = frac if dup_lens is None else np.where(np.isin(qlen, dup_lens), np.where(qlen < 64, 5 * frac, frac), 0.0)
        for i in np.nonzero(rng.random(n) < rate)[0]:
            if i > 0 and qid[i - 1] == qid[i]:
                X[i] = X[i - 1]
                if kind == "same_label":
                    y[i] = y[i - 1]
    return X, y, qid


def _fv_classes(lens):
    """The (keys per lane, lanes per candidate) class the library sorts a query of each length in (fr_debug_fullrank_class)."""
    from fastrank_amd import clib

    out = set()
    for n in lens:
        v = int(clib._load().fr_debug_fullrank_class(int(n)))
        out.add((v >> 16, v & 0xFFFF))
    return out


_DATA = {}


def _data(kind, lens_name="topk", frac=0.06, no_dup_groups=False):
    """(X, y, qid, a device dataset of the caller's own, model) of one data kind.  The arrays and the model are made once:
    the model's cache of oracle columns is shared by every run on the data (the pins of one depth follow one trajectory).
    The device dataset is new at every call: the list length and the back-off its trainers arrived at live in it, and a
    test's share of verified pairs must not depend on the tests before it.  (The position map is the layout's alone: the
    same for every dataset of these arrays, with or without duplicate groups.)"""
    key = (kind, lens_name, frac, no_dup_groups)
    if key not in _DATA:
        lens, d = (TOPK_LENS, 6) if lens_name == "topk" else (FV_LENS, 5)
        dup_lens = None if no_dup_groups else (TOPK_DUP_LENS if lens_name == "topk" else FV_DUP_LENS)   # (the routing case ties everywhere)
        X, y, qid = _make(kind, 11 + KINDS.index(kind), lens, d, frac, dup_lens)
        assert len(lens) <= 40 and len(y) <= 3000
        perm = native.device_form(fr.CDataset.from_numpy(X, y, qid))["perm"]
        _DATA[key] = (X, y, qid, TickModel(X, y, qid, perm))
    X, y, qid, model = _DATA[key]
    return X, y, qid, fr.CDataset.from_numpy(X, y, qid), model


def _request(measure, kind, restarts=2, iters=4, seed=5, **kw):
    req = fr.TrainRequest.coordinate_ascent()
    req.measure = measure
    p = req.params
    p.seed, p.quiet, p.num_restarts, p.num_max_iterations = seed, True, restarts, iters
    p.init_random = kind != "mixed_label"   # (uniform positive start weights: the duplicate groups are used)
    for k, v in kw.items():
        setattr(p, k, v)
    return req


def _run(g, model, req, capture=True, chunk=64):
    run = native.CoordinateAscentRun(g, req)
    if capture:
        run.capture(True)
    while not run.finished:
        run.step(chunk)
    log = run.take_capture() if capture else []
    st = run.state()
    run.close()
    tot = None
    if capture:
        model.reset()
        tot = check_log(model, log)
        print("capture:", {k: (sorted(v) if isinstance(v, set) else v) for k, v in tot.items()},
              "updates in verify launches / by resident_update_kernel:", model.updates_in_verify, model.updates_by_kernel)
        for ev in log:
            if ev["type"] == "tick" and ev["matrix"] is None:
                assert ev["ready"]
    return log, st, tot


def _oracle_restarts(model, req, st, fids=None):
    exp_s, exp_w, exp_e, err = model.ds.ca_learn(req.measure, req.params.to_dict(), fids=fids, threads=2)
    assert err == 0
    for r in st["restarts"]:
        assert r["score"] == exp_s[r["restart_id"]] and r["weights"] == exp_w[r["restart_id"]].tolist()
    assert st["stats"]["useful_evals"] == int(exp_e.sum())


def _mostly_verified(tot, resident_needed=True):
    """The condition of every case not built to tie: at least half of ALL (query, group) pairs of the run were decided by
    the verify kernel -- not recomputed from the redo list, not evaluated by the exact kernels alone."""
    if _verify_path_on(resident_needed):
        assert tot["ticks"] > 0 and tot["unreplayed"] == 0
        assert 2 * tot["verified"] >= tot["pairs"], tot


def _ticks(log):
    return [ev for ev in log if ev["type"] == "tick"]


# ---- 1. top-k: depth x list length x data ------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 2, 4, 5, 6, 9, 10, 11, 15, 19, 20])
@pytest.mark.parametrize("kind", KINDS)
def test_topk_values_at_every_depth_and_list_length(kind, depth, monkeypatch):
    X, y, qid, g, model = _data(kind)
    req = _request("ndcg@%d" % depth, kind)
    first = None
    for pin in (1, 2, 3, 4):
        monkeypatch.setenv("FR_VERIFY_XS", str(pin))
        log, st, tot = _run(g, model, req)
        if first is None:
            first = st["restarts"]
            _oracle_restarts(model, req, st)
        assert st["restarts"] == first
        _mostly_verified(tot)
        if _verify_path_on(resident_needed=True):
            verified = [t for t in _ticks(log) if t["approx"]]
            assert verified
            for t in verified:
                assert t["kind"] == "topk" and t["resident"]
                assert t["inst"]["k"] == (5 if depth <= 5 else 10 if depth <= 10 else 20)
                assert t["inst"]["xs_pinned"] and t["inst"]["xs_used"] == min(pin, 3 if depth <= 5 else 4)   # verify_xs_cap
                assert t["inst"]["dup"] == (kind == "mixed_label")


# ---- 2. pending updates: inside the verify launch, and by resident_update_kernel --------------------------------------
def _accepts_per_slot(log):
    n = {}
    for t in _ticks(log):
        seen = set()
        for grp in t["groups"]:
            if grp["has_update"] and grp["resident_slot"] not in seen:
                seen.add(grp["resident_slot"])
                n[grp["resident_slot"]] = n.get(grp["resident_slot"], 0) + 1
    return n


def test_pending_updates_applied_inside_the_verify_launch(monkeypatch):
    monkeypatch.setenv("FR_RESIDENT_REFRESH", "2")   # stores interleave with updates
    X, y, qid, g, model = _data("continuous")
    req = _request("ndcg@10", "continuous", restarts=3, iters=6, seed=9)
    log, st, tot = _run(g, model, req)
    _oracle_restarts(model, req, st)
    _mostly_verified(tot)
    if _verify_path_on(resident_needed=True):
        acc = _accepts_per_slot(log)
        assert len(acc) == 3 and min(acc.values()) >= 3, acc
        assert model.updates_in_verify > 0
        assert tot["stores"] > 3   # (the three initial ones, then a refresh after every second update)


def test_pending_updates_applied_by_the_update_kernel_when_groups_are_routed(monkeypatch):
    """Half of the documents copy their predecessor's row with a label of their own, the duplicate groups are off and the
    lists are pinned at K + 1: restarts are routed to the exact kernel one by one, whose pending updates
    resident_update_kernel applies.  Built to tie: both verified and recomputed pairs must occur."""
    monkeypatch.setenv("FR_RESIDENT_REFRESH", "2")
    monkeypatch.setenv("FR_NO_DUP_GROUPS", "1")
    monkeypatch.setenv("FR_VERIFY_XS", "1")
    X, y, qid, g, model = _data("mixed_label", frac=0.5, no_dup_groups=True)
    req = _request("ndcg@10", "continuous", restarts=3, iters=6, seed=9)
    log, st, tot = _run(g, model, req)
    _oracle_restarts(model, req, st)
    if _verify_path_on(resident_needed=True):
        assert tot["unreplayed"] == 0
        acc = _accepts_per_slot(log)
        assert len(acc) == 3 and min(acc.values()) >= 3, acc
        assert tot["verified"] > 0 and tot["redone"] > 0, tot
        # (three pipelined sets of one restart each: a routed restart's line search goes to the exact kernel whole)
        assert any(not t["approx"] and t["resident"] for t in _ticks(log)) and any(t["approx"] for t in _ticks(log))
        assert model.updates_by_kernel > 0 and model.updates_in_verify > 0
        assert not any(t["inst"]["dup"] for t in _ticks(log))


# ---- 3. not normalised; a start with a negative and a zero weight ----------------------------------------------------------
@pytest.mark.parametrize("measure", ["ndcg@10", "ndcg", "mrr"])
def test_unnormalised_weights_with_a_negative_and_a_zero_start_weight(measure):
    """normalize = False: the resident sums are never rescaled (norm = 1).  The view without feature 2 keeps that weight at
    zero for the whole run; the random start has negative weights."""
    X, y, qid, g, model = _data("continuous", "topk" if measure == "ndcg@10" else "fv")
    d = X.shape[1]
    fids = [f for f in range(d) if f != 2]
    view = g.subsample_feature_names([str(f) for f in fids])
    req = _request(measure, "continuous", restarts=2, iters=4, seed=3, normalize=False)
    log, st, tot = _run(view, model, req)
    starts = [grp["weights"] for t in _ticks(log)[:2] for grp in t["groups"]]   # (the first line search of both restarts)
    assert all(w0[2] == 0.0 and len(w0) == d for w0 in starts) and any((w0 < 0).any() for w0 in starts)
    assert all(grp["resident_norm"] == 1.0 for t in _ticks(log) for grp in t["groups"])
    _oracle_restarts(model, req, st, fids=np.asarray(fids, dtype=np.uint32))
    _mostly_verified(tot)


# ---- 4. candidate counts around the kernels' buckets -------------------------------------------------------------------
@pytest.mark.parametrize("iters", [7, 8, 15, 16, 25, 40])
def test_candidate_count_buckets(iters):
    """A line search has 1 + 2 * num_max_iterations candidates, always an odd number: 15 and 17 straddle the 16-candidate
    instantiations, 31 and 33 the second slice, 51 is the default's, and 81 gives a full group of 64 next to one of 17
    (two groups of one restart share a resident slot and a pending update)."""
    X, y, qid, g, model = _data("continuous")
    req = _request("ndcg@10", "continuous", restarts=2, iters=iters, seed=3, step_scale=1.3)
    log, st, tot = _run(g, model, req)
    sizes = {len(grp["candidates"]) for t in _ticks(log) for grp in t["groups"]}
    assert sizes == ({64, 17} if iters == 40 else {1 + 2 * iters})
    _oracle_restarts(model, req, st)
    _mostly_verified(tot)


# ---- 5. pipelined sets ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parts,measure", [("0", "ndcg@10"), ("2", "ndcg@10"), ("3", "ndcg@10"), ("4", "ndcg@10"),
                                           ("0", "mrr"), ("3", "mrr"), ("4", "mrr")])
def test_pipelined_sets_publish_the_oracles_values(parts, measure, monkeypatch):
    monkeypatch.setenv("FR_LS_PIPELINE", parts)
    monkeypatch.setenv("FR_RESIDENT_REFRESH", "3")   # exact refreshes on the main stream between pipelined ticks
    X, y, qid, g, model = _data("continuous", "topk" if measure == "ndcg@10" else "fv")
    req = _request(measure, "continuous", restarts=4, iters=4, seed=17)
    log, st, tot = _run(g, model, req, chunk=5)
    _oracle_restarts(model, req, st)
    _mostly_verified(tot)
    if _verify_path_on(resident_needed=True):
        assert len(tot["contexts"]) == max(1, int(parts)), tot["contexts"]


# ---- 6. full ranking and reciprocal rank on resident sums --------------------------------------------------------------
@pytest.mark.parametrize("measure", ["ndcg", "ndcg@21", "ndcg@50", "map", "mrr"])
@pytest.mark.parametrize("kind", KINDS)
def test_fullrank_and_reciprocal_rank_values(kind, measure):
    X, y, qid, g, model = _data(kind, "fv")
    req = _request(measure, kind, restarts=2, iters=4, seed=7)
    log, st, tot = _run(g, model, req)
    _oracle_restarts(model, req, st)
    _mostly_verified(tot)
    if _verify_path_on(resident_needed=True) and not os.environ.get("FR_FV_OFF") and not os.environ.get("FR_FORCE_GENERIC"):
        verified = [t for t in _ticks(log) if t["approx"]]
        assert verified
        for t in verified:
            assert t["resident"] and t["kind"] == ("rr" if measure == "mrr" else "fullrank")
            if measure != "mrr":   # (rr_verify_kernel has one instantiation: no size classes of its own to name, no DUP variant)
                assert {(nl, pl) for nl, pl, count in t["inst"]["classes"] if count} == _fv_classes(FV_LENS)
                assert t["inst"]["dup"] == (kind == "mixed_label")


# ---- 7. a query-sampled view ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", ["ndcg@10", "ndcg"])
def test_query_sampled_view_values(measure):
    """Every third query: the view's runs start inside the parent's tiles and its walk-tile list is used.  Expected values:
    the materialised subset's."""
    X, y, qid, g, _ = _data("continuous", "topk" if measure == "ndcg@10" else "fv")
    keep = sorted(set(qid.tolist()))[::3]
    view = g.subsample_queries([str(q) for q in keep])
    rows = np.nonzero(np.isin(qid, keep))[0]
    perm = np.asarray(native.device_form(view)["perm"], dtype=np.int64)
    index = np.full(len(y), 0xFFFFFFFF, dtype=np.int64)
    index[rows] = np.arange(len(rows))
    sub_perm = np.where(perm < len(y), index[np.minimum(perm, len(y) - 1)], 0xFFFFFFFF)
    model = TickModel(X[rows], y[rows], qid[rows], sub_perm)
    req = _request(measure, "continuous", restarts=2, iters=4, seed=5)
    log, st, tot = _run(view, model, req)
    assert native.device_info(view)["shares_parent_matrix"]
    _oracle_restarts(model, req, st)
    _mostly_verified(tot)


# ---- the capture changes nothing ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", ["ndcg@10", "map", "mrr"])
def test_capture_on_and_off_give_identical_restarts_and_statistics(measure):
    X, y, qid, _, model = _data("same_label", "topk" if measure == "ndcg@10" else "fv")
    req = _request(measure, "same_label", restarts=3, iters=4, seed=21)
    out = []
    for capture in (True, False):
        g = fr.CDataset.from_numpy(X, y, qid)   # (the list length a dataset's trainers arrived at outlives them)
        log, st, tot = _run(g, model, req, capture=capture)
        st["stats"].pop("seconds")
        out.append(st)
    assert out[0] == out[1]
