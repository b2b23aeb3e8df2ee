"""tests/linesearch_tick_model.py held to the oracle and to itself, without a device: hand-built capture logs (what
native.CoordinateAscentRun.take_capture returns) whose published values are formed here by direct oracle calls, and the
resident-sum replay against the chain tests/test_error_bound.py replays."""
import numpy as np
import pytest

from oracle import pyoracle as o
from tests import test_error_bound as teb
from tests.linesearch_tick_model import NO_DOCUMENT, TickModel, check_log, check_tick, device_mean, measure_name


def _dataset(seed, lens, d):
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens)
    n = int(lens.sum())
    qid = np.repeat(np.arange(1, len(lens) + 1, dtype=np.int64), lens)
    y = rng.choice(4, size=n).astype(np.float64)
    X = rng.normal(0.0, 1.0, (n, d)).astype(np.float32)
    X[:, 0] += (0.4 * y).astype(np.float32)
    return X, y, qid


def _perm_with_holes(rng, n):
    """A device-like position map: the instances in a shuffled order with positions that hold no document in between."""
    npos = n + 37
    perm = np.full(npos, NO_DOCUMENT, dtype=np.uint32)
    perm[np.sort(rng.choice(npos, n, replace=False))] = rng.permutation(n)
    return perm


def _group(f, base, cands, slot, norm, pend):
    g = {"feature": f, "weights": base.copy(), "candidates": np.asarray(cands, dtype=np.float64), "resident_slot": slot,
         "resident_owner": 1, "resident_norm": norm, "resident_base_f": float(base[f]), "resident_err": 0.0,
         "has_update": pend is not None, "upd_feature": 0, "upd_norm": 1.0, "upd_base_f": 0.0, "upd_cand": 0.0}
    if pend is not None:
        g.update(upd_feature=pend[0], upd_norm=pend[1], upd_base_f=pend[2], upd_cand=pend[3])
    return g


def _hand_log(seed, lens, d, measure, depth, steps, refresh_at, restarts=3):
    """A trainer in miniature: `restarts` restarts with a resident slot each, one line search of each per tick, every tick
    accepts a random candidate of every restart; the groups are staged in a rotating order with the last one 'routed'.
    Everything published is formed by direct calls of the oracle, the resident sums by position with o.resident_update."""
    rng = np.random.default_rng(seed)
    X, y, qid = _dataset(seed, lens, d)
    ds = o.Dataset(X, y, qid)
    name = measure_name(measure, depth)
    perm = _perm_with_holes(rng, len(y))
    valid = perm != NO_DOCUMENT
    xpos = np.zeros((len(perm), d), dtype=np.float32)
    xpos[valid] = X[perm[valid]]
    log = []
    w = [rng.uniform(-1, 1, d) for _ in range(restarts)]
    R = [None] * restarts      # by position
    pend = [None] * restarts

    def store(r):
        log.append({"type": "store", "slot": r, "v": w[r].copy()})
        R[r] = np.zeros(len(perm))
        R[r][valid] = ds.score_linear(w[r])[perm[valid]]
        pend[r] = None

    for r in range(restarts):
        store(r)
    for step in range(steps):
        if step == refresh_at:
            store(1)
        groups, accepted = [], []
        for r in range(restarts):
            norm = float(np.abs(w[r]).sum())
            base = w[r] / norm
            f = int(rng.integers(0, d))
            cands = base[f] + rng.normal(0.0, 0.3, 5 + 2 * r)   # 5, 7, 9 candidates: fewer than 64
            cands[0] = 0.0
            groups.append(_group(f, base, cands, r, norm, pend[r]))
            if pend[r] is not None:
                o.resident_update(R[r], np.ascontiguousarray(xpos[:, pend[r][0]]), pend[r][3], pend[r][2], 1.0 / pend[r][1])
            pick = float(cands[int(rng.integers(0, len(cands)))])
            accepted.append((f, norm, float(base[f]), pick))
            w[r] = base.copy()
            w[r][f] = pick
        gorder = np.roll(np.arange(restarts), step % restarts).astype(np.uint32)
        M = np.full((ds.nq, restarts * 64), 7.0)     # (the columns beyond a group's candidates hold anything)
        means = np.full(restarts * 64, -3.0)
        for k, g in enumerate(gorder):
            for c, cand in enumerate(groups[g]["candidates"]):
                wc = groups[g]["weights"].copy()
                wc[groups[g]["feature"]] = cand
                M[:, k * 64 + c], err = ds.metric_from_scores(name, ds.score_linear(wc))
                assert err == 0
                means[g * 64 + c] = ds.evaluate_mean(name, wc)
        nverify = restarts - 1
        redo = [(int(q) * nverify + int(k)) * 16 + 1 for q in rng.choice(ds.nq, 2, replace=False) for k in (0,)]
        log.append({"type": "tick", "ctx": step % 2, "kind": "topk", "measure": measure, "depth": depth, "groups": groups,
                    "gorder": gorder, "nverify": nverify, "approx": True, "resident": True, "ready": False,
                    "inst": {"k": 10, "xs_used": 1, "xs_pinned": False, "dup": False},
                    "redo": np.asarray(redo, dtype=np.uint32), "redo_groups": nverify, "means": means, "matrix": M,
                    "resident_sums": {r: R[r].copy() for r in range(restarts)}})
        pend = list(accepted)
    return (X, y, qid, perm), log


CASES = [(3, [1, 2, 9, 10, 11, 40, 130], 5, 0, 10), (4, [3, 17, 64, 65, 5, 1], 4, 2, -1)]


@pytest.mark.parametrize("seed,lens,d,measure,depth", CASES)
def test_hand_built_logs_pass_and_every_kind_of_error_is_named(seed, lens, d, measure, depth):
    (X, y, qid, perm), log = _hand_log(seed, lens, d, measure, depth, steps=55, refresh_at=30)
    model = TickModel(X, y, qid, perm)
    tot = check_log(model, log)
    assert tot["ticks"] == 55 and tot["stores"] == 4 and tot["unreplayed"] == 0 and tot["absent"] == 0
    assert tot["contexts"] == {0, 1}
    assert tot["pairs"] == 55 * 3 * len(lens) and tot["redone"] == 55 * 2 and tot["verified"] == 55 * (2 * len(lens) - 2)
    assert model.updates_in_verify > 50 and model.updates_by_kernel > 10   # (the last staged group is the routed one)
    # one wrong cell in a defined column, anywhere in the chain
    ticks = [i for i, ev in enumerate(log) if ev["type"] == "tick"]
    i = ticks[40]
    k, g = 1, int(log[i]["gorder"][1])
    q = 0   # (the redo list names staged group 0 only: this pair counts as verified)
    saved = log[i]["matrix"][q, k * 64 + 2]
    log[i]["matrix"][q, k * 64 + 2] = np.nextafter(saved, 2.0)
    model.reset()
    with pytest.raises(AssertionError, match=r"tick %d .*group %d .*candidate 2 query %d \(length %d, verified\)" % (i, g, q, model.qlen[q])):
        check_log(model, log)
    log[i]["matrix"][q, k * 64 + 2] = saved
    # ... a wrong mean
    log[i]["means"][g * 64 + 1] = np.nextafter(log[i]["means"][g * 64 + 1], 2.0)
    model.reset()
    with pytest.raises(AssertionError, match="mean of group %d candidate 1" % g):
        check_log(model, log)
    # ... one bit of one resident sum, which every later tick of the slot inherits in a real run
    _, log = _hand_log(seed, lens, d, measure, depth, steps=55, refresh_at=30)
    pos = int(np.nonzero(perm != NO_DOCUMENT)[0][5])
    log[ticks[10]]["resident_sums"][2][pos] = np.nextafter(log[ticks[10]]["resident_sums"][2][pos], 1e9)
    model.reset()
    with pytest.raises(AssertionError, match="tick %d: resident sum of slot 2 at position %d " % (ticks[10], pos)):
        check_log(model, log)
    # ... and a position that holds no document is not compared
    _, log = _hand_log(seed, lens, d, measure, depth, steps=55, refresh_at=30)
    hole = int(np.nonzero(perm == NO_DOCUMENT)[0][0])
    log[ticks[10]]["resident_sums"][0][hole] = 5.0
    model.reset()
    check_log(model, log)


def test_split_names_who_decided_a_pair():
    (X, y, qid, perm), log = _hand_log(3, [1, 2, 9, 10], 4, 0, 10, steps=3, refresh_at=99)
    model = TickModel(X, y, qid, perm)
    tick = [ev for ev in log if ev["type"] == "tick"][1]       # gorder = [2, 0, 1]: staged group 0 is the caller's 2
    assert list(tick["gorder"]) == [2, 0, 1]
    tick["redo"] = np.asarray([(3 * 2 + 0) * 16 + 0b0101, (1 * 2 + 1) * 16 + 0b0001, (3 * 2 + 0) * 16 + 0b1000], dtype=np.uint32)
    redone, verified = model.split(tick)
    assert redone == {(3, 2): 0b1101, (1, 0): 0b0001} and verified == 4 * 2 - 2
    tick["kind"], tick["redo_groups"], tick["nverify"] = "fullrank", 3, 3
    tick["redo"] = np.asarray([2 * 3 + 2], dtype=np.uint32)
    assert model.split(tick) == ({(2, 1): 15}, 4 * 3 - 1)
    tick["approx"] = False
    assert model.split(tick) == ({}, 0)
    # a line search evaluated at submit may come without its matrix, any other may not
    tick["matrix"] = None
    with pytest.raises(AssertionError, match="without its matrix"):
        check_tick(model, tick, 0, {})
    tick["ready"], tick["resident"], tick["resident_sums"] = True, False, {}
    assert check_tick(model, tick, 0, {}) == (0, 0, 1)


def test_means_are_the_oracles_in_the_device_shape():
    """evaluate_mean in the 256-segment shape, on more queries than one segment holds."""
    X, y, qid = _dataset(8, [2, 3] * 150, 3)
    model = TickModel(X, y, qid, np.arange(len(y)))
    rng = np.random.default_rng(8)
    base = rng.uniform(-1, 1, 3)
    cands = rng.uniform(-1, 1, 6)
    tick = {"measure": 0, "depth": 5, "groups": [_group(1, base, cands, -1, 1.0, None)], "gorder": [0]}
    means, defined = model.expected_means(tick)
    assert defined[:6].all() and not defined[6:].any()
    seq, seg = [], []
    for c in cands:
        wc = base.copy()
        wc[1] = c
        seq.append(model.ds.evaluate_mean("ndcg@5", wc))
        o.set_mean_segment(o.DEVICE_MEAN_SEGMENT)
        try:
            seg.append(model.ds.evaluate_mean("ndcg@5", wc))
        finally:
            o.set_mean_segment(0)
    assert means[:6].tolist() == seg
    assert seq != seg, "300 queries must tell the two summation shapes apart"
    assert o.lib().oracle_get_mean_segment() == 0
    assert device_mean(np.ones(7)) == 1.0


@pytest.mark.parametrize("normalize,refresh", [(True, 25), (False, None), (True, None)])
def test_replay_is_test_error_bounds_replay_bit_for_bit(normalize, refresh):
    """The chain of accepted candidates tests/test_error_bound.py replays (its generators, its arithmetic), written as a
    capture log: the model's resident sums equal that replay's after every update and every refresh."""
    def weights(rng, d):
        w = rng.uniform(-1, 1, d)
        return w / np.abs(w).sum()

    def cand(rng, orig):
        return float(orig + rng.normal() * 0.3) if rng.random() > 0.1 else 0.0

    trace = []
    teb._replay(211, 150, 12, 60, normalize, teb._signed_heavy_tail, weights, cand, refresh=refresh, trace=trace)
    X = trace[0][1]
    model = TickModel(X, np.zeros(len(X)), np.zeros(len(X), dtype=np.int64), np.arange(len(X)))
    updates = 0
    for what, val in trace[1:]:
        if what == "store":
            model.apply({"type": "store", "slot": 0, "v": val["w"]})
        else:
            base = np.zeros(X.shape[1])
            grp = _group(0, base, [0.0], 0, 1.0, (val["f"], val["norm"], val["base_f"], val["cand"]))
            got = model.apply({"type": "tick", "resident": True, "approx": True, "nverify": 1, "gorder": [0], "groups": [grp]})
            assert got[0] is model._sums[0]
            updates += 1
        assert model._sums[0].tobytes() == val["R"].tobytes(), (what, updates)
    assert updates == 60 and model.updates_in_verify == 60
    assert sum(1 for what, _ in trace if what == "store") == 1 + (60 // refresh if refresh else 0)
