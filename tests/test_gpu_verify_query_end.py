"""The query end of the NDCG@k bound-and-verify kernel (csrc/kernels_verify.inc, "the current query is complete"; csrc/verify_end.hpp)
on the shapes where it can go wrong: queries of 1, 2, K - 1 .. K + 2 documents for K = 5, 10, 20 and of 64, 65, 128, 129
documents (the walk-tile cuts); queries whose documents all tie, duplicates with equal and with different labels, scores one
f32 ulp apart, all-zero weights, negative and mixed-sign keys, a query with no relevant document.  Depth 5, 10, 20 (and 7: a
cut inside the list), lists of K + 1 .. K + 4 keys, duplicate groups on and off.

What is held: the trajectories and the per-candidate, per-query values are the oracle's bit for bit, and the counters that show
WHAT the kernel decided -- chain runs, (query, group) pairs sent to the exact kernel, their slice entries -- are the numbers
commit a80ce58 (the last one whose query end tested every pair with the exact bound and divided by the norm) counted on the
same inputs, on an MI355X.  A per-query gap bound in front of the pair tests and a division-free quotient change how a decided
value is computed, never what is decided.

Fallback taken / not taken (the plain K = 10, K + 1 keys variant is the one with the gap bound): the tie-heavy job lists pairs
for the exact kernel (verify_redone > 0), which only a pair that failed the cheap test and then the exact one can cause; on the
well-separated dataset every gap between two of a query's scores exceeds any bound the kernel can form by five orders of
magnitude (asserted here from the oracle's scores), so no rank of it reaches the fallback, and nothing is listed."""
import os

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import native
from oracle import pyoracle as o

pytestmark = pytest.mark.gpu

D = 6
LENGTHS = (1, 2, 4, 5, 6, 7, 9, 10, 11, 12, 19, 20, 21, 22, 64, 65, 128, 129)
FLAVOURS = ("plain", "all_tied", "dup_same_label", "dup_other_label", "ulp_apart", "no_relevant")


def _edge_dataset():
    """Six blocks of queries, one per flavour, each with every length of LENGTHS: 3210 documents."""
    rng = np.random.default_rng(20261020)
    Xs, ys, qs = [], [], []
    qid = 1
    for flavour in FLAVOURS:
        for n in LENGTHS:
            X = rng.normal(0.0, 1.0, (n, D)).astype(np.float32)   # mixed signs
            X[:, 1] = -np.abs(X[:, 1]) - 1.0                      # a column of negative values only
            y = rng.integers(0, 5, n).astype(np.float64)
            if flavour == "all_tied":
                X[:] = X[0]                                       # every document the same row: tied under every weight vector
            elif flavour in ("dup_same_label", "dup_other_label"):
                for i in range(1, n, 2):                          # pairs of identical rows
                    X[i] = X[i - 1]
                    y[i] = y[i - 1] if flavour == "dup_same_label" else (y[i - 1] + 1.0 + float(i % 3)) % 5.0
            elif flavour == "ulp_apart":
                X[:] = X[0]
                col = np.full(n, np.float32(1.5))
                for i in range(1, n):
                    col[i] = np.nextafter(col[i - 1], np.float32(2.0))   # neighbours one f32 ulp apart in column 0
                X[:, 0] = col[rng.permutation(n)]
            elif flavour == "no_relevant":
                y[:] = 0.0
            Xs.append(X), ys.append(y), qs.append(np.full(n, qid, dtype=np.int64))
            qid += 1
    X, y, q = np.concatenate(Xs), np.concatenate(ys), np.concatenate(qs)
    assert len(y) <= 4000
    return X, y, q


def _separated_dataset():
    """Scores far apart under every weight vector the test uses: column 0 holds a permutation of distinct integers per query,
    the other columns noise of 1e-3 -- no pair of a query comes near any error bound."""
    rng = np.random.default_rng(77)
    lens = [n for n in LENGTHS for _ in range(2)]
    q = np.repeat(np.arange(1, len(lens) + 1, dtype=np.int64), lens)
    X = (rng.uniform(-1.0, 1.0, (len(q), D)) * 1e-3).astype(np.float32)
    X[:, 0] = np.concatenate([rng.permutation(n) - n // 2 for n in lens]).astype(np.float32)
    y = rng.integers(0, 5, len(q)).astype(np.float64)
    return X, y, q


@pytest.fixture(scope="module")
def edge():
    X, y, q = _edge_dataset()
    return X, y, q, o.Dataset(X, y, q)


_ORACLE = {}


def _request(depth):
    req = fr.TrainRequest.coordinate_ascent()
    req.measure = "ndcg@%d" % depth
    p = req.params
    p.seed, p.quiet, p.num_restarts, p.num_max_iterations = 11, True, 2, 3
    return req


def _oracle_run(c, depth):
    """the oracle's trajectories and per-query values of the candidate check, once per depth"""
    if depth not in _ORACLE:
        req = _request(depth)
        exp_s, exp_w, exp_e, err = c.ca_learn(req.measure, req.params.to_dict(), threads=2)
        assert err == 0
        _ORACLE[depth] = (exp_s, exp_w, exp_e, {})
    return _ORACLE[depth]


def _candidate_groups():
    rng = np.random.default_rng(5)
    bases = np.zeros((3, D))
    bases[1] = rng.uniform(-1.0, 1.0, D)
    bases[2] = -np.abs(rng.uniform(0.1, 1.0, D))       # negative weights on every feature
    feats = [0, 3, 1]
    cands = [np.asarray([0.0, 1.0, -1.0, 1e-6, -250.0]),   # (candidate 0 of group 0: all-zero weights, every document tied)
             o.ca_candidates(bases[1][3], 0.05, 2.0, 6), o.ca_candidates(bases[2][1], 0.05, 2.0, 6)]
    return feats, bases, cands


def run_case(X, y, q, c, depth, xs, nodup):
    """One job of the edge dataset under (depth, list length, duplicate groups): the counters of the training run, after its
    trajectories and the candidate values have been held to the oracle.  (The environment must already be set: the duplicate
    groups are found when the dataset is made.)"""
    g = fr.CDataset.from_numpy(X, y, q)
    req = _request(depth)
    shard = native.train_model_shard(g, req, 0, 2)
    st = shard["stats"]
    if c is not None:
        exp_s, exp_w, exp_e, cache = _oracle_run(c, depth)
        for r in shard["restarts"]:
            k = r["restart_id"]
            assert r["score"] == exp_s[k] and r["weights"] == exp_w[k].tolist(), (depth, xs, nodup, k)
        assert st["useful_evals"] == int(exp_e.sum())
        feats, bases, cands = _candidate_groups()
        means, pq = native.evaluate_candidates(g, req.measure, feats, bases, cands, per_query=True)
        for gi in range(len(feats)):
            for ci in range(len(cands[gi])):
                if (gi, ci) not in cache:
                    w = bases[gi].copy()
                    w[feats[gi]] = cands[gi][ci]
                    cache[(gi, ci)] = c.metric_from_scores(req.measure, c.score_linear(w))[0]
                got, exp = pq[:, gi * 64 + ci], cache[(gi, ci)]
                assert np.array_equal(got, exp) and np.array_equal(np.signbit(got), np.signbit(exp)), (depth, xs, nodup, gi, ci)
    return {k: int(st[k]) for k in ("chain_runs", "verify_redone", "verify_redo_entries")}


# (depth, FR_VERIFY_XS, FR_NO_DUP_GROUPS set): what run_case returned at commit a80ce58 on an MI355X
# (recorded by calling run_case with that commit's library for every case below)
PARENT_COUNTERS = {
    (5, 1, False): {"chain_runs": 4208, "verify_redone": 208, "verify_redo_entries": 208},
    (5, 1, True): {"chain_runs": 3800, "verify_redone": 248, "verify_redo_entries": 248},
    (5, 2, False): {"chain_runs": 12773, "verify_redone": 251, "verify_redo_entries": 251},
    (5, 2, True): {"chain_runs": 3996, "verify_redone": 187, "verify_redo_entries": 187},
    (5, 3, False): {"chain_runs": 13050, "verify_redone": 238, "verify_redo_entries": 238},
    (5, 3, True): {"chain_runs": 4142, "verify_redone": 187, "verify_redo_entries": 187},
    (7, 1, False): {"chain_runs": 5010, "verify_redone": 179, "verify_redo_entries": 179},
    (7, 1, True): {"chain_runs": 4734, "verify_redone": 238, "verify_redo_entries": 238},
    (10, 1, False): {"chain_runs": 20960, "verify_redone": 402, "verify_redo_entries": 402},
    (10, 1, True): {"chain_runs": 5770, "verify_redone": 236, "verify_redo_entries": 236},
    (10, 2, False): {"chain_runs": 38695, "verify_redone": 470, "verify_redo_entries": 470},
    (10, 2, True): {"chain_runs": 6102, "verify_redone": 221, "verify_redo_entries": 221},
    (10, 3, False): {"chain_runs": 45753, "verify_redone": 475, "verify_redo_entries": 475},
    (10, 3, True): {"chain_runs": 6589, "verify_redone": 221, "verify_redo_entries": 221},
    (10, 4, False): {"chain_runs": 45077, "verify_redone": 475, "verify_redo_entries": 475},
    (10, 4, True): {"chain_runs": 6518, "verify_redone": 221, "verify_redo_entries": 221},
    (20, 1, False): {"chain_runs": 18246, "verify_redone": 210, "verify_redo_entries": 210},
    (20, 1, True): {"chain_runs": 6771, "verify_redone": 196, "verify_redo_entries": 196},
    (20, 2, False): {"chain_runs": 43552, "verify_redone": 285, "verify_redo_entries": 285},
    (20, 2, True): {"chain_runs": 7409, "verify_redone": 187, "verify_redo_entries": 187},
    (20, 3, False): {"chain_runs": 47656, "verify_redone": 255, "verify_redo_entries": 255},
    (20, 3, True): {"chain_runs": 8090, "verify_redone": 187, "verify_redo_entries": 187},
    (20, 4, False): {"chain_runs": 47536, "verify_redone": 255, "verify_redo_entries": 255},
    (20, 4, True): {"chain_runs": 8074, "verify_redone": 187, "verify_redo_entries": 187},
}

CASES = [(depth, xs, nodup) for depth in (5, 10, 20) for xs in (1, 2, 3, 4) for nodup in (False, True) if not (depth == 5 and xs == 4)] + \
        [(7, 1, True), (7, 1, False)]


def _verify_path_on():
    return not os.environ.get("FR_LS_EXACT") and os.environ.get("FR_LS_RESIDENT", "1")[:1] != "0"


@pytest.mark.parametrize("depth,xs,nodup", CASES)
def test_query_end_values_and_decisions_are_the_parents(edge, monkeypatch, depth, xs, nodup):
    X, y, q, c = edge
    monkeypatch.setenv("FR_VERIFY_XS", str(xs))
    if nodup:
        monkeypatch.setenv("FR_NO_DUP_GROUPS", "1")
    else:
        monkeypatch.delenv("FR_NO_DUP_GROUPS", raising=False)
    got = run_case(X, y, q, c, depth, xs, nodup)
    print("query end counters", (depth, xs, nodup), got)
    if _verify_path_on():
        assert got == PARENT_COUNTERS[(depth, xs, nodup)], (depth, xs, nodup)
        if depth in (7, 10) and xs == 1 and nodup:
            assert got["verify_redone"] > 0, "the variant with the gap bound must have taken its fallback here"


def test_well_separated_queries_never_reach_the_fallback(monkeypatch):
    monkeypatch.setenv("FR_VERIFY_XS", "1")
    monkeypatch.setenv("FR_NO_DUP_GROUPS", "1")
    X, y, q = _separated_dataset()
    g, c = fr.CDataset.from_numpy(X, y, q), o.Dataset(X, y, q)
    rng = np.random.default_rng(9)
    base = rng.uniform(-0.5, 0.5, (1, D))
    base[0, 0] = 1.0
    cands = [np.asarray([0.5, 1.0, 2.0, -1.0, -3.0, 40.0])]   # (never 0: column 0 keeps every pair apart)
    means, pq = native.evaluate_candidates(g, "ndcg@10", [0], base, cands, per_query=True)
    colmax = np.abs(X).max(axis=0).astype(np.float64)
    for ci, cv in enumerate(cands[0]):
        w = base[0].copy()
        w[0] = cv
        s = c.score_linear(w)
        assert np.array_equal(pq[:, ci], c.metric_from_scores("ndcg@10", s)[0]), ci
        # any bound the kernel forms is a few hundred u * sum_j |w_j| max|x_j|: 1e-9 of it is far above
        T = float((np.abs(w) * colmax).sum())
        for qq in np.unique(q):
            sq = np.sort(s[q == qq])
            assert len(sq) < 2 or np.diff(sq).min() > 1e-9 * T
    req = _request(10)
    shard = native.train_model_shard(g, req, 0, 2)
    exp_s, exp_w, _, err = c.ca_learn(req.measure, req.params.to_dict(), threads=2)
    assert err == 0
    for r in shard["restarts"]:
        assert r["score"] == exp_s[r["restart_id"]] and r["weights"] == exp_w[r["restart_id"]].tolist()
