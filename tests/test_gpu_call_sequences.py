"""A call's result is a function of its arguments, not of what the handle did before ("State between calls").

Every op of tests/call_catalogue.py is run once on handles built for it alone; those bytes are the reference of every later
run of the op, whatever ran before it on the same handles: after every other op (all ordered pairs, history accumulating
along a row), along seeded walks with handle-lifetime events between the ops, and from several host threads at once.  The
fresh bytes themselves are held to the oracle and the numpy restatements by the feature tests; here every comparison is bit
equality with them and nothing else.
"""
import threading
import time

import pytest

from fastrank_amd import native
from tests import call_catalogue as cc

pytestmark = pytest.mark.gpu

ROW_PARTS = 4        # a row of pairs (one first op, every second op) is split over this many cases: a few seconds each
THREAD_LIMIT = 240   # seconds a thread of the thread tests may take before the test fails with the op it is in

_FRESH = {}          # op name -> {part: bytes} on a fresh handle
_FRESH_PLAN = {}     # forest ops: native.last_tree_plan() after the fresh run


def _fresh_group(name):
    """The ops that share one set of fresh handles with `name`: the stepped trainer's parts (its reference is the
    uninterrupted run), or the op alone."""
    return list(cc.STEPPED_PARTS) if name in cc.STEPPED_PARTS else [name]


def fresh(name):
    """The op's bytes on handles built for it alone (computed once; run a second time on the same handles: the same bytes)."""
    if name not in _FRESH:
        group = _fresh_group(name)
        h = cc.Handles()
        first = {}
        for n in group:
            [(ran, got)] = cc.run_op(h, n)
            assert ran == n
            first[n] = got
            if cc.OPS[n].plan is not None:
                _FRESH_PLAN[n] = native.last_tree_plan()
        for n in group:  # determinism: the pair (a, a)
            [(ran, got)] = cc.run_op(h, n)
            assert cc.differing_parts(got, first[n]) == [], "op %s gives other bytes the second time on the same handles: %s" % (
                n, cc.differing_parts(got, first[n]))
        h.close()
        _FRESH.update(first)
    return _FRESH[name]


def check(h, ran, ctx=None):
    """Holds what run_op / run_step returned to the fresh bytes; a failure names the differing parts and the whole history."""
    for name, got in ran:
        bad = cc.differing_parts(got, fresh(name), ctx)
        assert not bad, "op %s: parts %s differ from a fresh handle's after the history\n  %s" % (name, bad, "\n  ".join(h.history))


# ---------------------------------------------------------------------------------------------- fresh references

@pytest.mark.parametrize("name", cc.NAMES)
def test_fresh_reference_and_determinism(name):
    got = fresh(name)
    o = cc.OPS[name]
    assert got and all(isinstance(v, bytes) and len(v) > 0 for v in got.values())
    if o.refusal:
        assert list(got) == ["refused"] and got["refused"] != cc.canon("NOT REFUSED"), name
        print(name, "->", got["refused"][:200])
    if o.plan is not None:
        plan = _FRESH_PLAN[name]
        assert plan["path"] == o.plan and plan["cache_hit"] is False, (name, plan)
    if any(k.startswith("hook:") for k in got):
        assert got["hook:measures"] != cc.canon({"train_measure": None, "valid_measure": None, "best_iteration": None})


def test_refusals_say_why_and_different_results_have_different_bytes():
    assert b"NaN" in fresh("refused_nan_scores")["refused"] and b"NaN" in fresh("refused_nan_scores_ndcg@qview")["refused"]
    assert b"32" in fresh("refused_explain_33_features")["refused"]
    assert b"symmetric" in fresh("refused_lm_exclusive_keys")["refused"]
    # the catalogue's variants are different calls: were two of these equal, a stale result of one would pass for the other
    for a, b in (("score_forest_rank_70", "score_forest_rank_70_ulp"), ("eval_ndcg@10", "eval_ndcg@5"), ("eval_ndcg@10+qrel_a", "eval_ndcg@10+qrel_b"),
                 ("eval_ndcg@10", "eval_ndcg@10+qrel_a"), ("eval_map+qrel_a", "eval_map+qrel_b"), ("lm_held_out_a@qview", "lm_held_out_b@qview"),
                 ("lm_leaves_255@qview", "lm_leaves_4@qview"), ("lm_hist_k64@qview", "lm_hist_k8@qview"), ("lm_hist_k16@qview", "lm_init_model@qview"),
                 ("lm_hist_k16@qview", "lm_valid_sibling@qview"), ("lm_hist_k16", "lm_hist_k16_ndcg"), ("hist_tree", "hist_tree_k64_leafwise"),
                 ("lambda_gradients_sampled", "lambda_gradients_sampled_b"), ("lambda_gradients_sampled_b", "lambda_gradients_trunc_norm"),
                 ("explain", "explain_background_sibling"), ("candidates_70_ndcg@10", "candidates_70_err@10"),
                 ("ca_stepped_1_open+step", "ca_stepped_2_step"), ("score_ensemble_linear", "score_linear")):
        assert fresh(a) != fresh(b), (a, b)
    # ... and the same call through another kernel or a second time is the same result
    assert fresh("eval_dcg@10[topk]") == fresh("eval_dcg@10[sort]") and fresh("eval_dcg@10[topk]+qrel_a") == fresh("eval_dcg@10[sort]+qrel_a")
    assert fresh("score_forest_rank_70") == fresh("score_forest_rank_70_again")
    assert fresh("lm_held_out_a@qview")["model"] != fresh("lm_hist_k16@qview")["model"]


# ---------------------------------------------------------------------------------------------- every ordered pair

PAIR_CASES = [(a, part) for a in cc.NAMES for part in range(ROW_PARTS)]


def _row(part):
    return cc.NAMES[part::ROW_PARTS]


def test_the_pair_cases_cover_every_ordered_pair():
    covered = [(a, b) for a, part in PAIR_CASES for b in _row(part)]
    assert len(covered) == len(cc.NAMES) ** 2 == len(set(covered)) and set(covered) == set(cc.pairs())


@pytest.mark.parametrize("a, part", PAIR_CASES, ids=["%s-%d" % c for c in PAIR_CASES])
def test_every_ordered_pair(a, part):
    """One set of handles per case: for every b of the case's share of the catalogue, a then b on the same handles, both held
    to their fresh bytes.  The handles are not rebuilt between the b's: the history accumulates."""
    h = cc.Handles()
    done = 0
    for b in _row(part):
        check(h, cc.run_op(h, a))
        check(h, cc.run_op(h, b))
        done += 1
    h.close()
    assert done == len(_row(part)) > 0


# ---------------------------------------------------------------------------------------------- seeded walks

@pytest.mark.parametrize("seed", range(8))
def test_seeded_walk(seed):
    h = cc.Handles()
    ran = 0
    for step in cc.walk(seed):
        out = cc.run_step(h, step)
        check(h, out)
        ran += len(out)
    h.close()
    assert ran >= 45


# ---------------------------------------------------------------------------------------------- the stateful paths are reached

def _lm_bins_ms():
    return native.last_train_stats()["lambdamart"]["bins_ms"]


def test_the_catalogue_reaches_the_stateful_paths_on_an_accumulated_handle():
    h = cc.Handles()

    def run(name):
        check(h, cc.run_op(h, name))

    for name in ("eval_ndcg@10", "lm_exact@qview", "permutation_importance_forest", "ca_ndcg@10"):
        run(name)
    # the packed-forest cache
    run("score_forest_rank_70")
    assert native.last_tree_plan()["path"] == "rank" and native.last_tree_plan()["cache_hit"] is False
    run("score_forest_rank_70_again")
    assert native.last_tree_plan()["path"] == "rank" and native.last_tree_plan()["cache_hit"] is True
    run("eval_ndcg@10_forest")  # evaluate after predict: the same forest
    assert native.last_tree_plan()["cache_hit"] is True
    run("score_forest_rank_70_ulp")
    assert native.last_tree_plan()["path"] == "rank" and native.last_tree_plan()["cache_hit"] is False
    run("score_forest_rank_70")
    assert native.last_tree_plan()["cache_hit"] is False
    run("score_forest_rank_70_again")
    assert native.last_tree_plan()["cache_hit"] is True
    run("score_forest_lds")
    assert native.last_tree_plan()["path"] == "lds"
    run("score_forest_rank_70")
    assert native.last_tree_plan()["path"] == "rank" and native.last_tree_plan()["cache_hit"] is False
    run("score_forest_l2")
    assert native.last_tree_plan()["path"] == "l2"
    run("score_forest_rank_2")
    assert native.last_tree_plan()["path"] == "rank" and native.last_tree_plan()["cache_hit"] is False
    # the kept bin matrix: the second histogram training with the same k does not bin again
    run("lm_hist_k16")
    assert _lm_bins_ms() > 0.0
    run("lm_hist_k16_ndcg")
    assert _lm_bins_ms() == 0.0
    run("lm_hist_k64@qview")
    run("lm_hist_k16@qview")
    assert _lm_bins_ms() > 0.0
    run("lm_hist_k16_ndcg@qview")
    assert _lm_bins_ms() == 0.0
    run("lm_sampled@qview")
    assert _lm_bins_ms() == 0.0
    run("lm_hist_k8@qview")
    assert _lm_bins_ms() > 0.0
    # the forced metric kernels
    run("eval_dcg@10[sort]")
    plan = native.last_metric_plan()
    assert {c["kernel"] for c in plan["classes"]} == {"sort"} and plan["measure"] == "dcg" and plan["depth"] == 10
    run("eval_dcg@10[topk]+qrel_a")
    assert {c["kernel"] for c in native.last_metric_plan()["classes"]} == {"topk"}
    run("candidates_70_err@10")
    assert native.last_metric_plan()["slots"] >= 70
    run("candidates_2_err@10")
    assert native.last_metric_plan()["slots"] == 2
    # the training paths the coordinate-ascent ops stand for
    paths = {}
    for name in ("ca_ndcg@10", "ca_ndcg", "ca_mrr", "ca_dcg@5"):
        run(name)
        paths[name] = native.last_train_stats()["path"]
    assert paths["ca_ndcg@10"] == "fused_linesearch" and paths["ca_dcg@5"] == "generic_sort", paths
    assert paths["ca_ndcg"] == paths["ca_mrr"] == "fused_fullrank", paths
    h.close()


# ---------------------------------------------------------------------------------------------- host threads, one process

def _run_threads(jobs):
    """jobs: [(label, function(report))]; report(op) notes the op a thread is in.  Daemon threads, joined with a limit."""
    state = {label: {"op": None, "error": None, "done": False} for label, _ in jobs}

    def body(label, fn):
        try:
            fn(lambda op: state[label].__setitem__("op", op))
            state[label]["done"] = True
        except BaseException as exc:  # noqa: BLE001 (reported by the test's thread)
            state[label]["error"] = exc

    assert len(jobs) <= 4
    threads = [threading.Thread(target=body, args=job, daemon=True, name=job[0]) for job in jobs]
    for t in threads:
        t.start()
    deadline = time.monotonic() + THREAD_LIMIT
    for t in threads:
        t.join(max(0.0, deadline - time.monotonic()))
    stuck = [(t.name, state[t.name]["op"]) for t in threads if t.is_alive()]
    assert not stuck, "threads still running after %d s, in the op: %s" % (THREAD_LIMIT, stuck)
    for label, s in state.items():
        if s["error"] is not None:
            raise AssertionError("thread %s, in op %s: %s" % (label, s["op"], s["error"])) from s["error"]
        assert s["done"]


def test_four_threads_each_on_handles_of_their_own():
    walks = {"walk-%d" % seed: cc.walk(seed, 40) for seed in (100, 101, 102, 103)}
    for w in walks.values():
        for step in w:
            if not step.startswith("@"):
                fresh(step)
    for n in cc.STEPPED_PARTS:
        fresh(n)
    ctx = cc.Ctx(threaded=True)

    def job(steps):
        def fn(report):
            h = cc.Handles()
            for step in steps:
                report(step)
                check(h, cc.run_step(h, step, ctx), ctx)
            h.close()
        return fn

    _run_threads([(label, job(steps)) for label, steps in walks.items()])


def test_three_threads_on_one_dataset_and_its_views():
    """The parent, its query view and its feature view from one thread each, at once: each runs the ops that touch its handle
    (the query view's thread: the sibling too, its validation set) in catalogue order."""
    h = cc.Handles()
    mine = {"parent": ("parent",), "qview": ("qview", "sibling"), "fview": ("fview",)}
    rows = {label: [n for n in cc.NAMES if set(cc.OPS[n].handles) <= set(hs)] for label, hs in mine.items()}
    assert all(len(r) >= 5 for r in rows.values()) and set(cc.STEPPED_PARTS) <= set(rows["qview"])
    for r in rows.values():
        for n in r:
            fresh(n)
    ctx = cc.Ctx(threaded=True)

    def job(names):
        def fn(report):
            for n in names:
                report(n)
                check(h, cc.run_op(h, n, ctx), ctx)
        return fn

    _run_threads([(label, job(names)) for label, names in rows.items()])
    h.close()
