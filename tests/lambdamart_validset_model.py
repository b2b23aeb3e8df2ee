"""numpy restatement of LambdaMART with a validation dataset of its own and with an init model (DESIGN.md section 11,
"Validation dataset" and "Continued training"), for the tests.  Built on lambdamart_valid_model (held-out queries, the
stopping rule) and lambdamart_sample_model (samples, both growers' trees on a sample).

The definition, restated:
  * A = the training view, B = the validation dataset.  No tree depends on B: gradients, grow, leaves, bins, fixed-point
    exponents and samples are those of the same request on A without B.  With early_stopping_rounds = 0 the model is that
    request's model.
  * After every tree s_B = s_B + w * tree(x), the scoring rule, unfused: the scores of the model so far on B.
  * valid_measure[t] = the plain two-level mean (oracle.pyoracle.mean) of the evaluator over ALL of B's queries in B's
    order, with B's own norms; zero-norm queries count 0.0 and count in the divisor.  train_measure[t] = the mean over all
    of A's queries (or over A's training queries when A also holds queries out: then B is not allowed).
  * An init model of T0 trees: scores start at sum_i w_i tree_i(x) in the ensemble's order (s = 0.0; s = s + w_i * tree_i(x)).
    New tree j is tree T0 + j: its samples are lambdamart_valid_model.sample(seed, T0 + j, ..).  num_trees counts new trees.
    The result is the init model's weights and trees followed by [learning_rate] and the new trees.
  * Stopping: best_iteration is a tree count of the result.  It starts at T0 with the init model's held-out measure (T0 = 0:
    no baseline); new tree j is iteration T0 + j + 1 and takes over only with a strictly greater measure; training ends once
    iteration - best_iteration >= r; with r > 0 the result is the first best_iteration trees, never fewer than T0.
"""
import numpy as np

from oracle import pyoracle as o
from tests import lambdamart_hist_model as hm
from tests import lambdamart_model as lm
from tests import lambdamart_sample_model as sm
from tests import lambdamart_valid_model as vm


def stopping(valid, r, num_trees=None, T0=0, init_valid=None):
    """The rule on the held-out measures of the NEW trees in training order: (best_iteration, new trees trained,
    stopped_early, trees in the result), the first and last counted with the init model's T0 trees.  init_valid: the init
    model's own held-out measure (read when T0 > 0).  With T0 = 0 it is lambdamart_valid_model.stopping."""
    num_trees = len(valid) if num_trees is None else num_trees
    best_it, best = (T0, init_valid) if T0 > 0 else (0, 0.0)
    for j in range(num_trees):
        it, v = T0 + j + 1, valid[j]
        if best_it == 0 or v > best:
            best_it, best = it, v
        if r > 0 and it - best_it >= r:
            return best_it, j + 1, j + 1 < num_trees, best_it
    return best_it, num_trees, False, best_it if r > 0 else T0 + num_trees


def ensemble_scores(weights, trees, X):
    """s = +0.0; s = s + w_i * tree_i(x) in the ensemble's order, product and sum rounded separately."""
    s = np.zeros(X.shape[0], dtype=np.float64)
    for w, tree in zip(weights, trees):
        s = s + float(w) * lm.tree_scores(tree, X)
    return s


def train(X, y, c, B=None, held_idx=(), init=None, grower="exact", measure="ndcg", num_trees=10, learning_rate=0.1, max_depth=6,
          min_leaf_support=10, split_candidates=64, sigma=1.0, norms=None, norms_b=None, feats=None, rates=(1.0, 1.0), seed=0,
          early_stopping_rounds=0, binned=None):
    """The boosting loop.  B = (X_B, y_B, oracle dataset of B) or None; held_idx: A's own held-out queries (not with B);
    init = (weights, trees) or None; binned: the histogram grower's (edges, bins) over A's full list (default: made here).
    Returns a dict: model, trees (the new ones), train_measure, valid_measure, init_train_measure, init_valid_measure,
    best_iteration, trees_trained, stopped_early, scores, scores_b."""
    queries = lm.query_lists(c)
    nq = len(queries)
    H = np.array(sorted(int(q) for q in held_idx), dtype=np.int64)
    assert B is None or len(H) == 0, "one source of the held-out measure"
    T = np.array([q for q in range(nq) if q not in set(H.tolist())], dtype=np.int64)
    held = B is not None or len(H) > 0
    assert len(T) > 0 and (early_stopping_rounds == 0 or held)
    order_ids = np.concatenate(queries)
    norms = c.default_norms(measure) if norms is None else norms
    feats = sorted(range(X.shape[1]) if feats is None else feats)
    if grower == "histogram" and binned is None:
        binned = hm.bin_matrix(X, order_ids, feats, split_candidates)  # A's list alone: B has no part in the bins
    w0, trees0 = ([], []) if init is None else (list(init[0]), list(init[1]))
    T0 = len(trees0)
    s = ensemble_scores(w0, trees0, X)
    if B is not None:
        XB, yB, cB = B
        norms_b = cB.default_norms(measure) if norms_b is None else norms_b
        sb = ensemble_scores(w0, trees0, XB)

    def measures():
        per_q, _ = c.metric_from_scores(measure, s, norms)
        if B is not None:
            per_b, _ = cB.metric_from_scores(measure, sb, norms_b)
            return o.mean(per_q), o.mean(per_b)
        if len(H):
            return vm.subset_mean(per_q, T), vm.subset_mean(per_q, H)
        return o.mean(per_q), None

    init_train, init_valid = measures() if init is not None else (None, None)
    trees, train_m, valid_m = [], [], []
    r = early_stopping_rounds
    best_it, best, stopped = (T0, init_valid, False) if (T0 > 0 and held) else (0, 0.0, False)
    for j in range(num_trees):
        fsel, qsel = vm.sample(seed, T0 + j, len(feats), T, rates)
        lam, wt = lm.gradients(s, y, [queries[q] for q in qsel], [norms[q] for q in qsel], lm.depth_of(measure), sigma)
        tree = sm.tree_for(grower, X, lam, wt, queries, feats, binned, qsel, fsel, max_depth, min_leaf_support, split_candidates)
        s = s + learning_rate * lm.tree_scores(tree, X)
        if B is not None:
            sb = sb + learning_rate * lm.tree_scores(tree, XB)
        trees.append(tree)
        tr, va = measures()
        train_m.append(tr)
        if held:
            valid_m.append(va)
            it = T0 + j + 1
            if best_it == 0 or va > best:
                best_it, best = it, va
            if r > 0 and it - best_it >= r:
                stopped = j + 1 < num_trees
                break
    kept = best_it if (held and r > 0) else T0 + len(trees)
    assert not held or (best_it, len(trees), stopped, kept) == stopping(valid_m + [0.0] * (num_trees - len(valid_m)), r, num_trees, T0, init_valid)
    all_w, all_t = (w0 + [learning_rate] * len(trees))[:kept], (trees0 + trees)[:kept]
    model = {"Ensemble": {"weights": all_w, "models": [{"DecisionTree": t} for t in all_t]}}
    return dict(model=model, trees=trees, train_measure=train_m, valid_measure=valid_m, init_train_measure=init_train,
                init_valid_measure=init_valid, best_iteration=best_it, trees_trained=len(trees), stopped_early=stopped,
                scores=ensemble_scores(all_w, all_t, X), scores_b=ensemble_scores(all_w, all_t, B[0]) if B is not None else None)
