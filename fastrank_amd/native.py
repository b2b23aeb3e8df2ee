"""Extensions of the C ABI that have no reference counterpart (include/fastrank.h part 2):
dense result buffers, the batched line-search evaluator, restart-sharded and query-sharded multi-GPU
training and HIP-event kernel timing.  numpy is used only to hold buffers that cross the ABI."""
import ctypes as C
import json
import math
from typing import Dict, List, Optional, Tuple

import numpy as np

from .clib import ALLREDUCE_SUM_FN, CDataset, CModel, CQRel, HistTreeOptions, _json_reply, _load, _status, _take_str, _unwrap


def device_count() -> int:
    return int(_load().fr_device_count())


def set_device(ordinal: int) -> None:
    if _load().fr_set_device(int(ordinal)) != 0:
        raise RuntimeError("fr_set_device({}) failed".format(ordinal))


def version() -> str:
    return _load().fr_version().decode("utf-8")


def synchronize() -> None:
    if _load().fr_synchronize() != 0:
        raise RuntimeError("device synchronize failed")


def num_queries(dataset: CDataset) -> int:
    nq = int(_load().fr_dataset_num_queries(dataset.pointer))
    if nq == C.c_size_t(-1).value:
        raise ValueError("dataset cannot be grouped by query (a NaN label?): compute calls report the reason")
    return nq


def device_info(dataset: CDataset) -> Dict:
    """How the dataset lives on the device (builds the device form if needed); see include/fastrank.h."""
    return _json_reply(_load().fr_dataset_device_info(dataset.pointer))


def predict_scores_dense(model: CModel, dataset: CDataset, n_total: Optional[int] = None) -> np.ndarray:
    """Scores indexed by instance id (NaN where the id is not part of a sampled dataset)."""
    n = int(n_total if n_total is not None else _load().fr_dataset_num_instances(dataset.pointer))
    if n_total is None and dataset.is_sampled():
        n = 1 + max(max(ids) for ids in dataset.instances_by_query().values())
    out = np.full(n, np.nan, dtype=np.float64)
    _status(_load().fr_predict_scores_dense(model.pointer, dataset.pointer, out.ctypes.data, n))
    return out


class Explanation:
    """What CModel.explain returns: values[n, F] (float64, by instance id; NaN rows where the id is not part of a sampled
    dataset), the columns' feature_ids / feature_names, expected_value (the bias: values.sum(1) + expected_value is the
    score) and the call's status (timings, sizes)."""

    def __init__(self, values, feature_ids, feature_names, expected_value, status):
        self.values, self.feature_ids, self.feature_names = values, feature_ids, feature_names
        self.expected_value, self.status = expected_value, status


def explain_dense(model: CModel, dataset: CDataset, background: Optional[CDataset] = None, n_total: Optional[int] = None) -> Explanation:
    """fr_explain_dense: exact TreeSHAP contributions by instance id (include/fastrank.h)."""
    n = int(n_total if n_total is not None else _load().fr_dataset_num_instances(dataset.pointer))
    if n_total is None and dataset.is_sampled():
        n = 1 + max(max(ids) for ids in dataset.instances_by_query().values())
    names = dataset.feature_index_to_name()
    ids = sorted(names)
    out = np.full((n, len(ids) + 1), np.nan, dtype=np.float64)
    rep = _json_reply(_load().fr_explain_dense(model.pointer, dataset.pointer, None if background is None else background.pointer,
                                               out.ctypes.data, n, len(ids) + 1))
    assert [int(f) for f in rep["feature_ids"]] == ids
    return Explanation(out[:, :-1], np.asarray(ids, dtype=np.uint32), [names[f] for f in ids], float(rep["expected_value"]), rep)


def feature_importance(model: CModel, dataset: CDataset, background: Optional[CDataset] = None) -> Tuple[np.ndarray, np.ndarray, Dict]:
    """fr_feature_importance: (feature ids ascending, mean |contribution| per feature, the status with "split_counts")."""
    ids = sorted(dataset.feature_ids())
    out = np.zeros(len(ids), dtype=np.float64)
    rep = _json_reply(_load().fr_feature_importance(model.pointer, dataset.pointer, None if background is None else background.pointer,
                                                    out.ctypes.data, len(ids)))
    assert [int(f) for f in rep["feature_ids"]] == ids
    return np.asarray(ids, dtype=np.uint32), out, rep


def explain_table(model: CModel, leaf_counts, dataset_features: int) -> Dict:
    """fr_debug_explain_table: the explain kernel's path table for given leaf counts (no device).  Doubles come back as
    float64 arrays (they cross as the hex of their bits)."""
    lc = np.ascontiguousarray(leaf_counts, dtype=np.uint32)
    rep = _json_reply(_load().fr_debug_explain_table(model.pointer, lc.ctypes.data if len(lc) else None, len(lc), int(dataset_features)))
    for key in ("weight", "value", "lo", "hi", "z", "bias"):
        rep[key] = np.asarray([int(h, 16) for h in rep[key]], dtype=np.uint64).view(np.float64)
    return rep


def evaluate_dense(model: CModel, dataset: CDataset, evaluator: str, qrel: Optional[CQRel] = None) -> Tuple[List[str], np.ndarray]:
    nq = num_queries(dataset)
    out = np.zeros(nq, dtype=np.float64)
    qids_ptr = C.c_void_p()
    _status(
        _load().fr_evaluate_dense(
            model.pointer, dataset.pointer, None if qrel is None else qrel.pointer, evaluator.encode("utf-8"),
            out.ctypes.data, nq, C.byref(qids_ptr),
        )
    )
    return json.loads(_take_str(qids_ptr.value)), out


def resample(V, trials: int, seed: int, alpha: float = 0.05, boot: bool = True, perm: bool = True) -> Tuple[Dict, Optional[np.ndarray], Optional[np.ndarray]]:
    """fr_resample (include/fastrank.h): V[Q, M] float64, row q one query's value under each of M
    systems.  Returns (report, boot, perm): the host's report with the call's stats, and the paired bootstrap's and the
    per-query permutation's means, trials x M float64 in trial order (None where boot / perm is False: that kernel is skipped)."""
    V = np.asarray(V, dtype=np.float64)
    if V.ndim != 2:
        raise ValueError("resample takes a table V[Q, M]")
    V = np.ascontiguousarray(V)
    nq, ncols = V.shape
    t = int(trials)
    rows = t if 0 < t <= (1 << 20) else 0  # (out of range: refused by the call before it writes)
    out_b = np.zeros((rows, ncols), dtype=np.float64) if boot else None
    out_p = np.zeros((rows, ncols), dtype=np.float64) if perm else None
    options = {"trials": t, "seed": int(seed), "alpha": float(alpha)}
    rep = _json_reply(_load().fr_resample(V.ctypes.data if V.size else None, nq, ncols, json.dumps(options).encode("utf-8"),
                                          out_b.ctypes.data if boot and rows else None, out_p.ctypes.data if perm and rows else None))
    return rep, out_b, out_p


def permutation_importance_dense(model: CModel, dataset: CDataset, evaluator: str, qrel: Optional[CQRel] = None, repeats: int = 5, seed: int = 0,
                                 scope: str = "dataset", features=None, skip_unused: bool = True, max_slots: Optional[int] = None,
                                 per_query: bool = True) -> Tuple[Dict, np.ndarray, Optional[np.ndarray]]:
    """fr_permutation_importance (include/fastrank.h).  features: ids (default: all of the view's, ascending).
    Returns (report, values, per_query): values[F, R] = the mean of `evaluator` with feature f permuted in repeat r; per_query
    [F * R + 1, nq] in evaluate_dense's query order, row f * R + r behind values[f, r], the last row the baseline's (None when
    per_query is False)."""
    options = {"repeats": int(repeats), "seed": int(seed), "scope": scope, "skip_unused": bool(skip_unused)}
    if features is not None:
        options["features"] = [int(f) for f in features]
    if max_slots is not None:
        options["max_slots"] = int(max_slots)
    F = len(options["features"]) if features is not None else len(dataset.feature_ids())
    R = int(repeats) if 0 < int(repeats) <= 64 else 0  # (out of range: refused by the call before it writes)
    nq = num_queries(dataset) if per_query and R else 0
    values = np.zeros((F, R), dtype=np.float64)
    rows = np.zeros((F * R + 1, nq), dtype=np.float64) if per_query and R else None
    rep = _json_reply(_load().fr_permutation_importance(model.pointer, dataset.pointer, None if qrel is None else qrel.pointer, evaluator.encode("utf-8"),
                                                        json.dumps(options).encode("utf-8"), values.ctypes.data if values.size else None, values.size,
                                                        rows.ctypes.data if rows is not None and rows.size else None))
    return rep, values, rows


def permutation_sources(dataset: CDataset, seed: int, repeat: int, scope: str = "dataset", n_total: Optional[int] = None) -> np.ndarray:
    """fr_debug_permutation_sources: uint32[n_total] by instance id, the instance whose value of a permuted feature each
    instance reads in repeat `repeat` (0xFFFFFFFF: not in the view).  Needs no device."""
    if n_total is None:
        held = [int(i) for ids in dataset.instances_by_query().values() for i in ids]
        n_total = max(held) + 1 if held else 0
    out = np.zeros(max(1, n_total), dtype=np.uint32)
    _json_reply(_load().fr_debug_permutation_sources(dataset.pointer, int(seed), int(repeat), scope.encode("utf-8"), out.ctypes.data, n_total))
    return out[:n_total]


def lambdamart_sample(dataset: CDataset, params, tree: int) -> Tuple[np.ndarray, np.ndarray]:
    """The sample LambdaMART's trainer uses for tree `tree` of `params` (LambdaMARTParams or its wire dict) on `dataset`:
    (feature ids ascending, indices of the view's queries ascending).  Needs no device."""
    wire = params if isinstance(params, dict) else params.to_dict()
    rep = _json_reply(_load().fr_debug_lambdamart_sample(dataset.pointer, json.dumps(wire).encode("utf-8"), int(tree)))
    return np.asarray(rep["features"], dtype=np.uint32), np.asarray(rep["queries"], dtype=np.uint32)


def lambdamart_dart_plan(params, num_trees: int) -> List[Dict]:
    """LambdaMART's DART plan ("DART") for the first `num_trees` trees of `params` (LambdaMARTParams or
    its wire dict): per tree {"dropped": the tree indices it is fitted without (ascending), "before": the weights of the
    earlier trees, "after": the weights including its own}.  Needs no device."""
    wire = params if isinstance(params, dict) else params.to_dict()
    rep = _json_reply(_load().fr_debug_lambdamart_dart_plan(json.dumps(wire).encode("utf-8"), int(num_trees)))
    return [{"dropped": [int(i) for i in r["dropped"]], "before": np.asarray(r["before"], dtype=np.float64),
             "after": np.asarray(r["after"], dtype=np.float64)} for r in rep]


def dart_scores(dataset: CDataset, model: CModel, weights, include, n_total: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """dart_rescore_kernel on its own: `model` is any Ensemble of DecisionTrees (its own weights are not read).  Fills the
    leaf cache for its trees, then forms s = sum over the trees `include` (ascending indices) of weights[t] * tree_t(x), the
    sequential unfused recurrence, once.  Returns (scores by instance id, NaN where the id is not part of a sampled dataset;
    the cache's rows uint16[trees, n] by instance id, 0xFFFF where the id is not part)."""
    n = int(n_total if n_total is not None else _load().fr_dataset_num_instances(dataset.pointer))
    if n_total is None and dataset.is_sampled():
        n = 1 + max(max(ids) for ids in dataset.instances_by_query().values())
    w = np.ascontiguousarray(weights, dtype=np.float64)
    inc = np.ascontiguousarray(include, dtype=np.uint32)
    scores = np.full(n, np.nan, dtype=np.float64)
    cache = np.full((len(w), n), 0xFFFF, dtype=np.uint16)
    _status(
        _load().fr_debug_dart_scores(
            dataset.pointer, model.pointer, w.ctypes.data if len(w) else None, len(w), inc.ctypes.data if len(inc) else None, len(inc),
            scores.ctypes.data, cache.ctypes.data, n,
        )
    )
    return scores, cache


def lambda_gradients(model: CModel, dataset: CDataset, measure: str = "ndcg", sigma: float = 1.0,
                     qrel: Optional[CQRel] = None, n_total: Optional[int] = None, queries=None,
                     truncation_level: int = 0, lambda_norm: bool = False, objective: str = "ndcg",
                     xe_key: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """LambdaMART's gradient pass on the scores of `model`: (lambda, weight) indexed by instance id (NaN where the id is
    not part of a sampled dataset).  `queries`: indices of the view's queries (its order) the pass visits, as for a tree's
    query sample; the instances of the others come back NaN.  `truncation_level` >= 1 / `lambda_norm`: the objective's
    options ("Truncation and normalisation"); `objective`: "ndcg", "map" or "mrr" (section 11,
    "Objectives"; `measure` must name NDCG all the same, and the norms are the AP / RR evaluator's) or "xendcg" (section 11,
    "Listwise objective": the listwise pass under the tree key `xe_key`, a u64; `sigma` and the measure's depth are not read,
    a truncation level or `lambda_norm` is refused).  At their defaults the call is the one it was."""
    n = int(n_total if n_total is not None else _load().fr_dataset_num_instances(dataset.pointer))
    if n_total is None and dataset.is_sampled():
        n = 1 + max(max(ids) for ids in dataset.instances_by_query().values())
    lam = np.full(n, np.nan, dtype=np.float64)
    wt = np.full(n, np.nan, dtype=np.float64)
    if int(truncation_level) != 0 or bool(lambda_norm) or objective != "ndcg":
        qs = None if queries is None else np.ascontiguousarray(queries, dtype=np.uint32)
        opts = {"truncation_level": int(truncation_level), "lambda_norm": bool(lambda_norm)}
        if objective != "ndcg":
            opts["objective"] = objective
        if objective == "xendcg":
            opts["xe_key"] = int(xe_key)
        opts = json.dumps(opts)
        _status(
            _load().fr_debug_lambda_gradients_opts(
                model.pointer, dataset.pointer, None if qrel is None else qrel.pointer, measure.encode("utf-8"), float(sigma),
                None if qs is None else qs.ctypes.data, 0 if qs is None else len(qs), opts.encode("utf-8"),
                lam.ctypes.data, wt.ctypes.data, n,
            )
        )
        return lam, wt
    if queries is not None:
        qs = np.ascontiguousarray(queries, dtype=np.uint32)
        _status(
            _load().fr_debug_lambda_gradients_sampled(
                model.pointer, dataset.pointer, None if qrel is None else qrel.pointer, measure.encode("utf-8"), float(sigma),
                qs.ctypes.data, len(qs), lam.ctypes.data, wt.ctypes.data, n,
            )
        )
        return lam, wt
    _status(
        _load().fr_debug_lambda_gradients(
            model.pointer, dataset.pointer, None if qrel is None else qrel.pointer, measure.encode("utf-8"), float(sigma),
            lam.ctypes.data, wt.ctypes.data, n,
        )
    )
    return lam, wt


def hist_bins(dataset: CDataset, split_candidates: int):
    """The histogram grower's bins of a dataset view: (instance list ids[n], feature ids[f] ascending, edges: a list of f
    float32 arrays, bins uint8[f, n] over the instance list)."""
    n = sum(len(ids) for ids in dataset.instances_by_query().values())
    f = len(dataset.feature_ids())
    ids = np.zeros(n, dtype=np.uint32)
    feats = np.zeros(f, dtype=np.uint32)
    edges = np.zeros((f, 256), dtype=np.float32)
    nedges = np.zeros(f, dtype=np.uint32)
    bins = np.zeros((f, n), dtype=np.uint8)
    _status(
        _load().fr_debug_hist_bins(
            dataset.pointer, int(split_candidates), n, f, ids.ctypes.data, feats.ctypes.data, edges.ctypes.data,
            nedges.ctypes.data, bins.ctypes.data,
        )
    )
    return ids, feats, [edges[s, : nedges[s]].copy() for s in range(f)], bins


def hist_tree(dataset: CDataset, lam: np.ndarray, wt: np.ndarray, split_candidates: int, max_depth: int,
              min_leaf_support: int, queries=None, features=None, split_gain: str = "variance", lambda_l2: float = 0.0,
              min_sum_hessian: float = 0.0, min_split_gain: float = 0.0, max_leaves: int = 0, monotone=None,
              clamped_out: Optional[list] = None, goss=None, symmetric: bool = False, lambda_l1: float = 0.0,
              max_delta_step: float = 0.0, path_smooth: float = 0.0, quant=None) -> CModel:
    """One tree of LambdaMART's histogram grower for the gradients lam / wt (indexed by instance id).  `queries` (indices of
    the view's queries) / `features` (feature ids): the tree's sample; gradients outside the query sample are not read.
    `split_gain` = "newton": the second-order gain with `lambda_l2`, `min_sum_hessian` and `min_split_gain` (DESIGN.md
    section 11, "Newton split gain").  `max_leaves` >= 2: the tree is grown leaf-wise under that leaf budget (DESIGN.md
    section 11, "Leaf-wise growth"), 0: level-wise.  `monotone` = {feature id: sign in -1, 0, +1} with some non-zero sign
    (needs `split_gain` = "newton"): the tree is grown under monotone constraints ("Monotone
    constraints"), level-wise or leaf-wise, and the number of leaves a bound moved is appended to `clamped_out` when that is
    a list.  `goss` = (top_rate, other_rate, seed, tree) (needs `split_gain` = "newton"): the tree is fitted to the GOSS list
    of the sample's instances under the key of tree `tree` of `seed`, the kept others' gradients amplified (DESIGN.md section
    11, "GOSS"); level-wise or leaf-wise, with or without monotone signs.  `symmetric` = True (level-wise, without monotone
    signs or GOSS): every node of a level splits on the level's one winning candidate ("Symmetric
    trees"), under either gain.  `lambda_l1`, `max_delta_step`, `path_smooth` (need `split_gain` = "newton"; `path_smooth` not
    with `symmetric`): the leaf regularisation ("Leaf regularisation"); all 0.0: off.  `quant` = (bits, seed, tree) (needs
    `split_gain` = "newton"; no monotone sign, no leaf regularisation): the searches read gradients quantised to `bits` bits
    (2..8) under the key of tree `tree` of `seed`, the leaves are renewed from the full-precision sums (DESIGN.md section 11,
    "Quantised gradients").  Arguments that contradict each other raise ValueError before the one native call."""
    lam = np.ascontiguousarray(lam, dtype=np.float64)
    wt = np.ascontiguousarray(wt, dtype=np.float64)
    newton = split_gain == "newton"
    mono = {} if monotone is None else {int(f): int(c) for f, c in monotone.items()}
    if not any(c != 0 for c in mono.values()):
        mono = {}
    if lam.shape != wt.shape or lam.ndim != 1:
        raise ValueError("lam and wt must be 1-d arrays of the same length")
    if split_gain not in ("variance", "newton"):
        raise ValueError("split_gain must be 'variance' or 'newton', not {!r}".format(split_gain))
    if symmetric and (goss is not None or int(max_leaves) != 0 or mono):
        raise ValueError("symmetric trees are grown level-wise, without monotone constraints or goss")
    if goss is not None and not newton:
        raise ValueError("goss needs split_gain='newton'")
    if mono and not newton:
        raise ValueError("monotone constraints need split_gain='newton'")
    if int(max_leaves) != 0 and int(max_leaves) < 2:
        raise ValueError("max_leaves must be 0 (level-wise) or at least 2")
    if not newton and (lambda_l2 != 0.0 or min_sum_hessian != 0.0 or min_split_gain != 0.0):
        raise ValueError("lambda_l2, min_sum_hessian and min_split_gain need split_gain='newton'")
    reg = (float(lambda_l1), float(max_delta_step), float(path_smooth))
    if any(not (math.isfinite(x) and x >= 0.0) for x in reg):
        raise ValueError("lambda_l1, max_delta_step and path_smooth must be finite and at least 0")
    if not newton and any(x != 0.0 for x in reg):
        raise ValueError("lambda_l1, max_delta_step and path_smooth need split_gain='newton'")
    if symmetric and reg[2] != 0.0:
        raise ValueError("symmetric trees take no path_smooth")
    quant_bits, quant_seed, quant_tree = (0, 0, 0) if quant is None else (int(x) for x in quant)
    if quant is not None and not 2 <= quant_bits <= 8:
        raise ValueError("quant bits must be between 2 and 8")
    if quant is not None and (not newton or mono or any(x != 0.0 for x in reg)):
        raise ValueError("quant needs split_gain='newton', and takes no monotone constraints or leaf regularisation")
    qs = None if queries is None else np.ascontiguousarray(queries, dtype=np.uint32)
    fs = None if features is None else np.ascontiguousarray(features, dtype=np.uint32)
    mf = np.ascontiguousarray(list(mono.keys()), dtype=np.uint32)
    ms = np.ascontiguousarray(list(mono.values()), dtype=np.int32)
    top_rate, other_rate, seed, tree = (0.0, 0.0, 0, 0) if goss is None else goss
    opt = HistTreeOptions(
        split_candidates=int(split_candidates), max_depth=int(max_depth), min_leaf_support=int(min_leaf_support),
        newton=1 if newton else 0, lambda_l2=float(lambda_l2), min_sum_hessian=float(min_sum_hessian),
        min_split_gain=float(min_split_gain), max_leaves=int(max_leaves), symmetric=1 if symmetric else 0,
        queries=None if qs is None else qs.ctypes.data, n_queries=0 if qs is None else len(qs),
        features=None if fs is None else fs.ctypes.data, n_features=0 if fs is None else len(fs),
        mono_features=mf.ctypes.data if mono else None, mono_signs=ms.ctypes.data if mono else None, n_mono=len(mono),
        goss=0 if goss is None else 1, top_rate=float(top_rate), other_rate=float(other_rate), seed=int(seed), tree=int(tree),
        lambda_l1=reg[0], max_delta_step=reg[1], path_smooth=reg[2], quant_bits=quant_bits, quant_seed=quant_seed, quant_tree=quant_tree,
    )
    clamped = C.c_uint32(0)
    model = CModel(
        _unwrap(_load().fr_debug_hist_tree(dataset.pointer, C.byref(opt), lam.ctypes.data, wt.ctypes.data, lam.shape[0], C.byref(clamped)))
    )
    if mono and clamped_out is not None:
        clamped_out.append(int(clamped.value))
    return model


def hist_reg_term(q: int, w: int, n: int, s_l: int, s_w: int, l1: float, l2: float, mds: float, smooth: float, parent, lo: float,
                  hi: float) -> Tuple[float, float]:
    """(v, term) of the leaf regularisation ("Leaf regularisation") for the integer sums (q, w) of a
    node or side of n instances under the exponents s_l / s_w: the host's own arithmetic, no device is touched.  `parent`:
    the parent's output, or None for the root; [lo, hi]: the node's interval."""
    v, term = C.c_double(0.0), C.c_double(0.0)
    _status(
        _load().fr_debug_hist_reg_term(
            int(q), int(w), int(n), int(s_l), int(s_w), float(l1), float(l2), float(mds), float(smooth), 0 if parent is None else 1,
            0.0 if parent is None else float(parent), float(lo), float(hi), C.byref(v), C.byref(term),
        )
    )
    return v.value, term.value


def goss_select(dataset: CDataset, lam: np.ndarray, top_rate: float, other_rate: float, seed: int, tree: int,
                queries=None) -> Tuple[np.ndarray, np.ndarray, int]:
    """LambdaMART's GOSS selection on its own ("GOSS") for the gradients `lam` (by instance id) under
    the key of tree `tree` of `seed`; `queries` (indices of the view's queries): the tree's query sample, whose instances are
    the list the selection runs over.  Returns (the GOSS list as ascending indices into the view's instance list, per entry
    whether it belongs to the top set, tau: the n_top-th largest 64-bit pattern of |lambda|)."""
    lam = np.ascontiguousarray(lam, dtype=np.float64)
    n = sum(len(ids) for ids in dataset.instances_by_query().values())
    qs = None if queries is None else np.ascontiguousarray(queries, dtype=np.uint32)
    rows = np.zeros(n, dtype=np.uint32)
    top = np.zeros(n, dtype=np.uint8)
    n_g = C.c_uint32(0)
    tau = C.c_uint64(0)
    _status(
        _load().fr_debug_goss_select(
            dataset.pointer, lam.ctypes.data, lam.shape[0], float(top_rate), float(other_rate), int(seed), int(tree),
            None if qs is None else qs.ctypes.data, 0 if qs is None else len(qs), rows.ctypes.data, top.ctypes.data, n,
            C.byref(n_g), C.byref(tau),
        )
    )
    return rows[: n_g.value].copy(), top[: n_g.value].astype(bool), int(tau.value)


def hist_quantise(dataset: CDataset, lam: np.ndarray, wt: np.ndarray, bits: int, seed: int, tree: int, queries=None, goss=None) -> dict:
    """The fixed-point step and the quantised gradients of one tree on their own ("Quantised
    gradients") for lam / wt (by instance id) under the key of tree `tree` of `seed`.  `queries` (indices of the view's
    queries): the tree's query sample; `goss` = (top_rate, other_rate, seed, tree): the tree's list is the GOSS list of the
    sample's instances, its values the amplified ones.  Returns dict(q, w: int64 arrays by index of the tree's list; s_l, s_w:
    the exponents S and S_w; search_s_l, search_s_w: S - d and S_w - d_w; d, d_w: the two shifts)."""
    lam = np.ascontiguousarray(lam, dtype=np.float64)
    wt = np.ascontiguousarray(wt, dtype=np.float64)
    if lam.shape != wt.shape or lam.ndim != 1:
        raise ValueError("lam and wt must be 1-d arrays of the same length")
    n = sum(len(ids) for ids in dataset.instances_by_query().values())
    qs = None if queries is None else np.ascontiguousarray(queries, dtype=np.uint32)
    top_rate, other_rate, goss_seed, goss_tree = (0.0, 0.0, 0, 0) if goss is None else goss
    q = np.zeros(n, dtype=np.int32)
    w = np.zeros(n, dtype=np.uint32)
    n_out = C.c_uint32(0)
    numbers = np.zeros(6, dtype=np.int32)
    _status(
        _load().fr_debug_hist_quantise(
            dataset.pointer, lam.ctypes.data, wt.ctypes.data, lam.shape[0], int(bits), int(seed), int(tree),
            None if qs is None else qs.ctypes.data, 0 if qs is None else len(qs), 0 if goss is None else 1, float(top_rate), float(other_rate),
            int(goss_seed), int(goss_tree), q.ctypes.data, w.ctypes.data, n, C.byref(n_out), numbers.ctypes.data,
        )
    )
    names = ("s_l", "s_w", "search_s_l", "search_s_w", "d", "d_w")
    out = {k: int(v) for k, v in zip(names, numbers)}
    out["q"], out["w"] = q[: n_out.value].astype(np.int64), w[: n_out.value].astype(np.int64)
    return out


def hist_root_histogram(dataset: CDataset, lam: np.ndarray, wt: np.ndarray, split_candidates: int, quant=None, features=None):
    """The root's histogram of one tree over every instance of the view, for lam / wt (by instance id): (count, sum Q, sum W)
    as int64 arrays [features][split_candidates].  `quant` = (bits, seed, tree): the packed build over the quantised values
    ("Quantised gradients"); None: the Newton build over the fixed-point values.  `features` (feature
    ids): the tree's feature sample."""
    lam = np.ascontiguousarray(lam, dtype=np.float64)
    wt = np.ascontiguousarray(wt, dtype=np.float64)
    if lam.shape != wt.shape or lam.ndim != 1:
        raise ValueError("lam and wt must be 1-d arrays of the same length")
    bits, seed, tree = (0, 0, 0) if quant is None else (int(x) for x in quant)
    if quant is not None and not 2 <= bits <= 8:
        raise ValueError("quant bits must be between 2 and 8")
    fs = None if features is None else np.ascontiguousarray(features, dtype=np.uint32)
    F = len(dataset.feature_ids()) if fs is None else len(fs)
    k = int(split_candidates)
    cnt = np.zeros(F * k, dtype=np.uint32)
    qs = np.zeros(F * k, dtype=np.int64)
    ws = np.zeros(F * k, dtype=np.int64)
    _status(
        _load().fr_debug_hist_root_histogram(
            dataset.pointer, lam.ctypes.data, wt.ctypes.data, lam.shape[0], k, bits, seed, tree, None if fs is None else fs.ctypes.data,
            0 if fs is None else len(fs), cnt.ctypes.data, qs.ctypes.data, ws.ctypes.data, F * k,
        )
    )
    return cnt.astype(np.int64).reshape(F, k), qs.reshape(F, k), ws.reshape(F, k)


def rank_order(model: CModel, dataset: CDataset) -> Tuple[np.ndarray, np.ndarray]:
    """(instance ids grouped by query, best first; offsets[nq+1]) under the reference's
    (score desc, gain asc, id asc) order."""
    nq = num_queries(dataset)
    n = int(_load().fr_dataset_num_instances(dataset.pointer))
    ids = np.zeros(n, dtype=np.uint32)
    offs = np.zeros(nq + 1, dtype=np.uint64)
    _status(_load().fr_rank_order(model.pointer, dataset.pointer, ids.ctypes.data, n, offs.ctypes.data, nq + 1))
    return ids, offs


def evaluate_candidates(dataset: CDataset, evaluator: str, features, base_weights, candidates: List,
                        qrel: Optional[CQRel] = None, per_query: bool = False):
    """Batched evaluate_mean for line-search candidates.  features[g], base_weights[g][d],
    candidates[g] = list of <=64 values for w[features[g]].  Returns means as a list of arrays
    (and, if per_query, the [nq][G*64] matrix)."""
    G = len(features)
    feats = np.ascontiguousarray(features, dtype=np.uint32)
    base = np.ascontiguousarray(base_weights, dtype=np.float64)
    assert base.ndim == 2 and base.shape[0] == G
    ncand = np.asarray([len(c) for c in candidates], dtype=np.uint32)
    cand = np.zeros((G, 64), dtype=np.float64)
    for g, c in enumerate(candidates):
        cand[g, : len(c)] = c
    means = np.zeros((G, 64), dtype=np.float64)
    pq = np.zeros((num_queries(dataset), G * 64), dtype=np.float64) if per_query else None
    _status(
        _load().fr_evaluate_candidates(
            dataset.pointer, None if qrel is None else qrel.pointer, evaluator.encode("utf-8"), G,
            feats.ctypes.data, base.ctypes.data, ncand.ctypes.data, cand.ctypes.data, means.ctypes.data,
            None if pq is None else pq.ctypes.data,
        )
    )
    out = [means[g, : ncand[g]].copy() for g in range(G)]
    return (out, pq) if per_query else out


def profile_enable(on: bool = True) -> None:
    _load().fr_profile_enable(1 if on else 0)


def profile_reset() -> None:
    _load().fr_profile_reset()


def profile_stats() -> Dict[str, Dict[str, float]]:
    """{kernel: {"launches", "total_ms", "avg_ms"}} measured with HIP events on the launch stream."""
    rows = _json_reply(_load().fr_profile_json())
    return {
        r["kernel"]: {"launches": r["launches"], "total_ms": r["total_ms"],
                      "avg_ms": r["total_ms"] / max(1, r["launches"])}
        for r in rows
    }


# RfCandDev of csrc/kernels_rf.inc (48 bytes), as the device writes it
RF_CAND_DTYPE = np.dtype([("position", "<f8"), ("importance", "<f8"), ("ids_i", "<u4"), ("flags", "<u4"), ("pos_l", "<u4"), ("pos_r", "<u4"),
                          ("sum_l", "<f8"), ("sum_r", "<f8")])
RF_ACTIVE_DTYPE = np.dtype([("tree", "<u4"), ("key", "<u4"), ("n", "<u4")])
RF_SPLIT_DTYPE = np.dtype([("fslot", "<i4"), ("pos", "<u4"), ("left", "<u4"), ("right", "<u4")])
RF_SPLIT_METHODS = ("SquaredError", "BinaryGiniImpurity", "InformationGain", "TrueVarianceReduction")


def rf_levels(dataset: CDataset, root_off, root_ids, feats, split_candidates: int, split_method: int, min_leaf_support: int,
              max_depth: int) -> Dict:
    """One batch of random-forest trees grown by the trainer's own level loop with every level recorded (fr_debug_rf_levels;
    DESIGN.md section 5.6).  Tree t grows over the instance ids root_ids[root_off[t]:root_off[t + 1]], in that order, and the
    features feats[t] (T x nf).  Returns {"levels": [per level: active (tree, key, n), depth, label_minmax [A, 2], cands
    [A, nf, k - 1] (RF_CAND_DTYPE), svals / sv / sg [items], splits [A], child_out [A, 2], children_from], "root_out": [T] or
    empty, "trees": the DecisionTree dicts}."""
    L = _load()
    off = np.ascontiguousarray(root_off, dtype=np.uint32)
    ids = np.ascontiguousarray(root_ids, dtype=np.uint32)
    fl = np.ascontiguousarray(feats, dtype=np.uint32)
    T = len(off) - 1
    if fl.ndim != 2 or fl.shape[0] != T or len(ids) != int(off[-1]):
        raise ValueError("rf_levels: feats must be [trees][nf] and root_ids as long as root_off says")
    nf, k = fl.shape[1], int(split_candidates)
    if RF_CAND_DTYPE.itemsize != 48:
        raise RuntimeError("rf_levels: the candidate record is not 48 bytes")
    head = _json_reply(L.fr_debug_rf_levels(dataset.pointer, off.ctypes.data, T, ids.ctypes.data, fl.ctypes.data, nf, k, int(split_method),
                                            int(min_leaf_support), int(max_depth), None, 0))
    if head["cand_bytes"] != RF_CAND_DTYPE.itemsize:
        raise RuntimeError("rf_levels: the library's candidate record is not the one this module describes")
    blob = np.zeros(max(int(head["bytes"]), 1), dtype=np.uint8)
    _json_reply(L.fr_debug_rf_levels(None, None, 0, None, None, 0, 0, 0, 0, 0, blob.ctypes.data, int(head["bytes"])))
    dtypes = {"active": RF_ACTIVE_DTYPE, "depth": np.uint32, "label_minmax": np.float32, "cands": RF_CAND_DTYPE, "svals": np.uint32,
              "sv": np.float32, "sg": np.float32, "splits": RF_SPLIT_DTYPE, "child_out": np.float64, "root_out": np.float64}
    levels = [dict(children_from=l["children_from"]) for l in head["levels"]]
    root_out = np.zeros(0)
    for s in head["sections"]:
        arr = blob[s["offset"]:s["offset"] + s["bytes"]].copy().view(dtypes[s["name"]])
        if s["name"] == "root_out":
            root_out = arr
            continue
        A = head["levels"][s["level"]]["A"]
        if s["name"] in ("label_minmax", "child_out"):
            arr = arr.reshape(A, 2)
        elif s["name"] == "cands":
            arr = arr.reshape(A, nf, max(k - 1, 0))
        levels[s["level"]][s["name"]] = arr
    return {"levels": levels, "root_out": root_out, "trees": [t["DecisionTree"] for t in head["trees"]]}


def last_train_stats() -> Dict:
    return _json_reply(_load().fr_last_train_stats())


def last_load_stats() -> Dict:
    """What the last CDataset.open_ranksvm of this process did (fr_last_load_stats): "parser" that ran and "reason", "bytes",
    "lines", "host_lines", "host_line_reasons", "seconds" per stage, and the parser's constants "scan_slice", "stage_limit",
    "auto_threshold"."""
    return _json_reply(_load().fr_last_load_stats())


def loaded_arrays(dataset: CDataset) -> Dict:
    """The host arrays of a file-loaded dataset, or of one Normalizer.apply made (fr_debug_dataset_core), for the tests: x
    (n x d), gain, qix, qnames, docids, doc_present (empty for a dataset without document ids), features, present_bits,
    present_words, has_docids.  qnames / docids are bytes (a comment need not be UTF-8)."""
    L = _load()
    s = _json_reply(L.fr_debug_dataset_core(dataset.pointer, None, None, 0))
    n, d = int(s["n"]), int(s["d"])
    out = {"n": n, "d": d, "present_words": int(s["present_words"]), "has_docids": bool(s["has_docids"]),
           "qnames": [bytes.fromhex(h) for h in s["qnames_hex"]], "docids": [bytes.fromhex(h) for h in s["docids_hex"]]}
    for name, dtype, count in (("x", np.float32, n * d), ("gain", np.float32, n), ("qix", np.uint32, n), ("doc_present", np.uint8, int(s["doc_present_len"])),
                               ("features", np.uint32, int(s["features_len"])), ("present_bits", np.uint32, int(s["present_bits_len"]))):
        arr = np.empty(count, dtype=dtype)
        _json_reply(L.fr_debug_dataset_core(dataset.pointer, name.encode("utf-8"), arr.ctypes.data if count else None, arr.nbytes))
        out[name] = arr
    out["x"] = out["x"].reshape(n, d)
    return out


def text_numbers(tokens: List[str]):
    """The device parser's number rule as the library's host compile runs it (fr_debug_text_number): (reason names per token,
    float64 values, float32 values); a value is meaningful where the reason is "none".  Tokens hold no newline."""
    n = len(tokens)
    reasons, v64, v32 = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.float32)
    rep = _json_reply(_load().fr_debug_text_number("\n".join(tokens).encode("utf-8"), n, reasons.ctypes.data, v64.ctypes.data, v32.ctypes.data))
    return [rep["reasons"][r] for r in reasons], v64, v32


def last_tree_plan() -> Dict:
    """What the last forest-scoring call of this process ran (fr_debug_tree_plan): {"path": "rank" | "lds" | "l2",
    "cache_hit", and per path "docs", "parts" / "rows_in_lds" / "nslots", "nrounds"; "batches": [[walks, levels], ...]}."""
    return _json_reply(_load().fr_debug_tree_plan())


_FOREST_TABLE_DTYPES = {"fdesc": np.uint32, "tables": np.float32, "rdesc": np.uint32, "desc": np.uint32, "leafprod": np.float64,
                        "roots": np.int32, "tweights": np.float64,
                        "nodes": np.dtype([("split", np.float64), ("fid", np.int32), ("lhs", np.int32)])}


def forest_pack(model: CModel, dataset_features: int, encoding: str) -> Dict:
    """fr_debug_forest_pack: the forest of `model` packed on the host (no device) for encoding "rank", "lds:DOCS,PARTS" or
    "l2" on a dataset of dataset_features features: the hook's JSON, its "tables" read back as numpy arrays ("forest": uint32
    words for "rank", uint64 words for an LDS shape)."""
    L, enc = _load(), encoding.encode("utf-8")
    rep = _json_reply(L.fr_debug_forest_pack(model.pointer, int(dataset_features), enc, None, None, 0))
    sizes, rep["tables"] = rep["tables"], {}
    for name, nbytes in sizes.items():
        dtype = np.dtype(_FOREST_TABLE_DTYPES.get(name, np.uint32 if encoding == "rank" else np.uint64))
        arr = np.zeros(int(nbytes) // dtype.itemsize, dtype=dtype)
        _json_reply(L.fr_debug_forest_pack(model.pointer, int(dataset_features), enc, name.encode("utf-8"), arr.ctypes.data if arr.size else None, arr.nbytes))
        rep["tables"][name] = arr
    return rep


def last_metric_plan() -> Dict:
    """What the last general metric pass of this process launched (fr_debug_metric_plan): {"measure", "depth", "slots",
    "classes": [{"npad", "queries", "kernel": "sort" | "topk"}, ...]}; {"measure": None} before the first one."""
    return _json_reply(_load().fr_debug_metric_plan())


def measure_ranked(evaluator: str, gains, norm: float = 0.0) -> float:
    """The library's scalar definition (csrc/measures_host.hpp) of dcg[@k], precision@k, recall[@k], success@k or err[@k] over a
    ranked list of gains, on the host; norm: precision: k, recall: the number of relevant documents (0: the list's own), err:
    2^(largest gain)."""
    g = np.ascontiguousarray(gains, dtype=np.float32)
    out = np.zeros(1, dtype=np.float64)
    _status(_load().fr_debug_measure_ranked(evaluator.encode("utf-8"), g.ctypes.data, len(g), float(norm), out.ctypes.data))
    return float(out[0])


def metric_topk_pays(depth: int, npad: int) -> bool:
    """The routing rule of the general metric pass: does a size class of npad documents go to the selection kernel at this
    cut-off?"""
    return bool(_load().fr_debug_metric_topk_pays(int(depth), int(npad)))


def train_model_shard(dataset: CDataset, train_req, restart_begin: int, restart_end: int) -> Dict:
    """Train restarts [begin, end) of the request on this process's GPU."""
    request = json.dumps(train_req.to_dict()).encode("utf-8")
    return _json_reply(_load().fr_train_model_shard(request, dataset.pointer, restart_begin, restart_end))


class CoordinateAscentRun:
    """Steppable coordinate ascent on this process's GPU (fr_ca_begin / fr_ca_step / fr_ca_state).
    One tick = one fused launch over every candidate of every live restart's line search."""

    def __init__(self, dataset: CDataset, train_req, restart_begin: int = 0, restart_end: Optional[int] = None):
        if restart_end is None:
            restart_end = int(train_req.params.num_restarts)
        err = C.c_void_p()
        request = json.dumps(train_req.to_dict()).encode("utf-8")
        self.pointer = _load().fr_ca_begin(request, dataset.pointer, restart_begin, restart_end, C.byref(err))
        if not self.pointer:
            _status(err.value)
            raise RuntimeError("fr_ca_begin failed")
        self._dataset = dataset  # keep the dataset (and its numpy buffers) alive
        self.finished = False

    def step(self, ticks: int) -> int:
        done = C.c_uint64(0)
        fin = C.c_int(0)
        _status(_load().fr_ca_step(self.pointer, int(ticks), C.byref(done), C.byref(fin)))
        self.finished = bool(fin.value)
        return int(done.value)

    def state(self) -> Dict:
        return _json_reply(_load().fr_ca_state(self.pointer))

    def capture(self, on: bool = True) -> None:
        """Tick capture (fr_ca_capture, a test hook): while on, every store of exact resident sums and every collected
        line search of this trainer's device dataset is logged; take_capture() hands the log over."""
        _status(_load().fr_ca_capture(self.pointer, 1 if on else 0))

    def take_capture(self) -> List[Dict]:
        """The events logged since the last call, oldest first (fr_ca_capture_take), arrays as numpy:
        {"type": "store", "slot", "v"} and {"type": "tick", "ctx", "kind", "measure", "depth", "groups" (every LineGroup
        field, the caller's order), "gorder", "nverify", "approx", "resident", "ready", "inst", "redo", "redo_groups",
        "means", "matrix" ([nq, ldm] in staged order, or None), "resident_sums" ({slot: [np]})}."""
        L = _load()
        head = _json_reply(L.fr_ca_capture_take(self.pointer, None, None, 0))
        blob = np.zeros(int(head["bytes"]), dtype=np.uint8)
        _json_reply(L.fr_ca_capture_take(self.pointer, b"blob", blob.ctypes.data if blob.size else None, blob.nbytes))

        def arr(ref, dtype):
            dt = np.dtype(dtype)
            return np.frombuffer(blob, dtype=dt, count=int(ref["n"]), offset=int(ref["off"])).copy()

        out = []
        for ev in head["events"]:
            if ev["type"] == "store":
                out.append({"type": "store", "slot": int(ev["slot"]), "v": arr(ev["v"], np.float64)})
                continue
            groups = []
            for g in ev["groups"]:
                par = arr(g["params"], np.float64)
                groups.append({"feature": int(g["feature"]), "weights": arr(g["weights"], np.float64),
                               "candidates": arr(g["candidates"], np.float64), "resident_slot": int(g["resident_slot"]),
                               "resident_owner": int(g["resident_owner"]), "has_update": bool(g["has_update"]),
                               "upd_feature": int(g["upd_feature"]), "resident_norm": float(par[0]),
                               "resident_base_f": float(par[1]), "resident_err": float(par[2]), "upd_norm": float(par[3]),
                               "upd_base_f": float(par[4]), "upd_cand": float(par[5])})
            inst = dict(ev["inst"])
            if "classes" in inst:
                inst["classes"] = arr(inst["classes"], np.uint32).reshape(-1, 3).tolist()
            nq, ldm, npos = int(ev["nq"]), int(ev["ldm"]), int(ev["np"])
            slots = arr(ev["res_slots"], np.int32)
            res = arr(ev["res"], np.float64).reshape(len(slots), npos) if len(slots) else np.zeros((0, npos))
            out.append({"type": "tick", "ctx": int(ev["ctx"]), "kind": ev["kind"], "measure": int(ev["measure"]),
                        "depth": int(ev["depth"]), "groups": groups, "gorder": arr(ev["gorder"], np.uint32),
                        "nverify": int(ev["nverify"]), "approx": bool(ev["approx"]), "resident": bool(ev["resident"]),
                        "ready": bool(ev["ready"]), "inst": inst, "redo": arr(ev["redo"], np.uint32),
                        "redo_groups": int(ev["redo_groups"]), "means": arr(ev["means"], np.float64),
                        "matrix": arr(ev["matrix"], np.float64).reshape(nq, ldm) if ev["has_matrix"] else None,
                        "resident_sums": {int(s): res[i] for i, s in enumerate(slots)}})
        return out

    def close(self):
        if self.pointer:
            _load().fr_ca_free(self.pointer)
            self.pointer = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def rank_ordered_sum(values: "np.ndarray", group=None) -> "np.ndarray":
    """Sum of a float64 vector over all ranks, added in rank order, so every rank gets the same
    bits (a ring all-reduce does not promise that).  One all_gather of len(values) doubles over
    RCCL/xGMI (backend "nccl") or gloo."""
    import torch
    import torch.distributed as dist

    if not dist.is_available() or not dist.is_initialized() or dist.get_world_size(group) == 1:
        return np.array(values, dtype=np.float64)
    backend = dist.get_backend(group)
    dev = torch.device("cuda", torch.cuda.current_device()) if backend == "nccl" else torch.device("cpu")
    mine = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64)).to(dev)
    parts = [torch.empty_like(mine) for _ in range(dist.get_world_size(group))]
    dist.all_gather(parts, mine, group=group)
    total = parts[0].cpu().numpy().copy()
    for t in parts[1:]:
        total = total + t.cpu().numpy()
    return total


class QueryShardedRun(CoordinateAscentRun):
    """Coordinate ascent with the QUERIES sharded over the ranks (the fallback for runs
    with fewer restarts than GPUs): `dataset` is this rank's block of queries, every rank runs all
    restarts in lock step, and after each device evaluation the per-candidate sums are combined with
    rank_ordered_sum (<= 13 KB per tick).  Every rank ends with identical restarts."""

    def __init__(self, dataset: CDataset, train_req, total_queries: Optional[int] = None, group=None):
        local_q = num_queries(dataset)
        if total_queries is None:
            total_queries = int(rank_ordered_sum(np.array([float(local_q)]), group)[0])

        def reduce_cb(_ctx, values, n):
            try:
                arr = np.ctypeslib.as_array(values, shape=(n,))
                arr[:] = rank_ordered_sum(arr, group)
                return 0
            except Exception as exc:  # surfaces as an error envelope from fr_ca_step
                self._callback_error = exc
                return 1

        self._callback_error = None
        self._callback = ALLREDUCE_SUM_FN(reduce_cb)  # keep alive as long as the trainer
        err = C.c_void_p()
        request = json.dumps(train_req.to_dict()).encode("utf-8")
        self.pointer = _load().fr_ca_begin_query_shard(request, dataset.pointer, int(total_queries), self._callback, None, C.byref(err))
        if not self.pointer:
            _status(err.value)
            raise RuntimeError("fr_ca_begin_query_shard failed")
        self._dataset = dataset
        self.finished = False
        self.total_queries = int(total_queries)


def train_model_query_sharded(dataset: CDataset, train_req, total_queries: Optional[int] = None, group=None) -> CModel:
    """Trains on query shards: call on every rank with that rank's block of queries (e.g.
    `full.subsample_queries(my_qids)` or a per-rank file).  Returns the same model on every rank."""
    run = QueryShardedRun(dataset, train_req, total_queries, group)
    try:
        while not run.finished:
            run.step(1 << 20)
        restarts = run.state()["restarts"]
    finally:
        run.close()
    model = select_model(restarts, bool(train_req.params.output_ensemble))
    model.params = train_req
    return model


def select_model(restarts: List[Dict], output_ensemble: bool = False) -> CModel:
    """src/coordinate_ascent.rs:232-252 over gathered restarts (last maximum wins ties)."""
    payload = json.dumps(restarts).encode("utf-8")
    return CModel(_unwrap(_load().fr_select_model(payload, 1 if output_ensemble else 0)))


def device_plan(devices: str, device_count: int, num_restarts: int, primary_device: int = 0) -> Dict:
    """How the library's own train_model would spread a request over the devices of FR_DEVICES=`devices` (no device needed)."""
    return _json_reply(_load().fr_debug_device_plan(devices.encode("utf-8"), device_count, num_restarts, primary_device))


def restart_queue_replay(num_restarts: int, n_workers: int, capacity: int, lengths) -> Dict:
    """The library's restart queue replayed without a device (fr_debug_restart_queue): which worker starts which restart
    ids, in which order, when restart r converges after lengths[r % len(lengths)] ticks."""
    arr = np.ascontiguousarray(lengths, dtype=np.uint32)
    return _json_reply(_load().fr_debug_restart_queue(int(num_restarts), int(n_workers), int(capacity), arr.ctypes.data, len(arr)))


def peer_copy(src_device: int, dst_device: int, nbytes: int = 256 << 20) -> Dict:
    """One timed device-to-device copy made like train_model's dataset copies: {"can_access", "enabled", "ms", "gbps", ...}."""
    return _json_reply(_load().fr_debug_peer_copy(int(src_device), int(dst_device), int(nbytes)))


def pack_restart_records(restarts: List[Dict], cap: int, dim: int) -> "np.ndarray":
    """A rank's restarts as the fixed-size block of the job's one exchange: `cap` records of 3 + dim doubles -- valid, restart
    id, score, weights (include/fastrank.h: fr_pack_restart_records; the library's own multi-device train_model packs with the
    same code)."""
    out = np.zeros((int(cap), 3 + int(dim)), dtype=np.float64)
    _status(_load().fr_pack_restart_records(json.dumps(restarts).encode("utf-8"), int(cap), int(dim), out.ctypes.data))
    return out


def unpack_restart_records(records: "np.ndarray", dim: int) -> List[Dict]:
    """The valid records of any number of blocks, as restarts in restart order."""
    arr = np.ascontiguousarray(records, dtype=np.float64).reshape(-1, 3 + int(dim))
    return _json_reply(_load().fr_unpack_restart_records(arr.ctypes.data, arr.shape[0], int(dim)))


def rccl_allgather_restarts(devices: List[int], parts: List[List[Dict]]) -> Tuple[Dict, Optional[List[Dict]]]:
    """The job's one exchange as ONE single-process RCCL all-gather over `devices` (one rank per entry; parts[i] = the restarts
    rank i trained): (report, restarts).  report["ran"] is False with a "reason" when RCCL does not apply (one rank; ranks that
    share a GPU) and restarts is then None; with N distinct GPUs a failure raises (include/fastrank.h: fr_rccl_allgather)."""
    n = len(devices)
    cap = max([1] + [len(p) for p in parts])
    dim = max([0] + [len(r["weights"]) for p in parts for r in p])
    blocks = np.stack([pack_restart_records(p, cap, dim) for p in parts]) if n else np.zeros((0, cap, 3 + dim))
    out = np.empty_like(blocks)
    devs = np.ascontiguousarray(devices, dtype=np.int32)
    rep = _json_reply(_load().fr_rccl_allgather(devs.ctypes.data, n, blocks.ctypes.data, cap * (3 + dim), out.ctypes.data))
    if not rep.get("ran"):
        return rep, None
    if not np.array_equal(out.view(np.uint64), blocks.view(np.uint64)):
        raise RuntimeError("rccl_allgather_restarts: rank 0's gathered records differ from the blocks the ranks contributed")
    return rep, unpack_restart_records(out, dim)


def walk_tiles(run_pos, run_q0, run_q1, qstart, qlen, np_positions: int) -> Dict:
    """The walk tiles the device form of a dataset gets for this layout of runs and queries (no device needed)."""
    arrs = [np.ascontiguousarray(a, dtype=np.uint32) for a in (run_pos, run_q0, run_q1, qstart, qlen)]
    return _json_reply(_load().fr_debug_walk_tiles(arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[2].ctypes.data, len(arrs[0]),
                                                   arrs[3].ctypes.data, arrs[4].ctypes.data, len(arrs[3]), int(np_positions)))


# ColStats of csrc/kernels_order.inc, as the device leaves them
COLSTATS_DTYPE = np.dtype([("sum", "<f8"), ("sumsq", "<f8"), ("mn", "<f4"), ("mx", "<f4"), ("at_min", "<u8"), ("at_max", "<u8")])


def device_form(dataset: CDataset, slot: int = 0) -> Dict:
    """The device form of a dataset read back as numpy arrays and scalars (fr_debug_device_form:
    read only, builds the form if needed).  Optional tables the dataset does not hold are None.  `slot` > 0: the copy
    train_model keeps for that entry of its device list.  For a query-sampled view qstart / qlen / the run tables /
    vtiles / wlist are the view's own and everything per position is the parent's, in the parent's position space."""
    L = _load()
    f = {k: int(v) for k, v in _json_reply(L.fr_debug_device_form(dataset.pointer, int(slot), None, None, 0)).items()}
    f["nonfinite"] = bool(f["nonfinite"])
    f["shares_parent_matrix"] = bool(f["shares_parent_matrix"])
    npos, dq, d, nq, nruns = f["np"], f["dq"], f["d"], f["nq"], f["nruns"]

    def table(name, dtype, count, shape=None):
        arr = np.zeros(count, dtype=dtype)
        rep = _json_reply(L.fr_debug_device_form(dataset.pointer, int(slot), name.encode("utf-8"), arr.ctypes.data, arr.nbytes))
        if not rep["present"]:
            return None
        return arr if shape is None else arr.reshape(shape)

    if f["colstats_bytes"] != COLSTATS_DTYPE.itemsize:
        raise RuntimeError("device_form: the library's ColStats record is not the one this module describes")
    f["xb"] = table("xb", np.float32, npos // 64 * dq * 256)
    f["xcol"] = table("xcol", np.float32, d * npos, (d, npos))
    f["xslot"] = table("xslot", np.uint8, d * npos, (d, npos))
    for name, dtype in (("perm", np.uint32), ("perm_host", np.uint32), ("gain", np.float32), ("gexp", np.float64), ("gcls", np.uint32),
                        ("gkey", np.uint16), ("segtab", np.uint16), ("wofs", np.uint8)):
        f[name] = table(name, dtype, npos)
    f["wt_start"] = table("wt_start", np.uint32, f["nwt"] + 1)
    f["qstart"] = table("qstart", np.uint32, nq)
    f["qlen"] = table("qlen", np.uint32, nq)
    f["qtight"] = table("qtight", np.uint32, nq + 1)
    for name in ("run_q0", "run_q1", "run_pos", "run_docs", "run_lo", "run_order", "run_wt0"):
        f[name] = table(name, np.uint32, nruns)
    f["vtiles"] = table("vtiles", np.uint32, f["nvtiles"])
    f["wlist"] = table("wlist", np.uint32, f["nwlist"])
    f["dcgtab"] = table("dcgtab", np.float64, f["ncls"] * f["dcg_ranks"], (f["ncls"], f["dcg_ranks"]))
    f["colmax"] = table("colmax", np.float64, d)
    f["colstd"] = table("colstd", np.float64, d)
    f["colmode"] = table("colmode", np.uint8, d)
    f["colstats"] = table("colstats", COLSTATS_DTYPE, d)
    return f


def host_layout(dataset: CDataset, parent_queries=None, row_hash=None, view: Optional[CDataset] = None) -> Dict:
    """The host-side layout of a dataset (csrc/dataset_layout.hpp) built from its host CSR without a device
    (fr_debug_dataset_layout): the scalars and tables of device_form that are host arithmetic, by the same names, plus termtab,
    qnpos, qnneg, qlist, fv_qlist and the size classes (rows of class, offset, count).  parent_queries: the result's "view"
    holds the tables of the view made of these queries of the dataset (`view`: the dataset whose own regrouping is the
    view's; default: the dataset's documents in its order).  row_hash[np]: the row hashes by position (default: a host hash)."""
    L = _load()
    pq = None if parent_queries is None else np.ascontiguousarray(parent_queries, dtype=np.uint32)
    rh = None if row_hash is None else np.ascontiguousarray(row_hash, dtype=np.uint64)

    def call(name, arr):
        return _json_reply(L.fr_debug_dataset_layout(
            dataset.pointer, None if pq is None else pq.ctypes.data, 0 if pq is None else len(pq), None if view is None else view.pointer,
            None if rh is None else rh.ctypes.data, 0 if rh is None else len(rh), None if name is None else name.encode("utf-8"),
            None if arr is None else arr.ctypes.data, 0 if arr is None else arr.nbytes))

    s = {k: int(v) for k, v in call(None, None).items()}

    def tables(pre, extra):
        out = {k[len(pre):]: v for k, v in s.items() if k.startswith(pre) and (pre or not k.startswith("view_"))}
        nq, nruns, npos = out["nq"], out["nruns"], out["np"]
        spec = [(n, np.uint32, nq, None) for n in ("qstart", "qlen", "qlist", "fv_qlist")] + [("qtight", np.uint32, nq + 1, None)]
        spec += [(n, np.uint32, nruns, None) for n in ("run_q0", "run_q1", "run_pos", "run_docs", "run_lo", "run_order", "run_wt0")]
        spec += [("perm_host", np.uint32, npos, None), ("size_classes", np.uint32, 3 * out["n_size_classes"], (-1, 3)),
                 ("fv_classes", np.uint32, 3 * out["n_fv_classes"], (-1, 3))]
        for name, dtype, count, shape in spec + extra:
            arr = np.zeros(count, dtype=dtype)
            call(pre + name, arr)
            out[name] = arr if shape is None else arr.reshape(shape)
        return out

    npos, nq, ncls = s["np"], s["nq"], s["ncls"]
    f = tables("", [(n, t, npos, None) for n, t in (("perm", np.uint32), ("gain", np.float32), ("gexp", np.float64), ("gcls", np.uint32),
                                                    ("gkey", np.uint16), ("segtab", np.uint16), ("wofs", np.uint8))] +
               [("wt_start", np.uint32, s["nwt"] + 1, None), ("qnpos", np.uint32, nq, None), ("qnneg", np.uint32, nq, None),
                ("dcgtab", np.float64, ncls * s["dcg_ranks"], (ncls, s["dcg_ranks"])),
                # (empty when the dataset has too many gain classes for it)
                ("termtab", np.float64, s["termtab_len"], (ncls + 1, s["tablen"]) if s["termtab_len"] else None)])
    f["labels_small_int"] = bool(f["labels_small_int"])
    if pq is not None:
        f["view"] = tables("view_", [("vtiles", np.uint32, s["view_nvtiles"], None), ("wlist", np.uint32, s["view_nwlist"], None)])
    return f


def rccl_selftest(device: int = 0) -> Dict:
    """A one-rank RCCL communicator on `device` through the library's exchange code (dlopen, ncclCommInitAll, grouped
    ncclAllGather, compare, destroy): the report of fr_rccl_allgather."""
    return _json_reply(_load().fr_debug_rccl_selftest(int(device)))


def release_replicas(dataset: CDataset) -> int:
    """Frees the copies of the dataset train_model made on other devices / in other contexts; returns how many."""
    return int(_load().fr_dataset_release_replicas(dataset.pointer))


def shard_bounds(num_restarts: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous block partition of restart ids over ranks (first ranks take the remainder)."""
    base, rem = divmod(num_restarts, world)
    begin = rank * base + min(rank, rem)
    return begin, begin + base + (1 if rank < rem else 0)


def gather_restarts(mine: List[Dict], num_restarts: int, group=None) -> List[Dict]:
    """The job's single exchange: one all_gather of fixed-size (valid, restart_id, score, weights)
    records over RCCL/xGMI (backend "nccl") or gloo (CPU test rigs).  Returns every rank's
    restarts in restart order, identically on every rank.  Ranks may hold different numbers of
    restarts (block partition with a remainder, or work stealing): the record count is the maximum
    over ranks, agreed in the same small all-reduce that agrees the weight dimension."""
    import torch
    import torch.distributed as dist

    if not dist.is_available() or not dist.is_initialized():
        return sorted(mine, key=lambda r: r["restart_id"])
    world = dist.get_world_size(group)
    backend = dist.get_backend(group)
    dev = torch.device("cuda", torch.cuda.current_device()) if backend == "nccl" else torch.device("cpu")
    shape_t = torch.tensor([max((len(r["weights"]) for r in mine), default=0), len(mine)], dtype=torch.int64, device=dev)
    dist.all_reduce(shape_t, op=dist.ReduceOp.MAX, group=group)
    dim, per_rank = int(shape_t[0].item()), max(1, int(shape_t[1].item()))
    buf = torch.zeros((per_rank, 3 + dim), dtype=torch.float64)
    for k, r in enumerate(mine):
        buf[k, 0] = 1.0
        buf[k, 1] = float(r["restart_id"])
        buf[k, 2] = r["score"]
        buf[k, 3:3 + len(r["weights"])] = torch.tensor(r["weights"], dtype=torch.float64)
    buf = buf.to(dev)
    gathered = [torch.empty_like(buf) for _ in range(world)]
    dist.all_gather(gathered, buf, group=group)
    restarts = []
    for t in gathered:
        for row in t.cpu().tolist():
            if row[0] == 1.0:
                restarts.append({"restart_id": int(row[1]), "score": row[2], "weights": row[3:]})
    restarts.sort(key=lambda r: r["restart_id"])
    if len(restarts) != num_restarts or any(r["restart_id"] != i for i, r in enumerate(restarts)):
        raise RuntimeError("gather_restarts: expected restarts 0..{} exactly once, got {}".format(
            num_restarts - 1, [r["restart_id"] for r in restarts]))
    return restarts


_steal_jobs = 0


def steal_blocks(num_restarts: int, block: int, group=None, store=None):
    """Work stealing over restart blocks (restarts converge after different
    numbers of ticks, so a static partition leaves GPUs idle at the end): yields [begin, end)
    blocks of `block` consecutive restart ids pulled from ONE shared counter -- an atomic add on
    the process group's rendezvous store (TCP), no data-path collective.  Which rank trains which
    block does not matter: a restart's trajectory depends only on its child seed
    (src/coordinate_ascent.rs:211-225)."""
    import torch.distributed as dist

    global _steal_jobs
    key = "fastrank_amd/steal/{}".format(_steal_jobs)  # every rank calls in the same order: same key
    _steal_jobs += 1
    if not dist.is_available() or not dist.is_initialized():
        for b in range(0, num_restarts, block):
            yield b, min(num_restarts, b + block)
        return
    if store is None:
        store = dist.distributed_c10d._get_default_store()
    while True:
        k = int(store.add(key, 1)) - 1
        if k * block >= num_restarts:
            return
        yield k * block, min(num_restarts, (k + 1) * block)


def train_model_work_stealing(dataset: CDataset, train_req, block: int = 8, group=None, store=None, stats: Optional[Dict] = None) -> CModel:
    """Like train_model_distributed, but the ranks pull restart blocks from a shared counter instead of
    taking one static block each.  Same model on every rank, identical to the unsharded run."""
    R = int(train_req.params.num_restarts)
    mine, blocks = [], []
    for begin, end in steal_blocks(R, block, group, store):
        shard = train_model_shard(dataset, train_req, begin, end)
        mine.extend(shard["restarts"])
        blocks.append((begin, end))
    if stats is not None:
        stats["blocks"] = blocks
    restarts = gather_restarts(mine, R, group)
    model = select_model(restarts, bool(train_req.params.output_ensemble))
    model.params = train_req
    return model


def train_model_distributed(dataset: CDataset, train_req, group=None) -> CModel:
    """One process per GPU: every rank holds a replica of the dataset, trains its block of random
    restarts, then ONE all-gather (gather_restarts) and the same deterministic selection on every
    rank.  No data-path collective."""
    import torch.distributed as dist

    if not dist.is_available() or not dist.is_initialized():
        return dataset.train_model(train_req)
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    R = int(train_req.params.num_restarts)
    begin, end = shard_bounds(R, rank, world)
    shard = train_model_shard(dataset, train_req, begin, end)
    restarts = gather_restarts(shard["restarts"], R, group)
    model = select_model(restarts, bool(train_req.params.output_ensemble))
    model.params = train_req
    return model
