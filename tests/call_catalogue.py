"""A catalogue of library calls for the call-sequence tests (tests/test_gpu_call_sequences.py, DESIGN.md "State between
calls"): an *op* is a name plus a function of a set of dataset handles that returns everything the call hands back as a
result.  The property the tests hold every op to is that its canonical bytes are a function of its arguments alone: the same
op on handles that did anything else before gives the bytes it gives on freshly built handles.

The module imports without a device (the requests take their defaults from the library's host side; nothing here touches a
GPU until an op is run).  All ops draw on one dataset and a sibling, built deterministically below:

  * d = 7 columns (odd, so the tiles' float4 groups pad): six of small integers with heavy ties, both signs of zero in
    column 0, and one continuous column; labels 0 .. 4 with some signal;
  * 40 queries whose lengths include 1, 2, 63, 64, 65, 129, 300, one of 1100 documents (past a 768-document run and the
    1024 sort class) and one of 8193 (the slab paths), rows interleaved;
  * the query view leaves the 8193-document query (and every fifth small one) out: the coordinate-ascent ops run there,
    because a tick evaluates every candidate of every restart, and so do the LambdaMART requests, because a pairwise
    gradient pass over the long query costs a hundred times a pass over the view (the parent and the feature view train
    three one-tree requests all the same);
  * the feature view holds five of the seven features;
  * the sibling is a second draw of about 600 documents: validation set and background.

An op's result is a dict of parts, each serialised by `canon`.  Parts whose name starts with "hook:" are read from
process-wide hooks (native.last_train_stats): a caller that runs ops on several host threads passes Ctx(threaded=True), and
those parts are then neither read nor compared; such a caller's FR_METRIC_KERNEL ops leave the environment alone too (putenv
beside another thread's getenv is not safe), which changes the kernel that answers, never the bytes.
"""
import json
import os
import struct

import numpy as np

import fastrank_amd as fr
from fastrank_amd import native
from tests import tree_shapes as ts

# ---------------------------------------------------------------------------------------------- the data
D = 7
SPECIAL_LENS = [1, 2, 63, 64, 65, 129, 300, 1100, 8193]
LONG_QUERY = 9  # the query id of the 8193 documents


def _lens():
    rng = np.random.default_rng(7001)
    return SPECIAL_LENS + [int(v) for v in rng.integers(3, 48, size=31)]


def _draw(seed, lens):
    rng = np.random.default_rng(seed)
    n = int(sum(lens))
    qid = np.repeat(np.arange(1, len(lens) + 1, dtype=np.int64), lens)[rng.permutation(n)]
    X = np.empty((n, D), dtype=np.float32)
    X[:, :6] = rng.integers(-3, 4, size=(n, 6)).astype(np.float32)
    zeros = np.flatnonzero(X[:, 0] == 0)
    X[zeros[::2], 0] = -0.0
    X[:, 6] = rng.normal(0.0, 1.0, n).astype(np.float32)
    signal = 0.5 * X[:, 1] - 0.25 * X[:, 3] + X[:, 6] + rng.normal(0.0, 1.0, n)
    y = np.clip(np.floor(signal * 0.8 + 1.5), 0, 4).astype(np.float64)
    return np.ascontiguousarray(X), y, qid


_ARRAYS = {}


def arrays(which="parent"):
    """(X, y, qid) of the parent or the sibling: the same arrays (read-only) on every call."""
    if which not in _ARRAYS:
        if which == "parent":
            out = _draw(7002, _lens())
        else:
            out = _draw(7003, [1, 2, 17, 40, 64, 65, 90, 33, 120, 70, 60, 38])
        for a in out:
            a.setflags(write=False)
        _ARRAYS[which] = out
    return _ARRAYS[which]


def view_queries():
    """The query view's queries, as the dataset spells them: not the 8193 documents, and not every fifth of the small ones."""
    nq = len(_lens())
    small = list(range(len(SPECIAL_LENS) + 1, nq + 1))
    return [str(q) for q in range(1, nq + 1) if q != LONG_QUERY and q not in small[::5]]


VIEW_FEATURES = [0, 1, 2, 4, 6]


class Handles:
    """The parent dataset, a query-sampled and a feature-sampled view of it, and the sibling; plus what ops keep on them
    between calls (the stepped trainer, models an earlier op trained)."""

    def __init__(self):
        self.parent = fr.CDataset.from_numpy(*[np.array(a) for a in arrays("parent")])
        self.sibling = fr.CDataset.from_numpy(*[np.array(a) for a in arrays("sibling")])
        self.qview = self.fview = None
        self.make_views()
        self.run = None        # the stepped trainer, open between its parts
        self.stage = None      # the name of its part that ran last (None: no run open)
        self.models = {}       # op name -> CModel it trained last
        self.history = []

    def make_views(self):
        """Drops the views and makes them again: a handle-lifetime event.  A stepped trainer open on the old view ends."""
        self.close_run()
        names = self.parent.feature_index_to_name()
        self.qview = self.fview = None
        self.qview = self.parent.subsample_queries(view_queries())
        self.fview = self.parent.subsample_feature_names([names[f] for f in VIEW_FEATURES])

    def close_run(self):
        if getattr(self, "run", None) is not None:
            self.run.close()
        self.run, self.stage = None, None

    def close(self):
        self.close_run()
        self.models = {}
        self.qview = self.fview = self.parent = self.sibling = None


class Ctx:
    def __init__(self, threaded=False):
        self.threaded = threaded


# ---------------------------------------------------------------------------------------------- canonical bytes

def _canon(obj, out):
    if obj is None:
        out.append(b"N")
    elif isinstance(obj, (bool, np.bool_)):
        out.append(b"T" if obj else b"F")
    elif isinstance(obj, (int, np.integer)):
        out.append(b"i" + str(int(obj)).encode() + b";")
    elif isinstance(obj, (float, np.floating)):
        out.append(b"f" + struct.pack("<d", float(obj)))
    elif isinstance(obj, str):
        raw = obj.encode("utf-8")
        out.append(b"s" + str(len(raw)).encode() + b":" + raw)
    elif isinstance(obj, (bytes, bytearray)):
        out.append(b"b" + str(len(obj)).encode() + b":" + bytes(obj))
    elif isinstance(obj, np.ndarray):
        a = np.ascontiguousarray(obj)
        out.append(b"a" + a.dtype.str.encode() + b"|" + repr(a.shape).encode() + b"|" + a.tobytes())
    elif isinstance(obj, dict):
        out.append(b"{")
        for k in sorted(obj, key=str):
            _canon(str(k), out)
            _canon(obj[k], out)
        out.append(b"}")
    elif isinstance(obj, (list, tuple)):
        out.append(b"[")
        for v in obj:
            _canon(v, out)
        out.append(b"]")
    else:
        raise TypeError("canon: no canonical form for {!r}".format(type(obj)))


def canon(obj) -> bytes:
    """Floats as the eight bytes of their bits, arrays as dtype, shape and raw bytes, dicts by sorted key."""
    out = []
    _canon(obj, out)
    return b"".join(out)


def model_json(model) -> str:
    return json.dumps(model.to_dict(), sort_keys=True)


# ---------------------------------------------------------------------------------------------- models

_THRESHOLDS = {f: [-2.5, -2.0, -1.0, -0.0, 0.0, 0.5, 1.0, 2.0] for f in range(6)}
_THRESHOLDS[6] = [float(v) for v in np.linspace(-2.0, 2.0, 41)]
_THRESHOLDS[9] = [-1.0, 0.0, 1.0]  # a feature the dataset does not hold reads 0.0


def _picker(seed, feats=range(D)):
    return ts.Picker(seed, feats, _THRESHOLDS)


def _weights_for(count, seed):
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], count) * 10.0 ** rng.uniform(-3.0, 3.0, count)).tolist()


def _ensemble(trees, weights):
    return {"Ensemble": {"weights": [float(w) for w in weights], "models": [{"DecisionTree": t} for t in trees]}}


def _chain33():
    """A chain over 33 distinct features: one more than the explain kernel's paths hold."""
    node = {"LeafNode": 1.0}
    for f in reversed(range(33)):
        node = {"FeatureSplit": {"fid": f, "split": 0.0, "lhs": {"LeafNode": -0.5 * f}, "rhs": node}}
    return node


_MODELS = {}


def model_dict(name):
    """The catalogue's fixed models, by name (built once; the same dict on every call)."""
    if not _MODELS:
        m = _MODELS
        m["linear"] = {"Linear": {"weights": [-0.7, -1.0 / 3.0, 0.0, 0.45, 0.125, -0.2, 0.6]}}
        m["linear_b"] = {"Linear": {"weights": [0.3, 0.0, -0.45, 0.1, -1.0 / 7.0, 0.25, -0.5]}}
        m["single_in"] = {"SingleFeature": {"fid": 0, "dir": -1.5}}   # -1.5 * +-0.0: both signs of zero tie
        m["single_out"] = {"SingleFeature": {"fid": 9, "dir": 2.0}}    # fid >= d: the fill path
        m["tree"] = {"DecisionTree": ts.complete(3, _picker(11, [0, 3, 6, 9]))}
        m["ensemble_linear"] = {"Ensemble": {"weights": [0.5, -2.0, 1e-3], "models": [m["linear"], m["single_in"], m["linear_b"]]}}
        trees70 = [ts.complete(4, _picker(100 + t)) for t in range(70)]
        w70 = _weights_for(70, 21)
        m["forest_rank_70"] = _ensemble(trees70, w70)
        ulp = list(w70)
        ulp[17] = float(np.nextafter(ulp[17], np.inf))
        m["forest_rank_70_ulp"] = _ensemble(trees70, ulp)
        m["forest_rank_2"] = _ensemble([ts.complete(4, _picker(300 + t)) for t in range(2)], _weights_for(2, 22))
        # a chain of 12 levels is deeper than the threshold-rank walk takes: the f32 LDS walk
        p = _picker(23)
        m["forest_lds"] = _ensemble([ts.chain(12, "left", p), ts.chain(3, "right", p), ts.chain(1, "left", p)], _weights_for(3, 23))
        # comb(12, 8): a child offset past the LDS walk's 8 bits: the L2 walk
        m["forest_l2"] = _ensemble([ts.comb(12, 8, _picker(24), "right"), ts.chain(2, "left", _picker(25, [0]))], _weights_for(2, 24))
        m["forest_8"] = _ensemble([ts.complete(4, _picker(400 + t)) for t in range(8)], [0.1] * 8)
        m["nan"] = {"Linear": {"weights": [1e308, -1e308, 0.0, 0.0, 0.0, 0.0, 0.0]}}  # +inf - inf; the format holds no NaN weight
        m["chain33"] = {"DecisionTree": _chain33()}
    return _MODELS[name]


def _model(name):
    return fr.CModel.from_dict(model_dict(name))


# two sets of judgments that move the norms of the same three queries, differently: the same number of queries, other norms.
# Every judged pool dominates the query's own documents (more documents, a larger gain), so that NDCG's ideal stays above
# what a ranking reaches.
QRELS = {
    "a": {"3": {"doc%d" % k: 4.0 for k in range(100)}, "7": {"doc%d" % k: 4.0 for k in range(400)}, "12": {"doc%d" % k: 6.0 for k in range(60)}},
    "b": {"3": {"doc%d" % k: 5.0 for k in range(80)}, "7": {"doc%d" % k: 5.0 for k in range(350)}, "12": {"doc%d" % k: 5.0 for k in range(60)}},
}


def _qrel(which):
    return None if which is None else fr.CQRel.from_dict(QRELS[which])


# ---------------------------------------------------------------------------------------------- requests

def ca_request(measure, seed=42):
    req = fr.TrainRequest.coordinate_ascent()
    req.measure = measure
    p = req.params
    p.num_restarts, p.num_max_iterations, p.quiet, p.seed = 2, 3, True, seed
    return req


def rf_request(split_method):
    req = fr.TrainRequest.random_forest()
    req.measure = "ndcg@10"
    p = req.params
    p.quiet, p.num_trees, p.seed, p.max_depth, p.split_method = True, 2, 7, 5, {split_method: []}
    return req


def lm_request(measure="ndcg@10", **kw):
    req = fr.TrainRequest.lambdamart()
    req.measure = measure
    p = req.params
    p.quiet, p.num_trees, p.max_depth, p.min_leaf_support, p.split_candidates, p.grower = True, 2, 4, 5, 16, "histogram"
    for k, v in kw.items():
        setattr(p, k, v)
    return req


_NEWTON = dict(split_gain="newton", lambda_l2=0.5)
HELD_OUT = {"a": ["2", "5", "11", "14", "21", "33"], "b": ["4", "6", "13", "17", "22", "31"]}  # two lists of one length

LM_REQUESTS = {
    "lm_exact": lambda: lm_request(grower="exact"),
    "lm_hist_k64": lambda: lm_request(split_candidates=64),
    "lm_hist_k16": lambda: lm_request(),
    "lm_hist_k16_ndcg": lambda: lm_request(measure="ndcg"),
    "lm_hist_k8": lambda: lm_request(split_candidates=8),
    "lm_newton_goss": lambda: lm_request(goss_top_rate=0.2, goss_other_rate=0.2, seed=3, **_NEWTON),
    "lm_leaves_255": lambda: lm_request(max_leaves=255, max_depth=10, min_leaf_support=1),
    "lm_leaves_4": lambda: lm_request(max_leaves=4, max_depth=10, min_leaf_support=1),
    "lm_monotone_reg": lambda: lm_request(monotone_constraints={"1": 1, "6": -1}, lambda_l1=0.01, max_delta_step=0.5, path_smooth=1.0, **_NEWTON),
    "lm_symmetric": lambda: lm_request(symmetric_trees=True),
    "lm_quant_4": lambda: lm_request(grad_quant_bits=4, seed=3, **_NEWTON),
    "lm_dart": lambda: lm_request(num_trees=3, drop_rate=0.5, skip_drop=0.0, seed=9),
    "lm_xendcg": lambda: lm_request(objective="xendcg", seed=4),
    "lm_map": lambda: lm_request(objective="map"),
    "lm_trunc_norm": lambda: lm_request(truncation_level=5, lambda_norm=True),
    "lm_sampled": lambda: lm_request(num_trees=3, query_sampling_rate=0.5, feature_sampling_rate=0.5, seed=5),
    "lm_held_out_a": lambda: lm_request(validation_queries=list(HELD_OUT["a"])),
    "lm_held_out_b": lambda: lm_request(validation_queries=list(HELD_OUT["b"])),
    "lm_refused_keys": lambda: lm_request(symmetric_trees=True, max_leaves=8),
}


def monotone_names(dataset):
    """{feature name: sign} for features 1 (+1) and 6 (-1), as the dataset spells its features."""
    names = dataset.feature_index_to_name()
    return {names[1]: 1, names[6]: -1}


# ---------------------------------------------------------------------------------------------- ops

class Op:
    def __init__(self, name, family, handles, fn, refusal=False, after=None, plan=None, request=None, size=None, process_wide=False):
        self.name, self.family, self.handles, self.fn = name, family, tuple(handles), fn
        self.refusal = refusal    # the call is refused: its bytes are the error text
        self.after = after        # a part of the stepped trainer: the part that must have run last on the handles
        self.plan = plan          # a forest: the path native.last_tree_plan() names on a fresh handle
        self.request = request    # () -> the TrainRequest the op sends (None: it sends none)
        self.size = size          # "large" / "small": a variant of a call whose buffers scale with an argument
        self.process_wide = process_wide  # the call hands its result over through a process-wide record: one thread at a time

    def call(self, h, ctx):
        """{part: canonical bytes}.  A refusal's part is the error text; any other op lets an error through."""
        if not self.refusal:
            return {k: canon(v) for k, v in self.fn(h, ctx).items()}
        try:
            self.fn(h, ctx)
        except Exception as exc:  # noqa: BLE001 (the library raises plain Exception)
            return {"refused": canon(str(exc))}
        return {"refused": canon("NOT REFUSED")}


OPS = {}


def op(name, family, handles, **kw):
    def reg(fn):
        assert name not in OPS, name
        OPS[name] = Op(name, family, handles, fn, **kw)
        return fn
    return reg


def _ds(h, which):
    return getattr(h, which)


# ---- scoring
def _score_op(name, model, which, plan=None, size=None):
    @op(name, "scoring", [which], plan=plan, size=size)
    def _fn(h, ctx, model=model, which=which):
        return {"scores": native.predict_scores_dense(_model(model), _ds(h, which))}


for _name, _m in (("score_linear", "linear"), ("score_single_in", "single_in"), ("score_single_out", "single_out"),
                  ("score_tree", "tree"), ("score_ensemble_linear", "ensemble_linear")):
    _score_op(_name, _m, "parent")
_score_op("score_forest_rank_70", "forest_rank_70", "parent", plan="rank", size="large")
_score_op("score_forest_rank_70_again", "forest_rank_70", "parent", plan="rank", size="large")  # the cache hit
_score_op("score_forest_rank_70_ulp", "forest_rank_70_ulp", "parent", plan="rank", size="large")
_score_op("score_forest_rank_2", "forest_rank_2", "parent", plan="rank", size="small")
_score_op("score_forest_lds", "forest_lds", "parent", plan="lds")
_score_op("score_forest_l2", "forest_l2", "parent", plan="l2")
_score_op("score_linear@qview", "linear", "qview")
_score_op("score_forest_rank_70@qview", "forest_rank_70", "qview", plan="rank", size="large")
_score_op("score_ensemble_linear@fview", "ensemble_linear", "fview")
_score_op("score_forest_rank_2@fview", "forest_rank_2", "fview", plan="rank", size="small")


# ---- evaluation
def _with_metric_kernel(ctx, kernel, fn):
    if kernel is None or ctx.threaded:
        return fn()
    old = os.environ.get("FR_METRIC_KERNEL")
    os.environ["FR_METRIC_KERNEL"] = kernel
    try:
        return fn()
    finally:
        if old is None:
            del os.environ["FR_METRIC_KERNEL"]
        else:
            os.environ["FR_METRIC_KERNEL"] = old


def _eval_op(name, measure, which, qrel=None, kernel=None, model="linear"):
    @op(name, "evaluation", [which])
    def _fn(h, ctx):
        names, values = _with_metric_kernel(ctx, kernel, lambda: native.evaluate_dense(_model(model), _ds(h, which), measure, _qrel(qrel)))
        return {"queries": names, "values": values}


EVAL_MEASURES = ["ndcg@10", "ndcg@5", "ndcg", "map", "mrr", "err@10", "recall", "precision@65"]
for _measure in EVAL_MEASURES:
    _eval_op("eval_%s" % _measure, _measure, "parent")
    _eval_op("eval_%s+qrel_a" % _measure, _measure, "parent", qrel="a")
for _kernel in ("topk", "sort"):
    _eval_op("eval_dcg@10[%s]" % _kernel, "dcg@10", "parent", kernel=_kernel)
    _eval_op("eval_dcg@10[%s]+qrel_a" % _kernel, "dcg@10", "parent", qrel="a", kernel=_kernel)
_eval_op("eval_ndcg@10+qrel_b", "ndcg@10", "parent", qrel="b")   # after +qrel_a: other norms for the same queries
_eval_op("eval_map+qrel_b", "map", "parent", qrel="b")
_eval_op("eval_ndcg@10_forest", "ndcg@10", "parent", model="forest_rank_70")
_eval_op("eval_ndcg@10@qview", "ndcg@10", "qview")
_eval_op("eval_ndcg@5@qview+qrel_a", "ndcg@5", "qview", qrel="a")
_eval_op("eval_err@10@fview", "err@10", "fview")


def _rank_order_op(name, model, which):
    @op(name, "evaluation", [which])
    def _fn(h, ctx):
        ids, offs = native.rank_order(_model(model), _ds(h, which))
        return {"ids": ids, "offsets": offs}


_rank_order_op("rank_order_linear", "linear", "parent")
_rank_order_op("rank_order_forest@qview", "forest_rank_2", "qview")


def _candidates(slots):
    """(features, base weights, candidates) of a batched line search of about `slots` slots."""
    base = np.array(model_dict("linear")["Linear"]["weights"]), np.array(model_dict("linear_b")["Linear"]["weights"])
    if slots <= 2:
        return [3], [base[0]], [[-0.25, 0.5]]
    grid = np.linspace(-1.0, 1.0, 35).tolist()
    return [1, 6], [base[0], base[1]], [grid, [v * 0.5 for v in grid]]


def _cand_op(name, measure, slots):
    @op(name, "evaluation", ["parent"], size="large" if slots > 2 else "small")
    def _fn(h, ctx):
        feats, base, cands = _candidates(slots)
        means, pq = native.evaluate_candidates(h.parent, measure, feats, np.array(base), cands, per_query=True)
        return {"means": means, "per_query": pq}


for _measure in ("ndcg@10", "err@10"):
    _cand_op("candidates_70_%s" % _measure, _measure, 70)
    _cand_op("candidates_2_%s" % _measure, _measure, 2)


# ---- coordinate ascent (on the query view)
def _ca_op(name, measure):
    @op(name, "coordinate_ascent", ["qview"], request=lambda: ca_request(measure))
    def _fn(h, ctx):
        return {"model": model_json(h.qview.train_model(ca_request(measure)))}


_ca_op("ca_ndcg@10", "ndcg@10")   # fused line search on resident sums
_ca_op("ca_ndcg", "ndcg")         # full ranking
_ca_op("ca_mrr", "mrr")
_ca_op("ca_dcg@5", "dcg@5")       # the generic sort evaluator

STEPPED_PARTS = ("ca_stepped_1_open+step", "ca_stepped_2_step", "ca_stepped_3_finish+state")


def _stepped_state(h):
    return {"restarts": h.run.state()["restarts"], "finished": h.run.finished}


@op(STEPPED_PARTS[0], "coordinate_ascent", ["qview"], request=lambda: ca_request("ndcg@10", seed=43))
def _stepped_open(h, ctx):
    h.close_run()
    h.run = native.CoordinateAscentRun(h.qview, ca_request("ndcg@10", seed=43))
    done = h.run.step(3)
    h.stage = STEPPED_PARTS[0]
    return dict(_stepped_state(h), ticks=done)


@op(STEPPED_PARTS[1], "coordinate_ascent", ["qview"], after=STEPPED_PARTS[0])
def _stepped_step(h, ctx):
    done = h.run.step(4)
    h.stage = STEPPED_PARTS[1]
    return dict(_stepped_state(h), ticks=done)


@op(STEPPED_PARTS[2], "coordinate_ascent", ["qview"], after=STEPPED_PARTS[1])
def _stepped_finish(h, ctx):
    ticks = 0
    while not h.run.finished:
        ticks += h.run.step(1 << 20)
    out = dict(_stepped_state(h), ticks=ticks)
    h.close_run()
    return out


# ---- random forest
def _rf_op(name, method):
    @op(name, "random_forest", ["parent"], request=lambda: rf_request(method))
    def _fn(h, ctx):
        return {"model": model_json(h.parent.train_model(rf_request(method)))}


_rf_op("rf_squared_error", "SquaredError")
_rf_op("rf_information_gain", "InformationGain")


@op("rf_levels_small_root", "random_forest", ["parent"], process_wide=True)
def _rf_levels(h, ctx):
    """(fr_debug_rf_levels records into one process-wide blob that a second call fetches: not for several threads at once)"""
    ids = np.random.default_rng(31).permutation(len(arrays("parent")[1]))[:50]
    return native.rf_levels(h.parent, [0, len(ids)], ids, [[0, 1, 6]], 4, 0, 2, 3)


# ---- LambdaMART
def _lm_stats(ctx):
    if ctx.threaded:
        return {}
    st = native.last_train_stats()["lambdamart"]
    return {"hook:measures": {k: st.get(k) for k in ("train_measure", "valid_measure", "best_iteration")}}


def _lm_train(h, ctx, name, req, which="parent", valid=None, init_model=None):
    if req.params.monotone_constraints:  # (the request names features 1 and 6; the dataset says how it spells them)
        req.params.monotone_constraints = monotone_names(_ds(h, which))
    model = _ds(h, which).train_model(req, valid=valid, init_model=init_model)
    h.models[name] = model
    return dict({"model": model_json(model)}, **_lm_stats(ctx))


_LM_SIZES = {"lm_hist_k64": "large", "lm_hist_k8": "small", "lm_leaves_255": "large", "lm_leaves_4": "small"}


def _lm_op(name, which, trees=None):
    """The request LM_REQUESTS[name] on a handle; the op is called name@handle (the parent's: the bare name).  `trees`: another
    number of trees than the request's."""
    full = name if which == "parent" else "%s@%s" % (name, which)

    def request():
        req = LM_REQUESTS[name]()
        if trees is not None:
            req.params.num_trees = trees
        return req

    @op(full, "lambdamart", [which], request=request, size=_LM_SIZES.get(name))
    def _fn(h, ctx):
        return _lm_train(h, ctx, full, request(), which)


# Every request trains on the query view.  A gradient pass over the 8193 documents of the parent's long query costs a
# hundred times a pass over the view, so the parent and the feature view (which holds that query too) train three requests,
# of one tree each: the slab path, the parent's kept bins, a feature-sampled bin matrix.
for _name in LM_REQUESTS:
    if _name != "lm_refused_keys":
        _lm_op(_name, "qview")
_lm_op("lm_hist_k16", "parent", trees=1)
_lm_op("lm_hist_k16_ndcg", "parent", trees=1)
_lm_op("lm_hist_k16", "fview", trees=1)


@op("lm_valid_sibling@qview", "lambdamart", ["qview", "sibling"], request=LM_REQUESTS["lm_hist_k16"])
def _lm_valid(h, ctx):
    return _lm_train(h, ctx, "lm_valid_sibling@qview", LM_REQUESTS["lm_hist_k16"](), "qview", valid=h.sibling)


@op("lm_init_model@qview", "lambdamart", ["qview"], request=LM_REQUESTS["lm_hist_k16"])
def _lm_init(h, ctx):
    """Continues from the model op lm_hist_k16@qview trained last on these handles (trained here if it has not run yet: its
    bytes do not depend on when)."""
    first = "lm_hist_k16@qview"
    if first not in h.models:
        _lm_train(h, ctx, first, LM_REQUESTS["lm_hist_k16"](), "qview")
    return _lm_train(h, ctx, "lm_init_model@qview", LM_REQUESTS["lm_hist_k16"](), "qview", init_model=h.models[first])


def _gradients_in():
    """lam / wt by instance id of the parent, for the grower's hooks: a fixed draw on a grid of 1/64 (exact in fixed point)."""
    rng = np.random.default_rng(41)
    n = len(arrays("parent")[1])
    return rng.integers(-128, 129, n) / 64.0, rng.integers(0, 65, n) / 64.0


def _lamgrad_op(name, measure, which="parent", **kw):
    @op(name, "lambdamart_hooks", [which])
    def _fn(h, ctx):
        lam, wt = native.lambda_gradients(_model("linear"), _ds(h, which), measure, **kw)
        return {"lam": lam, "wt": wt}


_lamgrad_op("lambda_gradients_ndcg@10", "ndcg@10")   # every query: the long one through the slab
_lamgrad_op("lambda_gradients_ndcg@qview", "ndcg", "qview")
# two query samples of one size that share no query (neither holds the long one)
_lamgrad_op("lambda_gradients_sampled", "ndcg@10", queries=list(range(2, 40, 3)))
_lamgrad_op("lambda_gradients_sampled_b", "ndcg@10", queries=list(range(1, 39, 3)))
_lamgrad_op("lambda_gradients_trunc_norm", "ndcg@10", queries=list(range(1, 39, 3)), truncation_level=3, lambda_norm=True)


@op("hist_tree_k64_leafwise", "lambdamart_hooks", ["parent"], size="large")
def _hist_tree_big(h, ctx):
    lam, wt = _gradients_in()
    return {"model": model_json(native.hist_tree(h.parent, lam, wt, 64, 8, 2, max_leaves=63))}


@op("hist_tree", "lambdamart_hooks", ["parent"], size="small")
def _hist_tree(h, ctx):
    lam, wt = _gradients_in()
    return {"model": model_json(native.hist_tree(h.parent, lam, wt, 16, 4, 5))}


@op("hist_tree_newton@fview", "lambdamart_hooks", ["fview"])
def _hist_tree_f(h, ctx):
    lam, wt = _gradients_in()
    return {"model": model_json(native.hist_tree(h.fview, lam, wt, 8, 3, 5, split_gain="newton", lambda_l2=0.5, max_leaves=6))}


@op("goss_select", "lambdamart_hooks", ["parent"])
def _goss(h, ctx):
    rows, top, tau = native.goss_select(h.parent, _gradients_in()[0], 0.2, 0.2, 3, 1)
    return {"rows": rows, "top": top, "tau": tau}


@op("hist_quantise", "lambdamart_hooks", ["parent"])
def _quantise(h, ctx):
    lam, wt = _gradients_in()
    return native.hist_quantise(h.parent, lam, wt, 4, 3, 0)


def _root_hist_op(name, k, quant):
    @op(name, "lambdamart_hooks", ["parent"])
    def _fn(h, ctx):
        lam, wt = _gradients_in()
        cnt, qs, ws = native.hist_root_histogram(h.parent, lam, wt, k, quant=quant)
        return {"count": cnt, "q": qs, "w": ws}


_root_hist_op("hist_root_histogram_k16", 16, None)
_root_hist_op("hist_root_histogram_k64_quant", 64, (4, 3, 0))


# ---- explanation and statistics
def _explain_op(name, which, background):
    @op(name, "explain", [which] + ([background] if background else []))
    def _fn(h, ctx):
        ex = _model("forest_8").explain(_ds(h, which), None if background is None else _ds(h, background))
        return {"values": ex.values, "feature_ids": ex.feature_ids, "expected_value": ex.expected_value}


_explain_op("explain", "parent", None)
_explain_op("explain_background_sibling", "parent", "sibling")
_explain_op("explain@qview", "qview", None)


@op("feature_importance", "explain", ["parent"])
def _importance(h, ctx):
    ids, mean_abs, rep = native.feature_importance(_model("forest_8"), h.parent)
    return {"ids": ids, "mean_abs": mean_abs, "split_counts": rep.get("split_counts")}


def _permimp_op(name, model, which, size, **kw):
    @op(name, "statistics", [which], size=size)
    def _fn(h, ctx):
        _, values, rows = native.permutation_importance_dense(_model(model), _ds(h, which), "ndcg@10", **kw)
        return {"values": values, "per_query": rows}


_permimp_op("permutation_importance_linear", "linear", "parent", "large", repeats=3, seed=5)
_permimp_op("permutation_importance_forest", "forest_8", "parent", "small", repeats=1, seed=6, features=[1, 6])
_permimp_op("permutation_importance_forest@qview", "forest_8", "qview", "small", repeats=2, seed=6, features=[0, 6], scope="query")


@op("bootstrap_eval", "statistics", ["parent"])
def _bootstrap(h, ctx):
    return h.parent.bootstrap_eval(_model("linear"), "ndcg@10", trials=200, seed=1)


@op("compare_models", "statistics", ["parent"])
def _compare(h, ctx):
    rep = fr.compare_models(h.parent, {"a": _model("linear"), "b": _model("forest_rank_2"), "c": _model("single_in")}, "map", trials=300, seed=3)
    return {k: v for k, v in rep.items() if k != "stats"}


def _stats_op(name, which):
    @op(name, "statistics", [which])
    def _fn(h, ctx):
        return {str(f): rec for f, rec in _ds(h, which).feature_stats().items()}


_stats_op("feature_stats", "parent")
_stats_op("feature_stats@qview", "qview")
_stats_op("feature_stats@fview", "fview")


def _normalised(ds):
    core = native.loaded_arrays(ds)
    return {"x": core["x"], "gain": core["gain"], "qix": core["qix"], "normalization": ds.normalization()}


@op("normalize_zscore_fit_apply", "statistics", ["parent"])
def _norm_dataset_scope(h, ctx):
    norm = fr.Normalizer.fit(h.parent, "zscore")
    return dict(_normalised(norm.apply(h.parent)), wire=norm.to_dict())


@op("normalize_maxmin_fit@qview_apply", "statistics", ["qview", "parent"])
def _norm_view_fit(h, ctx):
    norm = fr.Normalizer.fit(h.qview, "maxmin")
    return dict(_normalised(norm.apply(h.parent)), wire=norm.to_dict())


@op("normalize_per_query_zscore_apply", "statistics", ["parent"])
def _norm_query_scope(h, ctx):
    return _normalised(fr.Normalizer.per_query("zscore").apply(h.parent))


# ---- refusals
@op("refused_nan_scores", "refusals", ["parent"], refusal=True)
def _refused_nan(h, ctx):
    native.evaluate_dense(_model("nan"), h.parent, "dcg@10")


@op("refused_nan_scores_ndcg@qview", "refusals", ["qview"], refusal=True)
def _refused_nan_view(h, ctx):
    native.evaluate_dense(_model("nan"), h.qview, "ndcg@10")


@op("refused_explain_33_features", "refusals", ["parent"], refusal=True)
def _refused_explain(h, ctx):
    _model("chain33").explain(h.parent)


@op("refused_lm_exclusive_keys", "refusals", ["parent"], refusal=True, request=LM_REQUESTS["lm_refused_keys"])
def _refused_lm(h, ctx):
    h.parent.train_model(LM_REQUESTS["lm_refused_keys"]())


NAMES = list(OPS)

# what section 1 of the catalogue's contract lists: family -> op names that must be present
REQUIRED = {
    "scoring": ["score_linear", "score_single_in", "score_single_out", "score_tree", "score_ensemble_linear", "score_forest_rank_70",
                "score_forest_rank_70_again", "score_forest_rank_70_ulp", "score_forest_rank_2", "score_forest_lds", "score_forest_l2"],
    "evaluation": ["eval_%s%s" % (m, s) for m in EVAL_MEASURES for s in ("", "+qrel_a")] +
                  ["eval_dcg@10[%s]%s" % (k, s) for k in ("topk", "sort") for s in ("", "+qrel_a")] +
                  ["rank_order_linear", "candidates_70_ndcg@10", "candidates_2_ndcg@10"],
    "coordinate_ascent": ["ca_ndcg@10", "ca_ndcg", "ca_mrr", "ca_dcg@5"] + list(STEPPED_PARTS),
    "random_forest": ["rf_squared_error", "rf_information_gain", "rf_levels_small_root"],
    "lambdamart": ["%s@qview" % n for n in LM_REQUESTS if n != "lm_refused_keys"] +
                  ["lm_valid_sibling@qview", "lm_init_model@qview", "lm_hist_k16", "lm_hist_k16_ndcg", "lm_hist_k16@fview"],
    "lambdamart_hooks": ["lambda_gradients_ndcg@10", "lambda_gradients_ndcg@qview", "hist_tree", "goss_select", "hist_quantise",
                         "hist_root_histogram_k16"],
    "explain": ["explain", "explain_background_sibling", "feature_importance"],
    "statistics": ["permutation_importance_linear", "permutation_importance_forest", "bootstrap_eval", "compare_models", "feature_stats",
                   "normalize_zscore_fit_apply", "normalize_per_query_zscore_apply"],
    "refusals": ["refused_nan_scores", "refused_explain_33_features", "refused_lm_exclusive_keys"],
}
LARGE_SMALL = [("score_forest_rank_70", "score_forest_rank_2"), ("candidates_70_ndcg@10", "candidates_2_ndcg@10"),
               ("lm_hist_k64@qview", "lm_hist_k8@qview"), ("lm_leaves_255@qview", "lm_leaves_4@qview"), ("hist_tree_k64_leafwise", "hist_tree"),
               ("permutation_importance_linear", "permutation_importance_forest")]


# ---------------------------------------------------------------------------------------------- running ops

def run_op(h, name, ctx=None):
    """Runs op `name` on the handles, after the parts of the stepped trainer it needs if they are not what ran last.
    Returns [(op name, {part: bytes}), ...] in the order run, and notes every op in h.history."""
    ctx = ctx or Ctx()
    o = OPS[name]
    out = []
    if ctx.threaded and o.process_wide:
        return out
    if o.after is not None and h.stage != o.after:
        out += run_op(h, o.after, ctx)
    h.history.append(name)
    out.append((name, o.call(h, ctx)))
    return out


def differing_parts(got, fresh, ctx=None):
    """The parts of an op's result whose bytes are not the fresh handle's (hook parts are not compared on threads)."""
    threaded = ctx is not None and ctx.threaded
    keys = [k for k in fresh if not (threaded and k.startswith("hook:"))]
    extra = [k for k in got if k not in fresh]
    return [k for k in keys if got.get(k) != fresh[k]] + extra


def pairs():
    """Every ordered pair of ops, rows by the first one."""
    return [(a, b) for a in NAMES for b in NAMES]


def walk(seed, length=60, handles=None):
    """A seeded walk: a list of steps, each an op name or one of the lifetime events "@remake_views" / "@release_replicas".
    The stepped trainer's three parts appear in order, other ops between them.  `handles`: draw only ops that touch
    nothing but these (default: any op)."""
    rng = np.random.default_rng(seed)
    pool = [n for n in NAMES if n not in STEPPED_PARTS and (handles is None or set(OPS[n].handles) <= set(handles))]
    at = {}
    if handles is None or set(OPS[STEPPED_PARTS[0]].handles) <= set(handles):
        third = max(2, length // 3)
        where = np.cumsum(rng.integers(1, third, size=3))  # (the last part at 3 * (third - 1) at the latest: inside the walk)
        at = {int(w): part for w, part in zip(where, STEPPED_PARTS)}
    steps = []
    while len(steps) < length:
        u = rng.random()
        if len(steps) in at:
            steps.append(at[len(steps)])
        elif u < 0.04:
            steps.append("@remake_views")  # (a trainer open on the old view ends with it: run_op then opens another)
        elif u < 0.08:
            steps.append("@release_replicas")
        else:
            steps.append(pool[int(rng.integers(0, len(pool)))])
    return steps


def run_step(h, step, ctx=None):
    """One step of a walk: an op (run_op's list) or a lifetime event (an empty list)."""
    if step == "@remake_views":
        h.history.append(step)
        h.make_views()
        return []
    if step == "@release_replicas":
        h.history.append(step)
        for ds in (h.parent, h.qview, h.fview, h.sibling):
            native.release_replicas(ds)
        return []
    return run_op(h, step, ctx)
