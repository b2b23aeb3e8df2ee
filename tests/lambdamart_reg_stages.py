"""What the device tests of LambdaMART's leaf regularisation share (tests/test_gpu_lambdamart_reg.py and its soak): the small
designed dataset, and a training run held stage by stage to the restatements -- tree t is lambdamart_reg_model's fit to the
DEVICE's gradients of the ensemble the tree is fitted to, over the tree's samples (and, under GOSS, over
lambdamart_goss_model's list with its amplified gradients); the running measures are the oracle's."""
import numpy as np

import fastrank_amd as fr
from fastrank_amd import native
from oracle import pyoracle as o
from tests import lambdamart_composed_model as cmod
from tests import lambdamart_dart_model as dm
from tests import lambdamart_goss_model as gm
from tests import lambdamart_reg_model as rm
from tests import lambdamart_sample_model as sm
from tests import lambdamart_xendcg_model as xm

LENGTHS = [1, 2, 5, 9, 14, 20, 27, 33, 41, 48, 55, 60]  # 12 queries, 315 documents
REG_STATS = {"lambda_l1", "max_delta_step", "path_smooth"}
EMPTY = {"Ensemble": {"weights": [], "models": []}}


def small_dataset(seed, features=5):
    """(X f32 [315, features], y, qid): continuous features (up to 255 edges each), labels 0..4 that lean on feature 0."""
    rng = np.random.default_rng(seed)
    n = sum(LENGTHS)
    X = rng.normal(size=(n, features)).astype(np.float32)
    y = np.clip(np.rint(1.5 + X[:, 0] + 0.7 * rng.normal(size=n)), 0, 4).astype(np.float64)
    qid = np.repeat(np.arange(1, len(LENGTHS) + 1), LENGTHS).astype(np.int64)
    return X, y, qid


def reg_of(p):
    return (float(p.get("lambda_l1", 0.0)), float(p.get("max_delta_step", 0.0)), float(p.get("path_smooth", 0.0)))


def ensemble(trees, weights):
    if not trees:
        return fr.CModel.from_dict(EMPTY)
    return fr.CModel.from_dict({"Ensemble": {"weights": [float(w) for w in weights], "models": [{"DecisionTree": x} for x in trees]}})


def trees_of(model):
    return [m["DecisionTree"] for m in model.to_dict()["Ensemble"]["models"]]


def stagewise(g, c, X, y, measure, params, names=None):
    """Trains under `params` (the Newton gain is added) and holds every stage to the restatements.  Returns (model, stats,
    traces: per tree the restatement's split records)."""
    params = dict(params, split_gain="newton")
    req = cmod._request(measure, "histogram", **params)
    p = req.params
    reg = reg_of(params)
    cm = cmod.Composed(X, y, c, measure, dict(fr.LambdaMARTParams().to_dict(), **dict(params, grower="histogram")), names=names)
    model = g.train_model(req)
    st = native.last_train_stats()["lambdamart"]
    if any(reg):
        assert REG_STATS <= set(st) and (st["lambda_l1"], st["max_delta_step"], st["path_smooth"]) == reg
    else:
        assert not (REG_STATS & set(st))
    d = model.to_dict()
    trees = trees_of(model)
    T = st["trees"]
    assert len(trees) == T == p.num_trees
    goss = p.goss_top_rate > 0
    keys, xkeys = gm.keys(p.seed, T), xm.keys(p.seed, T)
    plan = dm.plan(p.seed, p.drop_rate, p.max_drop, p.skip_drop, T, p.learning_rate) if p.drop_rate > 0 else None
    if plan is not None:
        assert st["dropped"] == [len(D) for D, _, _ in plan]
        assert np.asarray(d["Ensemble"]["weights"], dtype=np.float64).tobytes() == plan[-1][2].tobytes()
    else:
        assert d["Ensemble"]["weights"] == [p.learning_rate] * T
    mono = {int(k): int(v) for k, v in p.monotone_constraints.items()}
    traces = []
    for t in range(T):
        fsel, qsel = cm.sample(t)
        if plan is not None:
            D, before, after = plan[t]
            keep = dm.kept(t, D)
            fitted_to = ensemble([trees[i] for i in keep], before[keep])
        else:
            after = [p.learning_rate] * (t + 1)
            fitted_to = ensemble(trees[:t], after[:t])
        lam, wt = native.lambda_gradients(fitted_to, g, measure, p.sigma, queries=qsel if cm.subset(qsel) else None,
                                          truncation_level=p.truncation_level, lambda_norm=p.lambda_norm, objective=p.objective,
                                          xe_key=xkeys[t])
        lam, wt = np.nan_to_num(lam), np.nan_to_num(wt)
        rows = sm.instance_rows(cm.queries, qsel)
        if goss:
            rows, top, _, amp = gm.goss_list(lam, rows, cm.order_ids, p.goss_top_rate, p.goss_other_rate, keys[t])
            lam, wt = gm.amplified(lam, wt, cm.order_ids, rows, top, amp)
            assert st["goss_instances"][t] == len(rows)
        trace = []
        exp = rm.tree_on_sample(X, lam, wt, cm.order_ids, cm.feats, cm.binned, rows, list(fsel), p.max_depth, p.min_leaf_support,
                                p.split_candidates, reg, monotone=mono, max_leaves=p.max_leaves, symmetric=p.symmetric_trees,
                                trace=trace, **cm.newton())
        assert trees[t] == exp, "tree %d differs from the restatement's fit" % t
        traces.append(trace)
        tr, va, err = cm.measures(c.score_ensemble(trees[:t + 1], after))
        assert err == 0
        assert st["train_measure"][t] == tr, "train_measure[%d]" % t
        if va is not None:
            assert st["valid_measure"][t] == va, "valid_measure[%d]" % t
    assert np.array_equal(native.predict_scores_dense(model, g), c.score_ensemble(trees, d["Ensemble"]["weights"]))
    return model, st, traces


def datasets(X, y, qid):
    return fr.CDataset.from_numpy(X, y, qid), o.Dataset(X, y, qid)


def designed_gradients(X, seed):
    """Dyadic lambda / w by instance id, so that the fixed-point step is exact: lambda in sixteenths, w in sixteenths, and the
    six documents with the smallest values of feature 2 with w = 2^-20 and lambda = 2: a side made of them alone has a
    quotient near 2^21."""
    rng = np.random.default_rng(seed)
    n = len(X)
    lam = rng.integers(-64, 65, n).astype(np.float64) / 16.0
    wt = rng.integers(1, 17, n).astype(np.float64) / 16.0
    tiny = np.argsort(X[:, 2], kind="stable")[:6]
    wt[tiny], lam[tiny] = 2.0 ** -20, 2.0
    return lam, wt


def root_sides(X, lam, wt, order_ids, feats, k):
    """(G, q0 = G / H) of every side of every candidate of the root over the features `feats`, under lambda_l2 = 0."""
    from tests import lambdamart_hist_model as hm
    from tests import lambdamart_newton_model as nm

    order_ids = np.asarray(order_ids, dtype=np.int64)
    edges, xbin = hm.bin_matrix(X, order_ids, feats, k)
    n = len(order_ids)
    Q, S, W, Sw = nm.quantise_pair(lam[order_ids], wt[order_ids], n)
    cands, (_, qtot, wtot) = nm.candidates(xbin, edges, Q, W, np.arange(n), 1, S, Sw, 0.0, 0.0)
    G, q0 = [], []
    for _, _, qL, wL, ok, _ in cands:
        for q, w in ((qL[ok], wL[ok]), (qtot - qL[ok], wtot - wL[ok])):
            G.append(np.ldexp(q.astype(np.float64), -S))
            q0.append(G[-1] / np.ldexp(w.astype(np.float64), -Sw))
    return np.concatenate(G), np.concatenate(q0)


# --- the designed single-tree cases ---------------------------------------------------------------

KS = [2, 64, 65, 256]      # 1, 1, 2 and 4 bins per lane of the scan kernels, the last lanes empty or partial
FSEL = [0, 2, 3, 4]        # the tree's feature sample: the bin matrix's row differs from the histogram's feature slot
L2, CAP, SMOOTH = 2.0 ** -4, 0.5, 64.0
LEVELS = dict(max_depth=5, max_leaves=0)
LEAVES = dict(max_depth=8, max_leaves=8)


class Designed:
    """The designed case at k bins: data, dyadic gradients, lambda_l1 set exactly at some root side's |G|, and what the
    restatement says about it (checked here, on the CPU, so that the case cannot silently stop exercising a path)."""

    def __init__(self, k, seed=1):
        from tests import lambdamart_hist_model as hm

        self.k = k
        self.X, self.y, self.qid = small_dataset(seed)
        self.order_ids = np.arange(len(self.y))  # (queries are contiguous and ids ascending: the instance list is 0..n-1)
        self.feats = list(range(self.X.shape[1]))
        self.lam, self.wt = designed_gradients(self.X, seed + 1)
        self.binned = hm.bin_matrix(self.X, self.order_ids, self.feats, k)
        G, _ = root_sides(self.X, self.lam, self.wt, self.order_ids, FSEL, k)
        mags = np.sort(np.abs(G[G != 0.0]))
        self.l1 = float(mags[len(mags) // 3])
        assert np.any(np.abs(G) == self.l1) and np.any(np.abs(G) < self.l1)  # a side exactly at the threshold, and sides inside it
        den = self.wt.copy()
        tiny = np.flatnonzero(self.wt == 2.0 ** -20)
        assert len(tiny) == 6 and abs(self.lam[tiny].sum() / (den[tiny].sum() + L2)) > CAP  # the cap has a quotient to stop

    def regs(self):
        return {"l1": (self.l1, 0.0, 0.0), "cap": (0.0, CAP, 0.0), "smooth": (0.0, 0.0, SMOOTH), "all": (self.l1 / 4.0, CAP, SMOOTH)}

    def expected(self, reg, fsel=FSEL, trace=None, **kw):
        return rm.tree_on_sample(self.X, self.lam, self.wt, self.order_ids, self.feats, self.binned, self.order_ids, list(fsel),
                                 kw.pop("max_depth"), 1, self.k, reg, lambda_l2=L2, trace=trace, **kw)

    def grown(self, g, reg, fsel=FSEL, **kw):
        return native.hist_tree(g, self.lam, self.wt, self.k, kw.pop("max_depth"), 1, features=[self.feats[s] for s in fsel], split_gain="newton",
                                lambda_l2=L2, lambda_l1=reg[0], max_delta_step=reg[1], path_smooth=reg[2], **kw).to_dict()["DecisionTree"]


def smoothing_changes_a_winner(trace):
    return any(r["rival"] != (r["slot"], r["edge"]) for r in trace)


def parents_at(trace, depth):
    """The distinct parent outputs of the nodes that split at `depth`."""
    return {r["parent"] for r in trace if r["depth"] == depth}
