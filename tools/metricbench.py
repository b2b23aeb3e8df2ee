"""metricbench.py -- the general metric pass (DeviceDataset::metric_from_scores) at the 30K shape under
both of its kernels: metric_sort_kernel (a bitonic sort of every query) and metric_topk_kernel (selection of the first k ranks),
forced with FR_METRIC_KERNEL.

For dcg and err at the depths 1, 10, 20 and 64, with 1 score slot (fr_evaluate_dense of a linear model) and with 64
(fr_evaluate_candidates: one line search's candidates through the general evaluator), --runs alternating rounds: the device
time of the pass alone (the profile's HIP events around its launches), in total and per size class.  `wins` lists, per depth,
the classes where the selection kernel's slowest run is below the sort kernel's fastest; `rule` is what metric_topk_pays says.

--parity adds what the project's standing rule asks of a change to this pass: fr_evaluate_dense under ndcg@10 (wall time per
call), and one permutation-importance call (linear model, every feature, 5 repeats) under dcg@10 against ndcg@10.

    python tools/metricbench.py --parity --out profiles/metric_topk_30k_bench.json

One JSON line (and the file).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bench import SHAPES, gen_mslr_shaped  # noqa: E402

DEPTHS = (1, 10, 20, 64)
MEASURES = ("dcg", "err")
SLOTS = (1, 64)


def spread(vals):
    return {"min": min(vals), "median": float(np.median(vals)), "max": max(vals)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="30k", choices=sorted(SHAPES))
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=3, help="calls timed per case and round")
    ap.add_argument("--parity", action="store_true", help="also time evaluate under ndcg@10 and permutation importance under dcg@10 / ndcg@10")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import fastrank_amd as fr
    from fastrank_amd import native

    n, d, q, seed = SHAPES[args.shape]
    X, y, qid = gen_mslr_shaped(seed, n, d, q)
    ds = fr.CDataset.from_numpy(X, y, qid)
    native.device_info(ds)
    rng = np.random.default_rng(1)
    w = rng.uniform(-1, 1, d)
    w /= np.abs(w).sum()
    model = fr.CModel.from_dict({"Linear": {"weights": w.tolist()}})
    cands = [list(np.linspace(-1.0, 1.0, 64))]

    def one_pass(evaluator, slots):
        """device ms of one metric pass: {"total": .., "<npad>": ..}, and the plan"""
        native.profile_reset()
        for _ in range(args.calls):
            if slots == 1:
                native.evaluate_dense(model, ds, evaluator)
            else:
                native.evaluate_candidates(ds, evaluator, [0], w[None, :], cands)
        stats = native.profile_stats()
        out = {"total": stats["metric_sort_kernel"]["total_ms"] / args.calls}
        for name, v in stats.items():
            if name.startswith("metric_sort_npad") or name.startswith("metric_topk_npad"):
                out[name.split("npad")[1]] = v["total_ms"] / args.calls
        return out, native.last_metric_plan()

    cases = [(m, k, s) for m in MEASURES for k in DEPTHS for s in SLOTS]
    runs = {"%s@%d/%d" % c: {"sort": [], "topk": []} for c in cases}
    classes = None
    native.profile_enable(True)
    try:
        for kernel in ("sort", "topk"):  # (the first launches' set-up, outside the rounds)
            os.environ["FR_METRIC_KERNEL"] = kernel
            one_pass("dcg@10", 1), one_pass("dcg@10", 64)
        for _ in range(args.runs):
            for m, k, s in cases:
                for kernel in ("sort", "topk"):
                    os.environ["FR_METRIC_KERNEL"] = kernel
                    ms, plan = one_pass("%s@%d" % (m, k), s)
                    assert {c["kernel"] for c in plan["classes"]} == {kernel}, plan
                    classes = {str(c["npad"]): c["queries"] for c in plan["classes"]}
                    runs["%s@%d/%d" % (m, k, s)][kernel].append(ms)
    finally:
        os.environ.pop("FR_METRIC_KERNEL", None)
        native.profile_enable(False)
    summary, wins = {}, {}
    for m, k, s in cases:
        key = "%s@%d/%d" % (m, k, s)
        rec = {}
        for part in ["total"] + sorted(classes, key=int):
            rec[part] = {kernel: spread([r[part] for r in runs[key][kernel]]) for kernel in ("sort", "topk")}
        summary[key] = rec
        wins[key] = [int(p) for p in sorted(classes, key=int) if rec[p]["topk"]["max"] < rec[p]["sort"]["min"]]
    rule = {str(k): [int(p) for p in sorted(classes, key=int) if native.metric_topk_pays(k, int(p))] for k in DEPTHS}
    # the rule may choose the selection kernel for no (depth, class) where its range lies above the sort kernel's
    above = [(key, p) for (m, k, s) in cases for key in ["%s@%d/%d" % (m, k, s)] for p in rule[str(k)]
             if summary[key][str(p)]["topk"]["min"] > summary[key][str(p)]["sort"]["max"]]
    out = {"metric": "general metric pass on MSLR-WEB30K shape" if args.shape == "30k" else "general metric pass", "shape": args.shape, "n": int(n),
           "d": int(d), "queries": int(q), "classes": classes, "calls_per_run": args.calls, "unit": "ms of device time per pass", "summary": summary,
           "topk_below_sort": wins, "rule": rule, "rule_chooses_a_slower_kernel": above, "runs": runs}
    if args.parity:
        def wall(call, times):
            call()
            t = time.perf_counter()
            for _ in range(times):
                call()
            return (time.perf_counter() - t) * 1e3 / times

        par = {"evaluate_ndcg@10_ms": [], "permimp_dcg@10_ms": [], "permimp_ndcg@10_ms": [], "permimp_dcg@10_metric_ms": [], "permimp_ndcg@10_metric_ms": []}
        for _ in range(args.runs):
            par["evaluate_ndcg@10_ms"].append(wall(lambda: native.evaluate_dense(model, ds, "ndcg@10"), 5))
            for ev in ("ndcg@10", "dcg@10"):
                t = time.perf_counter()
                rep, _, _ = native.permutation_importance_dense(model, ds, ev, repeats=5, seed=1, per_query=False)
                par["permimp_%s_ms" % ev].append((time.perf_counter() - t) * 1e3)
                par["permimp_%s_metric_ms" % ev].append(rep["stats"]["metric_ms"])
        out["parity"] = {k: dict(spread(v), runs=v) for k, v in par.items()}
        out["parity"]["permimp_plan"] = native.last_metric_plan()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
