"""Compare models on one dataset: bootstrap confidence intervals and a permutation test of their per-query values, resampled
on the device (include/fastrank.h, fr_compare_models)."""
import ctypes as C
import json
from typing import Dict, Optional

from .clib import CDataset, CModel, CQRel, _json_reply, _load


def compare_models(dataset: CDataset, models: Dict[str, CModel], evaluator: str, qrel: Optional[CQRel] = None, trials: int = 10000,
                   seed: int = 0, alpha: float = 0.05) -> Dict:
    """Evaluates every model of `models` ({name: model}, 1 to 8 of them) on `dataset` (a dataset or any view: the same
    queries in the same order for all) under `evaluator`, and resamples the per-query values `trials` times:

      "means"      {name: the observed mean over the queries}
      "intervals"  {name: [lo, hi]}: the bootstrap interval at level 1 - alpha (queries drawn with replacement, one draw for
                   every model, so the models stay paired; order statistics, no interpolation)
      "summary"    {name: {"p5", "p25", "p50", "p75", "p95"}} of the bootstrap means (CDataset.bootstrap_eval says how the
                   reference interpolates)
      "pairs"      one record per pair of models in the given order: {"a", "b": their names, "diff": mean a - mean b,
                   "diff_interval": the bootstrap interval of the difference, "p": the permutation test's p-value (each
                   query's values permuted among the models; the statistic is the range of the means, so the p-values of
                   three or more models are corrected for the number of pairs -- the randomised Tukey HSD test; for two
                   models this is the paired randomisation test), "wins" / "losses" / "ties": the queries where a is above /
                   below / equal to b}
      "systems" (the names in order), "queries", "trials", "seed", "alpha", and the device call's "stats"

    The result is a function of the values, `trials`, `seed` and `alpha` alone: the same call gives the same bytes."""
    dataset._require_init()
    names = list(models)
    if len(set(names)) != len(names):
        raise ValueError("compare_models: every model needs a name of its own")
    for m in models.values():
        m._require_init()
    pointers = (C.c_void_p * max(1, len(names)))(*[models[n].pointer for n in names])
    if qrel is not None:
        qrel._require_init()
    options = {"trials": int(trials), "seed": int(seed), "alpha": float(alpha)}
    rep = _json_reply(_load().fr_compare_models(pointers, len(names), dataset.pointer, None if qrel is None else qrel.pointer,
                                                evaluator.encode("utf-8"), json.dumps(options).encode("utf-8")))
    return named_report(rep, names)


def named_report(rep: Dict, names) -> Dict:
    """fr_resample's report (by column index) keyed by the systems' names."""
    out = {"systems": list(names), "trials": rep["trials"], "seed": rep["seed"], "alpha": rep["alpha"],
           "means": dict(zip(names, rep["means"]))}
    if "queries" in rep:
        out["queries"] = rep["queries"]
    if "intervals" in rep:
        out["intervals"] = dict(zip(names, rep["intervals"]))
        out["summary"] = dict(zip(names, rep["summary"]))
    out["pairs"] = []
    for p in rep["pairs"]:
        rec = {"a": names[p["i"]], "b": names[p["j"]]}
        rec.update((k, v) for k, v in p.items() if k not in ("i", "j"))
        out["pairs"].append(rec)
    out["stats"] = {k: rep[k] for k in ("boot_path", "boot_ms", "perm_ms", "upload_ms", "download_ms", "device_call_ms", "report_ms")}
    return out
