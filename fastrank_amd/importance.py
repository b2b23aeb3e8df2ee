"""Permutation importance: how far a measure falls when one feature at a time is shuffled, for any model `evaluate` takes,
scored on the device (include/fastrank.h, fr_permutation_importance)."""
from typing import Dict, List, Optional

from .clib import CDataset, CModel, CQRel


def permutation_importance(dataset: CDataset, model: CModel, evaluator: str, qrel: Optional[CQRel] = None, repeats: int = 5, seed: int = 0,
                           scope: str = "dataset", features: Optional[List[str]] = None) -> Dict:
    """For every feature of `features` (names; default: all the features of `dataset`, a dataset or any view), the mean of
    `evaluator` over the queries with that feature's column read from other rows, `repeats` times:

      "baseline"  the mean on the dataset as it is
      "features"  {name: {"importance": baseline minus the mean of the permuted values, "std": their sample standard
                  deviation (0.0 for one repeat), "values": the `repeats` permuted means}}
      "ranking"   the names by importance descending, then by feature id
      "skipped"   the names of features the model cannot read (no tree splits on them, a linear weight of exactly 0, ...):
                  never scored, importance and std exactly 0.0
      "repeats", "seed", "scope", "evaluator", and the call's "stats"

    scope "dataset" moves values across the whole dataset, "query" inside each query (the feature keeps its per-query
    distribution).  One permutation per (seed, repeat) is shared by all features, so their values are comparable, and a
    feature's values depend on neither `repeats` nor the other features asked for.  The same call gives the same bytes."""
    from . import native

    dataset._require_init()
    model._require_init()
    if qrel is not None:
        qrel._require_init()
    ids = None
    if features is not None:
        by_name = dataset.feature_name_to_index()
        unknown = [f for f in features if f not in by_name]
        if unknown:
            raise ValueError("permutation_importance: the dataset has no feature named {0!r}".format(unknown[0]))
        ids = [by_name[f] for f in features]
    rep, values, _ = native.permutation_importance_dense(model, dataset, evaluator, qrel=qrel, repeats=repeats, seed=seed, scope=scope, features=ids,
                                                         per_query=False)
    names = rep["names"]
    name_of = dict(zip(rep["features"], names))
    out = {"baseline": rep["baseline"], "features": {}}
    for k, name in enumerate(names):
        out["features"][name] = {"importance": rep["importance"][k], "std": rep["std"][k], "values": [float(v) for v in values[k]]}
    order = sorted(range(len(names)), key=lambda k: (-rep["importance"][k], rep["features"][k]))
    out["ranking"] = [names[k] for k in order]
    out["skipped"] = [name_of[f] for f in rep["skipped"]]
    for key in ("repeats", "seed", "scope", "evaluator", "stats"):
        out[key] = rep[key]
    return out
