"""Training requests for the C ABI's `train_model` (JSON wire form: src/json_api.rs:13-34).

The public names and fields are those of the reference's Python package so that user code keeps
working (`TrainRequest`, `CoordinateAscentParams`, `RandomForestParams`; fastrank/training.py; plus
`LambdaMARTParams`), but
the implementation is table-driven: every parameter class registers its serde variant name in
`_VARIANTS`, and `TrainRequest` (de)serialises through that registry.
"""
import dataclasses
import random
from typing import Any, ClassVar, Dict, List, Optional, Sequence, Type

import numpy as np

from .clib import CQRel, query_json

_VARIANTS: Dict[str, Type["_LearnerParams"]] = {}
# one seed per process, like the reference module (its dataclass default is evaluated at import)
_PROCESS_SEED = random.getrandbits(64)


class _LearnerParams:
    """Behaviour shared by the learner parameter dataclasses."""

    VARIANT: ClassVar[str] = ""

    def __init_subclass__(cls, **kwargs):
        super().__init_subclass__(**kwargs)
        if cls.VARIANT:
            _VARIANTS[cls.VARIANT] = cls

    def name(self) -> str:
        return self.VARIANT

    def to_dict(self) -> Dict[str, Any]:
        return dataclasses.asdict(self)

    @classmethod
    def from_dict(cls, params: Dict[str, Any]):
        return cls(**params)


@dataclasses.dataclass
class CoordinateAscentParams(_LearnerParams):
    """src/coordinate_ascent.rs:11-41.  The wire form requires all ten keys."""

    VARIANT: ClassVar[str] = "CoordinateAscent"

    num_restarts: int = 5
    num_max_iterations: int = 25
    step_base: float = 0.05
    step_scale: float = 2.0
    tolerance: float = 0.001
    normalize: bool = True
    init_random: bool = True
    output_ensemble: bool = False
    seed: int = _PROCESS_SEED
    quiet: bool = False


@dataclasses.dataclass
class RandomForestParams(_LearnerParams):
    """src/random_forest.rs:127-157; trained on the device (csrc/rf_train.hpp, kernels_rf.inc).  As in the reference
    (fastrank/training.py:36-60) the dataclass default of `split_method` is a bare string, which the request parser --
    serde there, its restatement here -- rejects: requests made by `TrainRequest.random_forest()` carry the wire
    form {"SquaredError": []} (one of SquaredError, BinaryGiniImpurity, InformationGain, TrueVarianceReduction)."""

    VARIANT: ClassVar[str] = "RandomForest"

    num_trees: int = 100
    weight_trees: bool = True
    split_method: Any = "SquaredError"
    instance_sampling_rate: float = 0.5
    feature_sampling_rate: float = 0.25
    min_leaf_support: int = 10
    split_candidates: int = 3
    max_depth: int = 8
    seed: int = _PROCESS_SEED
    quiet: bool = False


@dataclasses.dataclass
class LambdaMARTParams(_LearnerParams):
    """Gradient-boosted regression trees fitted to LambdaRank gradients, trained on the device (csrc/lambdamart.hpp,
    kernels_lambda.inc).  The wire form requires the first seven keys.  Measures: ndcg and ndcg@k.
    `grower`: "exact" (the default; not written to the wire form) or "histogram" (features binned once into at most
    `split_candidates` <= 256 bins, per-node histograms: csrc/lambdamart_hist.hpp, kernels_hist.inc).
    `query_sampling_rate`, `feature_sampling_rate` (0 < r <= 1, default 1.0) and `seed` (u64, default 0): every tree is
    fitted to a fresh sample of that share of the view's queries (whole queries, never single documents) and may split on a
    fresh sample of that share of its features; the samples are a function of `seed` alone.  Like `grower` the three keys are
    written to the wire form only when they differ from their defaults; with both rates at 1.0 `seed` has no effect.
    `validation_queries` (query ids as `CDataset.queries()` spells them, default none): these queries are held out of every
    tree's gradients, splits and leaf values (per-tree query samples are then drawn from the others); the training stats
    report the measure over the training and the held-out queries after every tree (`train_measure`, `valid_measure`,
    `best_iteration`).  `early_stopping_rounds` = r > 0 (needs a held-out query): training ends r trees after the first
    maximum of `valid_measure`, and the model is the trees up to that maximum.  Both keys are written only when set;
    `hold_out_queries` makes a split.
    `split_gain`: "variance" (the default: splits maximise sL^2/nL + sR^2/nR over the gradients) or "newton" (histogram
    grower only: splits maximise G^2/(H + lambda_l2) over gradient sums G and hessian sums H, leaves are G/(H + lambda_l2)).
    `lambda_l2`, `min_sum_hessian`, `min_split_gain` (finite, >= 0, default 0.0; only with "newton"): the L2 term, the least
    hessian mass of a child, and the gain a split must exceed.  The four keys are written only when they differ from their
    defaults ("Newton split gain").
    `max_leaves`: 0 (the default: a tree is grown level by level down to `max_depth`) or at least 2 (histogram grower only):
    the tree is grown leaf-wise, always splitting the open leaf whose best split gains most, until it has `max_leaves`
    leaves or no leaf can be split; `max_depth` still bounds the depth.  Written only when set (DESIGN.md section 11,
    "Leaf-wise growth").
    `truncation_level`: 0 (the default: every pair of a query's documents with different labels contributes to the
    gradients) or T >= 1: a pair contributes only when the better ranked of the two is in the current top T.
    `lambda_norm` (default False): every query's gradients and weights are scaled by log2(1 + S_q) / S_q, S_q the query's
    summed pair terms, so that a few long queries do not dominate a tree.  Both growers; both keys are written only when
    set ("Truncation and normalisation").
    `objective`: "ndcg" (the default, not written), "map" or "mrr" ("ap" and "rr" are accepted and stored as "map" and
    "mrr"): what the gradients optimise.  Under "map" / "mrr" a pair is one relevant (label > 0) and one non-relevant
    document, weighted by the change of AP / RR their swap would make, and AP / RR takes over every role of the training
    measure: the training stats' `train_measure`, `valid_measure`, `best_iteration`, early stopping and the printed table.
    The request's `measure` must still name NDCG ("ndcg", "ndcg@k") -- "map" there is refused as before -- and is then read
    for nothing else.  Both growers, every other key ("Objectives").
    "xendcg" (lower case only) is the listwise cross-entropy objective: every document's gradient comes from the softmax of
    its query's scores against the randomised targets 2^label - gamma, at a cost linear in the query's length, where the
    pairwise objectives are quadratic.  gamma is a function of `seed`, the tree and the document.  The request's NDCG measure
    (with its `@k` and judgments) keeps every role of the training measure; `sigma` is accepted and not read;
    `truncation_level` != 0 and `lambda_norm` are refused with it, every other key composes (DESIGN.md section 11,
    "Listwise objective").
    `drop_rate` (0 <= r <= 1, default 0.0 = off): DART boosting.  Before tree t >= 1 is fitted, with probability
    1 - `skip_drop` (default 0.5) every earlier tree is dropped with probability `drop_rate`, at most `max_drop` of them
    (default 50, 0 = no cap, the smallest indices are kept); the tree is fitted to the ensemble without the k dropped trees,
    gets the weight learning_rate / (k + 1), and the dropped trees' weights are scaled by k / (k + 1).  The drops are a
    function of `seed` (a stream of their own: the per-tree samples do not move).  The model's weights are then no longer
    uniform; the training stats report `dropped` (k per tree), `dart_ms` and `dart_cache_bytes`.  `max_drop` / `skip_drop`
    need `drop_rate` > 0, and `early_stopping_rounds` cannot be combined with it (`validation_queries` can).  Both growers,
    every other key; the three keys are written only when they differ from their defaults ("DART").
    `monotone_constraints` (default none): feature name, as `CDataset.feature_names()` spells it, to +1 (with every other
    feature fixed the model's score never falls as this feature rises), -1 (it never rises) or 0 (no constraint; such
    entries are dropped from the wire form, and the key is written only when an entry is left).  Histogram grower under
    `split_gain` = "newton" only, level-wise and leaf-wise, with every other key; a name the dataset does not hold is an
    error when training starts.  The training stats then report `monotone_constraints` (feature id -> sign) and
    `monotone_clamped_leaves` (per tree, the leaves whose value a bound moved) ("Monotone
    constraints").
    `goss_top_rate` = a (0 <= a < 1, default 0.0 = off) and `goss_other_rate` = b (0 < b <= 1, default 0.1; a + b <= 1):
    gradient-based one-side sampling.  Every tree is fitted to the a-share of its documents with the largest |gradient| and
    to a random b-share of the others, whose gradients and hessians are multiplied by (1 - a) / b so that the sums the split
    gain reads stay unbiased; the gradient pass, the score update and the measures still cover every document.  The random
    part is a function of `seed`, the tree and the document (a stream of its own).  Histogram grower under `split_gain` =
    "newton" only, with every other key; `goss_other_rate` needs `goss_top_rate` > 0; both keys are written only when they
    differ from their defaults.  The training stats then report `goss_ms`, `goss_instances` and `goss_top` (per tree: the
    documents the tree was fitted to, and how many of them for their gradient) ("GOSS").
    `symmetric_trees` (default False; written only when set): symmetric (oblivious) trees.  Every node of a level splits on
    the same (feature, threshold), the candidate whose importance summed over the level's open nodes is largest; a node
    that cannot split under it becomes a leaf, so leaves may sit at any depth and every leaf still honours
    `min_leaf_support`.  One split has to pay off across a whole level, which regularises strongly.  Histogram grower,
    level-wise (`max_leaves` = 0) and without `monotone_constraints`; both split gains and every other key compose.  The
    trees are ordinary decision trees; the training stats then report `symmetric_trees` and `levels` (per tree, the levels
    that split) ("Symmetric trees").
    `lambda_l1`, `max_delta_step`, `path_smooth` (finite, >= 0, default 0.0 = off; written only when set): regularisation
    of the leaf outputs.  A node's gradient sum is soft-thresholded by `lambda_l1` before it becomes an output or a gain
    (small sums give a leaf of exactly 0); an output's magnitude is capped at `max_delta_step`, which bounds the leaves of
    nodes whose hessian sum is tiny (LambdaRank's hessians vanish for pairs the model already orders confidently);
    `path_smooth` pulls a child's output toward its parent's, the more strongly the fewer documents the child holds, which
    steadies small, deep leaves.  Histogram grower under `split_gain` = "newton" only, level-wise and leaf-wise, with
    every other key; `path_smooth` cannot be combined with `symmetric_trees`.  The training stats then report the three
    keys ("Leaf regularisation").
    `grad_quant_bits` = b (0, the default, = off, or 2..8; written only when set): quantised training.  After the gradient
    pass every tree rounds its gradients and hessians stochastically (unbiased) to b bits, searches its splits over
    histograms of those small integers, which the device builds with one packed atomic per update, and renews its leaves
    from the full-precision sums.  The rounding is a function of `seed`, the tree and the document (a stream of its own),
    so two runs give the same model.  Histogram grower under `split_gain` = "newton" only; composes with every other key
    but `monotone_constraints`, `lambda_l1`, `max_delta_step` and `path_smooth`, which are refused.  The training stats then
    report `grad_quant_bits` and `quant_ms` ("Quantised gradients").
    Two things are arguments of `CDataset.train_model`, not keys: `valid` (a second dataset the held-out measure and early
    stopping are read from; `validation_queries` must then be empty and `early_stopping_rounds` needs no held-out query)
    and `init_model` (an Ensemble of DecisionTrees training continues from: `num_trees` counts new trees, and the per-tree
    streams of `seed` resume at the model's tree count) ("Validation dataset", "Continued training")."""

    VARIANT: ClassVar[str] = "LambdaMART"

    num_trees: int = 100
    learning_rate: float = 0.1
    max_depth: int = 6
    min_leaf_support: int = 10
    split_candidates: int = 64
    sigma: float = 1.0
    quiet: bool = False
    grower: str = "exact"
    query_sampling_rate: float = 1.0
    feature_sampling_rate: float = 1.0
    seed: int = 0
    validation_queries: List[str] = dataclasses.field(default_factory=list)
    early_stopping_rounds: int = 0
    split_gain: str = "variance"
    lambda_l2: float = 0.0
    min_sum_hessian: float = 0.0
    min_split_gain: float = 0.0
    max_leaves: int = 0
    truncation_level: int = 0
    lambda_norm: bool = False
    objective: str = "ndcg"
    drop_rate: float = 0.0
    max_drop: int = 50
    skip_drop: float = 0.5
    monotone_constraints: Dict[str, int] = dataclasses.field(default_factory=dict)
    goss_top_rate: float = 0.0
    goss_other_rate: float = 0.1
    symmetric_trees: bool = False
    lambda_l1: float = 0.0
    max_delta_step: float = 0.0
    path_smooth: float = 0.0
    grad_quant_bits: int = 0

    _WIRE_DEFAULTS: ClassVar[Dict[str, Any]] = {"grower": "exact", "query_sampling_rate": 1.0, "feature_sampling_rate": 1.0, "seed": 0,
                                                "validation_queries": [], "early_stopping_rounds": 0, "split_gain": "variance",
                                                "lambda_l2": 0.0, "min_sum_hessian": 0.0, "min_split_gain": 0.0,
                                                "max_leaves": 0, "truncation_level": 0, "lambda_norm": False, "objective": "ndcg",
                                                "drop_rate": 0.0, "max_drop": 50, "skip_drop": 0.5, "monotone_constraints": {},
                                                "goss_top_rate": 0.0, "goss_other_rate": 0.1, "symmetric_trees": False,
                                                "lambda_l1": 0.0, "max_delta_step": 0.0, "path_smooth": 0.0, "grad_quant_bits": 0}
    _OBJECTIVES: ClassVar[Dict[str, str]] = {"ap": "map", "rr": "mrr", "xendcg": "xendcg"}

    def __post_init__(self):
        if isinstance(self.objective, str):  # (anything else is left for the request parser to refuse)
            self.objective = self._OBJECTIVES.get(self.objective, self.objective)

    def to_dict(self) -> Dict[str, Any]:
        wire = dataclasses.asdict(self)
        if isinstance(wire["monotone_constraints"], dict):  # (anything else is left for the request parser to refuse)
            wire["monotone_constraints"] = {k: v for k, v in wire["monotone_constraints"].items() if not (type(v) is int and v == 0)}
        for key, default in self._WIRE_DEFAULTS.items():  # serde: skip_serializing_if
            if wire[key] == default:
                del wire[key]
        return wire


def hold_out_queries(queries: Sequence[str], rate: float, seed: int = 0) -> List[str]:
    """A validation split for `LambdaMARTParams.validation_queries`: about `rate` of `queries` (e.g. `dataset.queries()`),
    at least one and at most all but one, chosen by numpy's `default_rng(seed)`; the result keeps the order of `queries`.
    The same arguments give the same split; a set, which has no order of its own (`dataset.queries()` is one), is sorted
    first."""
    queries = sorted(queries) if isinstance(queries, (set, frozenset)) else list(queries)
    if len(queries) < 2:
        raise ValueError("hold_out_queries needs at least two queries (one to train on, one to hold out)")
    if not 0.0 < float(rate) < 1.0:
        raise ValueError("hold_out_queries: rate must be greater than 0 and less than 1")
    count = min(len(queries) - 1, max(1, int(len(queries) * float(rate))))
    held = np.zeros(len(queries), dtype=bool)
    held[np.random.default_rng(int(seed)).permutation(len(queries))[:count]] = True
    return [q for q, h in zip(queries, held) if h]


@dataclasses.dataclass
class TrainRequest:
    """What to optimise (`measure`: "ndcg", "ndcg@10", "map", "mrr", ...), how (`params`) and,
    optionally, the judgments that define ideal gains / relevant counts."""

    measure: str = "ndcg"
    params: _LearnerParams = dataclasses.field(default_factory=CoordinateAscentParams)
    judgments: Optional[CQRel] = None

    def to_dict(self) -> Dict[str, Any]:
        wire: Dict[str, Any] = {"measure": self.measure, "params": {self.params.name(): self.params.to_dict()}}
        wire["judgments"] = self.judgments.to_dict() if self.judgments is not None else None
        return wire

    @staticmethod
    def from_dict(params: Dict[str, Any]) -> "TrainRequest":
        variants = params["params"]
        if len(variants) != 1:
            raise ValueError("What do I do with this?: {}".format(variants))
        (variant, fields), = variants.items()
        if variant not in _VARIANTS:
            raise ValueError("Python doesn't know about model-params: {}".format(variants))
        qrel = params.get("judgments")
        return TrainRequest(
            measure=params["measure"],
            params=_VARIANTS[variant].from_dict(fields),
            judgments=CQRel.from_dict(qrel) if qrel is not None else None,
        )

    def clone(self) -> "TrainRequest":
        """An independent copy (through the wire form)."""
        return TrainRequest.from_dict(self.to_dict())

    @staticmethod
    def _defaults(which: str) -> "TrainRequest":
        # defaults come from the native side, like the reference (src/ffi.rs:215-236)
        return TrainRequest.from_dict(query_json(which))

    @staticmethod
    def coordinate_ascent() -> "TrainRequest":
        return TrainRequest._defaults("coordinate_ascent_defaults")

    @staticmethod
    def random_forest() -> "TrainRequest":
        return TrainRequest._defaults("random_forest_defaults")

    @staticmethod
    def lambdamart() -> "TrainRequest":
        return TrainRequest._defaults("lambdamart_defaults")
