"""ctypes binding of libfastrank_amd.so that mirrors the reference's Python surface.

Same class / method names, argument meaning and error behaviour as the reference's
fastrank/clib.py (CQRel :62-121, CModel :124-209, CDataset :212-488, query_json :491-503), so a
user script only changes its import.  The reference binds a Rust cdylib through cffi; cffi is
not part of this image, and the C ABI is identical (include/fastrank.h), so this module uses
ctypes.  Nothing here computes: every call crosses the C ABI into the HIP library.
"""
import ctypes as C
import json
import os
from typing import Dict, List, Optional, Set

from . import _build

# model.rs:10-16 ModelEnum variants (clib.py:6 keeps the same list)
_MODEL_TYPES = ["SingleFeature", "Linear", "DecisionTree", "Ensemble"]


# int (*fr_allreduce_sum_fn)(void *ctx, double *values, size_t n)  (include/fastrank.h)
ALLREDUCE_SUM_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_size_t)


class _CResult(C.Structure):
    _fields_ = [("error_message", C.c_void_p), ("success", C.c_void_p)]


class HistTreeOptions(C.Structure):  # FrHistTreeOptions (include/fastrank.h); a fresh one is all zeros
    _fields_ = [("split_candidates", C.c_uint32), ("max_depth", C.c_uint32), ("min_leaf_support", C.c_uint32), ("newton", C.c_int32), ("lambda_l2", C.c_double),
                ("min_sum_hessian", C.c_double), ("min_split_gain", C.c_double), ("max_leaves", C.c_uint32), ("symmetric", C.c_int32), ("queries", C.c_void_p),
                ("n_queries", C.c_size_t), ("features", C.c_void_p), ("n_features", C.c_size_t), ("mono_features", C.c_void_p), ("mono_signs", C.c_void_p),
                ("n_mono", C.c_size_t), ("goss", C.c_int32), ("top_rate", C.c_double), ("other_rate", C.c_double), ("seed", C.c_uint64), ("tree", C.c_uint32),
                ("quant_bits", C.c_uint32), ("quant_seed", C.c_uint64), ("quant_tree", C.c_uint32),
                ("lambda_l1", C.c_double), ("max_delta_step", C.c_double), ("path_smooth", C.c_double)]


_lib = None


def _load():
    """dlopen the in-tree library (building it first if hipcc is around and it is stale)."""
    global _lib
    if _lib is not None:
        return _lib
    path = _build.LIB_PATH
    if _build.needs_build():
        try:
            _build.build()
        except Exception as exc:  # keep a stale-but-present library usable on boxes without hipcc
            if not os.path.exists(path):
                raise ImportError(
                    "libfastrank_amd.so is not built and could not be built: {}".format(exc)
                ) from exc
    L = C.CDLL(path)
    vp, sz = C.c_void_p, C.c_size_t
    res = C.POINTER(_CResult)
    sigs = {
        "free_str": (None, [vp]),
        "free_c_result": (None, [res]),
        "free_dataset": (None, [vp]),
        "free_model": (None, [vp]),
        "free_cqrel": (None, [vp]),
        "load_cqrel": (res, [C.c_char_p]),
        "cqrel_from_json": (res, [C.c_char_p]),
        "cqrel_query_json": (vp, [vp, C.c_char_p]),
        "load_ranksvm_format": (res, [C.c_char_p, C.c_char_p]),
        "dataset_query_sampling": (res, [vp, C.c_char_p]),
        "dataset_feature_sampling": (res, [vp, C.c_char_p]),
        "dataset_query_json": (vp, [vp, C.c_char_p]),
        "query_json": (vp, [C.c_char_p]),
        "make_dense_dataset_f32_f64_i64": (res, [sz, sz, vp, vp, vp]),
        "train_model": (res, [C.c_char_p, vp]),
        "model_from_json": (res, [C.c_char_p]),
        "model_query_json": (vp, [vp, C.c_char_p]),
        "evaluate_by_query": (vp, [vp, vp, vp, C.c_char_p]),
        "predict_scores": (vp, [vp, vp]),
        "predict_to_trecrun": (vp, [vp, vp, C.c_char_p, C.c_char_p, sz]),
        # extensions
        "fr_device_count": (C.c_int, []),
        "fr_set_device": (C.c_int, [C.c_int]),
        "fr_version": (C.c_char_p, []),
        "fr_train_model_shard": (vp, [C.c_char_p, vp, C.c_uint32, C.c_uint32]),
        "fr_select_model": (res, [C.c_char_p, C.c_int]),
        "fr_train_model_with": (res, [C.c_char_p, vp, vp, vp]),
        "fr_ca_begin": (vp, [C.c_char_p, vp, C.c_uint32, C.c_uint32, C.POINTER(vp)]),
        "fr_ca_begin_query_shard": (vp, [C.c_char_p, vp, C.c_uint64, ALLREDUCE_SUM_FN, vp, C.POINTER(vp)]),
        "fr_ca_step": (vp, [vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
        "fr_ca_state": (vp, [vp]),
        "fr_ca_free": (None, [vp]),
        "fr_ca_capture": (vp, [vp, C.c_int]),
        "fr_ca_capture_take": (vp, [vp, C.c_char_p, vp, sz]),
        "fr_last_train_stats": (vp, []),
        "fr_debug_tree_plan": (vp, []),
        "fr_debug_forest_pack": (vp, [vp, C.c_uint32, C.c_char_p, C.c_char_p, vp, sz]),
        "fr_debug_metric_plan": (vp, []),
        "fr_debug_measure_ranked": (vp, [C.c_char_p, vp, sz, C.c_double, vp]),
        "fr_debug_metric_topk_pays": (C.c_int, [C.c_int64, C.c_uint32]),
        "fr_predict_scores_dense": (vp, [vp, vp, vp, sz]),
        "fr_explain_dense": (vp, [vp, vp, vp, vp, sz, sz]),
        "fr_feature_importance": (vp, [vp, vp, vp, vp, sz]),
        "fr_debug_explain_table": (vp, [vp, vp, sz, C.c_uint32]),
        "fr_debug_lambda_gradients": (vp, [vp, vp, vp, C.c_char_p, C.c_double, vp, vp, sz]),
        "fr_debug_hist_bins": (vp, [vp, C.c_uint32, sz, sz, vp, vp, vp, vp, vp]),
        "fr_debug_hist_tree": (res, [vp, C.POINTER(HistTreeOptions), vp, vp, sz, vp]),
        "fr_debug_lambdamart_sample": (vp, [vp, C.c_char_p, C.c_uint32]),
        "fr_debug_lambdamart_dart_plan": (vp, [C.c_char_p, C.c_uint32]),
        "fr_debug_dart_scores": (vp, [vp, vp, vp, sz, vp, sz, vp, vp, sz]),
        "fr_debug_lambda_gradients_sampled": (vp, [vp, vp, vp, C.c_char_p, C.c_double, vp, sz, vp, vp, sz]),
        "fr_debug_goss_select": (vp, [vp, vp, sz, C.c_double, C.c_double, C.c_uint64, C.c_uint32, vp, sz, vp, vp, sz, vp, vp]),
        "fr_debug_rf_levels": (vp, [vp, vp, sz, vp, vp, C.c_uint32, C.c_uint32, C.c_int32, C.c_uint32, C.c_uint32, vp, sz]),
        "fr_debug_hist_quantise": (vp, [vp, vp, vp, sz, C.c_uint32, C.c_uint64, C.c_uint32, vp, sz, C.c_int32, C.c_double, C.c_double, C.c_uint64, C.c_uint32,
                                        vp, vp, sz, vp, vp]),
        "fr_debug_hist_root_histogram": (vp, [vp, vp, vp, sz, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, vp, sz, vp, vp, vp, sz]),
        "fr_debug_hist_reg_term": (vp, [C.c_int64, C.c_int64, C.c_uint32, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double,
                                        C.c_int32, C.c_double, C.c_double, C.c_double, vp, vp]),
        "fr_debug_lambda_gradients_opts": (vp, [vp, vp, vp, C.c_char_p, C.c_double, vp, sz, C.c_char_p, vp, vp, sz]),
        "fr_evaluate_dense": (vp, [vp, vp, vp, C.c_char_p, vp, sz, C.POINTER(vp)]),
        "fr_rank_order": (vp, [vp, vp, vp, sz, vp, sz]),
        "fr_dataset_num_queries": (sz, [vp]),
        "fr_dataset_num_instances": (sz, [vp]),
        "fr_dataset_device_info": (vp, [vp]),
        "fr_evaluate_candidates": (vp, [vp, vp, C.c_char_p, sz, vp, vp, vp, vp, vp, vp]),
        "fr_profile_enable": (None, [C.c_int]),
        "fr_profile_reset": (None, []),
        "fr_profile_json": (vp, []),
        "fr_debug_resident_bound": (C.c_double, [C.c_int, C.c_double, C.c_double, C.c_double]),
        "fr_debug_verify_end": (C.c_int, [C.c_int, sz, vp, vp, vp, vp, vp]),
        "fr_synchronize": (C.c_int, []),
        "fr_debug_device_plan": (vp, [C.c_char_p, C.c_int, C.c_uint32, C.c_int]),
        "fr_debug_fullrank_class": (C.c_uint32, [C.c_uint32]),
        "fr_debug_restart_queue": (vp, [C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_uint32]),
        "fr_dataset_release_replicas": (sz, [vp]),
        "fr_debug_peer_copy": (vp, [C.c_int, C.c_int, sz]),
        "fr_pack_restart_records": (vp, [C.c_char_p, sz, sz, vp]),
        "fr_unpack_restart_records": (vp, [vp, sz, sz]),
        "fr_rccl_allgather": (vp, [vp, sz, vp, sz, vp]),
        "fr_debug_rccl_selftest": (vp, [C.c_int]),
        "fr_debug_walk_tiles": (vp, [vp, vp, vp, sz, vp, vp, sz, sz]),
        "fr_debug_device_form": (vp, [vp, C.c_int, C.c_char_p, vp, sz]),
        "fr_debug_dataset_layout": (vp, [vp, vp, sz, vp, vp, sz, C.c_char_p, vp, sz]),
        "fr_load_ranksvm": (res, [C.c_char_p, C.c_char_p, C.c_char_p]),
        "fr_last_load_stats": (vp, []),
        "fr_debug_dataset_core": (vp, [vp, C.c_char_p, vp, sz]),
        "fr_debug_text_number": (vp, [C.c_char_p, sz, vp, vp, vp]),
        "fr_fit_normalizer": (vp, [vp, C.c_char_p]),
        "fr_normalize_dataset": (res, [vp, C.c_char_p]),
        "fr_resample": (vp, [vp, sz, sz, C.c_char_p, vp, vp]),
        "fr_compare_models": (vp, [C.POINTER(vp), sz, vp, vp, C.c_char_p, C.c_char_p]),
        "fr_permutation_importance": (vp, [vp, vp, vp, C.c_char_p, C.c_char_p, vp, sz, vp]),
        "fr_debug_permutation_sources": (vp, [vp, C.c_uint64, C.c_uint32, C.c_char_p, vp, sz]),
    }
    for name, (restype, argtypes) in sigs.items():
        fn = getattr(L, name)
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = L
    return L


def exported_symbols() -> List[str]:
    """Names this binding expects the shared object to export (used by the ABI test)."""
    _load()
    return [
        "free_str", "free_c_result", "free_dataset", "free_model", "free_cqrel", "load_cqrel",
        "cqrel_from_json", "cqrel_query_json", "load_ranksvm_format", "dataset_query_sampling",
        "dataset_feature_sampling", "dataset_query_json", "query_json",
        "make_dense_dataset_f32_f64_i64", "train_model", "model_from_json", "model_query_json",
        "evaluate_by_query", "predict_scores", "predict_to_trecrun",
    ]


def _take_str(ptr) -> Optional[str]:
    """Copy a library-allocated C string into Python and release it (free_str)."""
    if not ptr:
        return None
    try:
        return C.cast(ptr, C.c_char_p).value.decode("utf-8")
    finally:
        _load().free_str(ptr)


def _raise_if_error_str(text: Optional[str]):
    if text is None:
        return
    if "{" in text:
        payload = json.loads(text)
        if "error" in payload and "context" in payload:
            raise Exception("{0}: {1}".format(payload["error"], payload["context"]))
    else:
        raise Exception(text)


def _raise_if_error_json(payload):
    if isinstance(payload, dict) and "error" in payload and "context" in payload:
        raise Exception("{0}: {1}".format(payload["error"], payload["context"]))


def _unwrap(result_ptr):
    """CResult{error_message, success} -> success pointer, or raise (src/ffi.rs:57-74)."""
    if not result_ptr:
        raise ValueError("CResult should not be NULL")
    res = result_ptr.contents
    err_ptr, ok_ptr = res.error_message, res.success
    _load().free_c_result(result_ptr)
    _raise_if_error_str(_take_str(err_ptr))
    return ok_ptr


def _status(ptr):
    """Extension calls return NULL on success or an error-envelope string."""
    _raise_if_error_str(_take_str(ptr))


def _json_reply(ptr):
    payload = json.loads(_take_str(ptr))
    _raise_if_error_json(payload)
    return payload


class CQRel:
    """A loaded set of TREC relevance judgments (needed for MAP's relevant counts and NDCG's
    ideal gains when a dataset holds only part of the judged pool)."""

    def __init__(self, pointer=None):
        self.pointer = pointer
        self._queries = None

    def __del__(self):
        if getattr(self, "pointer", None) is not None and _lib is not None:
            _lib.free_cqrel(self.pointer)
            self.pointer = None

    @staticmethod
    def load_file(path: str) -> "CQRel":
        return CQRel(_unwrap(_load().load_cqrel(path.encode("utf-8"))))

    @staticmethod
    def from_dict(dictionaries: Dict[str, Dict[str, float]]) -> "CQRel":
        return CQRel(_unwrap(_load().cqrel_from_json(json.dumps(dictionaries).encode("utf-8"))))

    def _require_init(self):
        if self.pointer is None:
            raise ValueError("CQRel is null!")

    def _query_json(self, message="queries"):
        self._require_init()
        return _json_reply(_load().cqrel_query_json(self.pointer, message.encode("utf-8")))

    def to_dict(self) -> Dict[str, Dict[str, float]]:
        return self._query_json("to_json")

    def queries(self) -> Set[str]:
        if self._queries is None:
            self._queries = set(self._query_json("queries"))
        return self._queries

    def query_judgments(self, qid: str) -> Dict[str, float]:
        if qid in self.queries():
            return self._query_json(qid)
        raise ValueError("No qid={0} in cqrel: {1}".format(qid, self.queries()))


class CModel:
    """A trained or deserialised ranking model living behind the C ABI."""

    def __init__(self, pointer, params=None):
        self.pointer = pointer
        self.params = params

    @staticmethod
    def _check_model_json(model_json: Dict):
        [single_key] = list(model_json.keys())
        assert single_key in _MODEL_TYPES

    @staticmethod
    def from_dict(model_json: Dict) -> "CModel":
        CModel._check_model_json(model_json)
        return CModel(_unwrap(_load().model_from_json(json.dumps(model_json).encode("utf-8"))))

    def predict_dense_scores(self, dataset: "CDataset", missing: float = float("nan")) -> List[float]:
        """Scores as a list indexed by instance id, 0 .. the largest id the dataset view holds; ids it does not hold
        (a sampled view) read `missing` (same result as fastrank/clib.py:159-168)."""
        by_id = self.predict_scores(dataset)
        if not by_id:
            return []
        dense = [missing] * (max(by_id) + 1)
        for index, score in by_id.items():
            dense[index] = score
        return dense

    def predict_scores(self, dataset: "CDataset") -> Dict[int, float]:
        self._require_init()
        dataset._require_init()
        response = _json_reply(_load().predict_scores(self.pointer, dataset.pointer))
        return dict((int(k), v) for k, v in response.items())

    def __del__(self):
        if getattr(self, "pointer", None) is not None and _lib is not None:
            _lib.free_model(self.pointer)
            self.pointer = None

    def _require_init(self):
        if self.pointer is None:
            raise ValueError("CModel is null!")

    def _query_json(self, message="to_json"):
        self._require_init()
        return _json_reply(_load().model_query_json(self.pointer, message.encode("utf-8")))

    def to_dict(self):
        return self._query_json("to_json")

    def explain(self, dataset: "CDataset", background: Optional["CDataset"] = None):
        """Exact TreeSHAP feature contributions of a tree model for every document of `dataset`:
        an object with `values` (n x F float64 by instance id, NaN rows outside a sampled view), `feature_ids`,
        `feature_names` and `expected_value`; values.sum(1) + expected_value is the model's score.  The covers are
        counted on `background` (default: `dataset` itself)."""
        from . import native

        return native.explain_dense(self, dataset, background)

    def feature_importance(self, dataset: "CDataset", background: Optional["CDataset"] = None) -> Dict[str, float]:
        """{feature name: mean |contribution|} over the documents of `dataset`, reduced on the device."""
        from . import native

        ids, mean_abs, _ = native.feature_importance(self, dataset, background)
        names = dataset.feature_index_to_name()
        return dict((names[int(f)], float(v)) for f, v in zip(ids, mean_abs))

    def permutation_importance(self, dataset: "CDataset", evaluator: str, **kw) -> Dict:
        """How far `evaluator` falls on `dataset` when one feature at a time is shuffled: fastrank_amd.permutation_importance
         with this model; `kw`: qrel, repeats, seed, scope, features."""
        from .importance import permutation_importance

        return permutation_importance(dataset, self, evaluator, **kw)

    def __str__(self):
        return str(self.to_dict())


class CDataset:
    """A ranking dataset behind the C ABI: open_ranksvm() for files, from_numpy() for arrays.
    The first compute call uploads it to HBM (column-major features, query CSR)."""

    def __init__(self, pointer=None):
        self.pointer = pointer
        self.numpy_arrays_to_keep = []  # the library borrows these buffers (src/lib.rs:232-234)

    def __del__(self):
        if getattr(self, "pointer", None) is not None and _lib is not None:
            _lib.free_dataset(self.pointer)
            self.pointer = None
        self.numpy_arrays_to_keep = []

    @staticmethod
    def open_ranksvm(data_path, feature_names_path=None, parser="auto") -> "CDataset":
        """parser: "auto" (the device parser for texts of 32 MiB and more when a device is present), "host" or "device";
        the dataset and the errors are the same whichever runs ("Text loading")."""
        names = feature_names_path.encode("utf-8") if feature_names_path is not None else None
        if parser == "auto":
            return CDataset(_unwrap(_load().load_ranksvm_format(data_path.encode("utf-8"), names)))
        if parser not in ("host", "device"):
            raise ValueError('unknown parser {0!r}: expected one of "auto", "host", "device"'.format(parser))
        return CDataset(_unwrap(_load().fr_load_ranksvm(data_path.encode("utf-8"), names, parser.encode("utf-8"))))

    @staticmethod
    def from_numpy(X, y, qid) -> "CDataset":
        import numpy as np

        (N, D) = X.shape
        assert N > 0
        assert D > 0
        assert len(y) == N
        assert len(qid) == N
        assert X.dtype == "float32"
        assert y.dtype == "float64"
        assert qid.dtype == "int64"
        # the ABI reads a C-contiguous row-major matrix; np.matrix (.todense()) and strided views
        # are normalised here instead of being mis-read
        X = np.ascontiguousarray(np.asarray(X))
        y = np.ascontiguousarray(np.asarray(y).reshape(-1))
        qid = np.ascontiguousarray(np.asarray(qid).reshape(-1))
        keep = [X, y, qid]
        dataset = CDataset(
            _unwrap(_load().make_dense_dataset_f32_f64_i64(N, D, X.ctypes.data, y.ctypes.data, qid.ctypes.data))
        )
        dataset.numpy_arrays_to_keep = keep
        return dataset

    def _require_init(self):
        if self.pointer is None:
            raise ValueError("Forgot to call open_* or from_numpy on CDataset!")

    def subsample_queries(self, queries: List[str]) -> "CDataset":
        self._require_init()
        actual_queries = self.queries()
        for q in queries:
            if q not in actual_queries:
                raise ValueError(
                    "Asked for query that does not exist in subsample: {0} not in {1}".format(q, actual_queries)
                )
        child = CDataset()
        child.numpy_arrays_to_keep = self.numpy_arrays_to_keep
        child.pointer = _unwrap(_load().dataset_query_sampling(self.pointer, json.dumps(queries).encode("utf-8")))
        return child

    def subsample_feature_names(self, features: List[str]) -> "CDataset":
        name_to_id = dict(zip(self._query_json("feature_names"), self._query_json("feature_ids")))
        fnums = sorted(set(name_to_id[f] for f in features))
        child = CDataset(_unwrap(_load().dataset_feature_sampling(self.pointer, json.dumps(fnums).encode("utf-8"))))
        child.numpy_arrays_to_keep = self.numpy_arrays_to_keep
        return child

    def train_model(self, train_req: "TrainRequest", valid: Optional["CDataset"] = None,  # noqa: F821
                    init_model: Optional[CModel] = None) -> CModel:
        """Train on this dataset.  LambdaMART requests only: `valid` is a second dataset the held-out measure and early
        stopping are read from (no tree sees it); `init_model` is an Ensemble of DecisionTrees training continues from
        (num_trees then counts new trees).  DESIGN.md section 11, "Validation dataset" and "Continued training"."""
        self._require_init()
        request = json.dumps(train_req.to_dict()).encode("utf-8")
        if valid is None and init_model is None:
            return CModel(_unwrap(_load().train_model(request, self.pointer)), train_req)
        if valid is not None:
            valid._require_init()
        if init_model is not None:
            init_model._require_init()
        return CModel(_unwrap(_load().fr_train_model_with(request, self.pointer, None if valid is None else valid.pointer,
                                                          None if init_model is None else init_model.pointer)), train_req)

    def _query_json(self, message="num_features"):
        self._require_init()
        return _json_reply(_load().dataset_query_json(self.pointer, message.encode("utf-8")))

    def is_sampled(self) -> bool:
        return self._query_json("is_sampled")

    def num_features(self) -> int:
        return self._query_json("num_features")

    def feature_ids(self) -> Set[int]:
        return set(self._query_json("feature_ids"))

    def feature_names(self) -> Set[str]:
        return set(self._query_json("feature_names"))

    def feature_index_to_name(self) -> Dict[int, str]:
        return dict(zip(self._query_json("feature_ids"), self._query_json("feature_names")))

    def feature_name_to_index(self) -> Dict[str, int]:
        return dict(zip(self._query_json("feature_names"), self._query_json("feature_ids")))

    def num_instances(self) -> int:
        return self._query_json("num_instances")

    def queries(self) -> Set[str]:
        return set(self._query_json("queries"))

    def instances_by_query(self) -> Dict[str, List[int]]:
        return self._query_json("instances_by_query")

    def feature_stats(self) -> Dict[int, Dict[str, float]]:
        """{feature id: {"num_elements", "mean", "variance", "max", "min", "total"}} over the values this dataset or view
        holds, taken on the device: the records of Normalizer.fit(self, "zscore").  A feature held
        by fewer than two instances has no record."""
        return Normalizer.fit(self, "zscore").feature_stats()

    def normalization(self) -> Optional[dict]:
        """The normaliser that made this dataset (Normalizer.apply), as its wire form; None for any other dataset."""
        return self._query_json("normalization")

    def evaluate(self, model: CModel, evaluator: str, qrel: CQRel = None) -> Dict[str, float]:
        self._require_init()
        model._require_init()
        qrel_pointer = None
        if qrel is not None:
            qrel._require_init()
            qrel_pointer = qrel.pointer
        return _json_reply(
            _load().evaluate_by_query(model.pointer, self.pointer, qrel_pointer, evaluator.encode("utf-8"))
        )

    def bootstrap_eval(self, model: CModel, evaluator: str, qrel: CQRel = None, trials: int = 200, seed: int = 0) -> Dict:
        """The reference's SetEvaluator::bootstrap_eval (src/evaluators.rs:157-171) with PercentileStats::summary: the
        model's per-query values resampled with replacement `trials` times on the device.  Returns
        {"mean": the observed mean, "summary": {"p5", "p25", "p50", "p75", "p95"} of the trials' means, "interval": [lo, hi]
        at level 0.95 from order statistics}.  The percentiles are the reference's PercentileStats::percentile exactly as
        written, including its interpolation weights, which give the NEARER of the two order statistics the smaller
        weight.  The random numbers cannot be the reference's: it draws from oorandom's Rand64(0xdeadbeef), whose source is
        not available; the draws here are a function of `seed`, the trial and the number of queries."""
        from .compare import compare_models

        rep = compare_models(self, {"model": model}, evaluator, qrel=qrel, trials=trials, seed=seed)
        return {"mean": rep["means"]["model"], "summary": rep["summary"]["model"], "interval": rep["intervals"]["model"]}

    def predict_scores(self, model: CModel) -> Dict[int, float]:
        return model.predict_scores(self)

    def predict_trecrun(self, model: CModel, output_path: str, system_name: str = "fastrank", quiet=True,
                        depth=0) -> int:
        self._require_init()
        model._require_init()
        response = _json_reply(
            _load().predict_to_trecrun(
                model.pointer, self.pointer, output_path.encode("utf-8"), system_name.encode("utf-8"), depth
            )
        )
        if not quiet:
            print("Wrote {} records to {} as {}.".format(response, output_path, system_name))
        return response


_STAT_KEYS = ("num_elements", "mean", "variance", "max", "min", "total")


class Normalizer:
    """Feature normalisation (the reference's Normalizer, src/normalizers.rs): zscore and maxmin
    fitted on a dataset or a view of one, the same two per query (RankLib's scope, nothing fitted), and sigmoid.  It holds
    its wire form; statistics and transform run on the device."""

    def __init__(self, wire: dict):
        self._wire = Normalizer._checked(wire)

    @staticmethod
    def _method(method: str) -> str:
        if method in ("maxmin", "linear"):
            return "maxmin"
        if method in ("zscore", "sigmoid"):
            return method
        raise Exception("Unsupported Normalizer: {0}".format(method))

    @staticmethod
    def _checked(wire: dict) -> dict:
        import math

        if not isinstance(wire, dict) or len(wire) != 1:
            raise Exception("Unsupported Normalizer: {0!r}".format(wire))
        [(name, body)] = wire.items()
        if name == "SigmoidNormalizer":
            if body != []:
                raise Exception("Unsupported Normalizer: SigmoidNormalizer takes []")
            return {"SigmoidNormalizer": []}
        if name == "PerQuery":
            if not isinstance(body, str) or Normalizer._method(body) == "sigmoid":
                raise Exception("Unsupported Normalizer: {0}".format(body))
            return {"PerQuery": Normalizer._method(body)}
        if name not in ("ZScoreNormalizer", "MaxMinNormalizer"):
            raise Exception("Unsupported Normalizer: {0}".format(name))
        if not isinstance(body, dict) or not isinstance(body.get("feature_stats"), dict):
            raise Exception("Normalizer: missing field `feature_stats`")
        stats = {}
        for fid, rec in body["feature_stats"].items():
            if not isinstance(rec, dict) or int(fid) < 0:
                raise Exception("Normalizer: feature {0} has no record".format(fid))
            n = rec.get("num_elements")
            if not isinstance(n, int) or isinstance(n, bool) or n < 0:
                raise Exception("Normalizer: feature {0} has no count num_elements".format(fid))
            out = {"num_elements": n}
            for key in _STAT_KEYS[1:]:
                v = rec.get(key)
                if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                    raise Exception("Normalizer: feature {0} has no finite number for {1}".format(fid, key))
                out[key] = float(v)
            stats[str(int(fid))] = out
        return {name: {"feature_stats": stats}}

    @staticmethod
    def fit(dataset: CDataset, method: str) -> "Normalizer":
        """The statistics of the values `dataset` (often a view: the training queries) holds, feature by feature."""
        dataset._require_init()
        Normalizer._method(method)
        return Normalizer(_json_reply(_load().fr_fit_normalizer(dataset.pointer, method.encode("utf-8"))))

    @staticmethod
    def per_query(method: str) -> "Normalizer":
        method = Normalizer._method(method)
        if method == "sigmoid":
            raise Exception("Unsupported Normalizer: sigmoid")
        return Normalizer({"PerQuery": method})

    @staticmethod
    def sigmoid() -> "Normalizer":
        return Normalizer({"SigmoidNormalizer": []})

    @staticmethod
    def from_dict(wire: dict) -> "Normalizer":
        return Normalizer(wire)

    def to_dict(self) -> dict:
        return json.loads(json.dumps(self._wire))

    def feature_stats(self) -> Dict[int, Dict[str, float]]:
        [body] = self._wire.values()
        if not isinstance(body, dict):
            return {}
        return dict((int(fid), dict(rec)) for fid, rec in body["feature_stats"].items())

    def apply(self, dataset: CDataset) -> CDataset:
        """A new unsampled dataset that owns its matrix: `dataset`'s rows with every held value transformed.  `dataset`
        must be unsampled and must not be the result of an apply itself."""
        dataset._require_init()
        return CDataset(_unwrap(_load().fr_normalize_dataset(dataset.pointer, json.dumps(self._wire).encode("utf-8"))))


def query_json(message: str):
    """Global JSON query: 'coordinate_ascent_defaults' | 'random_forest_defaults' | 'lambdamart_defaults' | 'measures'."""
    return _json_reply(_load().query_json(message.encode("utf-8")))


def measures():
    """The evaluators every call takes by name: [{"name", "aliases", "display", "cutoff": "optional" | "required" | "ignored"}, ...]
    ("precision@10": name@k; names are matched without regard to case)."""
    return query_json("measures")
