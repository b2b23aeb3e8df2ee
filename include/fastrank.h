/*
 * fastrank.h -- C ABI of libfastrank_amd.so, the MI355X-native drop-in for the fastrank cdylib.
 *
 * Part 1 re-declares, symbol for symbol, the `extern "C"` surface the reference exports from
 * src/lib.rs (file:line cited per entry, paths relative to the jjfiv/fastrank tree) and that
 * fastrank/clib.py binds through cffi.  Semantics (ownership, JSON envelopes, error strings)
 * follow src/ffi.rs; see INTEGRATION.md for the binding a reference maintainer would add.
 *
 * Part 2 declares extensions (prefix `fr_`) that have no reference counterpart: device
 * selection, restart sharding for multi-GPU runs, dense (non-JSON) result buffers, direct
 * access to the batched line-search evaluator, and HIP-event kernel timing for bench.py.
 *
 * Strings: NUL-terminated UTF-8.  Every `const void*` / `const char*` JSON return value is
 * heap-allocated by the library and must be released with free_str().  A CResult is released
 * with free_c_result() (non-recursive: release error_message with free_str(), and the success
 * handle later with free_dataset()/free_model()/free_cqrel()).  Exactly one of the two CResult
 * fields is non-NULL.  Errors never use errno or exceptions: they are the JSON envelope
 * {"error":"error","context":"<Rust Debug form of the message>"} (src/ffi.rs:22-26,45-74).
 *
 * All ranking arithmetic runs on the GPU; there is no CPU fallback.  Calls that need the
 * device return an error envelope when no MI355X/HIP device is available.
 */
#ifndef FASTRANK_AMD_H
#define FASTRANK_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* src/lib.rs:50-61 -- opaque handles */
typedef struct CDataset CDataset;
typedef struct CModel CModel;
typedef struct CQRel CQRel;

/* src/lib.rs:63-67 */
typedef struct CResult {
    const void *error_message;
    const void *success;
} CResult;

/* ---------------------------------------------------------------------------------------- */
/* Part 1: the reference surface                                                            */
/* ---------------------------------------------------------------------------------------- */

/* src/lib.rs:78-81 */
void free_str(void *originally_from_library);
/* src/lib.rs:85-91 (non-recursive) */
void free_c_result(CResult *originally_from_library);
/* src/lib.rs:95-98 */
void free_dataset(CDataset *originally_from_library);
/* src/lib.rs:102-105 */
void free_model(CModel *originally_from_library);
/* src/lib.rs:109-112 */
void free_cqrel(CQRel *originally_from_library);

/* src/lib.rs:117-121: TREC qrel file -> CQRel */
const CResult *load_cqrel(const void *data_path);
/* src/lib.rs:126-131: {"qid":{"docid":gain}} -> CQRel */
const CResult *cqrel_from_json(const void *json_str);
/* src/lib.rs:136-142: "to_json" | "queries" | <qid> */
const void *cqrel_query_json(const CQRel *cqrel, const void *query_str);

/* src/lib.rs:147-162: ranksvm/libsvm text file (+ optional feature-name JSON) -> CDataset */
const CResult *load_ranksvm_format(void *data_path, void *feature_names_path_or_null);
/* src/lib.rs:167-178: JSON list of qid strings -> sampled CDataset */
const CResult *dataset_query_sampling(CDataset *dataset, const void *queries_json_list);
/* src/lib.rs:183-197: JSON list of feature ids -> sampled CDataset */
const CResult *dataset_feature_sampling(CDataset *dataset, const void *feature_json_list);
/* src/lib.rs:202-211: is_sampled | num_features | feature_ids | num_instances | queries |
 * instances_by_query | feature_names */
const void *dataset_query_json(void *dataset, void *json_cmd_str);
/* src/lib.rs:216-218: coordinate_ascent_defaults | random_forest_defaults */
const void *query_json(const void *json_cmd_str);

/* src/lib.rs:224-240: borrowed row-major f32 X[n*d], f64 y[n], i64 qid[n].  The caller keeps
 * the arrays alive for the lifetime of the dataset and of every dataset sampled from it. */
const CResult *make_dense_dataset_f32_f64_i64(size_t n, size_t d, const float *x, const double *y,
                                              const int64_t *qids);

/* src/lib.rs:245-253: TrainRequest JSON -> CModel.  The coordinate-ascent line search runs as
 * batched HIP launches (src/coordinate_ascent.rs:87-254); RandomForest requests are trained on the device too,
 * level-synchronously over batches of trees (src/random_forest.rs:211-408; csrc/rf_train.hpp, kernels_rf.inc).
 * With several devices visible (FR_DEVICES, default: all) the restarts of a coordinate-ascent request are spread
 * over them inside this call, like the reference's rayon fan-out over restarts (src/coordinate_ascent.rs:215-225),
 * and so are the trees of a random-forest request (src/random_forest.rs:301-331). */
const CResult *train_model(void *train_request_json, void *dataset);
/* src/lib.rs:258-263 */
const CResult *model_from_json(const void *json_str);
/* src/lib.rs:268-277: "to_json" */
const void *model_query_json(const void *model, const void *json_cmd_str);

/* src/lib.rs:283-294: {qid: metric}; qrel may be NULL */
const void *evaluate_by_query(const CModel *model, const CDataset *dataset, const CQRel *qrel,
                              const void *evaluator_name);
/* src/lib.rs:299-303: {"<instance index>": score} */
const void *predict_scores(const CModel *model, const CDataset *dataset);
/* src/lib.rs:308-326: writes a TREC run file; JSON number of records written */
const void *predict_to_trecrun(const CModel *model, const CDataset *dataset, const void *output_path,
                               const void *system_name, size_t depth);

/* ---------------------------------------------------------------------------------------- */
/* Part 2: extensions (no reference counterpart)                                            */
/* ---------------------------------------------------------------------------------------- */

/* Number of visible HIP devices (0 when none / no driver). */
int fr_device_count(void);
/* Select the device used by datasets created afterwards on this thread. 0 on success.  The first call for a device also
 * pays the runtime's first-stream cost there (~80 ms once per process), so that the first dataset built on it does not. */
int fr_set_device(int ordinal);
/* Library/ABI version string (static storage; do NOT free). */
const char *fr_version(void);

/* Restart-sharded coordinate ascent for one-process-per-GPU runs: trains restarts
 * [restart_begin, restart_end) of the request's num_restarts (child seeds are still drawn in
 * order from the master RNG, src/coordinate_ascent.rs:211-213) and returns JSON
 * {"restarts":[{"restart_id":r,"score":s,"weights":[...]}...],"stats":{...}}.
 * The caller gathers shards (RCCL all_gather) and applies fr_select_model(). */
const void *fr_train_model_shard(const void *train_request_json, const CDataset *dataset,
                                 uint32_t restart_begin, uint32_t restart_end);
/* Steppable form of the same trainer (what bench.py times): begin -> step(k ticks)* -> state.
 * One tick = one fused launch evaluating every line-search candidate of every live restart.
 * fr_ca_begin returns NULL and sets *error_out (free_str) on failure. */
void *fr_ca_begin(const void *train_request_json, const CDataset *dataset, uint32_t restart_begin,
                  uint32_t restart_end, const void **error_out);
/* Query-sharded form (fewer restarts than GPUs).  `dataset` holds this rank's block of
 * the queries; all ranks run ALL restarts in lock step.  After every device evaluation the trainer
 * hands the per-candidate SUMS over its queries to `allreduce(ctx, values, n)`, which must replace
 * values[i] with the sum over all ranks added in rank order (identical bits on every rank; e.g.
 * all_gather + a sequential add) and return 0; the trainer divides by total_queries.  Step and read
 * it with fr_ca_step / fr_ca_state; every rank ends with the same restarts. */
typedef int (*fr_allreduce_sum_fn)(void *ctx, double *values, size_t n);
void *fr_ca_begin_query_shard(const void *train_request_json, const CDataset *dataset, uint64_t total_queries,
                              fr_allreduce_sum_fn allreduce, void *ctx, const void **error_out);
/* Runs up to max_ticks ticks; NULL on success. *finished = 1 once every restart converged.  Inside the call the
 * restarts are stepped as a few sets with one line search of each in flight on the device; everything submitted has
 * been collected and applied when the call returns, so the state is the lock-step state after *ticks_done ticks. */
const void *fr_ca_step(void *trainer, uint64_t max_ticks, uint64_t *ticks_done, int *finished);
/* JSON {"restarts":[...],"stats":{...},"finished":bool} (free_str). */
const void *fr_ca_state(void *trainer);
void fr_ca_free(void *trainer);
/* Tick capture, a test hook: while on (off is the default and costs an untaken branch), the device
 * dataset of this trainer appends an event to a host-side log at every store of exact resident sums and at every collected
 * line search -- its groups, staging order, path, kernel instantiation, redo list, published means and per-query matrix, and
 * the resident sums it left.  It reads only: no counter, policy decision or published value changes.  NULL on success. */
const void *fr_ca_capture(void *trainer, int on);
/* Hands the log over and clears it, with the name / out-buffer protocol of fr_debug_device_form.  table == NULL: JSON
 * {"events": [...], "bytes": n}, every array of an event given as {"off": byte offset, "n": elements} into one blob of n
 * bytes; table == "blob": the blob is copied to `out` (out_bytes must be n) and forgotten. */
const void *fr_ca_capture_take(void *trainer, const void *table, void *out, size_t out_bytes);

/* Selection rule of src/coordinate_ascent.rs:232-252 over gathered restarts.
 * restarts_json: JSON list of {"restart_id","score","weights"}; returns a CModel. */
const CResult *fr_select_model(const void *restarts_json, int output_ensemble);
/* train_model with a validation dataset and / or a model to continue from (LambdaMART requests only; DESIGN.md section 11,
 * "Validation dataset" and "Continued training").  With both NULL it is train_model.  valid_dataset_or_null: a second dataset
 * (file-loaded, from arrays, or a sampled view -- a sibling view of the trained one's parent included) that no tree reads; it
 * is scored after every tree on its own device form, and the mean of the request's measure over all of its queries is the
 * held-out measure early_stopping_rounds reads (validation_queries must then be empty).  It must hold every feature of the
 * trained view and live on the same device.  init_model_or_null: an Ensemble of DecisionTrees (T0 of them); num_trees counts
 * NEW trees, new tree j takes every per-tree random stream at index T0 + j, and the result is the init model's trees and
 * weights followed by the new ones (not with drop_rate > 0).  Returns a CModel; both datasets' locks are held for the call. */
const CResult *fr_train_model_with(const void *train_request_json, const CDataset *dataset, const CDataset *valid_dataset_or_null,
                                   const CModel *init_model_or_null);
/* JSON stats of the most recent train_model / fr_train_model_shard call in this process:
 * {"useful_evals","raw_evals","ticks","groups","seconds","path","restarts","verify_pairs","verify_redone",
 *  "exact_ticks","exact_groups","verify_redo_entries","line_searches","audit_values","audit_mismatches","devices",
 *  "refills","chain_runs","chain_visits","rank_slots_on","rank_slots_off"} (chain_*: documents that made the NDCG@k verify
 * kernel run its insertion chain, out of (document, group) visits -- the kernel's own counter; rank_slots_*: restarts whose
 * R-rank upkeep that counter switched on again / off) and, after a call that spread over several devices, "rccl": the report
 * of the exchange (fr_rccl_allgather below); and, after a call that ran
 * on several devices, "per_device": the same object for every entry of the device list (its "device", "restarts",
 * "ticks", "seconds", "refills": times converged restarts handed their places to ids from the shared restart queue)
 * (path: "fused_linesearch" | "fused_fullrank" | "generic_sort"; verify_*: (query, group) pairs evaluated by the
 * bound-and-verify kernels and how many of them were recomputed by the exact kernels -- NDCG@k recomputes only the
 * 16-candidate slices of a pair that hold an undecided candidate: verify_redo_entries counts those; exact_ticks of
 * line_searches batched line searches went to the exact kernels alone, exact_groups of groups single restarts' line
 * searches were routed there while the rest of their tick stayed on the verify kernel; audit_*: with FR_VERIFY_AUDIT=1 every value a
 * bound-and-verify line search publishes (NDCG@k, full ranking, reciprocal rank) is recomputed by the exact kernels and
 * compared bit for bit -- values compared / values that differed).
 * fr_train_model_with sets the stats as train_model does.  After a LambdaMART request a "lambdamart" object is added (DESIGN.md
 * section 11 lists its keys); fr_train_model_with adds to it, only with a validation dataset: "valid_dataset_queries",
 * "valid_dataset_instances", "valid_ms" (the validation side's wall time, outside "update_ms"), "valid_measure" (per new tree),
 * "best_iteration", "best_valid_measure", "stopped_early", "early_stopping_rounds" and, under DART, "valid_dart_cache_bytes" (that
 * dataset's own leaf cache, next to "dart_cache_bytes"); only with an init model: "init_trees", "init_train_measure",
 * "init_valid_measure" (with a validation dataset or validation_queries), "init_ms" (forming the initial scores); "trees",
 * "train_measure" and "valid_measure" then count new trees, "best_iteration" counts the returned model's. */
const void *fr_last_train_stats(void);
/* What the process's last forest-scoring call ran, a test hook; JSON (free_str), no timing in it and
 * no launch behind it: {"path": "rank" | "lds" | "l2" (null before the first call), "cache_hit": the rank path launched from
 * the buffers the call before left; lds: "docs", "parts" (the block shape); l2: "rows_in_lds"; rank: "nslots" (features in
 * use), "nrounds"; rank and lds: "batches": [[walks per thread, levels], ...]}. */
const void *fr_debug_tree_plan(void);
/* Test hook, no device: `model`'s forest (a DecisionTree or an Ensemble of DecisionTrees) packed on the host for one encoding of
 * DESIGN.md section 5.6 (csrc/forest_pack.hpp) on a dataset of dataset_features features -- the buffers a scoring call would
 * upload.  encoding: "rank", "lds:DOCS,PARTS" (one block shape of the f32 LDS walk) or "l2".  JSON (free_str): {"admitted":
 * false when the forest lies outside a limit of the encoding, "hash": the packed-forest cache's key as hex, "tables": {name:
 * bytes} (rank: "fdesc", "tables", "rdesc", "forest", "desc", "leafprod"; lds: "forest", "desc", "leafprod"; l2: "nodes",
 * "roots", "tweights"), rank and lds: "lds_bytes", "batches": [[walks per thread, levels], ...]; rank: "nslots", "nrounds"}.
 * table == NULL: the JSON alone; else also the named table's bytes into out[out_bytes], with the name / out-buffer protocol
 * of fr_debug_device_form (a wrong out_bytes or a name the encoding does not have is an error). */
const void *fr_debug_forest_pack(const CModel *model, uint32_t dataset_features, const void *encoding, const void *table,
                                 void *out, size_t out_bytes);
/* What the process's last general metric pass launched, a test hook; JSON (free_str), host
 * bookkeeping alone: {"measure": the measure's first name (null before the first call), "depth": the cut-off or null,
 * "slots": score slots evaluated at once, "classes": [{"npad": the size class, "queries", "kernel": "sort" | "topk"}, ...]}.
 * "topk" is the selection kernel, which only dcg, precision, recall, success and err at a cut-off of 1 .. 64 can take;
 * FR_METRIC_KERNEL=sort|topk in the environment forces one kernel wherever it is legal (same results). */
const void *fr_debug_metric_plan(void);
/* The scalar definition (csrc/measures_host.hpp) of dcg[@k], precision@k, recall[@k], success@k or err[@k] over a RANKED list
 * of n gains, on the host: *out = the value.  norm: what the query's norm would be -- precision: k; recall: the number of
 * relevant documents (0: the list's own); err: 2^(largest gain); else unused.  Returns NULL, or an error text (free_str). */
const void *fr_debug_measure_ranked(const void *evaluator, const float *gains, size_t n, double norm, double *out);
/* 1 if the general metric pass gives a size class of npad documents (a power of two >= 64) to the selection kernel at this
 * cut-off when nothing forces a kernel, else 0. */
int fr_debug_metric_topk_pays(int64_t depth, uint32_t npad);

/* Dense results without JSON.  out[i] = score of instance i (instances outside the dataset
 * view are left untouched).  Returns NULL on success or an error-envelope string. */
const void *fr_predict_scores_dense(const CModel *model, const CDataset *dataset, double *out, size_t out_len);
/* Per-query metric in the dataset's device query order.  out_values[nq]; out_qids (optional)
 * receives a JSON list of the qid strings in the same order via *out_qids_json (free_str). */
const void *fr_evaluate_dense(const CModel *model, const CDataset *dataset, const CQRel *qrel,
                              const void *evaluator_name, double *out_values, size_t out_len,
                              const void **out_qids_json);
/* Model explanation: exact TreeSHAP feature contributions of a DecisionTree or an Ensemble of
 * DecisionTrees, path-dependent, with the covers counted on `background_or_null` (NULL: the explained dataset itself).
 * out[id * cols + c], id = instance id as in fr_predict_scores_dense (rows outside the dataset view, and ids >= rows, are
 * left as the caller filled them); the columns are the dataset's feature ids ascending, then the bias, so cols must be
 * num_features + 1.  A row's sum is the model's score of the document up to rounding.  Returns JSON (free_str):
 * {"feature_ids": [...], "split_counts": [...], "expected_value": bias, "trees", "leaf_paths", "max_path", "documents",
 *  "cover_ms", "kernel_ms", "copy_ms"}, or the error envelope.  Refused: Linear and SingleFeature models, nested ensembles,
 * a background with no instance, a root-to-leaf path with more than 32 distinct features, an output that does not fit the
 * device's free memory (or FR_EXPLAIN_MAX_BYTES, if that is smaller). */
const void *fr_explain_dense(const CModel *model, const CDataset *dataset, const CDataset *background_or_null,
                             double *out, size_t rows, size_t cols);
/* out_mean_abs[f] = the mean over the dataset's documents of |phi_f|, columns as above without the bias; the documents
 * are explained and reduced on the device 65 536 at a time in a fixed shape (same bytes every run), the matrix is never
 * kept or downloaded.  The same JSON; "split_counts" = split nodes per feature over all trees. */
const void *fr_feature_importance(const CModel *model, const CDataset *dataset, const CDataset *background_or_null,
                                  double *out_mean_abs, size_t n_features);
/* Test hook, no device: the path table the explain kernel would read for `model` when leaf_counts[n_leaves] documents of
 * the background reach its leaves (depth first, tree after tree) on a dataset of dataset_features features.  JSON; doubles
 * travel as the hex of their bits. */
const void *fr_debug_explain_table(const CModel *model, const uint32_t *leaf_counts, size_t n_leaves,
                                   uint32_t dataset_features);
/* LambdaMART test hook: one gradient pass on the scores of `model` for `measure` (ndcg or ndcg@k;
 * qrel-judged norms when qrel is given) with sigmoid scale sigma.  lambda_out / weight_out[i] = the
 * LambdaRank gradient / weight of instance i (instances outside the view are left untouched).
 * Returns NULL on success or an error-envelope string. */
const void *fr_debug_lambda_gradients(const CModel *model, const CDataset *dataset, const CQRel *qrel,
                                      const void *measure, double sigma, double *lambda_out,
                                      double *weight_out, size_t out_len);
/* LambdaMART histogram grower, test hooks.  The view's instance list (queries in the view's
 * order, ids ascending inside each; n entries) and features (ascending; f entries) are written to ids_out / feats_out.
 * edges_out[s * 256 + j], j < nedges_out[s]: the edges of feature slot s for k = split_candidates (2..256);
 * bins_out[s * n + i]: the bin of instance-list entry i.  Returns NULL on success or an error-envelope string. */
const void *fr_debug_hist_bins(const CDataset *dataset, uint32_t split_candidates, size_t n, size_t f,
                               uint32_t *ids_out, uint32_t *feats_out, float *edges_out,
                               uint32_t *nedges_out, uint8_t *bins_out);
/* LambdaMART per-tree samples, test hooks ("Sampling").  fr_debug_lambdamart_sample: JSON
 * {"features": [feature ids ascending], "queries": [indices of the view's queries, ascending]} the trainer uses for
 * tree `tree` of the LambdaMART parameters params_json on this view; no device is touched.
 * fr_debug_lambda_gradients_sampled takes queries[n_queries] = indices of the view's queries; only instances of the
 * named queries are written. */
const void *fr_debug_lambdamart_sample(const CDataset *dataset, const void *params_json, uint32_t tree);
const void *fr_debug_lambda_gradients_sampled(const CModel *model, const CDataset *dataset, const CQRel *qrel,
                                              const void *measure, double sigma, const uint32_t *queries,
                                              size_t n_queries, double *lambda_out, double *weight_out,
                                              size_t out_len);
/* What fr_debug_hist_tree grows its one tree with; a zeroed struct with the first three fields set is a plain level-wise
 * tree under the variance criterion. */
typedef struct FrHistTreeOptions {
    uint32_t split_candidates, max_depth, min_leaf_support; /* max_depth >= 1 */
    /* newton != 0: the Newton split gain ("Newton split gain"): splits by G^2 / (H + lambda_l2) with the floors
     * min_sum_hessian and min_split_gain, leaves G / (H + lambda_l2).  The three numbers finite and >= 0, and 0 without it. */
    int32_t newton;
    double lambda_l2, min_sum_hessian, min_split_gain;
    /* 0: level-wise; >= 2: leaf-wise under that leaf budget ("Leaf-wise growth"): the open leaf with the largest gain is
     * split next */
    uint32_t max_leaves;
    /* != 0 ("Symmetric trees"; level-wise, without monotone signs or GOSS): every node of a level splits on the level's
     * one winning candidate */
    int32_t symmetric;
    /* the tree's sample ("Sampling"): indices of the view's queries / feature ids of the view (NULL = all); gradients of
     * instances outside the query sample are not read */
    const uint32_t *queries;
    size_t n_queries;
    const uint32_t *features;
    size_t n_features;
    /* "Monotone constraints" (Newton gain only): feature ids of the view and their signs in {-1, 0, 1} */
    const uint32_t *mono_features;
    const int32_t *mono_signs;
    size_t n_mono;
    /* goss != 0 ("GOSS"; Newton gain only): the tree is fitted to the GOSS list of the sample's instance list, the kept
     * others' lambda / weight amplified.  top_rate in (0, 1), other_rate in (0, 1], their sum at most 1; the tree's key is
     * that of tree `tree` of the request seed `seed`. */
    int32_t goss;
    double top_rate, other_rate;
    uint64_t seed;
    uint32_t tree;
    /* quant_bits != 0 ("Quantised gradients"; 2..8; Newton gain only, without monotone signs or leaf regularisation): the
     * searches read sums of gradients rounded stochastically to quant_bits bits under the key of tree quant_tree of the request
     * seed quant_seed; the leaves are renewed from the full-precision sums.  (The record still ends with the three doubles.) */
    uint32_t quant_bits;
    uint64_t quant_seed;
    uint32_t quant_tree;
    /* "Leaf regularisation" (Newton gain only; finite and >= 0, all 0: off): the gradient sum is soft-thresholded by
     * lambda_l1, an output's magnitude is capped at max_delta_step, a child's output is pulled toward its parent's by
     * path_smooth (not with symmetric). */
    double lambda_l1, max_delta_step, path_smooth;
} FrHistTreeOptions;
/* One histogram tree (a DecisionTree model) grown from lambda / weight indexed by instance id (len
 * entries).  Options that contradict each other or are out of range are refused before the dataset is looked at.
 * *clamped_leaves_out (may be NULL): the leaves whose value a monotone bound moved. */
const CResult *fr_debug_hist_tree(const CDataset *dataset, const FrHistTreeOptions *opt, const double *lambda,
                                  const double *weight, size_t len, uint32_t *clamped_leaves_out);
/* The GOSS selection alone (rates, seed and tree as in FrHistTreeOptions) for lambda[len] by instance id, over the
 * instances of queries[n_queries] (NULL = all).  list_out / top_out[cap] (cap >= the view's instances): the GOSS list as
 * ascending indices into the view's instance list, and per entry whether it belongs to the top set; *n_g_out: the list's
 * length; *tau_out: the n_top-th largest of the 64-bit patterns of |lambda|. */
/* The leaf regularisation's host arithmetic for one integer pair (q, w) of n instances ("Leaf
 * regularisation"; no device is touched): *v_out = the output, *term_out = its term.  has_parent == 0: the root, parent is
 * not read.  [lo, hi]: the node's interval (-inf, +inf: none). */
const void *fr_debug_hist_reg_term(int64_t q, int64_t w, uint32_t n, int32_t s_l, int32_t s_w, double lambda_l1,
                                   double lambda_l2, double max_delta_step, double path_smooth, int32_t has_parent,
                                   double parent, double lo, double hi, double *v_out, double *term_out);
const void *fr_debug_goss_select(const CDataset *dataset, const double *lambda, size_t len, double top_rate,
                                 double other_rate, uint64_t seed, uint32_t tree, const uint32_t *queries, size_t n_queries,
                                 uint32_t *list_out, uint8_t *top_out, size_t cap, uint32_t *n_g_out, uint64_t *tau_out);
/* Random-forest training, test hook: ONE batch of n_trees trees grown by the trainer's own level loop
 * with every level recorded.  Tree t grows over the instance ids root_ids[root_off[t] .. root_off[t + 1]) in that order
 * (root_off[0] = 0) and the features feats[t * nf .. t * nf + nf).  out == NULL: grows, keeps the record and returns a JSON
 * header -- "levels": per level {"A", "items", "children_from": "candidates" | "rf_childsum_kernel"}; "sections": per array
 * {"level", "name", "offset", "bytes"} inside the record, names active ([A] x (tree, key, n) u32), depth ([A] u32),
 * label_minmax ([A][2] f32), cands ([A][nf][k-1] x the 48-byte candidate record: position f64, importance f64, ids_i u32,
 * flags u32, pos_l u32, pos_r u32, sum_l f64, sum_r f64), svals / sv / sg ([items] u32 / f32 / f32: the level's sorted arrays
 * as the device holds them), splits ([A] x (fslot i32, pos, left, right u32)), child_out ([A][2] f64), and after the last level
 * root_out ([n_trees] f64 where a root did not split, else empty); "trees": the finished DecisionTree models; "bytes": the
 * record's size.  out != NULL: copies the kept record (out_bytes must be its size) and forgets it; the other arguments are
 * not read. */
const void *fr_debug_rf_levels(const CDataset *dataset, const uint32_t *root_off, size_t n_trees, const uint32_t *root_ids,
                               const uint32_t *feats, uint32_t nf, uint32_t split_candidates, int32_t split_method,
                               uint32_t min_leaf_support, uint32_t max_depth, void *out, size_t out_bytes);
/* Quantised gradients, test hooks ("Quantised gradients").  fr_debug_hist_quantise: the fixed-point step
 * and the quantisation to `bits` bits (2..8) under the key of tree `tree` of `seed`, for lambda / weight[len] by instance id
 * over the instances of queries[n_queries] (NULL = all) and, when goss != 0, over the GOSS list of those (rates, seed and tree
 * as in FrHistTreeOptions) with amplified values.  q_out / w_out[cap] (cap >= the view's instances): the values by index of the
 * tree's list; *n_out: its length; numbers_out[6] = S, S_w, the search's two exponents S - d and S_w - d_w, d, d_w.
 * fr_debug_hist_root_histogram: the root's histogram over every instance for the features features[n_features] (NULL = all):
 * count_out / sum_out / wsum_out[cells], cells = features x split_candidates, laid out [feature][bin]; bits == 0: the Newton
 * build over the fixed-point values, else the packed build over the quantised ones. */
const void *fr_debug_hist_quantise(const CDataset *dataset, const double *lambda, const double *weight, size_t len,
                                   uint32_t bits, uint64_t seed, uint32_t tree, const uint32_t *queries, size_t n_queries,
                                   int32_t goss, double top_rate, double other_rate, uint64_t goss_seed, uint32_t goss_tree,
                                   int32_t *q_out, uint32_t *w_out, size_t cap, uint32_t *n_out, int32_t *numbers_out);
const void *fr_debug_hist_root_histogram(const CDataset *dataset, const double *lambda, const double *weight, size_t len,
                                         uint32_t split_candidates, uint32_t bits, uint64_t seed, uint32_t tree,
                                         const uint32_t *features, size_t n_features, uint32_t *count_out, int64_t *sum_out,
                                         int64_t *wsum_out, size_t cells);
/* fr_debug_lambda_gradients under the LambdaRank objective's options ("Truncation and
 * normalisation").  options_json = {"truncation_level": T, "lambda_norm": bool}, either key optional: T >= 1 keeps a pair
 * only when the better ranked of its two documents is in the top T of the pass's ranks (0, the default: every pair);
 * lambda_norm scales every query's lambda and weight by log2(1 + S_q) / S_q, S_q the query's summed pair terms.
 * queries[n_queries] as in fr_debug_lambda_gradients_sampled, or NULL for every query.
 * A third optional key, "objective": "ndcg" (the default), "map" or "mrr" ("ap" / "rr" are accepted) -- the LambdaMART
 * variant's `objective` key ("Objectives"): a pair is then one relevant (gain > 0) and one
 * non-relevant document, weighted by the change of AP / RR their swap would make, and the norms are the AP / RR
 * evaluator's.  `measure` must still name NDCG (ndcg, ndcg@k) whatever the objective, as in a training request, where
 * "measure": "map" is refused with or without the key.
 * "objective": "xendcg" (lower case only) is the listwise cross-entropy pass ("Listwise
 * objective"; lambda_grad_xe_kernel) under the tree key "xe_key" (a fourth optional key: u64, default 0, read under
 * "xendcg" only).  The norms stay the NDCG evaluator's; sigma and the measure's depth are not read; a truncation_level
 * other than 0 or lambda_norm: true with it is an `invalid value` error, raised before any device work. */
const void *fr_debug_lambda_gradients_opts(const CModel *model, const CDataset *dataset, const CQRel *qrel,
                                           const void *measure, double sigma, const uint32_t *queries,
                                           size_t n_queries, const void *options_json, double *lambda_out,
                                           double *weight_out, size_t out_len);
/* LambdaMART's DART boosting, test hooks ("DART"; the variant's optional keys drop_rate, max_drop,
 * skip_drop).  fr_debug_lambdamart_dart_plan: JSON [{"dropped": [tree indices ascending], "before": [w_0 .. w_{t-1}],
 * "after": [w_0 .. w_t]}, ...] for the first num_trees trees of the LambdaMART parameters params_json (their own
 * num_trees is not read); no device is touched.  fr_debug_dart_scores: `model` is an Ensemble of DecisionTrees (its
 * weights are not read), weights[n_weights] one weight per tree, include[n_include] ascending tree indices; the leaf
 * cache is filled for the trees as the trainer fills it and dart_rescore_kernel runs once: scores_out[i] = the
 * sequential unfused sum over the included trees of weights[t] * tree_t(x_i), cache_out[t * out_len + i] = the leaf
 * (depth-first numbering) instance i reaches in tree t (instances outside the view are left untouched). */
const void *fr_debug_lambdamart_dart_plan(const void *params_json, uint32_t num_trees);
const void *fr_debug_dart_scores(const CDataset *dataset, const CModel *model, const double *weights, size_t n_weights,
                                 const uint32_t *include, size_t n_include, double *scores_out, uint16_t *cache_out,
                                 size_t out_len);
/* Full per-query rank order under the reference's total order (src/evaluators.rs:34-49):
 * out_instance_ids[n] grouped by query (device query order), best first; out_offsets[nq+1]. */
const void *fr_rank_order(const CModel *model, const CDataset *dataset, uint32_t *out_instance_ids,
                          size_t n, uint64_t *out_offsets, size_t nq_plus_1);
/* JSON about the dataset's device form (built on first use): {"hbm_bytes_owned","shares_parent_matrix",
 * "is_parent_device_dataset","queries","instances"}.  A view made by dataset_query_sampling /
 * dataset_feature_sampling does not tile a second copy of X: a feature sample uses its parent's device dataset as it is,
 * a query sample owns only query / run tables over the parent's tiles (src/dataset.rs:101-178 keeps views as id lists
 * over the parent for the same reason). */
const void *fr_dataset_device_info(const CDataset *dataset);
/* Number of queries / instances in the dataset view (0 for a NULL handle).  fr_dataset_num_queries returns SIZE_MAX
 * when the view cannot be grouped (e.g. a NaN label): the compute calls report the reason in their envelope. */
size_t fr_dataset_num_queries(const CDataset *dataset);
size_t fr_dataset_num_instances(const CDataset *dataset);

/* The hot operator itself: batched evaluate_mean of line-search candidates
 * (src/coordinate_ascent.rs:157-160 x src/evaluators.rs:173-184).
 *   n_groups line groups; group g shares base weights base_weights[g*d .. g*d+d) and feature
 *   features[g]; it has n_cand[g] (<=64) candidate values candidates[g*64 + c] for that
 *   feature's weight.  out_means[g*64 + c] receives the mean metric.  If out_per_query is
 *   non-NULL it receives the [nq][n_groups*64] per-query matrix.
 * Uses the fused HIP line-search kernel for ndcg@k (k<=20) and the general sort kernel
 * otherwise.  Returns NULL on success or an error-envelope string. */
const void *fr_evaluate_candidates(const CDataset *dataset, const CQRel *qrel, const void *evaluator_name,
                                   size_t n_groups, const uint32_t *features, const double *base_weights,
                                   const uint32_t *n_cand, const double *candidates, double *out_means,
                                   double *out_per_query);

/* HIP-event timing of the library's kernels on the stream they are launched on. */
void fr_profile_enable(int on);
void fr_profile_reset(void);
/* JSON list [{"kernel","launches","total_ms"}] (free_str). */
const void *fr_profile_json(void);
/* hipDeviceSynchronize; 0 on success. */
int fr_synchronize(void);
/* The constants of the resident-sum error bound the trainer and the bound-and-verify kernels use (DESIGN.md
 * section 4.2), so that a CPU test can replay the device's update arithmetic against extended precision with the
 * product's own numbers.  which = 0: bound after an exact refresh (a = feature count, b = T);
 * 1: bound after one incremental update (a = previous bound, b = norm, c = T);
 * 2: the term a candidate key's error bound gains from the resident form (a = bound, b = norm, c = T).
 * No device needed.  NaN for an unknown `which`. */
double fr_debug_resident_bound(int which, double a, double b, double c);
/* The arithmetic of a query's end in the NDCG@k bound-and-verify kernel (csrc/verify_end.hpp), over n entries, so that a
 * CPU test can hold the code the kernel compiles to the expressions it stands for.  which = 0: out[i] = the division-free
 * quotient a[i] / b[i] (a = dcg, b = norm) with the reciprocal the host uploads for b[i]; where that is "divide" (norm out of
 * range, zero, NaN), the division itself.  c and d are not read.  which = 1: out[i] = the per-query gap bound from the first
 * and last counted key a[i], b[i], the relative part c[i] and the absolute part d[i] of a pair's error bound.
 * which = 2: out[i] = fma(a[i], b[i], c[i]), the primitive a numpy restatement of either needs.  which = 3: every dcg a[i],
 * i < n, against every norm b[j], j < c[0]: out[0] = the number of pairs whose quotient differs bitwise from a[i] / b[j],
 * out[1], out[2] = one such pair (on a few host threads; out holds three entries).
 * No device needed.  Returns 0, or -1 for an unknown `which`. */
int fr_debug_verify_end(int which, size_t n, const double* a, const double* b, const double* c, const double* d, double* out);
/* Size class of the full-ranking bound-and-verify kernel (depth-less NDCG, MAP, NDCG@>20) for a query of `len` documents:
 * (keys per lane << 16) | lanes per candidate.  No device needed (the CPU tests check that every length has a class that
 * holds it and that classes grow with the length). */
uint32_t fr_debug_fullrank_class(uint32_t len);
/* The device plan of a request with `num_restarts` units of work (coordinate-ascent restarts, random-forest trees) over the
 * devices listed in `devices_csv` (the syntax of the FR_DEVICES environment variable: comma-separated ordinals, the same
 * ordinal twice = two contexts on that device) on a node with `device_count` devices, when the dataset's first device
 * form lives on `primary_device`: JSON {"devices": [...], "slots": [...], "blocks": [[begin, end], ...]} -- which
 * device-side copy every entry trains on and the contiguous block of ids it gets under a static partition (random
 * forests, and coordinate ascent with FR_RESTART_QUEUE=0; by default the entries of a coordinate-ascent request pull
 * restart ids from one shared queue instead -- the reference fans restarts out with rayon,
 * src/coordinate_ascent.rs:215-225).  No device needed; errors come back in the usual envelope. */
const void *fr_debug_device_plan(const void *devices_csv, int device_count, uint32_t num_restarts, int primary_device);
/* Replays the restart queue of train_model on the CPU (no device): `n_workers` trainers with `capacity` live restarts
 * each take the ids 0 .. num_restarts-1 from one queue; restart r is given a length of lengths[r % n_lengths] ticks and a
 * worker refills converged places at the end of a tick.  JSON {"order": [[ids in the order worker w started them] ...],
 * "ticks": [...]} -- the CPU tests check that every id is started exactly once and that a worker never holds more than
 * `capacity`. */
const void *fr_debug_restart_queue(uint32_t num_restarts, uint32_t n_workers, uint32_t capacity, const uint32_t *lengths,
                                   uint32_t n_lengths);
/* One timed device-to-device copy of `bytes` bytes from device `src_device` to device `dst_device`, made the way
 * train_model's fan-out copies a dataset to another GPU (peer access enabled where the link allows, hipMemcpyPeerAsync):
 * JSON {"src","dst","bytes","can_access","enabled","ms","gbps"}.  A first-contact check of the peer path on a multi-GPU
 * node (bench.py --gpus N reports it per device pair); src == dst measures a copy inside one device. */
const void *fr_debug_peer_copy(int src_device, int dst_device, size_t bytes);
/* The exchange records of a job's single all-gather (what src/coordinate_ascent.rs:232-252 selects from): a
 * rank's restarts as a fixed-size block of `cap` records of 3 + dim doubles -- valid (1.0; 0.0 = padding), restart id, score,
 * weights[dim].  fr_pack_restart_records writes the block for a JSON list of {"restart_id","score","weights"} (returns NULL
 * or an error envelope); fr_unpack_restart_records returns the valid records of n_records records as such a list, in
 * restart order.  Same layout as native.gather_restarts (torch.distributed) and train_model's own fan-out. */
const void *fr_pack_restart_records(const void *restarts_json, size_t cap, size_t dim, double *out);
const void *fr_unpack_restart_records(const double *records, size_t n_records, size_t dim);
/* ONE single-process RCCL all-gather over `devices` (ncclCommInitAll over the list, a grouped ncclAllGather; librccl.so is
 * dlopen-ed, no link-time dependency): rank i contributes blocks[i * block_len ..], `out` (optional, n * block_len doubles)
 * receives what rank 0 gathered.  JSON {"ran":true,"ranks","devices","us","first_us","init_us","matches_host_gather"}, or
 * {"ran":false,"reason"} when it does not apply (one rank; ranks that share a GPU).  With n distinct GPUs a failure is an
 * error envelope, not a fallback.  train_model's multi-device path runs it on the restarts' records itself
 * (fr_last_train_stats: "rccl"). */
const void *fr_rccl_allgather(const int *devices, size_t n, const double *blocks, size_t block_len, double *out);
/* The walk tiles of the resident NDCG@k verify kernel (csrc/device.hpp: build_walk_tiles) for a layout of runs and queries,
 * computed on the host alone: JSON {"walk_tile":128,"wt_start":[...],"run_wt0":[...],"seg":[...],"wofs":[...]}. */
const void *fr_debug_walk_tiles(const uint32_t *run_pos, const uint32_t *run_q0, const uint32_t *run_q1, size_t nruns,
                                const uint32_t *qstart, const uint32_t *qlen, size_t nq, size_t np);
/* Read-back of the device form of a dataset, for the tests that hold every table to its definition.
 * Read only: it takes the dataset's lock, waits for the dataset's stream and copies; no product path calls it.
 * slot 0 = the dataset's first device form (built if needed); slot k > 0 = the copy train_model keeps for entry k of its
 * device list (an error when there is none).  table == NULL: JSON of sizes, switches and buffer addresses by name ("np",
 * "dq", "d", "n", "nq", "nonfinite", "nruns", "nwt", "ncls", "key_bits", "key_cls_bits", "dup_groups", "no_document", ...).
 * Otherwise the named static table ("xb", "xcol", "xslot", "perm", "qstart", "qlen", "run_*", "wt_start", "segtab", "gain",
 * "gexp", "gcls", "gkey", "dcgtab", "colmax", "colstd", "colmode", "colstats", ...) is copied to `out` as raw bytes:
 * JSON {"present": bool, "bytes": n}; present = false when the dataset has no such table (xcol, xslot and the column
 * statistics are optional), an error when out_bytes is not n or the name is unknown. */
const void *fr_debug_device_form(const CDataset *dataset, int slot, const void *table, void *out, size_t out_bytes);
/* The host-side layout of a dataset (csrc/dataset_layout.hpp: runs, size classes, gain tables, duplicate groups, walk tiles)
 * built from its host CSR alone -- no device is touched, nothing is kept.  The protocol and the table names of
 * fr_debug_device_form: table == NULL gives the JSON of sizes ("np", "nq", "nruns", "nwt", "ncls", "tablen", "key_bits",
 * "key_cls_bits", "dup_groups", "verify_xs", "relmask", ...), otherwise the named table is copied to `out` (JSON {"bytes": n};
 * a wrong out_bytes or an unknown name is an error).  Beyond fr_debug_device_form's names: "termtab", "qnpos", "qnneg",
 * "qlist", "fv_qlist", "size_classes" / "fv_classes" (u32 triples class, offset, count).  parent_queries[n_parent_queries]
 * (optional): also the tables of the view that holds these queries of the dataset, as "view_qstart", "view_run_lo",
 * "view_vtiles", "view_wlist", ... ; `view` (optional) = the dataset whose CSR is the view's own (NULL: cut from `dataset`'s).
 * row_hash[n_row_hash = np] (optional): the 64-bit row hash of every position, as the device computes them (NULL: a host
 * hash of the row bytes). */
const void *fr_debug_dataset_layout(const CDataset *dataset, const uint32_t *parent_queries, size_t n_parent_queries,
                                    const CDataset *view, const uint64_t *row_hash, size_t n_row_hash, const void *table,
                                    void *out, size_t out_bytes);
/* The same call sequence with a one-rank communicator on `device` (what a one-GPU box can run of it): same JSON. */
const void *fr_debug_rccl_selftest(int device);
/* Frees the device-to-device copies train_model made of this dataset on other devices / in other contexts (they are kept
 * with the dataset so that the next request reuses them; a node shared with other jobs may want the HBM back).  The
 * dataset's first device form stays.  Returns the number of copies released.  Views sampled from the dataset
 * (dataset_query_sampling, train_test_split ...) that were trained on several devices hold copies of their own -- over
 * the same copied matrix -- and are released the same way, each through its own handle. */
size_t fr_dataset_release_replicas(const CDataset *dataset);

/* ---- Text loading ("Text loading") ----
 * load_ranksvm_format with a choice of parser: "host" = the line-by-line host parser; "device" = the HIP parser (line scan,
 * two parsing passes, host merge), which hands every line outside its fast grammar back to the host parser and gives the
 * same dataset and the same errors -- without a HIP device it returns the `no MI355X/HIP device available...` envelope;
 * "auto" (what load_ranksvm_format passes) = the device parser when a device is present and the inflated text is at least
 * 32 MiB, the host parser otherwise.  Any other word is an error that names the three. */
const CResult *fr_load_ranksvm(const void *data_path, const void *feature_names_path_or_null, const void *parser);
/* What the last successful load of this process did, as JSON: "parser" that ran ("host" | "device") and "reason", "bytes",
 * "lines", "host_lines" (lines handed back to the host parser), "host_line_reasons" {"too_long", "grammar", "number",
 * "unsorted", "range", "near_tie": counts}, "seconds" {"read", "upload", "line_scan", "pass1", "pass2", "download",
 * "host_merge", "total"} (wall), and the constants "scan_slice", "stage_limit", "auto_threshold" (bytes). */
const void *fr_last_load_stats(void);
/* The host arrays of a file-loaded dataset (or of one fr_normalize_dataset made), for the tests.  field == NULL: JSON {"n",
 * "d", "present_words", "has_docids", "present_bits_len", "features_len", "doc_present_len", "qnames_hex", "docids_hex" (the
 * strings' bytes in hex)}; otherwise "x" (f32 n * d),
 * "gain" (f32), "qix" (u32), "doc_present" (u8), "features" (u32) or "present_bits" (u32) is copied to `out`
 * (JSON {"bytes": n}; a wrong out_bytes or an unknown name is an error). */
const void *fr_debug_dataset_core(const CDataset *dataset, const void *field, void *out, size_t out_bytes);
/* The device parser's number rule (csrc/text_number.hpp), compiled for the host, on the n tokens of `tokens` (one per line):
 * reasons[i] = 0 and value64[i] / value32[i] = the value, or the code of the reason the token is declined with.  The JSON
 * reply lists the reasons' names by code. */
const void *fr_debug_text_number(const void *tokens, size_t n, uint32_t *reasons, double *value64, float *value32);

/* ---- Feature normalisation (the reference's Normalizer, src/normalizers.rs) ----
 * fr_fit_normalizer: the normaliser of `method` ("zscore" | "maxmin" | "linear" | "sigmoid"; anything else is
 * `Unsupported Normalizer: <method>`) fitted on the instances and features of `dataset` (a dataset or any view of one), as
 * JSON in the reference's serde shape: {"ZScoreNormalizer": {"feature_stats": {"<fid>": {"num_elements", "mean", "variance",
 * "max", "min", "total"}}}}, {"MaxMinNormalizer": {...}}, {"SigmoidNormalizer": []}; or an error envelope.  The statistics
 * are taken on the device over the values the instances hold; a held NaN or infinity is refused (`non-finite value in
 * feature F, instance I: feature statistics need finite values`).
 * fr_normalize_dataset: a new unsampled dataset that owns its matrix -- `dataset`'s instances, gains, queries, document
 * ids, feature names and presence bits, every held value transformed on the device by the normaliser `normalizer_json` (one
 * of the three shapes above, or {"PerQuery": "zscore" | "maxmin"}: statistics per query and feature, nothing fitted).
 * Refused: a sampled view (`normalise the whole dataset, then sample it`), a dataset that is itself the result of this call
 * (`Cannot apply normalization twice!`), a result that is NaN (`Normalization.<method> NaN: feature F, instance I`).
 * dataset_query_json learns "normalization" (the remembered normaliser's JSON, null for any other dataset) and
 * "normalization_stats" (where the call that made the dataset spent its time: {"prepare_seconds", "allocate_seconds",
 * "kernel_seconds", "download_seconds", "device_other_seconds", "core_build_seconds", "total_seconds"}, or null).  Without a HIP device both return the `no MI355X/HIP device available...` envelope. */
const void *fr_fit_normalizer(const CDataset *dataset, const void *method);
const CResult *fr_normalize_dataset(const CDataset *dataset, const void *normalizer_json);

/* ---- Model comparison: bootstrap intervals and permutation tests (the reference's
 * SetEvaluator::bootstrap_eval and PercentileStats, src/evaluators.rs:157-171, src/stats.rs:126-165) ----
 * fr_resample: `values` is a row-major f64 table of nq rows (queries) and ncols columns (systems, 1..8), every value finite
 * (`non-finite value in row R, column C: ...` otherwise).  options_json: {"trials": 1..2^20 (10000), "seed": u64 (0),
 * "alpha": 0 < a < 1 (0.05)}, each optional, any other key refused by name.  On the current device: the paired bootstrap into
 * out_boot and the per-query permutation (randomised Tukey HSD; two systems: the paired randomisation test) into out_perm,
 * trials x ncols f64 each in trial order; either may be NULL, which skips its kernel and its parts of the report.  Streams and
 * the sums' shape: csrc/resample.hpp.  Returns JSON: {"means": [..], "intervals": [[lo, hi], ..], "summary": [{"p5", "p25",
 * "p50", "p75", "p95"}, ..] (the reference's percentile, interpolation as written), "pairs": [{"i", "j", "diff",
 * "diff_interval": [lo, hi], "p", "wins", "losses", "ties"}, ..] for i < j, "trials", "seed", "alpha", "boot_path": "lds" |
 * "global", "boot_ms", "perm_ms", "upload_ms", "download_ms", "device_call_ms", "report_ms"}, or an error envelope (without a
 * HIP device: `no MI355X/HIP device available...`).
 * fr_compare_models: evaluates each of the n_models models (1..8) on `dataset` (a dataset or any view: the same queries in the
 * same order for all) through fr_evaluate_dense's path, makes the table of per-query values, and returns fr_resample's report
 * of it plus "queries" (their number).  With one model the permutation is skipped. */
const void *fr_resample(const double *values, size_t nq, size_t ncols, const void *options_json, double *out_boot, double *out_perm);
const void *fr_compare_models(const CModel *const *models, size_t n_models, const CDataset *dataset, const CQRel *qrel_or_null,
                              const void *evaluator_name, const void *options_json);

/* ---- Permutation importance: any model, any measure (the definition: csrc/permute.hpp) ----
 * fr_permutation_importance: how far the mean of `evaluator_name` over the queries of `dataset` (a dataset or any view) falls
 * when one feature column is read from other rows.  options_json, each key optional, any other refused by name: {"repeats":
 * 1..64 (5), "seed": u64 (0), "scope": "dataset" | "query" ("dataset": rows move across the whole view; "query": inside their
 * query), "features": [ids of the view's features, none twice] (all of them, ascending), "skip_unused": bool (true: a feature
 * the model cannot read -- no tree splits on it, a SingleFeature's other features, a Linear weight that is exactly 0 on a
 * finite column -- is never launched for; its values are the baseline, its importance and std 0.0), "max_slots": >= 1 (from
 * free memory; score slots per launch, never under one feature's repeats)}.  One permutation per (seed, repeat) is shared by
 * all features.  Models: Linear, SingleFeature, DecisionTree, an Ensemble of DecisionTrees, an Ensemble of Linear /
 * SingleFeature members; any other shape is refused by name.  Refused before the device is touched: bad options, a feature
 * the view does not hold or lists twice, an empty view, the model's shape; out_len < F * R.
 * out_values[f * R + r] (F = the features in the order asked for): the mean on the dataset with feature f permuted in repeat
 * r.  out_per_query_or_null: (F * R + 1) rows of nq values in the device's query order (fr_evaluate_dense's), row f * R + r
 * the per-query values behind out_values[f * R + r], the last row the baseline's.
 * Returns JSON: {"features": [ids], "names": [..], "baseline", "importance": [..], "std": [..], "skipped": [ids],
 * "repeats", "seed", "scope", "evaluator", "queries", "stats": {"gather": "xcol" | "tiles", "rows": "lds" | "global", "chunks", "slots", "score_ms",
 * "metric_ms", "upload_ms", "baseline_ms", "sources_ms", "launches": {"linear", "single", "trees", "axpy"}}}, or an error
 * envelope (a bad evaluator name: fr_evaluate_dense's texts; a NaN score: `Model.predict -> NaN`).
 * fr_debug_permutation_sources: host only, works with no device.  out_src_by_instance[id] = the instance whose value instance
 * id reads in repeat `repeat` under `scope`, 0xFFFFFFFF for ids the view does not hold; out_len > the view's largest id.
 * Returns {"n": the view's instances}. */
const void *fr_permutation_importance(const CModel *model, const CDataset *dataset, const CQRel *qrel_or_null, const void *evaluator_name,
                                      const void *options_json, double *out_values, size_t out_len, double *out_per_query_or_null);
const void *fr_debug_permutation_sources(const CDataset *dataset, uint64_t seed, uint32_t repeat, const void *scope,
                                         uint32_t *out_src_by_instance, size_t out_len);

#ifdef __cplusplus
}
#endif
#endif /* FASTRANK_AMD_H */
