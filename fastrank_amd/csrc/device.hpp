// Device-side interface of the MI355X hot path (no HIP types leak through this header).
//
// A DeviceDataset is the HBM-resident form of one reference `RankingDataset` view
// (src/dense_dataset.rs:11-20, src/dataset.rs:101-106):
//   * documents regrouped by query (CSR), and inside each query stored in REVERSE tie-break
//     order (gain desc, instance-id desc) so that "later document wins score ties" reproduces
//     the reference's (score desc, gain asc, id asc) total order (src/evaluators.rs:34-49);
//   * consecutive queries are packed into "runs" of whole 64-document tiles; features live in
//     tiles [tile][D/4][64 docs][4 features] f32, so lane = document reads 16 B per load;
//   * per-document gain (f32), 2^gain-1 (f64, host libm like the reference), relevance flag;
//   * per-query offsets, a longest-first query schedule, log2(i+2) discount table.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "dataset_layout.hpp"  // HostCSR, the walk tiles and the rest of the host-side layout arithmetic
#include "permute.hpp"         // PermuteMember, PermuteStats (permutation importance)

namespace frdev {

// Environment switches, three kinds (INTEGRATION.md lists the first):
//   * runtime configuration of the shipped library is read with std::getenv where it is used: FR_DEVICES, FR_RESTART_QUEUE,
//     FR_RESTART_SLOTS, FR_MIN_RESTARTS_PER_DEVICE, FR_XCOL, FR_VERIFY_ORDER, FR_LS_EXACT, FR_VERIFY_AUDIT, FR_LS_PIPELINE,
//     FR_UPLOAD_TIMING, FR_HOST_TIMING;
//   * path_env: selectors of ANOTHER BIT-EXACT path (the exact kernels instead of bound-and-verify, the generic sort
//     evaluator instead of the fused one, tiles instead of resident sums, ...).  The parity tests use them to reach every
//     path with the same inputs; whatever they are set to, results are the reference's;
//   * pricing_env: timing experiments and tuning sweeps, some of which return WRONG numbers on purpose (a kernel phase
//     skipped to price the rest).  They exist only in a library built with -DFR_PRICING (FR_BUILD_FLAGS=-DFR_PRICING):
//     the shipped library cannot be talked into wrong scores through its environment.
const char* path_env(const char* name);
inline const char* pricing_env(const char* name) {
#ifdef FR_PRICING
    return path_env(name);
#else
    (void)name;
    return nullptr;
#endif
}

// (0..2 are LambdaMART's objectives too, kernels_lambda.inc; the five after them are defined in measures_host.hpp)
enum Measure : int { M_NDCG = 0, M_AP = 1, M_RR = 2, M_DCG = 3, M_PRECISION = 4, M_RECALL = 5, M_SUCCESS = 6, M_ERR = 7 };
// LambdaMART's objectives are spelled as their measures; the listwise objective "xendcg" has no measure of its own
constexpr int LM_OBJECTIVE_XENDCG = 3;

// Error bound E >= |R - sum_j x_j v_j| of a trainer's resident sums, u = 2^-53, T from column
// maxima.  One place for the constants: the trainer (host.hpp), compute_eps2 (device_dataset.inc) and the CPU test
// that replays the device's update arithmetic against extended precision (tests/test_error_bound.py, through
// fr_debug_resident_bound) all use these.
//   after an exact refresh (score_linear: ordered unfused f64 sums of D products): gamma_D * T
inline double resident_err_refresh(uint32_t d, double T) { return 1.1 * (double)(d + 1) * 0x1p-53 * T; }
//   after R' = fma(x_f, cand, fma(-x_f, base_f, R * fl(1/norm))) with base = fl(v / norm), v' = base with [f] = cand:
//   the old error shrinks by 1/norm; the separately rounded divisions of l1_normalize (u T), the reciprocal and the
//   product R * inv (2 u T), and the two FMA roundings (u (|x_f base_f| + T) + u T) add at most 8 u T with
//   T = |base_f| X_f + sum_j |v'_j| X_j
inline double resident_err_update(double err, double norm, double T) { return 1.002 * err / norm + 8.0 * 0x1p-53 * T * (1.0 + 1e-6); }
//   what A = fma(-x_f, base_f, R * fl(1/norm)) adds to a candidate's key error (T = sum_j |base_j| X_j incl. j = f)
inline double resident_eps_extra(double err, double norm, double T) { return 1.01 * err / norm + 10.0 * 0x1p-53 * T; }

// error bits raised by kernels (the reference panics in these cases)
enum : int {
    FLAG_NAN_SCORE = 1,        // src/model.rs:49  "Model.predict -> NaN"
    FLAG_ACTUAL_GT_IDEAL = 2,  // src/evaluators.rs:368-374
};

struct FlatTrees {
    // node k: fid<0 => leaf with value `split`; else go lhs if f64(x[fid]) <= split else rhs
    std::vector<int32_t> fid, lhs, rhs;
    std::vector<double> split;
    std::vector<int32_t> root;    // per tree
    std::vector<double> weight;   // per tree (ignored when raw_single)
    bool raw_single = false;      // a bare DecisionTree model: output = leaf value
};
struct TreeShape;  // forest_pack.hpp: a block shape of the f32 LDS walk

// What the process's last DeviceDataset::score_trees call ran (fr_debug_tree_plan): which of the three
// encodings took the forest and in what shape.  Host bookkeeping alone: no timing, no launch of its own.
struct TreePlan {
    enum Path { NONE, RANK, LDS, L2 };
    Path path = NONE;
    bool cache_hit = false;             // RANK: launched from the buffers the call before left
    bool rows_in_lds = false;           // L2: tree_ensemble_kernel<true, 8> (rows staged in LDS) or <false, 8>
    uint32_t docs = 0, parts = 0;       // LDS: the block shape that took the forest
    uint32_t nslots = 0, nrounds = 0;   // RANK: features in use, ranking rounds
    std::vector<std::pair<uint32_t, uint32_t>> batches;  // RANK, LDS: (walks per thread, levels) of every batch
};
TreePlan last_tree_plan();

// What the process's last DeviceDataset::metric_from_scores call launched (fr_debug_metric_plan): the
// kernel that took each size class.  Host bookkeeping alone.
struct MetricPlan {
    struct Class {
        uint32_t npad = 0, queries = 0;
        bool topk = false;  // metric_topk_kernel; else metric_sort_kernel
    };
    int measure = -1;  // -1: no call yet
    int64_t depth = -1;
    size_t slots = 0;
    std::vector<Class> classes;
};
MetricPlan last_metric_plan();

// One line-search group: every candidate shares (feature f, base weights w) and differs only in
// the weight of f (src/coordinate_ascent.rs:131-171).
struct LineGroup {
    uint32_t feature = 0;
    std::vector<double> weights;     // [d] base weights (entry `feature` ignored)
    std::vector<double> candidates;  // <= 64 values for w[feature], in evaluation order
    // Optional (bound-and-verify path only): a resident per-document sum R ~ sum_j x_j * v_j for some
    // vector v (the trainer's un-normalised best weights) lives in slot `resident_slot`; the base dot
    // product is then formed as  A = R / resident_norm - x_f * resident_base_f  instead of from the
    // feature tiles (weights == v / resident_norm up to rounding).  `resident_err` bounds |R - sum_j x_j v_j|
    // for every document.  A pending update (the previous tick accepted a candidate, so v changed in one
    // coordinate after being normalised) is applied first:
    //   R <- fma(x_uf, upd_cand, fma(-x_uf, upd_base_f, R / upd_norm))
    int resident_slot = -1;
    uint64_t resident_owner = 0;  // ticket from resident_reserve(); a stale ticket means "form A from the tiles"
    double resident_norm = 1.0, resident_base_f = 0.0, resident_err = 0.0;
    bool has_update = false;
    uint32_t upd_feature = 0;
    double upd_norm = 1.0, upd_base_f = 0.0, upd_cand = 0.0;
};

// One event of the tick capture (a test hook, DeviceDataset::capture_enable): a store of exact resident sums,
// or one collected line search with what it published.
struct LsCapture {
    bool store = false;
    // store: slot <- the exact ordered sums of the un-normalised weight vector v
    int slot = -1;
    std::vector<double> v;
    // tick
    int ctx = 0, kind = 0, measure = 0;  // kind: 0 = top-k, 1 = reciprocal rank, 2 = full ranking
    int64_t depth = 0;
    std::vector<LineGroup> groups;  // the caller's order
    std::vector<uint32_t> gorder;   // staged group k = the caller's gorder[k]
    size_t nverify = 0;             // the verify kernel took the first nverify staged groups
    bool approx = false, resident = false, ready = false;
    int kbucket = 0, xs_used = 0;   // top-k: linesearch_verify_kernel<kbucket, ., ., xs_used, dup>
    bool xs_pinned = false, dup = false;
    std::vector<uint32_t> classes;  // full ranking / reciprocal rank: (keys per lane, lanes per candidate, queries) of every size class launched
    std::vector<uint32_t> redo;     // the redo list's entries: (query * redo_groups + staged group) [* 16 + slice mask, top-k]
    uint32_t redo_groups = 0;
    std::vector<double> means;      // as published (the caller's order)
    bool has_matrix = false;
    size_t nq = 0, ldm = 0, np = 0;
    std::vector<double> matrix;     // [nq][ldm], staged order, after every redo pass and any audit
    std::vector<int> res_slots;     // resident slots of the groups, ascending ...
    std::vector<double> res;        // ... and each one's current half ([np] per slot) after the launch's flip
};

struct KernelStat {
    std::string name;
    uint64_t launches = 0;
    double total_ms = 0.0;
};

class DeviceDataset {
  public:
    static std::shared_ptr<DeviceDataset> create(const HostCSR& csr, std::string* err);
    // A view of `parent` restricted to some of its queries (src/sampling.rs:117-133 with_queries): shares the parent's
    // feature tiles and per-document arrays in HBM (no second copy of X) and only builds its own query / run tables.
    // csr = the view's own CSR (same documents per query, same order inside a query as the parent);
    // parent_query[q] = index of the view's query q in the parent.
    static std::shared_ptr<DeviceDataset> create_view(const std::shared_ptr<DeviceDataset>& parent, const HostCSR& csr,
                                                      const std::vector<uint32_t>& parent_query, std::string* err);
    // A copy of `src` (which must own its matrix) in the HBM of device `device`, made device to device (hipMemcpyPeer);
    // the same ordinal as the source gives a second, independent context on that device.
    static std::shared_ptr<DeviceDataset> replicate(const std::shared_ptr<DeviceDataset>& src, int device, std::string* err);
    int device_ordinal() const;
    bool shares_parent_matrix() const;
    ~DeviceDataset();

    size_t n() const;
    size_t d() const;
    size_t nq() const;
    size_t max_query_len() const;
    size_t hbm_bytes() const;

    // --- scoring into the internal score buffer (slot b of B, CSR order) ---------------------
    // weights: B vectors of length d (row-major), exact reference dot product.
    bool score_linear(size_t B, const double* weights, std::string* err);
    bool score_single_feature(uint32_t fid, double dir, std::string* err);
    bool score_trees(const FlatTrees& trees, std::string* err);
    // out += w * tmp (unfused), used for mixed ensembles (src/model.rs:104-112)
    bool ensemble_begin(std::string* err);                 // acc = 0
    bool ensemble_accumulate(double w, std::string* err);  // acc = acc + w * slot0
    bool ensemble_finish(std::string* err);                // slot0 = acc

    // copy slot b back, scattered to original instance ids: out[perm[p]] = score[p]
    bool download_scores(size_t b, double* out_by_instance, size_t out_len, std::string* err);

    // --- metrics -------------------------------------------------------------------------------
    // per-query metric of the B score slots -> M[q][b]; norms[nq]: NDCG ideal (NaN=None) /
    // AP num_relevant (0=absent).  depth<0 = None.
    bool metric_from_scores(int measure, int64_t depth, const double* norms, size_t B,
                            bool want_rank, std::string* err);
    bool download_per_query(size_t B, double* out /*[nq*B], q-major*/, std::string* err);
    bool download_rank(uint32_t* out_instance_ids /*[n] grouped by query, rank order*/, std::string* err);
    // mean over queries of each of the last result's columns (sequential sum in query order)
    bool reduce_means(size_t ncols, double* out_means, std::string* err);
    // query-sharded training: every reduction over queries (reduce_means, the line searches) returns the
    // SUM over this dataset's queries, in the fixed two-level shape, instead of the mean
    void set_sums_only(bool on);
    // Means of column 0 of the last result over two subsets of the queries (LambdaMART's training and held-out queries):
    // subset_means_set uploads the two index lists (queries of this dataset, each ascending, both non-empty) once;
    // reduce_subset_means then gives {mean over a, mean over b}, each in the fixed two-level shape over the subset's
    // compacted list, with one copy back.  subset_means_end forgets the lists.
    bool subset_means_set(const std::vector<uint32_t>& a, const std::vector<uint32_t>& b, std::string* err);
    bool reduce_subset_means(double out_means[2], std::string* err);
    void subset_means_end();

    // --- line search: every candidate of every group, means[g*64 + c] --------------------------------------
    // Bound-and-verify: candidates are decided from approximate scores with a proven error bound, what is left
    // is recomputed by the exact kernels.  LS_TOPK: NDCG@k, k <= 20 (kernels_verify.inc).  LS_FULLRANK: NDCG of any depth
    // and AP (kernels_fullverify.inc), reciprocal rank (kernels_rr.inc).  LS_NONE: the general sort evaluator's (non-finite
    // features, too many gain classes or documents per query; FR_FORCE_GENERIC for the full-ranking measures).
    enum LsPath : int { LS_NONE = 0, LS_TOPK = 1, LS_FULLRANK = 2 };
    LsPath linesearch_path(int measure, int64_t depth) const;
    // Contexts 0 .. LINESEARCH_CONTEXTS-1 have their own streams and buffers: callers keep several sets of groups in flight
    // and the host's work between two line searches of one set overlaps the kernels of the others.  submit always leaves the
    // context pending (where bound-and-verify does not apply it runs the exact kernels at once); collect waits for it.
    // counts: the (query, group) pairs this line search gave to the verify kernels, and how many of them were redone.
    static constexpr int LINESEARCH_CONTEXTS = 4;
    struct LsCounts {
        unsigned long long pairs = 0, redone = 0;
    };
    bool linesearch_submit(int ctx, int measure, int64_t depth, const double* norms, const std::vector<LineGroup>& groups,
                           std::string* err);
    bool linesearch_collect(int ctx, std::vector<double>* means, LsCounts* counts, std::string* err);
    // lock step: submit, then collect (LS_TOPK on context 0, LS_FULLRANK on a context of its own on the main stream)
    bool linesearch(int measure, int64_t depth, const double* norms, const std::vector<LineGroup>& groups,
                    std::vector<double>* means, LsCounts* counts, std::string* err);
    // resident per-document sums for LineGroup::resident_slot: `slots` double-buffered arrays of np doubles
    // Returns an owner ticket (0 on failure).  A later reserve by someone else takes the buffers over: groups
    // and stores that carry the old ticket are then treated as non-resident / refused.
    uint64_t resident_reserve(size_t slots, std::string* err);
    // slot <- the scores of score slot b of the last score_linear() call (exact ordered sums); false with an
    // empty *err when the ticket is stale
    // (v: the d weights whose sums these are -- read by the tick capture only)
    bool resident_store_from_scores(uint64_t owner, size_t slot, size_t b, std::string* err, const double* v = nullptr);
    // Tick capture, a test hook: while on, every resident_store_from_scores and every collected line search
    // appends an event to a host-side log (copies and synchronisations of its own; nothing it records feeds back).  Off, the
    // default, costs an untaken branch at each of those points.  capture_take moves the log out.
    void capture_enable(bool on);
    // ... a store event for sums that were stored before the capture was switched on (v: the d weights; nothing is copied)
    void capture_note_store(size_t slot, const double* v);
    void capture_take(std::vector<LsCapture>* out);
    const std::vector<double>& column_absmax() const;  // per-column max |x|
    // line searches evaluated by the exact kernels alone (NDCG@k: every group of the line search was routed there; the other
    // measures: a recent line search had > 25 % of its pairs redone)
    unsigned long long exact_fallbacks() const;
    // NDCG@k: group line searches routed to the exact kernel (a restart whose last verified line search left > 25 % of its
    // pairs undecided goes there for 4, 8, 16 line searches; the other groups of the tick stay on the verify kernel), and
    // the (query, group, 16-candidate slice) entries the verify kernel listed for recomputation
    void routing_counters(unsigned long long* exact_groups, unsigned long long* redo_entries) const;
    // NDCG@k verify kernel: documents that made a wave run its insertion chain, and the (document, group) visits they are out of
    // ... and the restarts whose R ranks were found worth keeping / not worth it (linesearch_policy.hpp: LsPolicy::Slot::rank_mode)
    void chain_counters(unsigned long long* runs, unsigned long long* visits, unsigned long long* ranked_on = nullptr,
                        unsigned long long* ranked_off = nullptr) const;
    // FR_VERIFY_AUDIT=1: values re-derived by the exact kernel after a bound-and-verify line search / how many differed
    void audit_counters(unsigned long long* values, unsigned long long* mismatches) const;
    bool download_last_matrix(std::vector<double>* out, size_t* ldm, std::string* err);

    // --- random-forest training (src/random_forest.rs:211-408; kernels_rf.inc) ---------------------------------
    // A batch of trees is grown level by level.  rf_begin: tree t's sampled instances are root_ids[root_off[t] ..
    // root_off[t+1]) (original instance ids, in the order the sample is iterated), its sampled features
    // feats[t*nf .. t*nf+nf); every instance starts in node key t.
    struct RfActive { uint32_t tree, key, n; };
    struct RfCand { double position, importance; uint32_t ids_i, flags, pos_l, pos_r; double sum_l, sum_r; };
    struct RfSplit { int32_t fslot; uint32_t pos, left, right; };
    // File-loaded datasets: bit f of bits_by_instance[id * words + f / 32] = instance id HOLDS feature f (the reference's
    // FeatureStats skips absent values, src/normalizers.rs:24-29, while the sort reads them as 0.0).  nullptr: all held.
    bool rf_set_presence(const uint32_t* bits_by_instance, size_t words, size_t n_instances, std::string* err);
    // lambda_targets: the instances' split targets are the f32 LambdaMART gradients of the last lambda_gradients() call
    // instead of their gains (the tree then fits the gradients: labels_int does not apply)
    bool rf_begin(const std::vector<uint32_t>& root_off, const std::vector<uint32_t>& root_ids, uint32_t nf,
                  const std::vector<uint32_t>& feats, std::string* err, const uint32_t* positions = nullptr,
                  bool lambda_targets = false);
    // host only, callable from another thread while the device works: positions[g] = where instance root_ids[g] sits in the
    // tiled layout (what rf_begin otherwise works out itself); hand the result to rf_begin
    bool rf_positions(const std::vector<uint32_t>& root_ids, uint32_t* positions /*[root_ids.size()]*/, std::string* err);
    // compute_output of every tree's whole sample (random_forest.rs:344-351: a root that does not split)
    bool rf_root_outputs(std::vector<double>* out, std::string* err);
    // one level: for every active node (slot = its index in `active`; slot_of_key maps node keys to slots, IDX for
    // closed nodes) and every feature slot, the k-1 split candidates: cands[(slot*nf + fi)*(k-1) + c-1];
    // label_minmax[slot*2 .. +2)
    bool rf_level(const std::vector<RfActive>& active, const std::vector<uint32_t>& slot_of_key, uint32_t k, int method,
                  uint32_t min_leaf, std::vector<RfCand>* cands, std::vector<float>* label_minmax, std::string* err);
    // the host's decisions for the level just evaluated: instances move to the children's keys; child_out[slot*2 + side]
    // = compute_output of that child (random_forest.rs:32-41)
    bool rf_split(const std::vector<RfSplit>& splits, std::vector<double>* child_out, std::string* err);
    // test hook: the sorted arrays of the level rf_level just evaluated, as the device holds them (payloads, values, gains)
    bool rf_debug_sorted(std::vector<uint32_t>* svals, std::vector<float>* sv, std::vector<float>* sg, std::string* err);
    void rf_end();
    // device bytes per (sampled instance x sampled feature) of a batch: two key and two payload arrays (8 + 8 + 4 + 4), the sorted
    // gains and values of this level and the one before (4 x 4), the side byte of the stable partition
    size_t rf_bytes_per_item() const { return 41; }

    // --- LambdaMART gradients (kernels_lambda.inc) ------------------------------------------------
    // One gradient pass on score slot 0: per document the LambdaRank gradient lambda and weight w (f64) and float(lambda),
    // the split target rf_begin(.., lambda_targets = true) reads.  norms[nq]: the NDCG evaluator's; depth < 0 = None.
    struct LambdaPass {
        // [nq] (optional): only queries with a non-zero flag are visited (still longest first); they get the bits the full
        // pass gives them, the values of the others are left as they were and must not be read
        const unsigned char* query_flags = nullptr;
        // query_flags are those of the previous call (a fixed training split): the filtered query list already on the device
        // is used again, nothing is uploaded
        bool flags_unchanged = false;
        // T >= 1: a pair contributes only when the better ranked of its documents is in the top T (0: every pair)
        uint32_t truncation_level = 0;
        // every query's lambda and w are scaled by log2(1 + S_q) / S_q.  With this or a level set the pass runs
        // lambda_grad_trunc_kernel, with neither lambda_grad_kernel ("Truncation and normalisation")
        bool lambda_norm = false;
        // 0 = NDCG (the pair weight is |delta NDCG|), 1 = MAP, 2 = MRR; norms are then the AP / RR evaluator's and depth is
        // not read ("Objectives").  The same two kernels, instantiated for the objective
        int objective = 0;
        // objective = LM_OBJECTIVE_XENDCG (3; DESIGN.md section 11, "Listwise objective"): the listwise cross-entropy pass,
        // lambda_grad_xe_kernel; norms are the NDCG evaluator's (read for `> 0` only), depth and sigma are not read, and
        // truncation_level / lambda_norm must be at their defaults.  xe_key: the tree's key of the gamma stream
        uint64_t xe_key = 0;
    };
    bool lambda_gradients(const double* norms, int64_t depth, double sigma, const LambdaPass& pass, std::string* err);
    // the last pass's lambda / w by padded position ([np] each)
    bool lambda_download_positions(std::vector<double>* lambda, std::vector<double>* weight, std::string* err);
    // ... scattered to original instance ids (ids outside this dataset or >= out_len are left untouched)
    // (with query_flags: the instances of unflagged queries as well)
    bool lambda_download(double* lambda_by_instance, double* weight_by_instance, size_t out_len, std::string* err,
                         const unsigned char* query_flags = nullptr);

    // --- LambdaMART's DART boosting (kernels_dart.inc; DESIGN.md section 11, "DART") -----------------
    // A cache of the leaf (u16, depth-first numbering) every document reaches in every tree, by the documents' logical index
    // (a sampled view: its own tiles), next to a table of the trees' leaf values; the scores of any weighting of any subset
    // of the trees are re-formed from it without walking a tree.
    // dart_begin: an empty cache of `rows` trees, allocated after a check against the device's free memory (*cache_bytes:
    // its size); dart_end frees it.
    bool dart_begin(size_t rows, uint64_t* cache_bytes, std::string* err);
    // Row `row` (rows are filled in order, 0 first) from score slot 0, which must hold the documents' leaf numbers: the scores
    // of a copy of the tree whose leaves hold their own index.  leaf_values[n_leaves] (at most 65536): the tree's leaf values.
    bool dart_fill(size_t row, const double* leaf_values, size_t n_leaves, std::string* err);
    // score slot 0 = ensemble accumulator = s, per document: s = +0.0; for k ascending s = s + weights[trees[k]] * tree_{trees[k]}(x),
    // product and sum rounded separately (dart_rescore_kernel).  trees[n_trees]: ascending, every entry < n_weights <= filled rows.
    bool dart_rescore(const double* weights, size_t n_weights, const uint32_t* trees, size_t n_trees, std::string* err);
    // a row scattered to original instance ids (ids >= out_len are left out)
    bool dart_download_row(size_t row, uint16_t* out_by_instance, size_t out_len, std::string* err);
    void dart_end();

    // --- LambdaMART histogram grower (kernels_hist.inc) ----------------------
    // The host (lambdamart_hist.hpp) keeps the tree and decides; the device keeps the bin matrix, the fixed-point gradients,
    // an index list partitioned by node, and one level's histograms [slot][feature][bin] of (count u32, sum Q i64).
    struct HistNode { uint32_t slot, begin, end; };             // a node's histogram slot and its stretch of the index list
    struct HistSplit { uint32_t begin, end, fslot, edge, nl; }; // bins 0..edge of feature slot fslot go left: nl of them
    struct HistSub { uint32_t parent, small, large; };          // next level's slot `large` = this level's `parent` - next level's `small`
    struct HistBounds { double lo, hi; };                       // a node's interval for its output ("Monotone constraints")
    // What a tree's searches are made with.  newton ("Newton split gain"): the histograms also hold sum W, imp = term(L) +
    // term(R), term = G G / (H + lambda_l2) with G = ldexp(Q, -s_l), H = ldexp(W, -s_w), and a candidate also needs
    // H >= min_sum_hessian and H + lambda_l2 > 0 on both sides; without it min_leaf alone is read.  min_split_gain is read by
    // the symmetric pair only (elsewhere the host applies it).  monotone ("Monotone constraints"; Newton gain only): the two
    // sides' outputs are clamped to the node's interval, a clamped side's term is (2 G) v - ((H + lambda_l2) v) v, and the
    // order vL <= vR (sign +1) / vL >= vR (sign -1) is among a candidate's conditions.
    // lambda_l1 / max_delta_step / path_smooth ("Leaf regularisation"; Newton gain only; all 0: off): a side's output is the
    // soft-thresholded gradient sum over H + lambda_l2, capped, pulled toward the parent's output and clamped, and a moved
    // side's term is the clamped one's; with any of them set the scan kernels are those of kernels_histreg.inc, with or
    // without monotone signs, and a node's record is a HistRegNode.
    struct HistSearch {
        uint32_t min_leaf; bool newton; int s_l, s_w; double lambda_l2, min_sum_hessian, min_split_gain; bool monotone;
        double lambda_l1 = 0.0, max_delta_step = 0.0, path_smooth = 0.0;
        bool reg() const { return lambda_l1 != 0.0 || max_delta_step != 0.0 || path_smooth != 0.0; }
    };
    // a node's interval, its parent's output and whether it has one ("Leaf regularisation")
    struct HistRegNode { double lo, hi, parent; uint32_t has_parent, pad; };
    // A candidate (valid = 0: none): bins 0..edge go left, nl instances of sums (ql, wl); (qtot, wtot): the node's.  Under the
    // variance criterion wl = wtot = 0.  fi: the feature's index among the tree's, from the leaf-wise calls only (else 0).
    struct HistCand { double imp; long long ql, qtot, wl, wtot; uint32_t edge, nl, valid, fi; };
    // bins of the instance list (positions[n], rf_positions' output) for the features `feats` and k = split_candidates
    // (2..256); kept until any of the three changes.  *built = false when the kept ones were reused.
    bool hist_bins(const uint32_t* positions, size_t n, const std::vector<uint32_t>& feats, uint32_t k, bool* built, std::string* err);
    // edges[slot * 256 + j], j < nedges[slot]
    bool hist_edges(std::vector<float>* edges, std::vector<uint32_t>* nedges, std::string* err);
    bool hist_download_bins(uint8_t* out /*[features][n]*/, size_t len, std::string* err);
    // The sample of the trees grown from now on, until hist_bins is called again.  query_flags[nq] (nullptr: every query):
    // the root's index list becomes the ascending list of the instance-list indices whose query is flagged, made on the
    // device; n_t must be their number.  fsel[f_t] (nullptr: every feature): ascending slots of the bin matrix; a level's
    // histograms are then [slot][f_t][bin] and a search's records are indexed by these f_t features.  HistSplit::fslot
    // stays a slot of the bin matrix.  Bins and edges are never rebuilt.
    // keep_queries (with query_flags == nullptr): the query sample of the previous call stays (a fixed training split under
    // per-tree feature samples); only the feature sample changes.
    bool hist_sample(const unsigned char* query_flags, uint32_t n_t, const uint32_t* fsel, size_t f_t, std::string* err,
                     bool keep_queries = false);
    // GOSS ("GOSS"; kernels_goss.inc) for the next tree, on top of the sample: of the sample's list L (lambda from the last
    // gradient pass, or lam_list in instance-list order) the n_top entries with the largest |lambda| (ties in list order) and
    // every other entry whose uniform u(tree_key, original instance id) is below p are the tree's list; hist_quantise then
    // multiplies the kept others' lambda and w by amp.  *n_g: the list's length; *tau (may be nullptr): the n_top-th largest
    // key.  Holds until the next hist_sample, hist_bins or hist_goss.
    bool hist_goss(const double* lam_list, uint32_t n_top, double p, double amp, uint64_t tree_key, uint32_t* n_g, uint64_t* tau,
                   std::string* err);
    // the list hist_goss made (list[n_g], full-list indices ascending) and per entry of it whether it is in the top set
    bool hist_goss_download(uint32_t* list, uint8_t* top, size_t len, std::string* err);
    // Q / W of the tree to grow, from the last gradient pass (lam_list == nullptr) or from host arrays in instance-list
    // order.  *all_zero: every lambda is 0 (nothing was quantised); s_l / s_w: the exponents S of the definition
    bool hist_quantise(const double* lam_list, const double* wt_list, int* s_l, int* s_w, bool* all_zero, std::string* err);
    // Quantised gradients ("Quantised gradients"; kernels_histquant.inc; Newton gain only) for the tree hist_quantise has just
    // prepared: (q, w) of `bits` bits (2..8) per entry of the tree's list under tree_key and the documents' original instance
    // ids.  *d / *d_w: the two shifts: the sums the searches read are then under the exponents s_l - d and s_w - d_w, the leaf
    // sums stay under (s_l, s_w).  Holds until the next hist_quantise, hist_sample or hist_bins.  Waits for the stream.
    bool hist_quantq(uint32_t bits, uint64_t tree_key, int* d, int* d_w, std::string* err);
    // the values hist_quantq made, by index of the tree's list (len = its length)
    bool hist_quantq_download(int32_t* q, uint32_t* w, size_t len, std::string* err);
    // the level's slot 0 after hist_root(true): count, sum Q and sum W as [features][k] (cells = their product)
    bool hist_root_download(uint32_t* cnt, long long* sum, long long* wsum, size_t cells, std::string* err);
    // index list = the sample's root list (0..n-1 without one); the level holds the root's histogram in slot 0.  newton: with sum W
    bool hist_root(bool newton, std::string* err);
    // One level's search.  best[a * features + slot]: node a's last-maximum candidate of that feature (the level was made
    // with how.newton); bounds: nullptr unless how.monotone, then node a's interval is (*bounds)[a]; reg: nullptr unless
    // how.reg(), then node a's record is (*reg)[a] and bounds is not read (signs must be set, all zero without a constraint)
    bool hist_search(const std::vector<HistNode>& nodes, const HistSearch& how, const std::vector<HistBounds>* bounds,
                     std::vector<HistCand>* best, std::string* err, const std::vector<HistRegNode>* reg = nullptr);
    // signs[features] in {-1, 0, +1}, one per row of the bin matrix, kept until the next call or the next bins
    bool hist_monotone(const int* signs, size_t features, std::string* err);
    // Symmetric trees ("Symmetric trees").  hist_search_symmetric: best[f] = the last-maximum candidate of feature f of the
    // tree's by its level importance I over `nodes` in their order (key: I, -inf for a NaN one; valid = 0: no node splits
    // under any edge of f).  hist_symmetric_apply: out[a] = node a's record under the candidate (feature fi of the tree's,
    // edge), valid = the node splits under it.
    struct HistSymBest { double key; uint32_t edge, valid; };
    bool hist_search_symmetric(const std::vector<HistNode>& nodes, const HistSearch& how, std::vector<HistSymBest>* best, std::string* err);
    bool hist_symmetric_apply(const std::vector<HistNode>& nodes, const HistSearch& how, uint32_t fi, uint32_t edge, std::vector<HistCand>* out,
                              std::string* err);
    // stable partition of the splitting nodes' stretches, then the next level (next_slots histograms; 0: none): `builds` are
    // built from their stretches, `subs` by subtraction from the level just searched
    bool hist_split(const std::vector<HistSplit>& splits, const std::vector<HistNode>& builds, const std::vector<HistSub>& subs,
                    uint32_t next_slots, bool newton, std::string* err);
    bool hist_leaf_sums(const std::vector<HistNode>& leaves, std::vector<long long>* qw /*[leaf][2]*/, std::string* err);
    void hist_end();  // frees the level histograms and the leaf-wise pool (the bins stay)
    // Leaf-wise growth ("Leaf-wise growth"): a pool of `slots` histograms replaces the level arrays, one leaf is split per
    // step and one record per searched node comes back (hist_pick_kernel reduces the features on the device).
    // index list = the sample's root list; the root's histogram into slot 0 of a fresh pool; *root: the root's record (under
    // how.monotone its interval is the whole line, the children's come with the step)
    bool hist_leaf_begin(uint32_t slots, const HistSearch& how, HistCand* root, std::string* err);
    // One split step: the stable partition of split's stretch alone; then, when small_slot != HIST_NO_SLOT, the smaller child's
    // histogram is built into small_slot; a searched larger child is derived in place in parent_slot (parent - smaller) and a
    // searched child is scanned.  pick[0]: the lhs's record, pick[1]: the rhs's (written for the searched ones only).
    static constexpr uint32_t HIST_NO_SLOT = 0xffffffffu;
    // (bounds[0] / bounds[1]: the lhs's / rhs's interval, read only when how.monotone or how.reg(); parent_out: the output of
    // the node being split, both children's parent output, read only when how.reg())
    struct HistLeafStep { HistSplit split; uint32_t parent_slot, small_slot; bool search_lhs, search_rhs; HistBounds bounds[2] = {}; double parent_out = 0.0; };
    bool hist_leaf_step(const HistLeafStep& step, const HistSearch& how, HistCand pick[2], std::string* err);

    // --- model explanation (explain.hip, a translation unit of its own) ---------
    // What that unit reads of a dataset, once this dataset's stream has drained: the feature tiles (kernels_score.inc:
    // float index(p, j) = ((p >> 6) * dq + (j >> 2)) * 256 + (p & 63) * 4 + (j & 3)) and, per padded position, the
    // instance id of this dataset's document there (IDX_INVALID: padding, or a document of the parent that a sampled view
    // does not hold).  Read only; the pointers live as long as the dataset.
    struct TileForm {
        const float* xb = nullptr;
        size_t np = 0, dq = 0, d = 0, n = 0;
        int device = 0;
        bool nonfinite = false;
        const uint32_t* perm_host = nullptr;  // [np]
    };
    bool tile_form(TileForm* out, std::string* err);

    int take_flags();  // returns and clears the accumulated kernel error bits

    // --- permutation importance (kernels_permute.inc + permute.inc; DESIGN.md section 16, permute.hpp) -----------
    // [np] per padded position the instance id of this dataset's document there (IDX_INVALID: none); host memory
    const uint32_t* position_instances(size_t* np) const;
    // src_pos[r * np + p]: the position whose value of the permuted feature position p reads in repeat r (p itself wherever
    // no document of this dataset sits); uploaded once per call
    bool permute_begin(const uint32_t* src_pos, uint32_t R, PermuteStats* stats, std::string* err);
    // how many features a chunk may hold: max_slots (0: half of the free HBM) over R slots each, `sets` sets of score slots
    // beside the nq x B result matrix
    size_t permute_chunk_features(size_t nfeat, uint32_t R, size_t max_slots, size_t sets) const;
    // score slot fi * R + r = the model's scores on D_{feats[fi], r} (feats ascending); with `ensemble` the members are added
    // in order, else there is one member.  Waits for the stream.
    bool permute_score(const uint32_t* feats, size_t nf, const std::vector<PermuteMember>& members, bool ensemble, PermuteStats* stats,
                       std::string* err);
    // frees what permute_begin and permute_score allocated, the grown score slots included
    void permute_end();

    // --- read-back of the device form, for the tests that hold every table to its definition ------
    // Read only, used by no product path: sizes, switches and buffer addresses (to compare, never to follow) by name, and
    // a copy of one named static table as bytes once the dataset's stream has drained.  *present = false: the dataset has
    // no such table (an optional copy that was not made); an unknown name is an error.
    std::vector<std::pair<std::string, uint64_t>> debug_form_scalars() const;
    bool debug_form_table(const std::string& name, std::vector<unsigned char>* out, bool* present, std::string* err);

  private:
    DeviceDataset();
    bool try_score_trees_rank(const FlatTrees& trees, std::string* err);
    bool try_score_trees_lds(const FlatTrees& trees, std::string* err);
    bool try_score_trees_lds_shape(const FlatTrees& trees, const TreeShape& shape, std::string* err);
    struct Impl;
    Impl* impl_;
};

// process-wide helpers -------------------------------------------------------------------------
int device_count(std::string* err);
bool set_device(int ordinal, std::string* err);
void warm_device(int ordinal);  // pays the runtime's first-stream cost on that device once per process
void profile_enable(bool on);
void profile_reset();
std::vector<KernelStat> profile_stats();
bool device_synchronize(std::string* err);
// one timed device-to-device copy src -> dst as replicate() makes them (device_plumbing.inc)
// The job's one exchange as a single-process RCCL all-gather over `devices` (rccl_exchange.inc): rank i contributes
// blocks[i * block_len .. (i + 1) * block_len), every rank receives all blocks in rank order; *gathered = rank 0's buffer.
// rep->ran = false with a reason when it does not apply (one rank; ranks sharing a GPU); with N distinct GPUs any failure --
// and any gathered buffer that differs from the blocks -- returns false.
struct RcclReport {
    bool ran = false, matches_host_gather = false;
    int ranks = 0;
    std::vector<int> devices;
    size_t block_doubles = 0;
    double init_us = 0.0, first_us = 0.0, us = 0.0;  // ncclCommInitAll; the first all-gather (lazy set-up included); the second
    std::string reason;                               // why it did not run
    std::string library;                              // the librccl.so that ran (next to this library's own HIP runtime)
};
bool rccl_allgather(const std::vector<int>& devices, const double* blocks, size_t block_len, std::vector<double>* gathered, RcclReport* rep,
                    std::string* err, size_t min_ranks = 2);  // (min_ranks = 1: the self-test -- a one-rank communicator really runs)
bool peer_copy_probe(int src, int dst, size_t bytes, int* can_access, int* enabled, double* ms, std::string* err);
size_t device_free_bytes();
// page-locked host memory (nullptr when none is left: the caller falls back to ordinary memory); for staging uploads that
// a helper thread prepares -- a copy from ordinary memory ran at under 1 GB/s on some of the boxes this was measured on
void* pinned_alloc(size_t bytes);
void pinned_free(void* p);
// size class of the full-ranking kernel a query of `len` documents is sorted in: *nl keys per lane, *pl lanes per candidate
// (no device needed; fullverify.hpp FV_CLASSES)
void fullrank_class_of(uint32_t len, uint32_t* nl, uint32_t* pl);  // free HBM on the current device (0 if unknown)
// the two inputs of the host-side layout (dataset_layout.hpp) that create() / create_view() take from this library: the
// size classes of the full-ranking kernel over a dataset's queries (SizeClass::npad = index into FV_CLASSES; *list = the
// queries sorted by class) and the documents a run takes (no device needed)
std::vector<SizeClass> fv_build_classes(const std::vector<uint32_t>& qlen, std::vector<uint32_t>* list);
size_t run_docs_target();

}  // namespace frdev
