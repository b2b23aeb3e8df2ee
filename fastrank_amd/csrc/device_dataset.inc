// Part of device.hip (single translation unit; see that file's header).  DeviceDataset: its state (Impl), the scoring and metric
// launchers and the line search.  The dataset build (dataset_build.inc), forest scoring (score_trees.inc) and the trainers' launchers
// (train_*.inc) are included at the places their text had.  The scoring and line-search code stays in this file because bench.py
// keys its static counter captures to this file's hash: moved out, it could change without marking those captures stale (the tree
// captures are keyed to this file too: a change of score_trees.inc or forest_pack.hpp does not mark them).
// ----------------------------------------------------------------------------------------------
// DeviceDataset
// ----------------------------------------------------------------------------------------------

static constexpr int LS_CONTEXTS = DeviceDataset::LINESEARCH_CONTEXTS;

// ---- size classes of kernels_fullverify.inc ---------------------------------------------------------------------
// Modelled VALU wave-instructions to rank one query for 64 candidate lanes in class (nl keys per lane, pl lanes per
// candidate): key generation 2, the in-lane network 2 per compare-exchange, per merge round r its r cross-lane stages
// (two DPP moves + compare + two selects per key) and the in-lane bitonic tail, verification 2, term lookup 3, and the
// sequential sum whose pl phases every lane sits through; times a per-round factor measured on the device.
static double fv_class_cost(int ci) {
    static const int sort_ce[] = {63, 191, 384, 543, 849, 1056}, merge_ce[] = {32, 80, 144, 192, 304, 336};
    const uint32_t nl = FV_CLASSES[ci].nl, pl = FV_CLASSES[ci].pl;
    const int ni = (int)nl / 16 - 1;
    uint32_t rounds = 0;
    while ((1u << rounds) < pl) rounds++;
    double c = 2.0 * nl + 2.0 * sort_ce[ni] + 5.0 * nl + (double)nl * pl;
    for (uint32_t r = 1; r <= rounds; r++) c += 5.0 * r * nl + 2.0 * merge_ce[ni];
    // measured / modelled on the device (tools/ab/fv_ab.sh, 30K shape): the multi-lane classes lose issue slots to the
    // exchanges' latency, more with every round
    static const double lane_penalty[] = {1.0, 1.1, 1.25, 1.6, 2.0, 2.4};
    return c * pl * lane_penalty[rounds];
}

// class of a query of `len` documents: the cheapest one that holds it (FR_FV_CLASSES=pow2: only the power-of-two
// classes of round 2, for A/B runs)
static int fv_class_of(uint32_t len) {
    static const bool pow2_only = [] {
        const char* e = frdev::pricing_env("FR_FV_CLASSES");
        return e != nullptr && std::strcmp(e, "pow2") == 0;
    }();
    int best = -1;
    double best_cost = 0.0;
    for (int ci = 0; ci < FV_NCLASSES; ci++) {
        const uint32_t nl = FV_CLASSES[ci].nl, pl = FV_CLASSES[ci].pl, npad = nl * pl;
        if (npad < len) continue;
        if (pow2_only && ((npad & (npad - 1)) != 0 || (nl != 64 && pl != 1))) continue;
        const double c = fv_class_cost(ci);
        if (best < 0 || c < best_cost) best = ci, best_cost = c;
    }
    return best < 0 ? FV_NCLASSES - 1 : best;
}

void fullrank_class_of(uint32_t len, uint32_t* nl, uint32_t* pl) {
    const int ci = fv_class_of(len > 2048 ? 2048u : len);
    *nl = FV_CLASSES[ci].nl;
    *pl = FV_CLASSES[ci].pl;
}

// queries sorted by the class of kernels_fullverify.inc that takes them (stable: dataset order inside a class);
// SizeClass::npad = index into FV_CLASSES
std::vector<SizeClass> fv_build_classes(const std::vector<uint32_t>& qlen, std::vector<uint32_t>* list) {
    std::vector<int> cls_of_len(2049, -1);
    return bucket_queries(qlen, [&](uint32_t len) {
        const uint32_t l = len > 2048 ? 2048 : len;
        if (cls_of_len[l] < 0) cls_of_len[l] = fv_class_of(l);
        return cls_of_len[l];
    }, list);
}

static_assert(WT == WALK_TILE && LS_KT == DCG_RANKS && IDX_INVALID == NO_DOCUMENT, "the kernels' constants are the host layout's (dataset_layout.hpp)");

// The host-side description of a dataset: what create() / create_view() work out about it and a replica takes over from
// its source in one assignment (replicate()).  Impl derives from it, so the members read m.np, m.nq, ... everywhere.
struct DatasetDesc {
    size_t n = 0, d = 0, nq = 0, np = 0, dq = 0, maxlen = 0, nruns = 0;
    bool nonfinite = false;            // X holds inf/NaN: zero-weight masking is not exact -> no fused path
    bool labels_small_int = false;     // every label is an integer of magnitude <= 2^21: sums of up to 2^31 of them are exact in f64 in ANY order (kernels_rf.inc)
    std::vector<double> colmax;        // per-column max |x| (error bound of the bound-and-verify line search)
    int verify_xs = 1;                 // keys beyond K in the verify kernel's lists (1..4, raised on tie-heavy data)
    std::vector<uint32_t> perm_host;   // [np] original instance id or IDX_INVALID (padding, or not part of this view)
    std::vector<uint32_t> qstart_h, qlen_h, qnpos_h, qnneg_h;  // host copies (views of this dataset are cut from them)
    std::vector<uint32_t> wt_start_h;  // [nwt + 1] host copy of wt_start
    size_t nwt = 0;
    std::vector<double> colstd;        // per-column standard deviation over the dataset's documents
    std::vector<uint8_t> colmode;      // bit 0 / 1: more than a tenth of the documents sit at the column's maximum / minimum
    std::vector<ColStats> colstats_h;  // the records colstd / colmode were made from (read by debug_form_table alone)
    uint32_t key_bits = 0, key_cls_bits = 0;  // gkey: gain class | duplicate group << key_cls_bits
    uint64_t dup_groups = 0;           // duplicate groups found at upload, over all queries (whether or not gkey carries their ids)
    std::vector<SizeClass> size_classes;  // queries bucketed by next power of two of their length
    std::vector<SizeClass> fv_classes;    // queries bucketed by the cheapest class of kernels_fullverify.inc (npad = index into FV_CLASSES)
    uint64_t relmask = 0;              // bit c: gain class c has gain > 0
    size_t ncls = 0, tablen = 0;
    bool dcg_terms_in_range = false;   // every term of dcgtab is 0 or of a magnitude verify_quotient is proven for (verify_end.hpp)
};

// create()'s helper thread tells the tile thread that the main stream exists, or that it could not be made
struct StreamSignal {
    std::mutex mu;
    std::condition_variable cv;
    bool done = false, ok = true;
    void set(bool good) {
        {
            std::lock_guard<std::mutex> lk(mu);
            if (!good) ok = false;
            done = true;
        }
        cv.notify_all();
    }
    bool wait() {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return done; });
        return ok;
    }
};

struct PermuteState;  // permute.inc: what a permutation-importance call keeps on the device between its chunks

struct DeviceDataset::Impl : DatasetDesc {
    // resident base sums / error bounds shared by the bound-and-verify paths (defined further down)
    // Per-tick parameters of the bound-and-verify paths travel as ONE page-locked block and one copy (the redo
    // counter, zeroed, rides along); results come back into page-locked memory with one synchronisation.
    struct TickStage {
        size_t G = 0, dp = 0;
        size_t o_count = 0, o_gredo = 0, o_gthr = 0, o_gmode = 0, o_rank = 0, o_gfeat = 0, o_gncand = 0, o_slot = 0, o_updf = 0, o_gcand = 0, o_eps2 = 0, o_par = 0, o_gw = 0, total = 0;
    };
    // A line-search context: its own stream and every buffer one tick writes, so that two ticks (of disjoint sets
    // of restarts) can be in flight at once and the host's work between the ticks of one set hides behind the
    // kernels of the others.  ls[0 .. LS_CONTEXTS-1]: submit / collect (ls[0] also the lock-step top-k path);
    // ls[LS_CONTEXTS]: the lock-step full-ranking path (main stream).
    // The three verify kernels a line search can take: top-k NDCG, reciprocal rank, full-ranking NDCG / AP
    enum LsKind { LSK_TOPK, LSK_RR, LSK_FV };
    struct LsCtx {
        hipStream_t stream = nullptr;
        PinnedBuf tick_h, tick_res;
        DevBuf<unsigned char> tick_d;
        DevBuf<double> M, means, partial;
        DevBuf<uint32_t> redo;  // [nq * G]: the (query, group) pairs to redo exactly (NDCG@k: with a slice mask); their count: tick block
        DevBuf<int> flags;
        template <typename T> T* th(size_t off) { return reinterpret_cast<T*>(tick_h.p + off); }
        template <typename T> T* td(size_t off) { return reinterpret_cast<T*>(tick_d.p + off); }
        // a submitted, not yet collected line search
        bool pending = false, approx = false;
        bool ready = false;  // evaluated by the exact kernels at submit: exact_means holds the result
        LsKind kind = LSK_TOPK;
        TickStage ts;
        LSArgs a;     // top-k: the kernels' arguments; every kind: the resident parameters (resident_update_kernel)
        RRArgs ra;
        FSArgs fsa;   // full-ranking bound-and-verify: the exact kernels' arguments for the redo list
        RMArgs rma;
        DevBuf<double> fv_rows;  // score rows of this context's redo slots (contexts run concurrently: no sharing)
        size_t ldm = 0, maxc = 0, lds = 0;
        int64_t depth = 0;
        int measure = 0;
        int xs_used = 1;         // list length variant of the pending verify launch
        bool xs_pinned = false;  // ... chosen by FR_VERIFY_XS
        bool audit = false;      // FR_VERIFY_AUDIT
        std::vector<LineGroup> agroups;  // ... full ranking / reciprocal rank: the groups of the pending line search, for fr_audit
        unsigned redo_grid = 512, redo_grid_used = 512;  // pairs the exact kernels' fixed first launch takes (NDCG@k: adapts to the redo counts seen)
        // NDCG@k per-group routing: the pending line search staged its groups as [verify groups | exact groups];
        // gorder[k] = the caller's index of staged group k (empty: the caller's order), gslot[k] = its resident slot
        size_t nverify = 0;
        std::vector<uint32_t> gorder, gredo_h;
        std::vector<int> gslot;
        std::vector<LineGroup> pgroups;
        std::vector<double> exact_means;
        LsCounts counts;  // this line search's verify pairs / redone pairs
        // what the tick capture reports of the pending line search (cgroups: the caller's groups, copied only while it is on)
        bool resident = false, dup = false;
        int kbucket = 0;  // K of the linesearch_verify_kernel<K, ...> launched (0: no verify launch)
        std::vector<LineGroup> cgroups;
    };
    LsCtx ls[LS_CONTEXTS + 1];
    hipEvent_t res_ready = nullptr;  // recorded on the main stream after a resident-sum store; the contexts wait on it
    bool res_ready_set = false;
    const double* last_M = nullptr;  // device matrix of the last per-query result (download_per_query / reduce_means)
    // reduce_subset_means: the two subsets' queries (a then b), their sizes, the segment sums and the two means
    DevBuf<uint32_t> sub_idx;
    DevBuf<double> sub_partial, sub_means;
    uint32_t sub_na = 0, sub_nb = 0;
    bool ls_submit(LsCtx& c, int path, int measure, int64_t depth, const double* norms, const std::vector<LineGroup>& groups,
                   std::string* err);
    // what ls_submit's prologue hands the launcher of the line search's kind: the staged groups (routed ones last), of which the
    // verify kernel may take the first nV, and whether they read the resident sums / carry pending updates of them
    struct LsTick { const std::vector<LineGroup>& groups; const double* norms; size_t nV; bool resident, any_update; };
    bool submit_topk(LsCtx& c, const LsTick& t, std::string* err);
    bool submit_rr(LsCtx& c, const LsTick& t, std::string* err);
    bool submit_fv(LsCtx& c, const LsTick& t, std::string* err);
    bool exact_instead(LsCtx& c, const LsTick& t, std::string* err);
    bool submit_queued(LsCtx& c, const LsTick& t, size_t nverify, std::string* err);
    bool ls_collect(LsCtx& c, std::vector<double>* means, std::string* err);
    bool topk_policy(LsCtx& c, uint32_t nredo, uint32_t nslices, std::string* err);
    bool ls_exact(LsCtx& c, int measure, int64_t depth, const double* norms, const std::vector<LineGroup>& groups, std::string* err);
    bool exact_kernels(const std::vector<LineGroup>& groups, int measure, int64_t depth, size_t maxc, double* M, int* flags, std::string* err);
    bool fr_audit(LsCtx& c, std::string* err);
    // tick capture (DeviceDataset::capture_enable).  cap_outer: the context whose line search the lock-step context is
    // evaluating on its behalf (ls_exact): the event is recorded there, with the matrix, under the outer context's name
    bool cap_on = false;
    std::vector<LsCapture> cap_log;
    const LsCtx* cap_outer = nullptr;
    bool capture_tick(LsCtx& c, const std::vector<double>& means, uint32_t nredo, std::string* err);
    bool ls_means(LsCtx& c, std::string* err);
    bool tick_begin(LsCtx& c, const std::vector<LineGroup>& groups, std::string* err);
    bool tick_upload(LsCtx& c, bool with_eps2, std::string* err);
    bool tick_finish(LsCtx& c, size_t ldm, std::vector<double>* means, uint32_t* nredo, std::string* err, uint32_t* npairs = nullptr,
                     std::vector<uint32_t>* by_group = nullptr);
    bool stage_resident(LsCtx& c, const std::vector<LineGroup>& groups, bool* any_update_out);
    // key_relative (the NDCG@k verify kernel): eps2_host holds only the ABSOLUTE part of a pair's bound, eps_gamma the factor on
    // |key_a| + |key_b| the kernel adds (verify_far)
    bool compute_eps2(const std::vector<LineGroup>& groups, bool resident, uint32_t cls_bits, bool bare_admission = false, bool key_relative = false);
    double eps_gamma = 0.0;
    bool update_resident(LsCtx& c, size_t g_base, size_t ng, std::string* err);
    void flip_resident(const std::vector<LineGroup>& groups);
    bool redo_launch(LsCtx& c, uint32_t off, const uint32_t* count_dev, uint32_t n, std::string* err);
    FSArgs scores_args(const uint32_t* gfeat, const double* gw, const double* gcand, double* rows, int* flags, size_t gc) const;
    RMArgs rank_args(const double* rows, const uint32_t* gncand, double* M, int* flags, size_t gc, size_t ldm, int measure, int64_t depth) const;
    void topk_args(LsCtx& c, size_t G) const;
    RRArgs rr_args(LsCtx& c, size_t G) const;
    FVArgs fv_args(LsCtx& c, size_t G, uint32_t cls_bits, uint32_t dup_bits) const;
    int device = 0;
    hipStream_t stream = nullptr;
    std::vector<double> eps2_host;
    DevBuf<double> res;                // resident base sums: [slots][2][np]
    std::vector<uint8_t> res_half;     // which half of each slot is current
    uint64_t res_owner = 0;            // ticket of the trainer that owns the resident buffers
    LsPolicy pol;                      // what the next line searches are asked to do: routing / back-off, R-rank refreshes, skip counter (linesearch_policy.hpp)
    unsigned long long approx_pairs = 0, approx_redo = 0;  // statistics, in (query, group) pairs
    unsigned long long approx_redo_entries = 0;            // ... and in 16-candidate slices of them (NDCG@k)
    unsigned long long chain_runs = 0, chain_visits = 0;   // NDCG@k verify kernel: insertion-chain runs / (document, group) visits
    unsigned long long audit_values = 0, audit_mismatches = 0;  // FR_VERIFY_AUDIT=1: published values re-derived by the exact kernel
    DevBuf<double> audit;
    DevBuf<unsigned long long> audit_cnt;
    DevBuf<int> audit_flags;  // (the exact kernels' flags of an audit: the published ones are not touched)
    unsigned long long exact_fallbacks = 0;                // line searches evaluated by the exact kernels alone (every group routed there, or approx_skip)
    std::shared_ptr<DeviceDataset> parent;  // a view: the dataset whose tiles and per-document arrays this one aliases
    DevBuf<uint32_t> run_lo;
    DevBuf<uint32_t> vtiles;           // a view: the 64-position tiles of the parent's position space that hold its documents (ascending)
    size_t nvtiles = 0;                // (0: the dataset owns its position space and visits all of it)
    PosMap posmap() const { return PosMap{nvtiles ? vtiles.p : nullptr, (uint32_t)nvtiles, (uint32_t)np}; }
    size_t pos_threads() const { return nvtiles ? nvtiles * 64 : np; }  // threads of a position-parallel launch
    // visiting-order tables of the resident NDCG@k verify kernel (kernels_order.inc): static per dataset ...
    DevBuf<uint8_t> xslot;             // [d][np] slot of every document inside its (query, tile) segment by x_f descending (empty: storage order)
    DevBuf<uint16_t> segtab;           // [np] that segment's first slot | one past its last << 8, relative to the walk tile (0: not a document)
    // walk tiles of the resident NDCG@k verify kernel (kernels_order.inc): stretches of up to WT consecutive positions, cut so
    // that a query of up to WT documents lies inside one
    DevBuf<uint32_t> wt_start;         // [nwt + 1] first position of every walk tile, ascending; [nwt] = np
    DevBuf<uint32_t> run_wt0;          // [nruns] the walk tile that holds the run's first document
    DevBuf<uint8_t> wofs;              // [np] a position's offset inside its walk tile (the identity visiting order)
    DevBuf<uint32_t> wlist;            // a view: the walk tiles that hold its documents (ascending)
    size_t nwlist = 0;
    // ... and per trainer
    DevBuf<uint8_t> rslot;             // [slots][np] the same by the resident sum R descending
    // (when they are refreshed: LsPolicy::plan_rank_refresh / observe_chain)
    // the main stream, the line-search contexts' streams and res_ready
    hipError_t open_streams(bool* at_event, StreamSignal* main_stream = nullptr);
    bool open_streams(std::string* err);
    static bool upload_tiles(Impl& m, const HostCSR& csr, bool timing, StreamSignal& main_stream, std::string* terr);
    bool build_order_tables(std::string* err);
    DevBuf<float> xcol;                // [d][np] the tiles' columns, column-major: what the resident line search reads (empty: it reads the tiles)
    bool build_columns(std::string* err);
    DevBuf<uint16_t> gkey;             // [np] gain class | duplicate group << key_cls_bits (<= 16 bits wherever the verify kernel runs): the low mantissa bits of its keys
    DevBuf<float> xb, gain;
    DevBuf<double> gexp, disc;
    DevBuf<uint32_t> qstart, qlen, qtight, perm, rank, run_q0, run_q1, run_pos, run_docs, run_order, gcls, qlist;
    DevBuf<uint32_t> fv_qlist;
    DevBuf<uint32_t> qnpos, qnneg, sort_idx;
    DevBuf<double> sort_keys;  // global sort scratch for queries longer than the LDS sort takes
    DevBuf<double> termtab, rows;
    DevBuf<double> dcgtab;
    DevBuf<int> flags;
    DevBuf<unsigned long long> dbgc;
    // work buffers
    DevBuf<double> scores, acc, weights, M, means, partial, norms, rnorms, gw, gcand;
    DevBuf<uint32_t> gfeat, gncand;
    DevBuf<TreeNodeDev> nodes;
    DevBuf<int32_t> roots;
    DevBuf<double> tweights;
    // random-forest training batch (kernels_rf.inc)
    struct RfState {
        DevBuf<uint32_t> roff, pos, node_of, feats, slot_of_key, act_tree, act_n, vals_a, vals_b;
        DevBuf<uint64_t> act_off, act_first, keys_a, keys_b;
        DevBuf<float> sg, sv, sg_o, sv_o, label, gain_r;  // (sg_o / sv_o: the previous level's sorted gains / values, read by the partition's scatter)  // gain_r[g]: gain of sampled instance g (= gain[pos[g]]: one gather per item and level instead of two)
        DevBuf<unsigned char> temp;
        DevBuf<RfCandDev> cands;
        DevBuf<RfSplitDev> splits;
        DevBuf<double> child;
        std::vector<uint32_t> roff_h;
        std::vector<uint32_t> pos_of_id;  // original instance id -> padded position
        std::mutex pos_mu;                // (guards its one-time construction)
        uint32_t T = 0, nf = 0, total = 0;
        // the level last evaluated
        uint32_t A = 0;
        uint64_t items = 0, node_items = 0;
        bool sorted_in_b = false;
        uint64_t prev_items = 0;  // items of the previous level's open nodes, sorted, in keys_b / vals_b (0: sort from scratch)
        uint32_t prev_A = 0;
        DevBuf<uint32_t> act_tree_o, act_n_o;  // the previous level's tables (rf_rekey_kernel reads them)
        DevBuf<uint32_t> pres;  // [np][pw] which features the instance at a position holds (file-loaded datasets; empty: all)
        uint32_t pw = 0;
        DevBuf<uint64_t> act_off_o;
        // stable partition of the previous level's segments (rf_part_*_kernel)
        DevBuf<uint64_t> tile_first_o;
        DevBuf<uint32_t> tile_cnt;
        DevBuf<unsigned char> side, side_r;
        std::vector<uint32_t> prev_act_n;  // host copy of the previous level's node sizes
        uint32_t splits_for_A = 0;         // rf.splits holds the decisions of a level of this many nodes (0: none)
        const float* targets = nullptr;    // what the batch's trees fit, by padded position: the gains, or LambdaMART's lm.target
    } rf;
    void rf_args(RFArgs& a);
    // LambdaMART gradient pass (kernels_lambda.inc)
    struct LmState {
        bool built = false;
        DevBuf<uint32_t> off, pos, qorder;  // [nq+1] / [n] positions of every query's documents in stored order / queries longest first
        DevBuf<double> lam, wt;             // [np] by padded position
        DevBuf<float> target;               // [np] float(lam): the trees' split targets
        DevBuf<unsigned char> slab;         // staging for queries too long for LDS
        uint32_t n_lds = 0, max_len = 0;    // queries (qorder[n_lds..] are staged in the slab) / the longest one
        std::vector<uint32_t> order_h, qsel_h;  // host copy of qorder / a sampled pass's queries, in qorder's order
        uint32_t sel_long = 0;                  // ... of which the slab path takes this many
        bool qsel_valid = false;                // qsel holds qsel_h (lambda_gradients' flags_unchanged)
        DevBuf<uint32_t> qsel;                  // [nq] qsel_h on the device
        DevBuf<double> asum;                    // [np] lambda_norm: every document's pair mass A_p (lambda_grad_trunc_kernel)
    } lm;
    bool lm_build(std::string* err);
    // LambdaMART's DART boosting (kernels_dart.inc): the leaf cache [rows][stride] with `filled` rows, the trees' leaf values
    // (concatenated; voff[t] = where tree t's begin, vals_h / voff_h their host copies), the weights and the tree list of the
    // last re-forming
    struct DartState {
        DevBuf<uint16_t> leaf;
        DevBuf<double> vals, w;
        DevBuf<uint32_t> voff, trees;
        DevBuf<int> bad;
        std::vector<double> vals_h, w_h;
        std::vector<uint32_t> voff_h, trees_h;
        size_t rows = 0, filled = 0, stride = 0;
    } dart;
    // LambdaMART histogram grower (kernels_hist.inc).  The bin matrix is kept for as long as the instance list, the features
    // and k stay the same (across trees and across trainings); everything else is scratch of the tree being grown.
    struct HistState {
        uint32_t k = 0, n = 0, F = 0;
        // the sample of the tree being grown (hist_sample): nt of the n instance-list entries (root: their ascending list,
        // read when q_sampled) and Ft of the F feature slots (fsel, read when f_sampled).  Without a sample nt = n, Ft = F.
        uint32_t nt = 0, Ft = 0;
        bool q_sampled = false, f_sampled = false, qof_built = false, qof_ok = false;
        DevBuf<uint32_t> qof, root, fsel, total;  // qof[n]: the query of every instance-list entry (hist_qof: once per bin matrix)
        DevBuf<uint8_t> qflag;                     // [nq]
        // GOSS (hist_goss; kernels_goss.inc): set for the tree being grown, on top of the sample above.  The tree's list is then
        // groot[ng] (full-list indices ascending), gtop[r] != 0 marks the top set, the others' gradients are multiplied by g_amp
        bool g_on = false;
        uint32_t ng = 0;
        double g_amp = 1.0;
        DevBuf<unsigned long long> gkeys;  // [nt] the keys of the sample's list, in its order
        DevBuf<uint32_t> ghist, groot;     // [GOSS_PASSES][GOSS_BINS]; [n]
        DevBuf<GossStateDev> gstate;
        DevBuf<uint8_t> gtop;              // [n] by full-list index
        // the tree's list: its length and the list itself (nullptr: 0..n-1)
        uint32_t tree_n() const { return g_on ? ng : nt; }
        const uint32_t* tree_root() const { return g_on ? groot.p : q_sampled ? root.p : nullptr; }
        std::vector<uint32_t> feats, pos_host;
        std::vector<float> edges_host;      // [F][HIST_MAX_BINS]
        std::vector<uint32_t> nedges_host;  // [F]
        DevBuf<uint32_t> pos, nedges;
        DevBuf<float> edges;
        DevBuf<uint8_t> xbin;  // [F][n]
        DevBuf<double> lam_in, wt_in;
        DevBuf<long long> Q, W;
        // quantised gradients (hist_quantq; kernels_histquant.inc): set for the tree being grown, after hist_quantise.  The
        // Newton builds then read packed[r] (by full-list index) instead of Q / W; the leaf sums still read Q / W.
        bool qz_on = false;
        DevBuf<uint32_t> packed;
        DevBuf<unsigned long long> absmax, leaf;
        DevBuf<uint32_t> idx, idx_o, flag, scan;
        DevBuf<unsigned char> temp;
        DevBuf<uint32_t> cnt, cnt_o;  // level histograms [slot][F][k]: this level's, and the next one's while it is built
        DevBuf<unsigned long long> sum, sum_o;
        DevBuf<unsigned long long> wsum, wsum_o;  // sum W per (feature, bin): the Newton gain's levels only
        // leaf-wise growth: the pool [slot][Ft][k] of pool_slots histograms (pwsum: under the Newton gain), the per-feature
        // records of the (at most two) children a step scans and their two picks
        DevBuf<uint32_t> pcnt;
        DevBuf<unsigned long long> psum, pwsum;
        uint32_t pool_slots = 0;
        DevBuf<HistPickDev> rec, pick;
        DevBuf<HistItemDev> items, items_b, nodes;  // (items: partition and leaf sums; items_b: histogram builds)
        DevBuf<HistSplitDev> splits;
        DevBuf<HistSubDev> subs;
        DevBuf<HistBestDev> best;
        DevBuf<HistBestNewtonDev> best_n;
        DevBuf<HistSymBestDev> best_sym;  // symmetric trees: one record per feature of the tree
        // monotone constraints: the signs by row of the bin matrix (mono_F of them; 0: none set for these bins), the level's intervals
        DevBuf<int> mono;
        uint32_t mono_F = 0;
        DevBuf<HistBoundsDev> bounds;
        DevBuf<HistRegNodeDev> regn;  // leaf regularisation: the level's records (interval, parent output)
        // host staging of the tables above: overwritten only after the stream was waited for
        std::vector<HistItemDev> items_h, items_bh, nodes_h;
        std::vector<HistSplitDev> splits_h;
        std::vector<HistSubDev> subs_h;
        std::vector<HistBestDev> best_h;  // (the other way: a variance level's records as fetched, before they are widened)
    } hist;
    bool hist_items(const std::vector<HistItemDev>& stretches, std::vector<HistItemDev>& host, DevBuf<HistItemDev>& dev, std::string* err);
    bool hist_qof(std::string* err);
    // histograms as (cnt, sum, wsum) arrays; wsum == nullptr: the plain gain, which keeps no third array
    void hist_build(uint32_t* cnt, unsigned long long* sum, unsigned long long* wsum);  // over hist.items_b into a level's histograms
    bool hist_zero(uint32_t* cnt, unsigned long long* sum, unsigned long long* wsum, size_t off, size_t cells, std::string* err);
    bool hist_flag_scan(uint32_t begin, uint32_t count, std::string* err);  // hist.scan = exclusive prefix sums of hist.flag over [begin, begin + count)
    bool hist_stage_nodes(const std::vector<DeviceDataset::HistNode>& nodes, bool newton, std::string* err);
    bool hist_root_build(uint32_t* cnt, unsigned long long* sum, unsigned long long* wsum, std::string* err);  // the root's index list and histogram
    bool hist_leaf_scan(const HistLeafKids& kids, uint32_t count, const DeviceDataset::HistSearch& how, DeviceDataset::HistCand* out,
                        std::string* err, const HistLeafBoundsDev* bounds = nullptr, const HistLeafRegDev* reg = nullptr);
    DevBuf<uint64_t> forest;
    DevBuf<uint32_t> tree_fdesc;  // tree_ensemble_rank_kernel: per-feature descriptors, Eytzinger threshold tables
    DevBuf<float> tree_tables;
    DevBuf<uint32_t> tree_rdesc;
    DevBuf<double> leafprod;  // w_t * leaf of every leaf of the forest (tree_ensemble_lds_kernel gathers them)
    DevBuf<uint32_t> batch_off;  // batch descriptors of the LDS tree walk
    // the forest last packed for tree_ensemble_rank_kernel (threshold tables, heap images, leaf products are a function of
    // the forest alone): scoring the same forest again -- evaluate after predict, a forest over several calls -- skips the
    // host's 3 ms of packing and the uploads.  Invalidated by any other use of the forest buffers.
    struct RankKept {
        uint64_t hash = 0;  // forest_hash of the kept forest; 0: none
        uint32_t nrounds = 0, nslots = 0, nbatch = 0;
        size_t lds = 0;
        std::vector<std::pair<uint32_t, uint32_t>> batches;  // (walks per thread, levels), for the plan of a cache hit
    } tree_rank;
    size_t scores_slots = 0;
    bool sums_only = false;  // reductions over queries return sums instead of means
    size_t last_ldm = 0, last_cols = 0;
    int host_flags = 0;
    std::shared_ptr<PermuteState> permute;
    std::mutex mu;

    bool bind(std::string* err) {
        FR_HIP(hipSetDevice(device));
        return true;
    }
    // per-query norms change rarely (once per evaluator): skip the 8 * nq byte upload when they are already there
    std::vector<double> norms_cache;
    uint64_t norms_token = 0;               // resident-sum ticket of the trainer whose norms array (norms_token_ptr) is on the device
    const double* norms_token_ptr = nullptr;
    // ... and beside them their reciprocals for the NDCG@k verify kernel's quotient (verify_end.hpp: IEEE division here, once
    // per query; NaN where the kernel must divide) -- always uploaded together, so what holds for one array holds for both
    std::vector<double> rnorms_cache;
    bool upload_norms(const double* v, std::string* err) {
        if (norms_cache.size() == nq && std::memcmp(norms_cache.data(), v, nq * sizeof(double)) == 0) return true;
        if (!rnorms.ensure(nq, err)) return false;
        norms_token = 0;  // (other contents: whatever stood for the old ones no longer does)
        norms_cache.assign(v, v + nq);
        rnorms_cache.resize(nq);
        for (size_t q = 0; q < nq; q++) rnorms_cache[q] = verify_rnorm(norms_cache[q], dcg_terms_in_range);
        FR_HIP(hipMemcpyAsync(norms.p, norms_cache.data(), nq * sizeof(double), hipMemcpyHostToDevice, stream));
        FR_HIP(hipMemcpyAsync(rnorms.p, rnorms_cache.data(), nq * sizeof(double), hipMemcpyHostToDevice, stream));
        return true;
    }
    bool pull_flags(std::string* err) {
        int v = 0;
        FR_HIP(hipMemcpyAsync(&v, flags.p, sizeof(int), hipMemcpyDeviceToHost, stream));
        FR_HIP(hipStreamSynchronize(stream));
        if (v) {
            host_flags |= v;
            FR_HIP(hipMemsetAsync(flags.p, 0, sizeof(int), stream));
        }
        return true;
    }
};

DeviceDataset::DeviceDataset() : impl_(new Impl()) {}
DeviceDataset::~DeviceDataset() {
    if (impl_) {
        (void)hipSetDevice(impl_->device);
        for (int i = 0; i < LS_CONTEXTS; i++)
            if (impl_->ls[i].stream) {
                (void)hipStreamSynchronize(impl_->ls[i].stream);
                (void)hipStreamDestroy(impl_->ls[i].stream);
            }
        if (impl_->res_ready) (void)hipEventDestroy(impl_->res_ready);
        if (impl_->stream) {
            (void)hipStreamSynchronize(impl_->stream);
            (void)hipStreamDestroy(impl_->stream);
        }
        delete impl_;
    }
}

size_t DeviceDataset::n() const { return impl_->n; }
size_t DeviceDataset::d() const { return impl_->d; }
size_t DeviceDataset::nq() const { return impl_->nq; }
bool DeviceDataset::tile_form(TileForm* out, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    FR_HIP(hipStreamSynchronize(m.stream));
    out->xb = m.xb.p;
    out->np = m.np, out->dq = m.dq, out->d = m.d, out->n = m.n;
    out->device = m.device;
    out->nonfinite = m.nonfinite;
    out->perm_host = m.perm_host.data();
    return true;
}
size_t DeviceDataset::max_query_len() const { return impl_->maxlen; }
size_t DeviceDataset::hbm_bytes() const {
    // bytes of dataset arrays this object OWNS (aliases of a parent's buffers are the parent's)
    const Impl& m = *impl_;
    auto own = [](const auto& b) { return b.borrowed ? size_t(0) : b.bytes(); };
    return own(m.xb) + own(m.gain) + own(m.gexp) + own(m.disc) + own(m.qstart) + own(m.qlen) + own(m.qtight) + own(m.perm) +
           own(m.gcls) + own(m.termtab) + own(m.xslot) + own(m.segtab) + own(m.xcol) + own(m.wt_start) + own(m.run_wt0) + own(m.wofs);
}

int DeviceDataset::take_flags() {
    std::lock_guard<std::mutex> lk(impl_->mu);
    int v = impl_->host_flags;
    impl_->host_flags = 0;
    return v;
}

#include "dataset_build.inc"
static bool launch_means(const double* M, size_t ldm, size_t ncols, size_t nq, bool sums_only, DevBuf<double>& partial,
                         DevBuf<double>& means, hipStream_t st, std::string* err, const void* tail_count = nullptr,
                         const int* tail_flags = nullptr, double* host_copy = nullptr, const uint32_t* tail_groups = nullptr) {
    // (a tick's means, redo counter and error bits reach the host only through final_mean_kernel's copy into the
    // context's page-locked block: a tick -- the callers that pass tail_count -- without that block must fail here, not
    // read stale or null memory in tick_finish; ls_means has set *err)
    if (tail_count != nullptr && host_copy == nullptr) return false;
    const size_t nseg = (nq + MEAN_SEG - 1) / MEAN_SEG;
    if (!partial.ensure(std::max<size_t>(1, nseg) * ldm, err) || !means.ensure(ldm + mean_tail_words(ldm), err)) return false;
    {
        ProfScope ps("segment_sum_kernel", st);
        dim3 grid((unsigned)nseg, (unsigned)((ncols + 63) / 64));
        segment_sum_kernel<<<grid, 64, 0, st>>>(M, (uint32_t)ldm, (uint32_t)ncols, (uint32_t)nq, partial.p);
    }
    {
        ProfScope ps("final_mean_kernel", st);
        // (the tick block's counter slot is 16 bytes, zeroed per tick: paths that count in 32 bits leave the high word 0)
        final_mean_kernel<<<dim3((unsigned)((ncols + 63) / 64)), 64, 0, st>>>(partial.p, (uint32_t)ldm, (uint32_t)ncols,
                                                                              (uint32_t)nseg, (uint32_t)(sums_only ? (nq ? 1 : 0) : nq), means.p,
                                                                              static_cast<const unsigned long long*>(tail_count), tail_flags, host_copy,
                                                                              tail_groups);
    }
    FR_HIP(hipGetLastError());
    return true;
}

static inline dim3 grid1d(size_t n, unsigned bs) { return dim3((unsigned)((n + bs - 1) / bs)); }

bool DeviceDataset::score_linear(size_t B, const double* weights, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    if (B == 0) return true;
    const size_t dp = m.dq * 4;
    if (!m.scores.ensure(B * m.np, err) || !m.weights.ensure(B * dp, err)) return false;
    m.scores_slots = B;
    std::vector<double> wpad(B * dp, 0.0);
    for (size_t b = 0; b < B; b++) std::memcpy(&wpad[b * dp], weights + b * m.d, m.d * sizeof(double));
    FR_HIP(hipMemcpyAsync(m.weights.p, wpad.data(), wpad.size() * sizeof(double), hipMemcpyHostToDevice, m.stream));
    FR_HIP(hipStreamSynchronize(m.stream));  // wpad is a local
    {
        ProfScope ps("score_linear_kernel", m.stream);
        if (B >= 8) {
            dim3 grid((unsigned)((m.pos_threads() + 255) / 256), (unsigned)((B + 7) / 8));
            score_linear_kernel<8><<<grid, 256, 0, m.stream>>>((const float4*)m.xb.p, m.posmap(), (uint32_t)m.dq,
                                                               m.weights.p, (uint32_t)B, m.scores.p);
        } else {
            dim3 grid((unsigned)((m.pos_threads() + 255) / 256), (unsigned)B);
            score_linear_kernel<1><<<grid, 256, 0, m.stream>>>((const float4*)m.xb.p, m.posmap(), (uint32_t)m.dq,
                                                               m.weights.p, (uint32_t)B, m.scores.p);
        }
    }
    FR_HIP(hipGetLastError());
    return true;
}

bool DeviceDataset::score_single_feature(uint32_t fid, double dir, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    if (!m.scores.ensure(m.np, err)) return false;
    m.scores_slots = 1;
    if (fid >= m.d) {
        // Features::get -> None -> unwrap_or(0.0) for loaded data; dir * 0.0
        fill_kernel<<<grid1d(m.pos_threads(), 256), 256, 0, m.stream>>>(m.scores.p, m.posmap(), dir * 0.0);
    } else {
        score_single_feature_kernel<<<grid1d(m.pos_threads(), 256), 256, 0, m.stream>>>(m.xb.p, m.posmap(), (uint32_t)m.dq, fid,
                                                                             dir, m.scores.p);
    }
    FR_HIP(hipGetLastError());
    return true;
}

#include "score_trees.inc"

bool DeviceDataset::ensemble_begin(std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    if (!m.acc.ensure(m.np, err)) return false;
    fill_kernel<<<grid1d(m.pos_threads(), 256), 256, 0, m.stream>>>(m.acc.p, m.posmap(), 0.0);
    FR_HIP(hipGetLastError());
    return true;
}

bool DeviceDataset::ensemble_accumulate(double w, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    axpy_unfused_kernel<<<grid1d(m.pos_threads(), 256), 256, 0, m.stream>>>(m.acc.p, m.scores.p, m.posmap(), w);
    FR_HIP(hipGetLastError());
    return true;
}

bool DeviceDataset::ensemble_finish(std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    if (!m.scores.ensure(m.np, err)) return false;
    FR_HIP(hipMemcpyAsync(m.scores.p, m.acc.p, m.np * sizeof(double), hipMemcpyDeviceToDevice, m.stream));
    m.scores_slots = 1;
    return true;
}

bool DeviceDataset::download_scores(size_t b, double* out, size_t out_len, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    if (b >= m.scores_slots) {
        if (err) *err = "score slot out of range";
        return false;
    }
    if (out_len == 0) {  // nothing wanted back: the scores stay in HBM (bench.py --measure trees times the pass itself)
        FR_HIP(hipStreamSynchronize(m.stream));
        return true;
    }
    std::vector<double> tmp(m.np);
    FR_HIP(hipMemcpyAsync(tmp.data(), m.scores.p + b * m.np, m.np * sizeof(double), hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipStreamSynchronize(m.stream));
    for (size_t p = 0; p < m.np; p++) {
        size_t id = m.perm_host[p];
        if (id != IDX_INVALID && id < out_len) out[id] = tmp[p];
    }
    return true;
}

static std::mutex g_metric_plan_mu;
static MetricPlan g_metric_plan;
static void set_metric_plan(MetricPlan&& p) {
    std::lock_guard<std::mutex> lk(g_metric_plan_mu);
    g_metric_plan = std::move(p);
}
MetricPlan last_metric_plan() {
    std::lock_guard<std::mutex> lk(g_metric_plan_mu);
    return g_metric_plan;
}

// the profile's name of one size class's launch: "metric_sort_npad<N>" / "metric_topk_npad<N>" (tools/metricbench.py prices
// the two kernels class by class with these); the names live as long as the process, as ProfScope needs
static const char* metric_class_scope(uint32_t npad, bool topk) {
    static const std::vector<std::string> names = [] {
        std::vector<std::string> v;
        for (int k = 0; k < 2; k++)
            for (uint32_t lg = 0; lg < 32; lg++) v.push_back(std::string(k ? "metric_topk_npad" : "metric_sort_npad") + std::to_string(1u << lg));
        return v;
    }();
    uint32_t lg = 0;
    while (lg < 31 && (1u << lg) < npad) lg++;
    return names[(topk ? 32 : 0) + lg].c_str();
}

bool DeviceDataset::metric_from_scores(int measure, int64_t depth, const double* norms, size_t B, bool want_rank,
                                       std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    if (B == 0 || B > m.scores_slots) {
        if (err) *err = "metric_from_scores: no scores resident";
        return false;
    }
    // size classes whose sort does not fit LDS (> 8192 documents per query) sort in global scratch
    const size_t lds_limit = 160 * 1024 - 1024;
    size_t lds = 0;
    for (const auto& sc : m.size_classes) {
        const size_t b = (size_t)sc.npad * (sizeof(double) + sizeof(uint32_t));
        if (b <= lds_limit) lds = std::max(lds, b);
    }
    if (!m.M.ensure(m.nq * B, err) || !m.norms.ensure(m.nq, err)) return false;
    if (want_rank && !m.rank.ensure(m.n, err)) return false;
    if (!m.upload_norms(norms, err)) return false;
    FR_HIP(hipStreamSynchronize(m.stream));
    FR_HIP(hipFuncSetAttribute((const void*)metric_sort_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)lds));
    int dd = depth < 0 ? -1 : (depth > 0x7fffffff ? 0x7fffffff : (int)depth);
    // The five cut-off measures at a depth of 1 .. 64 may select instead of sorting (kernels_metric_topk.inc), a size class at
    // a time where measures_host.hpp's rule says it pays; FR_METRIC_KERNEL=sort|topk forces one kernel wherever it is legal.
    const bool topk_legal = frmeasure::metric_topk_legal(measure, depth, want_rank);
    const char* force = frdev::path_env("FR_METRIC_KERNEL");
    const bool force_sort = force != nullptr && std::strcmp(force, "sort") == 0;
    const bool force_topk = force != nullptr && std::strcmp(force, "topk") == 0;
    MetricPlan plan;
    plan.measure = measure, plan.depth = depth, plan.slots = B;
    {
        ProfScope ps("metric_sort_kernel", m.stream);
        for (const auto& sc : m.size_classes) {
            const bool topk = topk_legal && !force_sort && (force_topk || frmeasure::metric_topk_pays(depth, sc.npad));
            MetricPlan::Class pc;
            pc.npad = sc.npad, pc.queries = (uint32_t)sc.count, pc.topk = topk;
            plan.classes.push_back(pc);
            std::optional<ProfScope> pcs;  // (NDCG, AP and RR are profiled exactly as before: the outer scope alone)
            if (frmeasure::is_cut_measure(measure)) pcs.emplace(metric_class_scope(sc.npad, topk), m.stream);
            if (topk) {
                dim3 grid((unsigned)((sc.count + TOPK_WAVES - 1) / TOPK_WAVES), (unsigned)B);
                metric_topk_kernel<<<grid, 64 * TOPK_WAVES, 0, m.stream>>>(m.scores.p, (uint32_t)m.np, m.qstart.p, m.qlen.p, m.gexp.p,
                                                                          m.gain.p, m.disc.p, m.norms.p, measure, (uint32_t)dd,
                                                                          (uint32_t)B, m.M.p, m.flags.p, m.qlist.p + sc.offset,
                                                                          (uint32_t)sc.count);
                continue;
            }
            const size_t cls_lds = (size_t)sc.npad * (sizeof(double) + sizeof(uint32_t));
            unsigned bs = sc.npad >= 512 ? 256 : 64;
            if (cls_lds <= lds_limit) {
                dim3 grid((unsigned)sc.count, (unsigned)B);
                metric_sort_kernel<<<grid, bs, cls_lds, m.stream>>>(m.scores.p, (uint32_t)m.np, m.qstart.p, m.qlen.p,
                                                                    m.qtight.p, m.gexp.p, m.gain.p, m.disc.p, m.norms.p,
                                                                    measure, dd, (uint32_t)B, m.M.p,
                                                                    want_rank ? m.rank.p : nullptr, m.perm.p, m.flags.p,
                                                                    sc.npad, m.qlist.p + sc.offset, 0u, nullptr, nullptr);
                continue;
            }
            // slabs of npad entries per (query, slot), at most ~1 GiB of scratch per launch
            const size_t per_slot = (size_t)sc.count * sc.npad;
            const size_t slots = std::max<size_t>(1, std::min<size_t>(B, ((size_t)1 << 30) / (per_slot * 12)));
            if (!m.sort_keys.ensure(per_slot * slots, err) || !m.sort_idx.ensure(per_slot * slots, err)) return false;
            for (size_t b0 = 0; b0 < B; b0 += slots) {
                dim3 grid((unsigned)sc.count, (unsigned)std::min(slots, B - b0));
                metric_sort_kernel<<<grid, bs, 0, m.stream>>>(m.scores.p, (uint32_t)m.np, m.qstart.p, m.qlen.p, m.qtight.p,
                                                              m.gexp.p, m.gain.p, m.disc.p, m.norms.p, measure, dd,
                                                              (uint32_t)B, m.M.p, want_rank ? m.rank.p : nullptr, m.perm.p,
                                                              m.flags.p, sc.npad, m.qlist.p + sc.offset, (uint32_t)b0,
                                                              m.sort_keys.p, m.sort_idx.p);
            }
        }
    }
    FR_HIP(hipGetLastError());
    set_metric_plan(std::move(plan));
    m.last_ldm = B;
    m.last_cols = B;
    m.last_M = m.M.p;
    return m.pull_flags(err);
}

bool DeviceDataset::download_per_query(size_t B, double* out, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    if (B != m.last_ldm) {
        if (err) *err = "download_per_query: shape mismatch";
        return false;
    }
    FR_HIP(hipMemcpyAsync(out, m.last_M, m.nq * B * sizeof(double), hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipStreamSynchronize(m.stream));
    return true;
}

bool DeviceDataset::download_last_matrix(std::vector<double>* out, size_t* ldm, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    out->resize(m.nq * m.last_ldm);
    *ldm = m.last_ldm;
    FR_HIP(hipMemcpyAsync(out->data(), m.last_M, out->size() * sizeof(double), hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipStreamSynchronize(m.stream));
    return true;
}

bool DeviceDataset::download_rank(uint32_t* out, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    if (m.rank.cap < m.n) {
        if (err) *err = "no rank order resident";
        return false;
    }
    FR_HIP(hipMemcpyAsync(out, m.rank.p, m.n * sizeof(uint32_t), hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipStreamSynchronize(m.stream));
    return true;
}

void DeviceDataset::set_sums_only(bool on) {
    std::lock_guard<std::mutex> lk(impl_->mu);
    impl_->sums_only = on;
}

bool DeviceDataset::reduce_means(size_t ncols, double* out, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    if (ncols == 0 || ncols > m.last_ldm) {
        if (err) *err = "reduce_means: shape mismatch";
        return false;
    }
    if (!launch_means(m.last_M, m.last_ldm, ncols, m.nq, m.sums_only, m.partial, m.means, m.stream, err)) return false;
    FR_HIP(hipMemcpyAsync(out, m.means.p, ncols * sizeof(double), hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipStreamSynchronize(m.stream));
    return true;
}

bool DeviceDataset::subset_means_set(const std::vector<uint32_t>& a, const std::vector<uint32_t>& b, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    m.sub_na = m.sub_nb = 0;
    auto bad = [&](const char* what) {
        if (err) *err = std::string("subset_means_set: ") + what;
        return false;
    };
    if (a.empty() || b.empty()) return bad("an empty subset");
    for (const std::vector<uint32_t>* v : {&a, &b})
        for (size_t i = 0; i < v->size(); i++)
            if ((*v)[i] >= m.nq || (i > 0 && (*v)[i] <= (*v)[i - 1])) return bad("a subset must be ascending queries of the dataset");
    std::vector<uint32_t> idx(a);
    idx.insert(idx.end(), b.begin(), b.end());
    const size_t nseg = (a.size() + MEAN_SEG - 1) / MEAN_SEG + (b.size() + MEAN_SEG - 1) / MEAN_SEG;
    if (!m.sub_partial.ensure(nseg, err) || !m.sub_means.ensure(2, err)) return false;
    FR_HIP(hipStreamSynchronize(m.stream));  // (no earlier reader of the list is in flight)
    if (!upload(m.sub_idx, idx, err)) return false;
    m.sub_na = (uint32_t)a.size(), m.sub_nb = (uint32_t)b.size();
    return true;
}

bool DeviceDataset::reduce_subset_means(double out[2], std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    if (m.sub_na == 0 || m.sub_nb == 0 || m.last_M == nullptr || m.last_ldm == 0 || m.sums_only) {
        if (err) *err = "reduce_subset_means: no subsets set, or no per-query result";
        return false;
    }
    const uint32_t nseg_a = (m.sub_na + MEAN_SEG - 1) / MEAN_SEG, nseg_b = (m.sub_nb + MEAN_SEG - 1) / MEAN_SEG;
    {
        ProfScope ps("subset_mean_kernels", m.stream);
        subset_segment_sum_kernel<<<nseg_a + nseg_b, MEAN_SEG, 0, m.stream>>>(m.last_M, (uint32_t)m.last_ldm, m.sub_idx.p, m.sub_na, m.sub_nb,
                                                                            nseg_a, m.sub_partial.p);
        subset_final_mean_kernel<<<1, 128, 0, m.stream>>>(m.sub_partial.p, nseg_a, nseg_b, m.sub_na, m.sub_nb, m.sub_means.p);
    }
    FR_HIP(hipGetLastError());
    FR_HIP(hipMemcpyAsync(out, m.sub_means.p, 2 * sizeof(double), hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipStreamSynchronize(m.stream));
    return true;
}

void DeviceDataset::subset_means_end() {
    std::lock_guard<std::mutex> lk(impl_->mu);
    impl_->sub_na = impl_->sub_nb = 0;
}

DeviceDataset::LsPath DeviceDataset::linesearch_path(int measure, int64_t depth) const {
    const Impl& m = *impl_;
    // zero-weight masking is exact only for finite features (inf * 0 = NaN)
    if (m.nonfinite || m.dq * 4 > 2048) return LS_NONE;
    if (measure == M_NDCG && depth >= 0 && depth <= 20) return LS_TOPK;
    if (frdev::path_env("FR_FORCE_GENERIC") != nullptr) return LS_NONE;
    if (m.maxlen > 2048) return LS_NONE;                                          // per-lane rank table must fit LDS (64 B per rank)
    if (measure == M_NDCG && m.termtab.cap < m.ncls * m.tablen) return LS_NONE;  // too many gain classes
    return (measure == M_NDCG || measure == M_AP || measure == M_RR) ? LS_FULLRANK : LS_NONE;
}


// ---- resident base sums and error bounds shared by the bound-and-verify paths -------------------------

bool DeviceDataset::Impl::tick_begin(LsCtx& c, const std::vector<LineGroup>& groups, std::string* err) {
    Impl& m = *this;
    TickStage& ts = c.ts;
    const size_t G = groups.size(), dp = m.dq * 4;
    ts.G = G;
    ts.dp = dp;
    size_t o = 0;
    auto take = [&o](size_t bytes) {
        const size_t at = o;
        o += (bytes + 15) & ~size_t(15);
        return at;
    };
    ts.o_count = take(sizeof(unsigned long long));  // (a 16-byte slot; zeroed with the block: entries | pairs << 32)
    ts.o_gredo = take(2 * G * sizeof(uint32_t));    // per-group redo counts, directly behind the counter slot (kernels_verify.inc relies on it; zeroed with the block), then per-group chain runs
    ts.o_gthr = take(G * sizeof(double));           // visiting order: per-group threshold on |w_c - base_f| ...
    ts.o_gmode = take(G * sizeof(uint32_t));        // ... and mode bits
    ts.o_rank = take(2 * G * sizeof(int32_t));      // resident slots (* 2 + half) whose R ranks this tick refreshes, then a staged group of each (its pending update)
    ts.o_gfeat = take(G * sizeof(uint32_t));
    ts.o_gncand = take(G * sizeof(uint32_t));
    ts.o_slot = take(G * sizeof(int32_t));
    ts.o_updf = take(G * sizeof(uint32_t));
    ts.o_gcand = take(G * 64 * sizeof(double));
    ts.o_eps2 = take(G * 64 * sizeof(double));
    ts.o_par = take(G * 6 * sizeof(double));
    ts.o_gw = take(G * dp * sizeof(double));
    ts.total = o;
    if (!c.tick_h.ensure(ts.total, err) || !c.tick_d.ensure(ts.total, err)) return false;
    if (!c.flags.p) {
        if (!c.flags.ensure(1, err)) return false;
        FR_HIP(hipMemsetAsync(c.flags.p, 0, sizeof(int), c.stream));
    }
    std::memset(c.tick_h.p, 0, ts.total);  // (the context's previous tick ended with a synchronisation: the block is free)
    uint32_t* gfeat = c.th<uint32_t>(ts.o_gfeat);
    uint32_t* gncand = c.th<uint32_t>(ts.o_gncand);
    double* gcand = c.th<double>(ts.o_gcand);
    double* gw = c.th<double>(ts.o_gw);
    for (size_t g = 0; g < G; g++) {
        const LineGroup& lg = groups[g];
        gfeat[g] = lg.feature;
        gncand[g] = (uint32_t)lg.candidates.size();
        std::memcpy(gw + g * dp, lg.weights.data(), m.d * sizeof(double));
        std::memcpy(gcand + g * 64, lg.candidates.data(), lg.candidates.size() * sizeof(double));
    }
    return true;
}

bool DeviceDataset::Impl::tick_upload(LsCtx& c, bool with_eps2, std::string* err) {
    Impl& m = *this;
    if (with_eps2) std::memcpy(c.th<double>(c.ts.o_eps2), m.eps2_host.data(), c.ts.G * 64 * sizeof(double));
    // resident sums stored from the main stream (an exact refresh) must have landed
    if (m.res_ready_set && c.stream != m.stream) FR_HIP(hipStreamWaitEvent(c.stream, m.res_ready, 0));
    FR_HIP(hipMemcpyAsync(c.tick_d.p, c.tick_h.p, c.ts.total, hipMemcpyHostToDevice, c.stream));
    return true;
}
// column means of the context's result matrix.  final_mean_kernel writes them for the host into the context's page-locked
// result block (the means, then the redo counter, the kernel error bits and, top-k, the per-group redo counts) -- no copy of
// their own brings them back
bool DeviceDataset::Impl::ls_means(LsCtx& c, std::string* err) {
    Impl& m = *this;
    const size_t ldm = c.ldm;
    if (!c.tick_res.ensure((ldm + mean_tail_words(ldm)) * sizeof(double), err)) return false;
    return launch_means(c.M.p, ldm, ldm, m.nq, m.sums_only, c.partial, c.means, c.stream, err, c.td<unsigned long long>(c.ts.o_count),
                        c.flags.p, reinterpret_cast<double*>(c.tick_res.p), c.kind == LSK_TOPK ? c.td<uint32_t>(c.ts.o_gredo) : nullptr);
}

// waits for the context's stream and hands the results over: *nredo = entries of the redo list, *npairs = the high word of
// the counter (NDCG@k: slices the exact kernel recomputed; 0 on the other paths), by_group = the per-group counts
bool DeviceDataset::Impl::tick_finish(LsCtx& c, size_t ldm, std::vector<double>* means, uint32_t* nredo, std::string* err,
                                      uint32_t* npairs, std::vector<uint32_t>* by_group) {
    Impl& m = *this;
    const size_t tail = ldm * sizeof(double);
    hipStream_t st = c.stream;
    FR_HIP(hipStreamSynchronize(st));
    means->resize(ldm);
    std::memcpy(means->data(), c.tick_res.p, tail);
    unsigned long long words[2] = {0, 0};
    std::memcpy(words, c.tick_res.p + tail, sizeof(words));
    *nredo = (uint32_t)words[0];
    if (npairs) *npairs = (uint32_t)(words[0] >> 32);
    if (by_group) {  // redo pairs of every group, then chain runs of every group
        by_group->resize(2 * (ldm / 64));
        std::memcpy(by_group->data(), c.tick_res.p + tail + 16, 2 * (ldm / 64) * sizeof(uint32_t));
    }
    const int v = (int)(unsigned int)words[1];
    if (v) {
        m.host_flags |= v;
        FR_HIP(hipMemsetAsync(c.flags.p, 0, sizeof(int), st));
        FR_HIP(hipStreamSynchronize(st));
    }
    return true;
}
// Resident sums are used when every group carries the current owner's ticket.  Writes the per-group parameters (slot * 2 +
// current half; 1/norm, base_f, pending update) into the tick block and points c.a at their device copies.
bool DeviceDataset::Impl::stage_resident(LsCtx& c, const std::vector<LineGroup>& groups, bool* any_update_out) {
    Impl& m = *this;
    const TickStage& ts = c.ts;
    LSArgs& a = c.a;
    const size_t G = groups.size();
    bool resident = G > 0, any_update = false;
    for (const LineGroup& lg : groups) {
        resident = resident && lg.resident_owner == m.res_owner && m.res_owner != 0 && lg.resident_slot >= 0 &&
                   (size_t)lg.resident_slot < m.res_half.size();
        any_update = any_update || lg.has_update;
    }
    a.res_cur = m.res.p;
    a.np = (uint32_t)m.np;
    a.rs_slot = nullptr;
    a.rs_par = nullptr;
    a.rs_updf = nullptr;
    a.xcol = m.xcol.p;
    if (resident) {
        int32_t* rs_slot = c.th<int32_t>(ts.o_slot);
        double* rs_par = c.th<double>(ts.o_par);
        uint32_t* rs_updf = c.th<uint32_t>(ts.o_updf);
        for (size_t g = 0; g < G; g++) {
            const LineGroup& lg = groups[g];
            rs_slot[g] = (int32_t)(lg.resident_slot * 2 + m.res_half[lg.resident_slot]);
            rs_par[g * 6 + 0] = 1.0 / lg.resident_norm;
            rs_par[g * 6 + 1] = lg.resident_base_f;
            rs_par[g * 6 + 2] = lg.has_update ? 1.0 : 0.0;
            rs_par[g * 6 + 3] = 1.0 / lg.upd_norm;
            rs_par[g * 6 + 4] = lg.upd_base_f;
            rs_par[g * 6 + 5] = lg.upd_cand;
            rs_updf[g] = lg.upd_feature;
        }
        a.rs_slot = c.td<int32_t>(ts.o_slot);
        a.rs_par = c.td<double>(ts.o_par);
        a.rs_updf = c.td<uint32_t>(ts.o_updf);
    }
    *any_update_out = any_update;
    return resident;
}

// m.eps2_host[g*64 + c] = 2 * eps_c, where eps_c bounds |approximate key - reference score| for every document
// (DESIGN.md section 4.2): both lie within gamma_(D+1) * T of the real-number sum, T = sum_j |x_j w_j| <=
// sum_{j != f} |w_j| X_j + |w_c| X_f with X_j the column max |x|; 2.5 (D + 1) u T (u = 2^-53) covers both sides
// and the rounding of the products, 2^cls_bits ulp the gain class written over the lowest mantissa bits (of the key,
// and of x_f: kernels_verify.inc).
// Returns false when the bound is unusable (absurd or non-finite weights: keys could overflow).
bool DeviceDataset::Impl::compute_eps2(const std::vector<LineGroup>& groups, bool resident, uint32_t cls_bits, bool bare_admission, bool key_relative) {
    Impl& m = *this;
    const size_t G = groups.size();
    std::vector<double>& eps2 = m.eps2_host;
    eps2.assign(G * 64, 0.0);
    // (the class rides in the lowest mantissa bits of the f64 x_f word as well -- the low 29 bits of a converted f32 are
    // zero -- so the product x_f * w_c carries a second relative error of 2^(cls_bits - 52))
    // (bare_admission -- the NDCG@k verify kernel -- adds a third 2^(cls_bits - 52): it admits a document on the sum BEFORE
    // the class / duplicate-group bits go in, so a document turned away may have a key up to 2^cls_bits ulp above the
    // threshold it was compared with)
    // The factor on u = 2^-53.  Sums formed from the tiles: the reference's sequentially rounded sum of rounded products is within
    // ~D u T of the real-number sum and so is the kernel's FMA chain: 2.5 (D + 1) covers both.  Resident sums of the NDCG@k
    // verify kernel (key_relative): the kernel's own arithmetic is ONE rounding, key = fl(x_f w_c + A), and everything about A
    // -- the drift of R, the reciprocal, the rounded normalised weights, the base_f term -- is in `extra`; what is left for
    // this factor is the reference's side, (gamma_(D-1) (1 + u) + u) <= D u (1 + tiny), plus that one rounding: D + 2.
    const double dfac = (key_relative && resident) ? (double)(m.d + 2) : 2.5 * (double)(m.d + 1);
    const double gamma = (dfac * std::ldexp(1.0, -53) + (bare_admission ? 3.0 : 2.0) * std::ldexp(1.0, (int)cls_bits - 52)) * (1.0 + 1e-6);
    bool ok = true;
    for (size_t g = 0; g < G; g++) {
        const LineGroup& lg = groups[g];
        double T = 0.0;
        for (size_t j = 0; j < m.d; j++)
            if (j != lg.feature) T += std::fabs(lg.weights[j]) * m.colmax[j];
        // resident form A = R/norm - x_f*base_f: the subtracted term joins T, the reciprocal, the product
        // and the two extra roundings are covered by 10 u T, and R's own drift enters as resident_err / norm
        double extra = 0.0;
        if (resident) {
            T += std::fabs(lg.resident_base_f) * m.colmax[lg.feature];
            extra = resident_eps_extra(lg.resident_err, lg.resident_norm, T);
            if (!(lg.resident_norm > 0.0) || !(extra < 1e290)) ok = false;
        }
        for (size_t c = 0; c < lg.candidates.size(); c++) {
            const double Tc = T + std::fabs(lg.candidates[c]) * m.colmax[lg.feature];
            if (!(Tc < 1e290)) ok = false;
            // absolute floor: with T = 0 (all weight on all-zero columns) every true score is 0 and the keys differ only
            // by the class bits (subnormal numbers, also through x_f = 0 carrying its class, times |w_c|): never a
            // proven order
            const double floor_abs = 1e-300 + std::fabs(lg.candidates[c]) * std::ldexp(1.0, (int)cls_bits - 1070);
            // key_relative: the candidate's own term is bounded through the key, |x_f w_c| = |S - S_A| <= |key| + |key - S| + T
            // (T >= |S_A| by the column maxima of the OTHER features), so a key's bound is gamma (2 T + |key|) + extra + floor
            // and a pair's is the sum of two: the part that does not depend on the keys is staged here, gamma goes to the kernel
            eps2[g * 64 + c] = key_relative ? 2.0 * (gamma * 2.0 * T + extra + floor_abs) : 2.0 * (gamma * Tc + extra + floor_abs);
        }
    }
    m.eps_gamma = gamma;
    return ok;
}

// the pending updates of staged groups [g_base, g_base + ng) where no verify kernel applies them
bool DeviceDataset::Impl::update_resident(LsCtx& c, size_t g_base, size_t ng, std::string* err) {
    Impl& m = *this;
    LSArgs x = c.a;
    x.g_base = (uint32_t)g_base;
    x.posmap = m.posmap();
    {
        ProfScope ps("resident_update_kernel", c.stream);
        resident_update_kernel<<<dim3((unsigned)((m.pos_threads() + 255) / 256), (unsigned)ng), 256, 0, c.stream>>>(x);
    }
    FR_HIP(hipGetLastError());
    return true;
}


// after a launch that applied the pending updates: the updated sums are in the other half of their slot
void DeviceDataset::Impl::flip_resident(const std::vector<LineGroup>& groups) {
    Impl& m = *this;
    std::vector<char> flipped(m.res_half.size(), 0);
    for (const LineGroup& lg : groups)
        if (lg.has_update && !flipped[lg.resident_slot]) {
            m.res_half[lg.resident_slot] ^= 1;
            flipped[lg.resident_slot] = 1;
        }
}

template <int K, int CT>
static void launch_linesearch(const LSArgs& a, unsigned nblocks, size_t lds, hipStream_t st) {
    linesearch_ndcg_kernel<K, CT, 16><<<dim3(nblocks), dim3(WAVE), lds, st>>>(a);
}

template <int K>
static void dispatch_ct(const LSArgs& a, unsigned nblocks, size_t maxc, size_t lds, hipStream_t st) {
    if (maxc <= 4) launch_linesearch<K, 4>(a, nblocks, lds, st);
    else if (maxc <= 16) launch_linesearch<K, 16>(a, nblocks, lds, st);
    else if (maxc <= 32) launch_linesearch<K, 32>(a, nblocks, lds, st);
    else if (maxc <= 51) launch_linesearch<K, 51>(a, nblocks, lds, st);
    else launch_linesearch<K, 64>(a, nblocks, lds, st);
}

// the exact kernel: every (run, group) pair of groups [a.g_base, a.g_base + a.G) -- nblocks blocks -- or, a.work_list set,
// nblocks listed (query, group) entries with four blocks each, one per 16-candidate slice
static void dispatch_exact(const LSArgs& a, int64_t depth, unsigned nblocks, size_t maxc, size_t lds, hipStream_t st) {
    if (a.work_list != nullptr) {
        maxc = std::min<size_t>(maxc, 16);
        nblocks *= 4;
    }
    if (depth <= 5) dispatch_ct<5>(a, nblocks, maxc, lds, st);
    else if (depth <= 10) dispatch_ct<10>(a, nblocks, maxc, lds, st);
    else dispatch_ct<20>(a, nblocks, maxc, lds, st);
}

// pairs of the verify kernel's redo list the exact kernel takes in its first, fixed-size launch (blocks past the
// device-side count return at once: ~10 us when the list is short); FR_REDO_GRID pins it (tests)
static unsigned redo_grid_env() {
    const char* e = frdev::path_env("FR_REDO_GRID");
    return e ? (unsigned)std::min<long>(std::max<long>(std::atol(e), 64), 1 << 20) : 0u;
}

template <int K>
static void launch_verify(const LSArgs& a, bool resident, bool dupk, int xs, unsigned nruns8, size_t G, size_t dp, size_t tab_lds_kt, hipStream_t st) {
    // the kernel's copy of the DCG term table has K + 1 rows (the host's bound is for LS_KT + 1).  It matters: gfx950 hands out
    // LDS in granules of 1280 bytes, and the resident variants' two staged copies of a walk tile (4224 bytes) plus 21 rows of
    // six classes (1008 bytes) are 112 bytes over four granules -- 25 blocks per CU instead of the 28 the launch bounds ask for
    const size_t tab_lds = tab_lds_kt / (LS_KT + 1) * (K + 1);
    if (resident) {
        const dim3 grid((unsigned)(nruns8 * G));
        if (dupk) {
            if (xs <= 1) linesearch_verify_kernel<K, 1, true, 1, true><<<grid, dim3(WAVE), tab_lds, st>>>(a);
            else if (xs == 2) linesearch_verify_kernel<K, 1, true, 2, true><<<grid, dim3(WAVE), tab_lds, st>>>(a);
            else if (xs == 3 || K < 10) linesearch_verify_kernel<K, 1, true, 3, true><<<grid, dim3(WAVE), tab_lds, st>>>(a);
            else linesearch_verify_kernel<K, 1, true, (K < 10 ? 3 : 4), true><<<grid, dim3(WAVE), tab_lds, st>>>(a);
        } else if (xs <= 1) linesearch_verify_kernel<K, 1, true><<<grid, dim3(WAVE), tab_lds, st>>>(a);
        else if (xs == 2) linesearch_verify_kernel<K, 1, true, 2><<<grid, dim3(WAVE), tab_lds, st>>>(a);
        else if (xs == 3 || K < 10) linesearch_verify_kernel<K, 1, true, 3><<<grid, dim3(WAVE), tab_lds, st>>>(a);
        else linesearch_verify_kernel<K, 1, true, (K < 10 ? 3 : 4)><<<grid, dim3(WAVE), tab_lds, st>>>(a);  // (depth <= 5: K + 3 keys at most)
    } else {
        // sums from the tiles: two groups per wave share the tile loads
        const dim3 grid((unsigned)(nruns8 * ((G + 1) / 2)));
        linesearch_verify_kernel<K, 2, false><<<grid, dim3(WAVE), 2 * dp * sizeof(double) + tab_lds, st>>>(a);
    }
}

uint64_t DeviceDataset::resident_reserve(size_t slots, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return 0;
    m.res_owner++;  // whoever held the buffers before loses them, even if the allocation below fails
    // (how many keys beyond K the lists need is mostly a property of the DATA -- duplicated rows, quantised columns -- so a new
    // trainer starts one below what the last one on this dataset ended with instead of paying the whole ramp again: on the
    // tie kinds the first ticks at K + 1 send most of their pairs to the exact kernel)
    m.verify_xs = std::max(1, m.verify_xs - 1);
    m.res_half.clear();
    if (m.xcol.p == nullptr) {  // (FR_XCOL=0 or no HBM for it: the resident kernels read their column there -- the caller forms the sums from the tiles)
        if (err) *err = "resident_reserve: the dataset has no column-major copy";
        return 0;
    }
    m.pol.reset(slots);
    {
        std::string* e2 = err;
        auto ensure = [&]() -> bool { return m.res.ensure(slots * 2 * m.np, e2); };
        if (!ensure()) return 0;
    }
    m.res_half.assign(slots, 0);
    if (m.xslot.p != nullptr) {
        std::string e2;
        if (m.rslot.ensure(slots * m.np, &e2)) {
            rslot_identity_kernel<<<dim3(1024), dim3(256), 0, m.stream>>>(m.rslot.p, m.wofs.p, m.np, slots * m.np);
            if (hipGetLastError() != hipSuccess) m.rslot.release();
        } else {
            (void)hipGetLastError();  // (no HBM for the tables: storage order)
        }
    }
    return m.res_owner;
}

bool DeviceDataset::resident_store_from_scores(uint64_t owner, size_t slot, size_t b, std::string* err, const double* v) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (err) err->clear();
    if (owner != m.res_owner) return false;
    if (!m.bind(err)) return false;
    if (slot >= m.res_half.size() || b >= m.scores_slots) {
        if (err) *err = "resident_store_from_scores: slot out of range";
        return false;
    }
    FR_HIP(hipMemcpyAsync(m.res.p + (slot * 2 + m.res_half[slot]) * m.np, m.scores.p + b * m.np, m.np * sizeof(double),
                          hipMemcpyDeviceToDevice, m.stream));
    FR_HIP(hipEventRecord(m.res_ready, m.stream));
    m.res_ready_set = true;
    m.pol.new_sums(slot);
    if (m.cap_on) {
        LsCapture e;
        e.store = true;
        e.slot = (int)slot;
        if (v) e.v.assign(v, v + m.d);
        m.cap_log.push_back(std::move(e));
    }
    return true;
}

void DeviceDataset::capture_enable(bool on) {
    std::lock_guard<std::mutex> lk(impl_->mu);
    impl_->cap_on = on;
    if (!on) impl_->cap_log.clear();
    for (Impl::LsCtx& c : impl_->ls) std::vector<LineGroup>().swap(c.cgroups);  // (a line search in flight across the switch is not logged)
}

void DeviceDataset::capture_note_store(size_t slot, const double* v) {
    std::lock_guard<std::mutex> lk(impl_->mu);
    if (!impl_->cap_on) return;
    LsCapture e;
    e.store = true;
    e.slot = (int)slot;
    e.v.assign(v, v + impl_->d);
    impl_->cap_log.push_back(std::move(e));
}

void DeviceDataset::capture_take(std::vector<LsCapture>* out) {
    std::lock_guard<std::mutex> lk(impl_->mu);
    out->clear();
    out->swap(impl_->cap_log);
}

const std::vector<double>& DeviceDataset::column_absmax() const { return impl_->colmax; }

void DeviceDataset::audit_counters(unsigned long long* values, unsigned long long* mismatches) const {
    std::lock_guard<std::mutex> lk(impl_->mu);
    *values = impl_->audit_values;
    *mismatches = impl_->audit_mismatches;
}

unsigned long long DeviceDataset::exact_fallbacks() const {
    std::lock_guard<std::mutex> lk(impl_->mu);
    return impl_->exact_fallbacks;
}

void DeviceDataset::chain_counters(unsigned long long* runs, unsigned long long* visits, unsigned long long* ranked_on,
                                   unsigned long long* ranked_off) const {
    std::lock_guard<std::mutex> lk(impl_->mu);
    *runs = impl_->chain_runs;
    *visits = impl_->chain_visits;
    if (ranked_on) *ranked_on = impl_->pol.rank_slots_on;
    if (ranked_off) *ranked_off = impl_->pol.rank_slots_off;
}

void DeviceDataset::routing_counters(unsigned long long* exact_groups, unsigned long long* redo_entries) const {
    std::lock_guard<std::mutex> lk(impl_->mu);
    *exact_groups = impl_->pol.exact_groups;
    *redo_entries = impl_->approx_redo_entries;
}

static void launch_scores(const FSArgs& a, size_t maxc, unsigned nblocks, size_t lds, hipStream_t st) {
    if (maxc <= 16) linesearch_scores_kernel<16, 16><<<dim3(nblocks), dim3(WAVE), lds, st>>>(a);
    else if (maxc <= 51) linesearch_scores_kernel<51, 16><<<dim3(nblocks), dim3(WAVE), lds, st>>>(a);
    else linesearch_scores_kernel<64, 16><<<dim3(nblocks), dim3(WAVE), lds, st>>>(a);
}

// arguments of the exact full-ranking kernels (kernels_fullrank.inc): the chunked evaluation's, and the redo list's of the
// full-ranking verify kernel (work-list mode)
FSArgs DeviceDataset::Impl::scores_args(const uint32_t* gf, const double* w, const double* cand, double* rows, int* fl, size_t gc) const {
    FSArgs a{};
    a.xb = (const float4*)xb.p;
    a.run_pos = run_pos.p;
    a.run_docs = run_docs.p;
    a.run_order = run_order.p;
    a.gfeat = gf;
    a.gw = w;
    a.gcand = cand;
    a.rows = rows;
    a.flags = fl;
    a.dq = (uint32_t)dq;
    a.d = (uint32_t)d;
    a.nruns = (uint32_t)nruns;
    a.GC = (uint32_t)gc;
    a.np = (uint32_t)np;
    return a;
}

RMArgs DeviceDataset::Impl::rank_args(const double* rows, const uint32_t* gnc, double* out, int* fl, size_t gc, size_t ldm, int measure,
                                      int64_t depth) const {
    RMArgs a{};
    a.rows = rows;
    a.qstart = qstart.p;
    a.qlen = qlen.p;
    a.qnpos = qnpos.p;
    a.qnneg = qnneg.p;
    a.gcls = gcls.p;
    a.termtab = termtab.p;
    a.norms = norms.p;
    a.gncand = gnc;
    a.M = out;
    a.flags = fl;
    a.GC = (uint32_t)gc;
    a.np = (uint32_t)np;
    a.ldm = (uint32_t)ldm;
    a.tablen = (uint32_t)tablen;
    a.measure = measure;
    a.depth = depth < 0 ? -1 : (depth > 0x7fffffff ? 0x7fffffff : (int)depth);
    return a;
}

// arguments of the three verify kernels of a line search whose groups are staged in the context's tick block (tick_begin,
// stage_resident).  NDCG@k: into c.a, next to stage_resident's resident parameters; what depends on the bound and the
// routing (gamma, the visiting order, eps2, the verify launch's G) is set by submit_topk
void DeviceDataset::Impl::topk_args(LsCtx& c, size_t G) const {
    const Impl& m = *this;
    const TickStage& ts = c.ts;
    LSArgs& a = c.a;
    a.xb = (const float4*)m.xb.p;
    a.gcls = m.gcls.p;
    a.dcgtab = m.dcgtab.p;
    a.qstart = m.qstart.p;
    a.qlen = m.qlen.p;
    a.run_q0 = m.run_q0.p;
    a.run_q1 = m.run_q1.p;
    a.run_pos = m.run_pos.p;
    a.run_lo = m.run_lo.p;
    a.run_docs = m.run_docs.p;
    a.run_order = m.run_order.p;
    a.wt_start = m.wt_start.p;
    a.run_wt0 = m.run_wt0.p;
    a.norms = m.norms.p;
    a.rnorms = m.rnorms.p;
    a.disc = m.disc.p;
    a.gfeat = c.td<uint32_t>(ts.o_gfeat);
    a.gw = c.td<double>(ts.o_gw);
    a.gcand = c.td<double>(ts.o_gcand);
    a.gncand = c.td<uint32_t>(ts.o_gncand);
    a.M = c.M.p;
    a.flags = c.flags.p;
    a.dbg_counters = m.dbgc.p;
    a.dq = (uint32_t)m.dq;
    a.d = (uint32_t)m.d;
    a.nruns = (uint32_t)m.nruns;
    a.G = (uint32_t)G;
    a.ldm = (uint32_t)c.ldm;
    a.depth = (int)c.depth;
    a.ncls = (uint32_t)m.ncls;
    a.redo_count = c.td<unsigned long long>(ts.o_count);
    a.redo_list = c.redo.p;
    a.chain_count = c.td<uint32_t>(ts.o_gredo) + G;
    a.cls_mask = (1u << m.key_bits) - 1u;  // class bits + duplicate-group bits ride in the keys' low mantissa
    a.cls_only_mask = (1u << m.key_cls_bits) - 1u;
    a.gkey = m.gkey.p;
}

RRArgs DeviceDataset::Impl::rr_args(LsCtx& c, size_t G) const {
    const Impl& m = *this;
    const TickStage& ts = c.ts;
    const LSArgs& a = c.a;
    RRArgs ra{};
    ra.xb = (const float4*)m.xb.p;
    ra.qstart = m.qstart.p;
    ra.qlen = m.qlen.p;
    ra.qnpos = m.qnpos.p;
    ra.gfeat = c.td<uint32_t>(ts.o_gfeat);
    ra.gw = c.td<double>(ts.o_gw);
    ra.gcand = c.td<double>(ts.o_gcand);
    ra.gncand = c.td<uint32_t>(ts.o_gncand);
    ra.eps2 = c.td<double>(ts.o_eps2);
    ra.redo_count = c.td<uint32_t>(ts.o_count);
    ra.redo_list = c.redo.p;
    ra.res_cur = m.res.p;
    ra.rs_slot = a.rs_slot;
    ra.rs_par = a.rs_par;
    ra.rs_updf = a.rs_updf;
    ra.xcol = a.xcol;
    ra.M = c.M.p;
    ra.flags = c.flags.p;
    ra.G = (uint32_t)G;
    ra.ldm = (uint32_t)c.ldm;
    ra.dq = (uint32_t)m.dq;
    ra.d = (uint32_t)m.d;
    ra.np = (uint32_t)m.np;
    return ra;
}

// (cls_bits / dup_bits: low key bits of the gain class / duplicate group)
FVArgs DeviceDataset::Impl::fv_args(LsCtx& c, size_t G, uint32_t cls_bits, uint32_t dup_bits) const {
    const Impl& m = *this;
    const TickStage& ts = c.ts;
    const LSArgs& a = c.a;
    FVArgs fa{};
    fa.xb = (const float4*)m.xb.p;
    fa.qstart = m.qstart.p;
    fa.qlen = m.qlen.p;
    fa.qnpos = m.qnpos.p;
    fa.gcls = m.gcls.p;
    fa.gfeat = c.td<uint32_t>(ts.o_gfeat);
    fa.gw = c.td<double>(ts.o_gw);
    fa.gcand = c.td<double>(ts.o_gcand);
    fa.gncand = c.td<uint32_t>(ts.o_gncand);
    fa.eps2 = c.td<double>(ts.o_eps2);
    fa.termtab = m.termtab.p;
    fa.norms = m.norms.p;
    fa.redo_count = c.td<uint32_t>(ts.o_count);
    fa.redo_list = c.redo.p;
    fa.res_cur = m.res.p;
    fa.rs_slot = a.rs_slot;
    fa.rs_par = a.rs_par;
    fa.rs_updf = a.rs_updf;
    fa.M = c.M.p;
    fa.flags = c.flags.p;
    fa.relmask = m.relmask;
    fa.G = (uint32_t)G;
    fa.ldm = (uint32_t)c.ldm;
    fa.dq = (uint32_t)m.dq;
    fa.d = (uint32_t)m.d;
    fa.np = (uint32_t)m.np;
    fa.tablen = (uint32_t)m.tablen;
    fa.cls_mask = (1u << (cls_bits + dup_bits)) - 1u;
    fa.cls_only_mask = (1u << cls_bits) - 1u;
    fa.cls_bits = cls_bits;
    fa.key_cls_bits = m.key_cls_bits;
    fa.dup = dup_bits ? 1u : 0u;
    fa.gkey = m.gkey.p;
    fa.padcls = (uint32_t)m.ncls;
    fa.measure = c.measure;
    fa.depth = c.depth < 0 ? -1 : (c.depth > 0x7fffffff ? 0x7fffffff : (int)c.depth);
    return fa;
}

// ---- NDCG of any depth / AP by bound-and-verify (kernels_fullverify.inc) -------------------------------------

// (query, group) pairs of the redo list the exact kernels take per launch: each block owns one slot of score rows
static constexpr unsigned FV_REDO_GRID = 1024;

// One size class: workgroups of FV_BLOCK_WAVES waves, each walking a slice of the class's queries for one line group
// in batches of qb queries (kernels_fullverify.inc).  qb is chosen so that qb * ncand candidates fill whole sorting
// passes of the workgroup (5 queries x 51 candidates = 255 of 256 lanes) within the LDS that lets the class's
// waves-per-SIMD be resident; the grid is a few resident rounds of the chip, so that slices balance.
bool fv_launch_part0(int, int, bool, const FVArgs&, dim3, size_t, hipStream_t);
bool fv_launch_part1(int, int, bool, const FVArgs&, dim3, size_t, hipStream_t);
bool fv_launch_part2(int, int, bool, const FVArgs&, dim3, size_t, hipStream_t);
bool fv_launch_part3(int, int, bool, const FVArgs&, dim3, size_t, hipStream_t);
bool fv_launch_part4(int, int, bool, const FVArgs&, dim3, size_t, hipStream_t);
bool fv_launch_part5(int, int, bool, const FVArgs&, dim3, size_t, hipStream_t);
bool fv_launch_part6(int, int, bool, const FVArgs&, dim3, size_t, hipStream_t);
bool fv_launch_part7(int, int, bool, const FVArgs&, dim3, size_t, hipStream_t);
bool fv_launch(int ci, int mode, bool tablds, const FVArgs& a, dim3 grid, size_t lds, hipStream_t st) {
    static_assert(FV_PARTS == 8, "one declaration per part");
    switch (ci % FV_PARTS) {
        case 0: return fv_launch_part0(ci, mode, tablds, a, grid, lds, st);
        case 1: return fv_launch_part1(ci, mode, tablds, a, grid, lds, st);
        case 2: return fv_launch_part2(ci, mode, tablds, a, grid, lds, st);
        case 3: return fv_launch_part3(ci, mode, tablds, a, grid, lds, st);
        case 4: return fv_launch_part4(ci, mode, tablds, a, grid, lds, st);
        case 5: return fv_launch_part5(ci, mode, tablds, a, grid, lds, st);
        case 6: return fv_launch_part6(ci, mode, tablds, a, grid, lds, st);
        default: return fv_launch_part7(ci, mode, tablds, a, grid, lds, st);
    }
}

static constexpr size_t FV_LDS_PER_CU = size_t(160) << 10;
static constexpr uint32_t FV_NREC_MAX = 384;  // query records a workgroup keeps in LDS (24 bytes each)

static bool fv_launch_class(FVArgs a, int ci, unsigned nqueries, unsigned G, unsigned maxc, hipStream_t st) {
    const uint32_t nl = FV_CLASSES[ci].nl, pl = FV_CLASSES[ci].pl, npad = nl * pl;
    const uint32_t slots = (uint32_t)FV_BLOCK_WAVES * (64u / pl);  // candidates per sorting pass
    const unsigned wps = (unsigned)fv_waves_per_simd((int)nl);
    const int mode = a.measure == M_AP ? FV_AP : (a.depth >= 0 ? FV_NDCG_CUT : FV_NDCG);
    // the metric's table in LDS: AP's rank / reciprocal arrays always; the class's slice of the DCG term table when it is
    // small (5 gain classes: 12 KB at 256 documents)
    size_t tab = 0;
    bool tablds = false;
    if (mode == FV_AP) {
        tab = (size_t)npad * 2;
    } else if (mode == FV_NDCG && fv_has_tablds(ci)) {
        const size_t t = (size_t)(a.padcls + 1) * (npad + 1);
        if (t * sizeof(double) <= (size_t(40) << 10)) tab = t, tablds = true;
    }
    // queries per batch: the best lane utilisation that fits the workgroup's share of the LDS (smallest such qb); with
    // one word buffer instead of two when that buys more than 4 % of the lanes (long classes: many passes per batch,
    // the un-overlapped phase 1 is small against them)
    const size_t budget = FV_LDS_PER_CU / wps - 1024;
    auto pick = [&](bool dbuf, uint32_t* qb_out) {
        double best_u = 0.0;
        *qb_out = 1;
        for (uint32_t cand = 1; cand <= 64; cand++) {
            if (fv_lds_bytes(nl, pl, cand, std::min<uint32_t>(FV_NREC_MAX, cand * 8), tab, dbuf) > budget) break;
            const uint32_t items = cand * std::max(1u, maxc);
            const double u = (double)items / (double)(((items + slots - 1) / slots) * slots);
            if (u > best_u + 0.015) best_u = u, *qb_out = cand;
        }
        return best_u;
    };
    uint32_t qb = 1, qb1 = 1;
    const double u2 = pick(true, &qb), u1 = pick(false, &qb1);
    bool dbuf = true;
    if (u1 > u2 + 0.04) dbuf = false, qb = qb1;
    // a short class needs its batches more as parallel work than as full lanes: at least two rounds of resident workgroups
    qb = std::min<uint32_t>(qb, std::max<uint32_t>(1u, (uint32_t)(((uint64_t)nqueries * G) / (2u * 256u * wps))));
    qb = std::min<uint32_t>(qb, std::max(1u, nqueries));
    const uint32_t nbatches = (nqueries + qb - 1) / qb;
    const unsigned resident_blocks = 256u * wps;
    unsigned nbx = std::max(1u, (4u * resident_blocks + G - 1) / G);
    nbx = std::min<unsigned>(nbx, nbatches);
    const uint32_t max_batches = std::max(1u, FV_NREC_MAX / qb);  // per block, so that its records fit
    nbx = std::max<unsigned>(nbx, (nbatches + max_batches - 1) / max_batches);
    a.nqc = nqueries;
    a.qb = qb;
    a.nrec = qb * ((nbatches + nbx - 1) / nbx);
    a.dbuf = dbuf ? 1u : 0u;
    const size_t lds = fv_lds_bytes(nl, pl, qb, a.nrec, tab, dbuf);
    return fv_launch(ci, mode, tablds, a, dim3(nbx, G), lds, st);
}

#ifndef FV_REDO_WAVES
#define FV_REDO_WAVES 4  // waves per redone (query, group); 8 measured the same (tools/ab/rf_md.sh)
#endif
// The exact kernels on n entries of the context's redo list from entry `off` on.  count_dev: the device-side count of the
// list, which the blocks of the fixed-size first launch compare themselves with (the host does not wait for it); nullptr
// for the rest of a long list.
bool DeviceDataset::Impl::redo_launch(LsCtx& c, uint32_t off, const uint32_t* count_dev, uint32_t n, std::string* err) {
    Impl& m = *this;
    switch (c.kind) {
        case LSK_TOPK: {
            c.a.work_list = c.redo.p + off;
            c.a.work_count = count_dev;
            ProfScope ps("linesearch_ndcg_kernel", c.stream);
            dispatch_exact(c.a, c.depth, n, c.maxc, c.lds, c.stream);
            break;
        }
        case LSK_RR: {
            c.ra.work_list = c.redo.p + off;
            c.ra.work_count = count_dev;
            ProfScope ps("rr_exact_kernel", c.stream);
            rr_exact_kernel<<<dim3(n), WAVE, m.d * sizeof(double), c.stream>>>(c.ra);
            break;
        }
        case LSK_FV:  // the scores kernel, then the rank-counting kernel; a block owns one slot of score rows: FV_REDO_GRID at a time
            for (uint32_t k = 0; k < n; k += FV_REDO_GRID) {
                const uint32_t nb = std::min(FV_REDO_GRID, n - k);
                FSArgs fs = c.fsa;
                fs.work_list = c.redo.p + off + k;
                fs.work_count = count_dev;
                RMArgs rm = c.rma;
                rm.work_list = fs.work_list;
                rm.work_count = count_dev;
                {
                    ProfScope ps("linesearch_scores_kernel", c.stream);
                    launch_scores(fs, c.maxc, nb, 2 * m.dq * 4 * sizeof(double), c.stream);
                }
                FR_HIP(hipGetLastError());
                ProfScope ps("rank_metric_kernel", c.stream);
                FR_HIP(hipFuncSetAttribute((const void*)rank_metric_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
                const size_t npad_max = m.size_classes.empty() ? 64 : m.size_classes.back().npad;
                rank_metric_kernel<<<dim3(nb), WAVE * FV_REDO_WAVES, npad_max * 64, c.stream>>>(rm);
            }
            break;
    }
    FR_HIP(hipGetLastError());
    return true;
}

// ---- the line-search driver ----------------------------------------------------------------------------------------
// submit: validate, stage the groups and their resident parameters in the tick block, bound the error, then queue the verify
// kernel and a fixed-size first launch of the exact kernels on its redo list -- or, where bound-and-verify does not apply,
// the exact kernels alone.  collect: wait, finish a long redo list, count, and set the policies that steer the next line
// searches.  ls_submit is the prologue the three verify kernels share -- validation, the groups the policy routes, staging --
// and hands over to the launcher of the line search's kind (submit_topk / submit_rr / submit_fv: bound, fallback decision,
// launch, redo launch); the policies themselves are in linesearch_policy.hpp.

static constexpr unsigned RR_REDO_GRID = 8192;  // reciprocal rank: redo-list pairs the exact kernel's first launch takes

bool DeviceDataset::Impl::ls_submit(LsCtx& c, int path, int measure, int64_t depth, const double* norms,
                                    const std::vector<LineGroup>& groups_in, std::string* err) {
    Impl& m = *this;
    if (path == LS_NONE) {
        if (err) *err = "linesearch: unsupported measure, depth or dataset (the general sort evaluator takes it)";
        return false;
    }
    const size_t G = groups_in.size();
    size_t maxc = 0;
    for (const LineGroup& lg : groups_in) {
        if (lg.feature >= m.d || lg.weights.size() != m.d || lg.candidates.empty() || lg.candidates.size() > 64) {
            if (err) *err = "linesearch: malformed line group";
            return false;
        }
        maxc = std::max(maxc, lg.candidates.size());
    }
    if (&c == &m.ls[LS_CONTEXTS]) c.stream = m.stream;
    c.kind = path == LS_TOPK ? LSK_TOPK : (measure == M_RR ? LSK_RR : LSK_FV);
    c.ldm = G * 64;
    c.maxc = maxc;
    c.depth = depth;
    c.measure = measure;
    c.approx = c.ready = false;
    c.resident = c.dup = false;
    c.kbucket = 0;
    c.nverify = 0;
    c.gorder.clear();
    c.counts = LsCounts{};
    if (m.cap_on) c.cgroups = groups_in;
    if (G == 0) {
        c.pending = true;
        return true;
    }
    const bool topk = c.kind == LSK_TOPK;
    if (topk) {
        if (m.nq * G >= (size_t(1) << 28)) {  // (a redo entry is (q * G + g) * 16 + slice mask in 32 bits; M itself would be > 130 GB)
            if (err) *err = "linesearch: too many (query, group) pairs for one launch";
            return false;
        }
        if (!c.M.ensure(m.nq * c.ldm, err) || !c.redo.ensure(m.nq * G, err)) return false;
    }
    // FR_LS_EXACT=1: the exact kernels only
    const bool exact_only = std::getenv("FR_LS_EXACT") != nullptr;
    c.audit = std::getenv("FR_VERIFY_AUDIT") != nullptr;
    bool can_verify = !exact_only && m.colmax.size() == m.d;
    if (c.kind != LSK_RR) can_verify = can_verify && m.ncls <= 256;
    if (c.kind == LSK_FV)  // (AP: the relevance of a class is one bit of a 32-bit mask, the padding class included)
        can_verify = can_verify && frdev::path_env("FR_FV_OFF") == nullptr && (measure == M_NDCG ? m.termtab.cap > 0 : m.ncls <= 31);
    if (!can_verify && !topk) return m.ls_exact(c, measure, depth, norms, groups_in, err);
    if (c.kind != LSK_RR) {
        // (a trainer's norms never change: its resident-sum ticket + the array's address stand for the contents, so the two
        // 250 KB comparisons a tick used to make happen once.  Evaluator::norms must stay as it is for a trainer's lifetime.)
        if (!m.norms.ensure(m.nq, err)) return false;
        const uint64_t tok = groups_in[0].resident_owner;
        if (!(tok != 0 && tok == m.norms_token && norms == m.norms_token_ptr)) {
            const bool fresh = !(m.norms_cache.size() == m.nq && std::memcmp(m.norms_cache.data(), norms, m.nq * sizeof(double)) == 0);
            if (!m.upload_norms(norms, err)) return false;
            if (fresh) FR_HIP(hipStreamSynchronize(m.stream));  // uploaded on the main stream, read on the context's
            m.norms_token = tok;
            m.norms_token_ptr = norms;
        }
    }
    // top-k: the groups the policy routes to the exact kernel are staged behind the ones the verify kernel takes
    size_t nV = can_verify ? G : 0;  // groups the verify kernel takes (staged first)
    const std::vector<LineGroup>* gp = &groups_in;
    if (topk && can_verify && m.res_owner != 0) {
        const size_t nE = m.pol.route(G, [&](size_t g) { return groups_in[g].resident_owner == m.res_owner ? (long)groups_in[g].resident_slot : -1L; });
        nV = G - nE;
        if (nE > 0 && nV > 0) {  // verify groups first, exact groups behind them; collect() puts the columns back
            c.gorder.resize(G);
            size_t iv = 0, ie = nV;
            for (size_t g = 0; g < G; g++) c.gorder[m.pol.routed[g] ? ie++ : iv++] = (uint32_t)g;
            c.pgroups.clear();
            for (size_t k = 0; k < G; k++) c.pgroups.push_back(groups_in[c.gorder[k]]);
            gp = &c.pgroups;
        }
    }
    if (topk && nV == 0) m.exact_fallbacks++;
    if (!m.tick_begin(c, *gp, err)) return false;
    c.a = LSArgs{};
    LsTick t{*gp, norms, nV, false, false};
    t.resident = m.stage_resident(c, t.groups, &t.any_update);
    c.resident = t.resident;
    switch (c.kind) {
        case LSK_TOPK: return m.submit_topk(c, t, err);
        case LSK_RR: return m.submit_rr(c, t, err);
        case LSK_FV: return m.submit_fv(c, t, err);
    }
    return false;
}

// The end of a submit whose kernels are queued: the column means behind them, and what collect needs of the line search
// (nverify: the verify kernel took the first nverify staged groups; 0: the exact kernel took them all)
bool DeviceDataset::Impl::submit_queued(LsCtx& c, const LsTick& t, size_t nverify, std::string* err) {
    Impl& m = *this;
    const size_t G = t.groups.size();
    const bool approx = nverify > 0;
    FR_HIP(hipGetLastError());
    if (!m.ls_means(c, err)) return false;
    if (t.resident) m.flip_resident(t.groups);
    c.gslot.assign(G, -1);  // (top-k: the restarts the policies at collect steer)
    if (t.resident)
        for (size_t k = 0; k < G; k++) c.gslot[k] = t.groups[k].resident_slot;
    c.agroups.clear();
    if (c.audit && approx && c.kind != LSK_TOPK) c.agroups.assign(t.groups.begin(), t.groups.end());  // (fr_audit scores their weights from the tiles)
    c.approx = approx;
    c.nverify = nverify;
    c.pending = true;
    return true;
}

// Full ranking / reciprocal rank: the exact kernels take a staged line search after all -- the resident sums are kept current first
bool DeviceDataset::Impl::exact_instead(LsCtx& c, const LsTick& t, std::string* err) {
    Impl& m = *this;
    if (t.resident && t.any_update) {
        if (!m.update_resident(c, 0, t.groups.size(), err)) return false;
        m.flip_resident(t.groups);
    }
    FR_HIP(hipStreamSynchronize(c.stream));  // the tick block is reused by the next call; the exact kernels use the main stream
    return m.ls_exact(c, c.measure, c.depth, t.norms, t.groups, err);
}

// NDCG@k (kernels_verify.inc / kernels_linesearch.inc)
bool DeviceDataset::Impl::submit_topk(LsCtx& c, const LsTick& t, std::string* err) {
    Impl& m = *this;
    const std::vector<LineGroup>& groups = t.groups;
    const size_t G = groups.size(), dp = m.dq * 4, nruns8 = ((m.nruns + 7) / 8) * 8, maxc = c.maxc;
    const int64_t depth = c.depth;
    const bool resident = t.resident;
    const TickStage& ts = c.ts;
    size_t nV = t.nV;
    LSArgs& a = c.a;
    m.topk_args(c, G);
    static const int ls_debug = [] {  // FR_LS_DEBUG (timing ablations of the kernels: 1 = no phase K, 2 = no threshold filter, 16 = count rows)
        const char* dbg = frdev::pricing_env("FR_LS_DEBUG");
        return dbg ? atoi(dbg) : 0;
    }();
    LS_DEBUG_SET(a, ls_debug);
    if (LS_DEBUG(a) & 16) FR_HIP(hipMemsetAsync(m.dbgc.p, 0, 4 * sizeof(unsigned long long), c.stream));
    if (nruns8 * G > 0x7fffffffull) {
        if (err) *err = "linesearch: grid too large";
        return false;
    }
    c.lds = 2 * dp * sizeof(double);
    // the error bound of the approximate scores (false: unusable, the exact kernel takes the line search)
    bool approx = nV > 0 && (LS_DEBUG(a) & ~3) == 0;  // (debug 1/2: timing ablations)
    if (approx) approx = m.compute_eps2(groups, resident, m.key_bits, /*bare_admission=*/true, /*key_relative=*/true);
    a.gamma = m.eps_gamma;
    // (sums from the tiles keep two groups' weights in LDS next to the verify kernel's rank-major copy of the DCG term
    // table: a wide matrix with many gain classes does not fit)
    const size_t tab_lds = (m.ncls + 1) * (size_t)(LS_KT + 1) * sizeof(double);
    if (approx && !resident && 2 * dp * sizeof(double) + tab_lds + 2 * (WAVE + 4) * sizeof(uint4) > 64 * 1024) approx = false;
    if (!approx && nV > 0) {
        // the verify launch turned out unusable (compute_eps2 refused the weights, the tables do not fit LDS): the exact
        // kernel takes ALL staged groups; if some were routed, collect() puts the columns back through gorder
        m.exact_fallbacks++;
        nV = 0;
    }
    // visiting order of the resident verify kernel: per group the threshold (order_threshold) and the mode bits of columns
    // with crowded extremes, and the resident slots whose R ranks this tick refreshes (LsPolicy::plan_rank_refresh)
    size_t nrank = 0;
    a.xslot = nullptr;
    if (approx && resident && m.xslot.p != nullptr && m.rslot.p != nullptr && m.colstd.size() == m.d) {
        static const double kappa = [] {
            const char* e = frdev::pricing_env("FR_ORDER_KAPPA");
            return e ? std::atof(e) : 1.0;
        }();
        static const unsigned period = [] {
            const char* e = frdev::pricing_env("FR_RANK_PERIOD");
            return e ? (unsigned)std::max(1, std::atoi(e)) : 16u;
        }();
        double* gthr = c.th<double>(ts.o_gthr);
        uint32_t* gmode = c.th<uint32_t>(ts.o_gmode);
        for (size_t g = 0; g < nV; g++) {
            gthr[g] = order_threshold(groups[g].weights, m.colstd, groups[g].feature, kappa);
            gmode[g] = m.colmode[groups[g].feature];
        }
        int32_t* rank = c.th<int32_t>(ts.o_rank);
        nrank = m.pol.plan_rank_refresh(nV, [&](size_t g) { return (size_t)groups[g].resident_slot; }, [&](size_t g) { return groups[g].has_update; },
                                        period, m.res_half, rank, rank + G);
        a.xslot = m.xslot.p;
        a.rslot = m.rslot.p;
        a.gthr = c.td<double>(ts.o_gthr);
        a.gmode = c.td<uint32_t>(ts.o_gmode);
    }
    if (!m.tick_upload(c, approx, err)) return false;
    if (!approx) {  // the exact kernel on every (run, group) pair, the resident updates first (the verify kernel applies them)
        if (resident && t.any_update && !m.update_resident(c, 0, G, err)) return false;
        {
            ProfScope ps("linesearch_ndcg_kernel", c.stream);
            dispatch_exact(a, depth, (unsigned)(nruns8 * G), maxc, c.lds, c.stream);
        }
        return m.submit_queued(c, t, 0, err);
    }
    // the verify kernel, then the exact kernel on its redo list: a fixed-size grid whose blocks compare themselves with the
    // count on the device, so the host does not wait here (a longer list is finished when the results are collected)
    if (nrank > 0) {
        ProfScope ps("rslot_kernel", c.stream);
        const uint32_t* wl = m.nwlist ? m.wlist.p : nullptr;  // (a view ranks the walk tiles that hold its documents)
        const unsigned nw = (unsigned)(m.nwlist ? m.nwlist : m.nwt);
        rslot_kernel<<<dim3((nw + 3) / 4), 256, 0, c.stream>>>(m.res.p, c.td<int32_t>(ts.o_rank), c.td<int32_t>(ts.o_rank) + G, (uint32_t)nrank,
                                                              a.rs_par, a.rs_updf, m.xcol.p, m.segtab.p, m.wt_start.p, wl, nw, (uint32_t)m.np, m.rslot.p);
        FR_HIP(hipGetLastError());
        if (c.audit) {
            // the permutation invariant of the tables this launch reads (kernels_order.inc): the R ranks just rewritten and
            // the x_f ranks of the tick's features; an offending document counts as an audit mismatch
            if (!m.audit_cnt.ensure(1, err)) return false;
            FR_HIP(hipMemsetAsync(m.audit_cnt.p, 0, sizeof(unsigned long long), c.stream));
            const int32_t* rk = c.th<int32_t>(ts.o_rank);
            for (size_t k = 0; k < nrank; k++)
                order_audit_kernel<<<dim3((nw + 3) / 4), 256, 0, c.stream>>>(m.rslot.p + (size_t)(rk[k] >> 1) * m.np, m.segtab.p, m.wt_start.p, wl, nw, m.audit_cnt.p);
            for (size_t g = 0; g < nV; g++)
                order_audit_kernel<<<dim3((nw + 3) / 4), 256, 0, c.stream>>>(m.xslot.p + (size_t)groups[g].feature * m.np, m.segtab.p, m.wt_start.p, wl, nw, m.audit_cnt.p);
            unsigned long long bad = 0;
            FR_HIP(hipMemcpyAsync(&bad, m.audit_cnt.p, sizeof(bad), hipMemcpyDeviceToHost, c.stream));
            FR_HIP(hipStreamSynchronize(c.stream));
            m.audit_mismatches += bad;
        }
    }
    // keys kept per list: K + 1, or K + 2 / K + 3 once many pairs failed verification (tied clusters at the cut);
    // FR_VERIFY_XS=1|2|3 pins it (tests)
    const char* xs_e = frdev::path_env("FR_VERIFY_XS");
    const int xs = std::min(xs_e ? std::atoi(xs_e) : m.verify_xs, verify_xs_cap(depth));
    c.xs_used = xs;
    c.xs_pinned = xs_e != nullptr;
    a.eps2 = c.td<double>(ts.o_eps2);
    a.G = (uint32_t)nV;  // (the verify launch and its redo list cover the first nV staged groups)
    const bool dupk = resident && m.key_bits > m.key_cls_bits;  // duplicate groups with mixed gains exist: the DUP variants
    c.dup = dupk;
    {
        ProfScope ps("linesearch_verify_kernel", c.stream);
        if (depth <= 5) launch_verify<5>(a, resident, dupk, xs, (unsigned)nruns8, nV, dp, tab_lds, c.stream), c.kbucket = 5;
        else if (depth <= 10) launch_verify<10>(a, resident, dupk, xs, (unsigned)nruns8, nV, dp, tab_lds, c.stream), c.kbucket = 10;
        else launch_verify<20>(a, resident, dupk, xs, (unsigned)nruns8, nV, dp, tab_lds, c.stream), c.kbucket = 20;
    }
    FR_HIP(hipGetLastError());
    // (the first launch on the redo list: the grid this context's policy has arrived at, next_redo_grid)
    a.slice_count = c.td<uint32_t>(ts.o_count) + 1;
    const unsigned redo_pin = redo_grid_env();
    c.redo_grid_used = redo_pin ? redo_pin : c.redo_grid;
    if (!m.redo_launch(c, 0, c.td<uint32_t>(ts.o_count), c.redo_grid_used, err)) return false;
    if (nV < G) {  // the routed groups: the exact kernel over all their (run, group) pairs
        if (t.any_update && !m.update_resident(c, nV, G - nV, err)) return false;  // (the verify kernel applies the pending updates of its own groups only)
        LSArgs x = a;
        x.work_list = nullptr;
        x.work_count = nullptr;
        x.g_base = (uint32_t)nV;
        x.G = (uint32_t)(G - nV);
        ProfScope ps("linesearch_ndcg_kernel", c.stream);
        dispatch_exact(x, depth, (unsigned)(nruns8 * (G - nV)), maxc, c.lds, c.stream);
    }
    return m.submit_queued(c, t, nV, err);
}

// reciprocal rank (kernels_rr.inc): resident sums only
bool DeviceDataset::Impl::submit_rr(LsCtx& c, const LsTick& t, std::string* err) {
    Impl& m = *this;
    const size_t G = t.groups.size();
    if (!t.resident) return m.ls_exact(c, c.measure, c.depth, t.norms, t.groups, err);
    bool approx = m.compute_eps2(t.groups, true, 0);
    if (approx && m.pol.take_skip()) m.exact_fallbacks++, approx = false;  // (a recent line search redid many pairs)
    if (!m.tick_upload(c, approx, err)) return false;
    if (!approx) return m.exact_instead(c, t, err);
    if (!c.M.ensure(m.nq * c.ldm, err) || !c.redo.ensure(m.nq * G, err)) return false;
    RRArgs& ra = c.ra;
    ra = m.rr_args(c, G);
    {
        ProfScope ps("rr_verify_kernel", c.stream);
        FR_HIP(hipFuncSetAttribute((const void*)rr_verify_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
        for (size_t ci = m.size_classes.size(); ci-- > 0;) {
            const auto& sc = m.size_classes[ci];
            ra.qlist = m.qlist.p + sc.offset;
            rr_verify_kernel<<<dim3((unsigned)sc.count, (unsigned)G), WAVE, (size_t)sc.npad * sizeof(uint4), c.stream>>>(ra);
        }
    }
    FR_HIP(hipGetLastError());
    const unsigned redo_pin = redo_grid_env();
    c.redo_grid_used = redo_pin ? redo_pin : RR_REDO_GRID;
    if (!m.redo_launch(c, 0, c.td<uint32_t>(c.ts.o_count), c.redo_grid_used, err)) return false;
    return m.submit_queued(c, t, G, err);
}

// NDCG of any depth / AP (kernels_fullverify.inc)
bool DeviceDataset::Impl::submit_fv(LsCtx& c, const LsTick& t, std::string* err) {
    Impl& m = *this;
    const size_t G = t.groups.size();
    uint32_t cls_bits = 0;  // low key bits of the gain class / duplicate group
    while ((size_t(1) << cls_bits) < m.ncls + 1) cls_bits++;  // (+1: the padding class)
    // duplicate groups with mixed gain classes (found at upload): the DUP instantiations carry the group id in the keys
    // behind the class and decide pairs of one group by the reference's tie-break (kernels_fullverify.inc)
    const uint32_t dup_bits = (m.key_bits > m.key_cls_bits && cls_bits + (m.key_bits - m.key_cls_bits) <= 20) ? m.key_bits - m.key_cls_bits : 0u;
    bool approx = m.compute_eps2(t.groups, t.resident, cls_bits + dup_bits);
    if (approx && m.pol.take_skip()) m.exact_fallbacks++, approx = false;  // (a recent line search redid many pairs)
    if (!m.tick_upload(c, approx, err)) return false;
    if (!approx) return m.exact_instead(c, t, err);
    if (!c.M.ensure(m.nq * c.ldm, err) || !c.redo.ensure(m.nq * G, err)) return false;
    const size_t slot_rows = ((m.maxlen + 63) / 64 + 1) * 64;
    if (!c.fv_rows.ensure((size_t)FV_REDO_GRID * slot_rows * 64, err)) return false;
    FVArgs fa = m.fv_args(c, G, cls_bits, dup_bits);
    c.dup = dup_bits != 0;
    {
        // longest queries first (fewest blocks, longest running).  FR_FV_PROFILE=1 times every size class on its own.
        static const bool per_class = frdev::pricing_env("FR_FV_PROFILE") != nullptr;
        ProfScope ps_all(per_class ? "fullrank_verify_all" : "fullrank_verify_kernel", c.stream);
        for (size_t ci = m.fv_classes.size(); ci-- > 0;) {
            const auto& sc = m.fv_classes[ci];
            static std::vector<std::string> names = [] {
                std::vector<std::string> v;
                for (int i = 0; i < FV_NCLASSES; i++) v.push_back("fullrank_verify_kernel<" + std::to_string(FV_CLASSES[i].nl) + "x" + std::to_string(FV_CLASSES[i].pl) + ">");
                return v;
            }();
            std::unique_ptr<ProfScope> ps(per_class ? new ProfScope(names[sc.npad].c_str(), c.stream) : nullptr);
            fa.qlist = m.fv_qlist.p + sc.offset;
            if (!fv_launch_class(fa, (int)sc.npad, (unsigned)sc.count, (unsigned)G, (unsigned)c.maxc, c.stream)) {
                if (err) *err = "fullrank_verify_kernel: no instantiation for this size class";
                return false;
            }
        }
    }
    FR_HIP(hipGetLastError());
    // the exact kernels on the redo list: a block owns one slot of score rows
    FSArgs& fs = c.fsa;
    fs = m.scores_args(fa.gfeat, fa.gw, fa.gcand, c.fv_rows.p, c.flags.p, G);
    fs.qstart = m.qstart.p;
    fs.qlen = m.qlen.p;
    fs.G = (uint32_t)G;
    fs.slot_rows = (uint32_t)slot_rows;
    RMArgs& rm = c.rma;
    rm = m.rank_args(c.fv_rows.p, fa.gncand, c.M.p, c.flags.p, G, c.ldm, c.measure, c.depth);
    rm.G = (uint32_t)G;
    rm.slot_rows = (uint32_t)slot_rows;
    c.redo_grid_used = FV_REDO_GRID;
    if (!m.redo_launch(c, 0, c.td<uint32_t>(c.ts.o_count), FV_REDO_GRID, err)) return false;
    return m.submit_queued(c, t, G, err);
}

// The exact kernels alone (exact_kernels), then the means.  A context of its own hands the groups, their resident updates applied, to the
// lock-step form on the main stream's context, which tries bound-and-verify once more before it comes here (the skip
// counter has moved on: the last tick of a back-off verifies again).
bool DeviceDataset::Impl::ls_exact(LsCtx& c, int measure, int64_t depth, const double* norms, const std::vector<LineGroup>& groups,
                                   std::string* err) {
    Impl& m = *this;
    if (&c != &m.ls[LS_CONTEXTS]) {
        c.pgroups.assign(groups.begin(), groups.end());
        for (LineGroup& lg : c.pgroups) lg.has_update = false;
        LsCtx& l = m.ls[LS_CONTEXTS];
        m.cap_outer = &c;
        const bool done = m.ls_submit(l, LS_FULLRANK, measure, depth, norms, c.pgroups, err) && m.ls_collect(l, &c.exact_means, err);
        m.cap_outer = nullptr;
        if (!done) return false;
        c.counts = l.counts;
        c.ready = c.pending = true;
        return true;
    }
    const size_t G = groups.size(), ldm = G * 64;
    std::vector<double>& means = c.exact_means;
    means.assign(ldm, 0.0);
    if (!m.M.ensure(m.nq * ldm, err) || !m.norms.ensure(m.nq, err) || !m.means.ensure(ldm, err)) return false;
    if (!m.upload_norms(norms, err)) return false;
    if (!m.exact_kernels(groups, measure, depth, c.maxc, m.M.p, m.flags.p, err)) return false;
    if (!launch_means(m.M.p, ldm, ldm, m.nq, m.sums_only, m.partial, m.means, m.stream, err)) return false;
    FR_HIP(hipMemcpyAsync(means.data(), m.means.p, ldm * sizeof(double), hipMemcpyDeviceToHost, m.stream));
    m.last_ldm = ldm;
    m.last_cols = ldm;
    m.last_M = m.M.p;
    if (!m.pull_flags(err)) return false;
    c.ready = c.pending = true;
    return true;
}

// The exact kernels of ls_exact into M (nq x groups * 64, the main stream's norms): the scores kernel and the rank-counting
// kernel on the main stream, in chunks of groups whose score rows take at most half of the free HBM.
bool DeviceDataset::Impl::exact_kernels(const std::vector<LineGroup>& groups, int measure, int64_t depth, size_t maxc, double* M,
                                        int* flags, std::string* err) {
    Impl& m = *this;
    const size_t G = groups.size(), dp = m.dq * 4, ldm = G * 64;
    const size_t row_bytes = 64 * sizeof(double);
    size_t budget = m.rows.bytes();
    if (G * m.np * row_bytes > budget) {  // the buffer has to grow: see what is there (it is released first)
        size_t free_b = 0, total_b = 0;
        (void)hipMemGetInfo(&free_b, &total_b);
        budget = std::max<size_t>(size_t(1) << 30, (free_b + m.rows.bytes()) / 2);
    }
    size_t GC = std::max<size_t>(1, std::min<size_t>(G, budget / (m.np * row_bytes)));
    if (!m.rows.ensure(m.np * GC * 64, err) || !m.gfeat.ensure(GC, err) || !m.gncand.ensure(GC, err) || !m.gw.ensure(GC * dp, err) ||
        !m.gcand.ensure(GC * 64, err))
        return false;
    for (size_t g0 = 0; g0 < G; g0 += GC) {
        const size_t gc = std::min(GC, G - g0);
        std::vector<uint32_t> gfeat(gc), gncand(gc);
        std::vector<double> gw(gc * dp, 0.0), gcand(gc * 64, 0.0);
        for (size_t g = 0; g < gc; g++) {
            const LineGroup& lg = groups[g0 + g];
            gfeat[g] = lg.feature;
            gncand[g] = (uint32_t)lg.candidates.size();
            std::memcpy(&gw[g * dp], lg.weights.data(), m.d * sizeof(double));
            std::memcpy(&gcand[g * 64], lg.candidates.data(), lg.candidates.size() * sizeof(double));
        }
        FR_HIP(hipMemcpyAsync(m.gfeat.p, gfeat.data(), gc * sizeof(uint32_t), hipMemcpyHostToDevice, m.stream));
        FR_HIP(hipMemcpyAsync(m.gncand.p, gncand.data(), gc * sizeof(uint32_t), hipMemcpyHostToDevice, m.stream));
        FR_HIP(hipMemcpyAsync(m.gw.p, gw.data(), gc * dp * sizeof(double), hipMemcpyHostToDevice, m.stream));
        FR_HIP(hipMemcpyAsync(m.gcand.p, gcand.data(), gc * 64 * sizeof(double), hipMemcpyHostToDevice, m.stream));
        FR_HIP(hipStreamSynchronize(m.stream));  // the staging vectors are locals
        {
            ProfScope ps("linesearch_scores_kernel", m.stream);
            const FSArgs fa = m.scores_args(m.gfeat.p, m.gw.p, m.gcand.p, m.rows.p, flags, gc);
            launch_scores(fa, maxc, (unsigned)(((m.nruns + 7) / 8) * 8 * gc), 2 * dp * sizeof(double), m.stream);
        }
        FR_HIP(hipGetLastError());
        RMArgs ra = m.rank_args(m.rows.p, m.gncand.p, M, flags, gc, ldm, measure, depth);
        ra.col0 = (uint32_t)(g0 * 64);
        {
            ProfScope ps("rank_metric_kernel", m.stream);
            FR_HIP(hipFuncSetAttribute((const void*)rank_metric_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       128 * 1024));
            // longest queries first (their O(n^2) sweeps are the tail), several waves per long query
            for (size_t ci = m.size_classes.size(); ci-- > 0;) {
                const auto& sc = m.size_classes[ci];
                ra.qlist = m.qlist.p + sc.offset;
                dim3 grid((unsigned)sc.count, (unsigned)gc);
                // one wave up to 128 documents (measured: a second wave only adds traffic there), then 2/4/8
                const unsigned waves = (measure != M_NDCG && measure != M_AP) ? 1u  // reciprocal rank: linear, one wave
                                       : sc.npad <= 128 ? 1u : (sc.npad <= 256 ? 2u : (sc.npad <= 512 ? 4u : 8u));
                rank_metric_kernel<<<grid, WAVE * waves, (size_t)sc.npad * 64, m.stream>>>(ra);
            }
        }
        FR_HIP(hipGetLastError());
    }
    return true;
}

bool DeviceDataset::Impl::ls_collect(LsCtx& c, std::vector<double>* means, std::string* err) {
    Impl& m = *this;
    c.pending = false;
    if (c.ready) {
        *means = c.exact_means;
        if (m.cap_on) return m.capture_tick(c, *means, 0, err);
        return true;
    }
    const size_t ldm = c.ldm, G = ldm / 64;
    means->assign(ldm, 0.0);
    if (G == 0) return true;
    uint32_t nredo = 0, nslices = 0;  // pairs listed; top-k: slices of them the exact kernel recomputed
    std::vector<uint32_t>& by_group = c.gredo_h;
    if (!m.tick_finish(c, ldm, means, &nredo, err, &nslices, c.kind == LSK_TOPK ? &by_group : nullptr)) return false;
    LSArgs& a = c.a;  // (top-k: a.G = the groups of the verify launch)
    if (c.approx) {
        const size_t nV = c.nverify;
        m.approx_pairs += m.nq * nV;
        m.approx_redo += nredo;
        c.counts.pairs += m.nq * nV;
        c.counts.redone += nredo;
        const unsigned grid = c.redo_grid_used;
        uint32_t again = 0;
        if (nredo > grid &&  // the rest of a long redo list, then the column results again
            (!m.redo_launch(c, grid, nullptr, nredo - grid, err) || !m.ls_means(c, err) || !m.tick_finish(c, ldm, means, &again, err, &nslices)))
            return false;
        switch (c.kind) {
            case LSK_TOPK:
                if (!m.topk_policy(c, nredo, nslices, err)) return false;
                break;
            default:
                m.pol.observe_skip(nredo, m.nq, G);
                if (c.audit && !m.fr_audit(c, err)) return false;
                break;
        }
    }
    if (!c.gorder.empty()) {  // routed groups were staged behind the others: columns back in the caller's order
        std::vector<double> tmp(*means);
        for (size_t k = 0; k < G; k++) std::memcpy(means->data() + (size_t)c.gorder[k] * 64, tmp.data() + k * 64, 64 * sizeof(double));
    }
    m.last_ldm = ldm;
    m.last_cols = ldm;
    m.last_M = c.M.p;  // (per-query inspection is for stateless callers, whose groups are never routed)
    if (LS_DEBUG(a) & 16) {
        unsigned long long cnt[4];
        FR_HIP(hipMemcpyAsync(cnt, m.dbgc.p, sizeof(cnt), hipMemcpyDeviceToHost, c.stream));
        FR_HIP(hipStreamSynchronize(c.stream));
        fprintf(stderr, "[FR_LS_DEBUG] docs=%llu rows=%llu (%.3f of docs) batches=%llu insertion_rows=%llu\n", cnt[3], cnt[0],
                (double)cnt[0] / (double)cnt[3], cnt[1], cnt[2]);
    }
    if (m.cap_on) return m.capture_tick(c, *means, c.approx ? nredo : 0, err);
    return true;
}

// Tick capture: the collected line search of context c as one event of the log -- its groups and how they were staged, the
// path it took, the instantiation, the redo list, and copies of what it published and of the resident sums it left.  Reads
// only; the copies and the synchronisation are its own.  A line search the lock-step context evaluated for another context
// (ls_exact) was recorded there, matrix included, under that context's index with its groups and their pending updates.
bool DeviceDataset::Impl::capture_tick(LsCtx& c, const std::vector<double>& means, uint32_t nredo, std::string* err) {
    Impl& m = *this;
    const bool lockstep = &c == &m.ls[LS_CONTEXTS];
    if (c.ready && !lockstep) return true;
    const LsCtx& who = (lockstep && m.cap_outer) ? *m.cap_outer : c;
    if (who.cgroups.size() * 64 != c.ldm) return true;  // (submitted before the capture was switched on: its groups were not kept)
    LsCapture e;
    e.ctx = (int)(&who - m.ls);
    e.kind = (int)c.kind;
    e.measure = c.measure;
    e.depth = c.depth;
    e.groups = who.cgroups;
    const size_t G = e.groups.size();
    e.gorder = c.gorder;
    if (e.gorder.empty())
        for (size_t g = 0; g < G; g++) e.gorder.push_back((uint32_t)g);
    e.nverify = c.approx ? c.nverify : 0;
    e.approx = c.approx;
    e.resident = who.resident;
    e.ready = c.ready;
    hipStream_t st = c.ready ? m.stream : c.stream;
    if (c.kind == LSK_TOPK) {
        e.kbucket = c.kbucket;  // (all zero when the exact kernel took the line search whole: no verify launch)
        e.xs_used = c.kbucket ? c.xs_used : 0;
        e.xs_pinned = c.kbucket ? c.xs_pinned : false;
    } else if (c.approx) {
        if (c.kind == LSK_FV)
            for (const auto& sc : m.fv_classes) e.classes.insert(e.classes.end(), {FV_CLASSES[sc.npad].nl, FV_CLASSES[sc.npad].pl, sc.count});
        else
            for (const auto& sc : m.size_classes) e.classes.insert(e.classes.end(), {sc.npad, 1u, sc.count});
    }
    e.dup = c.dup;
    e.redo_groups = (uint32_t)(c.kind == LSK_TOPK ? c.nverify : G);
    if (c.approx && nredo > 0) {
        e.redo.resize(nredo);
        FR_HIP(hipMemcpyAsync(e.redo.data(), c.redo.p, nredo * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    e.means = means;
    e.nq = m.nq;
    e.ldm = G * 64;
    e.np = m.np;
    const double* M = c.ready ? m.M.p : c.M.p;
    e.has_matrix = M != nullptr;
    if (e.has_matrix) {
        e.matrix.resize(e.nq * e.ldm);
        FR_HIP(hipMemcpyAsync(e.matrix.data(), M, e.matrix.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    if (e.resident) {
        for (const LineGroup& lg : e.groups) e.res_slots.push_back(lg.resident_slot);
        std::sort(e.res_slots.begin(), e.res_slots.end());
        e.res_slots.erase(std::unique(e.res_slots.begin(), e.res_slots.end()), e.res_slots.end());
        e.res.resize(e.res_slots.size() * m.np);
        for (size_t i = 0; i < e.res_slots.size(); i++) {
            const size_t slot = (size_t)e.res_slots[i];
            FR_HIP(hipMemcpyAsync(e.res.data() + i * m.np, m.res.p + (slot * 2 + m.res_half[slot]) * m.np, m.np * sizeof(double), hipMemcpyDeviceToHost, st));
        }
    }
    FR_HIP(hipStreamSynchronize(st));
    m.cap_log.push_back(std::move(e));
    return true;
}

// Full ranking / reciprocal rank under FR_VERIFY_AUDIT, after a verified line search and its long-redo pass: every value it
// published (verified, or recomputed from the redo list by the work-list kernels) against ls_exact's kernels run over ALL
// (query, group) pairs of the same groups, bit for bit.  Those write into a matrix of their own, so the published one, the
// means and every counter but audit_* stay as they are.  It starts as all-ones words (a NaN no metric value has): a cell the
// exact kernels leave unwritten differs.  The columns beyond each group's candidates (defined by neither side) are copied
// from the published matrix and not counted.  The exact kernels read the norms on the device: those of this line search
// (ls_submit uploaded them for the full-ranking kind, whose trainer's norms never change; reciprocal rank reads none).
bool DeviceDataset::Impl::fr_audit(LsCtx& c, std::string* err) {
    Impl& m = *this;
    const size_t nel = m.nq * c.ldm;
    if (!m.audit.ensure(nel, err) || !m.audit_cnt.ensure(1, err) || !m.audit_flags.ensure(1, err)) return false;
    FR_HIP(hipMemsetAsync(m.audit.p, 0xFF, nel * sizeof(double), m.stream));
    size_t ncells = 0;
    for (size_t g = 0; g < c.agroups.size(); g++) {
        const size_t nc = c.agroups[g].candidates.size();
        ncells += m.nq * nc;
        if (nc < 64)  // (c.M is final: collected)
            FR_HIP(hipMemcpy2DAsync(m.audit.p + g * 64 + nc, c.ldm * sizeof(double), c.M.p + g * 64 + nc, c.ldm * sizeof(double),
                                    (64 - nc) * sizeof(double), m.nq, hipMemcpyDeviceToDevice, m.stream));
    }
    FR_HIP(hipMemsetAsync(m.audit_flags.p, 0, sizeof(int), m.stream));
    if (!m.exact_kernels(c.agroups, c.measure, c.depth, c.maxc, m.audit.p, m.audit_flags.p, err)) return false;
    FR_HIP(hipMemsetAsync(m.audit_cnt.p, 0, sizeof(unsigned long long), m.stream));
    audit_compare_kernel<<<dim3(1024), dim3(256), 0, m.stream>>>(m.audit.p, c.M.p, nel, m.audit_cnt.p);
    FR_HIP(hipGetLastError());
    unsigned long long bad = 0;
    FR_HIP(hipMemcpyAsync(&bad, m.audit_cnt.p, sizeof(bad), hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipStreamSynchronize(m.stream));
    m.audit_values += ncells;
    m.audit_mismatches += bad;
    return true;
}

// Top-k, after a verified line search: the redo grid, the restarts' R-rank modes, the audit, and the list length / back-off.
bool DeviceDataset::Impl::topk_policy(LsCtx& c, uint32_t nredo, uint32_t nslices, std::string* err) {
    Impl& m = *this;
    const size_t ldm = c.ldm, G = ldm / 64, nV = c.nverify;
    const std::vector<uint32_t>& by_group = c.gredo_h;
    LSArgs& a = c.a;
    c.redo_grid = next_redo_grid(c.redo_grid, c.redo_grid_used, nredo);
    m.approx_redo_entries += nslices;
    for (size_t k = 0; k < nV; k++) m.chain_runs += by_group[G + k];
    m.chain_visits += (unsigned long long)m.n * nV;
    {
        static const double t_off = [] {
            const char* e = frdev::pricing_env("FR_RANK_OFF_BELOW");
            return e ? std::atof(e) : RANK_OFF_BELOW;
        }();
        static const double t_on = [] {
            const char* e = frdev::pricing_env("FR_RANK_ON_ABOVE");
            return e ? std::atof(e) : RANK_ON_ABOVE;
        }();
        m.pol.observe_chain(nV, [&](size_t k) { return (long)c.gslot[k]; }, [&](size_t k) { return by_group[G + k]; }, m.n, t_off, t_on);
    }
    if (c.audit) {
        // audit: every value this line search published (verified, or recomputed from the redo list) against the
        // exact kernel run over ALL (run, group) pairs -- bit for bit.  The exact kernel rewrites M with what must
        // be the same numbers; the means were already formed from the published ones.
        const size_t nel = m.nq * ldm;
        if (!m.audit.ensure(nel, err) || !m.audit_cnt.ensure(1, err)) return false;
        FR_HIP(hipMemcpyAsync(m.audit.p, c.M.p, nel * sizeof(double), hipMemcpyDeviceToDevice, c.stream));
        LSArgs x = a;
        x.work_list = nullptr;
        x.work_count = nullptr;
        x.g_base = 0;
        x.G = (uint32_t)G;
        dispatch_exact(x, c.depth, (unsigned)(((m.nruns + 7) / 8) * 8 * G), c.maxc, c.lds, c.stream);
        FR_HIP(hipMemsetAsync(m.audit_cnt.p, 0, sizeof(unsigned long long), c.stream));
        audit_compare_kernel<<<dim3(1024), dim3(256), 0, c.stream>>>(m.audit.p, c.M.p, nel, m.audit_cnt.p);
        unsigned long long bad = 0;
        FR_HIP(hipMemcpyAsync(&bad, m.audit_cnt.p, sizeof(bad), hipMemcpyDeviceToHost, c.stream));
        FR_HIP(hipStreamSynchronize(c.stream));
        m.audit_values += nel;
        m.audit_mismatches += bad;
    }
    // the list length, or else the restarts' back-off (LsPolicy::observe_redo)
    m.pol.observe_redo(nV, [&](size_t k) { return (long)c.gslot[k]; }, [&](size_t k) { return by_group[k]; }, m.nq, c.xs_used, verify_xs_cap(c.depth),
                       c.xs_pinned, LS_DEBUG(a), m.verify_xs);
    return true;
}

bool DeviceDataset::linesearch_submit(int ctx, int measure, int64_t depth, const double* norms, const std::vector<LineGroup>& groups,
                                      std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    if (ctx < 0 || ctx >= LS_CONTEXTS || m.ls[ctx].pending) {
        if (err) *err = "linesearch_submit: no such context, or a submitted line search was not collected";
        return false;
    }
    return m.ls_submit(m.ls[ctx], linesearch_path(measure, depth), measure, depth, norms, groups, err);
}

bool DeviceDataset::linesearch_collect(int ctx, std::vector<double>* means, LsCounts* counts, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    if (ctx < 0 || ctx >= LS_CONTEXTS || !m.ls[ctx].pending) {
        if (err) *err = "linesearch_collect: nothing was submitted on this context";
        return false;
    }
    if (!m.ls_collect(m.ls[ctx], means, err)) return false;
    if (counts) *counts = m.ls[ctx].counts;
    return true;
}

bool DeviceDataset::linesearch(int measure, int64_t depth, const double* norms, const std::vector<LineGroup>& groups,
                               std::vector<double>* means, LsCounts* counts, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    const LsPath path = linesearch_path(measure, depth);
    Impl::LsCtx& c = m.ls[path == LS_TOPK ? 0 : LS_CONTEXTS];
    if (c.pending) {
        if (err) *err = "linesearch: context 0 busy (collect the submitted line search first)";
        return false;
    }
    if (!m.ls_submit(c, path, measure, depth, norms, groups, err) || !m.ls_collect(c, means, err)) return false;
    if (counts) *counts = c.counts;
    return true;
}





#include "train_rf.inc"
#include "train_lambda.inc"
#include "train_dart.inc"
#include "train_hist.inc"
