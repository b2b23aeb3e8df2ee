// Part of device.hip (single translation unit; see that file's header).  Forest scoring (DESIGN.md section 5.6): the launchers of
// kernels_treerank.inc and kernels_tree.inc, the packed-forest cache and the plan bookkeeping.  The three encodings and their
// limits are host arithmetic in forest_pack.hpp; every path here reads: fill options, pack, ensure, copy, launch, record the plan.

// The last score_trees call's plan (device.hpp: TreePlan), written by whichever path launched.
static std::mutex g_tree_plan_mu;
static TreePlan g_tree_plan;
static void set_tree_plan(TreePlan&& p) {
    std::lock_guard<std::mutex> lk(g_tree_plan_mu);
    g_tree_plan = std::move(p);
}
TreePlan last_tree_plan() {
    std::lock_guard<std::mutex> lk(g_tree_plan_mu);
    return g_tree_plan;
}

// The packers' timing switches (forest_pack.hpp: ForestPackOptions), read once per call; all unset in the shipped library.
static ForestPackOptions forest_pack_options() {
    ForestPackOptions opt;
    if (const char* e = frdev::pricing_env("FR_TREE_CAP_KB")) opt.cap_kb = std::atoi(e);
    if (const char* e = frdev::pricing_env("FR_TREE_NMAX")) opt.nmax = std::max(1, std::atoi(e));
    opt.nowalk = frdev::pricing_env("FR_TREE_NOWALK") != nullptr;
    opt.nostage = frdev::pricing_env("FR_TREE_NOSTAGE") != nullptr;
    return opt;
}

static void launch_tree_lds(const TreeShape& sh, size_t lds, hipStream_t stream, PosMap pm, size_t pos_threads, const float* xb, uint32_t dq,
                            const fr_u32x4* forest, const uint32_t* desc, uint32_t nbatch, int raw_single, const double* leafprod,
                            double* scores) {
    auto go = [&](auto kern) {
        (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        kern<<<grid1d(pos_threads, sh.docs), sh.docs * sh.parts, lds, stream>>>(xb, pm, dq, forest, desc, nbatch, raw_single, leafprod, scores);
    };
    const unsigned key = sh.docs * 10 + sh.parts;
    if (key == 2561) go(tree_ensemble_lds_kernel<256, 1, 6>);
    else if (key == 2562) go(tree_ensemble_lds_kernel<256, 2, 3>);
    else if (key == 2564) go(tree_ensemble_lds_kernel<256, 4, 4>);
    else if (key == 1922) go(tree_ensemble_lds_kernel<192, 2, 8>);
    else if (key == 1924) go(tree_ensemble_lds_kernel<192, 4, 4>);
    else if (key == 1281) go(tree_ensemble_lds_kernel<128, 1, 24>);
    else if (key == 1282) go(tree_ensemble_lds_kernel<128, 2, 24>);
    else if (key == 1284) go(tree_ensemble_lds_kernel<128, 4, 12>);
    else if (key == 641) go(tree_ensemble_lds_kernel<64, 1, 24>);
    else go(tree_ensemble_lds_kernel<64, 4, 24>);
}

// Scores a forest with tree_ensemble_lds_kernel.  Returns false with an empty *err when the forest
// does not fit the compact encoding in any block shape (caller falls back to the L2 walk).
// Shapes are tried in the order of forest_pack.hpp's tables.  FR_TREE_SHAPE="docs,parts" pins one shape (benchmarking).
bool DeviceDataset::try_score_trees_lds(const FlatTrees& t, std::string* err) {
    if (err) err->clear();
    unsigned want_docs = 0, want_parts = 0;
    if (const char* e = frdev::path_env("FR_TREE_SHAPE")) std::sscanf(e, "%u,%u", &want_docs, &want_parts);
    const auto* order = t.raw_single ? TREE_ORDER_SINGLE : TREE_ORDER_MULTI;
    const size_t norder = t.raw_single ? std::size(TREE_ORDER_SINGLE) : std::size(TREE_ORDER_MULTI);
    for (size_t i = 0; i < norder; i++) {
        if (want_docs && !t.raw_single && (order[i][0] != want_docs || order[i][1] != want_parts)) continue;
        for (const TreeShape& sh : TREE_SHAPES) {
            if (sh.docs != order[i][0] || sh.parts != order[i][1]) continue;
            if (try_score_trees_lds_shape(t, sh, err)) return true;
            if (err && !err->empty()) return false;
        }
    }
    if (want_docs && !t.raw_single) {  // pinned shape outside the default order (e.g. 256,1)
        for (const TreeShape& sh : TREE_SHAPES)
            if (sh.docs == want_docs && sh.parts == want_parts && try_score_trees_lds_shape(t, sh, err)) return true;
    }
    return false;
}

// Packs the forest for one block shape and launches the kernel.
bool DeviceDataset::try_score_trees_lds_shape(const FlatTrees& t, const TreeShape& shape, std::string* err) {
    Impl& m = *impl_;
    LdsForest f;
    if (!pack_forest_lds(t, shape, (uint32_t)m.d, (uint32_t)m.dq, forest_pack_options(), &f)) return false;
    const size_t nbatch = f.desc.size() / 4 - 1;
    m.tree_rank.hash = 0;  // (the forest buffers are about to hold another layout)
    if (!m.forest.ensure(f.forest.size(), err) || !m.batch_off.ensure(f.desc.size(), err) || !m.leafprod.ensure(f.leafprod.size(), err)) return false;
    FR_HIP(hipMemcpyAsync(m.forest.p, f.forest.data(), f.forest.size() * 8, hipMemcpyHostToDevice, m.stream));
    FR_HIP(hipMemcpyAsync(m.leafprod.p, f.leafprod.data(), f.leafprod.size() * 8, hipMemcpyHostToDevice, m.stream));
    FR_HIP(hipMemcpyAsync(m.batch_off.p, f.desc.data(), f.desc.size() * 4, hipMemcpyHostToDevice, m.stream));
    FR_HIP(hipStreamSynchronize(m.stream));
    {
        ProfScope ps("tree_ensemble_kernel", m.stream);
        const fr_u32x4* f16 = (const fr_u32x4*)m.forest.p;
        const int raw = t.raw_single ? 1 : 0;
        launch_tree_lds(shape, f.lds_bytes, m.stream, m.posmap(), m.pos_threads(), m.xb.p, (uint32_t)m.dq, f16, m.batch_off.p, (uint32_t)nbatch, raw, m.leafprod.p, m.scores.p);
    }
    FR_HIP(hipGetLastError());
    TreePlan plan;
    plan.path = TreePlan::LDS, plan.docs = shape.docs, plan.parts = shape.parts, plan.batches = tree_plan_batches(f.desc);
    set_tree_plan(std::move(plan));
    return true;
}

// Scores a forest with tree_ensemble_rank_kernel.  Returns false with an empty *err when the forest does not fit that
// encoding (pack_forest_rank) -- the caller then
// takes the f32 LDS walk.  FR_TREE_RANK=0 switches the path off (A/B, and the parity tests of the other paths).
bool DeviceDataset::try_score_trees_rank(const FlatTrees& t, std::string* err) {
    Impl& m = *impl_;
    if (err) err->clear();
    if (const char* e = frdev::path_env("FR_TREE_RANK"))
        if (std::atoi(e) == 0) return false;
    if (t.root.empty() || t.raw_single) return false;  // (before the cache is asked: its hash does not cover raw_single)
    constexpr unsigned DOCS = RankBlock::DOCS, H = RankBlock::H, PF = RankBlock::PF;
    auto launch = [&](uint32_t nrounds, uint32_t nslots, size_t nbatch, size_t lds) {
        ProfScope ps("tree_rank_kernel", m.stream);
        auto kern = tree_ensemble_rank_kernel<DOCS, H, PF>;
        (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (frdev::pricing_env("FR_TREE_INFO")) {
            int occ = -1;
            (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void*)kern, (int)(DOCS * H), lds);
            fprintf(stderr, "[tree_rank] slots %u rounds %u batches %zu lds %zu B blocks/CU %d\n", nslots, nrounds, nbatch, lds, occ);
        }
        kern<<<grid1d(m.pos_threads(), DOCS), DOCS * H, lds, m.stream>>>(m.xb.p, m.posmap(), (uint32_t)m.dq, (const uint4*)m.tree_fdesc.p, m.tree_tables.p,
                                                             (const uint4*)m.tree_rdesc.p, nrounds, nslots, (const fr_u32x4*)m.forest.p, m.batch_off.p, (uint32_t)nbatch,
                                                             m.leafprod.p, m.scores.p);
    };
    // the same forest as last time? (FR_TREE_CACHE=0 turns the cache off)
    const uint64_t hash = forest_hash(t);
    static const bool cache_off = [] {
        const char* e = frdev::pricing_env("FR_TREE_CACHE");
        return e != nullptr && e[0] == '0';
    }();
    Impl::RankKept& kept = m.tree_rank;
    if (!cache_off && hash == kept.hash) {
        launch(kept.nrounds, kept.nslots, kept.nbatch, kept.lds);
        FR_HIP(hipGetLastError());
        TreePlan plan;
        plan.path = TreePlan::RANK, plan.cache_hit = true, plan.nslots = kept.nslots, plan.nrounds = kept.nrounds;
        plan.batches = kept.batches;
        set_tree_plan(std::move(plan));
        return true;
    }
    const ForestPackOptions opt = forest_pack_options();
    RankForest f;
    if (!pack_forest_rank(t, (uint32_t)m.d, (uint32_t)m.dq, opt, &f)) return false;
    const size_t nbatch = f.desc.size() / 4 - 1;
    kept.hash = 0;  // only now: a forest refused above has touched no buffer, and the forest kept from before still launches
    if (!m.forest.ensure((f.forest.size() + 1) / 2, err) || !m.batch_off.ensure(f.desc.size(), err) ||
        !m.leafprod.ensure(f.leafprod.size() + (opt.nowalk ? 65536 : 0), err) || !m.tree_fdesc.ensure(f.fdesc.size(), err) || !m.tree_tables.ensure(std::max<size_t>(f.tables.size(), 1), err) ||
        !m.tree_rdesc.ensure(std::max<size_t>(f.rdesc.size(), 1), err))
        return false;
    FR_HIP(hipMemcpyAsync(m.forest.p, f.forest.data(), f.forest.size() * 4, hipMemcpyHostToDevice, m.stream));
    FR_HIP(hipMemcpyAsync(m.leafprod.p, f.leafprod.data(), f.leafprod.size() * 8, hipMemcpyHostToDevice, m.stream));
    FR_HIP(hipMemcpyAsync(m.batch_off.p, f.desc.data(), f.desc.size() * 4, hipMemcpyHostToDevice, m.stream));
    FR_HIP(hipMemcpyAsync(m.tree_fdesc.p, f.fdesc.data(), f.fdesc.size() * 4, hipMemcpyHostToDevice, m.stream));
    if (!f.tables.empty()) FR_HIP(hipMemcpyAsync(m.tree_tables.p, f.tables.data(), f.tables.size() * 4, hipMemcpyHostToDevice, m.stream));
    if (!f.rdesc.empty()) FR_HIP(hipMemcpyAsync(m.tree_rdesc.p, f.rdesc.data(), f.rdesc.size() * 4, hipMemcpyHostToDevice, m.stream));
    FR_HIP(hipStreamSynchronize(m.stream));
    launch(f.nrounds, f.nslots, nbatch, f.lds_bytes);
    FR_HIP(hipGetLastError());
    kept.hash = hash, kept.nrounds = f.nrounds, kept.nslots = f.nslots, kept.nbatch = (uint32_t)nbatch, kept.lds = f.lds_bytes;
    kept.batches = tree_plan_batches(f.desc);
    TreePlan plan;
    plan.path = TreePlan::RANK, plan.nslots = f.nslots, plan.nrounds = f.nrounds, plan.batches = kept.batches;
    set_tree_plan(std::move(plan));
    return true;
}

bool DeviceDataset::score_trees(const FlatTrees& t, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    if (!m.scores.ensure(m.np, err)) return false;
    m.scores_slots = 1;
    if (try_score_trees_rank(t, err)) return true;
    if (err && !err->empty()) return false;
    if (try_score_trees_lds(t, err)) return true;
    if (err && !err->empty()) return false;
    const size_t nt = t.root.size();
    std::vector<TreeNodeDev> nodes;
    std::vector<int32_t> roots;
    adjacent_children_layout(t, nodes, roots);
    const size_t nn = nodes.size();
    if (!m.nodes.ensure(std::max<size_t>(nn, 1), err) || !m.roots.ensure(std::max<size_t>(nt, 1), err) ||
        !m.tweights.ensure(std::max<size_t>(nt, 1), err))
        return false;
    FR_HIP(hipMemcpyAsync(m.nodes.p, nodes.data(), nn * sizeof(TreeNodeDev), hipMemcpyHostToDevice, m.stream));
    FR_HIP(hipMemcpyAsync(m.roots.p, roots.data(), nt * sizeof(int32_t), hipMemcpyHostToDevice, m.stream));
    std::vector<double> tw = t.weight;
    tw.resize(nt, 1.0);
    FR_HIP(hipMemcpyAsync(m.tweights.p, tw.data(), nt * sizeof(double), hipMemcpyHostToDevice, m.stream));
    FR_HIP(hipStreamSynchronize(m.stream));
    const unsigned bs = 64;  // one tile per block (np is a multiple of 64)
    size_t lds = (size_t)bs * (m.dq * 4 + 1) * sizeof(float);
    {
        TreePlan plan;
        plan.path = TreePlan::L2, plan.rows_in_lds = lds <= 150 * 1024;
        set_tree_plan(std::move(plan));
    }
    {
        ProfScope ps("tree_ensemble_kernel", m.stream);
        if (lds <= 150 * 1024) {
            FR_HIP(hipFuncSetAttribute((const void*)tree_ensemble_kernel<true, 8>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            tree_ensemble_kernel<true, 8><<<grid1d(m.pos_threads(), bs), bs, lds, m.stream>>>(
                m.xb.p, m.posmap(), (uint32_t)m.dq, (uint32_t)m.d, m.nodes.p, m.roots.p, m.tweights.p, (uint32_t)nt,
                t.raw_single ? 1 : 0, m.scores.p);
        } else {
            tree_ensemble_kernel<false, 8><<<grid1d(m.pos_threads(), bs), bs, 0, m.stream>>>(
                m.xb.p, m.posmap(), (uint32_t)m.dq, (uint32_t)m.d, m.nodes.p, m.roots.p, m.tweights.p, (uint32_t)nt,
                t.raw_single ? 1 : 0, m.scores.p);
        }
    }
    FR_HIP(hipGetLastError());
    return true;
}
