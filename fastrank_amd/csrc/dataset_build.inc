// Part of device.hip (single translation unit; see that file's header).  DeviceDataset's build: uploads of the host layout (tiles, tables), create, replicate, views.
// ----------------------------------------------------------------------------------------------
// dataset build
// ----------------------------------------------------------------------------------------------
template <typename T>
static bool upload(DevBuf<T>& buf, const std::vector<T>& host, std::string* err) {
    if (!buf.ensure(std::max<size_t>(host.size(), 1), err)) return false;
    if (!host.empty()) FR_HIP(hipMemcpy(buf.p, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
    return true;
}

static std::shared_ptr<DeviceDataset> fail_ds(std::string* err, const std::string& msg) {
    if (err) *err = msg;
    return std::shared_ptr<DeviceDataset>();
}
static bool hip_ok(hipError_t e, const char* what, std::string* err) {
    if (e == hipSuccess) return true;
    if (err) *err = std::string("HIP error: ") + hipGetErrorString(e) + " at " + what;
    return false;
}
struct ThreadJoiner {  // joins on every way out of create()
    std::thread& t;
    ~ThreadJoiner() { if (t.joinable()) t.join(); }
};
// documents a run takes (FR_RUN_DOCS: tuning sweeps)
size_t run_docs_target() {
    const char* t = frdev::pricing_env("FR_RUN_DOCS");
    return t ? std::max<size_t>(64, (size_t)atoll(t)) : 768;
}

// Returns the first error; *at_event: it was the event's.  main_stream hears of the main stream before the others are made.
hipError_t DeviceDataset::Impl::open_streams(bool* at_event, StreamSignal* main_stream) {
    hipError_t e = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
    if (main_stream) main_stream->set(e == hipSuccess);
    for (int i = 0; i < LS_CONTEXTS && e == hipSuccess; i++) e = hipStreamCreateWithFlags(&ls[i].stream, hipStreamNonBlocking);
    if (e != hipSuccess) return e;
    e = hipEventCreateWithFlags(&res_ready, hipEventDisableTiming);
    *at_event = e != hipSuccess;
    return e;
}
bool DeviceDataset::Impl::open_streams(std::string* err) {
    bool at_event = false;
    const hipError_t e = open_streams(&at_event);
    return hip_ok(e, at_event ? "hipEventCreate" : "hipStreamCreate", err);
}

// The feature tiles, on create()'s tile thread and the main stream while the caller builds and uploads the per-position tables.
bool DeviceDataset::Impl::upload_tiles(Impl& m, const HostCSR& csr, bool timing, StreamSignal& main_stream, std::string* terr) {
    if (hipSetDevice(m.device) != hipSuccess) {
        *terr = "hipSetDevice failed in the upload thread";
        return false;
    }
    auto tchk = [&](hipError_t e, const char* what) { return hip_ok(e, what, terr); };
    auto tt = std::chrono::steady_clock::now();
    double t_fill = 0.0, t_wait = 0.0;  // (FR_UPLOAD_TIMING: the tile thread's own stages)
    auto tlap = [&](const char* what) {
        if (!timing) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[upload/tiles] %-36s %7.1f ms\n", what, std::chrono::duration<double, std::milli>(now - tt).count());
        tt = now;
    };
    // ---- feature tiles.  The host only streams the view's rows, row-major as they lie in the caller's matrix, through two
    // pinned slabs (plain memcpy by a pool of threads while the previous slab is on the wire); tile_scatter_kernel moves
    // every row to its padded position in the tile layout and takes the per-column max |x| and the non-finite flag on
    // the way.  One-time cost; SURVEY 8d excludes it from evals/s and bench.py reports it separately.
    const size_t ntiles = m.np / 64;
    const size_t tile_floats = m.dq * 256;
    if (!m.xb.ensure(ntiles * tile_floats, terr)) return false;
    {
        if (!main_stream.wait()) {  // (created by the helper thread)
            *terr = "HIP error: hipStreamCreate failed";
            return false;
        }
        if (!tchk(hipMemsetAsync(m.xb.p, 0, ntiles * tile_floats * sizeof(float), m.stream), "clear feature tiles")) return false;
        // rows of the view in ascending row id (sequential reads of the caller's matrix) and where each one goes
        uint32_t maxrow = 0;
        for (size_t t = 0; t < csr.n; t++) maxrow = std::max(maxrow, csr.perm[t]);
        std::vector<uint32_t> pos_of_row((size_t)maxrow + 1, IDX_INVALID);
        for (size_t p = 0; p < m.np; p++)
            if (m.perm_host[p] != IDX_INVALID) pos_of_row[m.perm_host[p]] = (uint32_t)p;
        std::vector<uint32_t> rows, row_dst;
        rows.reserve(csr.n);
        row_dst.reserve(csr.n);
        for (size_t id = 0; id <= maxrow; id++)
            if (pos_of_row[id] != IDX_INVALID) {
                rows.push_back((uint32_t)id);
                row_dst.push_back(pos_of_row[id]);
            }
        tlap("clear tiles queued, row lists");
        DevBuf<uint32_t> d_dst, d_colmax;
        DevBuf<float> d_stage[2];
        DevBuf<int> d_bad;
        const size_t row_bytes = csr.d * sizeof(float);
        size_t slab_mb = 32;
        if (const char* e = frdev::pricing_env("FR_UPLOAD_SLAB_MB")) slab_mb = std::max(1, std::atoi(e));
        const size_t slab_rows = std::max<size_t>(1, std::min<size_t>(rows.size(), (slab_mb << 20) / row_bytes));
        if (!upload(d_dst, row_dst, terr) || !d_colmax.ensure(csr.d, terr) || !d_bad.ensure(1, terr) ||
            !d_stage[0].ensure(slab_rows * csr.d, terr) || !d_stage[1].ensure(slab_rows * csr.d, terr))
            return false;
        if (!tchk(hipMemsetAsync(d_colmax.p, 0, csr.d * sizeof(uint32_t), m.stream), "clear column maxima") ||
            !tchk(hipMemsetAsync(d_bad.p, 0, sizeof(int), m.stream), "clear flags"))
            return false;
        float* slabs[2] = {nullptr, nullptr};
        hipEvent_t done[2] = {nullptr, nullptr};
        bool pinned = hipHostMalloc((void**)&slabs[0], slab_rows * row_bytes, hipHostMallocDefault) == hipSuccess &&
                      hipHostMalloc((void**)&slabs[1], slab_rows * row_bytes, hipHostMallocDefault) == hipSuccess &&
                      hipEventCreateWithFlags(&done[0], hipEventDisableTiming) == hipSuccess &&
                      hipEventCreateWithFlags(&done[1], hipEventDisableTiming) == hipSuccess;
        std::vector<float> pageable;
        if (!pinned) {  // (no pinned memory left: one pageable slab, synchronous copies)
            (void)hipGetLastError();
            for (int i = 0; i < 2; i++) {
                if (slabs[i]) (void)hipHostFree(slabs[i]);
                if (done[i]) (void)hipEventDestroy(done[i]);
                slabs[i] = nullptr;
                done[i] = nullptr;
            }
            pageable.resize(slab_rows * csr.d);
            slabs[0] = slabs[1] = pageable.data();
        }
        auto release = [&]() {
            if (!pinned) return;
            for (int i = 0; i < 2; i++) {
                (void)hipHostFree(slabs[i]);
                (void)hipEventDestroy(done[i]);
            }
        };
        tlap("staging buffers, pinned slabs");
        unsigned hw = std::thread::hardware_concurrency();
        size_t want_threads = 12;
        if (const char* e = frdev::pricing_env("FR_UPLOAD_THREADS")) want_threads = std::max(1, std::atoi(e));
        const size_t nthreads = std::max<size_t>(1, std::min<size_t>(hw ? hw : 1, rows.size() > 100000 ? want_threads : 1));
        bool used[2] = {false, false};
        size_t turn = 0;
        for (size_t k0 = 0; k0 < rows.size(); k0 += slab_rows, turn ^= 1) {
            const size_t kn = std::min(slab_rows, rows.size() - k0);
            float* slab = slabs[turn];
            // (the slab's previous copy AND the kernel that read its staging buffer are behind this event)
            const auto w0 = std::chrono::steady_clock::now();
            if (pinned && used[turn] && !tchk(hipEventSynchronize(done[turn]), "upload feature rows")) {
                release();
                return false;
            }
            const auto w1 = std::chrono::steady_clock::now();
            t_wait += std::chrono::duration<double, std::milli>(w1 - w0).count();
            auto work = [&](size_t tid) {
                const size_t b0 = k0 + kn * tid / nthreads, b1 = k0 + kn * (tid + 1) / nthreads;
                for (size_t k = b0; k < b1;) {
                    size_t e = k + 1;  // a run of consecutive row ids is one memcpy
                    while (e < b1 && rows[e] == rows[e - 1] + 1) e++;
                    std::memcpy(slab + (k - k0) * csr.d, csr.x + (size_t)rows[k] * csr.d, (e - k) * row_bytes);
                    k = e;
                }
            };
            std::vector<std::thread> pool;
            for (size_t tid = 1; tid < nthreads; tid++) pool.emplace_back(work, tid);
            work(0);
            for (auto& th : pool) th.join();
            t_fill += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w1).count();
            bool ok = pinned ? tchk(hipMemcpyAsync(d_stage[turn].p, slab, kn * row_bytes, hipMemcpyHostToDevice, m.stream), "upload feature rows")
                             : tchk(hipMemcpy(d_stage[turn].p, slab, kn * row_bytes, hipMemcpyHostToDevice), "upload feature rows");
            if (ok) {
                const size_t work_items = kn * m.dq;
                tile_scatter_kernel<<<dim3((unsigned)std::min<size_t>((work_items + 255) / 256, 65535)), 256, 4 * m.dq * sizeof(uint32_t), m.stream>>>(
                    d_stage[turn].p, (uint32_t)kn, (uint32_t)csr.d, (uint32_t)m.dq, d_dst.p + k0, m.xb.p, d_colmax.p, d_bad.p);
                ok = tchk(hipGetLastError(), "tile_scatter_kernel");
            }
            if (ok && pinned) {
                ok = tchk(hipEventRecord(done[turn], m.stream), "upload feature rows");
                used[turn] = true;
            }
            if (!ok) {
                release();
                return false;
            }
        }
        tlap("slab loop (fill + queue + waits)");
        if (timing) fprintf(stderr, "[upload/tiles]   of which filling the slabs %.1f ms, waiting for a slab's turn %.1f ms (%u threads)\n", t_fill, t_wait, (unsigned)nthreads);
        std::vector<uint32_t> colbits(csr.d, 0);
        int bad = 0;
        const bool ok = tchk(hipMemcpyAsync(colbits.data(), d_colmax.p, csr.d * sizeof(uint32_t), hipMemcpyDeviceToHost, m.stream), "column maxima") &&
                        tchk(hipMemcpyAsync(&bad, d_bad.p, sizeof(int), hipMemcpyDeviceToHost, m.stream), "flags") &&
                        tchk(hipStreamSynchronize(m.stream), "upload feature rows");
        tlap("last copies + scatter kernels drained");
        release();
        if (!ok) return false;
        m.nonfinite = bad != 0;
        m.colmax.assign(csr.d, 0.0);
        for (size_t j = 0; j < csr.d; j++) {
            float f;
            std::memcpy(&f, &colbits[j], sizeof(f));
            m.colmax[j] = colbits[j] >= 0x7F800000u ? (double)std::numeric_limits<float>::infinity() : (double)f;
        }
    }
    return true;
}

std::shared_ptr<DeviceDataset> DeviceDataset::create(const HostCSR& csr, std::string* err) {
    std::string e2;
    if (device_count(&e2) <= 0)
        return fail_ds(err, "no MI355X/HIP device available for the fastrank_amd compute path (" +
                                (e2.empty() ? std::string("device count is 0") : e2) + ")");
    if (csr.n == 0 || csr.d == 0 || csr.nq == 0) return fail_ds(err, "empty dataset");
    if (csr.n >= 0xF0000000ull) return fail_ds(err, "dataset too large for 32-bit document positions");
    std::shared_ptr<DeviceDataset> ds(new DeviceDataset());
    Impl& m = *ds->impl_;
    if (hipGetDevice(&m.device) != hipSuccess) return fail_ds(err, "hipGetDevice failed");
    // FR_UPLOAD_TIMING=1: stage times of the one-time upload on stderr
    const bool timing = std::getenv("FR_UPLOAD_TIMING") != nullptr;
    auto tclock = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (!timing) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[upload] %-28s %7.1f ms\n", what, std::chrono::duration<double, std::milli>(now - tclock).count());
        tclock = now;
    };
    // A stream costs ~20 ms to create (a hardware queue each) and the process's first one ~80 ms (the runtime's first touch of
    // the device): 96 ms for the five of them used to be the largest single stage of the upload
    // (profiles/r05_upload_stages.txt).  A helper thread creates them -- the main stream first: the tile thread waits for it,
    // nothing else needs it before the tiles are up -- while this thread builds the host-side tables; the line-search
    // contexts' streams are not needed before the first tick.  Joined before create() returns.
    std::string serr;  // (written by the helper thread, read after its join)
    StreamSignal main_stream;
    std::thread stream_thread([&]() {
        hipError_t e = hipSetDevice(m.device);
        bool at_event = false;
        if (e == hipSuccess) e = m.open_streams(&at_event, &main_stream);
        else main_stream.set(false);
        if (e != hipSuccess) {
            std::lock_guard<std::mutex> lk(main_stream.mu);
            main_stream.ok = false;
            serr = std::string("HIP error: ") + hipGetErrorString(e) + " at hipStreamCreate";
        }
    });
    ThreadJoiner stream_joiner{stream_thread};
    m.n = csr.n;
    m.d = csr.d;
    m.nq = csr.nq;
    m.dq = (csr.d + 3) / 4;

    lap("helper thread started (streams)");
    RunPlan runs;
    if (!plan_runs(csr.qoff, m.nq, run_docs_target(), &runs, err)) return nullptr;
    m.maxlen = runs.maxlen;
    m.np = runs.np;
    m.nruns = runs.run_q0.size();
    // size classes for the general (sort) evaluator, and of the full-ranking bound-and-verify kernel
    // (kernels_fullverify.inc): every query goes to the cheapest (keys per lane, lanes per candidate) class that holds it
    std::vector<uint32_t> qlist, fv_qlist;
    m.size_classes = bucket_queries(runs.qlen, pow2_from_64, &qlist);
    m.fv_classes = fv_build_classes(runs.qlen, &fv_qlist);

    lap("runs, size classes");
    m.perm_host = position_map(csr, runs.qstart, runs.qlen, m.np);
    // (runs on its own thread and stream while this thread builds and uploads the per-position tables below)
    std::string terr;  // (written by the tile thread, read after its join)
    bool tiles_ok = false;
    std::thread tile_thread([&]() { tiles_ok = Impl::upload_tiles(m, csr, timing, main_stream, &terr); });
    ThreadJoiner tile_joiner{tile_thread};
    GainTables gt;
    position_gains(csr, runs.qstart, runs.qlen, m.np, &gt);
    m.labels_small_int = gt.labels_small_int;

    lap("perm / gain / gexp");
    gain_classes(m.perm_host, &gt);
    m.relmask = gt.relmask;

    lap("gain classes, dcgtab");
    term_tables(runs.qstart, runs.qlen, m.maxlen, &gt);
    m.ncls = gt.ncls;
    m.tablen = gt.tablen;
    m.dcg_terms_in_range = verify_terms_in_range(gt.dcgtab.data(), gt.dcgtab.size());

    lap("per-position tables (host)");
    {
        size_t nd = std::max<size_t>(m.maxlen, 64);
        std::vector<double> disc(nd);
        for (size_t i = 0; i < nd; i++) disc[i] = std::log2((double)i + 2.0);
        if (!upload(m.disc, disc, err) || !upload(m.gexp, gt.gexp, err) || !upload(m.gain, gt.gain, err) ||
            !upload(m.qstart, runs.qstart, err) || !upload(m.qlen, runs.qlen, err) || !upload(m.qtight, runs.qtight, err) ||
            !upload(m.perm, m.perm_host, err) || !upload(m.run_q0, runs.run_q0, err) || !upload(m.run_q1, runs.run_q1, err) ||
            !upload(m.run_pos, runs.run_pos, err) || !upload(m.run_docs, runs.run_docs, err) ||
            !upload(m.run_order, runs.run_order, err) || !upload(m.run_lo, std::vector<uint32_t>(m.nruns, 0u), err) ||
            !upload(m.gcls, gt.gcls, err) || !upload(m.dcgtab, gt.dcgtab, err) ||
            !upload(m.qlist, qlist, err) || !upload(m.fv_qlist, fv_qlist, err) || !upload(m.qnpos, gt.qnpos, err) ||
            !upload(m.qnneg, gt.qnneg, err) ||
            !upload(m.termtab, gt.termtab, err))
            return nullptr;
        if (!m.flags.ensure(1, err) || !m.dbgc.ensure(4, err)) return nullptr;
        if (!hip_ok(hipMemset(m.flags.p, 0, sizeof(int)), "clear flags", err)) return nullptr;
        m.qstart_h = runs.qstart;
        m.qlen_h = runs.qlen;
        m.qnpos_h = gt.qnpos;
        m.qnneg_h = gt.qnneg;
    }
    lap("small tables H2D");
    tile_thread.join();
    if (!tiles_ok) return fail_ds(err, terr);
    lap("feature rows H2D + device tiling (remaining wait)");
    {
        // duplicate groups (dataset_layout.hpp: duplicate_groups) from a 64-bit hash of every document's feature row,
        // computed on the device from the tiles just uploaded
        std::vector<uint64_t> row_hash(m.np, 0);
        {
            DevBuf<uint64_t> d_hash;
            if (!d_hash.ensure(m.np, err)) return nullptr;
            row_hash_kernel<<<dim3((unsigned)((m.np + 255) / 256)), 256, 0, m.stream>>>((const float4*)m.xb.p, (uint32_t)m.np, (uint32_t)m.dq, d_hash.p);
            if (!hip_ok(hipGetLastError(), "row_hash_kernel", err) ||
                !hip_ok(hipMemcpyAsync(row_hash.data(), d_hash.p, m.np * sizeof(uint64_t), hipMemcpyDeviceToHost, m.stream), "row hashes", err) ||
                !hip_ok(hipStreamSynchronize(m.stream), "row hashes", err))
                return nullptr;
        }
        unsigned hw = std::thread::hardware_concurrency();
        const size_t nthreads = std::max<size_t>(1, std::min<size_t>(hw ? hw : 1, m.np > 200000 ? 16 : 1));
        const DupGroups dg = duplicate_groups(row_hash, csr, m.perm_host, runs.qstart, runs.qlen, gt.gcls, gt.cls_gain.size(),
                                              frdev::path_env("FR_NO_DUP_GROUPS") != nullptr, nthreads);
        m.dup_groups = dg.dup_groups;
        m.key_bits = dg.key_bits;
        m.key_cls_bits = dg.key_cls_bits;
        m.verify_xs = dg.verify_xs;
        if (!upload(m.gkey, dg.gkey16, err)) return nullptr;
    }
    lap("duplicate groups (device hash, host grouping)");
    {
        // the walk tiles (kernels_order.inc; build_walk_tiles), then the (query, walk tile) segment of every position and the
        // static visiting-order tables
        WalkTileLayout wl = build_walk_tiles(runs.run_pos, runs.run_q0, runs.run_q1, runs.qstart, runs.qlen, m.np);
        m.wt_start_h = std::move(wl.wt_start);
        m.nwt = m.wt_start_h.size() - 1;
        if (!upload(m.segtab, wl.seg, err) || !upload(m.wt_start, m.wt_start_h, err) || !upload(m.run_wt0, wl.run_wt0, err) || !upload(m.wofs, wl.wofs, err)) return nullptr;
        if (!m.build_order_tables(err)) return nullptr;
        if (!m.build_columns(err)) return nullptr;
    }
    lap("visiting-order tables (device)");
    stream_thread.join();
    if (!main_stream.ok) return fail_ds(err, serr);
    lap("line-search streams (helper thread, remaining wait)");
    return ds;
}

// One line on stderr, once per process and message, when an optional device copy could not be made and a slower path takes
// over (results are the same; INTEGRATION.md section 6 lists what a dataset takes in HBM).
static void warn_degraded(const char* what) {
    static std::mutex mu;
    static std::vector<std::string> said;
    std::lock_guard<std::mutex> lk(mu);
    for (const std::string& s : said)
        if (s == what) return;
    said.emplace_back(what);
    fprintf(stderr, "[fastrank_amd] warning: %s\n", what);
}

// xslot + the column statistics of the host's lane-class rule, from the tiles (a dataset that owns its matrix).
// FR_VERIFY_ORDER=0, or no HBM for the table (a quarter of the tiles' size): the verify kernel walks in storage order.
bool DeviceDataset::Impl::build_order_tables(std::string* err) {
    Impl& m = *this;
    const char* oe = std::getenv("FR_VERIFY_ORDER");
    if ((oe != nullptr && oe[0] == '0') || m.nonfinite || m.dq * 4 > 2048) return true;
    {
        std::string e2;
        if (!m.xslot.ensure(m.d * m.np, &e2)) {
            (void)hipGetLastError();
            warn_degraded("no HBM for the visiting-order tables (a quarter of the matrix): the NDCG@k verify kernel walks in storage order");
            return true;
        }
    }
    const uint32_t ntiles = (uint32_t)(m.np / 64);
    {
        ProfScope ps("xslot_kernel", m.stream);
        xslot_kernel<<<dim3((unsigned)m.nwt, (unsigned)((m.dq + ORDER_OQ - 1) / ORDER_OQ)), WAVE, 0, m.stream>>>(
            (const float4*)m.xb.p, m.segtab.p, m.wt_start.p, (uint32_t)m.np, (uint32_t)m.dq, (uint32_t)m.d, m.xslot.p);
    }
    FR_HIP(hipGetLastError());
    std::vector<ColStats> init(m.d);
    for (ColStats& c : init) {
        c.sum = c.sumsq = 0.0;
        c.mn = std::numeric_limits<float>::infinity();
        c.mx = -std::numeric_limits<float>::infinity();
        c.at_min = c.at_max = 0;
    }
    DevBuf<ColStats> dst;
    if (!upload(dst, init, err)) return false;
    for (int pass = 0; pass < 2; pass++)
        colstats_kernel<<<dim3(128, (unsigned)m.dq), 256, 0, m.stream>>>((const float4*)m.xb.p, m.segtab.p, ntiles, (uint32_t)m.dq, (uint32_t)m.d, pass, dst.p);
    FR_HIP(hipGetLastError());
    FR_HIP(hipMemcpyAsync(init.data(), dst.p, m.d * sizeof(ColStats), hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipStreamSynchronize(m.stream));
    m.colstd.assign(m.d, 0.0);
    m.colmode.assign(m.d, 0);
    const double nd = (double)std::max<size_t>(m.n, 1);
    for (size_t j = 0; j < m.d; j++) {
        const double mean = init[j].sum / nd, var = init[j].sumsq / nd - mean * mean;
        m.colstd[j] = var > 0.0 ? std::sqrt(var) : 0.0;
        m.colmode[j] = (uint8_t)(((double)init[j].at_max > 0.1 * nd ? 1 : 0) | ((double)init[j].at_min > 0.1 * nd ? 2 : 0));
    }
    m.colstats_h = std::move(init);
    return true;
}

// The column-major copy of the tiles (kernels_order.inc: xcol_kernel): as large as the matrix again -- HBM is what this
// device has.  FR_XCOL=0, or no room for it: the resident line search reads its column out of the tiles.
bool DeviceDataset::Impl::build_columns(std::string* err) {
    Impl& m = *this;
    const char* xe = std::getenv("FR_XCOL");
    if ((xe != nullptr && xe[0] == '0') || m.np == 0 || m.d == 0) return true;
    {
        std::string e2;
        if (!m.xcol.ensure(m.d * m.np, &e2)) {
            (void)hipGetLastError();
            warn_degraded("no HBM for the column-major copy of the matrix (as large as the matrix again): coordinate ascent runs without "
                          "resident sums -- every line search forms its sums from the tiles, several times slower");
            return true;
        }
    }
    ProfScope ps("xcol_kernel", m.stream);
    xcol_kernel<<<dim3((unsigned)(m.np / 64), (unsigned)((m.dq + ORDER_OQ - 1) / ORDER_OQ)), WAVE, 0, m.stream>>>((const float4*)m.xb.p, (uint32_t)m.np,
                                                                                                               (uint32_t)m.dq, (uint32_t)m.d, m.xcol.p);
    FR_HIP(hipGetLastError());
    return true;
}

bool DeviceDataset::shares_parent_matrix() const { return (bool)impl_->parent; }

// ---- read-back of the device form (device.hpp: for the tests that hold every table to its definition) ------------------
std::vector<std::pair<std::string, uint64_t>> DeviceDataset::debug_form_scalars() const {
    const Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(impl_->mu);
    auto addr = [](const auto& b) { return (uint64_t) reinterpret_cast<uintptr_t>(b.p); };
    return {{"np", m.np}, {"dq", m.dq}, {"d", m.d}, {"n", m.n}, {"nq", m.nq}, {"nonfinite", m.nonfinite ? 1u : 0u},
            {"nruns", m.nruns}, {"nwt", m.nwt}, {"nvtiles", m.nvtiles}, {"nwlist", m.nwlist}, {"maxlen", m.maxlen},
            {"ncls", m.ncls}, {"key_bits", m.key_bits}, {"key_cls_bits", m.key_cls_bits}, {"dup_groups", m.dup_groups},
            {"no_document", IDX_INVALID}, {"walk_tile", WT}, {"dcg_ranks", (uint64_t)LS_KT}, {"colstats_bytes", sizeof(ColStats)},
            {"shares_parent_matrix", m.parent ? 1u : 0u}, {"device", (uint64_t)m.device},
            // (addresses, to be compared and never followed: a view's tables ARE its parent's)
            {"xb_addr", addr(m.xb)}, {"xcol_addr", addr(m.xcol)}, {"xslot_addr", addr(m.xslot)}, {"segtab_addr", addr(m.segtab)},
            {"gkey_addr", addr(m.gkey)}, {"perm_addr", addr(m.perm)}};
}

bool DeviceDataset::debug_form_table(const std::string& name, std::vector<unsigned char>* out, bool* present, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    // what create() queued last (xcol_kernel) may still be running; a view's tables were written on its parent's stream
    if (m.parent) FR_HIP(hipStreamSynchronize(m.parent->impl_->stream));
    FR_HIP(hipStreamSynchronize(m.stream));
    out->clear();
    *present = true;
    auto dev = [&](const auto& b, size_t count) {  // `count` elements of a device table (absent: an optional copy that was not made)
        using T = std::remove_pointer_t<decltype(b.p)>;
        if (b.p == nullptr || count == 0 || count > b.cap) {
            *present = false;
            return true;
        }
        out->resize(count * sizeof(T));
        FR_HIP(hipMemcpy(out->data(), b.p, out->size(), hipMemcpyDeviceToHost));
        return true;
    };
    auto host = [&](const auto& v) {
        using T = typename std::remove_reference_t<decltype(v)>::value_type;
        if (v.empty()) {
            *present = false;
            return true;
        }
        out->resize(v.size() * sizeof(T));
        std::memcpy(out->data(), v.data(), out->size());
        return true;
    };
    if (name == "xb") return dev(m.xb, m.np / 64 * m.dq * 256);
    if (name == "xcol") return dev(m.xcol, m.d * m.np);
    if (name == "xslot") return dev(m.xslot, m.d * m.np);
    if (name == "perm") return dev(m.perm, m.np);
    if (name == "perm_host") return host(m.perm_host);
    if (name == "gain") return dev(m.gain, m.np);
    if (name == "gexp") return dev(m.gexp, m.np);
    if (name == "gcls") return dev(m.gcls, m.np);
    if (name == "gkey") return dev(m.gkey, m.np);
    if (name == "segtab") return dev(m.segtab, m.np);
    if (name == "wofs") return dev(m.wofs, m.np);
    if (name == "wt_start") return dev(m.wt_start, m.nwt + 1);
    if (name == "qstart") return dev(m.qstart, m.nq);
    if (name == "qlen") return dev(m.qlen, m.nq);
    if (name == "qtight") return dev(m.qtight, m.nq + 1);
    if (name == "run_q0") return dev(m.run_q0, m.nruns);
    if (name == "run_q1") return dev(m.run_q1, m.nruns);
    if (name == "run_pos") return dev(m.run_pos, m.nruns);
    if (name == "run_docs") return dev(m.run_docs, m.nruns);
    if (name == "run_lo") return dev(m.run_lo, m.nruns);
    if (name == "run_order") return dev(m.run_order, m.nruns);
    if (name == "run_wt0") return dev(m.run_wt0, m.nruns);
    if (name == "vtiles") return dev(m.vtiles, m.nvtiles);
    if (name == "wlist") return dev(m.wlist, m.nwlist);
    if (name == "dcgtab") return dev(m.dcgtab, m.ncls * LS_KT);
    if (name == "colmax") return host(m.colmax);
    if (name == "colstd") return host(m.colstd);
    if (name == "colmode") return host(m.colmode);
    if (name == "colstats") return host(m.colstats_h);
    if (err) *err = "debug_form_table: no table named " + name;
    return false;
}

// A second copy of a dataset that owns its matrix, on another device (or a second context on the same one): everything
// create() built -- the feature tiles, the per-position and per-query tables -- is copied device to device
// (hipMemcpyPeer: over xGMI between two GPUs of a node), nothing is uploaded or recomputed from the host's matrix.
// The copy starts with empty work buffers and its own streams.  This is how train_model spreads the restarts of one
// request over the GPUs of a node (src/coordinate_ascent.rs:215-225 does it with rayon over the host's cores).
std::shared_ptr<DeviceDataset> DeviceDataset::replicate(const std::shared_ptr<DeviceDataset>& src, int device, std::string* err) {
    if (!src || src->impl_->parent) return fail_ds(err, "replicate: the source must own its matrix");
    Impl& sm = *src->impl_;
    // (no lock on the source for the copies: what create() left in HBM and its host-side description never change
    // afterwards, so the callers' threads -- one per destination -- really copy at the same time, each peer reading
    // the source over its own link; the source may run kernels of its own meanwhile)
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail_ds(err, "replicate: no such device");
    int prev = 0;
    (void)hipGetDevice(&prev);
    struct Restore {
        int d;
        ~Restore() { (void)hipSetDevice(d); }
    } restore{prev};
    if (hipSetDevice(device) != hipSuccess) return fail_ds(err, "replicate: hipSetDevice failed");
    if (device != sm.device) {  // direct peer copies where the link allows them (otherwise the runtime stages through the host)
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, device, sm.device) == hipSuccess && can) {
            const hipError_t e = hipDeviceEnablePeerAccess(sm.device, 0);
            if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
            (void)hipGetLastError();
        }
    }
    std::shared_ptr<DeviceDataset> ds(new DeviceDataset());
    Impl& m = *ds->impl_;
    m.device = device;
    if (!m.open_streams(err)) return nullptr;
    // ---- host-side description: everything, as the source holds it now (verify_xs included: whatever its trainers raised it
    // to).  What is not part of it keeps its default: a replica has no parent and visits its whole position space (nvtiles = 0).
    static_cast<DatasetDesc&>(m) = sm;
    // ---- everything create() left in HBM, device to device
    bool ok = true;
    auto copy = [&](auto& dst, const auto& from, const char* what) {
        if (!ok || from.p == nullptr || from.cap == 0) return;
        if (!dst.ensure(from.cap, err)) {
            ok = false;
            return;
        }
        ok = hip_ok(hipMemcpyPeerAsync(dst.p, device, from.p, sm.device, from.bytes(), m.stream), what, err);
    };
    copy(m.xb, sm.xb, "replicate feature tiles");
    copy(m.gain, sm.gain, "replicate gain");
    copy(m.gexp, sm.gexp, "replicate gexp");
    copy(m.disc, sm.disc, "replicate disc");
    copy(m.qstart, sm.qstart, "replicate qstart");
    copy(m.qlen, sm.qlen, "replicate qlen");
    copy(m.qtight, sm.qtight, "replicate qtight");
    copy(m.perm, sm.perm, "replicate perm");
    copy(m.run_q0, sm.run_q0, "replicate run_q0");
    copy(m.run_q1, sm.run_q1, "replicate run_q1");
    copy(m.run_pos, sm.run_pos, "replicate run_pos");
    copy(m.run_docs, sm.run_docs, "replicate run_docs");
    copy(m.run_order, sm.run_order, "replicate run_order");
    copy(m.run_lo, sm.run_lo, "replicate run_lo");
    copy(m.gcls, sm.gcls, "replicate gcls");
    copy(m.gkey, sm.gkey, "replicate gkey");
    copy(m.segtab, sm.segtab, "replicate segtab");
    copy(m.wt_start, sm.wt_start, "replicate wt_start");
    copy(m.run_wt0, sm.run_wt0, "replicate run_wt0");
    copy(m.wofs, sm.wofs, "replicate wofs");
    // the optional copies (create() itself goes without them when HBM is short): a replica that cannot hold them is a slower
    // replica, not a failed one -- xcol first, the resident line search cannot do without it
    auto copy_optional = [&](auto& dst, const auto& from, const char* what, const char* degraded) {
        if (!ok || from.p == nullptr || from.cap == 0) return;
        std::string e2;
        if (!dst.ensure(from.cap, &e2)) {
            (void)hipGetLastError();
            warn_degraded(degraded);
            return;
        }
        ok = hip_ok(hipMemcpyPeerAsync(dst.p, device, from.p, sm.device, from.bytes(), m.stream), what, err);
    };
    copy_optional(m.xcol, sm.xcol, "replicate xcol", "a device replica has no HBM for the column-major copy of the matrix: its line searches form their sums from the tiles");
    copy_optional(m.xslot, sm.xslot, "replicate xslot", "a device replica has no HBM for the visiting-order tables: its NDCG@k verify kernel walks in storage order");
    copy(m.qlist, sm.qlist, "replicate qlist");
    copy(m.fv_qlist, sm.fv_qlist, "replicate fv_qlist");
    copy(m.qnpos, sm.qnpos, "replicate qnpos");
    copy(m.qnneg, sm.qnneg, "replicate qnneg");
    copy(m.termtab, sm.termtab, "replicate termtab");
    copy(m.dcgtab, sm.dcgtab, "replicate dcgtab");
    if (!ok) return nullptr;
    if (!m.flags.ensure(1, err) || !m.dbgc.ensure(4, err)) return nullptr;
    if (!hip_ok(hipMemsetAsync(m.flags.p, 0, sizeof(int), m.stream), "clear flags", err) ||
        !hip_ok(hipStreamSynchronize(m.stream), "replicate", err))
        return nullptr;
    return ds;
}

int DeviceDataset::device_ordinal() const { return impl_->device; }

std::shared_ptr<DeviceDataset> DeviceDataset::create_view(const std::shared_ptr<DeviceDataset>& parent, const HostCSR& csr,
                                                          const std::vector<uint32_t>& parent_query, std::string* err) {
    if (!parent || parent->impl_->parent) return fail_ds(err, "create_view: the parent must own its matrix");
    const Impl& pm = *parent->impl_;
    if (csr.n == 0 || csr.nq == 0 || parent_query.size() != csr.nq) return fail_ds(err, "create_view: empty view");
    std::shared_ptr<DeviceDataset> ds(new DeviceDataset());
    Impl& m = *ds->impl_;
    m.device = pm.device;
    if (!hip_ok(hipSetDevice(m.device), "hipSetDevice", err)) return nullptr;
    if (!m.open_streams(err)) return nullptr;
    m.parent = parent;
    m.n = csr.n;
    m.d = pm.d;
    m.dq = pm.dq;
    m.nq = csr.nq;
    m.np = pm.np;  // the parent's position space
    m.nonfinite = pm.nonfinite;
    m.colmax = pm.colmax;  // maxima over a superset of the view's documents: still upper bounds
    m.ncls = pm.ncls;
    m.tablen = pm.tablen;
    m.dcg_terms_in_range = pm.dcg_terms_in_range;
    m.relmask = pm.relmask;
    // ---- the view's queries, runs, tiles and walk tiles inside the parent's position space
    RunPlan v;
    if (!plan_view_runs(pm.qstart_h, pm.qlen_h, pm.perm_host, pm.wt_start_h, csr, parent_query, run_docs_target(), &v, err)) return nullptr;
    m.maxlen = v.maxlen;
    m.perm_host = std::move(v.perm_host);
    m.nruns = v.run_q0.size();
    std::vector<uint32_t> qnpos(m.nq), qnneg(m.nq);
    for (size_t q = 0; q < m.nq; q++) {
        qnpos[q] = pm.qnpos_h[parent_query[q]];
        qnneg[q] = pm.qnneg_h[parent_query[q]];
    }
    std::vector<uint32_t> qlist, fv_qlist;
    m.size_classes = bucket_queries(v.qlen, pow2_from_64, &qlist);
    m.fv_classes = fv_build_classes(v.qlen, &fv_qlist);
    // ---- shared with the parent: the feature tiles and every per-document / per-class array
    m.xb.alias(pm.xb);
    m.gain.alias(pm.gain);
    m.labels_small_int = pm.labels_small_int;
    m.gexp.alias(pm.gexp);
    m.gcls.alias(pm.gcls);
    m.gkey.alias(pm.gkey);
    m.xslot.alias(pm.xslot);    // (segments are (query, walk tile) pairs of the parent's position space: the view's queries keep theirs)
    m.segtab.alias(pm.segtab);
    m.wt_start.alias(pm.wt_start);
    m.wofs.alias(pm.wofs);
    m.wt_start_h = pm.wt_start_h;
    m.nwt = pm.nwt;
    m.nwlist = v.wlist.size();
    m.xcol.alias(pm.xcol);
    m.colstd = pm.colstd;
    m.colmode = pm.colmode;
    m.colstats_h = pm.colstats_h;
    m.dup_groups = pm.dup_groups;
    m.key_bits = pm.key_bits;
    m.key_cls_bits = pm.key_cls_bits;
    m.verify_xs = pm.verify_xs;
    m.perm.alias(pm.perm);
    m.disc.alias(pm.disc);
    m.dcgtab.alias(pm.dcgtab);
    m.termtab.alias(pm.termtab);
    if (!upload(m.qstart, v.qstart, err) || !upload(m.qlen, v.qlen, err) || !upload(m.qtight, v.qtight, err) ||
        !upload(m.run_q0, v.run_q0, err) || !upload(m.run_q1, v.run_q1, err) || !upload(m.run_pos, v.run_pos, err) ||
        !upload(m.run_docs, v.run_docs, err) || !upload(m.run_order, v.run_order, err) || !upload(m.run_lo, v.run_lo, err) ||
        !upload(m.qlist, qlist, err) || !upload(m.fv_qlist, fv_qlist, err) || !upload(m.qnpos, qnpos, err) ||
        !upload(m.qnneg, qnneg, err) || !upload(m.vtiles, v.vtiles, err) || !upload(m.run_wt0, v.run_wt0, err) || !upload(m.wlist, v.wlist, err))
        return nullptr;
    m.nvtiles = frdev::pricing_env("FR_VIEW_ALL_TILES") ? 0 : v.vtiles.size();  // (FR_VIEW_ALL_TILES=1: round 2's behaviour, for A/B runs)
    if (!m.flags.ensure(1, err) || !m.dbgc.ensure(4, err)) return nullptr;
    if (!hip_ok(hipMemset(m.flags.p, 0, sizeof(int)), "clear flags", err)) return nullptr;
    m.qstart_h = std::move(v.qstart);
    m.qlen_h = std::move(v.qlen);
    m.qnpos_h = qnpos;
    m.qnneg_h = qnneg;
    return ds;
}

