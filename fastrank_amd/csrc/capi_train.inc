// capi.cpp: training.  The request's wire form, train_model's learners over the devices of a node, the restart records of the
// exchange, and the extensions that train: shards, the steppable trainer, selection, the last call's statistics.
namespace {

std::mutex g_stats_mu;  // fr_last_train_stats
fr::TrainStats g_last_stats;

Value rccl_report_to_json(const frdev::RcclReport& r) {
    Value o = Value::object();
    o.set("ran", Value::boolean(r.ran));
    o.set("ranks", Value::uint((uint64_t)r.ranks));
    Value d = Value::array();
    for (int x : r.devices) d.push(Value::uint((uint64_t)x));
    o.set("devices", std::move(d));
    o.set("block_doubles", Value::uint((uint64_t)r.block_doubles));
    if (r.ran) {
        o.set("us", Value::number(r.us));
        o.set("first_us", Value::number(r.first_us));
        o.set("init_us", Value::number(r.init_us));
        o.set("matches_host_gather", Value::boolean(r.matches_host_gather));
        o.set("library", Value::string(r.library));
    } else {
        o.set("reason", Value::string(r.reason));
    }
    return o;
}

Value stats_to_json(const fr::TrainStats& s) {
    Value o = Value::object();
    if (s.rccl_set) o.set("rccl", rccl_report_to_json(s.rccl));
    o.set("useful_evals", Value::uint(s.useful_evals));
    o.set("raw_evals", Value::uint(s.raw_evals));
    o.set("ticks", Value::uint(s.ticks));
    o.set("groups", Value::uint(s.groups));
    o.set("seconds", Value::number(s.seconds));
    o.set("path", Value::string(s.path));
    o.set("restarts", Value::uint(s.restarts));
    o.set("verify_pairs", Value::uint(s.verify_pairs));
    o.set("verify_redone", Value::uint(s.verify_redone));
    o.set("exact_ticks", Value::uint(s.exact_ticks));
    o.set("exact_groups", Value::uint(s.exact_groups));
    o.set("verify_redo_entries", Value::uint(s.verify_redo_entries));
    o.set("chain_runs", Value::uint(s.chain_runs));
    o.set("chain_visits", Value::uint(s.chain_visits));
    o.set("rank_slots_on", Value::uint(s.rank_slots_on));
    o.set("rank_slots_off", Value::uint(s.rank_slots_off));
    o.set("line_searches", Value::uint(s.line_searches));
    o.set("audit_values", Value::uint(s.audit_values));
    o.set("audit_mismatches", Value::uint(s.audit_mismatches));
    o.set("devices", Value::uint(s.devices));
    o.set("refills", Value::uint(s.refills));
    if (s.device >= 0) o.set("device", Value::uint((uint64_t)s.device));
    return o;
}

enum class Learner { CoordinateAscent, RandomForest, LambdaMART };

struct ParsedRequest {
    std::string measure;
    Learner learner = Learner::CoordinateAscent;
    fr::CAParams ca;
    fr::RFParams rf;
    fr::LambdaMARTParams lm;
    bool has_qrel = false;
    fr::QRel qrel;
};

// src/json_api.rs:13-34 TrainRequest
// (has_valid: the call brings a validation dataset, LambdaMARTParams::from_json)
ParsedRequest parse_train_request(const std::string& text, bool has_valid = false) {
    Value v = parse_json_or_fail(text);
    if (!v.is_object()) fr::fail_raw("Error(\"invalid type: expected struct TrainRequest\", line: 1, column: 1)");
    ParsedRequest rq;
    const Value& m = fr::json_field(v, "measure");
    if (!m.is_string()) fr::fail_raw("Error(\"invalid type: expected a string for measure\", line: 1, column: 1)");
    rq.measure = m.s;
    const auto& var = fr::json_variant(fr::json_field(v, "params"), "FastRankModelParams");
    if (var.first == "CoordinateAscent") {
        rq.learner = Learner::CoordinateAscent;
        rq.ca = fr::CAParams::from_json(var.second);
    } else if (var.first == "RandomForest") {
        rq.learner = Learner::RandomForest;
        rq.rf = fr::RFParams::from_json(var.second);
    } else if (var.first == "LambdaMART") {
        rq.learner = Learner::LambdaMART;
        rq.lm = fr::LambdaMARTParams::from_json(var.second, has_valid);
        fr::lambdamart_check_measure(rq.measure);
    } else {
        fr::fail_raw("Error(\"unknown variant `" + var.first +
                     "`, expected one of `CoordinateAscent`, `RandomForest`, `LambdaMART`\", line: 1, column: 1)");
    }
    const Value* j = v.find("judgments");
    if (j && !j->is_null()) {
        rq.has_qrel = true;
        rq.qrel = fr::qrel_from_json(*j);
    }
    return rq;
}

std::vector<fr::TrainStats> g_last_per_device;  // one entry per device of the last multi-device train_model call
Value g_last_lambdamart;                         // the last LambdaMART training's own numbers (null after any other training)
static void set_last_stats(const fr::TrainStats& st, std::vector<fr::TrainStats> per_device = {}) {
    std::lock_guard<std::mutex> lk(g_stats_mu);
    g_last_stats = st;
    g_last_per_device = std::move(per_device);
    g_last_lambdamart = Value::null();
}

// Per-trainer bound on the restarts kept live at once (FR_RESTART_SLOTS, default 64): a request with more restarts than
// that per device runs them through the restart queue, converged restarts handing their places to the next ids -- the
// resident sums, result matrices and launch width stay those of 64 restarts however many the request names.
static uint32_t restart_slots_max() {
    const char* e = std::getenv("FR_RESTART_SLOTS");
    const long v = e ? std::atol(e) : 64;
    return (uint32_t)std::min<long>(std::max<long>(v, 1), 1 << 20);
}

// the restarts `queue` still holds (at most `capacity` live at a time) on one device-side copy of the view (slot, device:
// DatasetView::device_ptr)
static std::vector<fr::RestartResult> train_ca_queue(const std::shared_ptr<fr::DatasetView>& view, const ParsedRequest& rq,
                                                     const fr::Evaluator& ev, std::shared_ptr<fr::RestartQueue> queue, uint32_t capacity,
                                                     int slot, int device, fr::TrainStats* stats_out) {
    auto t0 = std::chrono::steady_clock::now();
    fr::CATrainer trainer(view, ev, rq.ca, std::move(queue), capacity, fr::QueryShard(), slot, device);
    while (trainer.run(64, nullptr)) {
    }
    trainer.stats().seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    trainer.stats().device = device;
    if (stats_out) *stats_out = trainer.stats();
    return trainer.results();
}

fr::Model train_ca(const std::shared_ptr<fr::DatasetView>& view, const ParsedRequest& rq, uint32_t rbegin,
                   uint32_t rend, std::vector<fr::RestartResult>* hist_out) {
    fr::Evaluator ev = fr::make_evaluator(*view, rq.measure, rq.has_qrel ? &rq.qrel : nullptr);
    if (view->host_csr().nq == 0) fr::fail_str("assertion failed: !data.queries().is_empty()");
    fr::TrainStats st;
    rend = std::min(rend, rq.ca.num_restarts);
    std::vector<fr::RestartResult> hist =
        train_ca_queue(view, rq, ev, std::make_shared<fr::RestartQueue>(rbegin, rend), restart_slots_max(), 0, -1, &st);
    set_last_stats(st);
    fr::Model m;
    if (hist_out) {
        *hist_out = hist;
    } else {
        m = fr::ca_select(hist, rq.ca.output_ensemble);
    }
    return m;
}

// ---- train_model over the devices of a node -------------------------------------------------------------------------
// The reference fans a request's restarts out over the host's cores inside the call (rayon, src/coordinate_ascent.rs:
// 215-225).  Here the fan-out is over GPUs: FR_DEVICES (a comma list of ordinals; the same ordinal twice = two contexts
// on one device) or, if unset, the device chosen with fr_set_device or else every visible device.  Restart ids are
// block-partitioned (the child seeds are drawn in order from the master generator by every trainer, :211-213), each
// device gets its own host thread, trainer and device-side copy of the dataset -- made device to device from the first
// one (DeviceDataset::replicate, hipMemcpyPeer over xGMI) -- and the results are gathered in host memory and selected
// like a single trainer's history (last maximum, or the score-weighted ensemble: :232-251).  No collective: this is
// the in-process form of native.train_model_distributed.
static std::atomic<int> g_pinned_device{-1};  // fr_set_device: an explicit choice of ONE device for this process

static std::vector<int> parse_device_list(const char* e, int count) {
    std::vector<int> devs;
    const char* p = e;
    while (*p) {
        while (*p == ',' || *p == ' ') p++;
        if (!*p) break;
        char* end = nullptr;
        const long v = std::strtol(p, &end, 10);
        if (end == p) fr::fail_str(std::string("FR_DEVICES: not a list of device ordinals: ") + e);
        if (v < 0 || v >= count) fr::fail_str("FR_DEVICES: no device " + std::to_string(v) + " (" + std::to_string(count) + " visible)");
        devs.push_back((int)v);
        p = end;
    }
    if (devs.empty()) fr::fail_str("FR_DEVICES is empty");
    return devs;
}

std::vector<int> fr_train_devices() {
    const int count = frdev::device_count(nullptr);
    if (const char* e = std::getenv("FR_DEVICES")) return parse_device_list(e, count);
    if (const int pinned = g_pinned_device.load(); pinned >= 0) return {pinned};
    std::vector<int> devs;
    for (int d = 0; d < count; d++) devs.push_back(d);
    return devs;
}

// contiguous block partition of restart ids (first parts take the remainder), as native.shard_bounds
static void restart_block(uint32_t R, uint32_t part, uint32_t parts, uint32_t* b, uint32_t* e) {
    const uint32_t base = R / parts, rem = R % parts;
    *b = part * base + std::min(part, rem);
    *e = *b + base + (part < rem ? 1u : 0u);
}

// which entry of the device list trains which restarts, and on which device-side copy (slot 0 = the copy that exists
// on `primary_dev`, if that device is listed)
struct DevicePlan {
    std::vector<int> devs, slot;
    std::vector<uint32_t> begin, end;
};
static DevicePlan plan_devices(std::vector<int> devs, uint32_t R, int primary_dev) {
    DevicePlan pl;
    if (devs.size() > R) devs.resize(std::max<uint32_t>(R, 1));
    const size_t k = devs.size();
    pl.devs = devs;
    pl.slot.assign(k, -1);
    pl.begin.assign(k, 0);
    pl.end.assign(k, 0);
    int next_slot = 1;
    bool primary_used = false;
    for (size_t i = 0; i < k; i++) {
        if (!primary_used && devs[i] == primary_dev) pl.slot[i] = 0, primary_used = true;
        else pl.slot[i] = next_slot++;
        restart_block(R, (uint32_t)i, (uint32_t)k, &pl.begin[i], &pl.end[i]);
    }
    return pl;
}

// Fewest restarts a device must get before the DEFAULT device list (every visible device) adds it to a request
// (FR_MIN_RESTARTS_PER_DEVICE, default 4; an explicit FR_DEVICES is taken as given).  Measured on one MI355X at the 30K
// shape (tools/tick_sweep.py, profiles/r04_tick_vs_groups.json): a tick of G line groups takes 0.11 + 0.083 G ms
// (0.21 / 0.28 / 0.34 / 0.43 / 0.74 / 2.75 ms at G = 1 / 2 / 3 / 4 / 8 / 32), i.e. a device with one restart delivers 40 %
// of the evaluations per second it delivers with 32, with four 80 %; every further device also costs a device-to-device
// copy of the dataset the first time (2.2 GB) and the runtime's start-up there.  With the floor at 4 the reference's
// default request (5 restarts, coordinate_ascent.rs:29) stays on one GPU and 32 restarts spread over 8.
static uint32_t min_restarts_per_device() {
    const char* e = std::getenv("FR_MIN_RESTARTS_PER_DEVICE");
    const long v = e ? std::atol(e) : 4;
    return (uint32_t)std::min<long>(std::max<long>(v, 1), 1 << 20);
}

// The device list of one train_model call over `units` independent pieces of work (restarts, trees), with the view's
// device-side copies made: an empty / one-entry plan means "train on one device" (slot 0 = the view's first device
// form; slot 1 = a copy on the one device an explicit list names when the first form lives elsewhere).
// slots_max (coordinate ascent): the restarts one trainer keeps live; the list is cut to the entries that get restarts when
// every trainer takes its share from the one queue at the start (ADVICE r04: 5 restarts over 4 devices are 2 + 2 + 1, the
// fourth entry would have made a dataset copy and an empty trainer).
static DevicePlan devices_for_request(const std::shared_ptr<fr::DatasetView>& view, uint32_t units, uint32_t min_units_per_device = 1,
                                      uint32_t slots_max = 0) {
    std::vector<int> devs = fr_train_devices();
    const bool explicit_list = std::getenv("FR_DEVICES") != nullptr;
    if (!explicit_list) {
        // a small matrix is not worth a context on every GPU (each costs a device-to-device copy and, the first time, the
        // runtime's per-device start-up), and neither is a device that would get fewer than the floor of units
        if (view->instances.size() * (size_t)view->core->d < (size_t(1) << 23)) devs.resize(std::min<size_t>(devs.size(), 1));
        const size_t by_floor = std::max<size_t>(1, units / std::max<uint32_t>(min_units_per_device, 1));
        devs.resize(std::min(devs.size(), by_floor));
    }
    if (devs.size() > units) devs.resize(std::max<uint32_t>(units, 1));
    if (slots_max > 0 && devs.size() > 1) {
        const uint32_t cap = std::max<uint32_t>(1, std::min<uint32_t>(slots_max, (uint32_t)((units + devs.size() - 1) / devs.size())));
        devs.resize(std::min<size_t>(devs.size(), (units + cap - 1) / cap));
    }
    auto single = [&](const std::vector<int>& d, bool pin) {
        if (d.empty()) return plan_devices(d, units, -1);
        if (pin) {
            std::string err;
            if (!frdev::set_device(d[0], &err)) fr::fail_str(err);
        }
        // an explicit choice of a device other than the one the first device form already lives on: train on a copy there
        const int have = view->built_on_device();
        const int primary = (pin && have >= 0 && have != d[0]) ? have : d[0];
        return plan_devices(std::vector<int>(1, d[0]), units, primary);
    };
    if (devs.size() <= 1) return single(devs, explicit_list || g_pinned_device.load() >= 0);
    if (view->host_csr().nq == 0) return single(devs, false);  // (the trainer reports the empty dataset its own way)
    // slot 0 is the device form the view already has (or builds now, on the first listed device); every other entry of
    // the list gets the next slot
    {
        std::string err;
        if (!frdev::set_device(devs[0], &err)) fr::fail_str(err);
    }
    // The copies are made at the same time (one host thread per entry), then the training runs concurrently.
    // A device the dataset cannot be copied to is an error when FR_DEVICES named it; of the default "every visible
    // device" it is simply left out (the request then trains on the devices that took a copy).
    const int primary_dev = view->device_ptr()->device_ordinal();
    for (;;) {
        DevicePlan pl = plan_devices(devs, units, primary_dev);
        std::vector<int> kept;
        std::exception_ptr first_error;
        // every entry's copy at the same time (each on its own device and stream, reading the first device over its own
        // link); the slots are disjoint
        std::vector<std::exception_ptr> errs(pl.devs.size());
        {
            std::vector<std::thread> copiers;
            auto copy_to = [&](size_t i) {
                try {
                    (void)view->device_ptr(pl.slot[i], pl.devs[i]);
                } catch (...) {
                    errs[i] = std::current_exception();
                }
            };
            (void)view->device_ptr();  // (the first copy exists before anything reads it)
            for (size_t i = 1; i < pl.devs.size(); i++) copiers.emplace_back(copy_to, i);
            copy_to(0);
            for (auto& th : copiers) th.join();
        }
        for (size_t i = 0; i < pl.devs.size(); i++) {
            if (!errs[i]) kept.push_back(pl.devs[i]);
            else if (!first_error) first_error = errs[i];
        }
        if (!first_error) return pl;
        if (explicit_list || kept.empty()) std::rethrow_exception(first_error);
        devs = kept;
        if (devs.size() <= 1) return single(devs, true);
    }
}

fr::Model train_ca_devices(const std::shared_ptr<fr::DatasetView>& view, const ParsedRequest& rq) {
    const uint32_t R = rq.ca.num_restarts;
    auto t0 = std::chrono::steady_clock::now();
    const DevicePlan pl = devices_for_request(view, R, min_restarts_per_device(), restart_slots_max());
    if (pl.devs.empty() || (pl.devs.size() == 1 && pl.slot[0] == 0)) return train_ca(view, rq, 0, R, nullptr);
    fr::Evaluator ev = fr::make_evaluator(*view, rq.measure, rq.has_qrel ? &rq.qrel : nullptr);
    if (view->host_csr().nq == 0) fr::fail_str("assertion failed: !data.queries().is_empty()");
    const size_t k = pl.devs.size();
    // One queue of restart ids for all devices (the reference's rayon pool, src/coordinate_ascent.rs:215-225): every
    // trainer starts with its share and, once restarts of its own have converged, takes the next ids nobody has started.
    // FR_RESTART_QUEUE=0: the static block partition of round 3 (entry i trains block i of the ids) -- same model.
    const char* qe = std::getenv("FR_RESTART_QUEUE");
    const bool shared_queue = !(qe && qe[0] == '0');
    const uint32_t capacity = std::min<uint32_t>(restart_slots_max(), (uint32_t)((R + k - 1) / k));
    auto queue = std::make_shared<fr::RestartQueue>(0, R);
    std::vector<std::vector<fr::RestartResult>> parts(k);
    std::vector<fr::TrainStats> stats(k);
    std::vector<std::exception_ptr> errors(k);
    auto work = [&](size_t i) {
        try {
            std::string err;
            if (!frdev::set_device(pl.devs[i], &err)) fr::fail_str(err);
            auto q = shared_queue ? queue : std::make_shared<fr::RestartQueue>(pl.begin[i], pl.end[i]);
            parts[i] = train_ca_queue(view, rq, ev, std::move(q), shared_queue ? capacity : restart_slots_max(), pl.slot[i], pl.devs[i], &stats[i]);
        } catch (...) {
            errors[i] = std::current_exception();
        }
    };
    std::vector<std::thread> pool;
    for (size_t i = 1; i < k; i++) pool.emplace_back(work, i);
    work(0);
    for (auto& th : pool) th.join();
    for (size_t i = 0; i < k; i++)
        if (errors[i]) std::rethrow_exception(errors[i]);
    // ---- the job's one exchange.  Every entry of the device list contributes its restarts as a block of records; the
    // blocks meet in host memory (the threads share an address space) AND, when the entries are distinct GPUs, in ONE
    // RCCL all-gather across them (frdev::rccl_allgather: ncclCommInitAll over the list, a grouped ncclAllGather).  The
    // selection below reads what RCCL delivered to rank 0, which must equal the host-side concatenation bit for bit; ranks
    // that share a GPU (FR_DEVICES=0,0: contexts, not devices) cannot form a communicator and keep the host gather, with the
    // reason recorded.  With N distinct GPUs a failed exchange fails the request.
    size_t dim = 0, cap = 1;
    for (size_t i = 0; i < k; i++) {
        cap = std::max(cap, parts[i].size());
        for (const auto& h : parts[i]) dim = std::max(dim, h.weights.size());
    }
    const size_t block_len = cap * fr::restart_record_len(dim);
    std::vector<double> blocks(k * block_len);
    for (size_t i = 0; i < k; i++) fr::pack_restart_records(parts[i], cap, dim, blocks.data() + i * block_len);
    frdev::RcclReport rccl;
    std::vector<double> via_rccl;
    {
        std::string err;
        if (!frdev::rccl_allgather(pl.devs, blocks.data(), block_len, &via_rccl, &rccl, &err)) fr::fail_str(err);
    }
    const std::vector<double>& exchanged = rccl.ran ? via_rccl : blocks;
    std::vector<fr::RestartResult> hist = fr::unpack_restart_records(exchanged.data(), k * cap, dim, R);
    fr::TrainStats total = stats[0];
    total.rccl_set = true;
    total.rccl = rccl;
    for (size_t i = 0; i < k; i++) {
        if (i == 0) continue;
        total.useful_evals += stats[i].useful_evals, total.raw_evals += stats[i].raw_evals;
        total.ticks = std::max(total.ticks, stats[i].ticks), total.groups += stats[i].groups;
        total.restarts += stats[i].restarts, total.refills += stats[i].refills;
        total.verify_pairs += stats[i].verify_pairs, total.verify_redone += stats[i].verify_redone;
        total.line_searches += stats[i].line_searches, total.exact_ticks += stats[i].exact_ticks;
        total.exact_groups += stats[i].exact_groups, total.verify_redo_entries += stats[i].verify_redo_entries;
        total.chain_runs += stats[i].chain_runs, total.chain_visits += stats[i].chain_visits;
        total.rank_slots_on += stats[i].rank_slots_on, total.rank_slots_off += stats[i].rank_slots_off;
        total.audit_values += stats[i].audit_values, total.audit_mismatches += stats[i].audit_mismatches;
    }
    total.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    total.devices = (uint32_t)k;
    total.device = -1;
    set_last_stats(total, stats);
    return fr::ca_select(hist, rq.ca.output_ensemble);
}

// json_api.rs:41-48 -> random_forest::learn_ensemble
fr::Model train_rf(const std::shared_ptr<fr::DatasetView>& view, const ParsedRequest& rq) {
    auto t0 = std::chrono::steady_clock::now();
    fr::Evaluator ev = fr::make_evaluator(*view, rq.measure, rq.has_qrel ? &rq.qrel : nullptr);
    fr::RFTrainer trainer(view, std::move(ev), rq.rf);
    // the trees of a forest are independent given their seeds (random_forest.rs:301-331 grows them with rayon): spread
    // over FR_DEVICES like a coordinate-ascent request's restarts, block i of the trees on entry i of the list
    std::vector<fr::RFTrainer::DevicePart> parts;
    if (rq.rf.num_trees > 0) {
        // (a forest that prints its progress table grows on one device -- one unit of work, so no copies are made -- but an
        // explicit FR_DEVICES / fr_set_device choice of that device is still honoured)
        const DevicePlan pl = devices_for_request(view, rq.rf.quiet ? rq.rf.num_trees : 1);
        // several entries, or ONE entry that names a device other than the one the dataset was built on (slot 1: its copy there)
        if (pl.devs.size() > 1 || (pl.devs.size() == 1 && pl.slot[0] != 0))
            for (size_t i = 0; i < pl.devs.size(); i++)
                parts.push_back(fr::RFTrainer::DevicePart{pl.slot[i], pl.devs[i], rq.rf.quiet ? pl.begin[i] : 0u, rq.rf.quiet ? pl.end[i] : rq.rf.num_trees});
    }
    fr::Model m = trainer.learn(std::move(parts));
    fr::TrainStats st;
    st.devices = trainer.stats().devices;
    st.path = "random_forest";
    st.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    st.restarts = trainer.stats().trees;
    st.ticks = trainer.stats().levels;
    st.groups = trainer.stats().batches;
    st.raw_evals = trainer.stats().candidates;  // split candidates evaluated
    st.useful_evals = trainer.stats().nodes;    // tree nodes produced
    set_last_stats(st);
    return m;
}

// LambdaMART trains on the view's primary device only: its trees depend on each other, and a request that names several
// devices gets the single-device model
// (valid / init: fr_train_model_with's validation dataset and init model, or null)
fr::Model train_lambdamart(const std::shared_ptr<fr::DatasetView>& view, const ParsedRequest& rq, const std::shared_ptr<fr::DatasetView>& valid = nullptr,
                           const fr::Model* init = nullptr) {
    auto t0 = std::chrono::steady_clock::now();
    // under objective = map / mrr the AP / RR evaluator takes over every role of the request's measure (which was checked)
    const char* objective = rq.lm.objective_measure();
    fr::Evaluator ev = fr::make_evaluator(*view, objective ? std::string(objective) : rq.measure, rq.has_qrel ? &rq.qrel : nullptr);
    fr::LambdaMARTTrainer trainer(view, std::move(ev), rq.lm);
    if (valid) trainer.set_valid(valid, fr::make_evaluator(*valid, objective ? std::string(objective) : rq.measure, rq.has_qrel ? &rq.qrel : nullptr));
    trainer.set_init(init);
    fr::Model m = trainer.learn();
    fr::TrainStats st;
    st.devices = 1;
    st.path = "lambdamart";
    st.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    st.restarts = trainer.stats().trees;
    set_last_stats(st);
    std::lock_guard<std::mutex> lk(g_stats_mu);
    g_last_lambdamart = trainer.stats().to_json();
    return m;
}

Value restarts_to_json(const std::vector<fr::RestartResult>& hist) {
    Value arr = Value::array();
    for (const auto& h : hist) {
        Value r = Value::object();
        r.set("restart_id", Value::uint(h.restart_id));
        r.set("score", Value::number(h.score));
        Value w = Value::array();
        for (double x : h.weights) w.push(Value::number(x));
        r.set("weights", std::move(w));
        arr.push(std::move(r));
    }
    return arr;
}

// a JSON list of {"restart_id","score","weights"} (what fr_train_model_shard / fr_ca_state return)
static std::vector<fr::RestartResult> restarts_from_json_text(const std::string& text) {
    Value v = parse_json_or_fail(text);
    if (!v.is_array()) fr::fail_raw("Error(\"invalid type: expected a sequence\", line: 1, column: 1)");
    std::vector<fr::RestartResult> hist;
    for (const auto& r : v.arr) {
        fr::RestartResult h;
        h.restart_id = (uint32_t)fr::json_u64(fr::json_field(r, "restart_id"), "restart_id");
        h.score = fr::json_f64(fr::json_field(r, "score"), "score");
        for (const auto& x : fr::json_field(r, "weights").arr) h.weights.push_back(fr::json_f64(x, "weights"));
        hist.push_back(std::move(h));
    }
    return hist;
}

// the steppable trainer's handle (fr_ca_begin .. fr_ca_free)
struct FrTrainer {
    std::unique_ptr<fr::CATrainer> t;
    std::chrono::steady_clock::time_point t0;
    std::shared_ptr<fr::DataCore> core;  // (its api_mu serialises the calls on this handle with other jobs on the dataset)
    std::vector<unsigned char> capture_blob;  // fr_ca_capture_take: the arrays of the events last described, until they are fetched
};

// fr_ca_begin and fr_ca_begin_query_shard (`who`): the request's checks, then `make` -- under the dataset's lock -- refuses
// or gives the handle its CATrainer and its starting time.  NULL with *error_out set (when there is a place for it) on any refusal.
template <typename F>
void* begin_trainer(const char* who, const void* train_request_json, const CDataset* dataset, const void** error_out, F&& make) {
    if (error_out) *error_out = nullptr;
    FrTrainer* h = nullptr;
    const void* st = status_call([&]() {
        const CDataset& ds = require_dataset(dataset);
        ParsedRequest rq = parse_train_request(accept_str("train_request_json", train_request_json));
        if (rq.learner != Learner::CoordinateAscent) fr::fail_str(std::string(who) + ": only CoordinateAscent");
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        auto holder = std::make_unique<FrTrainer>();
        make(ds, rq, *holder);
        holder->core = ds.view->core;
        h = holder.release();
    });
    if (st) {
        if (error_out) *error_out = st; else free((void*)st);
        return nullptr;
    }
    return h;
}

}  // namespace

extern "C" {

// The exchange records (host.hpp: pack_restart_records) for callers that gather outside the library.
const void* fr_pack_restart_records(const void* restarts_json, size_t cap, size_t dim, double* out) {
    return status_call([&]() {
        if (out == nullptr) fr::fail_str("fr_pack_restart_records: null output buffer");
        fr::pack_restart_records(restarts_from_json_text(accept_str("restarts_json", restarts_json)), cap, dim, out);
    });
}

const void* fr_unpack_restart_records(const double* records, size_t n_records, size_t dim) {
    return json_call([&]() {
        if (records == nullptr && n_records > 0) fr::fail_str("fr_unpack_restart_records: null input buffer");
        return frjson::dump(restarts_to_json(fr::unpack_restart_records(records, n_records, dim)));
    });
}

// One single-process RCCL all-gather of `n` blocks of block_len doubles over `devices` (rccl_exchange.inc): out (optional)
// receives rank 0's gathered buffer, n * block_len doubles.  Returns the report as JSON ({"ran": false, "reason"} when it
// does not apply), or the error envelope when N distinct GPUs were named and the exchange failed.
const void* fr_rccl_allgather(const int* devices, size_t n, const double* blocks, size_t block_len, double* out) {
    return json_call([&]() {
        if ((devices == nullptr || blocks == nullptr) && n > 0) fr::fail_str("fr_rccl_allgather: null argument");
        std::vector<int> devs(devices, devices + n);
        frdev::RcclReport rep;
        std::vector<double> got;
        std::string err;
        if (!frdev::rccl_allgather(devs, blocks, block_len, &got, &rep, &err)) fr::fail_str(err);
        if (rep.ran && out != nullptr) std::memcpy(out, got.data(), got.size() * sizeof(double));
        return frjson::dump(rccl_report_to_json(rep));
    });
}

const void* fr_train_model_shard(const void* train_request_json, const CDataset* dataset, uint32_t restart_begin,
                                 uint32_t restart_end) {
    return json_call([&]() {
        const CDataset& ds = require_dataset(dataset);
        ParsedRequest rq = parse_train_request(accept_str("train_request_json", train_request_json));
        if (rq.learner != Learner::CoordinateAscent) fr::fail_str("fr_train_model_shard: only CoordinateAscent shards by restart");
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        std::vector<fr::RestartResult> hist;
        train_ca(ds.view, rq, restart_begin, restart_end, &hist);
        Value o = Value::object();
        o.set("restarts", restarts_to_json(hist));
        {
            std::lock_guard<std::mutex> slk(g_stats_mu);
            o.set("stats", stats_to_json(g_last_stats));
        }
        return frjson::dump(o);
    });
}

void* fr_ca_begin(const void* train_request_json, const CDataset* dataset, uint32_t restart_begin,
                  uint32_t restart_end, const void** error_out) {
    return begin_trainer("fr_ca_begin", train_request_json, dataset, error_out, [&](const CDataset& ds, const ParsedRequest& rq, FrTrainer& h) {
        fr::Evaluator ev = fr::make_evaluator(*ds.view, rq.measure, rq.has_qrel ? &rq.qrel : nullptr);
        if (ds.view->host_csr().nq == 0) fr::fail_str("assertion failed: !data.queries().is_empty()");
        h.t0 = std::chrono::steady_clock::now();
        h.t = std::make_unique<fr::CATrainer>(ds.view, std::move(ev), rq.ca, restart_begin, restart_end);
    });
}

void* fr_ca_begin_query_shard(const void* train_request_json, const CDataset* dataset, uint64_t total_queries,
                              fr_allreduce_sum_fn allreduce, void* ctx, const void** error_out) {
    return begin_trainer("fr_ca_begin_query_shard", train_request_json, dataset, error_out, [&](const CDataset& ds, const ParsedRequest& rq, FrTrainer& h) {
        if (!allreduce) fr::fail_str("fr_ca_begin_query_shard: allreduce callback is null!");
        fr::Evaluator ev = fr::make_evaluator(*ds.view, rq.measure, rq.has_qrel ? &rq.qrel : nullptr);
        if (total_queries == 0) fr::fail_str("assertion failed: !data.queries().is_empty()");  // (the job's queries, not this shard's)
        fr::QueryShard shard;
        shard.total_queries = total_queries;
        shard.allreduce = [allreduce, ctx](double* v, size_t n) {
            if (allreduce(ctx, v, n) != 0) fr::fail_str("query-shard allreduce callback failed");
        };
        h.t0 = std::chrono::steady_clock::now();
        h.t = std::make_unique<fr::CATrainer>(ds.view, std::move(ev), rq.ca, 0u, rq.ca.num_restarts, std::move(shard));
    });
}

const void* fr_ca_step(void* trainer, uint64_t max_ticks, uint64_t* ticks_done, int* finished) {
    return status_call([&]() {
        if (!trainer) fr::fail_str("trainer pointer is null!");
        FrTrainer* h = (FrTrainer*)trainer;
        std::lock_guard<std::mutex> lk(h->core->api_mu);
        uint64_t n = 0;
        const bool alive = h->t->run(max_ticks, &n);
        if (ticks_done) *ticks_done = n;
        if (finished) *finished = (!alive || h->t->done()) ? 1 : 0;
    });
}

const void* fr_ca_state(void* trainer) {
    return json_call([&]() {
        if (!trainer) fr::fail_str("trainer pointer is null!");
        FrTrainer* h = (FrTrainer*)trainer;
        std::lock_guard<std::mutex> lk(h->core->api_mu);  // fr_ca_step may be mutating the trainer on another thread
        h->t->stats().seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - h->t0).count();
        Value o = Value::object();
        o.set("restarts", restarts_to_json(h->t->results()));
        o.set("stats", stats_to_json(h->t->stats()));
        o.set("finished", Value::boolean(h->t->done()));
        return frjson::dump(o);
    });
}

void fr_ca_free(void* trainer) { delete (FrTrainer*)trainer; }

const CResult* fr_select_model(const void* restarts_json, int output_ensemble) {
    return c_call<CModel>([&]() {
        std::vector<fr::RestartResult> hist = restarts_from_json_text(accept_str("restarts_json", restarts_json));
        // restart order defines "last maximum" (src/coordinate_ascent.rs:244-251)
        std::stable_sort(hist.begin(), hist.end(),
                         [](const fr::RestartResult& a, const fr::RestartResult& b) { return a.restart_id < b.restart_id; });
        return new_model([&] { return fr::ca_select(hist, output_ensemble != 0); });
    });
}

const void* fr_last_train_stats(void) {
    return json_call([&]() {
        std::lock_guard<std::mutex> slk(g_stats_mu);
        Value o = stats_to_json(g_last_stats);
        if (!g_last_per_device.empty()) {  // what every device of the call did (ticks above = the longest device's)
            Value a = Value::array();
            for (const fr::TrainStats& st : g_last_per_device) a.push(stats_to_json(st));
            o.set("per_device", std::move(a));
        }
        if (!g_last_lambdamart.is_null()) o.set("lambdamart", g_last_lambdamart);
        return frjson::dump(o);
    });
}

const CResult* fr_train_model_with(const void* train_request_json, const CDataset* dataset, const CDataset* valid_dataset_or_null,
                                   const CModel* init_model_or_null) {
    if (!valid_dataset_or_null && !init_model_or_null) return train_model((void*)train_request_json, (void*)dataset);
    return c_call<CModel>([&]() {
        const CDataset& ds = require_dataset(dataset);
        ParsedRequest rq = parse_train_request(accept_str("train_request_json", train_request_json), valid_dataset_or_null != nullptr);
        if (rq.learner != Learner::LambdaMART)
            fr::fail_str(std::string("fr_train_model_with: a validation dataset and an init model are LambdaMART's; the request's learner is ") +
                         (rq.learner == Learner::CoordinateAscent ? "CoordinateAscent" : "RandomForest"));
        DatasetLocks lk(ds, valid_dataset_or_null);
        return new_model([&] {
            return train_lambdamart(ds.view, rq, valid_dataset_or_null ? valid_dataset_or_null->view : nullptr,
                                    init_model_or_null ? &init_model_or_null->actual : nullptr);
        });
    });
}

}  // extern "C"
