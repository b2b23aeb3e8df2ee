// extern "C" boundary of libfastrank_amd.so -- see include/fastrank.h for the contract and the
// reference file:line each symbol replaces (src/lib.rs, src/ffi.rs, src/json_api.rs).
#include <atomic>
#include <limits>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>

#include "../../include/fastrank.h"
#include "host.hpp"
#include "loader.hpp"
#include "explain_host.hpp"
#include "normalize_host.hpp"
#include "resample_host.hpp"
#include "permute_host.hpp"
#include "forest_pack.hpp"
#include "lambdamart.hpp"
#include "rf_train.hpp"
#include "verify_end.hpp"

using fr::FrError;
using frjson::Value;

struct CDataset {
    std::shared_ptr<fr::DatasetView> view;
};
struct CModel {
    fr::Model actual;
};
struct CQRel {
    fr::QRel actual;
};

namespace {

// Device jobs are serialised per dataset (DataCore::api_mu: the views of one core share device forms and work buffers),
// not per process: two host threads that train on different datasets -- each on its own devices -- do not wait for
// each other.  (Round 2 had one process-wide lock.)
std::mutex g_stats_mu;  // fr_last_train_stats
std::mutex g_load_mu;   // fr_last_load_stats
fr::LoadStats g_last_load;
static std::mutex& api_mu_of(const CDataset& ds) { return ds.view->core->api_mu; }
fr::TrainStats g_last_stats;

// What fr_normalize_dataset remembers of the datasets it made: the normaliser's JSON (a second one is refused) and what
// making the dataset took.  Kept beside DataCore, not in it: host.hpp is one of device.o's sources, and a dataset that was
// never normalised has nothing here.  Entries of cores that are gone are dropped at the next insert.
struct NormMemo {
    std::string normalization, stats;
};
std::mutex g_norm_mu;
std::vector<std::pair<std::weak_ptr<fr::DataCore>, NormMemo>> g_norm_memo;
NormMemo norm_memo_of(const std::shared_ptr<fr::DataCore>& core) {
    std::lock_guard<std::mutex> lk(g_norm_mu);
    for (const auto& e : g_norm_memo)
        if (e.first.lock() == core) return e.second;
    return NormMemo();
}
void norm_memo_set(const std::shared_ptr<fr::DataCore>& core, NormMemo memo) {
    std::lock_guard<std::mutex> lk(g_norm_mu);
    g_norm_memo.erase(std::remove_if(g_norm_memo.begin(), g_norm_memo.end(), [](const auto& e) { return e.first.expired(); }), g_norm_memo.end());
    g_norm_memo.emplace_back(core, std::move(memo));
}

// src/ffi.rs:40-43 return_string
const void* return_string(const std::string& s) {
    char* p = (char*)malloc(s.size() + 1);
    memcpy(p, s.c_str(), s.size() + 1);
    return p;
}

std::string error_envelope(const std::string& debug_context) {
    Value o = Value::object();
    o.set("error", Value::string("error"));
    o.set("context", Value::string(debug_context));
    return frjson::dump(o);
}

// src/ffi.rs:29-37 accept_str
std::string accept_str(const char* name, const void* input) {
    if (!input) fr::fail_str(std::string("NULL pointer: ") + name);
    return std::string((const char*)input);
}

Value parse_json_or_fail(const std::string& text) {
    try {
        return frjson::parse(text.c_str());
    } catch (const frjson::ParseError& e) {
        fr::fail_raw(e.debug());
    }
}

// src/ffi.rs:45-55 result_to_json
template <typename F>
const void* json_call(F&& body) {
    std::string out;
    try {
        out = body();
    } catch (const FrError& e) {
        out = error_envelope(e.debug);
    } catch (const std::exception& e) {
        out = error_envelope(frjson::rust_debug_str(e.what()));
    }
    return return_string(out);
}

// src/ffi.rs:57-74 result_to_c
template <typename T, typename F>
const CResult* c_call(F&& body) {
    CResult* r = (CResult*)malloc(sizeof(CResult));
    r->error_message = nullptr;
    r->success = nullptr;
    try {
        T* item = body();
        r->success = item;
    } catch (const FrError& e) {
        r->error_message = return_string(error_envelope(e.debug));
    } catch (const std::exception& e) {
        r->error_message = return_string(error_envelope(frjson::rust_debug_str(e.what())));
    }
    return r;
}

// the model `make` returns as a CModel the caller owns (nothing is left behind when it throws)
template <typename F>
CModel* new_model(F&& make) {
    std::unique_ptr<CModel> out(new CModel());
    out->actual = make();
    return out.release();
}

// NULL on success, else envelope string
template <typename F>
const void* status_call(F&& body) {
    try {
        body();
        return nullptr;
    } catch (const FrError& e) {
        return return_string(error_envelope(e.debug));
    } catch (const std::exception& e) {
        return return_string(error_envelope(frjson::rust_debug_str(e.what())));
    }
}

const CDataset& require_dataset(const void* p) {
    if (!p) fr::fail_str("Dataset pointer is null!");
    return *(const CDataset*)p;
}
const CModel& require_model(const void* p) {
    if (!p) fr::fail_str("Model pointer is null!");
    return *(const CModel*)p;
}

Value unknown_cmd(const char* kind, const std::string& cmd) {
    Value o = Value::object();
    o.set("error", Value::string(kind));
    o.set("context", Value::string(cmd));
    return o;
}

// instances_by_query of a view: qid -> instance ids in view order (ascending for unsampled data)
std::vector<std::pair<std::string, std::vector<uint32_t>>> instances_by_query(const fr::DatasetView& v) {
    std::vector<std::pair<std::string, std::vector<uint32_t>>> out;
    std::unordered_map<uint32_t, size_t> slot;
    for (uint32_t id : v.instances) {
        uint32_t qi = v.core->qix[id];
        auto it = slot.find(qi);
        if (it == slot.end()) {
            it = slot.emplace(qi, out.size()).first;
            out.emplace_back(v.core->qnames[qi], std::vector<uint32_t>());
        }
        out[it->second].second.push_back(id);
    }
    return out;
}

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

Value random_forest_defaults_json() {
    // src/random_forest.rs:141-157 (+ :14-20 tuple-variant wire form {"SquaredError":[]})
    fr::Rand64 rand(0xdeadbeefULL);
    Value p = Value::object();
    p.set("seed", Value::uint(rand.rand_u64()));
    p.set("quiet", Value::boolean(false));
    p.set("num_trees", Value::uint(100));
    p.set("weight_trees", Value::boolean(false));
    Value sm = Value::object();
    sm.set("SquaredError", Value::array());
    p.set("split_method", std::move(sm));
    p.set("instance_sampling_rate", Value::number(0.5));
    p.set("feature_sampling_rate", Value::number(0.25));
    p.set("min_leaf_support", Value::uint(10));
    p.set("split_candidates", Value::uint(3));
    p.set("max_depth", Value::uint(8));
    return p;
}

// Rust's Display for f64: shortest round-trip digits, never exponent form
std::string rust_display_f64(double v) {
    if (v != v) return "NaN";
    if (std::isinf(v)) return v > 0 ? "inf" : "-inf";
    char buf[64];
    auto r = std::to_chars(buf, buf + sizeof(buf), v, std::chars_format::scientific);
    std::string sci(buf, r.ptr);
    bool neg = sci[0] == '-';
    if (neg) sci.erase(0, 1);
    size_t epos = sci.find('e');
    std::string digits;
    for (char c : sci.substr(0, epos))
        if (c != '.') digits += c;
    int exp10 = atoi(sci.c_str() + epos + 1);
    while (digits.size() > 1 && digits.back() == '0') digits.pop_back();
    std::string out = neg ? "-" : "";
    int kk = exp10 + 1;
    if (digits == "0") return out + "0";
    if (kk <= 0) {
        out += "0.";
        out.append((size_t)(-kk), '0');
        out += digits;
    } else if ((int)digits.size() <= kk) {
        out += digits;
        out.append((size_t)(kk - (int)digits.size()), '0');
    } else {
        out.append(digits, 0, (size_t)kk);
        out += '.';
        out.append(digits, (size_t)kk, std::string::npos);
    }
    return out;
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
// every trainer takes its share from the one queue at the start (5 restarts over 4 devices are 2 + 2 + 1, the
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

}  // namespace

extern "C" {

void free_str(void* p) { free(p); }
void free_c_result(CResult* p) { free(p); }
void free_dataset(CDataset* p) { delete p; }
void free_model(CModel* p) { delete p; }
void free_cqrel(CQRel* p) { delete p; }

const CResult* load_cqrel(const void* data_path) {
    return c_call<CQRel>([&]() {
        std::string path = accept_str("data_path", data_path);
        auto* q = new CQRel();
        try {
            q->actual = fr::load_qrel_file(path);
        } catch (...) {
            delete q;
            throw;
        }
        return q;
    });
}

const CResult* cqrel_from_json(const void* json_str) {
    return c_call<CQRel>([&]() {
        Value v = parse_json_or_fail(accept_str("json_str", json_str));
        auto* q = new CQRel();
        try {
            q->actual = fr::qrel_from_json(v);
        } catch (...) {
            delete q;
            throw;
        }
        return q;
    });
}

const void* cqrel_query_json(const CQRel* cqrel, const void* query_str) {
    return json_call([&]() {
        if (!cqrel) fr::fail_str("cqrel pointer is null!");
        std::string cmd = accept_str("query_str", query_str);
        if (cmd == "to_json") return frjson::dump(fr::qrel_to_json(cqrel->actual));
        if (cmd == "queries") {
            Value a = Value::array();
            for (const auto& q : cqrel->actual.queries) a.push(Value::string(q.first));
            return frjson::dump(a);
        }
        const auto* docs = cqrel->actual.get(cmd);
        if (!docs) fr::fail_str("Unknown request: " + cmd);
        return frjson::dump(fr::qrel_query_to_json(*docs));
    });
}

const CResult* fr_load_ranksvm(const void* data_path, const void* feature_names_path, const void* parser) {
    return c_call<CDataset>([&]() {
        std::string path = accept_str("data_path", data_path);
        const std::string word = accept_str("parser", parser);
        std::map<uint32_t, std::string> names;
        bool has_names = false;
        if (feature_names_path) {
            names = fr::load_feature_names(accept_str("feature_names_path", feature_names_path));
            has_names = true;
        }
        auto* d = new CDataset();
        fr::LoadStats st;
        try {
            d->view = fr::load_ranksvm_with(path, has_names ? &names : nullptr, word, &st);
        } catch (...) {
            delete d;
            throw;
        }
        std::lock_guard<std::mutex> lk(g_load_mu);
        g_last_load = st;
        return d;
    });
}

const CResult* load_ranksvm_format(void* data_path, void* feature_names_path) { return fr_load_ranksvm(data_path, feature_names_path, "auto"); }

// what the last successful fr_load_ranksvm / load_ranksvm_format of this process did (include/fastrank.h)
const void* fr_last_load_stats(void) {
    return json_call([&]() {
        std::lock_guard<std::mutex> lk(g_load_mu);
        const fr::LoadStats& s = g_last_load;
        Value o = Value::object();
        o.set("parser", Value::string(s.parser));
        o.set("reason", Value::string(s.reason));
        o.set("bytes", Value::uint(s.bytes));
        o.set("lines", Value::uint(s.lines));
        o.set("host_lines", Value::uint(s.host_lines));
        Value r = Value::object();
        for (uint32_t k = 1; k < frtext::R_COUNT; k++) r.set(frtext::reason_name(k), Value::uint(s.reasons[k]));
        o.set("host_line_reasons", std::move(r));
        Value t = Value::object();
        t.set("read", Value::number(s.read)), t.set("upload", Value::number(s.dev.upload)), t.set("line_scan", Value::number(s.dev.line_scan));
        t.set("pass1", Value::number(s.dev.pass1)), t.set("pass2", Value::number(s.dev.pass2)), t.set("download", Value::number(s.dev.download));
        t.set("host_merge", Value::number(s.merge)), t.set("total", Value::number(s.total));
        o.set("seconds", std::move(t));
        o.set("scan_slice", Value::uint(frdev::TEXT_SCAN_SLICE));
        o.set("stage_limit", Value::uint(frdev::TEXT_STAGE_LIMIT));
        o.set("auto_threshold", Value::uint(fr::TEXT_DEVICE_THRESHOLD));
        return frjson::dump(o);
    });
}

// The DataCore of a file-loaded dataset, for the tests (include/fastrank.h).  field == NULL: JSON of the scalars and the
// string lists; else the named array's bytes into out[out_bytes] (the protocol of fr_debug_device_form).
const void* fr_debug_dataset_core(const CDataset* dataset, const void* field, void* out, size_t out_bytes) {
    return json_call([&]() {
        const fr::DataCore& c = *require_dataset(dataset).view->core;
        Value o = Value::object();
        if (!field) {
            o.set("n", Value::uint(c.n)), o.set("d", Value::uint(c.d)), o.set("present_words", Value::uint(c.present_words));
            o.set("has_docids", Value::boolean(c.has_docids)), o.set("present_bits_len", Value::uint(c.present_bits.size()));
            o.set("features_len", Value::uint(c.features.size())), o.set("doc_present_len", Value::uint(c.doc_present.size()));
            Value q = Value::array(), dn = Value::array();
            // (names are bytes of the file, not always UTF-8: served in hex)
            auto hex = [](const std::string& s) {
                static const char* dig = "0123456789abcdef";
                std::string h;
                for (unsigned char ch : s) h += dig[ch >> 4], h += dig[ch & 15];
                return h;
            };
            for (const auto& s : c.qnames) q.push(Value::string(hex(s)));
            for (const auto& s : c.docids) dn.push(Value::string(hex(s)));
            o.set("qnames_hex", std::move(q)), o.set("docids_hex", std::move(dn));
            return frjson::dump(o);
        }
        const std::string name = accept_str("field", field);
        const void* p = nullptr;
        size_t bytes = 0;
        if (name == "x") p = c.x, bytes = c.n * c.d * sizeof(float);
        else if (name == "gain") p = c.gain.data(), bytes = c.gain.size() * sizeof(float);
        else if (name == "qix") p = c.qix.data(), bytes = c.qix.size() * sizeof(uint32_t);
        else if (name == "doc_present") p = c.doc_present.data(), bytes = c.doc_present.size();
        else if (name == "features") p = c.features.data(), bytes = c.features.size() * sizeof(uint32_t);
        else if (name == "present_bits") p = c.present_bits.data(), bytes = c.present_bits.size() * sizeof(uint32_t);
        else fr::fail_str("fr_debug_dataset_core: no field named " + name);
        if (out_bytes != bytes || (!out && bytes)) fr::fail_str("fr_debug_dataset_core: field " + name + " holds " + std::to_string(bytes) + " bytes, the buffer " + std::to_string(out_bytes));
        if (bytes) std::memcpy(out, p, bytes);
        o.set("bytes", Value::uint(bytes));
        return frjson::dump(o);
    });
}

// The host compile of the device parser's number rule (csrc/text_number.hpp) on n tokens, one per line of `tokens`:
// reasons[i] (frtext::Reason; the reply lists their names by code) and, where it is 0, the f64 / f32 the rule gives.
// The CPU tests hold it to their Python restatement.
const void* fr_debug_text_number(const void* tokens, size_t n, uint32_t* reasons, double* value64, float* value32) {
    return json_call([&]() {
        const std::string text = accept_str("tokens", tokens);
        if (n && (!reasons || !value64 || !value32)) fr::fail_str("NULL pointer: fr_debug_text_number arrays");
        size_t at = 0, i = 0;
        for (; i < n && at <= text.size(); i++) {
            size_t end = text.find('\n', at);
            if (end == std::string::npos) end = text.size();
            double v = 0.0;
            reasons[i] = frtext::fast_number((const unsigned char*)text.data() + at, (uint32_t)(end - at), &v);
            value64[i] = reasons[i] == frtext::R_NONE ? v : 0.0;
            value32[i] = reasons[i] == frtext::R_NONE ? (float)v : 0.0f;
            at = end + 1;
        }
        if (i != n) fr::fail_str("fr_debug_text_number: fewer tokens than n");
        Value names = Value::array();
        for (uint32_t k = 0; k < frtext::R_COUNT; k++) names.push(Value::string(frtext::reason_name(k)));
        Value o = Value::object();
        o.set("reasons", std::move(names));
        return frjson::dump(o);
    });
}

const CResult* dataset_query_sampling(CDataset* dataset, const void* queries_json_list) {
    return c_call<CDataset>([&]() {
        const CDataset& ds = require_dataset(dataset);
        Value v = parse_json_or_fail(accept_str("queries_json_list", queries_json_list));
        if (!v.is_array()) fr::fail_raw("Error(\"invalid type: expected a sequence\", line: 1, column: 1)");
        std::set<std::string> wanted;
        for (const auto& x : v.arr) {
            if (!x.is_string()) fr::fail_raw("Error(\"invalid type: expected a string\", line: 1, column: 1)");
            wanted.insert(x.s);
        }
        // src/sampling.rs:117-133 with_queries
        auto child = std::make_shared<fr::DatasetView>();
        child->core = ds.view->core;
        child->features = ds.view->features;
        child->sampled = true;
        child->parent = ds.view;
        for (auto& qi : instances_by_query(*ds.view))
            if (wanted.count(qi.first)) child->instances.insert(child->instances.end(), qi.second.begin(), qi.second.end());
        auto* out = new CDataset();
        out->view = child;
        return out;
    });
}

const CResult* dataset_feature_sampling(CDataset* dataset, const void* feature_json_list) {
    return c_call<CDataset>([&]() {
        const CDataset& ds = require_dataset(dataset);
        Value v = parse_json_or_fail(accept_str("feature_json_list", feature_json_list));
        if (!v.is_array()) fr::fail_raw("Error(\"invalid type: expected a sequence\", line: 1, column: 1)");
        // src/sampling.rs:91-115 with_features
        std::set<uint32_t> valid(ds.view->features.begin(), ds.view->features.end());
        std::set<uint32_t> keep, missing;
        for (const auto& x : v.arr) {
            uint32_t fid = (uint32_t)fr::json_u64(x, "FeatureId");
            (valid.count(fid) ? keep : missing).insert(fid);
        }
        if (!missing.empty()) {
            std::string s = "Missing Features: {";
            bool first = true;
            for (uint32_t f : missing) {
                if (!first) s += ", ";
                s += "FeatureId(" + std::to_string(f) + ")";
                first = false;
            }
            fr::fail_str(s + "}");
        }
        if (keep.empty()) fr::fail_str("No Features!");
        auto child = std::make_shared<fr::DatasetView>();
        child->core = ds.view->core;
        child->features.assign(keep.begin(), keep.end());
        child->instances = ds.view->instances;
        child->sampled = true;
        child->parent = ds.view;
        child->same_instances_as_parent = true;
        auto* out = new CDataset();
        out->view = child;
        return out;
    });
}

const void* dataset_query_json(void* dataset, void* json_cmd_str) {
    return json_call([&]() {
        const CDataset& ds = require_dataset(dataset);
        const fr::DatasetView& v = *ds.view;
        std::string cmd = accept_str("dataset_query_json", json_cmd_str);
        // src/ffi.rs:144-183
        if (cmd == "is_sampled") return std::string(v.sampled ? "true" : "false");
        if (cmd == "num_features") return std::to_string(v.n_dim());
        if (cmd == "feature_ids") {
            Value a = Value::array();
            for (uint32_t f : v.features) a.push(Value::uint(f));
            return frjson::dump(a);
        }
        if (cmd == "num_instances") return std::to_string(v.instances.size());
        if (cmd == "queries") {
            Value a = Value::array();
            for (auto& qi : instances_by_query(v)) a.push(Value::string(qi.first));
            return frjson::dump(a);
        }
        if (cmd == "instances_by_query") {
            Value o = Value::object();
            for (auto& qi : instances_by_query(v)) {
                Value a = Value::array();
                for (uint32_t id : qi.second) a.push(Value::uint(id));
                o.obj.emplace_back(qi.first, std::move(a));
            }
            return frjson::dump(o);
        }
        if (cmd == "feature_names") {
            Value a = Value::array();
            for (uint32_t f : v.features) a.push(Value::string(v.core->feature_name(f)));
            return frjson::dump(a);
        }
        // the normaliser a dataset made by fr_normalize_dataset remembers (null for any other), and what making it took
        if (cmd == "normalization" || cmd == "normalization_stats") {
            const NormMemo memo = norm_memo_of(v.core);
            const std::string& text = cmd == "normalization" ? memo.normalization : memo.stats;
            return text.empty() ? std::string("null") : text;
        }
        return frjson::dump(unknown_cmd("unknown_dataset_query_str", cmd));
    });
}

const void* query_json(const void* json_cmd_str) {
    return json_call([&]() {
        std::string cmd = accept_str("query_json_str", json_cmd_str);
        // src/ffi.rs:215-236
        if (cmd == "coordinate_ascent_defaults" || cmd == "random_forest_defaults" || cmd == "lambdamart_defaults") {
            Value o = Value::object();
            o.set("measure", Value::string("ndcg"));
            Value params = Value::object();
            if (cmd == "coordinate_ascent_defaults")
                params.set("CoordinateAscent", fr::CAParams::defaults().to_json());
            else if (cmd == "lambdamart_defaults")
                params.set("LambdaMART", fr::LambdaMARTParams().to_json());
            else
                params.set("RandomForest", random_forest_defaults_json());
            o.set("params", std::move(params));
            o.set("judgments", Value::null());
            return frjson::dump(o);
        }
        if (cmd == "measures") {  // the evaluators every call takes by name (measures_host.hpp)
            Value a = Value::array();
            const frmeasure::MeasureInfo* t = frmeasure::measure_table();
            for (int i = 0; i < frmeasure::MEASURE_COUNT; i++) {
                Value o = Value::object();
                o.set("name", Value::string(t[i].names[0]));
                Value al = Value::array();
                if (t[i].names[1] != nullptr) al.push(Value::string(t[i].names[1]));
                o.set("aliases", std::move(al));
                o.set("display", Value::string(t[i].display));
                o.set("cutoff", Value::string(frmeasure::cutoff_name(t[i].cutoff)));
                a.push(std::move(o));
            }
            return frjson::dump(a);
        }
        return frjson::dump(unknown_cmd("unknown_query_str", cmd));
    });
}

const CResult* make_dense_dataset_f32_f64_i64(size_t n, size_t d, const float* x, const double* y,
                                              const int64_t* qids) {
    return c_call<CDataset>([&]() {
        if ((n && (!x || !y || !qids))) fr::fail_str("NULL pointer: dense dataset arrays");
        auto* out = new CDataset();
        try {
            out->view = fr::make_dense(n, d, x, y, qids);
        } catch (...) {
            delete out;
            throw;
        }
        return out;
    });
}

const CResult* train_model(void* train_request_json, void* dataset) {
    return c_call<CModel>([&]() {
        // src/lib.rs:249-252: the dataset pointer is checked after the request is parsed lazily;
        // result_train_model reports the null dataset first (src/ffi.rs:189-193)
        const CDataset& ds = require_dataset(dataset);
        ParsedRequest rq = parse_train_request(accept_str("train_request_json", train_request_json));
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        auto* out = new CModel();
        try {
            switch (rq.learner) {
                case Learner::CoordinateAscent: out->actual = train_ca_devices(ds.view, rq); break;
                case Learner::RandomForest: out->actual = train_rf(ds.view, rq); break;
                case Learner::LambdaMART: out->actual = train_lambdamart(ds.view, rq); break;
            }
        } catch (...) {
            delete out;
            throw;
        }
        return out;
    });
}

const CResult* model_from_json(const void* json_str) {
    return c_call<CModel>([&]() {
        Value v = parse_json_or_fail(accept_str("json_str", json_str));
        return new_model([&] { return fr::model_from_json(v); });
    });
}

const void* model_query_json(const void* model, const void* json_cmd_str) {
    return json_call([&]() {
        const CModel& m = require_model(model);
        std::string cmd = accept_str("query_json", json_cmd_str);
        if (cmd == "to_json") return frjson::dump(fr::model_to_json(m.actual));
        return frjson::dump(unknown_cmd("unknown_dataset_query_str", cmd));  // sic: src/ffi.rs:206-209
    });
}

const void* evaluate_by_query(const CModel* model, const CDataset* dataset, const CQRel* qrel,
                              const void* evaluator) {
    return json_call([&]() {
        const CModel& m = require_model(model);
        const CDataset& ds = require_dataset(dataset);
        std::string name = accept_str("evaluator_name", evaluator);
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        fr::Evaluator ev = fr::make_evaluator(view, name, qrel ? &qrel->actual : nullptr);
        Value o = Value::object();
        if (view.instances.empty()) return frjson::dump(o);
        frdev::DeviceDataset& dev = view.device();
        fr::score_model(view, m.actual);
        std::string err;
        if (!dev.metric_from_scores(ev.measure, ev.depth, ev.norms.data(), 1, false, &err)) fr::fail_str(err);
        fr::check_flags(dev);
        std::vector<double> vals(dev.nq());
        if (!dev.download_per_query(1, vals.data(), &err)) fr::fail_str(err);
        for (size_t q = 0; q < vals.size(); q++)
            o.obj.emplace_back(view.core->qnames[view.csr_query[q]], Value::number(vals[q]));
        return frjson::dump(o);
    });
}

const void* predict_scores(const CModel* model, const CDataset* dataset) {
    return json_call([&]() {
        const CModel& m = require_model(model);
        const CDataset& ds = require_dataset(dataset);
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        if (view.instances.empty()) return std::string("{}");
        frdev::DeviceDataset& dev = view.device();
        fr::score_model(view, m.actual);
        std::vector<double> scores(view.core->n, 0.0);
        std::string err;
        if (!dev.download_scores(0, scores.data(), scores.size(), &err)) fr::fail_str(err);
        for (uint32_t id : view.instances)
            if (scores[id] != scores[id]) fr::fail_str("Model.predict -> NaN");
        // src/json_api.rs:53-72: {"<instance index>": score}
        std::string out = "{";
        bool first = true;
        std::vector<uint32_t> ids = view.instances;
        std::sort(ids.begin(), ids.end());
        for (uint32_t id : ids) {
            if (!first) out += ',';
            first = false;
            out += '"';
            out += std::to_string(id);
            out += "\":";
            frjson::write_double(out, scores[id]);
        }
        out += '}';
        return out;
    });
}

const void* predict_to_trecrun(const CModel* model, const CDataset* dataset, const void* output_path,
                               const void* system_name, size_t depth) {
    return json_call([&]() {
        const CModel& m = require_model(model);
        const CDataset& ds = require_dataset(dataset);
        std::string path = accept_str("output_path", output_path);
        std::string sysname = accept_str("system_name", system_name);
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        // src/json_api.rs:75-120
        std::ofstream out(path);
        if (!out) fr::fail_str("could not open " + path + " for writing");
        size_t written = 0;
        if (view.instances.empty()) return std::to_string(written);
        frdev::DeviceDataset& dev = view.device();
        fr::score_model(view, m.actual);
        std::string err;
        std::vector<double> norms(dev.nq(), 0.0);
        if (!dev.metric_from_scores(frdev::M_RR, -1, norms.data(), 1, true, &err)) fr::fail_str(err);
        fr::check_flags(dev);
        std::vector<uint32_t> rank(dev.n());
        if (!dev.download_rank(rank.data(), &err)) fr::fail_str(err);
        std::vector<double> scores(view.core->n, 0.0);
        if (!dev.download_scores(0, scores.data(), scores.size(), &err)) fr::fail_str(err);
        const frdev::HostCSR& csr = view.host_csr();
        const fr::DataCore& c = *view.core;
        for (size_t q = 0; q < csr.nq; q++) {
            const std::string& qid = c.qnames[view.csr_query[q]];
            for (uint32_t p = csr.qoff[q]; p < csr.qoff[q + 1]; p++) {
                size_t rk = p - csr.qoff[q] + 1;
                if (depth > 0 && rk > depth) break;
                uint32_t id = rank[p];
                if (!c.has_docids || id >= c.doc_present.size() || !c.doc_present[id])
                    fr::fail_str("Dataset does not contain document ids and therefore cannot save to trecrun!");
                out << qid << " Q0 " << c.docids[id] << " " << rk << " " << rust_display_f64(scores[id]) << " "
                    << sysname << "\n";
                written++;
            }
            out.flush();
        }
        return std::to_string(written);
    });
}

// ------------------------------------------------------------------------------------------
// extensions
// ------------------------------------------------------------------------------------------

int fr_device_count(void) { return frdev::device_count(nullptr); }

// keys per lane << 16 | lanes per candidate of the full-ranking kernel's size class for a query of `len` documents
uint32_t fr_debug_fullrank_class(uint32_t len) {
    uint32_t nl = 0, pl = 0;
    frdev::fullrank_class_of(len, &nl, &pl);
    return (nl << 16) | pl;
}

// The restart queue without a device: n_workers "trainers" of `capacity` places each, restart r converges after
// lengths[r % n_lengths] ticks, places are refilled at the end of a tick (include/fastrank.h).
const void* fr_debug_restart_queue(uint32_t num_restarts, uint32_t n_workers, uint32_t capacity, const uint32_t* lengths,
                                   uint32_t n_lengths) {
    return json_call([&]() {
        if (n_workers == 0 || capacity == 0 || !lengths || n_lengths == 0) fr::fail_str("fr_debug_restart_queue: bad arguments");
        fr::RestartQueue queue(0, num_restarts);
        struct Place { uint32_t id, left; };
        std::vector<std::vector<Place>> live(n_workers);
        std::vector<std::vector<uint32_t>> order(n_workers);
        std::vector<uint64_t> ticks(n_workers, 0);
        auto fill = [&](uint32_t w) {
            uint32_t id = 0;
            while (live[w].size() < capacity && queue.pop(&id)) {
                live[w].push_back(Place{id, std::max<uint32_t>(lengths[id % n_lengths], 1)});
                order[w].push_back(id);
            }
        };
        for (uint32_t w = 0; w < n_workers; w++) fill(w);
        for (bool any = true; any;) {
            any = false;
            for (uint32_t w = 0; w < n_workers; w++) {
                if (live[w].empty()) continue;
                any = true;
                ticks[w]++;
                for (auto& p : live[w]) p.left--;
                live[w].erase(std::remove_if(live[w].begin(), live[w].end(), [](const Place& p) { return p.left == 0; }), live[w].end());
                fill(w);
            }
        }
        Value o = Value::object(), ord = Value::array(), tk = Value::array();
        for (uint32_t w = 0; w < n_workers; w++) {
            Value a = Value::array();
            for (uint32_t id : order[w]) a.push(Value::uint(id));
            ord.push(std::move(a));
            tk.push(Value::uint(ticks[w]));
        }
        o.set("order", std::move(ord));
        o.set("ticks", std::move(tk));
        return frjson::dump(o);
    });
}

size_t fr_dataset_release_replicas(const CDataset* dataset) {
    if (!dataset || !dataset->view) return 0;
    std::lock_guard<std::mutex> lk(api_mu_of(*dataset));
    size_t n = 0;
    for (fr::DatasetView* v = dataset->view.get(); v; v = v->parent.get()) n += v->release_replicas();
    return n;
}

// The device plan of a request of `num_restarts` units over the devices of `devices_csv` (the FR_DEVICES syntax) on a
// node with `device_count` devices whose first device form lives on `primary_device`: {"devices","slots","blocks"}.
// No device is touched (the CPU tests check the partition and the list parsing with it).
const void* fr_debug_device_plan(const void* devices_csv, int device_count, uint32_t num_restarts, int primary_device) {
    return json_call([&]() {
        const std::string csv = accept_str("devices_csv", devices_csv);
        const DevicePlan pl = plan_devices(parse_device_list(csv.c_str(), device_count), num_restarts, primary_device);
        Value o = Value::object(), d = Value::array(), sl = Value::array(), bl = Value::array();
        for (size_t i = 0; i < pl.devs.size(); i++) {
            d.push(Value::uint((uint64_t)pl.devs[i]));
            sl.push(Value::uint((uint64_t)pl.slot[i]));
            Value b = Value::array();
            b.push(Value::uint(pl.begin[i]));
            b.push(Value::uint(pl.end[i]));
            bl.push(std::move(b));
        }
        o.set("devices", std::move(d));
        o.set("slots", std::move(sl));
        o.set("blocks", std::move(bl));
        return frjson::dump(o);
    });
}

// One timed device-to-device copy of `bytes` bytes src -> dst, made like the dataset copies of train_model's fan-out:
// {"src","dst","bytes","can_access","enabled","ms","gbps"}.
const void* fr_debug_peer_copy(int src_device, int dst_device, size_t bytes) {
    return json_call([&]() {
        int can = 0, en = 0;
        double ms = 0.0;
        std::string err;
        if (!frdev::peer_copy_probe(src_device, dst_device, bytes, &can, &en, &ms, &err)) fr::fail_str(err);
        Value o = Value::object();
        o.set("src", Value::uint((uint64_t)src_device));
        o.set("dst", Value::uint((uint64_t)dst_device));
        o.set("bytes", Value::uint((uint64_t)bytes));
        o.set("can_access", Value::boolean(can != 0));
        o.set("enabled", Value::boolean(en != 0));
        o.set("ms", Value::number(ms));
        o.set("gbps", Value::number(ms > 0.0 ? (double)bytes / (ms * 1e-3) / 1e9 : 0.0));
        return frjson::dump(o);
    });
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

// The walk tiles the device form of a dataset would get for these runs and queries (frdev::build_walk_tiles; no device).
const void* fr_debug_walk_tiles(const uint32_t* run_pos, const uint32_t* run_q0, const uint32_t* run_q1, size_t nruns, const uint32_t* qstart,
                                const uint32_t* qlen, size_t nq, size_t np) {
    return json_call([&]() {
        if (nruns > 0 && (!run_pos || !run_q0 || !run_q1)) fr::fail_str("fr_debug_walk_tiles: null run table");
        if (nq > 0 && (!qstart || !qlen)) fr::fail_str("fr_debug_walk_tiles: null query table");
        for (size_t q = 0; q < nq; q++)
            if ((size_t)qstart[q] + qlen[q] > np) fr::fail_str("fr_debug_walk_tiles: a query lies beyond np");
        for (size_t r = 0; r < nruns; r++)
            if (run_q0[r] > run_q1[r] || run_q1[r] > nq) fr::fail_str("fr_debug_walk_tiles: a run names queries that do not exist");
        const frdev::WalkTileLayout wl = frdev::build_walk_tiles(std::vector<uint32_t>(run_pos, run_pos + nruns), std::vector<uint32_t>(run_q0, run_q0 + nruns),
                                                                std::vector<uint32_t>(run_q1, run_q1 + nruns), std::vector<uint32_t>(qstart, qstart + nq),
                                                                std::vector<uint32_t>(qlen, qlen + nq), np);
        Value o = Value::object();
        auto list = [](const auto& v) {
            Value a = Value::array();
            for (auto x : v) a.push(Value::uint((uint64_t)x));
            return a;
        };
        o.set("walk_tile", Value::uint(frdev::WALK_TILE));
        o.set("wt_start", list(wl.wt_start));
        o.set("run_wt0", list(wl.run_wt0));
        o.set("seg", list(wl.seg));
        o.set("wofs", list(wl.wofs));
        return frjson::dump(o);
    });
}

// Read-back of the device form of a dataset (include/fastrank.h; DeviceDataset::debug_form_*): read only, no product path
// calls it.  slot 0 = the view's first device form (built if needed), slot k > 0 = the copy train_model keeps in context k
// of its device list (an error when there is none: the hook makes no copies).
const void* fr_debug_device_form(const CDataset* dataset, int slot, const void* table, void* out, size_t out_bytes) {
    return json_call([&]() {
        const CDataset& ds = require_dataset(dataset);
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        std::shared_ptr<frdev::DeviceDataset> devp;
        if (slot <= 0) {
            devp = ds.view->device_ptr();
        } else {
            std::lock_guard<std::mutex> vlk(ds.view->mu);
            if ((size_t)slot <= ds.view->replicas.size()) devp = ds.view->replicas[(size_t)slot - 1];
            if (!devp) fr::fail_str("fr_debug_device_form: the dataset has no device copy in slot " + std::to_string(slot));
        }
        Value o = Value::object();
        if (!table) {
            for (const auto& kv : devp->debug_form_scalars()) o.set(kv.first.c_str(), Value::uint(kv.second));
            return frjson::dump(o);
        }
        const std::string name = accept_str("table", table);
        std::vector<unsigned char> bytes;
        bool present = false;
        std::string err;
        if (!devp->debug_form_table(name, &bytes, &present, &err)) fr::fail_str(err);
        o.set("present", Value::boolean(present));
        o.set("bytes", Value::uint(bytes.size()));
        if (present) {
            if (!out || out_bytes != bytes.size())
                fr::fail_str("fr_debug_device_form: table " + name + " holds " + std::to_string(bytes.size()) + " bytes, the buffer " + std::to_string(out_bytes));
            std::memcpy(out, bytes.data(), bytes.size());
        }
        return frjson::dump(o);
    });
}

// The host-side layout of a dataset (csrc/dataset_layout.hpp) built from its host CSR alone: no device is touched.  Same
// name / out-buffer protocol as fr_debug_device_form and the same table names, plus termtab, qnpos, qnneg, qlist, fv_qlist and
// the size classes.  parent_queries: also the tables of the view that holds these queries of the dataset, under "view_" + name;
// `view` (optional): the dataset whose CSR is the view's own (NULL: cut from `dataset`'s).  row_hash[np] (optional): the
// row hashes by position (NULL: a host hash of the row bytes).
const void* fr_debug_dataset_layout(const CDataset* dataset, const uint32_t* parent_queries, size_t n_parent_queries, const CDataset* view,
                                    const uint64_t* row_hash, size_t n_row_hash, const void* table, void* out, size_t out_bytes) {
    return json_call([&]() {
        using namespace frdev;
        const CDataset& ds = require_dataset(dataset);
        const HostCSR& csr = ds.view->host_csr();
        if (csr.n == 0 || csr.nq == 0) fr::fail_str("fr_debug_dataset_layout: empty dataset");
        std::map<std::string, std::vector<unsigned char>> tables;
        Value scalars = Value::object();
        auto put = [&](const std::string& name, const auto& v) {
            using T = typename std::remove_reference_t<decltype(v)>::value_type;
            std::vector<unsigned char>& b = tables[name];
            b.resize(v.size() * sizeof(T));
            if (!v.empty()) std::memcpy(b.data(), v.data(), b.size());
        };
        auto num = [&](const std::string& name, uint64_t v) { scalars.set(name.c_str(), Value::uint(v)); };
        auto put_runs = [&](const std::string& pre, const RunPlan& r) {
            put(pre + "qstart", r.qstart), put(pre + "qlen", r.qlen), put(pre + "qtight", r.qtight);
            put(pre + "run_q0", r.run_q0), put(pre + "run_q1", r.run_q1), put(pre + "run_pos", r.run_pos);
            put(pre + "run_docs", r.run_docs), put(pre + "run_order", r.run_order);
            std::vector<uint32_t> qlist, fv_qlist;
            const std::vector<SizeClass> sc = bucket_queries(r.qlen, pow2_from_64, &qlist), fv = fv_build_classes(r.qlen, &fv_qlist);
            static_assert(sizeof(SizeClass) == 3 * sizeof(uint32_t), "served as triples of u32");
            put(pre + "qlist", qlist), put(pre + "fv_qlist", fv_qlist), put(pre + "size_classes", sc), put(pre + "fv_classes", fv);
            num(pre + "nq", r.qlen.size()), num(pre + "nruns", r.run_q0.size()), num(pre + "maxlen", r.maxlen), num(pre + "np", r.np);
            num(pre + "n_size_classes", sc.size()), num(pre + "n_fv_classes", fv.size());
        };
        std::string err;
        RunPlan runs;
        if (!plan_runs(csr.qoff, csr.nq, run_docs_target(), &runs, &err)) fr::fail_str(err);
        const std::vector<uint32_t> perm_host = position_map(csr, runs.qstart, runs.qlen, runs.np);
        const GainTables gt = gain_tables(csr, runs.qstart, runs.qlen, perm_host, runs.maxlen);
        if (row_hash && n_row_hash != runs.np) fr::fail_str("fr_debug_dataset_layout: row_hash must hold one hash per position (" + std::to_string(runs.np) + ")");
        const std::vector<uint64_t> hashes = row_hash ? std::vector<uint64_t>(row_hash, row_hash + n_row_hash) : host_row_hash(csr, perm_host);
        const DupGroups dg = duplicate_groups(hashes, csr, perm_host, runs.qstart, runs.qlen, gt.gcls, gt.cls_gain.size(),
                                              path_env("FR_NO_DUP_GROUPS") != nullptr, 1);
        const WalkTileLayout wl = build_walk_tiles(runs.run_pos, runs.run_q0, runs.run_q1, runs.qstart, runs.qlen, runs.np);
        put_runs("", runs);
        put("run_lo", std::vector<uint32_t>(runs.run_q0.size(), 0u));
        put("perm_host", perm_host), put("perm", perm_host), put("gain", gt.gain), put("gexp", gt.gexp), put("gcls", gt.gcls);
        put("dcgtab", gt.dcgtab), put("termtab", gt.termtab), put("qnpos", gt.qnpos), put("qnneg", gt.qnneg), put("gkey", dg.gkey16);
        put("wt_start", wl.wt_start), put("run_wt0", wl.run_wt0), put("segtab", wl.seg), put("wofs", wl.wofs);
        num("n", csr.n), num("d", csr.d), num("dq", (csr.d + 3) / 4), num("nwt", wl.wt_start.size() - 1), num("ncls", gt.ncls);
        num("tablen", gt.tablen), num("termtab_len", gt.termtab.size()), num("relmask", gt.relmask), num("labels_small_int", gt.labels_small_int ? 1u : 0u);
        num("key_bits", dg.key_bits), num("key_cls_bits", dg.key_cls_bits), num("dup_groups", dg.dup_groups), num("verify_xs", (uint64_t)dg.verify_xs);
        num("no_document", NO_DOCUMENT), num("walk_tile", WALK_TILE), num("dcg_ranks", (uint64_t)DCG_RANKS);
        if (parent_queries) {
            const std::vector<uint32_t> pq(parent_queries, parent_queries + n_parent_queries);
            HostCSR cut;  // the view's own CSR: the chosen queries of the dataset's, documents in its order
            cut.d = csr.d, cut.x = csr.x, cut.nq = pq.size();
            cut.qoff.assign(1, 0);
            for (uint32_t q : pq) {
                if (q >= csr.nq) fr::fail_str("fr_debug_dataset_layout: no such query");
                cut.perm.insert(cut.perm.end(), csr.perm.begin() + csr.qoff[q], csr.perm.begin() + csr.qoff[q + 1]);
                cut.gain.insert(cut.gain.end(), csr.gain.begin() + csr.qoff[q], csr.gain.begin() + csr.qoff[q + 1]);
                cut.qoff.push_back((uint32_t)cut.perm.size());
            }
            cut.n = cut.perm.size();
            const HostCSR& vcsr = view ? require_dataset(view).view->host_csr() : cut;
            if (vcsr.n == 0 || vcsr.nq == 0 || pq.size() != vcsr.nq) fr::fail_str("create_view: empty view");
            RunPlan v;
            if (!plan_view_runs(runs.qstart, runs.qlen, perm_host, wl.wt_start, vcsr, pq, run_docs_target(), &v, &err)) fr::fail_str(err);
            put_runs("view_", v);
            put("view_run_lo", v.run_lo), put("view_run_wt0", v.run_wt0), put("view_vtiles", v.vtiles), put("view_wlist", v.wlist);
            put("view_perm_host", v.perm_host);
            num("view_n", vcsr.n), num("view_nvtiles", v.vtiles.size()), num("view_nwlist", v.wlist.size());
        }
        if (!table) return frjson::dump(scalars);
        const std::string name = accept_str("table", table);
        const auto it = tables.find(name);
        if (it == tables.end()) fr::fail_str("fr_debug_dataset_layout: no table named " + name);
        Value o = Value::object();
        o.set("bytes", Value::uint(it->second.size()));
        if (out_bytes != it->second.size() || (!out && out_bytes))
            fr::fail_str("fr_debug_dataset_layout: table " + name + " holds " + std::to_string(it->second.size()) + " bytes, the buffer " + std::to_string(out_bytes));
        if (out_bytes) std::memcpy(out, it->second.data(), out_bytes);
        return frjson::dump(o);
    });
}

// The same call sequence on ONE device (a one-rank communicator): librccl.so opens, its symbols bind, ncclCommInitAll /
// grouped ncclAllGather / ncclCommDestroy run and the data comes back.  What a one-GPU box can check of the exchange.
const void* fr_debug_rccl_selftest(int device) {
    return json_call([&]() {
        std::vector<double> block(16), got;
        for (size_t i = 0; i < block.size(); i++) block[i] = 0.5 + (double)i;
        frdev::RcclReport rep;
        std::string err;
        if (!frdev::rccl_allgather(std::vector<int>(1, device), block.data(), block.size(), &got, &rep, &err, 1)) fr::fail_str(err);
        return frjson::dump(rccl_report_to_json(rep));
    });
}

int fr_set_device(int ordinal) {
    std::string err;
    if (!frdev::set_device(ordinal, &err)) return 1;
    frdev::warm_device(ordinal);
    g_pinned_device = ordinal;  // train_model then stays on this device unless FR_DEVICES says otherwise
    return 0;
}

const char* fr_version(void) { return "fastrank_amd 0.1.0 (fastrank C ABI 0.9.0-dev / python 0.7.0)"; }

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

struct FrTrainer {
    std::unique_ptr<fr::CATrainer> t;
    std::chrono::steady_clock::time_point t0;
    std::shared_ptr<fr::DataCore> core;  // (its api_mu serialises the calls on this handle with other jobs on the dataset)
    std::vector<unsigned char> capture_blob;  // fr_ca_capture_take: the arrays of the events last described, until they are fetched
};

void* fr_ca_begin(const void* train_request_json, const CDataset* dataset, uint32_t restart_begin,
                  uint32_t restart_end, const void** error_out) {
    if (error_out) *error_out = nullptr;
    FrTrainer* h = nullptr;
    const void* st = status_call([&]() {
        const CDataset& ds = require_dataset(dataset);
        ParsedRequest rq = parse_train_request(accept_str("train_request_json", train_request_json));
        if (rq.learner != Learner::CoordinateAscent) fr::fail_str("fr_ca_begin: only CoordinateAscent");
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::Evaluator ev = fr::make_evaluator(*ds.view, rq.measure, rq.has_qrel ? &rq.qrel : nullptr);
        if (ds.view->host_csr().nq == 0) fr::fail_str("assertion failed: !data.queries().is_empty()");
        auto holder = std::make_unique<FrTrainer>();
        holder->t0 = std::chrono::steady_clock::now();
        holder->t = std::make_unique<fr::CATrainer>(ds.view, std::move(ev), rq.ca, restart_begin, restart_end);
        holder->core = ds.view->core;
        h = holder.release();
    });
    if (st) {
        if (error_out) *error_out = st; else free((void*)st);
        return nullptr;
    }
    return h;
}

void* fr_ca_begin_query_shard(const void* train_request_json, const CDataset* dataset, uint64_t total_queries,
                              fr_allreduce_sum_fn allreduce, void* ctx, const void** error_out) {
    if (error_out) *error_out = nullptr;
    FrTrainer* h = nullptr;
    const void* st = status_call([&]() {
        const CDataset& ds = require_dataset(dataset);
        ParsedRequest rq = parse_train_request(accept_str("train_request_json", train_request_json));
        if (rq.learner != Learner::CoordinateAscent) fr::fail_str("fr_ca_begin_query_shard: only CoordinateAscent");
        if (!allreduce) fr::fail_str("fr_ca_begin_query_shard: allreduce callback is null!");
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::Evaluator ev = fr::make_evaluator(*ds.view, rq.measure, rq.has_qrel ? &rq.qrel : nullptr);
        if (total_queries == 0) fr::fail_str("assertion failed: !data.queries().is_empty()");
        fr::QueryShard shard;
        shard.total_queries = total_queries;
        shard.allreduce = [allreduce, ctx](double* v, size_t n) {
            if (allreduce(ctx, v, n) != 0) fr::fail_str("query-shard allreduce callback failed");
        };
        auto holder = std::make_unique<FrTrainer>();
        holder->t0 = std::chrono::steady_clock::now();
        holder->t = std::make_unique<fr::CATrainer>(ds.view, std::move(ev), rq.ca, 0u, rq.ca.num_restarts, std::move(shard));
        holder->core = ds.view->core;
        h = holder.release();
    });
    if (st) {
        if (error_out) *error_out = st; else free((void*)st);
        return nullptr;
    }
    return h;
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

// Tick capture (include/fastrank.h; DeviceDataset::capture_enable): a test hook, no product path calls it.
const void* fr_ca_capture(void* trainer, int on) {
    return status_call([&]() {
        if (!trainer) fr::fail_str("trainer pointer is null!");
        FrTrainer* h = (FrTrainer*)trainer;
        std::lock_guard<std::mutex> lk(h->core->api_mu);
        h->t->capture(on != 0);
        if (!on) h->capture_blob.clear();
    });
}

// table == NULL: moves the log out of the device dataset and describes it -- JSON {"events": [...], "bytes": n}, every array
// of an event as {"off": byte offset into the blob, "n": elements}; table == "blob": the n bytes, after which they are
// forgotten (the name / out-buffer protocol of fr_debug_device_form).
const void* fr_ca_capture_take(void* trainer, const void* table, void* out, size_t out_bytes) {
    return json_call([&]() {
        if (!trainer) fr::fail_str("trainer pointer is null!");
        FrTrainer* h = (FrTrainer*)trainer;
        std::lock_guard<std::mutex> lk(h->core->api_mu);
        Value o = Value::object();
        if (table) {
            const std::string name = accept_str("table", table);
            if (name != "blob") fr::fail_str("fr_ca_capture_take: no table named " + name);
            if (out_bytes != h->capture_blob.size() || (!out && out_bytes))
                fr::fail_str("fr_ca_capture_take: the blob holds " + std::to_string(h->capture_blob.size()) + " bytes, the buffer " + std::to_string(out_bytes));
            if (out_bytes) std::memcpy(out, h->capture_blob.data(), out_bytes);
            o.set("bytes", Value::uint(out_bytes));
            h->capture_blob.clear();
            h->capture_blob.shrink_to_fit();
            return frjson::dump(o);
        }
        std::vector<frdev::LsCapture> log;
        h->t->take_capture(&log);
        std::vector<unsigned char>& blob = h->capture_blob;
        blob.clear();
        auto put = [&blob](const auto& v) {
            using T = typename std::remove_reference_t<decltype(v)>::value_type;
            blob.resize((blob.size() + 7) & ~size_t(7));
            Value r = Value::object();
            r.set("off", Value::uint(blob.size()));
            r.set("n", Value::uint(v.size()));
            const size_t at = blob.size();
            blob.resize(at + v.size() * sizeof(T));
            if (!v.empty()) std::memcpy(blob.data() + at, v.data(), v.size() * sizeof(T));
            return r;
        };
        Value events = Value::array();
        for (const frdev::LsCapture& e : log) {
            Value ev = Value::object();
            if (e.store) {
                ev.set("type", Value::string("store"));
                ev.set("slot", Value::sint(e.slot));
                ev.set("v", put(e.v));
                events.push(std::move(ev));
                continue;
            }
            static const char* const kinds[] = {"topk", "rr", "fullrank"};
            ev.set("type", Value::string("tick"));
            ev.set("ctx", Value::sint(e.ctx));
            ev.set("kind", Value::string(kinds[e.kind]));
            ev.set("measure", Value::sint(e.measure));
            ev.set("depth", Value::sint(e.depth));
            Value groups = Value::array();
            for (const frdev::LineGroup& lg : e.groups) {
                Value g = Value::object();
                g.set("feature", Value::uint(lg.feature));
                g.set("weights", put(lg.weights));
                g.set("candidates", put(lg.candidates));
                g.set("resident_slot", Value::sint(lg.resident_slot));
                g.set("resident_owner", Value::uint(lg.resident_owner));
                g.set("has_update", Value::boolean(lg.has_update));
                g.set("upd_feature", Value::uint(lg.upd_feature));
                // (the doubles travel as bytes: resident_norm, resident_base_f, resident_err, upd_norm, upd_base_f, upd_cand)
                g.set("params", put(std::vector<double>{lg.resident_norm, lg.resident_base_f, lg.resident_err, lg.upd_norm, lg.upd_base_f, lg.upd_cand}));
                groups.push(std::move(g));
            }
            ev.set("groups", std::move(groups));
            ev.set("gorder", put(e.gorder));
            ev.set("nverify", Value::uint(e.nverify));
            ev.set("approx", Value::boolean(e.approx));
            ev.set("resident", Value::boolean(e.resident));
            ev.set("ready", Value::boolean(e.ready));
            Value inst = Value::object();
            if (e.kind == 0) {
                inst.set("k", Value::sint(e.kbucket));
                inst.set("xs_used", Value::sint(e.xs_used));
                inst.set("xs_pinned", Value::boolean(e.xs_pinned));
            } else {
                inst.set("classes", put(e.classes));
            }
            inst.set("dup", Value::boolean(e.dup));
            ev.set("inst", std::move(inst));
            ev.set("redo", put(e.redo));
            ev.set("redo_groups", Value::uint(e.redo_groups));
            ev.set("means", put(e.means));
            ev.set("nq", Value::uint(e.nq));
            ev.set("ldm", Value::uint(e.ldm));
            ev.set("np", Value::uint(e.np));
            ev.set("has_matrix", Value::boolean(e.has_matrix));
            ev.set("matrix", put(e.matrix));
            ev.set("res_slots", put(e.res_slots));
            ev.set("res", put(e.res));
            events.push(std::move(ev));
        }
        o.set("events", std::move(events));
        o.set("bytes", Value::uint(blob.size()));
        return frjson::dump(o);
    });
}

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

const void* fr_debug_tree_plan(void) {
    return json_call([&]() {
        const frdev::TreePlan p = frdev::last_tree_plan();
        Value o = Value::object();
        if (p.path == frdev::TreePlan::NONE) {
            o.set("path", Value::null());
            return frjson::dump(o);
        }
        o.set("path", Value::string(p.path == frdev::TreePlan::RANK ? "rank" : p.path == frdev::TreePlan::LDS ? "lds" : "l2"));
        o.set("cache_hit", Value::boolean(p.cache_hit));
        if (p.path == frdev::TreePlan::LDS) o.set("docs", Value::uint(p.docs)), o.set("parts", Value::uint(p.parts));
        if (p.path == frdev::TreePlan::L2) o.set("rows_in_lds", Value::boolean(p.rows_in_lds));
        if (p.path == frdev::TreePlan::RANK) o.set("nslots", Value::uint(p.nslots)), o.set("nrounds", Value::uint(p.nrounds));
        if (p.path != frdev::TreePlan::L2) {
            Value a = Value::array();
            for (const auto& b : p.batches) {
                Value pair = Value::array();
                pair.push(Value::uint(b.first)), pair.push(Value::uint(b.second));
                a.push(std::move(pair));
            }
            o.set("batches", std::move(a));
        }
        return frjson::dump(o);
    });
}

// `model`'s forest packed for one of the three encodings (csrc/forest_pack.hpp) on a dataset of dataset_features features,
// with the packers' options unset: what score_trees would upload.  No device is touched.  The name / out-buffer protocol of
// fr_debug_device_form.
const void* fr_debug_forest_pack(const CModel* model, uint32_t dataset_features, const void* encoding, const void* table, void* out, size_t out_bytes) {
    return json_call([&]() {
        const CModel& m = require_model(model);
        frdev::FlatTrees ft;
        if (!fr::flat_trees_of(m.actual, &ft)) fr::fail_str("fr_debug_forest_pack: the model is neither a DecisionTree nor an Ensemble of DecisionTrees");
        const std::string enc = accept_str("encoding", encoding);
        const uint32_t d = dataset_features, dq = (d + 3) / 4;
        std::vector<std::pair<std::string, std::pair<const void*, size_t>>> tables;  // name -> (bytes, count of bytes)
        auto add = [&](const char* name, const auto& v) { tables.push_back({name, {v.data(), v.size() * sizeof(v[0])}}); };
        frdev::RankForest rank;
        frdev::LdsForest lds;
        std::vector<frdev::TreeNodeDev> nodes;
        std::vector<int32_t> roots;
        std::vector<double> tweights;
        Value o = Value::object();
        bool admitted = true;
        const std::vector<uint32_t>* desc = nullptr;
        unsigned docs = 0, parts = 0;
        if (enc == "rank") {
            admitted = frdev::pack_forest_rank(ft, d, dq, frdev::ForestPackOptions(), &rank);
            if (admitted) {
                add("fdesc", rank.fdesc), add("tables", rank.tables), add("rdesc", rank.rdesc), add("forest", rank.forest);
                add("desc", rank.desc), add("leafprod", rank.leafprod);
                o.set("lds_bytes", Value::uint(rank.lds_bytes)), o.set("nslots", Value::uint(rank.nslots)), o.set("nrounds", Value::uint(rank.nrounds));
                desc = &rank.desc;
            }
        } else if (std::sscanf(enc.c_str(), "lds:%u,%u", &docs, &parts) == 2) {
            const frdev::TreeShape* shape = nullptr;
            for (const frdev::TreeShape& sh : frdev::TREE_SHAPES)
                if (sh.docs == docs && sh.parts == parts) shape = &sh;
            if (!shape) fr::fail_str("fr_debug_forest_pack: no block shape " + enc.substr(4));
            admitted = frdev::pack_forest_lds(ft, *shape, d, dq, frdev::ForestPackOptions(), &lds);
            if (admitted) {
                add("forest", lds.forest), add("desc", lds.desc), add("leafprod", lds.leafprod);
                o.set("lds_bytes", Value::uint(lds.lds_bytes));
                desc = &lds.desc;
            }
        } else if (enc == "l2") {
            frdev::adjacent_children_layout(ft, nodes, roots);
            tweights = ft.weight;
            tweights.resize(ft.root.size(), 1.0);
            add("nodes", nodes), add("roots", roots), add("tweights", tweights);
        } else {
            fr::fail_str("fr_debug_forest_pack: encoding is \"rank\", \"lds:DOCS,PARTS\" or \"l2\", not " + enc);
        }
        o.set("admitted", Value::boolean(admitted));
        char hash[24];
        snprintf(hash, sizeof hash, "%016llx", (unsigned long long)frdev::forest_hash(ft));
        o.set("hash", Value::string(hash));  // the packed-forest cache's key, as hex
        Value sizes = Value::object();
        for (const auto& kv : tables) sizes.set(kv.first.c_str(), Value::uint(kv.second.second));
        o.set("tables", std::move(sizes));
        if (desc) {
            Value a = Value::array();
            for (const auto& b : frdev::tree_plan_batches(*desc)) {
                Value pair = Value::array();
                pair.push(Value::uint(b.first)), pair.push(Value::uint(b.second));
                a.push(std::move(pair));
            }
            o.set("batches", std::move(a));
        }
        if (table) {
            const std::string name = accept_str("table", table);
            const std::pair<const void*, size_t>* found = nullptr;
            for (const auto& kv : tables)
                if (kv.first == name) found = &kv.second;
            if (!found) fr::fail_str("fr_debug_forest_pack: encoding " + enc + (admitted ? " has no table " : " refused the forest: no table ") + name);
            if (found->second && (!out || out_bytes != found->second))
                fr::fail_str("fr_debug_forest_pack: table " + name + " holds " + std::to_string(found->second) + " bytes, the buffer " + std::to_string(out_bytes));
            if (found->second) std::memcpy(out, found->first, found->second);
        }
        return frjson::dump(o);
    });
}

const void* fr_debug_metric_plan(void) {
    return json_call([&]() {
        const frdev::MetricPlan p = frdev::last_metric_plan();
        Value o = Value::object();
        if (p.measure < 0) {
            o.set("measure", Value::null());
            return frjson::dump(o);
        }
        o.set("measure", Value::string(frmeasure::measure_table()[p.measure].names[0]));
        o.set("depth", p.depth < 0 ? Value::null() : Value::uint((uint64_t)p.depth));
        o.set("slots", Value::uint(p.slots));
        Value a = Value::array();
        for (const auto& c : p.classes) {
            Value e = Value::object();
            e.set("npad", Value::uint(c.npad)), e.set("queries", Value::uint(c.queries));
            e.set("kernel", Value::string(c.topk ? "topk" : "sort"));
            a.push(std::move(e));
        }
        o.set("classes", std::move(a));
        return frjson::dump(o);
    });
}

// measures_host.hpp's scalar form of one of the five cut-off measures over a RANKED list of n gains (no device): what the
// kernels are held to.  measure: the evaluator's name; norm: the query's entry of the norms (measures_host.hpp lists them).
const void* fr_debug_measure_ranked(const void* evaluator, const float* gains, size_t n, double norm, double* out) {
    return status_call([&]() {
        std::string name = accept_str("evaluator_name", evaluator);
        if ((n && !gains) || !out) fr::fail_str("NULL pointer: ranked gains");
        int64_t depth = -1;
        const size_t at = name.find('@');
        if (at != std::string::npos) {
            depth = (int64_t)std::strtoull(name.c_str() + at + 1, nullptr, 10);
            name.resize(at);
        }
        for (auto& ch : name) ch = (char)std::tolower((unsigned char)ch);
        frmeasure::Resolved res;
        std::string rule;
        if (!frmeasure::resolve(name, depth, &res, &rule) || !frmeasure::is_cut_measure(res.measure))
            fr::fail_str(rule.empty() ? "fr_debug_measure_ranked: not one of dcg, precision, recall, success, err: \"" + name + "\"" : rule);
        std::vector<double> gexp(n);
        for (size_t i = 0; i < n; i++) gexp[i] = std::pow(2.0, (double)gains[i]) - 1.0;
        *out = frmeasure::cut_measure_at(res.measure, gains, gexp.data(), n, depth, norm);
    });
}

int fr_debug_metric_topk_pays(int64_t depth, uint32_t npad) { return frmeasure::metric_topk_pays(depth, npad) ? 1 : 0; }

const void* fr_predict_scores_dense(const CModel* model, const CDataset* dataset, double* out, size_t out_len) {
    return status_call([&]() {
        const CModel& m = require_model(model);
        const CDataset& ds = require_dataset(dataset);
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        if (view.instances.empty()) return;
        frdev::DeviceDataset& dev = view.device();
        fr::score_model(view, m.actual);
        std::string err;
        if (!dev.download_scores(0, out, out_len, &err)) fr::fail_str(err);
    });
}

// ---------------------------------------------------------------------------------------------
// Model explanation (csrc/explain_host.hpp, explain.hip)
// ---------------------------------------------------------------------------------------------
namespace {

// the documents of a view as explain.hip's kernels visit them
frdev::ExDocs explain_docs(fr::DatasetView& view) {
    frdev::DeviceDataset::TileForm tf;
    std::string err;
    if (!view.device().tile_form(&tf, &err)) fr::fail_str(err);
    if (tf.nonfinite) fr::fail_str("explain: the dataset holds inf or NaN feature values");
    frdev::ExDocs docs;
    docs.xb = tf.xb, docs.dq = (uint32_t)tf.dq, docs.d = (uint32_t)tf.d, docs.device = tf.device;
    docs.pos.reserve(tf.n), docs.ids.reserve(tf.n);
    for (size_t p = 0; p < tf.np; p++)
        if (tf.perm_host[p] != 0xFFFFFFFFu) docs.pos.push_back((uint32_t)p), docs.ids.push_back(tf.perm_host[p]);
    return docs;
}

// bytes of device memory an explanation's output may take: what is free less a margin, or FR_EXPLAIN_MAX_BYTES if smaller
size_t explain_budget() {
    const size_t free_b = frdev::device_free_bytes(), margin = (size_t)256 << 20;
    size_t budget = free_b > margin ? free_b - margin : 0;
    if (free_b == 0) budget = std::numeric_limits<size_t>::max();  // (unknown)
    if (const char* e = std::getenv("FR_EXPLAIN_MAX_BYTES")) budget = std::min<size_t>(budget, (size_t)std::strtoull(e, nullptr, 10));
    return budget;
}

struct ExplainJob {
    fr::ExplainModel em;
    fr::ExplainPlan plan;
    frdev::ExDocs docs;
    std::vector<uint32_t> view_feats;  // the dataset's feature ids, ascending: the output's columns
    std::vector<int64_t> out_col;      // model feature -> output column, -1: a feature the dataset does not hold (phi = 0.0)
    frdev::ExTimes cover_t;
};

// everything up to the launch: the model's check (before any device is touched), the background's covers, the path table
ExplainJob explain_prepare(const CModel& m, const CDataset& ds, const CDataset* bg) {
    ExplainJob job;
    job.em = fr::explain_model(m.actual);
    fr::DatasetView& view = *ds.view;
    fr::DatasetView& bview = bg ? *bg->view : view;
    if (bview.instances.empty()) fr::fail_str("explain: the background dataset holds no instance");
    job.view_feats = view.features;
    std::sort(job.view_feats.begin(), job.view_feats.end());
    if (view.instances.empty()) return job;
    job.docs = explain_docs(view);
    for (uint32_t f : job.em.feats) {
        const auto it = std::lower_bound(job.view_feats.begin(), job.view_feats.end(), f);
        const bool listed = it != job.view_feats.end() && *it == f;
        if (!listed && f < job.docs.d)
            fr::fail_str("explain: the model splits on feature " + std::to_string(f) + ", which the dataset's matrix holds but this feature sample does not list");
        job.out_col.push_back(listed ? (int64_t)(it - job.view_feats.begin()) : -1);
    }
    const frdev::ExWalk walk = fr::explain_walk(job.em);
    std::vector<uint32_t> counts;
    std::string err;
    if (&bview == &view) {
        if (!frdev::explain_covers(job.docs, walk, &counts, &job.cover_t, &err)) fr::fail_str(err);
    } else {
        const frdev::ExDocs bdocs = explain_docs(bview);
        if (bdocs.device != job.docs.device) fr::fail_str("explain: the background dataset lives on another device");
        if (!frdev::explain_covers(bdocs, walk, &counts, &job.cover_t, &err)) fr::fail_str(err);
    }
    job.plan = fr::explain_plan(job.em, counts, job.docs.d);
    return job;
}

Value explain_status(const ExplainJob& job, const frdev::ExTimes& t) {
    Value o = Value::object(), ids = Value::array(), sc = Value::array();
    for (uint32_t f : job.view_feats) ids.push(Value::uint(f));
    std::vector<uint64_t> counts(job.view_feats.size(), 0);
    for (size_t k = 0; k < job.out_col.size(); k++)
        if (job.out_col[k] >= 0) counts[(size_t)job.out_col[k]] = job.em.split_counts[k];
    for (uint64_t c : counts) sc.push(Value::uint(c));
    o.set("feature_ids", std::move(ids));
    o.set("split_counts", std::move(sc));
    o.set("expected_value", Value::number(job.plan.bias));
    o.set("trees", Value::uint(job.em.trees.size()));
    o.set("leaf_paths", Value::uint(job.plan.tab.value.size()));
    o.set("max_path", Value::uint(job.plan.tab.max_path));
    o.set("documents", Value::uint(job.docs.pos.size()));
    o.set("cover_ms", Value::number(job.cover_t.kernel_ms));
    o.set("kernel_ms", Value::number(t.kernel_ms));
    o.set("copy_ms", Value::number(t.copy_ms));
    return o;
}

// the two handles' locks (one when they share a core), taken together
struct ExplainLocks {
    std::unique_lock<std::mutex> a, b;
    ExplainLocks(const CDataset& ds, const CDataset* bg) {
        std::mutex& ma = api_mu_of(ds);
        std::mutex* mb = bg ? &api_mu_of(*bg) : nullptr;
        if (mb && mb != &ma) {
            a = std::unique_lock<std::mutex>(ma, std::defer_lock), b = std::unique_lock<std::mutex>(*mb, std::defer_lock);
            std::lock(a, b);
        } else {
            a = std::unique_lock<std::mutex>(ma);
        }
    }
};

}  // namespace

const CResult* fr_train_model_with(const void* train_request_json, const CDataset* dataset, const CDataset* valid_dataset_or_null,
                                   const CModel* init_model_or_null) {
    if (!valid_dataset_or_null && !init_model_or_null) return train_model((void*)train_request_json, (void*)dataset);
    return c_call<CModel>([&]() {
        const CDataset& ds = require_dataset(dataset);
        ParsedRequest rq = parse_train_request(accept_str("train_request_json", train_request_json), valid_dataset_or_null != nullptr);
        if (rq.learner != Learner::LambdaMART)
            fr::fail_str(std::string("fr_train_model_with: a validation dataset and an init model are LambdaMART's; the request's learner is ") +
                         (rq.learner == Learner::CoordinateAscent ? "CoordinateAscent" : "RandomForest"));
        ExplainLocks lk(ds, valid_dataset_or_null);
        return new_model([&] {
            return train_lambdamart(ds.view, rq, valid_dataset_or_null ? valid_dataset_or_null->view : nullptr,
                                    init_model_or_null ? &init_model_or_null->actual : nullptr);
        });
    });
}

const void* fr_explain_dense(const CModel* model, const CDataset* dataset, const CDataset* background_or_null, double* out, size_t rows, size_t cols) {
    return json_call([&]() {
        const CModel& m = require_model(model);
        const CDataset& ds = require_dataset(dataset);
        ExplainLocks lk(ds, background_or_null);
        ExplainJob job = explain_prepare(m, ds, background_or_null);
        const size_t nf = job.view_feats.size();
        if (cols != nf + 1) fr::fail_str("fr_explain_dense: the dataset has " + std::to_string(nf) + " features, so cols must be " + std::to_string(nf + 1) + " (the bias comes last)");
        if (rows && !out) fr::fail_str("NULL pointer: fr_explain_dense out");
        frdev::ExTimes t;
        if (!job.docs.pos.empty()) {
            std::vector<double> phi;
            std::string err;
            if (!frdev::explain_values(job.docs, job.plan.tab, explain_budget(), &phi, &t, &err)) fr::fail_str(err);
            const size_t nc = job.plan.tab.ncols;
            for (size_t i = 0; i < job.docs.ids.size(); i++) {
                const size_t id = job.docs.ids[i];
                if (id >= rows) continue;
                double* row = out + id * cols;
                std::fill(row, row + nf, 0.0);
                for (size_t c = 0; c < nc; c++)
                    if (job.out_col[c] >= 0) row[job.out_col[c]] = phi[i * nc + c];
                row[nf] = job.plan.bias;
            }
        }
        return frjson::dump(explain_status(job, t));
    });
}

const void* fr_feature_importance(const CModel* model, const CDataset* dataset, const CDataset* background_or_null, double* out_mean_abs, size_t n_features) {
    return json_call([&]() {
        const CModel& m = require_model(model);
        const CDataset& ds = require_dataset(dataset);
        ExplainLocks lk(ds, background_or_null);
        ExplainJob job = explain_prepare(m, ds, background_or_null);
        const size_t nf = job.view_feats.size();
        if (n_features != nf) fr::fail_str("fr_feature_importance: the dataset has " + std::to_string(nf) + " features, n_features is " + std::to_string(n_features));
        if (nf && !out_mean_abs) fr::fail_str("NULL pointer: fr_feature_importance out_mean_abs");
        if (job.docs.pos.empty()) fr::fail_str("fr_feature_importance: the dataset holds no instance");
        frdev::ExTimes t;
        std::vector<double> sums;
        std::string err;
        if (!frdev::explain_sum_abs(job.docs, job.plan.tab, &sums, &t, &err)) fr::fail_str(err);
        std::fill(out_mean_abs, out_mean_abs + nf, 0.0);
        const double n = (double)job.docs.pos.size();
        for (size_t c = 0; c < sums.size(); c++)
            if (job.out_col[c] >= 0) out_mean_abs[job.out_col[c]] = sums[c] / n;
        return frjson::dump(explain_status(job, t));
    });
}

// The path table of `model` for the leaf counts leaf_counts[n_leaves] (the trees' leaves, depth first, tree after tree) on a
// dataset of dataset_features features, as JSON -- what the kernel would read.  No device is touched.
const void* fr_debug_explain_table(const CModel* model, const uint32_t* leaf_counts, size_t n_leaves, uint32_t dataset_features) {
    return json_call([&]() {
        const CModel& m = require_model(model);
        const fr::ExplainModel em = fr::explain_model(m.actual);
        const frdev::ExWalk walk = fr::explain_walk(em);
        if (n_leaves != walk.leaf0.back()) fr::fail_str("fr_debug_explain_table: the model has " + std::to_string(walk.leaf0.back()) + " leaves, n_leaves is " + std::to_string(n_leaves));
        if (n_leaves && !leaf_counts) fr::fail_str("NULL pointer: fr_debug_explain_table leaf_counts");
        const fr::ExplainPlan plan = fr::explain_plan(em, std::vector<uint32_t>(leaf_counts, leaf_counts + n_leaves), dataset_features);
        const frdev::ExTables& tab = plan.tab;
        auto uints = [](const std::vector<uint32_t>& v) {
            Value a = Value::array();
            for (uint32_t x : v) a.push(Value::uint(x));
            return a;
        };
        // (+-inf have no JSON form: the bounds travel as strings of their bits' hex)
        auto bits = [](const std::vector<double>& v) {
            Value a = Value::array();
            for (double x : v) {
                uint64_t b;
                std::memcpy(&b, &x, 8);
                char buf[24];
                snprintf(buf, sizeof buf, "%016llx", (unsigned long long)b);
                a.push(Value::string(buf));
            }
            return a;
        };
        Value o = Value::object();
        o.set("features", uints(em.feats));
        o.set("leaf0", uints(tab.leaf0)), o.set("feat0", uints(tab.feat0)), o.set("m", uints(tab.m)), o.set("eoff", uints(tab.eoff));
        o.set("slot", uints(tab.slot)), o.set("fid", uints(tab.fid)), o.set("col", uints(tab.col));
        o.set("weight", bits(tab.weight)), o.set("value", bits(tab.value)), o.set("lo", bits(tab.lo)), o.set("hi", bits(tab.hi)), o.set("z", bits(tab.z));
        o.set("bias", bits(std::vector<double>{plan.bias}));
        o.set("max_path", Value::uint(tab.max_path)), o.set("max_tree_feats", Value::uint(tab.max_tree_feats));
        o.set("lds_bytes", Value::uint(frdev::ex_lds_bytes(tab.max_path, tab.max_tree_feats)));
        return frjson::dump(o);
    });
}

// ---------------------------------------------------------------------------------------------
// Feature normalisation (csrc/normalize_host.hpp, normalize.hip)
// ---------------------------------------------------------------------------------------------
namespace {

// the instances `list` of a view (its iteration order, or a regrouping of it) as normalize.hip's kernels visit them
frdev::NormDocs normalize_docs(fr::DatasetView& view, const std::vector<uint32_t>& list) {
    frdev::DeviceDataset::TileForm tf;
    std::string err;
    if (!view.device().tile_form(&tf, &err)) fr::fail_str(err);
    const fr::DataCore& c = *view.core;
    frdev::NormDocs docs;
    docs.xb = tf.xb, docs.dq = (uint32_t)tf.dq, docs.d = (uint32_t)tf.d, docs.device = tf.device;
    std::vector<uint32_t> at(c.n, 0xFFFFFFFFu);
    for (size_t p = 0; p < tf.np; p++)
        if (tf.perm_host[p] != 0xFFFFFFFFu && tf.perm_host[p] < c.n) at[tf.perm_host[p]] = (uint32_t)p;
    docs.pos.reserve(list.size());
    for (uint32_t id : list) {
        if (id >= c.n || at[id] == 0xFFFFFFFFu) fr::fail_str("normalisation: instance " + std::to_string(id) + " has no place in the dataset's device form");
        docs.pos.push_back(at[id]);
    }
    docs.ids = list;
    if (!c.present_bits.empty()) docs.present = c.present_bits.data(), docs.present_words = c.present_words, docs.core_n = c.n;
    docs.fmask.assign((docs.d + 31) / 32, 0u);
    for (uint32_t f : view.features)
        if (f < docs.d) docs.fmask[f >> 5] |= 1u << (f & 31u);
    return docs;
}

[[noreturn]] void normalize_fail_stat(uint64_t cell) {
    fr::fail_str("non-finite value in feature " + std::to_string(cell & 0xFFFFFFFFu) + ", instance " + std::to_string(cell >> 32) +
                 ": feature statistics need finite values");
}

}  // namespace

const void* fr_fit_normalizer(const CDataset* dataset, const void* method) {
    return json_call([&]() {
        const CDataset& ds = require_dataset(dataset);
        fr::Normalizer nm;
        nm.kind = fr::norm_method(accept_str("method", method));
        if (nm.kind == fr::Normalizer::Sigmoid) return frjson::dump(fr::norm_to_json(nm));
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        if (view.instances.empty()) return frjson::dump(fr::norm_to_json(nm));
        const frdev::NormDocs docs = normalize_docs(view, view.instances);
        std::vector<frdev::NormRecord> records;
        uint64_t bad = frdev::NORM_NO_CELL;
        std::string err;
        if (!frdev::normalize_stats(docs, &records, &bad, nullptr, &err)) fr::fail_str(err);
        if (bad != frdev::NORM_NO_CELL) normalize_fail_stat(bad);
        for (uint32_t f : view.features) {
            fr::ComputedStats cs;
            if (f < docs.d && fr::norm_finish(records[f], &cs)) nm.stats[f] = cs;
        }
        return frjson::dump(fr::norm_to_json(nm));
    });
}

const CResult* fr_normalize_dataset(const CDataset* dataset, const void* normalizer_json) {
    return c_call<CDataset>([&]() {
        const CDataset& ds = require_dataset(dataset);
        const fr::Normalizer nm = fr::norm_from_json(parse_json_or_fail(accept_str("normalizer_json", normalizer_json)));
        fr::DatasetView& view = *ds.view;
        const fr::DataCore& c = *view.core;
        if (view.sampled || view.instances.size() != c.n) fr::fail_str("normalise the whole dataset, then sample it");
        if (!norm_memo_of(view.core).normalization.empty()) fr::fail_str("Cannot apply normalization twice!");
        if (c.n == 0 || c.d == 0) fr::fail_str("normalisation: the dataset holds no instance");
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<uint32_t> list(c.n);
        std::vector<uint32_t> qoff;
        if (nm.per_query()) {  // the queries' instances in the view's order, query after query (instances_by_query)
            std::vector<uint32_t> count(c.qnames.size(), 0);
            for (uint32_t id : view.instances) count[c.qix[id]]++;
            std::vector<uint32_t> start(c.qnames.size() + 1, 0);
            for (size_t q = 0; q < count.size(); q++) start[q + 1] = start[q] + count[q];
            std::vector<uint32_t> fill(start.begin(), start.end() - 1);
            for (uint32_t id : view.instances) list[fill[c.qix[id]]++] = id;
            for (size_t q = 0; q < count.size(); q++)
                if (count[q]) qoff.push_back(start[q]);
            qoff.push_back((uint32_t)c.n);
        } else {
            for (size_t i = 0; i < c.n; i++) list[i] = (uint32_t)i;
        }
        const frdev::NormDocs docs = normalize_docs(view, list);
        if (docs.d != c.d) fr::fail_str("normalisation: the device form holds " + std::to_string(docs.d) + " columns, the dataset " + std::to_string(c.d));
        const auto t_docs = std::chrono::steady_clock::now();
        auto core = std::make_shared<fr::DataCore>();
        core->x_own.resize(c.n * c.d);
        const auto t_alloc = std::chrono::steady_clock::now();
        frdev::NormTimes times;
        uint64_t bad = frdev::NORM_NO_CELL, bad_stat = frdev::NORM_NO_CELL;
        std::string err;
        if (nm.per_query()) {
            if (!frdev::normalize_per_query(docs, qoff, nm.kind == fr::Normalizer::PerQueryMaxMin ? frdev::NORM_M_MAXMIN : frdev::NORM_M_ZSCORE,
                                            core->x_own.data(), &bad_stat, &bad, &times, &err))
                fr::fail_str(err);
        } else {
            if (!frdev::normalize_apply(docs, fr::norm_params(nm, c.d), core->x_own.data(), &bad, &times, &err)) fr::fail_str(err);
        }
        if (bad_stat != frdev::NORM_NO_CELL) normalize_fail_stat(bad_stat);
        if (bad != frdev::NORM_NO_CELL)
            fr::fail_str(std::string("Normalization.") + nm.method() + " NaN: feature " + std::to_string(bad & 0xFFFFFFFFu) + ", instance " + std::to_string(bad >> 32));
        const auto t1 = std::chrono::steady_clock::now();
        core->n = c.n, core->d = c.d, core->x = core->x_own.data();
        core->gain = c.gain, core->qix = c.qix, core->qnames = c.qnames;
        core->has_docids = c.has_docids, core->docids = c.docids, core->doc_present = c.doc_present;
        core->features = c.features, core->feature_names = c.feature_names;
        core->present_bits = c.present_bits, core->present_words = c.present_words;
        auto* out = new CDataset();
        out->view = std::make_shared<fr::DatasetView>();
        out->view->core = core;
        out->view->features = view.features;
        out->view->instances = view.instances;
        // where the call's time went: the list and its positions; the new matrix's host memory; on the device the kernel, the
        // download and the rest (buffers, the list's upload); the new core's other fields
        const auto secs = [](auto a, auto b) { return std::chrono::duration<double>(b - a).count(); };
        const auto t2 = std::chrono::steady_clock::now();
        Value st = Value::object();
        st.set("prepare_seconds", Value::number(secs(t0, t_docs)));
        st.set("allocate_seconds", Value::number(secs(t_docs, t_alloc)));
        st.set("kernel_seconds", Value::number(times.kernel_ms * 1e-3));
        st.set("download_seconds", Value::number(times.copy_ms * 1e-3));
        st.set("device_other_seconds", Value::number(secs(t_alloc, t1) - (times.kernel_ms + times.copy_ms) * 1e-3));
        st.set("core_build_seconds", Value::number(secs(t1, t2)));
        st.set("total_seconds", Value::number(secs(t0, t2)));
        norm_memo_set(core, NormMemo{frjson::dump(fr::norm_to_json(nm)), frjson::dump(st)});
        return out;
    });
}

// ---------------------------------------------------------------------------------------------
// Model comparison (csrc/resample_host.hpp, kernels_resample.inc)
// ---------------------------------------------------------------------------------------------
namespace {

// the checked table through both kernels (a null output skips its kernel), then the host's report with the call's stats
Value resample_table(const double* V, size_t Q, size_t M, const fr::ResampleOptions& op, double* boot, double* perm) {
    fr::resample_check(V, Q, M);
    frdev::ResampleTimes times;
    std::string err;
    const auto t0 = std::chrono::steady_clock::now();
    if (!frdev::resample_run(V, Q, (uint32_t)M, op.trials, op.seed, boot, perm, &times, &err)) fr::fail_str(err);
    const auto t1 = std::chrono::steady_clock::now();
    Value o = fr::resample_report(V, Q, M, op.trials, op.alpha, boot, perm);
    const auto t2 = std::chrono::steady_clock::now();
    o.set("trials", Value::uint(op.trials)), o.set("seed", Value::uint(op.seed)), o.set("alpha", Value::number(op.alpha));
    o.set("boot_path", Value::string(times.lds ? "lds" : "global"));
    o.set("boot_ms", Value::number(times.boot_ms)), o.set("perm_ms", Value::number(times.perm_ms));
    o.set("upload_ms", Value::number(times.upload_ms)), o.set("download_ms", Value::number(times.download_ms));
    o.set("device_call_ms", Value::number(std::chrono::duration<double, std::milli>(t1 - t0).count()));
    o.set("report_ms", Value::number(std::chrono::duration<double, std::milli>(t2 - t1).count()));
    return o;
}

}  // namespace

const void* fr_resample(const double* values, size_t nq, size_t ncols, const void* options_json, double* out_boot, double* out_perm) {
    return json_call([&]() {
        const fr::ResampleOptions op = fr::resample_options_from_json(parse_json_or_fail(accept_str("options_json", options_json)));
        return frjson::dump(resample_table(values, nq, ncols, op, out_boot, out_perm));
    });
}

const void* fr_compare_models(const CModel* const* models, size_t n_models, const CDataset* dataset, const CQRel* qrel, const void* evaluator_name,
                              const void* options_json) {
    return json_call([&]() {
        const CDataset& ds = require_dataset(dataset);
        const std::string name = accept_str("evaluator_name", evaluator_name);
        const fr::ResampleOptions op = fr::resample_options_from_json(parse_json_or_fail(accept_str("options_json", options_json)));
        if (n_models < 1 || n_models > frresample::MAX_SYSTEMS)
            fr::fail_str("invalid value: a comparison takes between 1 and " + std::to_string(frresample::MAX_SYSTEMS) + " systems, not " + std::to_string(n_models));
        if (!models) fr::fail_str("NULL pointer: models");
        for (size_t c = 0; c < n_models; c++) require_model(models[c]);
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        fr::Evaluator ev = fr::make_evaluator(view, name, qrel ? &qrel->actual : nullptr);
        if (view.instances.empty()) fr::fail_str("invalid value: a comparison needs at least one query");
        // every model through fr_evaluate_dense's path on the one view: the same queries in the same order for all
        frdev::DeviceDataset& dev = view.device();
        const size_t Q = dev.nq(), M = n_models;
        std::vector<double> V(Q * M), column(Q);
        std::string err;
        for (size_t c = 0; c < M; c++) {
            fr::score_model(view, models[c]->actual);
            if (!dev.metric_from_scores(ev.measure, ev.depth, ev.norms.data(), 1, false, &err)) fr::fail_str(err);
            fr::check_flags(dev);
            if (!dev.download_per_query(1, column.data(), &err)) fr::fail_str(err);
            for (size_t q = 0; q < Q; q++) V[q * M + c] = column[q];
        }
        std::vector<double> boot((size_t)op.trials * M), perm(M > 1 ? (size_t)op.trials * M : 0);  // (one system: nothing to permute)
        Value o = resample_table(V.data(), Q, M, op, boot.data(), M > 1 ? perm.data() : nullptr);
        o.set("queries", Value::uint(Q));
        return frjson::dump(o);
    });
}

// ---------------------------------------------------------------------------------------------
// Permutation importance (csrc/permute_host.hpp, kernels_permute.inc)
// ---------------------------------------------------------------------------------------------
namespace {

// I (the view's instance ids ascending) and, for scope "query", each one's query
void permute_view_lists(const fr::DatasetView& view, bool per_query, std::vector<uint32_t>* ids, std::vector<uint32_t>* query_of) {
    *ids = view.instances;
    std::sort(ids->begin(), ids->end());
    query_of->clear();
    if (per_query)
        for (uint32_t id : *ids) query_of->push_back(view.core->qix[id]);
}

struct PermuteEnd {
    frdev::DeviceDataset& dev;
    ~PermuteEnd() { dev.permute_end(); }
};

}  // namespace

const void* fr_permutation_importance(const CModel* model, const CDataset* dataset, const CQRel* qrel, const void* evaluator_name, const void* options_json,
                                      double* out_values, size_t out_len, double* out_per_query) {
    return json_call([&]() {
        using clk = std::chrono::steady_clock;
        auto ms_since = [](clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); };
        const CModel& cm = require_model(model);
        const CDataset& ds = require_dataset(dataset);
        const std::string name = accept_str("evaluator_name", evaluator_name);
        const fr::PermuteOptions op = fr::permute_options_from_json(parse_json_or_fail(accept_str("options_json", options_json)));
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        const fr::Model& m = cm.actual;
        // every refusal that needs no device
        const fr::PermuteShape shape = fr::permute_model_shape(m);
        const std::vector<uint32_t> feats = fr::permute_features(op, view.features);
        if (view.instances.empty()) fr::fail_str("invalid value: permutation importance needs at least one document");
        const size_t F = feats.size(), R = op.repeats;
        if (F * R > 0 && !out_values) fr::fail_str("NULL pointer: out_values");
        if (out_len < F * R) fr::fail_str("fr_permutation_importance: output buffer too small");
        fr::Evaluator ev = fr::make_evaluator(view, name, qrel ? &qrel->actual : nullptr);

        frdev::DeviceDataset& dev = view.device();
        const size_t Q = dev.nq(), d = dev.d();
        std::string err;
        frdev::PermuteStats stats;
        // the baseline: fr_evaluate_dense's path on the view itself
        const auto t_base = clk::now();
        double baseline = 0.0;
        std::vector<double> base_pq(Q);
        fr::score_model(view, m);
        if (!dev.metric_from_scores(ev.measure, ev.depth, ev.norms.data(), 1, false, &err)) fr::fail_str(err);
        fr::check_flags(dev);
        if (!dev.reduce_means(1, &baseline, &err) || !dev.download_per_query(1, base_pq.data(), &err)) fr::fail_str(err);
        const double baseline_ms = ms_since(t_base);

        // which features are launched for: a feature past the matrix reads 0.0 whatever the rows are
        const std::vector<double>& colmax = dev.column_absmax();
        std::vector<std::pair<uint32_t, size_t>> run;  // (feature, its index in feats), ascending by feature
        std::vector<uint32_t> skipped;
        for (size_t fi = 0; fi < F; fi++) {
            if (feats[fi] < d && (!op.skip_unused || fr::permute_feature_used(m, feats[fi], colmax)))
                run.emplace_back(feats[fi], fi);
            else
                skipped.push_back(feats[fi]);
        }
        std::sort(run.begin(), run.end());
        for (size_t i = 0; i < F * R; i++) out_values[i] = baseline;
        if (out_per_query) {
            for (size_t b = 0; b <= F * R; b++) std::memcpy(out_per_query + b * Q, base_pq.data(), Q * sizeof(double));
        }

        size_t chunks = 0, max_slots_used = 0;
        double metric_ms = 0.0, sources_ms = 0.0;
        if (!run.empty()) {
            // one permutation per (seed, r), as positions
            const auto t_src = clk::now();
            std::vector<uint32_t> ids, query_of;
            permute_view_lists(view, op.per_query, &ids, &query_of);
            size_t np = 0;
            const uint32_t* instance_at = dev.position_instances(&np);
            const std::vector<uint32_t> pos = fr::permute_position_table(instance_at, np, ids.data(), ids.size());
            std::vector<uint32_t> src_pos(R * np);
            {  // the repeats are independent: one host sort each, side by side
                const size_t nthreads = std::max<size_t>(1, std::min<size_t>({R, 16, (size_t)std::max(1u, std::thread::hardware_concurrency())}));
                auto work = [&](size_t tid) {
                    std::vector<uint32_t> src_index(ids.size());
                    for (size_t r = tid; r < R; r += nthreads) {
                        fr::permute_sources(op.seed, (uint32_t)r, op.per_query ? query_of.data() : nullptr, ids.size(), src_index.data());
                        fr::permute_positions(pos.data(), src_index.data(), ids.size(), np, src_pos.data() + r * np);
                    }
                };
                std::vector<std::thread> pool;
                for (size_t tid = 1; tid < nthreads; tid++) pool.emplace_back(work, tid);
                work(0);
                for (auto& th : pool) th.join();
            }
            sources_ms = ms_since(t_src);
            PermuteEnd guard{dev};
            if (!dev.permute_begin(src_pos.data(), (uint32_t)R, &stats, &err)) fr::fail_str(err);

            // the model as the kernels take it
            std::vector<frdev::PermuteMember> members;
            std::vector<std::vector<double>> weight_store;
            frdev::FlatTrees ft;
            auto add_flat = [&](const fr::Model& mm, double ens_w) {
                frdev::PermuteMember pm;
                pm.ens_weight = ens_w;
                if (mm.kind == fr::Model::Linear) {
                    weight_store.emplace_back(d, 0.0);
                    for (size_t j = 0; j < d && j < mm.weights.size(); j++) weight_store.back()[j] = mm.weights[j];
                    pm.kind = frdev::PermuteMember::LINEAR;
                } else {
                    pm.kind = frdev::PermuteMember::SINGLE, pm.fid = mm.fid, pm.dir = mm.dir;
                }
                members.push_back(pm);
            };
            const bool ensemble = shape == fr::PermuteShape::ENSEMBLE_LINEAR;
            if (shape == fr::PermuteShape::TREES) {
                if (m.kind == fr::Model::DecisionTree) {
                    ft.raw_single = true;
                    ft.root.push_back(fr::flatten_tree(*m.tree, ft));
                    ft.weight.push_back(1.0);
                } else {  // zip(weights, models) stops at the shorter (src/model.rs:106)
                    const size_t nt = std::min(m.members.size(), m.ens_weights.size());
                    for (size_t t = 0; t < nt; t++) {
                        ft.root.push_back(fr::flatten_tree(*m.members[t].tree, ft));
                        ft.weight.push_back(m.ens_weights[t]);
                    }
                }
                frdev::PermuteMember pm;
                pm.kind = frdev::PermuteMember::TREES, pm.trees = &ft;
                members.push_back(pm);
            } else if (ensemble) {
                const size_t nt = std::min(m.members.size(), m.ens_weights.size());
                weight_store.reserve(nt);
                for (size_t t = 0; t < nt; t++) add_flat(m.members[t], m.ens_weights[t]);
            } else {
                weight_store.reserve(1);
                add_flat(m, 1.0);
            }
            {  // (weight_store no longer grows: its vectors' addresses hold)
                size_t k = 0;
                for (auto& pm : members)
                    if (pm.kind == frdev::PermuteMember::LINEAR) pm.weights = weight_store[k++].data();
            }

            const size_t C = dev.permute_chunk_features(run.size(), (uint32_t)R, (size_t)op.max_slots, ensemble ? 2 : 1);
            std::vector<uint32_t> chunk_feats;
            std::vector<double> vals, pq;
            for (size_t c0 = 0; c0 < run.size(); c0 += C) {
                const size_t nf = std::min(C, run.size() - c0), B = nf * R;
                chunk_feats.resize(nf);
                for (size_t k = 0; k < nf; k++) chunk_feats[k] = run[c0 + k].first;
                if (!dev.permute_score(chunk_feats.data(), nf, members, ensemble, &stats, &err)) fr::fail_str(err);
                const auto t_metric = clk::now();
                if (!dev.metric_from_scores(ev.measure, ev.depth, ev.norms.data(), B, false, &err)) fr::fail_str(err);
                fr::check_flags(dev);
                vals.resize(B);
                if (!dev.reduce_means(B, vals.data(), &err)) fr::fail_str(err);
                metric_ms += ms_since(t_metric);
                if (out_per_query) {
                    pq.resize(Q * B);
                    if (!dev.download_per_query(B, pq.data(), &err)) fr::fail_str(err);
                }
                for (size_t k = 0; k < nf; k++) {
                    const size_t fi = run[c0 + k].second;
                    for (size_t r = 0; r < R; r++) {
                        out_values[fi * R + r] = vals[k * R + r];
                        if (out_per_query)
                            for (size_t q = 0; q < Q; q++) out_per_query[(fi * R + r) * Q + q] = pq[q * B + k * R + r];
                    }
                }
                chunks++;
                max_slots_used = std::max(max_slots_used, B);
            }
        }

        Value o = Value::object(), jf = Value::array(), jn = Value::array(), ji = Value::array(), js = Value::array(), jk = Value::array();
        for (size_t fi = 0; fi < F; fi++) {
            const fr::PermuteScore s = fr::permute_report(baseline, out_values + fi * R, R);
            jf.push(Value::uint(feats[fi])), jn.push(Value::string(view.core->feature_name(feats[fi])));
            ji.push(Value::number(s.importance)), js.push(Value::number(s.std));
        }
        for (uint32_t f : skipped) jk.push(Value::uint(f));
        o.set("features", jf), o.set("names", jn), o.set("baseline", Value::number(baseline)), o.set("importance", ji), o.set("std", js);
        o.set("skipped", jk), o.set("repeats", Value::uint(R)), o.set("seed", Value::uint(op.seed));
        o.set("scope", Value::string(op.per_query ? "query" : "dataset")), o.set("evaluator", Value::string(ev.name)), o.set("queries", Value::uint(Q));
        Value st = Value::object(), jl = Value::object();
        st.set("gather", Value::string(run.empty() ? "none" : (stats.gather_xcol ? "xcol" : "tiles")));
        st.set("rows", Value::string(stats.rows_in_lds ? "lds" : "global"));
        st.set("chunks", Value::uint(chunks)), st.set("slots", Value::uint(max_slots_used));
        st.set("score_ms", Value::number(stats.score_ms)), st.set("metric_ms", Value::number(metric_ms)), st.set("upload_ms", Value::number(stats.upload_ms));
        st.set("baseline_ms", Value::number(baseline_ms)), st.set("sources_ms", Value::number(sources_ms));
        jl.set("linear", Value::uint(stats.launches_linear)), jl.set("single", Value::uint(stats.launches_single));
        jl.set("trees", Value::uint(stats.launches_trees)), jl.set("axpy", Value::uint(stats.launches_axpy));
        st.set("launches", jl);
        o.set("stats", st);
        return frjson::dump(o);
    });
}

const void* fr_debug_permutation_sources(const CDataset* dataset, uint64_t seed, uint32_t repeat, const void* scope, uint32_t* out_src_by_instance,
                                         size_t out_len) {
    return json_call([&]() {
        const CDataset& ds = require_dataset(dataset);
        const bool per_query = fr::permute_scope_from_string(accept_str("scope", scope));
        if (repeat >= frpermute::MAX_REPEATS) fr::fail_str("invalid value: repeat must be below " + std::to_string(frpermute::MAX_REPEATS));
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        const fr::DatasetView& view = *ds.view;
        std::vector<uint32_t> ids, query_of;
        permute_view_lists(view, per_query, &ids, &query_of);
        if (!ids.empty() && (!out_src_by_instance || out_len <= ids.back())) fr::fail_str("fr_debug_permutation_sources: output buffer too small");
        std::vector<uint32_t> src_index(ids.size());
        fr::permute_sources(seed, repeat, per_query ? query_of.data() : nullptr, ids.size(), src_index.data());
        for (size_t i = 0; i < out_len; i++) out_src_by_instance[i] = 0xFFFFFFFFu;
        for (size_t i = 0; i < ids.size(); i++) out_src_by_instance[ids[i]] = ids[src_index[i]];
        Value o = Value::object();
        o.set("n", Value::uint(ids.size()));
        return frjson::dump(o);
    });
}

// per query of the view (its order) whether `queries` names it
static std::vector<unsigned char> debug_query_flags(const uint32_t* queries, size_t n_queries, size_t nq) {
    if (n_queries == 0) fr::fail_str("a query sample must name at least one query");
    std::vector<unsigned char> flags(nq, 0);
    for (size_t i = 0; i < n_queries; i++) {
        if (queries[i] >= nq) fr::fail_str("a query sample names query " + std::to_string(queries[i]) + " of " + std::to_string(nq));
        flags[queries[i]] = 1;
    }
    return flags;
}

// The sample LambdaMART's trainer uses for tree `tree` of the request parameters `params_json` ({"num_trees": ..}, the
// LambdaMART variant's payload) on this view: {"features": [ids ascending], "queries": [indices in the view's order]}; with
// validation_queries these are the sampled TRAINING queries.
// No device is touched.
const void* fr_debug_lambdamart_sample(const CDataset* dataset, const void* params_json, uint32_t tree) {
    return json_call([&]() {
        const CDataset& ds = require_dataset(dataset);
        const fr::LambdaMARTParams p = fr::LambdaMARTParams::from_json(parse_json_or_fail(accept_str("params_json", params_json)));
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        std::vector<uint32_t> feats = view.features;
        std::sort(feats.begin(), feats.end());
        const size_t nq = view.host_csr().nq;
        const fr::LambdaSplit split = fr::lambdamart_split(view, p);  // (held-out queries: the sample is drawn from the others)
        fr::Rand64 master(p.seed);
        fr::LambdaSample smp;
        for (uint32_t t = 0; t <= tree; t++) smp = fr::lambdamart_next_sample(master, feats.size(), nq, p, split.held.empty() ? nullptr : &split.train);
        Value o = Value::object(), f = Value::array(), q = Value::array();
        for (uint32_t s : smp.features) f.push(Value::uint(feats[s]));
        for (uint32_t x : smp.queries) q.push(Value::uint(x));
        o.set("features", std::move(f));
        o.set("queries", std::move(q));
        return frjson::dump(o);
    });
}

// LambdaMART's DART plan (csrc/lambdamart_dart.hpp) for the first `num_trees` trees of the request parameters `params_json`
// (the LambdaMART variant's payload; its own num_trees is not read): [{"dropped": [tree indices ascending], "before": [the
// weights w_0 .. w_{t-1}], "after": [w_0 .. w_t]}, ...], one entry per tree.  No device is touched.
const void* fr_debug_lambdamart_dart_plan(const void* params_json, uint32_t num_trees) {
    return json_call([&]() {
        const fr::LambdaMARTParams p = fr::LambdaMARTParams::from_json(parse_json_or_fail(accept_str("params_json", params_json)));
        fr::DartPlan plan(p.seed, p.drop_rate, p.max_drop, p.skip_drop);
        std::vector<double> w;
        Value out = Value::array();
        auto numbers = [](const std::vector<double>& v) {
            Value a = Value::array();
            for (double x : v) a.push(Value::number(x));
            return a;
        };
        for (uint32_t t = 0; t < num_trees; t++) {
            const std::vector<uint32_t> dropped = p.dart() ? plan.next(t) : std::vector<uint32_t>();
            Value o = Value::object(), d = Value::array();
            for (uint32_t i : dropped) d.push(Value::uint(i));
            o.set("dropped", std::move(d));
            o.set("before", numbers(w));
            fr::dart_reweight(w, dropped, p.learning_rate);
            o.set("after", numbers(w));
            out.push(std::move(o));
        }
        return frjson::dump(out);
    });
}

// dart_rescore_kernel on its own: `model` must be an Ensemble of DecisionTrees (its own weights are not read).  The leaf cache
// is filled for its trees as the trainer fills it, then the scores s = sum over include[k] (ascending tree indices) of
// weights[include[k]] * tree(x) are formed once.  scores_out[out_len]: by instance id; cache_out[n_weights][out_len]: the
// cache's rows by instance id (entries of instances outside the dataset are left as they are).  n_weights = the number of trees.
const void* fr_debug_dart_scores(const CDataset* dataset, const CModel* model, const double* weights, size_t n_weights,
                                 const uint32_t* include, size_t n_include, double* scores_out, uint16_t* cache_out, size_t out_len) {
    return status_call([&]() {
        const CModel& m = require_model(model);
        const CDataset& ds = require_dataset(dataset);
        const fr::Model& ens = m.actual;
        bool trees = ens.kind == fr::Model::Ensemble && !ens.members.empty();
        for (const auto& mm : ens.members) trees = trees && mm.kind == fr::Model::DecisionTree;
        if (!trees) fr::fail_str("fr_debug_dart_scores: the model must be an Ensemble of DecisionTrees");
        if (n_weights != ens.members.size()) fr::fail_str("fr_debug_dart_scores: one weight per tree of the model");
        if ((n_weights && !weights) || (n_include && !include) || (out_len && (!scores_out || !cache_out)))
            fr::fail_str("NULL pointer: fr_debug_dart_scores");
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        if (view.instances.empty()) return;
        frdev::DeviceDataset& dev = view.device();
        std::string err;
        struct End {
            frdev::DeviceDataset& d;
            ~End() { d.dart_end(); }
        } end{dev};
        if (!dev.dart_begin(n_weights, nullptr, &err)) fr::fail_str(err);
        for (size_t t = 0; t < n_weights; t++) {
            std::vector<fr::TreeNode*> leaves;
            fr::Model rm;
            rm.kind = fr::Model::DecisionTree;
            rm.tree = fr::LambdaMARTTrainer::number_leaves(*ens.members[t].tree, leaves);
            fr::score_model(view, rm, &dev);
            std::vector<double> values(leaves.size());
            for (size_t L = 0; L < leaves.size(); L++) values[L] = leaves[L]->value;
            if (!dev.dart_fill(t, values.data(), values.size(), &err)) fr::fail_str(err);
        }
        if (!dev.dart_rescore(weights, n_weights, include, n_include, &err)) fr::fail_str(err);
        if (!dev.download_scores(0, scores_out, out_len, &err)) fr::fail_str(err);
        for (size_t t = 0; t < n_weights; t++)
            if (!dev.dart_download_row(t, cache_out + t * out_len, out_len, &err)) fr::fail_str(err);
    });
}

// The body of the three gradient hooks below: one gradient pass on the model's scores, downloaded by instance id.  queries ==
// NULL: every query (need_queries: refused); else only the named queries' instances are computed and written.  options_json:
// nullptr for a hook that takes no options, else the address of the caller's string (fr_debug_lambda_gradients_opts below).
static const void* lambda_gradients_debug(const CModel* model, const CDataset* dataset, const CQRel* qrel, const void* measure, double sigma,
                                          const uint32_t* queries, size_t n_queries, bool need_queries, const void* const* options_json,
                                          double* lambda_out, double* weight_out, size_t out_len) {
    return status_call([&]() {
        const CModel& m = require_model(model);
        const CDataset& ds = require_dataset(dataset);
        std::string name = accept_str("measure", measure);
        fr::lambdamart_check_measure(name);
        fr::LambdaMARTParams op;
        uint64_t xe_key = 0;
        if (options_json) {
            const Value opts = parse_json_or_fail(accept_str("options_json", *options_json));
            if (!opts.is_object()) fr::fail_raw("Error(\"invalid type: expected a map of gradient options\", line: 0, column: 0)");
            for (const auto& kv : opts.obj) {
                if (kv.first == "truncation_level") op.truncation_level = fr::json_u32(kv.second, "truncation_level");
                else if (kv.first == "lambda_norm") op.lambda_norm = fr::json_bool(kv.second, "lambda_norm");
                else if (kv.first == "objective") op.objective = fr::LambdaMARTParams::objective_from_json(kv.second);
                else if (kv.first == "xe_key") xe_key = fr::json_u64(kv.second, "xe_key");
                else fr::fail_raw("Error(\"unknown field `" + kv.first + "`, expected `truncation_level` or `lambda_norm`\", line: 0, column: 0)");
            }
            op.check_objective_options();  // (before any device work, as the request parser does)
        }
        if (out_len && (!lambda_out || !weight_out)) fr::fail_str("NULL pointer: gradient outputs");
        if (need_queries && !queries) fr::fail_str("NULL pointer: query sample");
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        if (view.instances.empty()) return;
        std::vector<unsigned char> flags;
        if (queries) flags = debug_query_flags(queries, n_queries, view.host_csr().nq);
        const unsigned char* fl = queries ? flags.data() : nullptr;
        fr::Evaluator ev = fr::make_evaluator(view, op.objective_measure() ? std::string(op.objective_measure()) : name, qrel ? &qrel->actual : nullptr);
        frdev::DeviceDataset& dev = view.device();
        fr::score_model(view, m.actual);
        std::string err;
        if (!dev.lambda_gradients(ev.norms.data(), ev.depth, sigma, op.pass(fl, false, xe_key), &err)) fr::fail_str(err);
        if (!dev.lambda_download(lambda_out, weight_out, out_len, &err, fl)) fr::fail_str(err);
    });
}

const void* fr_debug_lambda_gradients(const CModel* model, const CDataset* dataset, const CQRel* qrel, const void* measure,
                                      double sigma, double* lambda_out, double* weight_out, size_t out_len) {
    return lambda_gradients_debug(model, dataset, qrel, measure, sigma, nullptr, 0, false, nullptr, lambda_out, weight_out, out_len);
}

// fr_debug_lambda_gradients for a query sample: queries[n_queries] = indices of the view's queries (its order).  Only their
// instances are written.
const void* fr_debug_lambda_gradients_sampled(const CModel* model, const CDataset* dataset, const CQRel* qrel, const void* measure,
                                              double sigma, const uint32_t* queries, size_t n_queries, double* lambda_out,
                                              double* weight_out, size_t out_len) {
    return lambda_gradients_debug(model, dataset, qrel, measure, sigma, queries, n_queries, true, nullptr, lambda_out, weight_out, out_len);
}

// fr_debug_lambda_gradients under the objective's options ("Truncation and normalisation"):
// options_json = {"truncation_level": u32, "lambda_norm": bool, "objective": "ndcg" | "map" | "mrr" | "xendcg", "xe_key": u64},
// every key optional (0 / false / "ndcg" / 0).  queries == NULL: the full pass; else the query sample of fr_debug_lambda_gradients_sampled.  With
// every option at its default this is the pass of the two other hooks.  `measure` must name NDCG whatever the objective;
// under "map" / "mrr" the norms are the AP / RR evaluator's ("Objectives").  "objective": "xendcg" is
// the listwise pass (section 11, "Listwise objective") under the key "xe_key" (u64, default 0; read under "xendcg" only); it
// keeps the NDCG norms, reads neither sigma nor the measure's depth, and refuses truncation_level != 0 and lambda_norm.
const void* fr_debug_lambda_gradients_opts(const CModel* model, const CDataset* dataset, const CQRel* qrel, const void* measure,
                                           double sigma, const uint32_t* queries, size_t n_queries, const void* options_json,
                                           double* lambda_out, double* weight_out, size_t out_len) {
    return lambda_gradients_debug(model, dataset, qrel, measure, sigma, queries, n_queries, false, &options_json, lambda_out, weight_out, out_len);
}

// the histogram grower's inputs for a view: its instance list and their positions, its features ascending
static void hist_debug_lists(fr::DatasetView& view, std::vector<uint32_t>* ids, std::vector<uint32_t>* positions, std::vector<uint32_t>* feats) {
    *ids = fr::lambdamart_instance_list(view.host_csr());
    *feats = view.features;
    std::sort(feats->begin(), feats->end());
    positions->resize(ids->size());
    std::string err;
    if (!view.device().rf_positions(*ids, positions->data(), &err)) fr::fail_str(err);
}

const void* fr_debug_hist_bins(const CDataset* dataset, uint32_t split_candidates, size_t n, size_t f, uint32_t* ids_out,
                               uint32_t* feats_out, float* edges_out, uint32_t* nedges_out, uint8_t* bins_out) {
    return status_call([&]() {
        const CDataset& ds = require_dataset(dataset);
        if (!ids_out || !feats_out || !edges_out || !nedges_out || !bins_out) fr::fail_str("NULL pointer: bin outputs");
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        std::vector<uint32_t> ids, positions, feats, nedges;
        hist_debug_lists(view, &ids, &positions, &feats);
        if (ids.size() != n || feats.size() != f) fr::fail_str("fr_debug_hist_bins: the view has " + std::to_string(ids.size()) + " instances and " + std::to_string(feats.size()) + " features");
        frdev::DeviceDataset& dev = view.device();
        std::string err;
        std::vector<float> edges;
        if (!dev.hist_bins(positions.data(), n, feats, split_candidates, nullptr, &err)) fr::fail_str(err);
        if (!dev.hist_edges(&edges, &nedges, &err)) fr::fail_str(err);
        if (!dev.hist_download_bins(bins_out, n * f, &err)) fr::fail_str(err);
        std::copy(ids.begin(), ids.end(), ids_out);
        std::copy(feats.begin(), feats.end(), feats_out);
        std::copy(edges.begin(), edges.end(), edges_out);
        std::copy(nedges.begin(), nedges.end(), nedges_out);
    });
}

// What the tree hook and the selection hook below share: the view's lists, a query sample (queries == NULL: every query) as
// flags with its instance count, and values by instance id gathered into instance-list order.
struct HistDebugInput {
    const frdev::HostCSR& csr;
    std::vector<uint32_t> ids, positions, feats;
    const bool sampled;
    std::vector<unsigned char> flags;  // [nq] when sampled
    size_t n_t;                        // the sample's instances
    HistDebugInput(fr::DatasetView& view, const uint32_t* queries, size_t n_queries) : csr(view.host_csr()), sampled(queries != nullptr) {
        hist_debug_lists(view, &ids, &positions, &feats);
        n_t = ids.size();
        if (!sampled) return;
        flags = debug_query_flags(queries, n_queries, csr.nq);
        n_t = 0;
        for (size_t q = 0; q < csr.nq; q++)
            if (flags[q]) n_t += csr.qoff[q + 1] - csr.qoff[q];
    }
    const unsigned char* query_flags() const { return sampled ? flags.data() : nullptr; }
    // The caller's values go to the device as they are, also outside the query sample: the grower must not read those.  An
    // id past len is refused (too_short) inside the sample only; so is, when not_finite is given, a value that is not finite.
    std::vector<double> gather(const double* values, size_t len, const std::string& too_short, const char* not_finite = nullptr) const {
        std::vector<double> out(ids.size(), 0.0);
        size_t g = 0;
        for (size_t q = 0; q < csr.nq; q++) {
            const bool read = !sampled || flags[q];
            for (size_t j = csr.qoff[q]; j < csr.qoff[q + 1]; j++, g++) {
                if (ids[g] >= len) {
                    if (!read) continue;
                    fr::fail_str(too_short);
                }
                out[g] = values[ids[g]];
                if (not_finite && read && !std::isfinite(out[g])) fr::fail_str(not_finite);
            }
        }
        return out;
    }
};
// (the bins stay with the view: leave them without a sample, also when the hook fails)
struct HistDebugUnsample {
    fr::HistGrower& g;
    ~HistDebugUnsample() {
        try {
            g.set_sample(nullptr, 0, nullptr);
        } catch (...) {
        }
    }
};

// the two GOSS rates as a debug hook takes them: the request parser's ranges, and top_rate > 0
static bool goss_debug_rates_ok(double top_rate, double other_rate) {
    return std::isfinite(top_rate) && top_rate > 0.0 && top_rate < 1.0 && std::isfinite(other_rate) && other_rate > 0.0 && other_rate <= 1.0 &&
           top_rate + other_rate <= 1.0;
}
static const char* const GOSS_DEBUG_RATES = "top_rate must lie in (0, 1), other_rate in (0, 1], and their sum must be at most 1";

// what is wrong with the tree hook's options (nullptr: nothing): every rule that can be held without the dataset
static const char* hist_tree_options_error(const FrHistTreeOptions& o) {
    if (o.max_depth < 1) return "max_depth must be at least 1";
    if (o.max_leaves == 1) return "max_leaves must be 0 (level-wise) or at least 2";
    for (double x : {o.lambda_l2, o.min_sum_hessian, o.min_split_gain})
        if (!(std::isfinite(x) && x >= 0.0) || (!o.newton && x != 0.0))
            return "lambda_l2, min_sum_hessian and min_split_gain must be finite and at least 0, and 0 without the Newton gain";
    if (o.goss && !goss_debug_rates_ok(o.top_rate, o.other_rate)) return GOSS_DEBUG_RATES;
    if ((o.n_mono != 0 || o.goss) && !o.newton) return "monotone constraints and GOSS need the Newton gain";
    if (o.symmetric && (o.max_leaves != 0 || o.n_mono != 0 || o.goss))
        return "symmetric trees are grown level-wise (max_leaves = 0), without monotone constraints or GOSS";
    for (double x : {o.lambda_l1, o.max_delta_step, o.path_smooth})
        if (!(std::isfinite(x) && x >= 0.0) || (!o.newton && x != 0.0))
            return "lambda_l1, max_delta_step and path_smooth must be finite and at least 0, and 0 without the Newton gain";
    if (o.symmetric && o.path_smooth != 0.0) return "symmetric trees take no path_smooth";
    if (!fr::quant_bits_ok(o.quant_bits)) return "quant_bits must be 0 (off) or between 2 and 8";
    if (o.quant_bits != 0 && (!o.newton || o.n_mono != 0 || o.lambda_l1 != 0.0 || o.max_delta_step != 0.0 || o.path_smooth != 0.0))
        return "quantised gradients need the Newton gain, and take no monotone constraints, lambda_l1, max_delta_step or path_smooth";
    return nullptr;
}

// One tree of the histogram grower for lambda / weight by instance id, under the options
// include/fastrank.h describes; *clamped_leaves_out (may be NULL): the leaves a monotone bound moved.
const CResult* fr_debug_hist_tree(const CDataset* dataset, const FrHistTreeOptions* opt, const double* lambda, const double* weight, size_t len,
                                  uint32_t* clamped_leaves_out) {
    return c_call<CModel>([&]() {
        const std::string who = "fr_debug_hist_tree";
        if (!opt) fr::fail_str("NULL pointer: tree options");
        const FrHistTreeOptions& o = *opt;
        if (const char* wrong = hist_tree_options_error(o)) fr::fail_str(who + ": " + wrong);
        if (clamped_leaves_out) *clamped_leaves_out = 0;
        const CDataset& ds = require_dataset(dataset);
        if (!lambda || !weight) fr::fail_str("NULL pointer: gradient inputs");
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        const HistDebugInput in(view, o.queries, o.n_queries);
        const std::vector<uint32_t>& feats = in.feats;
        fr::HistGrowOptions grow{o.split_candidates, o.max_depth, o.min_leaf_support, fr::HistNewton(), o.max_leaves, {}, o.symmetric != 0};
        if (o.newton) grow.newton = {true, o.lambda_l2, o.min_sum_hessian, o.min_split_gain};
        grow.reg = {o.lambda_l1, o.max_delta_step, o.path_smooth};
        grow.quant_bits = o.quant_bits;
        std::vector<uint32_t> sel;
        if (o.features) {
            std::vector<uint32_t> want(o.features, o.features + o.n_features);
            std::sort(want.begin(), want.end());
            for (size_t i = 0; i < want.size(); i++) {
                const auto it = std::lower_bound(feats.begin(), feats.end(), want[i]);
                if (it == feats.end() || *it != want[i] || (i > 0 && want[i] == want[i - 1]))
                    fr::fail_str(who + ": feature " + std::to_string(want[i]) + " is not in the view, or is named twice");
                sel.push_back((uint32_t)(it - feats.begin()));
            }
        }
        if (o.n_mono != 0) {
            if (!o.mono_features || !o.mono_signs) fr::fail_str("NULL pointer: monotone constraints");
            grow.monotone.assign(feats.size(), 0);
            for (size_t i = 0; i < o.n_mono; i++) {
                const auto it = std::lower_bound(feats.begin(), feats.end(), o.mono_features[i]);
                if (it == feats.end() || *it != o.mono_features[i]) fr::fail_str(who + ": feature " + std::to_string(o.mono_features[i]) + " is not in the view");
                if (o.mono_signs[i] < -1 || o.mono_signs[i] > 1) fr::fail_str(who + ": a monotone sign must be -1, 0 or 1");
                grow.monotone[(size_t)(it - feats.begin())] = (int)o.mono_signs[i];
            }
        }
        const std::string too_short = who + ": the gradient arrays are shorter than the largest " + (in.sampled ? "sampled " : "") + "instance id";
        const std::vector<double> lam = in.gather(lambda, len, too_short), wt = in.gather(weight, len, too_short);
        const fr::HistGoss goss{o.top_rate, o.other_rate, fr::GossKeys::of_tree(o.seed, o.tree)};
        fr::HistGrower grower(view.device(), feats, grow);
        grower.prepare(in.positions);
        HistDebugUnsample unsample{grower};
        grower.set_sample(in.query_flags(), (uint32_t)in.n_t, o.features ? &sel : nullptr);
        return new_model([&] {
            fr::Model tree;
            tree.kind = fr::Model::DecisionTree;
            fr::HistTreeReport rep;
            tree.tree = grower.grow(lam.data(), wt.data(), o.goss ? &goss : nullptr, &rep,
                                    o.quant_bits != 0 ? fr::QuantKeys::of_tree(o.quant_seed, o.quant_tree) : 0);
            if (clamped_leaves_out) *clamped_leaves_out = rep.clamped_leaves;
            return tree;
        });
    });
}

// lambdamart_reg.hpp's output and term of one integer pair, without a device
const void* fr_debug_hist_reg_term(int64_t q, int64_t w, uint32_t n, int32_t s_l, int32_t s_w, double lambda_l1, double lambda_l2,
                                   double max_delta_step, double path_smooth, int32_t has_parent, double parent, double lo, double hi, double* v_out,
                                   double* term_out) {
    return status_call([&]() {
        if (!v_out || !term_out) fr::fail_str("NULL pointer: fr_debug_hist_reg_term");
        const fr::HistReg reg{lambda_l1, max_delta_step, path_smooth};
        const fr::RegSide s = fr::reg_side((long long)q, (long long)w, n, s_l, s_w, lambda_l2, reg, has_parent ? &parent : nullptr, lo, hi);
        *v_out = s.v, *term_out = s.term;
    });
}

// The GOSS selection on its own: lambda[len] by instance id; queries[n_queries] (NULL: all) = the tree's query sample, whose
// instances are the list L.  list_out / top_out[cap] (cap >= the view's instances): the GOSS list as indices into the view's
// full instance list, ascending, and per entry whether it is in the top set; *n_g_out: its length; *tau_out: the n_top-th
// largest key.
const void* fr_debug_goss_select(const CDataset* dataset, const double* lambda, size_t len, double top_rate, double other_rate, uint64_t seed,
                                 uint32_t tree, const uint32_t* queries, size_t n_queries, uint32_t* list_out, uint8_t* top_out, size_t cap,
                                 uint32_t* n_g_out, uint64_t* tau_out) {
    return status_call([&]() {
        const CDataset& ds = require_dataset(dataset);
        if (!lambda || !list_out || !top_out || !n_g_out || !tau_out) fr::fail_str("NULL pointer: fr_debug_goss_select");
        if (!goss_debug_rates_ok(top_rate, other_rate)) fr::fail_str(std::string("fr_debug_goss_select: ") + GOSS_DEBUG_RATES);
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        const HistDebugInput in(view, queries, n_queries);
        if (cap < in.ids.size()) fr::fail_str("fr_debug_goss_select: the outputs are shorter than the instance list");
        const std::vector<double> lam = in.gather(lambda, len, "fr_debug_goss_select: the gradient array is shorter than the largest instance id",
                                                  "fr_debug_goss_select: a gradient is not finite");
        frdev::DeviceDataset& dev = view.device();
        // (the selection reads no bin: the smallest bin matrix there is keeps the hook cheap on a view that has none yet)
        fr::HistGrower grower(dev, in.feats, {2u, 1u, 1u, fr::HistNewton{true, 0.0, 0.0, 0.0}, 0u, {}});
        grower.prepare(in.positions);
        HistDebugUnsample unsample{grower};
        grower.set_sample(in.query_flags(), (uint32_t)in.n_t, nullptr);
        const fr::GossPlan plan = fr::goss_plan(in.n_t, top_rate, other_rate);
        std::string err;
        uint32_t n_g = 0;
        if (!dev.hist_goss(lam.data(), plan.n_top, plan.p, plan.amp, fr::GossKeys::of_tree(seed, tree), &n_g, tau_out, &err)) fr::fail_str(err);
        if (!dev.hist_goss_download(list_out, top_out, n_g, &err)) fr::fail_str(err);
        *n_g_out = n_g;
    });
}

// One batch of random-forest trees grown by the trainer's own grow_batch with every level recorded (include/fastrank.h;
// DESIGN.md section 5.6).  out == NULL: grow, keep the record, return its JSON header; else hand the kept record's bytes over.
static std::mutex g_rf_levels_mu;
static std::vector<unsigned char> g_rf_levels_blob;
const void* fr_debug_rf_levels(const CDataset* dataset, const uint32_t* root_off, size_t n_trees, const uint32_t* root_ids, const uint32_t* feats,
                               uint32_t nf, uint32_t split_candidates, int32_t split_method, uint32_t min_leaf_support, uint32_t max_depth, void* out,
                               size_t out_bytes) {
    return json_call([&]() {
        const std::string who = "fr_debug_rf_levels";
        if (out) {
            std::lock_guard<std::mutex> lk(g_rf_levels_mu);
            if (out_bytes != g_rf_levels_blob.size())
                fr::fail_str(who + ": the record holds " + std::to_string(g_rf_levels_blob.size()) + " bytes, the buffer " + std::to_string(out_bytes));
            if (out_bytes) std::memcpy(out, g_rf_levels_blob.data(), out_bytes);
            std::vector<unsigned char>().swap(g_rf_levels_blob);
            return frjson::dump(Value::object());
        }
        const CDataset& ds = require_dataset(dataset);
        if (!root_off || !root_ids || !feats) fr::fail_str("NULL pointer: " + who);
        if (n_trees == 0 || nf == 0 || split_method < 0 || split_method > 3) fr::fail_str(who + ": at least one tree and one feature, split_method 0..3");
        for (size_t t = 0; t < n_trees; t++)
            if (root_off[t + 1] < root_off[t]) fr::fail_str(who + ": root_off must not decrease");
        if (root_off[0] != 0) fr::fail_str(who + ": root_off must start at 0");
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        const std::vector<uint32_t> off(root_off, root_off + n_trees + 1), ids(root_ids, root_ids + root_off[n_trees]), fl(feats, feats + n_trees * nf);
        for (uint32_t f : fl)
            if (std::find(ds.view->features.begin(), ds.view->features.end(), f) == ds.view->features.end())
                fr::fail_str(who + ": feature " + std::to_string(f) + " is not in the view");
        {
            std::vector<char> in_view(ds.view->core->n, 0);
            for (uint32_t id : ds.view->instances)
                if (id < in_view.size()) in_view[id] = 1;
            for (uint32_t id : ids)
                if (id >= in_view.size() || !in_view[id]) fr::fail_str(who + ": instance " + std::to_string(id) + " is not in the view");
        }
        fr::RFParams p;
        p.quiet = true;
        p.num_trees = (uint32_t)n_trees;
        p.split_method = split_method;
        p.min_leaf_support = min_leaf_support;
        p.split_candidates = split_candidates;
        p.max_depth = max_depth;
        fr::RFTrainer trainer(ds.view, fr::Evaluator(), p);
        fr::RFRecorder rec;
        const fr::Model forest = trainer.grow_recorded(off, ids, nf, fl, rec);
        std::vector<unsigned char> blob;
        Value sections = Value::array();
        auto put = [&](size_t level, const char* name, const void* data, size_t bytes) {
            Value s = Value::object();
            s.set("level", Value::uint(level));
            s.set("name", Value::string(name));
            s.set("offset", Value::uint(blob.size()));
            s.set("bytes", Value::uint(bytes));
            sections.push(s);
            const unsigned char* b = static_cast<const unsigned char*>(data);
            if (bytes) blob.insert(blob.end(), b, b + bytes);
        };
        Value levels = Value::array();
        for (size_t i = 0; i < rec.levels.size(); i++) {
            const fr::RFLevelRecord& lv = rec.levels[i];
            Value l = Value::object();
            l.set("A", Value::uint(lv.active.size()));
            l.set("items", Value::uint(lv.svals.size()));
            l.set("children_from", Value::string(lv.children_from_cands ? "candidates" : "rf_childsum_kernel"));
            levels.push(l);
            put(i, "active", lv.active.data(), lv.active.size() * sizeof(lv.active[0]));
            put(i, "depth", lv.depth.data(), lv.depth.size() * 4);
            put(i, "label_minmax", lv.label_minmax.data(), lv.label_minmax.size() * 4);
            put(i, "cands", lv.cands.data(), lv.cands.size() * sizeof(lv.cands[0]));
            put(i, "svals", lv.svals.data(), lv.svals.size() * 4);
            put(i, "sv", lv.sv.data(), lv.sv.size() * 4);
            put(i, "sg", lv.sg.data(), lv.sg.size() * 4);
            put(i, "splits", lv.splits.data(), lv.splits.size() * sizeof(lv.splits[0]));
            put(i, "child_out", lv.child_out.data(), lv.child_out.size() * 8);
        }
        put(rec.levels.size(), "root_out", rec.root_out.data(), rec.root_out.size() * 8);
        Value o = Value::object();
        o.set("cand_bytes", Value::uint(sizeof(frdev::DeviceDataset::RfCand)));
        o.set("levels", levels);
        o.set("sections", sections);
        o.set("bytes", Value::uint(blob.size()));
        Value trees = Value::array();
        for (const fr::Model& m : forest.members) trees.push(fr::model_to_json(m));
        o.set("trees", trees);
        {
            std::lock_guard<std::mutex> blk(g_rf_levels_mu);
            g_rf_levels_blob.swap(blob);
        }
        return frjson::dump(o);
    });
}

// The fixed-point step and the quantised gradients of one tree on their own ("Quantised gradients").
const void* fr_debug_hist_quantise(const CDataset* dataset, const double* lambda, const double* weight, size_t len, uint32_t bits, uint64_t seed,
                                   uint32_t tree, const uint32_t* queries, size_t n_queries, int32_t goss, double top_rate, double other_rate,
                                   uint64_t goss_seed, uint32_t goss_tree, int32_t* q_out, uint32_t* w_out, size_t cap, uint32_t* n_out,
                                   int32_t* numbers_out) {
    return status_call([&]() {
        const std::string who = "fr_debug_hist_quantise";
        const CDataset& ds = require_dataset(dataset);
        if (!lambda || !weight || !q_out || !w_out || !n_out || !numbers_out) fr::fail_str("NULL pointer: " + who);
        if (bits < fr::QUANT_MIN_BITS || bits > fr::QUANT_MAX_BITS) fr::fail_str(who + ": bits must be between 2 and 8");
        if (goss && !goss_debug_rates_ok(top_rate, other_rate)) fr::fail_str(who + ": " + GOSS_DEBUG_RATES);
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        const HistDebugInput in(view, queries, n_queries);
        if (cap < in.ids.size()) fr::fail_str(who + ": the outputs are shorter than the instance list");
        const std::string too_short = who + ": the gradient arrays are shorter than the largest instance id";
        const std::vector<double> lam = in.gather(lambda, len, too_short), wt = in.gather(weight, len, too_short);
        frdev::DeviceDataset& dev = view.device();
        // (no bin is read: the smallest bin matrix there is keeps the hook cheap on a view that has none yet)
        fr::HistGrower grower(dev, in.feats, {2u, 1u, 1u, fr::HistNewton{true, 0.0, 0.0, 0.0}, 0u, {}});
        grower.prepare(in.positions);
        HistDebugUnsample unsample{grower};
        grower.set_sample(in.query_flags(), (uint32_t)in.n_t, nullptr);
        std::string err;
        uint32_t n = (uint32_t)in.n_t;
        if (goss) {
            const fr::GossPlan plan = fr::goss_plan(in.n_t, top_rate, other_rate);
            if (!dev.hist_goss(lam.data(), plan.n_top, plan.p, plan.amp, fr::GossKeys::of_tree(goss_seed, goss_tree), &n, nullptr, &err)) fr::fail_str(err);
        }
        int s_l = 0, s_w = 0, d = 0, d_w = 0;
        bool all_zero = false;
        if (!dev.hist_quantise(lam.data(), wt.data(), &s_l, &s_w, &all_zero, &err)) fr::fail_str(err);
        if (all_zero) fr::fail_str(who + ": every lambda is zero (the tree is one leaf, nothing is quantised)");
        if (!dev.hist_quantq(bits, fr::QuantKeys::of_tree(seed, tree), &d, &d_w, &err)) fr::fail_str(err);
        if (!dev.hist_quantq_download(q_out, w_out, n, &err)) fr::fail_str(err);
        *n_out = n;
        const int32_t numbers[6] = {s_l, s_w, s_l - d, s_w - d_w, d, d_w};
        std::copy(numbers, numbers + 6, numbers_out);
    });
}

// The root's histogram of one tree (count, sum Q, sum W as [features][k]) for lambda / weight by instance id: bits == 0 by the
// Newton build over Q / W, else by the packed build over the quantised values of tree `tree` of `seed`.
const void* fr_debug_hist_root_histogram(const CDataset* dataset, const double* lambda, const double* weight, size_t len, uint32_t split_candidates,
                                         uint32_t bits, uint64_t seed, uint32_t tree, const uint32_t* features, size_t n_features,
                                         uint32_t* count_out, int64_t* sum_out, int64_t* wsum_out, size_t cells) {
    return status_call([&]() {
        const std::string who = "fr_debug_hist_root_histogram";
        const CDataset& ds = require_dataset(dataset);
        if (!lambda || !weight || !count_out || !sum_out || !wsum_out) fr::fail_str("NULL pointer: " + who);
        if (!fr::quant_bits_ok(bits)) fr::fail_str(who + ": bits must be 0 or between 2 and 8");
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        const HistDebugInput in(view, nullptr, 0);
        const std::vector<uint32_t>& feats = in.feats;
        std::vector<uint32_t> sel;
        if (features) {
            std::vector<uint32_t> want(features, features + n_features);
            std::sort(want.begin(), want.end());
            for (size_t i = 0; i < want.size(); i++) {
                const auto it = std::lower_bound(feats.begin(), feats.end(), want[i]);
                if (it == feats.end() || *it != want[i] || (i > 0 && want[i] == want[i - 1]))
                    fr::fail_str(who + ": feature " + std::to_string(want[i]) + " is not in the view, or is named twice");
                sel.push_back((uint32_t)(it - feats.begin()));
            }
        }
        const size_t Ft = features ? sel.size() : feats.size();
        if (cells != Ft * (size_t)split_candidates) fr::fail_str(who + ": the outputs must hold features x split_candidates cells");
        const std::string too_short = who + ": the gradient arrays are shorter than the largest instance id";
        const std::vector<double> lam = in.gather(lambda, len, too_short), wt = in.gather(weight, len, too_short);
        frdev::DeviceDataset& dev = view.device();
        fr::HistGrower grower(dev, feats, {split_candidates, 1u, 1u, fr::HistNewton{true, 0.0, 0.0, 0.0}, 0u, {}});
        grower.prepare(in.positions);
        HistDebugUnsample unsample{grower};
        grower.set_sample(nullptr, (uint32_t)in.n_t, features ? &sel : nullptr);
        std::string err;
        int s_l = 0, s_w = 0, d = 0, d_w = 0;
        bool all_zero = false;
        if (!dev.hist_quantise(lam.data(), wt.data(), &s_l, &s_w, &all_zero, &err)) fr::fail_str(err);
        if (all_zero) fr::fail_str(who + ": every lambda is zero (no fixed-point values are made)");
        if (bits != 0 && !dev.hist_quantq(bits, fr::QuantKeys::of_tree(seed, tree), &d, &d_w, &err)) fr::fail_str(err);
        if (!dev.hist_root(true, &err)) fr::fail_str(err);
        static_assert(sizeof(long long) == sizeof(int64_t), "the histograms' sums are 64-bit");
        if (!dev.hist_root_download(count_out, reinterpret_cast<long long*>(sum_out), reinterpret_cast<long long*>(wsum_out), cells, &err)) fr::fail_str(err);
    });
}

const void* fr_evaluate_dense(const CModel* model, const CDataset* dataset, const CQRel* qrel,
                              const void* evaluator_name, double* out_values, size_t out_len,
                              const void** out_qids_json) {
    return status_call([&]() {
        const CModel& m = require_model(model);
        const CDataset& ds = require_dataset(dataset);
        std::string name = accept_str("evaluator_name", evaluator_name);
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        fr::Evaluator ev = fr::make_evaluator(view, name, qrel ? &qrel->actual : nullptr);
        frdev::DeviceDataset& dev = view.device();
        if (out_len < dev.nq()) fr::fail_str("fr_evaluate_dense: output buffer too small");
        fr::score_model(view, m.actual);
        std::string err;
        if (!dev.metric_from_scores(ev.measure, ev.depth, ev.norms.data(), 1, false, &err)) fr::fail_str(err);
        fr::check_flags(dev);
        if (!dev.download_per_query(1, out_values, &err)) fr::fail_str(err);
        if (out_qids_json) {
            Value a = Value::array();
            for (size_t q = 0; q < dev.nq(); q++) a.push(Value::string(view.core->qnames[view.csr_query[q]]));
            *out_qids_json = return_string(frjson::dump(a));
        }
    });
}

const void* fr_rank_order(const CModel* model, const CDataset* dataset, uint32_t* out_instance_ids, size_t n,
                          uint64_t* out_offsets, size_t nq_plus_1) {
    return status_call([&]() {
        const CModel& m = require_model(model);
        const CDataset& ds = require_dataset(dataset);
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        frdev::DeviceDataset& dev = view.device();
        if (n < dev.n() || nq_plus_1 < dev.nq() + 1) fr::fail_str("fr_rank_order: output buffers too small");
        fr::score_model(view, m.actual);
        std::string err;
        std::vector<double> norms(dev.nq(), 0.0);
        if (!dev.metric_from_scores(frdev::M_RR, -1, norms.data(), 1, true, &err)) fr::fail_str(err);
        fr::check_flags(dev);
        if (!dev.download_rank(out_instance_ids, &err)) fr::fail_str(err);
        const frdev::HostCSR& csr = view.host_csr();
        for (size_t q = 0; q <= csr.nq; q++) out_offsets[q] = csr.qoff[q];
    });
}

size_t fr_dataset_num_queries(const CDataset* dataset) {
    if (!dataset) return 0;
    // host_csr() validates the labels (a NaN label is an error): nothing may unwind through extern "C".
    // SIZE_MAX = "this dataset cannot be grouped"; the compute calls report the reason in their envelope.
    try {
        return dataset->view->host_csr().nq;
    } catch (...) {
        return SIZE_MAX;
    }
}

const void* fr_dataset_device_info(const CDataset* dataset) {
    return json_call([&]() {
        const CDataset& ds = require_dataset(dataset);
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        std::shared_ptr<frdev::DeviceDataset> devp = ds.view->device_ptr();
        frdev::DeviceDataset& dev = *devp;
        fr::DatasetView* owner = ds.view->matrix_owner(nullptr);
        const bool is_parents = owner != ds.view.get() && owner->device_ptr() == devp;  // a feature sample: the parent's object itself
        Value o = Value::object();
        o.set("hbm_bytes_owned", Value::uint(is_parents ? 0 : dev.hbm_bytes()));
        o.set("shares_parent_matrix", Value::boolean(is_parents || dev.shares_parent_matrix()));
        o.set("is_parent_device_dataset", Value::boolean(is_parents));
        o.set("queries", Value::uint(dev.nq()));
        o.set("instances", Value::uint(dev.n()));
        return frjson::dump(o);
    });
}

size_t fr_dataset_num_instances(const CDataset* dataset) {
    if (!dataset) return 0;
    return dataset->view->instances.size();
}

const void* fr_evaluate_candidates(const CDataset* dataset, const CQRel* qrel, const void* evaluator_name,
                                   size_t n_groups, const uint32_t* features, const double* base_weights,
                                   const uint32_t* n_cand, const double* candidates, double* out_means,
                                   double* out_per_query) {
    return status_call([&]() {
        const CDataset& ds = require_dataset(dataset);
        std::string name = accept_str("evaluator_name", evaluator_name);
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        fr::Evaluator ev = fr::make_evaluator(view, name, qrel ? &qrel->actual : nullptr);
        frdev::DeviceDataset& dev = view.device();
        dev.set_sums_only(false);
        const size_t d = dev.d();
        std::string err;
        for (size_t g = 0; g < n_groups; g++)
            if (n_cand[g] == 0 || n_cand[g] > 64 || features[g] >= d)
                fr::fail_str("fr_evaluate_candidates: malformed group");
        if (dev.linesearch_path(ev.measure, ev.depth) != frdev::DeviceDataset::LS_NONE) {
            std::vector<frdev::LineGroup> groups(n_groups);
            for (size_t g = 0; g < n_groups; g++) {
                groups[g].feature = features[g];
                groups[g].weights.assign(base_weights + g * d, base_weights + (g + 1) * d);
                groups[g].candidates.assign(candidates + g * 64, candidates + g * 64 + n_cand[g]);
            }
            std::vector<double> means;
            if (!dev.linesearch(ev.measure, ev.depth, ev.norms.data(), groups, &means, nullptr, &err)) fr::fail_str(err);
            fr::check_flags(dev);
            std::copy(means.begin(), means.end(), out_means);
            if (out_per_query) {
                std::vector<double> M;
                size_t ldm = 0;
                if (!dev.download_last_matrix(&M, &ldm, &err)) fr::fail_str(err);
                std::copy(M.begin(), M.end(), out_per_query);
            }
        } else {
            std::vector<double> w;
            std::vector<size_t> slot;
            for (size_t g = 0; g < n_groups; g++)
                for (uint32_t c = 0; c < n_cand[g]; c++) {
                    size_t off = w.size();
                    w.insert(w.end(), base_weights + g * d, base_weights + (g + 1) * d);
                    w[off + features[g]] = candidates[g * 64 + c];
                    slot.push_back(g * 64 + c);
                }
            std::vector<double> means, pq;
            fr::evaluate_means_generic(view.device(), ev, w, slot.size(), means, out_per_query ? &pq : nullptr);
            for (size_t g = 0; g < n_groups * 64; g++) out_means[g] = 0.0;
            for (size_t k = 0; k < slot.size(); k++) out_means[slot[k]] = means[k];
            if (out_per_query) {  // [nq][n_groups * 64] as the fused paths give it; slots no candidate fills hold 0
                const size_t ld = n_groups * 64, B = slot.size();
                std::fill(out_per_query, out_per_query + dev.nq() * ld, 0.0);
                for (size_t q = 0; q < dev.nq(); q++)
                    for (size_t k = 0; k < B; k++) out_per_query[q * ld + slot[k]] = pq[q * B + k];
            }
        }
    });
}

void fr_profile_enable(int on) { frdev::profile_enable(on != 0); }
void fr_profile_reset(void) { frdev::profile_reset(); }

double fr_debug_resident_bound(int which, double a, double b, double c) {
    switch (which) {
        case 0: return frdev::resident_err_refresh((uint32_t)a, b);
        case 1: return frdev::resident_err_update(a, b, c);
        case 2: return frdev::resident_eps_extra(a, b, c);
        default: return std::numeric_limits<double>::quiet_NaN();
    }
}

// one norm against n dcg values: how many quotients differ bitwise from the division (*first: one of them).  3 * 10^10 pairs
// in tests/test_verify_end_host.py: the loop is compiled a second time for hosts with FMA instructions, where
// verify_quotient's five FMAs are five instructions instead of five calls into libm
static inline __attribute__((always_inline)) size_t verify_end_row_body(const double* a, size_t n, double norm, size_t* first) {
    const double rn = frdev::verify_rnorm(norm, true);
    size_t bad = 0;
    for (size_t i = 0; i < n; i++) {
        const double got = rn == rn ? frdev::verify_quotient(a[i], norm, rn) : a[i] / norm, exp = a[i] / norm;
        uint64_t gb, eb;
        std::memcpy(&gb, &got, 8);
        std::memcpy(&eb, &exp, 8);
        if (gb != eb && bad++ == 0) *first = i;
    }
    return bad;
}
#if defined(__x86_64__)
__attribute__((target("avx2,fma"))) static size_t verify_end_row_fma(const double* a, size_t n, double norm, size_t* first) {
    return verify_end_row_body(a, n, norm, first);
}
#endif
static size_t verify_end_row(const double* a, size_t n, double norm, size_t* first) {
#if defined(__x86_64__)
    if (__builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma")) return verify_end_row_fma(a, n, norm, first);
#endif
    return verify_end_row_body(a, n, norm, first);
}

int fr_debug_verify_end(int which, size_t n, const double* a, const double* b, const double* c, const double* d, double* out) {
    if (which == 0) {
        for (size_t i = 0; i < n; i++) {
            const double rn = frdev::verify_rnorm(b[i], true);
            out[i] = rn == rn ? frdev::verify_quotient(a[i], b[i], rn) : a[i] / b[i];
        }
        return 0;
    }
    if (which == 1) {
        for (size_t i = 0; i < n; i++) out[i] = frdev::verify_gap_bound(a[i], b[i], c[i], d[i]);
        return 0;
    }
    if (which == 2) {
        for (size_t i = 0; i < n; i++) out[i] = std::fma(a[i], b[i], c[i]);
        return 0;
    }
    if (which == 3) {
        // every a[i] against every b[j], j < m = (size_t)c[0]: how many quotients differ from the division, and the first pair
        const size_t m = (size_t)c[0];
        const unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
        std::vector<size_t> bad(nt, 0), first(nt, (size_t)-1);
        std::vector<std::thread> pool;
        for (unsigned t = 0; t < nt; t++)
            pool.emplace_back([&, t]() {
                for (size_t j = t; j < m; j += nt) {
                    size_t f = (size_t)-1;
                    const size_t k = verify_end_row(a, n, b[j], &f);
                    if (k != 0 && bad[t] == 0) first[t] = j * n + f;
                    bad[t] += k;
                }
            });
        for (auto& th : pool) th.join();
        size_t total = 0, f = (size_t)-1;
        for (unsigned t = 0; t < nt; t++) total += bad[t], f = std::min(f, first[t]);
        out[0] = (double)total;
        out[1] = total ? a[f % n] : 0.0;
        out[2] = total ? b[f / n] : 0.0;
        return 0;
    }
    return -1;
}

const void* fr_profile_json(void) {
    return json_call([&]() {
        Value a = Value::array();
        for (const auto& s : frdev::profile_stats()) {
            Value o = Value::object();
            o.set("kernel", Value::string(s.name));
            o.set("launches", Value::uint(s.launches));
            o.set("total_ms", Value::number(s.total_ms));
            a.push(std::move(o));
        }
        return frjson::dump(a);
    });
}

int fr_synchronize(void) {
    std::string err;
    return frdev::device_synchronize(&err) ? 0 : 1;
}

}  // extern "C"
