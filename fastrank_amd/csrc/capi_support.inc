// capi.cpp's shared plumbing: the reference's string / result envelopes (src/ffi.rs), the handle checks, the per-dataset
// lock, and the few sequences more than one group of exports runs.
namespace {

// Device jobs are serialised per dataset (DataCore::api_mu: the views of one core share device forms and work buffers),
// not per process: two host threads that train on different datasets -- each on its own devices -- do not wait for
// each other.  (Round 2 had one process-wide lock.)
static std::mutex& api_mu_of(const CDataset& ds) { return ds.view->core->api_mu; }

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

// what `make` returns as a handle (CModel, CDataset, CQRel: each holds one thing) the caller owns; nothing is left behind
// when it throws
template <typename H, typename F>
H* new_handle(F&& make) {
    std::unique_ptr<H> out(new H());
    *out = H{make()};
    return out.release();
}
template <typename F>
CModel* new_model(F&& make) {
    return new_handle<CModel>(make);
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

// a view's feature ids, ascending (the order the tree trainers, the explanations and their hooks number columns in)
std::vector<uint32_t> features_ascending(const fr::DatasetView& v) {
    std::vector<uint32_t> feats = v.features;
    std::sort(feats.begin(), feats.end());
    return feats;
}

// The evaluator's measure of the first `slots` score slots, per query, with the flags the kernels raised checked.  What the
// caller reads next (the means, the per-query values) is its own business.
void evaluate_scores(frdev::DeviceDataset& dev, const fr::Evaluator& ev, size_t slots) {
    std::string err;
    if (!dev.metric_from_scores(ev.measure, ev.depth, ev.norms.data(), slots, false, &err)) fr::fail_str(err);
    fr::check_flags(dev);
}

// Ranks every query of the view by the model's scores (slot 0): the reciprocal-rank kernel over zero norms, asked to keep
// its ranking, which download_rank then hands out.
void rank_view(fr::DatasetView& view, const fr::Model& m) {
    frdev::DeviceDataset& dev = view.device();
    fr::score_model(view, m);
    std::string err;
    std::vector<double> norms(dev.nq(), 0.0);
    if (!dev.metric_from_scores(frdev::M_RR, -1, norms.data(), 1, true, &err)) fr::fail_str(err);
    fr::check_flags(dev);
}

// the locks of two dataset handles (one lock when they share a core, or when there is no second handle), taken together
struct DatasetLocks {
    std::unique_lock<std::mutex> a, b;
    DatasetLocks(const CDataset& ds, const CDataset* other) {
        std::mutex& ma = api_mu_of(ds);
        std::mutex* mb = other ? &api_mu_of(*other) : nullptr;
        if (mb && mb != &ma) {
            a = std::unique_lock<std::mutex>(ma, std::defer_lock), b = std::unique_lock<std::mutex>(*mb, std::defer_lock);
            std::lock(a, b);
        } else {
            a = std::unique_lock<std::mutex>(ma);
        }
    }
};

}  // namespace
