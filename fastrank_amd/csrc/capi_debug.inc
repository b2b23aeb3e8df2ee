// capi.cpp: the test hooks (fr_debug_*, and the steppable trainer's tick capture) of the dataset, its layouts and device form,
// the device plan and the exchange, forest packing, the measures, the line search's bounds.  No product path calls one; the
// tree trainers' hooks are in capi_debug_trees.inc.  Nothing else belongs here.
extern "C" {

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

}  // extern "C"
