// csrc/dataset_layout.hpp run on its own under -fsanitize=address,undefined (tests/test_device_form_host.py builds and runs
// this): three tiny layouts -- single-document queries, a query longer than a walk tile and than a run, and a view of every
// second query -- through every function of the header, with a few invariants checked on the way.
#include "dataset_layout.hpp"

#include <cstdio>
#include <cstdlib>

using namespace frdev;

#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                \
        }                                                                \
    } while (0)

struct Case {
    std::vector<float> x;
    HostCSR csr;
};

// queries of the given lengths, d = 3, gains descending inside a query, every fifth row a copy of the one before it
static void make_case(const std::vector<uint32_t>& qlens, Case* c) {
    HostCSR& csr = c->csr;
    csr.d = 3;
    csr.nq = qlens.size();
    csr.qoff.assign(1, 0);
    for (uint32_t n : qlens) csr.qoff.push_back(csr.qoff.back() + n);
    csr.n = csr.qoff.back();
    c->x.resize(csr.n * csr.d);
    for (size_t i = 0; i < csr.n; i++)
        for (size_t j = 0; j < csr.d; j++) c->x[i * csr.d + j] = (i % 5 == 4) ? c->x[(i - 1) * csr.d + j] : (float)((i * 7 + j * 3) % 11) - 5.0f;
    csr.x = c->x.data();
    for (size_t q = 0; q < csr.nq; q++)
        for (uint32_t k = 0; k < qlens[q]; k++) {
            csr.perm.push_back(csr.qoff[q] + k);
            csr.gain.push_back((float)(4 - (4 * k) / qlens[q]) - (k + 1 == qlens[q] ? 0.5f : 0.0f));
        }
}

static void run_case(const std::vector<uint32_t>& qlens, size_t nthreads) {
    Case c;
    make_case(qlens, &c);
    const HostCSR& csr = c.csr;
    RunPlan runs;
    std::string err;
    CHECK(plan_runs(csr.qoff, csr.nq, 768, &runs, &err));
    CHECK(runs.np % 64 == 0 && runs.run_order.size() == runs.run_q0.size() && runs.maxlen == *std::max_element(qlens.begin(), qlens.end()));
    const std::vector<uint32_t> perm = position_map(csr, runs.qstart, runs.qlen, runs.np);
    std::vector<uint32_t> qlist;
    const std::vector<SizeClass> sc = bucket_queries(runs.qlen, pow2_from_64, &qlist);
    size_t covered = 0;
    for (const SizeClass& s : sc) covered += s.count;
    CHECK(covered == csr.nq && qlist.size() == csr.nq);
    const GainTables gt = gain_tables(csr, runs.qstart, runs.qlen, perm, runs.maxlen);
    CHECK(gt.ncls == gt.cls_gain.size() && gt.dcgtab.size() == gt.ncls * DCG_RANKS && gt.termtab.size() == (gt.ncls + 1) * gt.tablen);
    CHECK(!gt.labels_small_int);
    const WalkTileLayout wl = build_walk_tiles(runs.run_pos, runs.run_q0, runs.run_q1, runs.qstart, runs.qlen, runs.np);
    CHECK(wl.wt_start.back() == runs.np && wl.seg.size() == runs.np);
    for (int pass = 0; pass < 2; pass++) {  // the host hash, then every row colliding
        const std::vector<uint64_t> hashes = pass ? std::vector<uint64_t>(runs.np, 0) : host_row_hash(csr, perm);
        const DupGroups dg = duplicate_groups(hashes, csr, perm, runs.qstart, runs.qlen, gt.gcls, gt.cls_gain.size(), false, nthreads);
        CHECK(dg.gkey16.size() == runs.np && dg.key_bits <= 16 && dg.key_cls_bits <= dg.key_bits);
        CHECK(csr.n < 5 || dg.dup_groups > 0);
    }
    if (csr.nq < 2) return;
    // a view of every second query, in the parent's position space
    HostCSR v;
    std::vector<uint32_t> pq;
    v.d = csr.d, v.x = csr.x;
    v.qoff.assign(1, 0);
    for (uint32_t q = 0; q < csr.nq; q += 2) {
        pq.push_back(q);
        v.perm.insert(v.perm.end(), csr.perm.begin() + csr.qoff[q], csr.perm.begin() + csr.qoff[q + 1]);
        v.gain.insert(v.gain.end(), csr.gain.begin() + csr.qoff[q], csr.gain.begin() + csr.qoff[q + 1]);
        v.qoff.push_back((uint32_t)v.perm.size());
    }
    v.nq = pq.size();
    v.n = v.perm.size();
    RunPlan vr;
    CHECK(plan_view_runs(runs.qstart, runs.qlen, perm, wl.wt_start, v, pq, 768, &vr, &err));
    CHECK(vr.np == runs.np && vr.run_lo.size() == vr.run_q0.size() && !vr.vtiles.empty() && !vr.wlist.empty());
    CHECK(vr.vtiles.back() < runs.np / 64 && vr.wlist.back() + 1 < wl.wt_start.size());
    std::swap(v.perm[0], v.perm[v.qoff[1] - 1]);  // (a no-op for a one-document query)
    const bool swapped = v.qoff[1] > 1;
    RunPlan bad;
    CHECK(plan_view_runs(runs.qstart, runs.qlen, perm, wl.wt_start, v, pq, 768, &bad, &err) == !swapped);
    CHECK(!swapped || err == "create_view: document order inside a query differs from the parent's");
}

int main() {
    run_case({1, 1, 1}, 1);
    run_case({800, 800, 1, 767, 1, 768, 769}, 1);                   // runs that close exactly at, and one past, the target
    run_case({5, 300, 2, 129, 64, 63, 1, 128, 127, 65, 900, 40}, 3);  // queries longer than a walk tile; three grouping threads
    std::printf("dataset_layout ok\n");
    return 0;
}
