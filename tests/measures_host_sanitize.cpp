// csrc/measures_host.hpp under -fsanitize=address,undefined (tests/test_measures_host.py builds and runs this program): the
// name table and the cut-off rules, the norms, the five measures on designed lists (empty, one document, k beyond the list, a
// judged count above the list's own), the routing rule at its edges.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "measures_host.hpp"

namespace m = frmeasure;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            return 1;                                                        \
        }                                                                    \
    } while (0)

static std::vector<double> gexp_of(const std::vector<float>& g) {
    std::vector<double> e(g.size());
    for (size_t i = 0; i < g.size(); i++) e[i] = std::pow(2.0, (double)g[i]) - 1.0;
    return e;
}

int main() {
    m::Resolved r;
    std::string err;
    // names and cut-off rules
    CHECK(m::resolve("ndcg", 10, &r, &err) && r.measure == m::NDCG && r.display == "NDCG@10");
    CHECK(m::resolve("map", 5, &r, &err) && r.measure == m::AP && r.display == "AP");
    CHECK(m::resolve("rr", -1, &r, &err) && r.measure == m::RR && r.display == "RR");
    CHECK(m::resolve("dcg", -1, &r, &err) && r.measure == m::DCG && r.display == "DCG");
    CHECK(m::resolve("prec", 3, &r, &err) && r.measure == m::PRECISION && r.display == "Precision@3");
    CHECK(m::resolve("recall", 0, &r, &err) && r.measure == m::RECALL && r.display == "Recall@0");
    CHECK(m::resolve("success", 1, &r, &err) && r.measure == m::SUCCESS && r.display == "Success@1");
    CHECK(m::resolve("err", 20, &r, &err) && r.measure == m::ERR && r.display == "ERR@20");
    CHECK(!m::resolve("p", 5, &r, &err) && err.empty());
    CHECK(!m::resolve("", -1, &r, &err) && err.empty());
    CHECK(!m::resolve("precision", -1, &r, &err) && err.find("Precision needs a cut-off") != std::string::npos);
    CHECK(!m::resolve("success", 0, &r, &err) && err.find("Success needs a cut-off of at least 1") != std::string::npos);
    CHECK(m::find_measure("ERR") == nullptr && m::find_measure("err")->id == m::ERR);
    for (int i = 0; i < m::MEASURE_COUNT; i++) CHECK(m::measure_table()[i].id == i && m::is_cut_measure(i) == (i >= m::DCG));

    // norms
    const std::vector<float> none;
    CHECK(m::gmax_of(none.data(), 0) == 0.0f && m::gmax_of(none.data(), 0, 3.0f) == 3.0f);
    const std::vector<float> neg = {-2.0f, -1.0f, std::numeric_limits<float>::quiet_NaN()};
    CHECK(m::gmax_of(neg.data(), neg.size()) == 0.0f);
    double den = 0.0;
    CHECK(m::err_den(4.0f, &den, &err) && den == 16.0);
    CHECK(m::err_den(-3.0f, &den, &err) && den == 1.0);
    CHECK(!m::err_den(2000.0f, &den, &err) && err.find("no finite 2^gain") != std::string::npos);
    CHECK(!m::err_den(std::numeric_limits<float>::infinity(), &den, &err));
    CHECK(m::count_relevant(neg.begin(), neg.end()) == 0);

    // the measures: gains 2 0 1 0 0 3 ranked, den = 8
    const std::vector<float> g = {2.0f, 0.0f, 1.0f, 0.0f, 0.0f, 3.0f};
    const std::vector<double> e = gexp_of(g);
    CHECK(m::cut_len(6, -1) == 6 && m::cut_len(6, 0) == 0 && m::cut_len(6, 6) == 6 && m::cut_len(6, INT64_MAX / 2) == 6);
    CHECK(m::dcg_at(e.data(), 6, 1) == 3.0 && m::dcg_at(e.data(), 6, 3) == 3.0 + 0.0 / std::log2(3.0) + 1.0 / 2.0);
    CHECK(m::dcg_at(e.data(), 6, 0) == 0.0 && m::dcg_at(e.data(), 6, -1) == m::dcg_at(e.data(), 6, 100));
    CHECK(m::precision_at(g.data(), 6, 5, 5.0) == 0.4 && m::precision_at(g.data(), 6, 10, 10.0) == 0.3);
    CHECK(m::recall_at(g.data(), 6, 5, 3.0) == 2.0 / 3.0 && m::recall_at(g.data(), 6, 5, 0.0) == 2.0 / 3.0);
    CHECK(m::recall_at(g.data(), 6, -1, 7.0) == 3.0 / 7.0);  // a judged count above the list's own
    CHECK(m::success_at(g.data(), 6, 1) == 1.0 && m::success_at(g.data() + 1, 1, 4) == 0.0);
    // ERR@3: R = 3/8, 0, 1/8: e = 3/8 + (5/8 * 1/8) / 3
    CHECK(m::err_at(g.data(), e.data(), 6, 3, 8.0) == 0.375 + (0.625 * 0.125) / 3.0);
    CHECK(m::err_at(g.data(), e.data(), 6, 1, 8.0) == 0.375 && m::err_at(g.data(), e.data(), 0, -1, 8.0) == 0.0);
    // an empty list and a list without a relevant document
    CHECK(m::recall_at(none.data(), 0, -1, 0.0) == 0.0 && m::dcg_at(nullptr, 0, 5) == 0.0 && m::success_at(none.data(), 0, 3) == 0.0);
    const std::vector<float> z = {0.0f, -1.0f, 0.0f};
    CHECK(m::recall_at(z.data(), 3, 2, 0.0) == 0.0 && m::precision_at(z.data(), 3, 2, 2.0) == 0.0);
    CHECK(m::cut_measure_at(m::ERR, g.data(), e.data(), 6, 3, 8.0) == m::err_at(g.data(), e.data(), 6, 3, 8.0));
    CHECK(std::isnan(m::cut_measure_at(m::NDCG, g.data(), e.data(), 6, 3, 8.0)));

    // routing
    CHECK(!m::metric_topk_legal(m::NDCG, 10, false) && !m::metric_topk_legal(m::DCG, 0, false) && !m::metric_topk_legal(m::DCG, -1, false));
    CHECK(m::metric_topk_legal(m::DCG, 1, false) && m::metric_topk_legal(m::ERR, 64, false) && !m::metric_topk_legal(m::ERR, 65, false));
    CHECK(!m::metric_topk_legal(m::RECALL, 10, true));
    CHECK(!m::metric_topk_pays(0, 64) && !m::metric_topk_pays(65, 1u << 20) && !m::metric_topk_pays(-1, 64) && !m::metric_topk_pays(10, 0));
    for (uint32_t lg = 0; lg < 32; lg++)
        for (int64_t d : {(int64_t)1, (int64_t)10, (int64_t)64, INT64_MAX / 2}) (void)m::metric_topk_pays(d, 1u << lg);
    (void)m::metric_topk_pays(64, 0xFFFFFFFFu);
    std::printf("measures_host ok\n");
    return 0;
}
