// A program of its own over csrc/ca_restart.hpp alone (tests/test_ca_restart_host.py builds it with
// -fsanitize=address,undefined and runs it): one restart driven to convergence over a synthetic objective,
//   f(w) = - sum_j a_j |w_j - t_j|,   NaN where w[nan_f] lies in [nan_lo, nan_hi],
// made of + - * /, fabs and comparisons only, so that tests/ca_restart_model.py computes the same bits.  Every line search
// is printed; the test compares the print-out with the model's.  With the one argument `select` it prints ca_select's
// answers instead.
//   ca_restart_sanitize seed=.. d=.. fids=0,3,4 init_random=0|1 normalize=0|1 iters=.. step_base=.. step_scale=.. tolerance=..
//                       a=..,.. t=..,.. [nan_f=.. nan_lo=.. nan_hi=..]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "ca_restart.hpp"

static std::map<std::string, std::string> g_args;

static std::vector<double> list_of(const std::string& key) {
    std::vector<double> out;
    const std::string& s = g_args[key];
    for (size_t at = 0; at < s.size();) {
        size_t end = s.find(',', at);
        if (end == std::string::npos) end = s.size();
        out.push_back(strtod(s.substr(at, end - at).c_str(), nullptr));
        at = end + 1;
    }
    return out;
}
static double num(const std::string& key, double otherwise) { return g_args.count(key) ? strtod(g_args[key].c_str(), nullptr) : otherwise; }

static void print_list(const char* key, const std::vector<double>& v) {
    printf(" %s=", key);
    for (size_t i = 0; i < v.size(); i++) printf("%s%a", i ? "," : "", v[i]);
}

static int select_cases() {
    using fr::RestartResult;
    // equal scores: the last maximum (Iterator::max); an ensemble request over one restart is that restart's linear model
    std::vector<RestartResult> hist = {{0, 0.5, {1.0, 2.0}}, {1, 0.75, {3.0, -1.0}}, {2, 0.75, {0.5, 0.25}}, {3, 0.25, {9.0, 9.0}}};
    fr::Model m = fr::ca_select(hist, false);
    printf("best kind=%d", (int)m.kind);
    print_list("weights", m.weights);
    printf("\n");
    m = fr::ca_select({hist[1]}, true);
    printf("one kind=%d", (int)m.kind);
    print_list("weights", m.weights);
    printf("\n");
    hist.push_back({4, 0.125, {0.0, 0.0}});  // (an all-zero member stays as it is)
    m = fr::ca_select(hist, true);
    printf("ensemble kind=%d", (int)m.kind);
    print_list("weights", m.ens_weights);
    printf("\n");
    for (const fr::Model& mm : m.members) {
        printf("member kind=%d", (int)mm.kind);
        print_list("weights", mm.weights);
        printf("\n");
    }
    bool refused = false;
    try {
        fr::ca_select({}, false);
    } catch (const fr::FrError&) {
        refused = true;
    }
    printf("empty refused=%d\n", (int)refused);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && std::string(argv[1]) == "select") return select_cases();
    for (int i = 1; i < argc; i++) {
        const std::string kv = argv[i];
        const size_t eq = kv.find('=');
        if (eq == std::string::npos) return 2;
        g_args[kv.substr(0, eq)] = kv.substr(eq + 1);
    }
    fr::CAParams p;
    p.num_max_iterations = (uint32_t)num("iters", 25);
    p.step_base = num("step_base", 0.05);
    p.step_scale = num("step_scale", 2.0);
    p.tolerance = num("tolerance", 0.001);
    p.normalize = num("normalize", 1) != 0.0;
    p.init_random = num("init_random", 1) != 0.0;
    const size_t d = (size_t)num("d", 1);
    std::vector<uint32_t> fids;
    for (double f : list_of("fids")) fids.push_back((uint32_t)f);
    const std::vector<double> a = list_of("a"), t = list_of("t");
    const long nan_f = (long)num("nan_f", -1);
    const double nan_lo = num("nan_lo", 0.0), nan_hi = num("nan_hi", 0.0);
    if (a.size() != d || t.size() != d || fids.empty()) return 2;
    auto objective = [&](const std::vector<double>& w) {
        double s = 0.0;
        for (size_t j = 0; j < d; j++) {
            if ((long)j == nan_f && w[j] >= nan_lo && w[j] <= nan_hi) return std::nan("");
            s = s - a[j] * std::fabs(w[j] - t[j]);
        }
        return s;
    };

    fr::CARestart r(0, (uint64_t)num("seed", 1));
    r.init_weights(fids, d, p.init_random);
    r.best_score = objective(r.best_w);
    printf("init");
    print_list("best_w", r.best_w);
    printf("\n");
    unsigned long long evals = 1, passes = 0, searches = 0;
    std::vector<double> w;
    while (!r.done) {
        const fr::CARestart::Staged st = r.stage(fids, p);
        passes += st.new_pass;
        const fr::CARestart::Replayed rep = r.replay(p, [&](size_t c) {
            w = r.base;
            w[st.feature] = r.cands[c];
            return objective(w);
        });
        evals += rep.evaluated;
        printf("ls pass=%llu f=%u norm=%a", passes, st.feature, r.norm);
        print_list("cands", r.cands);
        printf(" evaluated=%zu accepted=", rep.evaluated);
        for (size_t i = 0; i < r.accepted.size(); i++) printf("%s%zu", i ? "," : "", r.accepted[i].cand);
        printf(" best_score=%a", r.best_score);
        print_list("best_w", r.best_w);
        printf(" evals=%llu\n", evals);
        if (rep.finished != r.done) return 3;
        for (const auto& acc : r.accepted)
            if (acc.score != acc.score || acc.score > r.best_score) return 3;  // (scores accepted rise to best_score)
        if (++searches >= 20000) {
            printf("no convergence\n");
            return 4;
        }
    }
    printf("done passes=%llu evals=%llu\n", passes, evals);
    return 0;
}
