// A program of its own over csrc/resample_host.hpp (the options, the refusals, the fixed-shape sum, the reference's percentile
// and the report of DESIGN.md section 15), for -fsanitize=address,undefined: segment edges of the sum, the percentile at both
// ends and over one value, a report with either array missing, one trial, malformed options.
// tests/test_resample_host.py builds and runs it.
#include <cstdio>
#include <cstring>

#include "resample_host.hpp"

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                   \
        }                                                               \
    } while (0)

static bool options_refused(const char* text, const char* needle) {
    try {
        fr::resample_options_from_json(frjson::parse(text));
    } catch (const fr::FrError& e) {
        return e.debug.find(needle) != std::string::npos;
    } catch (const frjson::ParseError&) {
        return std::strcmp(needle, "parse") == 0;
    }
    return false;
}

static bool table_refused(const double* V, size_t Q, size_t M, const char* needle) {
    try {
        fr::resample_check(V, Q, M);
    } catch (const fr::FrError& e) {
        return e.debug.find(needle) != std::string::npos;
    }
    return false;
}

int main() {
    // the stream keys: splitmix64's first two outputs for seed 0 are mix(G) and mix(2 G)
    CHECK(frresample::boot_key(0) == 0xE220A8397B1DCDAFull && frresample::perm_key(0) == 0x6E789E6AA1B965F4ull);

    // the reference's two medians (src/stats.rs:193-198) and the interpolation as written
    std::vector<double> ten, nine;
    for (int i = 0; i < 10; i++) ten.push_back(i);
    for (int i = 0; i < 9; i++) nine.push_back(i);
    CHECK(fr::resample_percentile(ten, 0.5) == 4.5 && fr::resample_percentile(nine, 0.5) == 4.0);
    const std::vector<double> four = {0.0, 10.0, 20.0, 30.0};
    CHECK(fr::resample_percentile(four, 0.25) == 2.5 && fr::resample_percentile(four, 0.75) == 27.5);
    CHECK(fr::resample_percentile(four, 0.0) == 0.0 && fr::resample_percentile(four, 1.0) == 30.0);
    CHECK(fr::resample_percentile(std::vector<double>{3.0}, 0.95) == 3.0);
    std::vector<double> many;
    for (int i = 0; i < 200; i++) many.push_back(i);
    CHECK(fr::resample_interval(many, 0.05) == std::make_pair(4.0, 195.0));
    CHECK(fr::resample_interval(std::vector<double>{7.0}, 0.05) == std::make_pair(7.0, 7.0));
    CHECK(fr::resample_interval(many, 0.999999) == std::make_pair(99.0, 100.0));

    // SUM at the segment edges: 1e16 then ones.  Added one after the other every 1.0 is lost; a new segment keeps its ones
    for (size_t n : {size_t(1), size_t(2), size_t(255), size_t(256), size_t(257), size_t(258), size_t(513), size_t(600)}) {
        std::vector<double> x(2 * n, -1.0);  // (stride 2: the odd cells are never read)
        for (size_t i = 0; i < n; i++) x[2 * i] = i == 0 ? 1e16 : 1.0;
        const double in_later_segments = n > 256 ? (double)(n - 256) : 0.0;
        CHECK(fr::resample_sum(x.data(), n, 2) == 1e16 + in_later_segments);
    }
    CHECK(fr::resample_sum(nullptr, 0, 1) == 0.0);
    const double minus_zero[2] = {-0.0, -0.0};
    CHECK(!std::signbit(fr::resample_sum(minus_zero, 2, 1)));

    // a report: 3 queries, 2 systems, 4 trials
    const double V[6] = {1.0, 0.0, 0.5, 0.5, 0.25, 1.0};
    const double boot[8] = {0.5, 0.4, 0.7, 0.6, 0.6, 0.5, 0.4, 0.9};
    const double perm[8] = {0.5, 0.5, 0.75, 0.25, 0.6, 0.5, 1.0, 0.0};
    fr::Value rep = fr::resample_report(V, 3, 2, 4, 0.05, boot, perm);
    CHECK(rep.find("means")->arr[0].as_double() == (1.0 + 0.5 + 0.25) / 3.0 && rep.find("means")->arr[1].as_double() == 1.5 / 3.0);
    CHECK(rep.find("intervals")->arr[0].arr[0].as_double() == 0.4 && rep.find("intervals")->arr[0].arr[1].as_double() == 0.7);
    CHECK(rep.find("summary")->arr.size() == 2 && rep.find("summary")->arr[1].find("p50") != nullptr);
    const fr::Value& pair = rep.find("pairs")->arr[0];
    // |diff| = 1/12; the ranges are 0, 0.5, 0.6 - 0.5 and 1: all but the first reach it
    CHECK(pair.find("p")->as_double() == 4.0 / 5.0);
    CHECK(pair.find("wins")->u == 1 && pair.find("losses")->u == 1 && pair.find("ties")->u == 1);
    CHECK(pair.find("diff_interval")->arr[0].as_double() == -0.5);
    fr::Value no_perm = fr::resample_report(V, 3, 2, 4, 0.05, boot, nullptr);
    CHECK(no_perm.find("pairs")->arr[0].find("p") == nullptr && no_perm.find("intervals") != nullptr);
    fr::Value no_boot = fr::resample_report(V, 3, 2, 4, 0.05, nullptr, perm);
    CHECK(no_boot.find("intervals") == nullptr && no_boot.find("summary") == nullptr && no_boot.find("pairs")->arr[0].find("diff_interval") == nullptr);
    fr::Value one = fr::resample_report(V, 6, 1, 1, 0.5, boot, perm);  // one system, one trial: no pair, every percentile the one value
    CHECK(one.find("pairs")->arr.empty() && one.find("summary")->arr[0].find("p95")->as_double() == 0.5);
    CHECK(frjson::dump(rep).find("\"p\":0.8") != std::string::npos);

    // options
    fr::ResampleOptions op = fr::resample_options_from_json(frjson::parse("{}"));
    CHECK(op.trials == 10000 && op.seed == 0 && op.alpha == 0.05);
    op = fr::resample_options_from_json(frjson::parse("{\"seed\": 18446744073709551615, \"trials\": 1048576, \"alpha\": 0.5}"));
    CHECK(op.seed == 0xFFFFFFFFFFFFFFFFull && op.trials == (1u << 20) && op.alpha == 0.5);
    CHECK(options_refused("{\"trials\": 0}", "trials must be between 1 and 1048576, not 0"));
    CHECK(options_refused("{\"trials\": 1048577}", "not 1048577"));
    CHECK(options_refused("{\"trials\": -3}", "expected unsigned integer for trials"));
    CHECK(options_refused("{\"trials\": 2.5}", "expected unsigned integer for trials"));
    CHECK(options_refused("{\"seed\": \"x\"}", "expected unsigned integer for seed"));
    CHECK(options_refused("{\"alpha\": 0}", "alpha must lie strictly between 0 and 1"));
    CHECK(options_refused("{\"alpha\": 1}", "alpha must lie strictly between 0 and 1"));
    CHECK(options_refused("{\"alpha\": null}", "expected f64 for alpha"));
    CHECK(options_refused("{\"trails\": 5}", "unknown field `trails`"));
    CHECK(options_refused("[]", "expected a map"));
    CHECK(options_refused("{\"trials\": ", "parse"));

    // the table's refusals name the cell
    double bad[6] = {1.0, 0.0, 0.5, 0.5, 0.25, 1.0};
    fr::resample_check(bad, 3, 2);
    bad[5] = std::nan("");
    CHECK(table_refused(bad, 3, 2, "non-finite value in row 2, column 1"));
    bad[5] = 1.0, bad[2] = -INFINITY;
    CHECK(table_refused(bad, 3, 2, "non-finite value in row 1, column 0"));
    CHECK(table_refused(bad, 3, 0, "between 1 and 8 systems, not 0") && table_refused(bad, 3, 9, "not 9"));
    CHECK(table_refused(bad, 0, 2, "at least one query") && table_refused(nullptr, 3, 2, "NULL pointer"));
    std::printf("resample_host ok\n");
    return 0;
}
