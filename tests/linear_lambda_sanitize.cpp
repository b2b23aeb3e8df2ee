// csrc/linear_lambda.hpp run on its own under -fsanitize=address,undefined (tests/test_linear_lambda_host.py builds and runs
// this): the solver at n = 0, 1 and 17 and at a pivot that is not positive, the choice of the returned iteration at its edges,
// one parse, one refusal and the statistics' report.
#include "linear_lambda.hpp"

#include <cstdio>
#include <cstdlib>

using namespace fr;

#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                \
        }                                                                \
    } while (0)

int main() {
    double pivot = 0.0, one = 0.0;
    const double h = 3.0, g1 = 8.0;
    CHECK(newton_step(nullptr, nullptr, 0, 1.0, nullptr, &pivot) == -1);
    CHECK(newton_step(&h, &g1, 1, 1.0, &one, &pivot) == -1 && one == 2.0);
    CHECK(newton_step(&h, &g1, 1, -3.0, &one, &pivot) == 0 && pivot == 0.0);
    const size_t n = 17;  // A = B^T B + n I over small integers; delta = A^-1 (A e) comes back as e up to rounding
    std::vector<double> B(n * n), A(n * n, 0.0), g(n, 0.0), d(n, 0.0);
    for (size_t i = 0; i < n * n; i++) B[i] = (double)((int)((i * 7919u) % 7) - 3);
    for (size_t i = 0; i < n; i++)
        for (size_t j = 0; j < n; j++) {
            for (size_t k = 0; k < n; k++) A[i * n + j] += B[k * n + i] * B[k * n + j];
            if (i == j) A[i * n + j] += (double)n;
        }
    for (size_t i = 0; i < n; i++)
        for (size_t j = 0; j < n; j++) g[i] += A[i * n + j];
    CHECK(newton_step(A.data(), g.data(), n, 0.0, d.data(), &pivot) == -1);
    for (size_t i = 0; i < n; i++) CHECK(std::fabs(d[i] - 1.0) < 1e-12);
    d.assign(n, 7.0);
    A[5 * n + 5] = -1.0;  // a pivot that is not positive: reported at its column, delta untouched
    CHECK(newton_step(A.data(), g.data(), n, 0.0, d.data(), &pivot) == 5 && !(pivot > 0.0) && d[0] == 7.0);
    A[5 * n + 5] = std::nan("");
    CHECK(newton_step(A.data(), g.data(), n, 0.0, d.data(), &pivot) == 5);
    CHECK(newton_pivot_message("7", -0.5, 0.25).find("larger lambda_l2") != std::string::npos);
    CHECK(linear_lambda_best(0.5, {0.4, 0.5, 0.3}) == 1);       // none beats the all-zero model: w^1
    CHECK(linear_lambda_best(0.5, {0.4, 0.7, 0.7, 0.6}) == 2);  // the first of equal maxima
    CHECK(linear_lambda_best(0.0, {std::nan("")}) == 1);

    const char* text = "{\"num_iterations\":3,\"learning_rate\":0.5,\"lambda_l2\":0.0,\"sigma\":2.0,\"quiet\":true,\"objective\":\"map\"}";
    LinearLambdaRankStats st;
    st.request = LinearLambdaRankParams::from_json(frjson::parse(text));
    CHECK(frjson::dump(st.request.to_json()) == text && st.request.pass().objective == frdev::M_AP);
    bool refused = false;
    try {
        LinearLambdaRankParams::from_json(frjson::parse("{\"num_iterations\":3,\"init_model\":null}"));
    } catch (const FrError& e) {
        refused = e.debug.find("init_model is not supported") != std::string::npos;
    }
    CHECK(refused);
    st.train_measure = {0.25, 0.5};
    st.weights = {{0.0, 1.0}, {0.5, -1.0}};
    CHECK(frjson::dump(st.to_json()).find("\"weights\":[[0.0,1.0],[0.5,-1.0]]") != std::string::npos);
    std::printf("linear_lambda ok\n");
    return 0;
}
