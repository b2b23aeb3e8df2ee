// csrc/neural_lambda.hpp's two-hidden-layer code on its own under -fsanitize=address,undefined (tests/test_neural_lambda2_host.py
// builds and runs this): the `hidden2` key, the initialiser (its net for seed 7 is printed for the test to restate), the
// numbering through flatten / unflatten, the model's two optional keys.
#include "neural_lambda.hpp"

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

static bool refused(const char* text, const char* words) {
    try {
        NeuralLambdaRankParams::from_json(frjson::parse(text));
    } catch (const FrError& e) {
        return e.debug.find(words) != std::string::npos;
    }
    return false;
}

int main() {
    const char* text = "{\"hidden\":3,\"num_iterations\":4,\"learning_rate\":0.5,\"lambda_l2\":0.0,\"sigma\":2.0,\"seed\":7,\"quiet\":true,\"hidden2\":2}";
    const NeuralLambdaRankParams p = NeuralLambdaRankParams::from_json(frjson::parse(text));
    CHECK(frjson::dump(p.to_json()) == text && p.hidden2 == 2);
    std::string zero(text), big(text);
    zero.replace(zero.find("\"hidden2\":2"), 11, "\"hidden2\":0"), big.replace(big.find("\"hidden2\":2"), 11, "\"hidden2\":65");
    CHECK(refused(zero.c_str(), "hidden2 must be between 1 and 64") && refused(big.c_str(), "hidden2 must be between 1 and 64"));

    std::vector<unsigned char> flags, flags1;
    const std::vector<uint32_t> held = {1, 2, 4};
    const size_t h = 3, d = 5, h2 = 2, n = h * d + h + h2 * h + 2 * h2 + 1;
    Model net = neural_init(7, h, d, held, &flags, h2);
    CHECK(net.nn_w1 == neural_init(7, h, d, held, &flags1).nn_w1 && flags1.size() == h * d + 2 * h + 1);  // the one-layer W1, bit for bit
    CHECK(flags.size() == n && net.nn_hw2.size() == h2 * h && net.nn_hb2.size() == h2 && net.nn_w2.size() == h2);
    for (size_t c = h * d; c < n; c++) {
        const bool bias = c < h * d + h || (c >= h * d + h + h2 * h && c < h * d + h + h2 * h + h2) || c + 1 == n;
        CHECK(flags[c] == (bias ? ADAM_UPDATED : (ADAM_UPDATED | ADAM_DECAYS)));
    }
    const std::string wire = frjson::dump(model_to_json(net));
    std::printf("%s\n", wire.c_str());
    const Model back = model_from_json(frjson::parse(wire.c_str()));
    CHECK(back.nn_w1 == net.nn_w1 && back.nn_hw2 == net.nn_hw2 && back.nn_hb2 == net.nn_hb2 && back.nn_w2 == net.nn_w2 && back.nn_hidden2() == h2);

    std::vector<double> theta = neural_flatten(net);
    CHECK(theta.size() == n && theta[h * d + h] == net.nn_hw2[0] && theta[n - 1 - h2] == net.nn_w2[0]);
    for (size_t c = 0; c < n; c++) theta[c] = (double)c;
    neural_unflatten(theta, &net);
    CHECK(net.nn_b1[0] == (double)(h * d) && net.nn_hw2[1] == (double)(h * d + h + 1) && net.nn_hb2[1] == (double)(h * d + h + h2 * h + 1));
    CHECK(net.nn_w2[0] == (double)(n - 1 - h2) && net.nn_b2 == (double)(n - 1) && neural_flatten(net) == theta);
    frdev::DeviceDataset::MlpPlan plan;
    CHECK(frjson::dump(mlp_plan_json(plan)).find("hidden2") == std::string::npos);
    plan.hidden2 = 2;
    CHECK(frjson::dump(mlp_plan_json(plan)).find("\"hidden2\":2") != std::string::npos);
    std::printf("neural_lambda2 ok\n");
    return 0;
}
