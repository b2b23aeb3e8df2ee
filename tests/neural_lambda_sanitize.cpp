// csrc/neural_lambda.hpp on its own under -fsanitize=address,undefined (tests/test_neural_lambda_host.py builds and runs this):
// parse and refusal, the initialiser (its net for seed 7 is printed for the test to restate), Adam, the choice, the report.
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

int main() {
    const char* text = "{\"hidden\":3,\"num_iterations\":4,\"learning_rate\":0.5,\"lambda_l2\":0.0,\"sigma\":2.0,\"seed\":7,\"quiet\":true,\"objective\":\"map\",\"trace\":true}";
    NeuralLambdaRankStats st;
    st.request = NeuralLambdaRankParams::from_json(frjson::parse(text));
    CHECK(frjson::dump(st.request.to_json()) == text && st.request.pass().objective == frdev::M_AP);
    bool refused = false;
    try {
        NeuralLambdaRankParams::from_json(frjson::parse("{\"hidden\":3,\"init_model\":null}"));
    } catch (const FrError& e) {
        refused = e.debug.find("init_model is not supported") != std::string::npos;
    }
    CHECK(refused);

    std::vector<unsigned char> flags;
    const std::vector<uint32_t> held = {1, 2, 4};
    Model net = neural_init(7, 3, 5, held, &flags);
    CHECK(flags.size() == 3 * 5 + 2 * 3 + 1 && flags[0] == 0 && flags[1] == (ADAM_UPDATED | ADAM_DECAYS) && flags[15] == ADAM_UPDATED);
    CHECK(net.nn_w1[0] == 0.0 && net.nn_w1[1] != 0.0 && std::fabs(net.nn_w1[1]) < 1.0 && net.nn_b2 == 0.0);
    const std::string wire = frjson::dump(model_to_json(net));
    std::printf("%s\n", wire.c_str());
    const Model back = model_from_json(frjson::parse(wire.c_str()));
    CHECK(back.nn_w1 == net.nn_w1 && back.nn_w2 == net.nn_w2 && back.nn_cols == 5);

    std::vector<double> theta = neural_flatten(net), grad(theta.size(), 0.5), m(theta.size(), 0.0), v(theta.size(), 0.0);
    const std::vector<double> before = theta;
    for (uint32_t t = 1; t <= 3; t++) adam_step(theta.data(), grad.data(), m.data(), v.data(), theta.size(), flags.data(), t, 0.1, 0.25);
    CHECK(theta[0] == before[0] && m[0] == 0.0);                 // a column the view does not hold: frozen
    CHECK(theta[1] != before[1] && theta[15] > before[15]);      // ascent along a positive gradient
    adam_step(nullptr, nullptr, nullptr, nullptr, 0, nullptr, 1, 0.1, 0.0);
    neural_unflatten(theta, &net);
    CHECK(net.nn_b1[0] == theta[15] && net.nn_b2 == theta.back());

    CHECK(neural_lambda_best(0.5, {0.4, 0.5, 0.3}) == 1);       // none beats the initial net: iterate 1
    CHECK(neural_lambda_best(0.5, {0.4, 0.7, 0.7, 0.6}) == 2);  // the first of equal maxima
    CHECK(neural_lambda_best(0.0, {std::nan("")}) == 1);
    st.train_measure = {0.25, 0.5};
    st.initial = model_to_json(net);
    st.iterates.push(model_to_json(net));
    const std::string rep = frjson::dump(st.to_json());
    CHECK(rep.find("\"train_measure\":[0.25,0.5]") != std::string::npos && rep.find("\"iterates\":[{\"NeuralNet\"") != std::string::npos);
    std::printf("neural_lambda ok\n");
    return 0;
}
