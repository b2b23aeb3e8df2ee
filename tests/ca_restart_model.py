"""One restart of the reference's coordinate ascent (optimize_inner, src/coordinate_ascent.rs:87-195)
restated in Python over an arbitrary objective f(w), with a log of every line search in the form
tests/ca_restart_sanitize.cpp prints for csrc/ca_restart.hpp.  Written from the reference's lines, which the comments name.
The random draws are the oracle's generator's (oracle/pyoracle.py: Rand64)."""
import math

from oracle import pyoracle as o

SIGN = (0, -1, 1)  # :85


def c_hex(x):
    """x as C's printf("%a") writes a double."""
    if x != x:
        return "nan"
    if math.isinf(x):
        return "inf" if x > 0 else "-inf"
    sign, rest = ("-", float.hex(x)[1:]) if math.copysign(1.0, x) < 0 else ("", float.hex(x))
    mant, exp = rest.split("p")
    mant = mant.rstrip("0").rstrip(".") if "." in mant else mant
    return "%s%sp%s" % (sign, mant, exp)


def hex_list(v):
    return ",".join(c_hex(x) for x in v)


def shuffle(v, rand):
    """src/randutil.rs:21-27"""
    n = len(v)
    for i in range(n):
        j = rand.rand_range(i, n)
        v[i], v[j] = v[j], v[i]


def l1_normalize(w):
    """:72-82; returns what the weights were divided by (1.0: they were left as they are)"""
    total = 0.0
    for x in w:
        total += abs(x)
    if total > 0.0:
        for i in range(len(w)):
            w[i] /= total
        return total
    return 1.0


def optimize_inner(fids, width, seed, p, f, max_line_searches=20000):
    """p: dict of the reference's parameters (:11-23).  width: how many weights the log shows (the reference's model has
    max(fids) + 1, :97-103; the library keeps the dataset's width, the rest are zeros).  Returns (score, weights, log lines)."""
    rand = o.Rand64(seed)
    model_dim = max(fids) + 1
    model = [0.0] * model_dim  # :43-48
    if p["init_random"]:  # :50-58
        for i in fids:
            model[i] = rand.rand_float() * 2.0 - 1.0
    else:  # :60-70
        for i in fids:
            model[i] = 1.0 / float(len(fids))
    pad = [0.0] * (width - model_dim)
    best_score, best = f(model), list(model)  # :110-111
    assert best_score == best_score, "NaN found!"  # core.rs:50-55
    log = ["init best_w=%s" % hex_list(best + pad)]
    evals, passes, searches = 1, 0, 0
    while True:  # :113
        order = list(fids)
        shuffle(order, rand)  # :114-116
        passes += 1
        successes = 0
        for feature in order:  # :131-133
            start_score = best_score  # :134
            model = list(best)  # :135
            norm = l1_normalize(model) if p["normalize"] else 1.0  # :136-138
            orig = model[feature]  # :142
            cands, accepted, evaluated = [], [], 0
            go_on = True
            for d in SIGN:  # :145
                step = p["step_base"] * float(d)  # :146
                if orig != 0.0 and abs(step) > 0.5 * abs(orig):  # :147-149
                    step = p["step_base"] * abs(orig) * float(d)
                total_step = step  # :150
                num_iter = p["num_max_iterations"]  # :151
                if d == 0:  # :152-155
                    num_iter = 1
                    total_step = -orig
                for _ in range(num_iter):  # :157
                    w = orig + total_step  # :158
                    cands.append(w)  # (the library lists the candidates of all three directions before it scores any)
                    if go_on:
                        model[feature] = w  # :159
                        score = f(model)  # :160
                        evaluated += 1
                        if score == score and score > best_score:  # :162, core.rs:57-66: NaN never replaces, strict >
                            best_score, best = score, list(model)
                            accepted.append(len(cands) - 1)
                    step *= p["step_scale"]  # :169
                    total_step += step  # :170
                if best_score - start_score > p["tolerance"]:  # :174-176
                    go_on = False
            if best_score - start_score > p["tolerance"]:  # :179-181
                successes += 1
            evals += evaluated
            searches += 1
            log.append("ls pass=%d f=%d norm=%s cands=%s evaluated=%d accepted=%s best_score=%s best_w=%s evals=%d" % (
                passes, feature, c_hex(norm), hex_list(cands), evaluated, ",".join(str(i) for i in accepted), c_hex(best_score),
                hex_list(best + pad), evals))
            assert searches < max_line_searches, "no convergence"
        if successes == 0:  # :185-187
            break
    log.append("done passes=%d evals=%d" % (passes, evals))
    return best_score, best + pad, log
