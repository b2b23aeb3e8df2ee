"""csrc/ca_restart.hpp without a device: one restart's search (stage / replay) driven by tests/ca_restart_sanitize.cpp, a
program of its own built with the address and undefined-behaviour sanitizers, against tests/ca_restart_model.py, a
restatement of the reference's optimize_inner -- every line search bit for bit; and ca_select.

Which case reaches which branch: an objective that is NaN for some candidates -- nan_subset; orig == 0 -- zero_optimum and
zero_optimum_one_feature; an L1 norm of 0 -- zero_optimum_one_feature; a tolerance every gain exceeds -- tolerance_zero; one
that none exceeds, hence a pass with successes == 0 at the first try -- tolerance_huge; scores equal to the best so far --
no_normalize (a_1 = 0).  Mutations of the header tried on a copy, and the cases of the test below that fail under each:
  `>=` for `>`                          no_normalize, zero_optimum, zero_optimum_one_feature, one_feature, init_random,
                                        nan_subset, seventy_iterations, step_scale_one
  NaN accepted (`!(sc <= best_score)`)  nan_subset
  the break moved into the inner loop   init_random, init_uniform, nan_subset, no_normalize, one_feature, seventy_iterations,
                                        step_scale_one, zero_optimum
  successes not reset at a shuffle      every case of more than one pass (all but tolerance_huge): the restart never ends
  l1_normalize returning 0 for a norm   zero_optimum_one_feature, zero_optimum, one_feature, seventy_iterations
  of 0"""
import os
import shutil
import subprocess

import pytest

from tests import ca_restart_model as model

HERE = os.path.dirname(os.path.abspath(__file__))

# The objective is f(w) = - sum_j a_j |w_j - t_j| with dyadic a and t, NaN where w[nan_f] lies in [nan_lo, nan_hi]
# (tests/ca_restart_sanitize.cpp).  Parameters not named are the reference's defaults (coordinate_ascent.rs:25-41).
DEFAULTS = dict(seed=20250929, init_random=1, normalize=1, iters=25, step_base=0.05, step_scale=2.0, tolerance=0.001)
CASES = {
    "one_feature": dict(d=1, fids=[0], a=[1.0], t=[0.25]),
    "init_random": dict(d=5, fids=[0, 1, 2, 3, 4], a=[1.0, 0.5, 2.0, 0.25, 1.5], t=[0.5, -0.25, 0.125, 0.75, -0.5]),
    "init_uniform": dict(d=4, fids=[0, 1, 2, 3], init_random=0, a=[1.0, 0.5, 2.0, 0.25], t=[0.5, -0.25, 0.125, 0.75]),
    # a_1 = 0: every candidate of feature 1 scores exactly the best so far (strict > accepts none of them)
    "no_normalize": dict(d=3, fids=[0, 1, 2], normalize=0, a=[1.0, 0.0, 0.5], t=[0.5, 0.25, -0.75]),
    # the maximum is at w_1 = 0: the direction-0 candidate is accepted, and the next visit of feature 1 has orig == 0
    "zero_optimum": dict(d=3, fids=[0, 1, 2], a=[1.0, 4.0, 0.5], t=[0.5, 0.0, -0.25]),
    # ... with one feature the weights are then all zero: the L1 norm is 0, the divisor 1
    "zero_optimum_one_feature": dict(d=1, fids=[0], a=[2.0], t=[0.0]),
    # NaN wherever w_1 comes within 1/8 of its optimum: the candidates that would have been the best are among them
    "nan_subset": dict(d=3, fids=[0, 1, 2], normalize=0, a=[1.0, 2.0, 0.5], t=[0.5, -0.25, 0.125], nan_f=1, nan_lo=-0.375, nan_hi=-0.125),
    "tolerance_zero": dict(d=3, fids=[0, 1, 2], tolerance=0.0, a=[1.0, 2.0, 0.5], t=[0.5, -0.25, 0.125]),
    # no gain exceeds it: no direction is skipped, and the first pass is the last
    "tolerance_huge": dict(d=3, fids=[0, 1, 2], tolerance=1048576.0, a=[1.0, 2.0, 0.5], t=[0.5, -0.25, 0.125]),
    "one_iteration": dict(d=3, fids=[0, 1, 2], iters=1, a=[1.0, 2.0, 0.5], t=[0.5, -0.25, 0.125]),
    # 141 candidates: more than two of the trainer's groups of 64
    # (steps that do not grow, and an optimum far up: the candidates accepted reach into the third group)
    "seventy_iterations": dict(d=2, fids=[0, 1], iters=70, step_scale=1.0, a=[1.0, 2.0], t=[3.25, -0.25]),
    "step_scale_one": dict(d=3, fids=[0, 1, 2], step_scale=1.0, a=[1.0, 2.0, 0.5], t=[0.5, -0.25, 0.125]),
    # feature ids with a gap: the entries no feature names stay 0 (they would cost a_j |0 - t_j| either way)
    "fid_gap": dict(d=6, fids=[0, 3, 4], a=[1.0, 8.0, 8.0, 0.5, 2.0, 8.0], t=[0.5, 1.0, -1.0, -0.25, 0.125, 2.0]),
}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """tests/ca_restart_sanitize.cpp over csrc/ca_restart.hpp alone, built with the sanitizers and run directly"""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("ca_restart") / "ca_restart_sanitize")
    build = subprocess.run([cxx, "-std=c++17", "-O0", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(HERE, "..", "fastrank_amd", "csrc"), os.path.join(HERE, "ca_restart_sanitize.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    return exe


def _run(exe, args):
    run = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout[-4000:]
    return run.stdout.splitlines()


def _objective(c):
    a, t, nan_f, lo, hi = c["a"], c["t"], c.get("nan_f", -1), c.get("nan_lo", 0.0), c.get("nan_hi", 0.0)

    def f(w):
        s = 0.0
        for j in range(len(w)):  # (weights beyond the model's own are zeros on both sides)
            if j == nan_f and lo <= w[j] <= hi:
                return float("nan")
            s = s - a[j] * abs(w[j] - t[j])
        for j in range(len(w), len(a)):
            s = s - a[j] * abs(0.0 - t[j])
        return s
    return f


def _fields(line):
    return dict(kv.split("=", 1) for kv in line.split()[1:])


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_line_search_of_a_restart_is_the_models(program, name):
    c = dict(DEFAULTS, **CASES[name])
    args = ["%s=%s" % (k, ",".join(repr(x) for x in v) if isinstance(v, list) else repr(v)) for k, v in c.items()]
    got = _run(program, args)
    p = dict(init_random=bool(c["init_random"]), normalize=bool(c["normalize"]), num_max_iterations=c["iters"],
             step_base=c["step_base"], step_scale=c["step_scale"], tolerance=c["tolerance"])
    nans = []
    f = _objective(c)

    def counted(w):
        s = f(w)
        nans.extend([1] * (s != s))
        return s
    score, weights, want = model.optimize_inner(c["fids"], c["d"], c["seed"], p, counted)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (name, k)
    assert len(got) == len(want)
    searches = [_fields(line) for line in want if line.startswith("ls ")]
    ncand = 1 + 2 * c["iters"]
    assert all(len(s["cands"].split(",")) == ncand for s in searches)
    assert all(weights[j] == 0.0 for j in range(c["d"]) if j not in c["fids"])
    # what the case is there for happens in it
    done = _fields(want[-1])
    accepted = [[int(i) for i in s["accepted"].split(",") if i] for s in searches]
    if name == "zero_optimum":
        hit = [k for k, s in enumerate(searches) if s["f"] == "1" and 0 in accepted[k]]
        assert hit and any(s["f"] == "1" and s["cands"].split(",")[0:2] == ["0x0p+0", model.c_hex(-0.05)] for s in searches[hit[0] + 1:])
    if name == "zero_optimum_one_feature":
        assert any(s["norm"] == "0x1p+0" and s["best_w"] in ("0x0p+0", "-0x0p+0") and s["cands"].startswith("0x0p+0,") for s in searches[1:])
    if name == "nan_subset":
        assert nans and not (-0.375 <= weights[1] <= -0.125) and score == score  # (candidates scored NaN, and were passed over)
    else:
        assert not nans
    if name == "tolerance_huge":
        assert done["passes"] == "1" and all(int(s["evaluated"]) == ncand for s in searches) and any(accepted)
    if name == "tolerance_zero":
        assert int(done["passes"]) > 1 and not any(accepted[-len(c["fids"]):])
    if name == "no_normalize":
        assert all(s["norm"] == "0x1p+0" for s in searches) and not any(a for a, s in zip(accepted, searches) if s["f"] == "1")
    if name in ("one_iteration", "seventy_iterations"):
        assert int(done["passes"]) > 1
    if name == "seventy_iterations":
        assert ncand == 141 and any(i >= 128 for a in accepted for i in a)  # an accepted candidate of the third group of 64


def test_ca_select(program):
    """The last maximum on equal scores (Iterator::max, coordinate_ascent.rs:244-251); an ensemble request over a single
    restart is that restart's linear model (:232); ensemble members are L1-normalised, weighted by their scores (:232-242)."""
    LINEAR, ENSEMBLE = 1, 3
    h = model.hex_list
    got = _run(program, ["select"])
    assert got[0] == "best kind=%d weights=%s" % (LINEAR, h([0.5, 0.25]))
    assert got[1] == "one kind=%d weights=%s" % (LINEAR, h([3.0, -1.0]))
    assert got[2] == "ensemble kind=%d weights=%s" % (ENSEMBLE, h([0.5, 0.75, 0.75, 0.25, 0.125]))
    members = [[1.0, 2.0], [3.0, -1.0], [0.5, 0.25], [9.0, 9.0], [0.0, 0.0]]
    for line, w in zip(got[3:8], members):
        w = list(w)
        model.l1_normalize(w)
        assert line == "member kind=%d weights=%s" % (LINEAR, h(w))
    assert got[8:] == ["empty refused=1"]
