"""Model comparison without a device: the numpy restatement (tests/resample_model.py) against its own
term-by-term form, the reference's percentiles, the permutation test against exact enumeration, the bootstrap's centring, the
uniformity of both streams, the refusals that need no device, and csrc/resample_host.hpp under the sanitizers."""
import itertools
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import native
from tests import resample_model as rm

NO_DEVICE = "no MI355X/HIP device available"


@pytest.mark.parametrize("Q,M,T", [(1, 1, 3), (5, 2, 4), (258, 3, 2), (300, 4, 2), (7, 8, 3)])
def test_vectorised_restatement_equals_the_term_by_term_one(Q, M, T):
    V = rm.designed_table(Q, M, 11 * Q + M)
    for seed in (0, 0xFFFFFFFFFFFFFFFF):
        assert np.array_equal(rm.boot(V, T, seed).view(np.uint64), rm.boot_scalar(V, T, seed).view(np.uint64))
        assert np.array_equal(rm.perm(V, T, seed).view(np.uint64), rm.perm_scalar(V, T, seed).view(np.uint64))
    assert np.array_equal(rm.means(V).view(np.uint64), np.array([rm._sum_scalar([float(x) for x in V[:, c]]) / float(Q) for c in range(M)]).view(np.uint64))


def test_a_trial_does_not_depend_on_the_number_of_trials_and_seeds_differ():
    V = rm.designed_table(40, 3, 5)
    a, b = rm.boot(V, 9, 3), rm.boot(V, 4, 3)
    assert np.array_equal(a[:4].view(np.uint64), b.view(np.uint64))
    assert not np.array_equal(rm.boot(V, 4, 4), b) and not np.array_equal(rm.perm(V, 4, 4), rm.perm(V, 4, 3))
    # a chunked run is the run in one piece
    old, rm.CHUNK_CELLS = rm.CHUNK_CELLS, 90
    try:
        assert np.array_equal(rm.boot(V, 9, 3).view(np.uint64), a.view(np.uint64))
    finally:
        rm.CHUNK_CELLS = old


@pytest.mark.parametrize("Q", [258, 513, 600, 16385])
def test_the_sums_shape_shows_on_the_designed_tables(Q):
    """The tables tests/test_gpu_resample.py uses for Q >= 258: SUM differs from the plain sequential sum and from np.sum, so
    a device that added in another shape would not give the restatement's bits."""
    V = rm.visible_table(Q, 2)
    m, plain = rm.seq_sum(V.T), np.cumsum(V, axis=0)[-1]
    for c in range(2):
        assert m[c] != plain[c] and m[c] != np.sum(V[:, c])


def test_one_extra_term_cannot_tell_the_shapes_apart():
    V = rm.designed_table(257, 2, 257)
    assert np.array_equal(rm.seq_sum(V.T), np.cumsum(V, axis=0)[-1])


def test_percentiles_are_the_references_as_written():
    assert rm.percentile(np.arange(10.0), 0.5) == 4.5  # src/stats.rs:193-198
    assert rm.percentile(np.arange(9.0), 0.5) == 4.0
    # by hand: four values, p = 0.25: position 0.75 between 0 and 10; as written 0.75 * 0 + 0.25 * 10 = 2.5 (a linear
    # interpolation would give 7.5: the nearer order statistic, 10, weighs less)
    assert rm.percentile([0.0, 10.0, 20.0, 30.0], 0.25) == 2.5
    assert rm.percentile([0.0, 10.0, 20.0, 30.0], 0.75) == 27.5  # position 2.25: 0.25 * 20 + 0.75 * 30 (linear: 22.5)
    assert rm.percentile([0.0, 10.0, 20.0, 30.0], 0.0) == 0.0 and rm.percentile([0.0, 10.0, 20.0, 30.0], 1.0) == 30.0
    assert rm.percentile([3.0], 0.95) == 3.0
    # the interval: order statistics, no interpolation
    assert rm.interval(np.arange(200.0), 0.05) == [4.0, 195.0]  # floor(0.025 * 199) = 4, ceil(0.975 * 199) = ceil(194.025) = 195
    assert rm.interval([7.0], 0.05) == [7.0, 7.0]


def test_permutation_p_value_against_exact_enumeration():
    """Q = 10, M = 2: all 2^10 assignments of straight / swapped, in the restatement's own arithmetic.  The T = 20 000 estimate
    must lie within 5 sqrt(p (1 - p) / T) of the exact value (the binomial standard error; 5 sigma for a fixed seed)."""
    rng = np.random.default_rng(2024)
    Q, T = 10, 20000
    V = np.stack([rng.normal(size=Q), rng.normal(size=Q) + 0.25], axis=1)
    m = rm.means(V)
    observed = abs(m[0] - m[1])
    hits = 0
    for swaps in itertools.product((0, 1), repeat=Q):
        W = np.where(np.array(swaps)[:, None] == 1, V[:, ::-1], V)
        w = rm.means(W)
        hits += (max(w) - min(w)) >= observed
    exact = hits / 2.0 ** Q
    got = rm.p_values(V, rm.perm(V, T, 7))[(0, 1)]
    print("exact", exact, "estimate", got, "bound", 5.0 * math.sqrt(exact * (1.0 - exact) / T))
    assert 0.0 < exact < 1.0
    assert abs(got - exact) <= 5.0 * math.sqrt(exact * (1.0 - exact) / T)


def test_bootstrap_means_are_centred_on_the_observed_means():
    Q, T = 1000, 2000
    V = np.random.default_rng(5).normal(size=(Q, 2)) * [1.0, 3.0] + [0.5, -2.0]
    b = rm.boot(V, T, 1)
    m = rm.means(V)
    for c in range(2):
        bound = 5.0 * np.std(V[:, c]) / math.sqrt(Q * T)
        print("column", c, "error", abs(b[:, c].mean() - m[c]), "bound", bound)
        assert abs(b[:, c].mean() - m[c]) <= bound


def test_bootstrap_indices_are_uniform():
    """2 000 trials x 1 000 draws over 1 000 rows: chi-square per degree of freedom inside [0.8, 1.2] (999 degrees: its
    standard deviation is sqrt(2 / 999) = 0.045)."""
    T, Q = 2000, 1000
    counts = np.bincount(rm.draws(9, np.arange(T), Q).ravel(), minlength=Q)
    assert counts.sum() == T * Q and len(counts) == Q
    chi = float(((counts - T) ** 2 / T).sum()) / (Q - 1)
    print("chi-square per degree of freedom", chi)
    assert 0.8 <= chi <= 1.2


@pytest.mark.parametrize("M", [2, 3, 4])
def test_permutations_are_uniform(M):
    """400 trials x 500 permutations.  Per trial, the counts of the M! permutations among its 500: 400 (M! - 1) degrees of
    freedom in all, chi-square per degree inside [0.8, 1.2] (its standard deviation is sqrt(2 / (400 (M! - 1))), 0.07 at M = 2:
    pooled over the trials M = 2 would leave one degree, and no seed could be held to [0.8, 1.2] with that).  The pooled
    counts are held to their own bound: chi-square at most dof + 5 sqrt(2 dof)."""
    T, Q, F = 400, 500, math.factorial(M)
    p = rm.permutations(13, np.arange(T), Q, M)
    assert np.array_equal(np.sort(p, axis=-1), np.broadcast_to(np.arange(M), p.shape))
    index = {perm: n for n, perm in enumerate(itertools.permutations(range(M)))}
    code = np.zeros((T, Q), dtype=np.int64)
    for c in range(M):
        code = code * M + p[:, :, c]
    lookup = np.full(M ** M, -1, dtype=np.int64)
    for perm, n in index.items():
        k = 0
        for x in perm:
            k = k * M + x
        lookup[k] = n
    which = lookup[code]
    assert which.min() >= 0
    counts = np.stack([np.bincount(row, minlength=F) for row in which])
    chi = float(((counts - Q / F) ** 2 / (Q / F)).sum()) / (T * (F - 1))
    pooled = counts.sum(axis=0)
    chi_pooled = float(((pooled - T * Q / F) ** 2 / (T * Q / F)).sum())
    print("M", M, "chi-square per degree of freedom", chi, "pooled chi-square", chi_pooled, "degrees", F - 1)
    assert 0.8 <= chi <= 1.2
    assert chi_pooled <= (F - 1) + 5.0 * math.sqrt(2.0 * (F - 1))


def test_m2_permutation_rows_are_straight_or_swapped():
    V = rm.designed_table(30, 2, 3)
    p = rm.permutations(5, np.arange(6), 30, 2)
    assert set(map(tuple, p.reshape(-1, 2))) == {(0, 1), (1, 0)}


def test_report_of_a_model_against_itself():
    V = np.repeat(np.random.default_rng(1).random((50, 1)), 2, axis=1)
    rep = rm.report(V, 0.05, rm.boot(V, 20, 0), rm.perm(V, 20, 0))
    [pair] = rep["pairs"]
    assert pair["diff"] == 0.0 and pair["p"] == 1.0 and (pair["wins"], pair["losses"], pair["ties"]) == (0, 0, 50)
    assert pair["diff_interval"] == [0.0, 0.0]


def test_refusals_that_need_no_device():
    ok = np.ones((4, 2))
    bad = ok.copy()
    bad[2, 1] = np.nan
    with pytest.raises(Exception, match="non-finite value in row 2, column 1"):
        native.resample(bad, 10, 0)
    bad[2, 1], bad[3, 0] = 1.0, -np.inf
    with pytest.raises(Exception, match="non-finite value in row 3, column 0"):
        native.resample(bad, 10, 0)
    with pytest.raises(Exception, match="between 1 and 8 systems, not 0"):
        native.resample(np.ones((4, 0)), 10, 0)
    with pytest.raises(Exception, match="between 1 and 8 systems, not 9"):
        native.resample(np.ones((4, 9)), 10, 0)
    with pytest.raises(Exception, match="trials must be between 1 and 1048576, not 0"):
        native.resample(ok, 0, 0)
    with pytest.raises(Exception, match="trials must be between 1 and 1048576, not 1048577"):
        native.resample(ok, (1 << 20) + 1, 0)
    with pytest.raises(Exception, match="at least one query"):
        native.resample(np.ones((0, 2)), 10, 0)
    with pytest.raises(Exception, match="alpha must lie strictly between 0 and 1"):
        native.resample(ok, 10, 0, alpha=1.0)
    reply = fr.clib._json_reply
    with pytest.raises(Exception, match="unknown field `trails`, expected one of `trials`, `seed`, `alpha`"):
        reply(fr.clib._load().fr_resample(ok.ctypes.data, 4, 2, b'{"trails": 10}', None, None))


@pytest.mark.skipif(native.device_count() > 0, reason="checks the no-GPU failure mode")
def test_resample_without_gpu_fails_loudly():
    with pytest.raises(Exception, match=NO_DEVICE):
        native.resample(np.ones((4, 2)), 10, 0)


def test_host_header_under_address_and_undefined_sanitizers(tmp_path):
    """tests/resample_host_sanitize.cpp: a program of its own over csrc/resample_host.hpp (the sum's segment edges, the
    percentile at both ends and on one value, the report with either array missing, every refusal), built with
    -fsanitize=address,undefined and run directly."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "resample_host_sanitize")
    build = subprocess.run([cxx, "-std=c++17", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                            "-I", os.path.join(here, "..", "fastrank_amd", "csrc"), os.path.join(here, "resample_host_sanitize.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "resample_host ok" in run.stdout, run.stdout
