"""The resampling kernels (csrc/kernels_resample.inc) against the numpy restatement
(tests/resample_model.py): `boot` and `perm` bit for bit at the lane, segment, column and staging edges, the streams'
properties, the host's report, and every refusal."""
import os

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import native
from tests import resample_model as rm

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check(V, T, seed, alpha=0.05):
    """one call: both arrays and the report against the restatement; returns (report, boot, perm)"""
    rep, boot, perm = native.resample(V, T, seed, alpha)
    want_b, want_p = rm.boot(V, T, seed), rm.perm(V, T, seed)
    assert rep["boot_path"] == ("lds" if V.size * 8 <= rm.LDS_BYTES else "global")
    if rep["boot_path"] == "lds":  # the same table through the kernel's other form
        os.environ["FR_RESAMPLE_BOOT"] = "global"
        try:
            rep_g, boot_g, _ = native.resample(V, T, seed, alpha, perm=False)
        finally:
            del os.environ["FR_RESAMPLE_BOOT"]
        assert rep_g["boot_path"] == "global" and np.array_equal(_bits(boot_g), _bits(want_b))
    assert boot.shape == want_b.shape == (T, V.shape[1]) and perm.shape == (T, V.shape[1])
    assert np.array_equal(_bits(boot), _bits(want_b))
    assert np.array_equal(_bits(perm), _bits(want_p))
    want = rm.report(V, alpha, want_b, want_p)
    for key in rm.REPORT_KEYS:
        assert rep[key] == want[key], key  # (floats cross as shortest round-trip digits: == is bit for bit; p is a ratio of integers)
    assert (rep["trials"], rep["seed"], rep["alpha"]) == (T, seed, alpha)
    return rep, boot, perm


@pytest.mark.parametrize("T", [1, 63, 64, 65, 130])
def test_lane_and_trial_edges(T):
    for M, Q in ((1, 37), (2, 300)):
        _check(rm.designed_table(Q, M, 100 + T), T, 5)


@pytest.mark.parametrize("Q", [1, 2, 255, 256, 258, 513, 600])
def test_segment_edges(Q):
    """Values N(0,1) 10^U{-8..8}.  From Q = 258 the table is one on which SUM differs, in every column, from the plain
    sequential sum and from np.sum (asserted here, on the host): bits equal to the restatement's then say that the device
    adds in SUM's shape.  (Q = 257 cannot tell: one extra term gives the same bits either way.)"""
    if Q >= 258:
        V = rm.visible_table(Q, 2)
        shaped, plain = rm.seq_sum(V.T), np.cumsum(V, axis=0)[-1]
        for c in range(2):
            assert shaped[c] != plain[c] and shaped[c] != np.sum(V[:, c])
    else:
        V = rm.designed_table(Q, 2, Q)
    rep, boot, perm = _check(V, 65, 9)
    assert np.array_equal(_bits(rep["means"]), _bits(rm.means(V)))


@pytest.mark.parametrize("M", [1, 2, 3, 8])
def test_columns(M):
    V = rm.designed_table(300, M, 40 + M)
    rep, boot, perm = _check(V, 65, 3)
    assert len(rep["pairs"]) == M * (M - 1) // 2
    # the draws are shared: column c of the M-column call is the one-column call on V[:, c]
    for c in range(M):
        _, one, _ = native.resample(V[:, c:c + 1], 65, 3, perm=False)
        assert np.array_equal(_bits(one[:, 0]), _bits(boot[:, c]))
    # a permutation moves values inside a row only: the row sums stay (here: the multiset of every trial's row of means
    # is made of the same queries' values, so for M = 1 perm is the observed mean itself)
    if M == 1:
        assert np.array_equal(_bits(perm[:, 0]), _bits(np.repeat(rm.means(V), 65)))


def test_m2_permutation_rows_are_straight_or_swapped_in_lane_order():
    """Q = 1: a trial's permuted row is the query's pair straight or swapped, as that trial's stream says."""
    V = np.array([[0.25, -3.0]])
    _, _, perm = native.resample(V, 130, 11, boot=False)
    p = rm.permutations(11, np.arange(130), 1, 2)[:, 0, :]
    assert np.array_equal(_bits(perm), _bits(V[0][p]))
    assert {tuple(r) for r in perm.tolist()} == {(0.25, -3.0), (-3.0, 0.25)}
    # several queries, powers of two (every sum exact): a trial's two means hold each query's pair once, so they add up to
    # the table's sum, and the first mean is the sum of the values its stream chose
    V = np.ldexp(1.0, np.arange(32)).reshape(16, 2)
    _, _, perm = native.resample(V, 65, 11, boot=False)
    p = rm.permutations(11, np.arange(65), 16, 2)
    assert np.array_equal(perm.sum(axis=1) * 16, np.full(65, V.sum()))
    assert np.array_equal(perm[:, 0] * 16, np.take_along_axis(np.broadcast_to(V, p.shape), p, axis=-1)[:, :, 0].sum(axis=1))


def test_streams():
    V = rm.designed_table(300, 3, 77)
    _, b65, p65 = native.resample(V, 65, 21)
    _, b130, p130 = native.resample(V, 130, 21)
    assert np.array_equal(_bits(b65), _bits(b130[:65])) and np.array_equal(_bits(p65), _bits(p130[:65]))
    _, b_other, p_other = native.resample(V, 65, 22)
    assert not np.array_equal(_bits(b_other), _bits(b65)) and not np.array_equal(_bits(p_other), _bits(p65))
    _, b_again, p_again = native.resample(V, 65, 21)
    assert b_again.tobytes() == b65.tobytes() and p_again.tobytes() == p65.tobytes()
    # a seed beyond 2^63 crosses the ABI whole
    _check(V[:40], 3, 0xFFFFFFFFFFFFFFFF)


@pytest.mark.parametrize("Q,M,path", [(16384, 1, "lds"), (16385, 1, "global"), (2048, 8, "lds"), (2049, 8, "global")])
def test_bootstrap_path_at_the_staging_limit(Q, M, path):
    """Q M 8 bytes exactly 128 KiB, and one row more"""
    assert (Q * M * 8 <= rm.LDS_BYTES) == (path == "lds")
    V = rm.designed_table(Q, M, Q + M)
    rep, boot, _ = native.resample(V, 64, 2, perm=False)
    assert rep["boot_path"] == path
    assert np.array_equal(_bits(boot), _bits(rm.boot(V, 64, 2)))


def test_either_output_may_be_skipped():
    V = rm.designed_table(50, 2, 1)
    rep, boot, perm = native.resample(V, 10, 4, boot=False)
    assert boot is None and "intervals" not in rep and "summary" not in rep and "diff_interval" not in rep["pairs"][0]
    assert np.array_equal(_bits(perm), _bits(rm.perm(V, 10, 4))) and rep["pairs"][0]["p"] == rm.p_values(V, perm)[(0, 1)]
    rep, boot, perm = native.resample(V, 10, 4, perm=False)
    assert perm is None and "p" not in rep["pairs"][0] and rep["intervals"] == rm.report(V, 0.05, boot)["intervals"]


def test_report_at_another_level_and_with_ties():
    rng = np.random.default_rng(8)
    V = np.round(rng.random((120, 3)), 1)  # (one decimal: many queries tie)
    rep, _, _ = _check(V, 130, 6, alpha=0.2)
    assert all(p["ties"] > 0 and p["wins"] + p["losses"] + p["ties"] == 120 for p in rep["pairs"])
    assert all(0.0 < p["p"] <= 1.0 for p in rep["pairs"])


def test_refusals():
    ok = np.ones((4, 2))
    bad = ok.copy()
    bad[2, 1] = np.nan
    with pytest.raises(Exception, match="non-finite value in row 2, column 1"):
        native.resample(bad, 10, 0)
    bad[2, 1], bad[3, 0] = 1.0, np.inf
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
    with pytest.raises(Exception, match="unknown field `trails`, expected one of `trials`, `seed`, `alpha`"):
        fr.clib._json_reply(fr.clib._load().fr_resample(ok.ctypes.data, 4, 2, b'{"trails": 10}', None, None))
    # and a good call right after them
    _check(ok, 3, 0)
