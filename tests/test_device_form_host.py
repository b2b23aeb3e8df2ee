"""The numpy restatement of the device form (tests/device_form_model.py) held to its own definitions, without a device:
tests/test_gpu_device_form.py compares the tables the device built with it, so the restatement must not be wrong in the
same way.  The tile index is a bijection, the restated walk tiles are the library's host rule, every segment's visiting
order is a permutation of it, and the storage order inside a query reproduces the oracle's total order."""
import numpy as np

from fastrank_amd import native
from oracle import pyoracle as o
from tests import device_form_model as dfm

QLENS = [1, 2, 63, 64, 65, 127, 128, 129, 300, 800]


def _random_layouts():
    rng = np.random.default_rng(5)
    yield QLENS
    yield QLENS[::-1]
    yield [800, 800, 1, 767, 1, 768, 769]
    for _ in range(20):
        nq = int(rng.integers(1, 50))
        yield np.clip(rng.lognormal(np.log(60), 1.1, nq), 1, 900).astype(np.int64).tolist()


def test_tile_index_is_a_bijection_onto_the_buffer():
    for npos, d in ((64, 1), (128, 3), (192, 4), (256, 5), (64, 8), (320, 9), (128, 136)):
        dq = (d + 3) // 4
        idx = dfm.xb_index(np.arange(npos)[:, None], np.arange(4 * dq)[None, :], dq).ravel()
        assert np.array_equal(np.sort(idx), np.arange(npos * 4 * dq)), (npos, d)
    # four consecutive features of one document are 16 contiguous bytes; the 64 documents of a tile follow each other
    assert dfm.xb_index(5, 4, 3) + 1 == dfm.xb_index(5, 5, 3) and dfm.xb_index(5, 4, 3) + 4 == dfm.xb_index(6, 4, 3)
    assert dfm.xb_index(64, 0, 3) == 3 * 256


def test_runs_start_on_tile_boundaries_and_hold_about_768_documents():
    for qlens in _random_layouts():
        lay = dfm.layout(qlens)
        assert lay["np"] % 64 == 0 and (lay["run_pos"] % 64 == 0).all()
        assert lay["run_q0"][0] == 0 and lay["run_q1"][-1] == len(qlens) and np.array_equal(lay["run_q0"][1:], lay["run_q1"][:-1])
        for r in range(len(lay["run_pos"])):
            q0, q1 = int(lay["run_q0"][r]), int(lay["run_q1"][r])
            assert lay["run_docs"][r] == sum(qlens[q0:q1])
            assert lay["run_docs"][r] <= dfm.RUN_DOCS or q1 == q0 + 1             # only a single long query exceeds it
            assert lay["qstart"][q0] == lay["run_pos"][r]                           # packed tightly from the run's start
            assert np.array_equal(lay["qstart"][q0:q1], lay["run_pos"][r] + np.concatenate([[0], np.cumsum(qlens[q0:q1])[:-1]]))
            if q1 < len(qlens):                                                     # the next query did not fit
                assert lay["run_docs"][r] + qlens[q1] > dfm.RUN_DOCS
        docs = lay["run_docs"][lay["run_order"]].astype(np.int64)
        assert (np.diff(docs) <= 0).all() and sorted(lay["run_order"].tolist()) == list(range(len(docs)))


def test_restated_walk_tiles_are_the_librarys_host_rule():
    for qlens in _random_layouts():
        lay = dfm.layout(qlens)
        wt, run_wt0, seg = dfm.walk_tiles(lay)
        w = native.walk_tiles(lay["run_pos"], lay["run_q0"], lay["run_q1"], lay["qstart"], lay["qlen"], lay["np"])
        assert w["walk_tile"] == dfm.WALK_TILE
        assert wt.tolist() == w["wt_start"] and run_wt0.tolist() == w["run_wt0"] and seg.tolist() == w["seg"]


def test_every_segments_restated_visiting_order_is_a_permutation_of_it():
    rng = np.random.default_rng(9)
    lay = dfm.layout(QLENS)
    wt, _, seg = dfm.walk_tiles(lay)
    Xp = np.zeros((lay["np"], 5), dtype=np.float32)
    Xp[:, 0] = rng.normal(size=lay["np"])
    Xp[:, 1] = rng.integers(0, 2, lay["np"])
    Xp[:, 2] = 3.0
    Xp[:, 3] = np.where(rng.random(lay["np"]) < 0.3, np.nan, rng.integers(-2, 3, lay["np"]))
    Xp[:, 4] = np.where(rng.random(lay["np"]) < 0.5, -0.0, 0.0)
    xs = dfm.xslot(Xp, wt, seg)
    segs = dfm.segments(wt, seg)
    assert sum(hi - lo for lo, hi in segs) == sum(QLENS) and max(hi - lo for lo, hi in segs) == dfm.WALK_TILE
    starts = wt.astype(np.int64)
    for lo, hi in segs:
        t0 = int(starts[np.searchsorted(starts[:-1], lo, side="right") - 1])
        for f in range(5):
            slots = xs[f, lo:hi].astype(np.int64) + t0
            assert np.array_equal(np.sort(slots), np.arange(lo, hi)), (lo, hi, f)
            by_slot = np.empty(hi - lo, dtype=np.int64)
            by_slot[slots - lo] = np.arange(lo, hi)                       # the positions in visiting order
            x = np.where(np.isnan(Xp[by_slot, f]), -np.inf, Xp[by_slot, f])
            assert (x[1:] <= x[:-1]).all()                                # x descending ...
            assert (np.diff(by_slot)[x[1:] == x[:-1]] > 0).all()          # ... and ties to the earlier position
        assert np.array_equal(xs[2, lo:hi], np.arange(lo, hi) - t0)       # a constant column: storage order
        assert np.array_equal(xs[4, lo:hi], np.arange(lo, hi) - t0)       # -0.0 == +0.0: storage order as well


def test_storage_order_with_later_wins_ties_is_the_oracles_rank_order(trec):
    """Inside a query documents are stored gain descending, then id descending: ranking by score descending where, among
    equal scores, the LATER stored document comes first gives the reference's total order (score desc, gain asc, id asc)."""
    X, y, qid = trec["train_X"], trec["train_y"], trec["train_qid"]
    keys, groups = dfm.regroup(y, qid)
    assert sorted(np.concatenate(groups).tolist()) == list(range(len(y)))
    first = [int(np.flatnonzero(qid == k)[0]) for k in keys]
    assert first == sorted(first)                                         # first-appearance order
    gain = y.astype(np.float32)
    rng = np.random.default_rng(3)
    score_sets = [np.zeros(len(y)), X[:, 1].astype(np.float64), np.floor(rng.normal(size=len(y)) * 2.0) / 2.0, -gain.astype(np.float64)]
    for scores in score_sets:
        for k, ids in zip(keys, groups):
            assert (qid[ids] == k).all()
            s = scores[ids]
            # stable sort of the REVERSED storage order by score descending: later stored documents win ties
            rev = ids[::-1]
            mine = rev[np.argsort(-s[::-1], kind="stable")]
            exp = o.rank_order(s, gain[ids], ids.astype(np.uint32))
            assert mine.tolist() == exp.tolist(), k


def test_gain_tables_and_duplicate_groups_of_a_small_case():
    gain = np.array([3.0, 0.0, -0.0, 0.5, -1.0, 0.0], dtype=np.float32)
    has = np.array([True, True, True, True, True, False])
    gexp, cls, tab = dfm.gain_tables(gain, has)
    assert gexp.tolist() == [7.0, 0.0, 0.0, 2.0 ** 0.5 - 1.0, -0.5, 0.0]
    assert cls.tolist() == [0, 2, 2, 1, 3, 0] and tab.shape == (4, dfm.DCG_RANKS)
    assert tab[0, 0] == 7.0 and tab[0, 2] == 7.0 / 2.0 and tab[3, 0] == -0.5
    X = np.array([[1.0, 0.0], [1.0, -0.0], [1.0, 0.0], [2.0, 0.0], [1.0, 0.0]], dtype=np.float32)
    label, n = dfm.duplicate_groups(X, [np.array([0, 1, 2, 3]), np.array([4])])
    assert n == 1 and set(label) == {0, 2}                                # row 1 differs in a zero's sign; row 4 is another query's
    mn, mx, at_min, at_max, mode = dfm.column_stats(np.array([[-0.0, -3.0], [0.0, -0.0], [0.0, -3.0]], dtype=np.float32))
    assert mn.tolist() == [0.0, -3.0] and mx.tolist() == [0.0, 0.0] and at_min.tolist() == [3, 2] and at_max.tolist() == [3, 1]
    assert mode.tolist() == [3, 3]
    assert dfm.colmax(np.array([[1.0, np.nan, -np.inf, -0.0], [-2.0, 1.0, 1.0, 0.0]], dtype=np.float32)).tolist() == [2.0, np.inf, np.inf, 0.0]
