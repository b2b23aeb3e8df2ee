"""The numpy restatement of the device form (tests/device_form_model.py) held to its own definitions, without a device:
tests/test_gpu_device_form.py compares the tables the device built with it, so the restatement must not be wrong in the
same way.  The tile index is a bijection, the restated walk tiles are the library's host rule, every segment's visiting
order is a permutation of it, and the storage order inside a query reproduces the oracle's total order.

The second half holds the library's own host-side layout (csrc/dataset_layout.hpp, read with native.host_layout: what
DeviceDataset::create / create_view compute before they upload) to the same restatement, again without a device."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import fastrank_amd as fr
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


# ---- the library's host-side layout (csrc/dataset_layout.hpp through native.host_layout) -----------------------------------


def _dataset(qlens, d, labels, seed):
    """Queries of the given lengths with interleaved rows (first appearance in order 0, 1, ...), labels drawn from `labels`."""
    rng = np.random.default_rng(seed)
    rest = np.repeat(np.arange(len(qlens), dtype=np.int64), np.asarray(qlens, dtype=np.int64) - 1)
    qid = np.concatenate([np.arange(len(qlens), dtype=np.int64), rest[rng.permutation(len(rest))]])   # one row of every query first
    y = rng.choice(np.asarray(labels, dtype=np.float64), size=len(qid))
    X = rng.normal(size=(len(qid), d)).astype(np.float32)
    return rng, X, y, qid


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _partition_matches(h, m, label):
    """gkey's group ids (0 = no duplicate, ids per query) describe the partition `label` {instance id: group}."""
    group = h["gkey"].astype(np.int64) >> h["key_cls_bits"]
    for q, ids in enumerate(m.groups):
        lo = int(m.lay["qstart"][q])
        got = group[lo: lo + len(ids)]
        exp = np.array([label.get(int(i), -1) for i in ids])
        assert np.array_equal(got == 0, exp == -1), q
        assert np.array_equal(got[:, None] == got[None, :], exp[:, None] == exp[None, :]), q


def test_host_layout_run_and_position_tables_are_the_restatement():
    for k, qlens in enumerate(_random_layouts()):
        _, X, y, qid = _dataset(qlens, 2, range(5), 20 + k)
        h = native.host_layout(fr.CDataset.from_numpy(X, y, qid))
        m = dfm.Form(X, y, qid, order_tables=False)
        assert (h["np"], h["nq"], h["n"], h["d"], h["dq"], h["nruns"]) == (m.np, len(qlens), len(y), 2, 1, len(m.lay["run_pos"]))
        assert h["maxlen"] == max(qlens) and h["no_document"] == dfm.NO_DOCUMENT and h["walk_tile"] == dfm.WALK_TILE
        for name in ("qstart", "qlen", "run_q0", "run_q1", "run_pos", "run_docs", "run_order"):
            assert h[name].dtype == np.uint32 and np.array_equal(h[name], m.lay[name]), (name, qlens)
        assert not h["run_lo"].any() and np.array_equal(h["qtight"], np.concatenate([[0], np.cumsum(qlens)]))
        assert np.array_equal(h["perm_host"], m.perm) and np.array_equal(h["perm"], m.perm)
        assert h["nwt"] == len(m.wt_start) - 1 and np.array_equal(h["wt_start"], m.wt_start)
        assert np.array_equal(h["run_wt0"], m.run_wt0) and np.array_equal(h["segtab"], m.segtab)
        starts = m.wt_start.astype(np.int64)
        docs = np.flatnonzero(m.has_document)
        assert np.array_equal(h["wofs"][docs], docs - starts[np.searchsorted(starts[:-1], docs, side="right") - 1])
        assert not h["wofs"][~m.has_document].any()


@pytest.mark.parametrize("labels", [tuple(range(5)), tuple(range(32)), (-1.5, -0.0, 0.0, 0.25, 2.75, 3.0)], ids=["0..4", "0..31", "fractional"])
def test_host_layout_gain_tables(labels):
    _, X, y, qid = _dataset(QLENS, 3, labels, 40 + len(labels))
    h = native.host_layout(fr.CDataset.from_numpy(X, y, qid))
    m = dfm.Form(X, y, qid, order_tables=False)
    assert np.array_equal(_bits(h["gain"]), _bits(m.gain)) and np.array_equal(_bits(h["gexp"]), _bits(m.gexp))
    assert np.array_equal(h["gcls"], m.gcls) and h["ncls"] == len(m.dcgtab) == len(set(float(v) + 0.0 for v in labels))
    assert np.array_equal(_bits(h["dcgtab"]), _bits(m.dcgtab))
    assert h["labels_small_int"] == all(float(v).is_integer() for v in labels)
    class_gain = np.unique(m.gain[m.has_document] + np.float32(0.0))[::-1]
    assert h["relmask"] == sum(1 << c for c, g in enumerate(class_gain) if g > 0)
    for q, ids in enumerate(m.groups):
        g = np.asarray(y, dtype=np.float32)[ids]
        assert (h["qnpos"][q], h["qnneg"][q]) == ((g > 0).sum(), (g < 0).sum()), q
    tablen = 16
    while tablen < max(QLENS):
        tablen *= 2
    assert h["tablen"] == tablen and h["termtab"].shape == (h["ncls"] + 1, tablen)
    exp = np.array([[m.dcgtab[c, 0] / math.log2(r + 2.0) for r in range(tablen)] for c in range(h["ncls"])])
    assert np.array_equal(_bits(h["termtab"][:-1]), _bits(exp)) and not _bits(h["termtab"][-1]).any()


def _planted_duplicates(across_classes):
    """About six queries of 2-40 documents, d = 3: rows equal bit for bit inside a query -- inside one gain class, and
    (across_classes) under different labels -- and rows that differ from another only in the sign of a zero."""
    qlens = [2, 7, 40, 13, 25, 31]
    rng, X, y, qid = _dataset(qlens, 3, range(5), 77)
    X[:, 1] = rng.integers(-1, 2, len(y))                     # a column with zeros to flip
    rows = [np.flatnonzero(qid == q) for q in range(len(qlens))]
    for q in (1, 2, 3, 4, 5):
        a, b, c, e = (int(v) for v in rows[q][:4])
        X[b], y[b] = X[a], y[a]                               # a duplicate inside one gain class
        X[a, 1] = X[b, 1] = 0.0
        X[c], y[c] = X[a], y[a]
        X[c, 1] = -0.0                                        # equal by value, not bit for bit: another row
        if across_classes:
            X[e], y[e] = X[a], (y[a] + 1.0) % 5.0             # a duplicate under another label
    three = rows[2][10:13]
    X[three] = X[three[0]]                                    # a group of three
    y[three] = y[three[0]]
    return X, y, qid


def test_host_layout_duplicate_groups_under_any_row_hash():
    X, y, qid = _planted_duplicates(across_classes=True)
    ds = fr.CDataset.from_numpy(X, y, qid)
    m = dfm.Form(X, y, qid, order_tables=False)
    label, ngroups = dfm.duplicate_groups(X, m.groups)
    assert ngroups == 6 and len(label) == 5 * 3 + 3
    colliding = np.zeros(m.np, dtype=np.uint64)
    colliding[m.has_document] = (X[m.perm[m.has_document], 1] == 0).astype(np.uint64)   # -0.0 / +0.0 rows and others that hold a zero share a hash
    for row_hash in (None, np.zeros(m.np, dtype=np.uint64), colliding):
        h = native.host_layout(ds, row_hash=row_hash)
        cls_bits = h["key_cls_bits"]
        assert (1 << cls_bits) >= h["ncls"] > (1 << cls_bits) // 2 and cls_bits < h["key_bits"] <= 16
        assert np.array_equal(h["gkey"] & ((1 << cls_bits) - 1), m.gcls)
        assert h["dup_groups"] == ngroups
        _partition_matches(h, m, label)


def test_host_layout_duplicates_inside_one_class_need_no_group_bits_and_verify_xs_starts_by_their_share():
    X, y, qid = _planted_duplicates(across_classes=False)
    m = dfm.Form(X, y, qid, order_tables=False)
    label, ngroups = dfm.duplicate_groups(X, m.groups)
    h = native.host_layout(fr.CDataset.from_numpy(X, y, qid))
    assert h["dup_groups"] == ngroups == 6 and h["key_bits"] == h["key_cls_bits"] and np.array_equal(h["gkey"], m.gcls)
    assert len(label) * 200 > len(y) and h["verify_xs"] == 4
    # exactly 0.5 % duplicated (2 of 400 documents) stays at 1, one pair more (4 of 400) starts at 4
    for pairs, xs in ((1, 1), (2, 4)):
        rng, X, y, qid = _dataset([100, 100, 100, 100], 3, range(5), 5)
        for q in range(pairs):
            a, b = (int(v) for v in np.flatnonzero(qid == q)[:2])
            X[b] = X[a]
        h = native.host_layout(fr.CDataset.from_numpy(X, y, qid))
        assert h["dup_groups"] == pairs and h["verify_xs"] == xs, pairs


def test_host_layout_views_are_the_restatement_and_refuse_a_view_that_differs():
    rng, X, y, qid = _dataset(QLENS + [129, 1, 300, 64, 2, 127], 3, range(5), 11)
    ds = fr.CDataset.from_numpy(X, y, qid)
    m = dfm.Form(X, y, qid, order_tables=False)
    nq = len(m.groups)
    for sel in (np.arange(0, nq, 2), np.arange(3, 11)):       # every second query; a contiguous block
        v = native.host_layout(ds, parent_queries=sel)["view"]
        vl = dfm.view_layout(m.lay, m.wt_start, sel)
        assert (v["np"], v["nq"], v["n"], v["nruns"]) == (m.np, len(sel), int(vl["qlen"].sum()), len(vl["run_q0"]))
        for name in ("qstart", "qlen", "run_q0", "run_q1", "run_pos", "run_lo", "run_docs", "run_order", "run_wt0", "vtiles", "wlist"):
            assert np.array_equal(v[name], vl[name]), name
        assert np.array_equal(v["qtight"], np.concatenate([[0], np.cumsum(vl["qlen"])]))
        mine = np.zeros(m.np, dtype=bool)
        for b, n in zip(vl["qstart"], vl["qlen"]):
            mine[int(b): int(b + n)] = True
        assert np.array_equal(v["perm_host"], np.where(mine, m.perm, dfm.NO_DOCUMENT))
    assert native.host_layout(ds, parent_queries=np.arange(3, 11))["view"]["run_lo"].any()
    # a view whose own regrouping differs from the parent's: another length, then another order inside a query
    with pytest.raises(Exception, match="create_view: a query of the view differs from the parent's"):
        native.host_layout(ds, parent_queries=[2, 4], view=ds.subsample_queries(["2", "3"]))
    y2 = y.copy()
    ids = m.groups[4]
    y2[ids] = y[ids][::-1] + 10.0 * (np.arange(len(ids)) == 0)  # (the first stored document can no longer be first)
    other = fr.CDataset.from_numpy(X, y2, qid)
    with pytest.raises(Exception, match="create_view: document order inside a query differs from the parent's"):
        native.host_layout(ds, parent_queries=[2, 4], view=other.subsample_queries(["2", "4"]))
    same = native.host_layout(ds, parent_queries=[2, 4], view=ds.subsample_queries(["2", "4"]))["view"]
    assert np.array_equal(same["qstart"], m.lay["qstart"][[2, 4]])


def test_size_classes_are_stable_partitions_of_the_queries():
    qlens = [129, 1, 64, 2049, 65, 128, 1, 129, 64, 65, 2049, 128, 63]
    _, X, y, qid = _dataset(qlens, 1, range(3), 3)
    h = native.host_layout(fr.CDataset.from_numpy(X, y, qid), parent_queries=np.arange(1, len(qlens)))
    pad = lambda n: max(64, 1 << (int(n) - 1).bit_length())
    assert [pad(n) for n in (1, 64, 65, 128, 129, 2049)] == [64, 64, 128, 128, 256, 4096]
    for lay, lens in ((h, np.asarray(qlens)), (h["view"], np.asarray(qlens[1:]))):
        for classes, qlist, rule in ((lay["size_classes"], lay["qlist"], pad), (lay["fv_classes"], lay["fv_qlist"], None)):
            assert sorted(qlist.tolist()) == list(range(len(lens)))                 # a partition of 0..nq-1 ...
            assert classes[:, 1].tolist() == np.concatenate([[0], np.cumsum(classes[:, 2])[:-1]]).tolist() and classes[:, 2].sum() == len(lens)
            assert (np.diff(classes[:, 0].astype(np.int64)) > 0).all()              # ... into ascending classes ...
            seen = {}
            for c, off, cnt in classes.tolist():
                members = qlist[off: off + cnt]
                assert cnt > 0 and (np.diff(members.astype(np.int64)) > 0).all()    # ... in dataset order inside a class
                if rule is not None:
                    assert [rule(n) for n in lens[members]] == [c] * cnt
                for n in lens[members]:
                    assert seen.setdefault(min(int(n), 2048), c) == c               # one class per length
        assert lay["size_classes"][:, 0].tolist() == [64, 128, 256, 4096]


def test_dataset_layout_header_under_address_and_undefined_sanitizers(tmp_path):
    """tests/dataset_layout_sanitize.cpp: a program of its own over csrc/dataset_layout.hpp alone (a query longer than a
    walk tile, a view), built with -fsanitize=address,undefined and run directly."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "dataset_layout_sanitize")
    build = subprocess.run([cxx, "-std=c++17", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                            "-I", os.path.join(here, "..", "fastrank_amd", "csrc"), os.path.join(here, "dataset_layout_sanitize.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "dataset_layout ok" in run.stdout, run.stdout


def test_linesearch_policy_header_under_address_and_undefined_sanitizers(tmp_path):
    """tests/linesearch_policy_sanitize.cpp: a program of its own over csrc/linesearch_policy.hpp alone (the refresh schedule,
    the rank-mode switch, routing and back-off, the list-length ramp, the redo grid, the skip counter: sequences worked out by
    hand), built with -fsanitize=address,undefined and run directly."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "linesearch_policy_sanitize")
    build = subprocess.run([cxx, "-std=c++17", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                            "-I", os.path.join(here, "..", "fastrank_amd", "csrc"), os.path.join(here, "linesearch_policy_sanitize.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "linesearch_policy ok" in run.stdout, run.stdout
