"""The device form of a dataset, read back with native.device_form and held table by table to the
numpy restatement in tests/device_form_model.py: tiles, the column-major copy, the position map and run tables, walk tiles
and visiting order, column maxima and statistics, gains, gain classes and duplicate groups -- for owned datasets, sampled
views, a file-loaded dataset, a device-to-device copy, and the upload path only a large dataset takes.

Every equality is bitwise.  The one tolerance is the bound any-order f64 summation allows the column sums:
(n - 1) * 2^-53 * sum |t| around math.fsum."""
import functools
import math
import os

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import native
from tests import device_form_model as dfm

pytestmark = pytest.mark.gpu

# every boundary of the layout: one document, a tile and a walk tile minus / plus one, longer than a run (3001 documents)
QLENS = [1, 2, 63, 64, 65, 127, 128, 129, 300, 800, 129, 1, 300, 64, 2, 127, 65, 63, 128, 256, 100, 87]
DIMS = [1, 3, 4, 5, 8, 9, 136]  # dq = 1, 1, 1, 2, 2, 3, 34: odd and even quad counts under two quads per block
ARRAYS = ("xb", "xcol", "xslot", "perm", "perm_host", "gain", "gexp", "gcls", "gkey", "segtab", "wofs", "wt_start", "qstart", "qlen",
          "qtight", "run_q0", "run_q1", "run_pos", "run_docs", "run_lo", "run_order", "run_wt0", "vtiles", "wlist", "dcgtab", "colmax",
          "colstd", "colmode", "colstats")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_bytes(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes())


def _queries(seed, labels=(0.0, 1.0, 2.0, 3.0, 4.0)):
    """Query ids in shuffled row order (queries interleave) and labels."""
    rng = np.random.default_rng(seed)
    qid = np.repeat(np.arange(1, len(QLENS) + 1, dtype=np.int64), QLENS)[rng.permutation(sum(QLENS))]
    y = rng.choice(np.asarray(labels, dtype=np.float64), size=len(qid))
    return rng, y, qid


def _matrix(rng, n, d):
    """Columns by j % 6: continuous (signed), 0/1, constant, small integers with both zeros, denormals, heavy-tailed."""
    X = np.empty((n, d), dtype=np.float32)
    for j in range(d):
        k = j % 6
        if k == 0:
            col = rng.normal(size=n)
        elif k == 1:
            col = rng.integers(0, 2, n).astype(np.float64)
        elif k == 2:
            col = np.full(n, 2.5)
        elif k == 3:
            col = rng.integers(-2, 3, n).astype(np.float64)
            col[(col == 0) & (rng.random(n) < 0.5)] = -0.0
        elif k == 4:
            col = rng.integers(-5, 6, n) * float(np.float32(1e-45))
        else:
            col = rng.lognormal(0.0, 2.0, n)
        X[:, j] = col.astype(np.float32)
    return X


def _duplicate_rows(rng, X, y, qid, pairs=40):
    """Copies of rows inside their query (under another label where `y` allows: a group of mixed gain classes)."""
    for _ in range(pairs):
        a = int(rng.integers(0, len(qid)))
        same = np.flatnonzero(qid == qid[a])
        b = int(rng.choice(same))
        if a != b:
            X[b] = X[a]


@functools.lru_cache(maxsize=None)
def _case(d):
    rng, y, qid = _queries(100 + d)
    X = _matrix(rng, len(qid), d)
    _duplicate_rows(rng, X, y, qid)
    ds = fr.CDataset.from_numpy(X, y, qid)
    return X, y, qid, ds, native.device_form(ds), dfm.Form(X, y, qid)


# ---- the layout ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("d", DIMS)
def test_position_map_and_run_tables(d):
    X, y, qid, ds, f, m = _case(d)
    assert (f["np"], f["dq"], f["d"], f["n"], f["nq"]) == (m.np, m.dq, d, len(y), len(QLENS)) and f["nonfinite"] is False
    assert f["no_document"] == dfm.NO_DOCUMENT and not f["shares_parent_matrix"] and f["nvtiles"] == 0
    assert np.array_equal(f["perm"], m.perm) and np.array_equal(f["perm_host"], m.perm)
    for name in ("qstart", "qlen", "run_q0", "run_q1", "run_pos", "run_docs", "run_order"):
        assert np.array_equal(f[name], m.lay[name]), name
    assert not f["run_lo"].any()
    assert np.array_equal(f["qtight"], np.concatenate([[0], np.cumsum(m.lay["qlen"])]))
    assert max(QLENS) > dfm.RUN_DOCS and f["nruns"] == len(m.lay["run_pos"]) > 3


@pytest.mark.parametrize("d", DIMS)
def test_tiles_hold_the_rows_bit_for_bit_and_zero_everywhere_else(d):
    X, y, qid, ds, f, m = _case(d)
    xb = f["xb"]
    assert xb.shape == (m.np // 64 * m.dq * 256,)
    docs = np.flatnonzero(f["perm"] != dfm.NO_DOCUMENT)
    got = xb[dfm.xb_index(docs[:, None], np.arange(d)[None, :], m.dq)]
    assert np.array_equal(_bits(got), _bits(X[f["perm"][docs]]))          # sign of zero and denormals included
    if d >= 5:
        assert (_bits(X) == 0x80000000).any() and ((_bits(X) & 0x7F800000 == 0) & (_bits(X) & 0x007FFFFF != 0)).any()
    pad_cols = np.arange(d, 4 * m.dq)
    if len(pad_cols):
        assert not _bits(xb[dfm.xb_index(np.arange(m.np)[:, None], pad_cols[None, :], m.dq)]).any()   # +0.0 bits
    empty = np.flatnonzero(f["perm"] == dfm.NO_DOCUMENT)
    assert len(empty) > 0
    assert not _bits(xb[dfm.xb_index(empty[:, None], np.arange(4 * m.dq)[None, :], m.dq)]).any()
    assert np.array_equal(_bits(xb), _bits(m.tiles()))


@pytest.mark.parametrize("d", DIMS)
def test_columns_are_the_transpose_of_the_tiles(d):
    X, y, qid, ds, f, m = _case(d)
    assert f["xcol"] is not None and f["xcol"].shape == (d, m.np)
    exp = f["xb"][dfm.xb_index(np.arange(m.np)[None, :], np.arange(d)[:, None], m.dq)]   # every p < np: padding positions too
    assert np.array_equal(_bits(f["xcol"]), _bits(exp))
    assert np.array_equal(_bits(f["xcol"]), _bits(np.ascontiguousarray(m.Xp.T)))


@pytest.mark.parametrize("d", DIMS)
def test_walk_tiles_and_visiting_order(d):
    X, y, qid, ds, f, m = _case(d)
    assert f["walk_tile"] == dfm.WALK_TILE and f["nwt"] == len(m.wt_start) - 1
    assert np.array_equal(f["wt_start"], m.wt_start) and np.array_equal(f["run_wt0"], m.run_wt0)
    assert np.array_equal(f["segtab"], m.segtab)
    starts = m.wt_start.astype(np.int64)
    tile = np.searchsorted(starts[:-1], np.arange(m.np), side="right") - 1
    assert np.array_equal(f["wofs"][m.has_document], (np.arange(m.np) - starts[tile])[m.has_document])
    # x descending inside every (query, walk tile) segment, ties to the earlier position: constant, 0/1 and duplicated
    # columns are all ties, the continuous ones have none.  (Positions without a document are never written.)
    assert f["xslot"] is not None and f["xslot"].shape == (d, m.np)
    assert np.array_equal(f["xslot"][:, m.has_document], m.xslot[:, m.has_document])


@pytest.mark.parametrize("d", DIMS)
def test_column_maxima_are_exact(d):
    X, y, qid, ds, f, m = _case(d)
    assert np.array_equal(f["colmax"], np.abs(X).max(axis=0).astype(np.float64)) and np.array_equal(f["colmax"], dfm.colmax(X))


# ---- optional copies -----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("switch, gone", [("FR_XCOL", ("xcol",)), ("FR_VERIFY_ORDER", ("xslot", "colstd", "colmode", "colstats"))])
def test_a_switched_off_copy_is_absent_and_the_rest_unchanged(monkeypatch, switch, gone):
    """FR_XCOL=0: no column-major copy.  FR_VERIFY_ORDER=0: no visiting-order table, and the column statistics that only
    steer it are not taken either.  Every other table is what the default build holds (the column sums and what is made
    from them up to the order of their additions: the statistics kernel adds them with atomics)."""
    X, y, qid, _, f, m = _case(5)
    monkeypatch.setenv(switch, "0")
    g = native.device_form(fr.CDataset.from_numpy(X.copy(), y.copy(), qid.copy()))
    for name in ARRAYS:
        if name in gone:
            assert f[name] is not None and g[name] is None, name
        elif name == "xslot":                                # (positions without a document are never written)
            assert np.array_equal(f[name][:, m.has_document], g[name][:, m.has_document])
        elif name == "colstats":                             # (the sums are added in any order: two builds may differ in
            for field in ("mn", "mx", "at_min", "at_max"):   # their last bits, each within test_column_statistics' bound)
                assert _same_bytes(f[name][field], g[name][field]), field
        elif name == "colstd":                               # (... and colstd is the host's formula on the build's own sums)
            assert np.array_equal(_bits(g[name]), _bits(dfm.colstd_from_sums(g["colstats"]["sum"], g["colstats"]["sumsq"], len(y))))
            _check_column_stats(g, X)
        else:
            assert _same_bytes(f[name], g[name]), name


# ---- column maxima: what the error bound of bound-and-verify multiplies by ------------------------------------------------


def _maxima_matrix():
    rng, y, qid = _queries(7)
    n = len(qid)
    X = np.zeros((n, 9), dtype=np.float32)
    X[:, 1] = -0.0
    X[:, 2] = (rng.integers(-9, 10, n) * float(np.float32(1e-45))).astype(np.float32)     # only denormals (and zeros)
    X[:, 3] = rng.uniform(-3.0, 3.0, n)
    X[n // 2, 3] = -7.25                                                                  # the maximum |x| is negative
    X[:, 4] = rng.uniform(-1.0, 1.0, n)
    X[0, 4] = 5.5                                                                         # in the first row
    X[:, 5] = rng.uniform(-1.0, 1.0, n)
    X[n - 1, 5] = -6.5                                                                    # in the last row
    X[:, 6] = rng.uniform(-1.0, 1.0, n)
    X[::256, 6] = 9.0                                                                     # in every 256th row
    X[:, 7] = rng.normal(size=n)
    X[:, 8] = rng.lognormal(0.0, 3.0, n)
    return X, y, qid


def test_column_maxima_of_designed_columns():
    X, y, qid = _maxima_matrix()
    f = native.device_form(fr.CDataset.from_numpy(X, y, qid))
    exp = np.abs(X).max(axis=0).astype(np.float64)
    assert exp[0] == 0.0 and exp[1] == 0.0 and 0.0 < exp[2] < 2e-44 and exp[3] == 7.25 and exp[4] == 5.5 and exp[5] == 6.5 and exp[6] == 9.0
    assert np.array_equal(_bits(f["colmax"]), _bits(exp))
    assert f["nonfinite"] is False


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
def test_a_non_finite_column_has_an_infinite_maximum(bad):
    X, y, qid = _maxima_matrix()
    X[1234, 7] = bad
    f = native.device_form(fr.CDataset.from_numpy(X, y, qid))
    assert f["nonfinite"] is True
    assert np.array_equal(_bits(f["colmax"]), _bits(dfm.colmax(X))) and f["colmax"][7] == np.inf and np.isfinite(np.delete(f["colmax"], 7)).all()


# ---- the upload path of a large dataset ------------------------------------------------------------------------------------


def test_large_upload_two_slabs_many_threads_gapped_row_ids(monkeypatch):
    """120 000 rows x 72 features = 34.6 MB: above 100 000 rows the slabs are filled by a pool of threads, one memcpy per
    stretch of consecutive row ids, and above 32 MB a second slab follows the first.  The dataset is a query sample that
    tiles its own matrix (FR_VIEW_COPIES=1), so its row ids come in three stretches with gaps between them.  Every
    column's extreme sits at a seam: the first uploaded row, the last row of slab 1, the first row of slab 2, the last row."""
    d = 72
    stretches = [(0, 50000), (50100, 90100), (90300, 120300)]
    rows = np.concatenate([np.arange(a, b) for a, b in stretches])
    total = stretches[-1][1]
    slab_rows = (32 << 20) // (d * 4)
    assert len(rows) == 120000 > 100000 and slab_rows < len(rows) and len(rows) * d * 4 > (32 << 20)
    rng = np.random.default_rng(12)
    qid = np.zeros(total, dtype=np.int64)                    # query 0: the rows in the gaps, not sampled
    qid[rows] = rng.integers(1, 1001, len(rows))
    y = rng.integers(0, 5, total).astype(np.float64)
    X = rng.uniform(-1.0, 1.0, (total, d)).astype(np.float32)
    seams = [0, slab_rows - 1, slab_rows, len(rows) - 1]
    for j in range(d):
        X[rows[seams[j % 4]], j] = (100.0 + j) * (-1.0 if (j // 4) % 2 else 1.0)
    X[np.setdiff1d(np.arange(total), rows)] = 1e6           # rows outside the sample must not be seen
    monkeypatch.setenv("FR_VIEW_COPIES", "1")
    whole = fr.CDataset.from_numpy(X, y, qid)
    view = whole.subsample_queries([str(q) for q in range(1, 1001)])
    f = native.device_form(view)
    m = dfm.Form(X, y, qid, rows=rows, order_tables=False)
    assert (f["n"], f["d"], f["np"], f["nq"]) == (len(rows), d, m.np, 1000) and not f["shares_parent_matrix"] and f["nonfinite"] is False
    assert np.array_equal(f["perm"], m.perm) and np.array_equal(f["qstart"], m.lay["qstart"])
    assert np.array_equal(_bits(f["xb"]), _bits(m.tiles()))
    assert np.array_equal(_bits(f["xcol"]), _bits(np.ascontiguousarray(m.Xp.T)))
    Xd = X[rows]
    exp = np.abs(Xd).max(axis=0).astype(np.float64)
    assert np.array_equal(exp, 100.0 + np.arange(d))
    assert np.array_equal(_bits(f["colmax"]), _bits(exp))
    _check_column_stats(f, Xd, sums_of=range(0, d, 9))


# ---- column statistics ---------------------------------------------------------------------------------------------------


def _check_column_stats(f, Xd, sums_of=None):
    n, d = Xd.shape
    st = f["colstats"]
    mn, mx, at_min, at_max, mode = dfm.column_stats(Xd)
    print("colstats mn", st["mn"][:8], "mx", st["mx"][:8], "at_min", st["at_min"][:8], "at_max", st["at_max"][:8])
    assert np.array_equal(st["mn"], mn) and np.array_equal(st["mx"], mx)                   # by value: -0.0 == 0.0
    assert np.array_equal(st["at_min"], at_min) and np.array_equal(st["at_max"], at_max)
    assert np.array_equal(f["colmode"], mode)
    for j in (range(d) if sums_of is None else sums_of):
        t = Xd[:, j].astype(np.float64)
        for got, terms in ((st["sum"][j], t), (st["sumsq"][j], t * t)):                    # (a product of two f32 is exact in f64)
            allow = (n - 1) * 2.0 ** -53 * math.fsum(np.abs(terms))
            assert abs(got - math.fsum(terms)) <= allow, (j, got, math.fsum(terms), allow)
    assert np.array_equal(_bits(f["colstd"]), _bits(dfm.colstd_from_sums(st["sum"], st["sumsq"], n)))


@pytest.mark.parametrize("d", DIMS)
def test_column_statistics(d):
    X, y, qid, ds, f, m = _case(d)
    _check_column_stats(f, X)


def _zero_sign_matrix():
    """Column 0: negatives among the documents stored first, many +0.0, positives and a few -0.0 among those stored last (a
    thread of the statistics kernel then sees only -0.0 or positive values).  Column 1: all negative but for a few -0.0."""
    rng, y, qid = _queries(21)
    keys, groups = dfm.regroup(y, qid)
    perm = dfm.position_map(dfm.layout([len(g) for g in groups]), groups)
    docs = perm[perm != dfm.NO_DOCUMENT].astype(np.int64)    # instance ids in storage order
    n = len(docs)
    X = np.zeros((n, 4), dtype=np.float32)
    early, late = docs[: n // 2], docs[n // 2:]
    X[early, 0] = np.where(rng.random(len(early)) < 0.5, 0.0, -rng.integers(1, 6, len(early)))
    X[late, 0] = np.where(rng.random(len(late)) < 0.7, 0.0, rng.integers(1, 4, len(late)))
    X[late[-40::4], 0] = -0.0
    X[:, 1] = -rng.integers(1, 5, n)
    X[docs[5::97], 1] = -0.0
    X[:, 2] = rng.normal(size=n)
    X[:, 3] = rng.integers(0, 2, n)
    assert (_bits(X[:, 0]) == 0x80000000).sum() == 10 and (_bits(X[:, 1]) == 0x80000000).sum() > 5
    return X, y, qid


def test_extremes_take_zeros_by_value_on_every_build():
    """A minimum of -0.0 in one thread must not beat the negative minimum of another, and a maximum of -0.0 must beat every
    negative one: the records, and the lane classes made from them, are the same on every build of the form."""
    X, y, qid = _zero_sign_matrix()
    mn, mx, at_min, at_max, mode = dfm.column_stats(X)
    assert mn[0] == -5.0 and mx[0] == 3.0 and mn[1] == -4.0 and mx[1] == 0.0 and at_max[1] == (_bits(X[:, 1]) == 0x80000000).sum()
    for build in range(5):
        f = native.device_form(fr.CDataset.from_numpy(X.copy(), y.copy(), qid.copy()))
        _check_column_stats(f, X)


# ---- gains, gain classes, duplicate groups ---------------------------------------------------------------------------------


@pytest.mark.parametrize("labels", [tuple(range(5)), tuple(range(32)), (-1.5, -0.0, 0.0, 0.25, 2.75, 3.0)], ids=["0..4", "0..31", "fractional"])
def test_gains_classes_and_duplicate_groups(labels):
    rng, y, qid = _queries(40 + len(labels), labels)
    n, d = len(qid), 5
    X = _matrix(rng, n, d)
    for _ in range(60):                                     # duplicated rows inside a query, under another label
        a = int(rng.integers(0, n))
        same = np.flatnonzero((qid == qid[a]) & (y != y[a]))
        if len(same):
            X[int(rng.choice(same))] = X[a]
    # the rule for a zero's sign, pinned: rows that differ ONLY there are different rows (groups are of bit-identical rows)
    big = np.flatnonzero(qid == 10)
    a, b, c = (int(v) for v in big[:3])
    X[a, 1] = 0.0
    X[b] = X[a]
    X[c] = X[a]
    X[c, 1] = -0.0
    y[a], y[b] = labels[0], labels[-1]
    ds = fr.CDataset.from_numpy(X, y, qid)
    f = native.device_form(ds)
    m = dfm.Form(X, y, qid, order_tables=False)
    assert np.array_equal(_bits(f["gain"]), _bits(m.gain))
    assert np.array_equal(_bits(f["gexp"]), _bits(m.gexp))
    assert np.array_equal(f["gcls"], m.gcls) and f["ncls"] == len(m.dcgtab) == len(set(float(v) + 0.0 for v in labels))
    assert np.array_equal(_bits(f["dcgtab"]), _bits(m.dcgtab))
    # gkey = class | group << class bits, at most 16 bits in all
    cls_bits = f["key_cls_bits"]
    assert (1 << cls_bits) >= f["ncls"] > (1 << cls_bits) // 2 and f["key_bits"] <= 16
    assert not (f["gkey"].astype(np.int64) >> f["key_bits"]).any()
    assert np.array_equal(f["gkey"] & ((1 << cls_bits) - 1), m.gcls)
    label, ngroups = dfm.duplicate_groups(X, m.groups)
    assert f["dup_groups"] == ngroups > 10 and f["key_bits"] > cls_bits
    assert a in label and label[a] == label[b] and label.get(c, -1) != label[a]
    group = f["gkey"].astype(np.int64) >> cls_bits
    for q, ids in enumerate(m.groups):
        lo = int(m.lay["qstart"][q])
        got = group[lo: lo + len(ids)]
        exp = np.array([label.get(int(i), -1) for i in ids])
        assert np.array_equal(got == 0, exp == -1), q      # 0 = no duplicate in the query
        assert np.array_equal(got[:, None] == got[None, :], exp[:, None] == exp[None, :]), q


# ---- the host-side layout the library serves without a device is what create() / create_view() uploaded -------------------


def test_host_layout_is_what_the_device_holds():
    qlens = [1, 2, 63, 64, 65, 127, 128, 129, 300, 800]
    rng = np.random.default_rng(77)
    qid = np.repeat(np.arange(1, len(qlens) + 1, dtype=np.int64), qlens)[rng.permutation(sum(qlens))]
    y = rng.choice(np.arange(5.0), size=len(qid))
    X = _matrix(rng, len(qid), 5)
    for _ in range(12):                                     # duplicated rows inside a query, some under another label
        a = int(rng.integers(0, len(qid)))
        X[int(rng.choice(np.flatnonzero(qid == qid[a])))] = X[a]
    ds = fr.CDataset.from_numpy(X, y, qid)
    f = native.device_form(ds)
    sel = np.arange(0, len(qlens), 2)                       # the view's queries, as indices of the dataset's stored queries
    keys, _ = dfm.regroup(y, qid)
    view = ds.subsample_queries([str(q) for q in keys[sel]])
    vf = native.device_form(view)
    h = native.host_layout(ds, parent_queries=sel)
    assert vf["shares_parent_matrix"] and len(h["view"]["vtiles"]) and len(h["view"]["wlist"])
    shared = sorted(k for k in h if k in f and k != "gkey" and k != "view")
    assert {"perm", "perm_host", "gain", "gexp", "gcls", "segtab", "wofs", "wt_start", "qstart", "qlen", "qtight", "run_q0", "run_q1",
            "run_pos", "run_docs", "run_lo", "run_order", "run_wt0", "dcgtab", "np", "nq", "n", "d", "dq", "nruns", "nwt", "maxlen",
            "ncls", "key_bits", "key_cls_bits", "dup_groups", "no_document", "walk_tile", "dcg_ranks"} <= set(shared)
    for name in shared:
        if isinstance(h[name], np.ndarray):
            assert _same_bytes(h[name], f[name]), name
        else:
            assert h[name] == f[name], name
    for name in sorted(k for k in h["view"] if k in vf):
        if isinstance(h["view"][name], np.ndarray):
            assert _same_bytes(h["view"][name], vf[name]), name
        else:
            assert h["view"][name] == vf[name], name
    assert {"qstart", "qlen", "qtight", "run_lo", "run_wt0", "vtiles", "wlist", "perm_host", "nruns", "maxlen"} <= set(h["view"]) & set(vf)
    # the host hook hashes rows on the host, the device with row_hash_kernel: group ids may be numbered differently, the
    # groups they name are the same
    cls_bits = f["key_cls_bits"]
    assert f["dup_groups"] > 0 and f["key_bits"] > cls_bits
    assert np.array_equal(h["gkey"] & ((1 << cls_bits) - 1), f["gkey"] & ((1 << cls_bits) - 1))
    for b, n in zip(f["qstart"], f["qlen"]):
        got, exp = (g[int(b): int(b + n)].astype(np.int64) >> cls_bits for g in (h["gkey"], f["gkey"]))
        assert np.array_equal(got == 0, exp == 0) and np.array_equal(got[:, None] == got[None, :], exp[:, None] == exp[None, :])


# ---- views -----------------------------------------------------------------------------------------------------------------


def test_query_sample_aliases_its_parent_and_owns_its_query_tables():
    X, y, qid, ds, pf, m = _case(9)
    picked = m.keys[[0, 1, 2, 4, 5, 8, 9, 10, 14, 15, 16, 18]].tolist()   # stretches of queries stored back to back, and gaps
    view = ds.subsample_queries([str(q) for q in picked])
    f = native.device_form(view)
    assert f["shares_parent_matrix"] and native.device_info(view)["shares_parent_matrix"]
    for name in ("xb", "xcol", "xslot", "segtab", "gkey", "perm"):
        assert f[name + "_addr"] == pf[name + "_addr"] != 0, name
    for name in ("xb", "xcol", "xslot", "segtab", "wofs", "wt_start", "perm", "gain", "gexp", "gcls", "gkey", "dcgtab", "colmax", "colstd",
                 "colmode", "colstats"):
        assert _same_bytes(f[name], pf[name]), name
    sel = np.array([list(m.keys).index(q) for q in picked if q in set(m.keys.tolist())])
    sel = np.sort(sel)                                       # the view keeps the parent's query order
    vl = dfm.view_layout(m.lay, m.wt_start, sel)
    assert (f["np"], f["nq"], f["n"]) == (m.np, len(sel), int(vl["qlen"].sum()))
    for name in ("qstart", "qlen", "run_q0", "run_q1", "run_pos", "run_lo", "run_docs", "run_order", "run_wt0", "vtiles", "wlist"):
        assert np.array_equal(f[name], vl[name]), name
    assert len(vl["run_q0"]) < len(sel) and vl["run_lo"].any()
    mine = np.zeros(m.np, dtype=bool)
    for b, n in zip(vl["qstart"], vl["qlen"]):
        mine[int(b): int(b + n)] = True
    assert np.array_equal(f["perm_host"], np.where(mine, m.perm, dfm.NO_DOCUMENT))
    own = np.abs(X[m.perm[mine]]).max(axis=0)
    assert np.array_equal(f["colmax"], pf["colmax"]) and (f["colmax"] >= own).all()


def test_feature_sample_reports_its_parents_form():
    X, y, qid, ds, pf, m = _case(9)
    fview = ds.subsample_feature_names([str(j) for j in (0, 2, 3, 7)])
    f = native.device_form(fview)
    assert all(f[k] == pf[k] for k in pf if not isinstance(pf[k], np.ndarray) and pf[k] is not None)
    assert all(_same_bytes(f[name], pf[name]) for name in ARRAYS)


# ---- a file-loaded dataset -------------------------------------------------------------------------------------------------


def test_absent_values_of_a_file_loaded_dataset_read_zero_in_the_tiles(tmp_path):
    rng = np.random.default_rng(31)
    n, d = 300, 9
    qid = np.repeat(np.arange(1, 7), 50)
    y = rng.integers(0, 5, n).astype(np.float64)
    X = np.zeros((n, d + 1), dtype=np.float32)
    X[:, 1:] = 4.0 + rng.integers(0, 17, (n, d)) / 8.0
    path = str(tmp_path / "sparse.train")
    with open(path, "w") as fh:
        for i in range(n):
            if rng.random() < 0.4:                          # a sparse row: three of nine features, the rest absent
                keep = np.zeros(d + 1, dtype=bool)
                keep[rng.choice(np.arange(1, d), 2, replace=False)] = True
                keep[d] = True
                X[i, ~keep] = 0.0
            fh.write("%d qid:%d %s\n" % (int(y[i]), int(qid[i]), " ".join("%d:%r" % (j, float(X[i, j])) for j in range(1, d + 1) if X[i, j] != 0.0)))
    f = native.device_form(fr.CDataset.open_ranksvm(path))
    m = dfm.Form(X, y, qid)
    assert f["d"] == d + 1 and f["n"] == n and (X[:, 1:] == 0.0).any()
    assert np.array_equal(f["perm"], m.perm)
    assert np.array_equal(_bits(f["xb"]), _bits(m.tiles()))
    assert np.array_equal(_bits(f["xcol"]), _bits(np.ascontiguousarray(m.Xp.T)))
    assert np.array_equal(f["colmax"], dfm.colmax(X))


# ---- nothing a trainer does moves a static table ---------------------------------------------------------------------------


def _train(ds, req, devices=None):
    old = os.environ.pop("FR_DEVICES", None)
    try:
        if devices is not None:
            os.environ["FR_DEVICES"] = devices
        return ds.train_model(req)
    finally:
        os.environ.pop("FR_DEVICES", None)
        if old is not None:
            os.environ["FR_DEVICES"] = old


def _ca_request(restarts):
    req = fr.TrainRequest.coordinate_ascent()
    req.measure = "ndcg@10"
    p = req.params
    p.num_restarts, p.num_max_iterations, p.seed, p.quiet = restarts, 3, 42, True
    return req


def test_training_leaves_every_static_table_byte_identical():
    X, y, qid, _, _, _ = _case(8)
    ds = fr.CDataset.from_numpy(X.copy(), y.copy(), qid.copy())
    before = native.device_form(ds)
    _train(ds, _ca_request(4))
    lm = fr.TrainRequest.lambdamart()
    lm.measure = "ndcg@10"
    lm.params.quiet, lm.params.grower, lm.params.num_trees, lm.params.max_depth = True, "histogram", 3, 3
    _train(ds, lm)
    after = native.device_form(ds)
    assert set(before) == set(after)
    for k in before:
        if isinstance(before[k], np.ndarray):
            assert _same_bytes(before[k], after[k]), k
        else:
            assert before[k] == after[k], k                  # sizes, switches and addresses: nothing was rebuilt


def test_device_to_device_copy_holds_the_sources_tables():
    """The same ordinal listed twice gives train_model a second context on this device whose dataset is a device-to-device
    copy of the first (tests/test_gpu_multidevice.py): every table of the copy is the source's, byte for byte."""
    X, y, qid, _, _, _ = _case(8)
    ds = fr.CDataset.from_numpy(X.copy(), y.copy(), qid.copy())
    with pytest.raises(Exception, match="no device copy"):
        native.device_form(ds, slot=1)
    _train(ds, _ca_request(4), "0,0")
    src, rep = native.device_form(ds), native.device_form(ds, slot=1)
    assert rep["xb_addr"] != src["xb_addr"] and rep["xcol_addr"] not in (0, src["xcol_addr"]) and not rep["shares_parent_matrix"]
    for k in src:
        if isinstance(src[k], np.ndarray):
            assert _same_bytes(src[k], rep[k]), k
        elif not k.endswith("_addr"):
            assert src[k] == rep[k], k
    assert native.release_replicas(ds) == 1
