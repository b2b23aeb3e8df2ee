"""Feature normalisation on the device against the numpy restatement (tests/normalize_model.py), bit for
bit: the statistics of datasets and views, the matrices Normalizer.apply returns and the device form built from them, the
query scope, sigmoid against 60-digit decimals, every refusal, and training on a normalised dataset."""
import decimal

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import native
from tests import normalize_model as nm

pytestmark = pytest.mark.gpu


def _bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _hexes(stats):
    return {int(f): {k: (v if k == "num_elements" else float.hex(float(v))) for k, v in rec.items()} for f, rec in stats.items()}


def _qids(m, seed, lengths=None):
    """query ids of m rows in shuffled row order; query lengths from 1 up to 800 (as far as m allows)"""
    rng = np.random.default_rng(seed)
    if lengths is None:
        lengths, left = [], m
        for want in (800, 1, 2, 129, 65, 64, 300, 37):
            if left <= 0:
                break
            lengths.append(min(want, left))
            left -= lengths[-1]
        while left > 0:
            lengths.append(min(int(rng.integers(1, 60)), left))
            left -= lengths[-1]
    qid = np.repeat(np.arange(1, len(lengths) + 1, dtype=np.int64) * 3, lengths)
    assert len(qid) == m
    return qid[rng.permutation(m)]


def _matrix(m, d, seed):
    rng = np.random.default_rng(seed)
    X = np.empty((m, d), dtype=np.float32)
    for j in range(d):
        kind = j % 4
        if kind == 0:
            col = rng.normal(size=m) * 3 + 1
        elif kind == 1:
            col = np.floor(rng.exponential(2.0, m))
        elif kind == 2:
            col = rng.lognormal(0.0, 2.0, m) * 1e3
        else:
            col = np.where(rng.random(m) < 0.7, 0.0, rng.random(m))
        X[:, j] = col.astype(np.float32)
    return X


def _dataset(X, qid, seed=0):
    y = np.random.default_rng(seed).integers(0, 5, size=len(X)).astype(np.float64)
    return fr.CDataset.from_numpy(np.ascontiguousarray(X, dtype=np.float32), y, np.asarray(qid, dtype=np.int64)), y


_ALL = {}


def _all_held(X):
    key = X.shape
    if key not in _ALL:
        _ALL[key] = np.ones(X.shape, dtype=bool)
    return _ALL[key]


# -----------------------------------------------------------------------------------------------------------------------
# statistics
# -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 255, 256, 257, 513, 3001])
@pytest.mark.parametrize("d", [1, 3, 4, 5, 136])
def test_feature_stats_shapes(m, d):
    X = _matrix(m, d, 1000 * d + m)
    ds, _ = _dataset(X, _qids(m, m + d))
    got = ds.feature_stats()
    want = nm.fit(X, _all_held(X), np.arange(m), range(d))
    assert sorted(got) == sorted(want) == (list(range(d)) if m >= 2 else [])
    assert _hexes(got) == _hexes(want)
    if m <= nm.CHUNK:  # one chunk: the reference's StreamingStats itself
        for f in range(min(d, 5)):
            assert _hexes({f: nm.finish(nm.sequential(X[:, f]))}) == _hexes({f: got[f]}) if m >= 2 else f not in got


def test_feature_stats_designed_columns():
    m = 600
    rng = np.random.default_rng(8)
    X = np.zeros((m, 6), dtype=np.float32)
    X[:, 0] = 7.25
    X[:, 1] = -0.0
    X[:, 2] = (rng.integers(-50, 50, size=m).astype(np.float64) * 1.4e-45).astype(np.float32)                # f32 denormals
    X[:, 3] = (1e6 + 0.0625 * rng.integers(-3, 4, size=m)).astype(np.float32)                                 # one ulp apart
    X[:, 4] = np.float32(1e-30) * rng.normal(size=m).astype(np.float32)
    X[:, 5] = np.float32(1e30) * rng.normal(size=m).astype(np.float32)
    assert np.any((X[:, 2] != 0) & (np.abs(X[:, 2]) < 1.1754944e-38)) and np.signbit(X[:, 1]).all()
    ds, _ = _dataset(X, _qids(m, 4))
    got, want = ds.feature_stats(), nm.fit(X, _all_held(X), np.arange(m), range(6))
    assert _hexes(got) == _hexes(want)
    assert got[0]["variance"] == 0.0 and got[0]["mean"] == 7.25 and got[1]["variance"] == 0.0 and got[1]["max"] == 0.0
    for method in ("zscore", "maxmin"):
        n = fr.Normalizer.fit(ds, method)
        out = native.loaded_arrays(n.apply(ds))["x"]
        assert np.array_equal(_bits32(out), _bits32(nm.apply(X, _all_held(X), want, method)))
        assert not out[:, 0].any() and not out[:, 1].any() and not np.signbit(out[:, :2]).any()  # a constant column: exactly +0.0


def _write_sparse(path, m, seed):
    """a ranksvm text whose rows are sparse (each lists feature 40 and few others, so it holds exactly what it lists):
    feature 1 everywhere but in instances 256..511 (absent from one whole chunk), feature 2 in no row, 3 in one, 4 in two, 5
    and 6 at random; returns nothing -- the test reads the loaded arrays back"""
    rng = np.random.default_rng(seed)
    with open(path, "w") as fh:
        for i in range(m):
            feats = []
            if not 256 <= i < 512:
                feats.append((1, rng.normal()))
            if i == 300:
                feats.append((3, 2.5))
            if i in (10, 599):
                feats.append((4, float(i)))
            if rng.random() < 0.7:
                feats.append((5, float(np.floor(rng.exponential(3.0)))))
            if rng.random() < 0.5:
                feats.append((6, rng.lognormal(0, 2)))
            feats.append((40, rng.random()))
            fh.write("%d qid:%d %s # doc%d\n" % (i % 3, 1 + i // 50, " ".join("%d:%.9g" % (f, np.float32(v)) for f, v in feats), i))


@pytest.fixture(scope="module")
def sparse(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("normalize") / "sparse.ranksvm")
    _write_sparse(path, 700, 21)
    ds = fr.CDataset.open_ranksvm(path, parser="host")
    arr = native.loaded_arrays(ds)
    H = nm.held_mask(arr["present_bits"], arr["present_words"], arr["n"], arr["d"])
    return ds, arr, H


def test_feature_stats_skip_absent_values(sparse):
    ds, arr, H = sparse
    assert arr["present_words"] > 0 and not H[256:512, 1].any() and H[:256, 1].all() and H[:, 2].sum() == 0 and H[:, 3].sum() == 1 and H[:, 4].sum() == 2
    feats = sorted(ds.feature_ids())
    got = ds.feature_stats()
    want = nm.fit(arr["x"], H, np.arange(arr["n"]), feats)
    assert _hexes(got) == _hexes(want)
    assert 2 not in got and 3 not in got and got[4]["num_elements"] == 2 and got[1]["num_elements"] == 700 - 256
    assert got[5]["num_elements"] == int(H[:, 5].sum()) < 700


def test_apply_keeps_absent_values_absent(sparse):
    ds, arr, H = sparse
    st = nm.fit(arr["x"], H, np.arange(arr["n"]), sorted(ds.feature_ids()))
    for n, want in ((fr.Normalizer.fit(ds, "zscore"), nm.apply(arr["x"], H, st, "zscore")),
                    (fr.Normalizer.fit(ds, "linear"), nm.apply(arr["x"], H, st, "maxmin")),
                    (fr.Normalizer.per_query("zscore"), nm.per_query(arr["x"], H, arr["qix"], "zscore")),
                    (fr.Normalizer.per_query("maxmin"), nm.per_query(arr["x"], H, arr["qix"], "maxmin"))):
        out_ds = n.apply(ds)
        out = native.loaded_arrays(out_ds)
        assert np.array_equal(_bits32(out["x"]), _bits32(want))
        assert np.array_equal(out["present_bits"], arr["present_bits"]) and out["present_words"] == arr["present_words"]
        assert not out["x"][~H].any()
        for key in ("gain", "qix", "doc_present", "features"):
            assert np.array_equal(out[key], arr[key])
        assert out["qnames"] == arr["qnames"] and out["docids"] == arr["docids"] and out["has_docids"] == arr["has_docids"]
        assert out_ds.feature_index_to_name() == ds.feature_index_to_name() and out_ds.instances_by_query() == ds.instances_by_query()
        assert out_ds.normalization() == n.to_dict() and not out_ds.is_sampled()
    assert fr.Normalizer.fit(ds, "linear").to_dict().keys() == {"MaxMinNormalizer"}
    # the feature held once keeps its value (no record), the one held twice is mapped
    z = native.loaded_arrays(fr.Normalizer.fit(ds, "zscore").apply(ds))["x"]
    assert z[300, 3] == np.float32(2.5) and z[10, 4] != np.float32(10.0)


def test_fit_on_a_view_in_its_own_order():
    m, d = 1500, 7
    X = _matrix(m, d, 31)
    qid = _qids(m, 32)
    ds, _ = _dataset(X, qid)
    view = ds.subsample_queries(["21", "3", "6", "15", "12", "24"])  # the queries of 300, 800, 1, 65, 129 and 37 documents
    order = [i for ids in view.instances_by_query().values() for i in ids]
    assert order != sorted(order) and len(order) > 256
    assert _hexes(view.feature_stats()) == _hexes(nm.fit(X, _all_held(X), order, range(d)))
    fview = view.subsample_feature_names(["1", "4"])
    got = fview.feature_stats()
    assert sorted(got) == [1, 4] and _hexes(got) == _hexes(nm.fit(X, _all_held(X), order, [1, 4]))


# -----------------------------------------------------------------------------------------------------------------------
# apply
# -----------------------------------------------------------------------------------------------------------------------
def _same_device_form(a, b):
    fa, fb = native.device_form(a), native.device_form(b)
    for name in ("xb", "xcol", "perm"):
        assert (fa[name] is None) == (fb[name] is None), name
        if fa[name] is not None:
            assert fa[name].dtype == fb[name].dtype and np.array_equal(fa[name].view(np.uint8), fb[name].view(np.uint8)), name
    for name in ("np", "dq", "d", "n", "nq"):
        assert fa[name] == fb[name], name


@pytest.fixture(scope="module")
def wide():
    m, d = 3001, 136
    X = _matrix(m, d, 77)
    qid = _qids(m, 78)
    ds, y = _dataset(X, qid, 79)
    return ds, X, y, qid


@pytest.mark.parametrize("method", ["zscore", "maxmin"])
def test_apply_fitted(wide, method):
    ds, X, y, qid = wide
    H = _all_held(X)
    n = fr.Normalizer.fit(ds, method)
    want = nm.apply(X, H, nm.fit(X, H, np.arange(len(X)), range(X.shape[1])), method)
    out_ds = n.apply(ds)
    out = native.loaded_arrays(out_ds)
    assert np.array_equal(_bits32(out["x"]), _bits32(want)) and len(out["present_bits"]) == 0
    assert np.array_equal(out["gain"], y.astype(np.float32)) and out_ds.instances_by_query() == ds.instances_by_query()
    assert out_ds.num_features() == ds.num_features() and out_ds.feature_ids() == ds.feature_ids() and not out_ds.is_sampled()
    _same_device_form(out_ds, fr.CDataset.from_numpy(want, y, qid))
    assert out_ds.normalization() == n.to_dict() and ds.normalization() is None


@pytest.mark.parametrize("method", ["zscore", "maxmin"])
def test_apply_per_query(method):
    lengths = [1, 2, 64, 65, 129, 800, 3, 257, 256]
    m, d = sum(lengths), 37
    X = _matrix(m, d, 91)
    X[:, 5] = 2.0                      # constant in every query
    qid = _qids(m, 92, lengths)
    X[qid == 3 * 5, 6] = np.float32(4.5)   # constant in the query of 129
    ds, y = _dataset(X, qid, 93)
    want = nm.per_query(X, _all_held(X), qid, method)
    assert not want[qid == 3].any() and not want[:, 5].any() and want[qid == 18].any()
    out_ds = fr.Normalizer.per_query(method).apply(ds)
    out = native.loaded_arrays(out_ds)
    assert np.array_equal(_bits32(out["x"]), _bits32(want))
    _same_device_form(out_ds, fr.CDataset.from_numpy(want, y, qid))
    assert out_ds.normalization() == {"PerQuery": method}


def test_unknown_features_are_unchanged():
    m = 400
    A, B = _matrix(m, 6, 41), _matrix(300, 4, 42)
    train, _ = _dataset(A, _qids(m, 43))
    n = fr.Normalizer.fit(train.subsample_feature_names(["0", "2", "5"]), "zscore")
    assert sorted(n.feature_stats()) == [0, 2, 5]  # (5 is past the second dataset's matrix: ignored there)
    other, _ = _dataset(B, _qids(300, 44))
    out = native.loaded_arrays(n.apply(other))["x"]
    st = nm.fit(A, _all_held(A), np.arange(m), [0, 2, 5])
    assert np.array_equal(_bits32(out), _bits32(nm.apply(B, _all_held(B), st, "zscore")))
    assert np.array_equal(_bits32(out[:, [1, 3]]), _bits32(B[:, [1, 3]])) and not np.array_equal(out[:, 0], B[:, 0])


# -----------------------------------------------------------------------------------------------------------------------
# sigmoid
# -----------------------------------------------------------------------------------------------------------------------
def _sigmoid_neighbours(v):
    """the two f32 neighbours of the exact sigmoid of the f32 v, from 60-digit decimals"""
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        ctx.Emin, ctx.Emax = -999999, 999999
        x = decimal.Decimal(float(v))
        exact = 1 / (1 + (-x).exp())
        lo = np.float32(float(exact))  # (double rounding cannot leave the pair: both neighbours are taken below)
        if decimal.Decimal(float(lo)) > exact:
            lo = np.nextafter(lo, np.float32(-np.inf))
        hi = lo if decimal.Decimal(float(lo)) == exact else np.nextafter(lo, np.float32(np.inf))
        return lo, hi


def test_sigmoid_is_faithfully_rounded():
    rng = np.random.default_rng(55)
    special = [0.0, -0.0, 1.4e-45, -1.4e-45, 1e-40, -1e-40, 88.0, -88.0, 104.0, -104.0, 103.0, -103.0, np.inf, -np.inf, 1.0, -1.0, 17.0, -17.0]
    vals = np.concatenate([np.array(special, dtype=np.float32), (rng.normal(size=1500) * 8).astype(np.float32),
                           (rng.uniform(-110, 110, size=500)).astype(np.float32)])
    X = vals.reshape(-1, 2)
    ds, _ = _dataset(X, _qids(len(X), 56))
    out = native.loaded_arrays(fr.Normalizer.sigmoid().apply(ds))["x"].reshape(-1)
    assert np.all((out >= 0.0) & (out <= 1.0))
    order = np.argsort(vals, kind="stable")
    assert np.all(np.diff(out[order]) >= 0.0)  # non-decreasing in the input
    assert out[vals == np.inf][0] == 1.0 and out[vals == -np.inf][0] == 0.0 and out[0] == 0.5
    worst = 0
    for v, got in zip(vals, out):
        if np.isinf(v):
            continue
        lo, hi = _sigmoid_neighbours(v)
        assert got == lo or got == hi, (v, got, lo, hi)
        worst += int(got != nm.sigmoid_value(v))
    print("sigmoid: %d of %d values differ from the host's f64 exp form (both faithful)" % (worst, len(vals)))


# -----------------------------------------------------------------------------------------------------------------------
# refusals
# -----------------------------------------------------------------------------------------------------------------------
def _still_works(ds, X):
    got = ds.feature_stats()
    assert _hexes(got) == _hexes(nm.fit(X, _all_held(X), np.arange(len(X)), range(X.shape[1])))


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_values_are_refused_by_the_statistics(bad):
    m = 700
    X = _matrix(m, 6, 61)
    clean = X.copy()
    X[650, 1] = bad
    X[300, 4] = bad
    X[300, 2] = bad
    X[299, 5] = bad  # lies in a feature the sampled view below does not list
    ds, _ = _dataset(X, _qids(m, 62))
    text = "non-finite value in feature 2, instance 300: feature statistics need finite values"
    listed = ds.subsample_feature_names(["0", "1", "2", "3", "4"])
    for call in (lambda: fr.Normalizer.fit(listed, "zscore"), lambda: fr.Normalizer.fit(listed, "maxmin"), lambda: listed.feature_stats()):
        with pytest.raises(Exception) as exc:
            call()
        assert text in str(exc.value)
    for method in ("zscore", "maxmin"):
        with pytest.raises(Exception) as exc:
            fr.Normalizer.per_query(method).apply(ds)
        assert "non-finite value in feature 5, instance 299: feature statistics need finite values" in str(exc.value)
    # the source dataset goes on working: the features without the value, and a clean dataset after the refusals
    got = ds.subsample_feature_names(["0", "3"]).feature_stats()
    assert _hexes(got) == _hexes(nm.fit(X, _all_held(X), np.arange(m), [0, 3]))
    _still_works(_dataset(clean, _qids(m, 62))[0], clean)


def test_nan_results_are_refused_by_apply():
    m = 300
    X = _matrix(m, 4, 65)
    good, _ = _dataset(X, _qids(m, 66))
    n = fr.Normalizer.fit(good, "zscore")
    Y = X.copy()
    Y[200, 3] = np.nan
    Y[120, 2] = np.nan
    Y[120, 1] = np.inf   # passes through the arithmetic
    bad, _ = _dataset(Y, _qids(m, 66))
    with pytest.raises(Exception) as exc:
        n.apply(bad)
    assert "Normalization.zscore NaN: feature 2, instance 120" in str(exc.value)
    with pytest.raises(Exception) as exc:
        fr.Normalizer.sigmoid().apply(bad)
    assert "Normalization.sigmoid NaN: feature 2, instance 120" in str(exc.value)
    assert bad.normalization() is None
    Y[200, 3], Y[120, 2] = 1.0, 2.0
    ok, _ = _dataset(Y, _qids(m, 66))
    out = native.loaded_arrays(n.apply(ok))["x"]
    assert out[120, 1] == np.inf
    assert np.array_equal(_bits32(out), _bits32(nm.apply(Y, _all_held(Y), nm.fit(X, _all_held(X), np.arange(m), range(4)), "zscore")))
    _still_works(good, X)


def test_f32_range_overflow_under_maxmin():
    X = _matrix(40, 3, 67)
    X[7, 1], X[9, 1], X[30, 1] = 3e38, -3e38, 3e38
    ds, _ = _dataset(X, _qids(40, 68, [40]))
    n = fr.Normalizer.fit(ds, "maxmin")
    assert n.feature_stats()[1]["max"] == float(np.float32(3e38)) and n.feature_stats()[1]["min"] == -float(np.float32(3e38))
    with pytest.raises(Exception) as exc:
        n.apply(ds)
    assert "Normalization.maxmin NaN: feature 1, instance 7" in str(exc.value)   # (3e38 - -3e38) / inf
    with pytest.raises(Exception) as exc:
        fr.Normalizer.per_query("maxmin").apply(ds)
    assert "Normalization.maxmin NaN: feature 1, instance 7" in str(exc.value)
    z = fr.Normalizer.fit(ds, "zscore").apply(ds)  # zscore of the same column is finite
    assert np.isfinite(native.loaded_arrays(z)["x"]).all()
    _still_works(ds, X)


def test_views_and_second_applications_are_refused():
    m = 500
    X = _matrix(m, 5, 69)
    ds, _ = _dataset(X, _qids(m, 70))
    n = fr.Normalizer.fit(ds, "zscore")
    names = list(ds.instances_by_query())
    for view in (ds.subsample_queries(names[:3]), ds.subsample_feature_names(["0", "1"])):
        for norm in (n, fr.Normalizer.per_query("zscore"), fr.Normalizer.sigmoid()):
            with pytest.raises(Exception, match="normalise the whole dataset, then sample it"):
                norm.apply(view)
    once = n.apply(ds)
    for norm in (n, fr.Normalizer.per_query("maxmin"), fr.Normalizer.sigmoid()):
        with pytest.raises(Exception, match="Cannot apply normalization twice!"):
            norm.apply(once)
    # statistics of the normalised dataset, and a sample of it, are ordinary calls
    want = nm.apply(X, _all_held(X), nm.fit(X, _all_held(X), np.arange(m), range(5)), "zscore")
    assert _hexes(once.feature_stats()) == _hexes(nm.fit(want, _all_held(X), np.arange(m), range(5)))
    assert once.subsample_queries(names[:2]).normalization() == n.to_dict()
    _still_works(ds, X)


# -----------------------------------------------------------------------------------------------------------------------
# end to end
# -----------------------------------------------------------------------------------------------------------------------
def _tables(ds):
    f = native.device_form(ds)
    return {k: (v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in f.items()}


def test_training_on_a_normalised_dataset(wide):
    ds, X, y, qid = wide
    before = _tables(ds)
    H = _all_held(X)
    names = list(ds.instances_by_query())
    train_view = ds.subsample_queries(names[::2])
    order = [i for ids in train_view.instances_by_query().values() for i in ids]
    n = fr.Normalizer.fit(train_view, "zscore")
    normed = n.apply(ds)
    after = _tables(ds)
    assert before.keys() == after.keys() and all(before[k] == after[k] for k in before), "the source dataset's device tables moved"
    want = nm.apply(X, H, nm.fit(X, H, order, range(X.shape[1])), "zscore")
    twin = fr.CDataset.from_numpy(want, y, qid)
    ca = fr.TrainRequest.coordinate_ascent()
    ca.params.quiet, ca.params.num_restarts, ca.params.num_max_iterations, ca.params.seed = True, 2, 3, 42
    lm = fr.TrainRequest.lambdamart()
    lm.params.quiet, lm.params.grower, lm.params.num_trees = True, "histogram", 10
    for req in (ca, lm):
        a, b = normed.train_model(req).to_dict(), twin.train_model(req).to_dict()
        assert a == b
    half = normed.subsample_queries(names[1::2])
    assert half.train_model(lm).to_dict() == twin.subsample_queries(names[1::2]).train_model(lm).to_dict()
