"""The device text parser against the host parser ("Text loading"): for every case the dataset loaded under
parser="device" equals the one under parser="host" field for field (x as bytes, so -0.0 counts), every error has the host's
text, and the lines handed back are the ones the Python restatement (tests/ranksvm_text_cases.py) says."""
import gzip
import json
import os

import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import native
from tests import ranksvm_text_cases as tc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_TRAIN = os.path.join(ROOT, "tests", "golden", "data", "trec_news_2018.train")


def _consts():
    st = native.last_load_stats()
    return st["scan_slice"], st["stage_limit"]


def _load(path, parser):
    arrays = native.loaded_arrays(fr.CDataset.open_ranksvm(path, parser=parser))
    return arrays, native.last_load_stats()


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
            assert np.array_equal(a[k].view(np.uint8).reshape(-1), b[k].view(np.uint8).reshape(-1)), k
        else:
            assert a[k] == b[k], k


def _both(tmp_path, text: bytes, name="case.txt"):
    """Writes `text`, loads it under both parsers, holds the arrays equal and the handed-back lines to the restatement."""
    path = str(tmp_path / name)
    with open(path, "wb") as fh:
        fh.write(text)
    host, hs = _load(path, "host")
    dev, ds = _load(path, "device")
    assert hs["parser"] == "host" and ds["parser"] == "device", (hs, ds)
    _same(host, dev)
    reasons = tc.text_reasons(text, ds["stage_limit"])
    want = {r: reasons.count(r) for r in tc.REASONS[1:]}
    assert ds["lines"] == len(reasons) == hs["lines"] and ds["host_line_reasons"] == want and ds["host_lines"] == sum(want.values()), (ds, want)
    return dev, ds


def _error(path, parser):
    with pytest.raises(Exception) as e:
        fr.CDataset.open_ranksvm(path, parser=parser)
    return str(e.value)


@pytest.mark.parametrize("gz", [False, True])
def test_golden_file(tmp_path, gz):
    path = GOLDEN_TRAIN
    if gz:
        path = str(tmp_path / "train.gz")
        with gzip.open(path, "wb") as fh:
            fh.write(open(GOLDEN_TRAIN, "rb").read())
    host, _ = _load(path, "host")
    dev, ds = _load(path, "device")
    _same(host, dev)
    assert ds["parser"] == "device" and ds["lines"] == 782 and ds["host_lines"] == 0


@pytest.fixture(scope="module")
def mslr(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("mslr") / "mslr.txt")
    text = tc.mslr_like(np.random.default_rng(5), 20000)
    with open(path, "wb") as fh:
        fh.write(text)
    return path, text


def test_mslr_like_file_spans_many_slices_and_workgroups(mslr):
    path, text = mslr
    host, _ = _load(path, "host")
    dev, ds = _load(path, "device")
    _same(host, dev)
    assert ds["parser"] == "device" and ds["lines"] == 20000 and ds["host_lines"] == 0 and ds["bytes"] == len(text) > 1000 * ds["scan_slice"]
    assert dev["x"].shape == (20000, 137) and dev["present_words"] == 0
    # under the threshold "auto" is the host parser
    fr.CDataset.open_ranksvm(path)
    st = native.last_load_stats()
    assert len(text) < st["auto_threshold"] and st["parser"] == "host"


def test_device_loaded_dataset_trains_and_uploads_like_its_host_twin(mslr):
    path, _ = mslr
    req = fr.TrainRequest.lambdamart()
    req.measure = "ndcg@10"
    req.params.num_trees, req.params.quiet, req.params.grower = 2, True, "histogram"
    models, forms = [], []
    for parser in ("host", "device"):
        ds = fr.CDataset.open_ranksvm(path, parser=parser)
        assert native.last_load_stats()["parser"] == parser
        models.append(json.dumps(ds.train_model(req).to_dict(), sort_keys=True))
        forms.append(native.device_form(ds))
    assert models[0] == models[1]
    assert forms[0].keys() == forms[1].keys()
    for k, v in forms[0].items():
        w = forms[1][k]
        if k == "colstats":     # (the column sums are added in any order: two builds of ONE matrix may differ in their last bits,
            for field in ("mn", "mx", "at_min", "at_max"):   # tests/test_gpu_device_form.py; colstd is made from those sums)
                assert v[field].tobytes() == w[field].tobytes(), field
        elif k == "colstd":
            # n = 20 000 terms in any order: each sum within (n - 1) 2^-53 of sum|terms|, and the variance of values spread over
            # 0 .. 5000 loses about two bits to the subtraction of the squared mean: 2e4 * 1.1e-16 * 4 < 1e-10
            assert np.allclose(v, w, rtol=1e-10, atol=0)
        elif isinstance(v, np.ndarray):
            assert w is not None and v.tobytes() == w.tobytes(), k
        elif not k.endswith("_addr"):   # (addresses are the buffers' own)
            assert v == w, k


def test_lines_straddling_a_scan_slice_boundary(tmp_path):
    slice_bytes, _ = _consts()
    text, starts = b"", []
    for off in range(64):
        # a filler line ends so that the next line starts on byte `off` of some slice's last 64 and runs on into the next slice
        boundary = (len(text) + 200 + slice_bytes - 1) // slice_bytes * slice_bytes
        head = b"1 qid:%d 1:0.25 2:7 3:1e-3 # pad" % off
        text += head + b"x" * (boundary - 64 + off - len(text) - len(head) - 1) + b"\n"
        starts.append(len(text))
        text += b"0 qid:%d 2:5.5 5:1 7:0.125 9:%d 11:2.5e-2 13:77 15:0.001 # straddles the boundary at offset %d\n" % (off, off, off)
        assert starts[-1] == boundary - 64 + off and len(text) > boundary + 8
    dev, ds = _both(tmp_path, text)
    assert ds["host_lines"] == 0 and dev["n"] == 128 and [s % slice_bytes for s in starts] == list(range(slice_bytes - 64, slice_bytes))


@pytest.mark.parametrize("name,text", [
    ("one_line", b"1 qid:1 1:0.5 2:3\n"),
    ("no_final_newline", b"1 qid:1 1:0.5 2:3\n0 qid:1 1:1.5 2:4"),
    ("crlf", b"1 qid:1 1:0.5 2:3 # a\r\n0 qid:2 1:1.5 2:4\r\n"),
    ("tabs_and_blank_runs", b"1\tqid:1 \t 1:0.5\v\f2:3   #  doc one \t\n0    qid:1\t\t1:1.5 2:4 #\tdoc\ttwo\n"),
    ("leading_blanks", b"   1 qid:1 1:0.5 2:3\n\t0 qid:1 1:1.5 2:4\n"),
    ("feature_zero", b"1 qid:1 0:0.5\n0 qid:1 0:2 1:3\n"),
    ("descending_fids", b"1 qid:1 3:0.5 2:3 1:7\n0 qid:1 1:1.5 2:4 3:1\n"),
    ("comments", "1 qid:1 1:1 2:2 #\n0 qid:1 1:3 2:4 # déjà 文\n2 qid:2 1:5 2:6 #x#y # z\n1 qid:2 1:7 2:8\n".encode("utf-8") + b"0 qid:2 1:9 2:1 # \xff\xfe\n"),
    ("dense_after_sparse", b"1 qid:1 7:1 100:2\n0 qid:1 1:1 2:2 3:3\n1 qid:1 50:1 51:2 100:3\n"),
    ("density_half", b"1 qid:1 2:1 4:5\n0 qid:1 2:1 5:5\n1 qid:1 1:1 2:1 3:1 6:2\n0 qid:1 1:1 2:1 3:1 7:2\n1 qid:1 7:7\n"),
    ("big_fid_small_matrix", b"1 qid:1 5:1\n0 qid:1 999999:2\n"),
])
def test_small_texts(tmp_path, name, text):
    _both(tmp_path, text, name + ".txt")


def test_largest_fast_feature_id(tmp_path):
    """fid 999 999 999 (the 9-digit limit of the fast grammar) in a two-line file of one feature each: d = 10^9."""
    dev, ds = _both(tmp_path, b"1 qid:1 999999999:2.5\n0 qid:2 7:1\n")
    assert dev["d"] == 1000000000 and ds["host_lines"] == 0 and dev["features"].tolist() == [7, 999999999]


def test_a_line_of_the_staging_limit_and_one_byte_more(tmp_path):
    _, limit = _consts()
    head = b"1 qid:1 1:0.5 2:3 #"
    exact, longer = head + b"d" * (limit - len(head)), head + b"d" * (limit + 1 - len(head))
    text = exact + b"\n" + longer + b"\n0 qid:1 1:1 2:2\n"
    dev, ds = _both(tmp_path, text)
    assert ds["host_line_reasons"]["too_long"] == 1 and ds["host_lines"] == 1


@pytest.mark.parametrize("feats", [1, 63, 64, 65, 257, 1000])
def test_feature_counts(tmp_path, feats):
    rng = np.random.default_rng(feats)
    rows = ["%d qid:%d %s # r%d" % (i % 3, i // 2, " ".join("%d:%.6g" % (j + 1, rng.uniform(-5, 5)) for j in range(feats)), i) for i in range(5)]
    dev, ds = _both(tmp_path, ("\n".join(rows) + "\n").encode())
    assert ds["host_lines"] == 0 and dev["d"] == feats + 1


@pytest.mark.parametrize("d", [32, 33, 64, 65])
def test_presence_words(tmp_path, d):
    rows = ["1 qid:1 " + " ".join("%d:%d" % (j, j + 1) for j in range(d)),          # dense, every feature
            "0 qid:1 %d:1" % (d - 1),                                                # sparse, the last bit of the last word
            "2 qid:1 0:1 %d:3" % (d - 2),
            "1 qid:2 " + " ".join("%d:0.5" % j for j in range(0, d - 1))]            # dense, one short
    dev, ds = _both(tmp_path, ("\n".join(rows) + "\n").encode())
    assert dev["d"] == d and dev["present_words"] == (d + 31) // 32 and ds["host_lines"] == 0


def test_values_that_are_handed_back(tmp_path):
    rng = np.random.default_rng(11)
    values = tc.EDGE_VALUES + tc.exact_midpoints(rng, 9, 4) + tc.exact_midpoints(rng, 17, 4)
    ok = [v for v in values if v not in ("1e", ".", "-", "1.2.3", "0e99")]            # (those are errors: below)
    rows = ["1 qid:%d 1:1 2:%s 3:0.5" % (i, v) for i, v in enumerate(ok)] + ["%s qid:x 1:1 2:2" % v for v in ok if v not in ("nan",)]
    dev, ds = _both(tmp_path, ("\n".join(rows) + "\n").encode())
    r = ds["host_line_reasons"]
    assert r["near_tie"] >= 2 * 9 and r["range"] >= 2 * 2 and r["number"] >= 2 * 5 and 0 < ds["host_lines"] < len(rows)
    assert np.signbit(dev["x"][ok.index("-0"), 2]) and dev["x"][ok.index("+1"), 2] == 1 and dev["x"][ok.index("1e5"), 2] == 1e5


def test_a_mixed_file_flags_the_intended_share(tmp_path):
    rng = np.random.default_rng(3)
    toks = tc.random_tokens(rng, 7 * 600)
    rows = []
    for i in range(600):
        vals = toks[7 * i: 7 * i + 7]
        rows.append("%d qid:%d %s # d%d" % (i % 4, i // 20, " ".join("%d:%s" % (3 * j + 1, v) for j, v in enumerate(vals)), i))
    rows[17] = "2 qid:0 5:1 3:2"
    rows[99] = "2 qid:qid:4 5:1"
    text = ("\n".join(rows) + "\n").encode()
    dev, ds = _both(tmp_path, text)   # (the count per reason is the restatement's)
    assert 0 < ds["host_lines"] < 600 and ds["host_line_reasons"]["unsorted"] >= 1 and ds["host_line_reasons"]["grammar"] >= 1


GOOD = ["1 qid:1 1:1 2:2", "0 qid:1 1:3 2:4 # c"]
FLAGGED_VALID = ["1 qid:1 2:16777217 1:5", "0 qid:2 1:inf 2:1e39"]
BAD = {
    "EmptyLine": "  \t ",
    "Label": "x1 qid:1 1:1",
    "LabelIsNan": "nan qid:1 1:1",
    "FeatureNoColon": "1 qid:1 1:1 22",
    "FeatureNum": "1 qid:1 a:1",
    "FeatureValNotFloat": "1 qid:1 1:1e",
    "NoFeatures": "1 qid:1 # only a comment",
    "MultipleDefinitions": "1 qid:1 3:1 2:1 3:2",
    "Missing qid": "1 1:1 2:2",
}


@pytest.mark.parametrize("kind", sorted(BAD))
def test_errors_have_the_host_parsers_text(tmp_path, kind):
    other = BAD["FeatureNum" if kind != "FeatureNum" else "Label"]
    layouts = {"first": [BAD[kind]] + GOOD, "last": GOOD + [BAD[kind]], "after_flagged": GOOD + FLAGGED_VALID + GOOD + [BAD[kind]] + GOOD,
               "twice": GOOD + [BAD[kind]] + FLAGGED_VALID + [other] + GOOD, "second": GOOD + [other] + [BAD[kind]]}
    for name, rows in layouts.items():
        for ending in ("\n", ""):
            path = str(tmp_path / (name + ("_nl" if ending else "") + ".txt"))
            with open(path, "w") as fh:
                fh.write("\n".join(rows) + ending)
            host, dev = _error(path, "host"), _error(path, "device")
            assert host == dev, (name, host, dev)
            if name != "second":
                assert kind in host, (name, host)


def test_empty_and_missing_files(tmp_path):
    empty = str(tmp_path / "empty.txt")
    open(empty, "w").close()
    assert _error(empty, "host") == _error(empty, "device") and "No features defined!" in _error(empty, "device")
    missing = str(tmp_path / "none.txt")
    assert _error(missing, "host") == _error(missing, "device") and "Os { code" in _error(missing, "device")
    nul = str(tmp_path / "nul.txt")
    with open(nul, "wb") as fh:
        fh.write(b"1 qid:1 1:1 2:2\n0 qid:1 1:3\x00 2:4\n")
    try:
        host = native.loaded_arrays(fr.CDataset.open_ranksvm(nul, parser="host"))
    except Exception as e:   # whatever the host parser makes of a NUL byte, the device path gives the same: it hands the text over whole
        assert str(e) == _error(nul, "device")
    else:
        _same(host, native.loaded_arrays(fr.CDataset.open_ranksvm(nul, parser="device")))
        assert native.last_load_stats()["parser"] == "host" and "NUL" in native.last_load_stats()["reason"]
