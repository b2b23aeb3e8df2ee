"""The random-forest trainer's level step on the device (csrc/rf_train.hpp, train_rf.inc, kernels_rf.inc) against
tests/rf_level_model.py, which tests/test_rf_level_host.py anchors to the oracle: native.rf_levels grows one batch with the
trainer's own grow_batch and records every level, and every array of the record -- the sorted arrays, every candidate's
position, ids_i, flags, importance, sums and positive counts, the splits, the children's outputs, the root outputs, the trees
-- must equal the restatement's bit for bit (label_minmax by value: fminf / fmaxf leave the sign of a zero open).  Every case
sits on a limit of a kernel, says so from its capture, and runs under the default switches and under each switch that selects
another kernel (FR_RF_PARTITION=0, FR_RF_INT_SUMS=0, FR_RF_CHILDSUM=1, FR_RF_RESORT=1), whose captures must equal the
default's.  No tolerance anywhere.

Sums of f32 labels in f64 are exact while the labels' exponents lie within 29 bits of each other, in any order; the "wide"
labels here span 35, so a wrong order of a sum or of a sort shows in its last bits."""
import numpy as np
import pytest

import fastrank_amd as fr
from fastrank_amd import native
from oracle import pyoracle as o
from tests import rf_level_model as lm
from tests.conftest import ranksvm_presence

pytestmark = pytest.mark.gpu

RF_CHUNK, RF_PT = 512, 2048  # kernels_rf.inc
SWITCHES = ({"FR_RF_PARTITION": "0"}, {"FR_RF_INT_SUMS": "0"}, {"FR_RF_CHILDSUM": "1"}, {"FR_RF_RESORT": "1"})


def wide(rng, n):
    """f32 labels of either sign with exponents from 2^-20 to 2^14."""
    return (rng.choice([-1.0, 1.0], n) * np.ldexp(1.0 + rng.random(n), rng.integers(-20, 15, n))).astype(np.float32).astype(np.float64)


def small_int(rng, n):
    return rng.choice(5, size=n, p=[0.4, 0.3, 0.15, 0.1, 0.05]).astype(np.float64)


def dataset(X, y, per_query=40):
    qid = (np.arange(len(y)) // per_query + 1).astype(np.int64)
    return fr.CDataset.from_numpy(np.ascontiguousarray(X, dtype=np.float32), np.ascontiguousarray(y, dtype=np.float64), qid)


def check(monkeypatch, ds, X, y, roots, feats, k, method, min_leaf, max_depth, present=None):
    """The hook against the restatement, then every switch against the default capture.  Returns the default capture."""
    roots = [np.asarray(r, dtype=np.int64) for r in roots]
    off = np.concatenate(([0], np.cumsum([len(r) for r in roots])))
    ids = np.concatenate(roots)
    want = lm.grow(X, present, y, roots, feats, k, method, min_leaf, max_depth)
    got = native.rf_levels(ds, off, ids, feats, k, method, min_leaf, max_depth)
    d = lm.diff(got, want)
    assert d is None, d
    for lv in got["levels"]:
        assert lv["children_from"] == ("candidates" if method == 0 else "rf_childsum_kernel")
    for env in SWITCHES:
        with monkeypatch.context() as m:
            for name, value in env.items():
                m.setenv(name, value)
            other = native.rf_levels(ds, off, ids, feats, k, method, min_leaf, max_depth)
        d = lm.diff(other, got)
        assert d is None, (env, d)
        if "FR_RF_CHILDSUM" in env:
            assert all(lv["children_from"] == "rf_childsum_kernel" for lv in other["levels"])
    return got


def evaluated(cap, fslot=0, level=0):
    """(n, ids_i) of every evaluated candidate of one feature slot of one level."""
    lv = cap["levels"][level]
    out = set()
    for a in range(len(lv["active"])):
        for c in lv["cands"][a, fslot]:
            if c["flags"] & 1:
                out.add((int(lv["active"][a]["n"]), int(c["ids_i"])))
    return out


def segment(lv, a, fi, nf, name):
    """One (node, feature slot) segment of a level's sorted arrays."""
    ns = lv["active"]["n"].astype(np.int64)
    start = int((ns[:a] * nf).sum()) + fi * int(ns[a])
    return lv[name][start:start + int(ns[a])]


def blocks(pairs, rng, label_fn):
    """One tree per (n, nl) over rows of its own: feature 0 holds nl zeros and n - nl ones (k = 2 puts the split at nl exactly),
    feature 1 a shuffled arange(n) (k = 8 gives the lanes different splits in one segment).  The rows are shuffled."""
    Xs, roots, start = [], [], 0
    for n, nl in pairs:
        a = np.zeros(n)
        a[nl:] = 1.0
        Xs.append(np.stack([rng.permutation(a), rng.permutation(n).astype(np.float64)], axis=1))
        roots.append(rng.permutation(n) + start)
        start += n
    X = np.concatenate(Xs).astype(np.float32)
    return X, label_fn(rng, len(X)), roots


def pairs_of(ns, nls):
    out = []
    for n in ns:
        for nl in sorted(set(x if x != "n-1" else n - 1 for x in nls)):
            if 1 <= nl < n:
                out.append((n, nl))
    return out


CHUNK_NS = (2, 15, 16, 17, 63, 64, 65, 511, 512, 513, 527, 528, 1023, 1024, 1025, 1040)
CHUNK_NLS = (1, 15, 16, 17, 511, 512, 513, "n-1")


@pytest.fixture(scope="module")
def chunk_data():
    out = {}
    for kind, fn in (("int", small_int), ("wide", wide)):
        X, y, roots = blocks(pairs_of(CHUNK_NS, CHUNK_NLS), np.random.default_rng(11), fn)
        out[kind] = (dataset(X, y), X, y, roots)
    return out


@pytest.mark.parametrize("labels", ["int", "wide"])
@pytest.mark.parametrize("method", [0, 1, 2, 3])
def test_chunk_and_chain_boundaries(chunk_data, method, labels, monkeypatch):
    """RF_CHUNK = 512 and the 16-wide chain of rf_eval_kernel and rf_childsum_kernel: node sizes and split positions on, one
    below and one above them; integer labels take the integer sums (and the chain under FR_RF_INT_SUMS=0), wide labels the chain."""
    ds, X, y, roots = chunk_data[labels]
    pairs = pairs_of(CHUNK_NS, CHUNK_NLS)
    feats = [[0, 1]] * len(roots)
    ml = 2 if method == 3 else 1
    cap = check(monkeypatch, ds, X, y, roots, feats, 2, method, ml, 2)
    want = {(n, nl) for n, nl in pairs if nl >= ml and n - nl >= ml}
    assert want <= evaluated(cap, 0), "every (n, nl) is an evaluated candidate of the two-valued column"
    assert {nl for _, nl in want} >= {15, 16, 17, 511, 512, 513} and {n for n, _ in want} >= set(CHUNK_NS[4:])
    pos = {(int(a["n"]), int(s["pos"])) for a, s in zip(cap["levels"][0]["active"], cap["levels"][0]["splits"]) if s["fslot"] >= 0}
    assert len(pos & {(n, nl) for n, nl in want if nl in (511, 512, 513)}) > 0, "a child sum is cut on, below and above a chunk"
    # k = 8 on the shuffled arange: in one segment some lanes' splits fall inside a chunk and others do not
    cap8 = check(monkeypatch, ds, X, y, roots, feats, 8, method, ml, 2)
    lv = cap8["levels"][0]
    mixed = chained = 0
    for a in range(len(lv["active"])):
        n = int(lv["active"][a]["n"])
        cd = lv["cands"][a, 1]
        nls = cd["ids_i"].astype(np.int64)  # (every lane's position steers the block, evaluated or not)
        if not (cd["flags"] & 1).any():
            continue
        for base in range(0, n, RF_CHUNK):
            inside = (nls > base) & (nls < min(base + RF_CHUNK, n))
            mixed += bool(inside.any() and not inside.all())
            chained += bool(not inside.any())
    assert mixed > 0 and chained > 0, "a straddled chunk with lanes on both paths, and a chunk no lane's split falls into"


def test_integer_sum_path_limits(monkeypatch):
    """Labels of magnitude 2^21 exactly take the integer sums, one label of 2^21 + 1 sends the dataset to the chain; negative
    integers and -0.0 labels; a node whose labels are -0.0 and +0.0 only has label_min == label_max and stays a leaf."""
    rng = np.random.default_rng(5)
    pairs = [(700, 300), (513, 512), (64, 1)]
    for top in (2.0 ** 21, 2.0 ** 21 + 1.0):
        X, _, roots = blocks(pairs + [(40, 20)], rng, small_int)
        y = rng.choice([-top, -3.0, -1.0, -0.0, 0.0, 2.0, top], size=len(X))
        zeros = roots[-1]
        y[zeros] = np.where(rng.random(len(zeros)) < 0.5, -0.0, 0.0)
        ds = dataset(X, y)
        cap = check(monkeypatch, ds, X, y, roots, [[0, 1]] * len(roots), 4, 0, 1, 3)
        sg = np.concatenate([lv["sg"] for lv in cap["levels"]])
        assert np.abs(sg).max() == top and (sg == np.round(sg)).all() and (sg < 0).any()
        assert np.signbit(sg[sg == 0]).any() and not np.signbit(sg[sg == 0]).all()
        lv = cap["levels"][0]
        a = [i for i in range(len(lv["active"])) if lv["active"][i]["tree"] == len(roots) - 1][0]
        z = segment(lv, a, 0, 2, "sg")
        assert (z == 0).all() and np.signbit(z).any() and not np.signbit(z).all()
        assert lv["label_minmax"][a, 0] == lv["label_minmax"][a, 1] and lv["splits"][a]["fslot"] == -1
        assert cap["trees"][-1] == {"LeafNode": 0.0} and len(cap["root_out"]) == len(roots)
        assert len(cap["levels"]) == 2 and (cap["levels"][0]["splits"]["fslot"][:3] >= 0).all()


@pytest.mark.parametrize("method", [1, 2])
def test_positive_count_masks(method, monkeypatch):
    """The 64-lane ballots of the Gini / entropy count: splits at 63, 64, 65 and 128 in nodes of 64, 65 and 129 instances."""
    rng = np.random.default_rng(3)
    pairs = pairs_of((64, 65, 129), (63, 64, 65, 128))
    X, y, roots = blocks(pairs, rng, small_int)
    cap = check(monkeypatch, dataset(X, y), X, y, roots, [[0, 1]] * len(roots), 2, method, 1, 2)
    assert set(pairs) <= evaluated(cap, 0) and set(pairs) == {(64, 63), (65, 63), (65, 64), (129, 63), (129, 64), (129, 65), (129, 128)}
    cd = cap["levels"][0]["cands"][:, 0, 0]
    assert (cd["pos_l"] > 0).any() and (cd["pos_r"] > 0).any() and (cd["importance"] == 0).all()


@pytest.mark.parametrize("method", [0, 1, 3])
def test_candidate_blocks(method, monkeypatch):
    """rf_eval_kernel's loop over blocks of 64 candidates: k - 1 = 63, 64, 65, 128 and 129 on real-valued columns; a two-valued
    column at k = 130, whose second and third block have no evaluated lane; a column whose best split is candidate 100 of 129."""
    rng = np.random.default_rng(17)
    n = 600
    steps = rng.permutation(n).astype(np.float64)
    X = np.stack([rng.random(n), -7.0 * rng.random(n), rng.permutation(np.repeat([0.0, 1.0], n // 2)), steps], axis=1).astype(np.float32)
    X64 = X.astype(np.float64)
    y = wide(rng, n) if method == 0 else small_int(rng, n)
    ml = 2 if method == 3 else 1
    ds = dataset(X, y)
    roots = [rng.permutation(n)]
    for k in (64, 65, 66, 129, 130):
        cap = check(monkeypatch, ds, X, y, roots, [[0, 1]], k, method, ml, 2)
        cd = cap["levels"][0]["cands"][0]
        last = 64 * ((k - 2) // 64)  # the first candidate of the last block
        assert cd.shape == (2, k - 1) and (cd["flags"][:, last:] & 1).any(axis=1).all(), "the last block holds an evaluated candidate"
        assert (cd["flags"][:, :64] & 1).sum() > 60
    cap = check(monkeypatch, ds, X, y, roots, [[2, 0]], 130, method, ml, 2)
    two = cap["levels"][0]["cands"][0, 0]
    assert (two["flags"][:64] & 1).sum() == 1 and not (two["flags"][64:] & 1).any() and (two["ids_i"] == n // 2).all()
    assert not two["sum_l"][1:].any() and not two["importance"][1:].any()
    # labels that step where candidate 100 of 129 cuts the shuffled arange: no other candidate separates them
    cut = (100.0 / 130.0) * (X64[:, 3].max() - X64[:, 3].min()) + X64[:, 3].min()
    ystep = np.where(X64[:, 3] < cut, 0.0, 3.0)
    cap = check(monkeypatch, dataset(X, ystep), X, ystep, roots, [[3]], 130, method, ml, 2)
    lv = cap["levels"][0]
    assert lv["splits"][0]["fslot"] == 0 and lv["splits"][0]["pos"] == lv["cands"][0, 0, 99]["ids_i"] and lv["cands"][0, 0, 99]["flags"] & 1
    assert cap["trees"][0]["FeatureSplit"]["split"] == cut, "a second candidate block holds the winner"
    assert len({int(c["ids_i"]) for c in lv["cands"][0, 0]}) > 100


def test_min_leaf_support_on_and_below(monkeypatch):
    """A side of exactly min_leaf_support instances is evaluated, one of one fewer is not -- on either side."""
    rng = np.random.default_rng(2)
    pairs = [(30, 10), (30, 9), (30, 20), (30, 21), (20, 10), (19, 10), (19, 9)]
    X, y, roots = blocks(pairs, rng, wide)
    cap = check(monkeypatch, dataset(X, y), X, y, roots, [[0, 1]] * len(roots), 2, 0, 10, 2)
    assert evaluated(cap, 0) == {(30, 10), (30, 20), (20, 10)}
    ids = {(int(a["n"]), int(c["ids_i"])) for a, c in zip(cap["levels"][0]["active"], cap["levels"][0]["cands"][:, 0, 0])}
    assert ids == set(pairs), "the others were placed and refused"


def test_label_kernel_block_sizes(monkeypatch):
    """rf_label_kernel's 1 024 threads and 64-lane waves: nodes of 63 .. 2 049 instances whose largest (or smallest) label is the
    last of the segment the kernel reads, so only the last thread's last trip sees it.  (A node of one instance is never
    active -- a split needs two -- so the tree of one instance here is the batch's leaf beside them.)"""
    rng = np.random.default_rng(9)
    sizes = (1, 63, 64, 65, 1023, 1024, 1025, 2049)
    Xs, ys, roots, start = [], [], [], 0
    for i, n in enumerate(sizes):
        col = rng.permutation(n).astype(np.float64)
        lab = small_int(rng, n)
        lab[np.argmax(col)] = 9.0 if i % 2 else -9.0
        Xs.append(col[:, None]), ys.append(lab), roots.append(rng.permutation(n) + start)
        start += n
    X, y = np.concatenate(Xs).astype(np.float32), np.concatenate(ys)
    cap = check(monkeypatch, dataset(X, y), X, y, roots, [[0]] * len(sizes), 3, 1, 1, 2)
    lv = cap["levels"][0]
    assert [int(x) for x in lv["active"]["n"]] == list(sizes[1:]) and cap["trees"][0] == {"LeafNode": float(np.float32(y[0]))}
    for a in range(len(lv["active"])):
        sg = segment(lv, a, 0, 1, "sg")
        assert abs(sg[-1]) == 9.0 and (np.abs(sg[:-1]) < 9.0).all()
        assert lv["label_minmax"][a, 1 if sg[-1] > 0 else 0] == sg[-1]


def partition_case(rng, method):
    """Trees whose root splits at a chosen position (a two-valued column the labels follow), then grow on two more columns."""
    pairs = pairs_of((2047, 2048, 2049, 4097), (1, 255, 256, 257, 2047, 2048)) + [(2, 1), (300, 150)]
    Xs, ys, roots, start = [], [], [], 0
    for n, nl in pairs:
        a = np.zeros(n)
        a[nl:] = 1.0
        a = rng.permutation(a)
        b = rng.permutation(n).astype(np.float64)
        c = np.floor(rng.exponential(2.0, n))
        if method == 0:
            lab = wide(rng, n) + a * 2.0 ** 22
        else:
            lab = a * small_int(rng, n).clip(1)  # (Gini: the two-valued column alone separates the positive labels)
        if n == 300 and method == 0:
            lab[a == 0] = 1.0
        # (the left child's labels are all equal, here and under Gini everywhere: it stays a leaf beside a sibling that splits)
        Xs.append(np.stack([a, b, c], axis=1)), ys.append(lab), roots.append(rng.permutation(n) + start)
        start += n
    return pairs, np.concatenate(Xs).astype(np.float32), np.concatenate(ys).astype(np.float32).astype(np.float64), roots


@pytest.mark.parametrize("method", [0, 1])
def test_partition_tiles(method, monkeypatch):
    """rf_part_count / rf_part_scan / rf_part_scatter against the definition (and against rekey + radix sort under
    FR_RF_PARTITION=0): parents of RF_PT - 1, RF_PT, RF_PT + 1 and 2 RF_PT + 1 instances cut at 1, 255 .. 257, 2 047 and 2 048,
    three feature slots, trees of different sizes in one batch, four levels."""
    pairs, X, y, roots = partition_case(np.random.default_rng(23), method)
    cap = check(monkeypatch, dataset(X, y), X, y, roots, [[0, 1, 2]] * len(roots), 2, method, 1, 5)
    assert len(cap["levels"]) == 4, "every ping-pong buffer is swapped twice"
    l0 = cap["levels"][0]
    cut = {(int(a["n"]), int(s["pos"])) for a, s in zip(l0["active"], l0["splits"]) if s["fslot"] >= 0}
    assert cut == set(pairs), "every root is cut where its two-valued column says"
    one_open = both_closed = leaf_beside = 0
    for i, lv in enumerate(cap["levels"][:-1]):
        keys = set(int(x) for x in cap["levels"][i + 1]["active"]["key"])
        kids = [((int(s["left"]) in keys), (int(s["right"]) in keys)) for s in lv["splits"] if s["fslot"] >= 0]
        one_open += sum(1 for l, r in kids if l != r)
        both_closed += sum(1 for l, r in kids if not l and not r)
        assert len(lv["active"]) >= 3 and len(set(int(t) for t in lv["active"]["tree"])) >= 2
        if i > 0:
            leaf_beside += int((lv["splits"]["fslot"] < 0).any() and (lv["splits"]["fslot"] >= 0).any())
    assert one_open > 0 and both_closed > 0 and leaf_beside > 0
    assert max(int(n) for n in l0["active"]["n"]) > 2 * RF_PT


@pytest.mark.parametrize("method", [0, 1])
def test_scan_carry_beyond_64_tiles(method, monkeypatch):
    """rf_part_scan_kernel's carry: segments of 65 and of 129 tiles (131 073 and 2 x 131 072 + 5 instances) are partitioned
    into children that are both open."""
    rng = np.random.default_rng(31)
    sizes = (64 * RF_PT + 1, 2 * 64 * RF_PT + 5)
    n = sum(sizes)
    X = np.stack([rng.random(n), np.floor(rng.exponential(3.0, n))], axis=1).astype(np.float32)
    y = small_int(rng, n)
    y = np.where(X[:, 0] > 0.55, np.minimum(y + 1.0, 4.0), y)
    perm = rng.permutation(n)
    roots = [perm[:sizes[0]], perm[sizes[0]:]]
    cap = check(monkeypatch, dataset(X, y, per_query=100), X, y, roots, [[0, 1], [1, 0]], 3, method, 10, 3)
    l0, l1 = cap["levels"]
    tiles = [-(-int(x) // RF_PT) for x in l0["active"]["n"]]
    assert tiles == [65, 129] and (l0["splits"]["fslot"] >= 0).all(), "tiles per segment > 64"
    assert len(l1["active"]) == 4 and sorted(int(k) for k in l1["active"]["key"]) == [2, 3, 4, 5]
    # items beyond the 64th tile go to both children of both trees: the carry is what places them
    for a in range(2):
        nsz, pos = int(l0["active"][a]["n"]), int(l0["splits"][a]["pos"])
        assert 64 * RF_PT < nsz and 0 < pos < nsz
        for fi in range(2):
            if fi != int(l0["splits"][a]["fslot"]):
                went = np.isin(segment(l0, a, fi, 2, "svals")[64 * RF_PT:], segment(l0, a, int(l0["splits"][a]["fslot"]), 2, "svals")[:pos])
                assert len(went) == nsz - 64 * RF_PT and (a == 0 or (went.any() and not went.all()))


def test_batch_tables_and_views(monkeypatch):
    """Trees of 1, 255, 256 and 257 instances in one batch (the 256-thread grids of the per-instance kernels), instance lists
    that are neither sorted nor contiguous, and the same batch through a query-sampled and a feature-sampled view."""
    rng = np.random.default_rng(41)
    n = 1600
    X = np.stack([rng.random(n), np.floor(rng.exponential(2.0, n)), rng.normal(size=n), rng.permutation(n)], axis=1).astype(np.float32)
    y = wide(rng, n)
    ds = dataset(X, y, per_query=30)
    pool = rng.permutation(n)
    roots, at = [], 0
    for size in (1, 255, 256, 257):
        roots.append(pool[at:at + 2 * size:2])  # every other entry of a shuffled pool
        at += 2 * size
    assert all((np.diff(r) < 0).any() and (np.diff(np.sort(r)) > 1).any() for r in roots[1:])
    feats = [[0, 1], [2, 3], [3, 1], [0, 2]]
    cap = check(monkeypatch, ds, X, y, roots, feats, 8, 0, 2, 5)
    assert [int(x) for x in cap["levels"][0]["active"]["n"]] == [255, 256, 257] and len(cap["levels"]) == 4
    assert cap["trees"][0] == {"LeafNode": float(y[roots[0][0]])}
    # a query-sampled view: the instance ids stay the parent's, the device form is the view's own
    names = sorted(ds.queries(), key=int)
    keep = names[::2]
    view = ds.subsample_queries(keep)
    rows = np.nonzero(np.isin((np.arange(n) // 30 + 1), [int(q) for q in keep]))[0]
    vroots = [rng.permutation(rows)[:size] for size in (1, 255, 256)]
    vcap = check(monkeypatch, view, X, y, vroots, feats[:3], 8, 0, 2, 4)
    assert len(vcap["levels"]) == 3
    with pytest.raises(Exception, match="not in the view"):
        native.rf_levels(view, [0, 2], [int(rows[0]), int(np.setdiff1d(np.arange(n), rows)[0])], [[0, 1]], 3, 0, 1, 3)
    # a feature-sampled view: its own features only
    name_of = ds.feature_index_to_name()
    fview = ds.subsample_feature_names([name_of[1], name_of[3]])
    fcap = check(monkeypatch, fview, X, y, roots, [[3, 1]] * 4, 8, 0, 2, 5)
    assert len(fcap["levels"]) >= 3
    with pytest.raises(Exception, match="not in the view"):
        native.rf_levels(fview, [0, 2], [0, 1], [[0, 1]], 3, 0, 1, 3)


def test_presence_from_sparse_text(tmp_path, monkeypatch):
    """A dataset read with open_ranksvm from sparse text: nodes that hold 0, 1 and 2 values of a feature, and absent rows
    that sort (as 0.0) between the negative and the positive held values without entering the range."""
    rng = np.random.default_rng(13)
    n, d = 240, 9
    X = np.zeros((n, d), dtype=np.float32)
    y = small_int(rng, n)
    lines = []
    for i in range(n):
        held = {8: float(np.float32(rng.normal()))}
        if i % 2 == 0:
            held[1] = float(np.float32(rng.choice([-1.0, 1.0]) * (0.5 + rng.random())))
        if i in (3, 100, 101):
            held[2] = float(np.float32(1.0 + rng.random()))
        for f, v in held.items():
            X[i, f] = v
        lines.append("%d qid:%d %s" % (int(y[i]), i // 20 + 1, " ".join("%d:%r" % (f, held[f]) for f in sorted(held))))
    path = str(tmp_path / "sparse.train")
    open(path, "w").write("\n".join(lines) + "\n")
    present = ranksvm_presence(path, d)
    assert present[:, 8].all() and present[:, 1].sum() == n // 2 and present[:, 2].sum() == 3 and not present[:, 0].any()
    ds = fr.CDataset.open_ranksvm(path)
    assert ds.num_instances() == n and ds.num_features() == d
    roots = [np.concatenate(([100, 101], rng.permutation(np.arange(120, 200)))), np.concatenate(([3], rng.permutation(np.arange(20, 90)))),
             rng.permutation(np.arange(130, 230))]
    for method in (0, 3):
        cap = check(monkeypatch, ds, X, y, roots, [[2, 1, 8]] * 3, 4, method, 2, 4, present=present)
        lv = cap["levels"][0]
        held2 = [int((~np.signbit(segment(lv, a, 0, 3, "sv")) | (segment(lv, a, 0, 3, "sv") != 0)).sum()) for a in range(3)]
        assert held2 == [2, 1, 0], "nodes with two, one and no held value of feature 2"
        assert (lv["cands"][0, 0]["position"] >= 1.0).all() and not lv["cands"][1:, 0]["position"].any() and not lv["cands"][1:, 0]["flags"].any()
        for a in range(3):
            sv = segment(lv, a, 1, 3, "sv")
            absent = np.nonzero((sv == 0) & np.signbit(sv))[0]
            assert len(absent) and (sv[:absent[0]] < 0).all() and len(sv[:absent[0]]) and (sv[absent[-1] + 1:] > 0).all() and len(sv[absent[-1] + 1:])
            assert lv["cands"][a, 1]["position"].min() < 0 < lv["cands"][a, 1]["position"].max()
        assert len(cap["levels"]) >= 2


def test_roots_that_cannot_split(monkeypatch):
    """Constant columns under differing labels: no candidate, the root stays a leaf, and rf_rootsum_kernel takes the mean of
    the sample in LIST order -- 511, 512, 513 and 1 500 instances, wide labels, shuffled lists."""
    rng = np.random.default_rng(19)
    sizes = (511, 512, 513, 1500)
    n = sum(sizes)
    X = np.full((n, 2), 1.5, dtype=np.float32)
    y = wide(rng, n)
    pool = rng.permutation(n)
    roots = [pool[sum(sizes[:i]):sum(sizes[:i + 1])] for i in range(4)]
    cap = check(monkeypatch, dataset(X, y), X, y, roots, [[0, 1]] * 4, 3, 0, 1, 4)
    assert len(cap["levels"]) == 1 and (cap["levels"][0]["splits"]["fslot"] == -1).all() and not cap["levels"][0]["cands"]["flags"].any()
    assert len(cap["root_out"]) == 4 and cap["trees"] == [{"LeafNode": float(v)} for v in cap["root_out"]]
    y32 = y.astype(np.float32)
    assert any(lm.seq_sum(y32[np.sort(r)]) != lm.seq_sum(y32[r]) for r in roots), "the order of the list shows in the mean"


@pytest.mark.parametrize("min_leaf,column", [(1, "one_low"), (0, "constant")])
def test_the_two_error_cases(min_leaf, column, monkeypatch):
    """TrueVarianceReduction with a one-label side, and with min_leaf_support = 0 and an empty side: the reference panics,
    the oracle says so, the restatement raises and the trainer returns a plain error -- under every switch -- and goes on
    to grow the next batch."""
    rng = np.random.default_rng(4)
    n = 200
    X = np.full((n, 2), 2.0 if column == "constant" else 1.0, dtype=np.float32)
    if column == "one_low":
        X[17, :] = 0.0
    y = small_int(rng, n)
    qid = (np.arange(n) // 40 + 1).astype(np.int64)
    with pytest.raises(RuntimeError, match="error 2"):
        o.Dataset(X, y, qid).rf_learn("ndcg", dict(seed=1, num_trees=1, split_method="TrueVarianceReduction", instance_sampling_rate=1.0,
                                                   feature_sampling_rate=1.0, min_leaf_support=min_leaf, split_candidates=2, max_depth=3))
    with pytest.raises(lm.ReferencePanic):
        lm.grow(X, None, y, [np.arange(n)], [[0, 1]], 2, 3, min_leaf, 3)
    ds = dataset(X, y)
    for env in ({},) + SWITCHES:
        with monkeypatch.context() as m:
            for name, value in env.items():
                m.setenv(name, value)
            with pytest.raises(Exception, match="variance of fewer than two labels"):
                native.rf_levels(ds, [0, n], np.arange(n), [[0, 1]], 2, 3, min_leaf, 3)
    check(monkeypatch, ds, X, y, [np.arange(n)], [[0, 1]], 2, 0, min_leaf, 3)
