"""Numpy decoders of the three forest encodings the scoring kernels read, written from the layout comments of
csrc/kernels_tree.inc and csrc/kernels_treerank.inc (not from the packers of csrc/forest_pack.hpp, which they check): given
the packed tables (native.forest_pack) and a feature matrix they walk every document through the forest the way the
kernels do and return the f64 scores.  Every index a decoder follows is checked against its buffer first, so a packer slip
shows as an assertion, not as a wrong read.

    score_lds   tree_ensemble_lds_kernel: 8-byte node words, cur += rel + (x > thr), the leaf word's low half = product index
    score_rank  tree_ensemble_rank_kernel: Eytzinger ranking of the features to u16 codes (NaN -> 0xFFFF), heap walk
                cur = 2 * cur + (code > j), u16 leaf ids behind the heap
    score_l2    tree_ensemble_kernel: 16-byte node records, children adjacent
Sums are formed in tree order, part after part: acc = acc + product, from +0.0, unfused.
"""
import numpy as np

ABSENT = 0xFFFFFFFF
RANK_DOCS, RANK_PARTS = 192, 4  # the block of tree_ensemble_rank_kernel (forest_pack.hpp: RankBlock)


def _batches(desc, unit_words):
    """[(first word, end word, n, levels, fourth field)] of a descriptor list [nbatch + 1][4] whose offsets count 16-byte
    units (unit_words words each); the list ends in a terminator that holds the stream's end."""
    desc = np.asarray(desc, dtype=np.uint32)
    assert desc.ndim == 1 and len(desc) % 4 == 0 and len(desc) >= 8, len(desc)
    rows = desc.reshape(-1, 4)
    assert rows[-1, 1:].tolist() == [0, 0, 0], rows[-1]
    out = []
    for b in range(len(rows) - 1):
        first, end = int(rows[b, 0]) * unit_words, int(rows[b + 1, 0]) * unit_words
        assert first < end, (b, first, end)
        out.append((first, end, int(rows[b, 1]), int(rows[b, 2]), int(rows[b, 3])))
    return out


def _column(X, fid):
    return X[:, fid] if fid < X.shape[1] else np.zeros(X.shape[0], dtype=np.float32)


# --------------------------------------------------------------------------------------------- the f32 LDS walk

def score_lds(X, docs, parts, tables, raw_single):
    """Block shape docs x parts.  LDS holds the feature columns slot-major, [4 * dq + 1][docs] f32, the last slot 0.0."""
    X = np.asarray(X, dtype=np.float32)
    n_docs, d = X.shape
    dq = (d + 3) // 4
    forest, leafprod = np.asarray(tables["forest"], dtype=np.uint64), np.asarray(tables["leafprod"], dtype=np.float64)
    assert leafprod[0] == 0 and not np.signbit(leafprod[0])
    assert not raw_single or parts == 1
    acc = np.zeros(n_docs, dtype=np.float64)
    stream_end = 0
    for first, end, n, levels, zero in _batches(tables["desc"], 2):
        assert zero == 0 and n in (1, 2, 4, 8, 16) and end <= len(forest) and first == stream_end, (first, end, n)
        stream_end = end
        trees = forest[first:end]  # the batch as it lies in LDS
        assert len(trees) % 2 == 0 and len(trees) >= parts * n
        for part in range(parts):
            for k in range(n):
                cur = np.full(n_docs, int(trees[part * n + k]) & 0xFFFFFFFF, dtype=np.int64)
                assert parts * n <= cur[0] < len(trees)
                for _ in range(levels):
                    word = trees[cur]
                    lo, hi = (word & np.uint64(0xFFFFFFFF)).astype(np.uint32), (word >> np.uint64(32)).astype(np.uint32)
                    thr = lo.view(np.float32)
                    offset, rel = hi & np.uint32(0xFFFFFF), (hi >> np.uint32(24)).astype(np.int64)
                    assert (offset % (docs * 4) == 0).all()
                    slot = (offset // (docs * 4)).astype(np.int64)
                    assert ((slot < d) | (slot == dq * 4)).all(), "a node reads a slot that holds no feature"
                    x = np.zeros(n_docs, dtype=np.float32)
                    for s in np.unique(slot[slot < d]):
                        x = np.where(slot == s, X[:, s], x)
                    with np.errstate(invalid="ignore"):
                        cur = cur + rel + (~(x <= thr)).astype(np.int64)
                    assert (cur < len(trees)).all(), "a child index past the batch"
                leaf = trees[cur]
                # a leaf: the 0.0 slot, no child offset, the low half a product index
                assert ((leaf >> np.uint64(32)) == np.uint64(dq * 4 * docs * 4)).all(), "the walk did not end on a leaf"
                index = (leaf & np.uint64(0xFFFFFFFF)).astype(np.int64)
                assert (index < len(leafprod)).all() and (index < 1 << 23).all()
                acc = leafprod[index] if raw_single else acc + leafprod[index]
    assert stream_end == len(forest)
    return acc


# --------------------------------------------------------------------------------------------- the threshold-rank walk

def rank_codes(X, tables, nslots):
    """{byte offset of a slot in a document's code column: u16 codes of the documents}: the ranking rounds of the kernel, part
    after part, and the two constant slots."""
    X = np.asarray(X, dtype=np.float32)
    n_docs, d = X.shape
    dq = (d + 3) // 4
    docs, H = RANK_DOCS, RANK_PARTS
    fdesc = np.asarray(tables["fdesc"], dtype=np.uint32).reshape(-1, 4)
    rdesc = np.asarray(tables["rdesc"], dtype=np.uint32)
    tabs = np.asarray(tables["tables"], dtype=np.float32)
    assert len(fdesc) == dq * 4 and len(rdesc) % (8 * H) == 0
    rdesc = rdesc.reshape(-1, H, 2, 4)
    codes, ranked = {}, set()
    taken = [None] * H  # the float4 group whose features a part holds in registers
    for r in range(len(rdesc)):
        for h in range(H):
            (base, length, j4, flags), offs = (int(v) for v in rdesc[r, h, 0]), [int(v) for v in rdesc[r, h, 1]]
            if j4 == ABSENT:
                continue
            assert j4 < dq and j4 % H == h, (r, h, j4)
            assert length % docs == 0 and 0 < length <= 8 * docs and base + length <= len(tabs), (base, length)
            if flags & 1:
                taken[h] = j4
            assert taken[h] == j4, "a round ranks a group whose features the part has not taken"
            comps = [(flags >> (8 + 2 * j)) & 3 for j in range(4)]
            assert sorted(comps) == [0, 1, 2, 3]
            depths = []
            for cc, to in zip(comps, offs):
                if to == ABSENT:
                    depths.append(0)
                    continue
                f = j4 * 4 + cc
                so, _, logp, P = (int(v) for v in fdesc[f])
                assert so != ABSENT and P == 1 << logp and 1 <= logp <= 10 and to + P <= length, (f, so, logp, P, to)
                assert f < d and f not in ranked
                ranked.add(f)
                depths.append(logp)
                T = tabs[base + to:base + to + P]
                x = X[:, f]
                i = np.ones(n_docs, dtype=np.int64)
                with np.errstate(invalid="ignore"):
                    for _ in range(logp):
                        i = 2 * i + (T[i] < x)
                code = (i - P).astype(np.uint16)
                code[np.isnan(x)] = 0xFFFF
                assert so % 2 == 0 and so not in codes
                codes[so] = code
            assert depths == sorted(depths, reverse=True), "the round's features come deepest table first, absent ones last"
    used = {f for f in range(len(fdesc)) if int(fdesc[f, 0]) != ABSENT}
    assert used == ranked and len(used) == nslots, (sorted(used ^ ranked), nslots)
    # slot s = half (s & 1) of word s / 2 of the column: the used features take slots 0 .. nslots - 1, then P0 and P1
    slot_offset = lambda s: (s >> 1) * docs * 4 + (s & 1) * 2
    assert sorted(codes) == [slot_offset(s) for s in range(nslots)]
    codes[slot_offset(nslots)] = np.zeros(n_docs, dtype=np.uint16)
    codes[slot_offset(nslots + 1)] = np.full(n_docs, 0xFFFF, dtype=np.uint16)
    assert max(codes) <= 0xFFFF
    return codes


def score_rank(X, tables, nslots):
    X = np.asarray(X, dtype=np.float32)
    n_docs = X.shape[0]
    H = RANK_PARTS
    codes = rank_codes(X, tables, nslots)
    forest, leafprod = np.asarray(tables["forest"], dtype=np.uint32), np.asarray(tables["leafprod"], dtype=np.float64)
    halves = forest.view(np.uint16)
    acc = np.zeros(n_docs, dtype=np.float64)
    stream_end = 0
    for first, end, n, L, leafbase in _batches(tables["desc"], 4):
        assert n in (1, 2, 4, 8) and 1 <= L <= 10 and end <= len(forest) and first == stream_end, (first, end, n, L)
        stream_end = end
        stride = 3 << (L - 1)  # 2^L node words + 2^L u16 leaf ids
        assert H * n * stride <= end - first < H * n * stride + 4 and (end - first) % 4 == 0
        assert (end - first) * 4 <= 2 * 16 * RANK_DOCS * H, "a batch is what two prefetch slots of a block carry"
        assert leafbase < len(leafprod) and leafprod[leafbase] == 0 and not np.signbit(leafprod[leafbase])
        for part in range(H):
            for k in range(8):
                if k >= n:
                    acc = acc + 0.0
                    continue
                tree = first + (part * n + k) * stride
                cur = np.ones(n_docs, dtype=np.int64)
                for _ in range(L):
                    word = forest[tree + cur]
                    offset, j = word & np.uint32(0xFFFF), word >> np.uint32(16)
                    code = np.zeros(n_docs, dtype=np.uint32)
                    for so in np.unique(offset):
                        assert int(so) in codes, "a node reads a slot that holds no code"
                        code = np.where(offset == so, codes[int(so)], code)
                    cur = 2 * cur + (code > j)
                leaf_id = halves[2 * (tree + (1 << L)) + (cur - (1 << L))].astype(np.int64)
                assert (leafbase + leaf_id < len(leafprod)).all()
                acc = acc + leafprod[leafbase + leaf_id]
    assert stream_end == len(forest)
    return acc


# --------------------------------------------------------------------------------------------- the L2 walk

def score_l2(X, tables, raw_single):
    X = np.asarray(X, dtype=np.float32)
    n_docs, d = X.shape
    nodes, roots, tw = tables["nodes"], np.asarray(tables["roots"], dtype=np.int64), np.asarray(tables["tweights"], dtype=np.float64)
    assert len(roots) == len(tw) and (not raw_single or len(roots) == 1)
    acc = np.zeros(n_docs, dtype=np.float64)
    for t, root in enumerate(roots):
        end = roots[t + 1] if t + 1 < len(roots) else len(nodes)  # a tree's nodes are contiguous
        cur = np.full(n_docs, root, dtype=np.int64)
        while True:
            fid = nodes["fid"][cur]
            inner = fid >= 0
            if not inner.any():
                break
            x = np.zeros(n_docs, dtype=np.float64)
            for f in np.unique(fid[inner]):
                x = np.where(fid == f, _column(X, int(f)).astype(np.float64), x)
            with np.errstate(invalid="ignore"):
                step = nodes["lhs"][cur].astype(np.int64) + (~(x <= nodes["split"][cur]))
            assert (root < step[inner]).all() and (step[inner] < end).all(), "a child outside its tree"
            cur = np.where(inner, step, cur)
        leaf = nodes["split"][cur]
        acc = leaf if raw_single else acc + tw[t] * leaf
    return acc
