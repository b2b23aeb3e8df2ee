"""The device form of a dataset restated in plain numpy: what every table IS, written from the
design's definitions and the header comments of csrc/kernels_score.inc and csrc/kernels_order.inc -- not from the kernels.
tests/test_device_form_host.py holds this restatement to its own invariants without a device;
tests/test_gpu_device_form.py holds the tables the device built (native.device_form) to it, bit for bit.

Everything here is indexed the way the device form is: documents live at POSITIONS p of a padded position space, a
position that holds no document reads NO_DOCUMENT in `perm`."""
import math

import numpy as np

NO_DOCUMENT = 0xFFFFFFFF
RUN_DOCS = 768     # a run takes queries while it stays at or below this many documents
TILE = 64          # positions per feature tile; every run starts on a multiple of it
WALK_TILE = 128    # positions per walk tile, at most
DCG_RANKS = 20     # ranks the gain-class table covers


def xb_index(p, j, dq):
    """Float index of feature j of position p in the tile buffer xb[tile][dq][64 documents][4 features]."""
    p = np.asarray(p, dtype=np.int64)
    j = np.asarray(j, dtype=np.int64)
    return ((p >> 6) * dq + (j >> 2)) * 256 + (p & 63) * 4 + (j & 3)


def regroup(y, qid, rows=None):
    """Documents regrouped by query in first-appearance order, inside a query by gain descending, then id descending
    (the f32 gain; +0.0 and -0.0 are one gain).  `rows`: the instance ids the dataset holds, in iteration order (None:
    all, ascending).  Returns (query keys in first-appearance order, [ids of each query in storage order])."""
    qid = np.asarray(qid)
    rows = np.arange(len(qid), dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    gain = np.asarray(y, dtype=np.float64).astype(np.float32) + np.float32(0.0)
    keys, first, inverse = np.unique(qid[rows], return_index=True, return_inverse=True)
    appearance = np.argsort(first, kind="stable")            # unique() sorts by key: back to first-appearance order
    slot_of_key = np.empty(len(keys), dtype=np.int64)
    slot_of_key[appearance] = np.arange(len(keys))
    slot = slot_of_key[inverse]
    order = np.lexsort((-rows, -gain[rows].astype(np.float64), slot))  # last key first: query, gain desc, id desc
    sorted_rows, sorted_slot = rows[order], slot[order]
    cuts = np.flatnonzero(np.diff(sorted_slot)) + 1
    return keys[appearance], np.split(sorted_rows, cuts)


def layout(qlens):
    """Runs and query starts: consecutive queries share a run while it stays at or below RUN_DOCS documents (a longer query
    has a run of its own); a run's queries are packed tightly and every run starts on a multiple of TILE.  Returns a dict
    of qstart, qlen, run_q0, run_q1 (queries [q0, q1) of a run), run_pos, run_docs, run_order (longest first, ties in run
    order) and np, the size of the padded position space."""
    qstart, run_q0, run_q1, run_pos, run_docs = [], [], [], [], []
    pos, cur, q0 = 0, 0, 0
    for q, n in enumerate(int(v) for v in qlens):
        if cur > 0 and cur + n > RUN_DOCS:
            run_q0.append(q0), run_q1.append(q), run_pos.append(pos - cur), run_docs.append(cur)
            pos, cur, q0 = -(-pos // TILE) * TILE, 0, q
        qstart.append(pos)
        pos += n
        cur += n
    if cur > 0:
        run_q0.append(q0), run_q1.append(len(qstart)), run_pos.append(pos - cur), run_docs.append(cur)
        pos = -(-pos // TILE) * TILE
    u32 = lambda v: np.asarray(v, dtype=np.uint32)
    order = np.argsort(-np.asarray(run_docs, dtype=np.int64), kind="stable")
    return dict(qstart=u32(qstart), qlen=u32(list(qlens)), run_q0=u32(run_q0), run_q1=u32(run_q1), run_pos=u32(run_pos),
                run_docs=u32(run_docs), run_order=u32(order), np=pos)


def view_layout(parent_lay, parent_wt_start, queries):
    """A query sample lives in its parent's position space: query k of the view is the parent's queries[k], where the
    parent stores it.  Its runs are the maximal groups of its queries that are consecutive there, at most RUN_DOCS
    documents each; a run starts in the tile its first query starts in (run_pos) at lane run_lo, and run_docs counts from
    the tile's start.  vtiles = the 64-position tiles, wlist = the parent's walk tiles that hold its documents."""
    qstart = parent_lay["qstart"][queries].astype(np.int64)
    qlen = parent_lay["qlen"][queries].astype(np.int64)
    run_q0, run_q1, run_docs = [], [], []
    q0 = 0
    while q0 < len(qstart):
        q1, docs = q0 + 1, int(qlen[q0])
        while q1 < len(qstart) and qstart[q1] == qstart[q1 - 1] + qlen[q1 - 1] and docs + qlen[q1] <= RUN_DOCS:
            docs += int(qlen[q1])
            q1 += 1
        run_q0.append(q0), run_q1.append(q1), run_docs.append(docs)
        q0 = q1
    first = qstart[run_q0]
    last = qstart[np.asarray(run_q1) - 1] + qlen[np.asarray(run_q1) - 1] - 1
    run_docs = np.asarray(run_docs) + (first & 63)
    starts = np.asarray(parent_wt_start[:-1], dtype=np.int64)
    tile_of = lambda p: np.searchsorted(starts, p, side="right") - 1
    vt, wl = set(), set()
    for b, n in zip(qstart, qlen):
        vt.update(range(int(b) >> 6, ((int(b + n) - 1) >> 6) + 1))
    for a, b in zip(tile_of(first), tile_of(last)):
        wl.update(range(int(a), int(b) + 1))
    u32 = lambda v: np.asarray(v, dtype=np.uint32)
    return dict(qstart=u32(qstart), qlen=u32(qlen), run_q0=u32(run_q0), run_q1=u32(run_q1), run_pos=u32(first & ~63),
                run_lo=u32(first & 63), run_docs=u32(run_docs), run_order=u32(np.argsort(-run_docs, kind="stable")),
                run_wt0=u32(tile_of(first)), vtiles=u32(sorted(vt)), wlist=u32(sorted(wl)))


def position_map(lay, groups):
    """perm[p] = the instance id stored at position p (NO_DOCUMENT where there is none)."""
    perm = np.full(lay["np"], NO_DOCUMENT, dtype=np.uint32)
    for q, ids in enumerate(groups):
        perm[int(lay["qstart"][q]): int(lay["qstart"][q]) + len(ids)] = ids
    return perm


def walk_tiles(lay):
    """Every run's positions cut, greedily and in query order, into stretches of at most WALK_TILE positions such that a
    query of up to WALK_TILE documents is never cut; a longer one is cut every WALK_TILE documents from its start and what
    is left of it shares a tile with the queries behind it.  Returns (wt_start with np appended, run_wt0, seg) where
    seg[p] = lo | hi << 8 is position p's (query, tile) segment [lo, hi) relative to its tile's start, 0 for no document."""
    wt, run_wt0 = [], []
    for r in range(len(lay["run_pos"])):
        run_wt0.append(len(wt))
        start, length = int(lay["run_pos"][r]), 0
        for q in range(int(lay["run_q0"][r]), int(lay["run_q1"][r])):
            n = int(lay["qlen"][q])
            if n > WALK_TILE:
                if length:
                    wt.append(start)
                    start, length = start + length, 0
                while n > WALK_TILE:
                    wt.append(start)
                    start += WALK_TILE
                    n -= WALK_TILE
                length = n
            else:
                if length + n > WALK_TILE:
                    wt.append(start)
                    start, length = start + length, 0
                length += n
        if length:
            wt.append(start)
    wt.append(lay["np"])
    starts = np.asarray(wt, dtype=np.int64)
    seg = np.zeros(lay["np"], dtype=np.uint16)
    for q in range(len(lay["qlen"])):
        b = int(lay["qstart"][q])
        e = b + int(lay["qlen"][q])
        t = int(np.searchsorted(starts[:-1], b, side="right")) - 1
        while t < len(starts) - 1 and starts[t] < e:
            t0 = int(starts[t])
            t1 = min(int(starts[t + 1]), t0 + WALK_TILE)
            lo, hi = max(b, t0), min(e, t1)
            seg[lo:hi] = (lo - t0) | ((hi - t0) << 8)
            t += 1
    return np.asarray(wt, dtype=np.uint32), np.asarray(run_wt0, dtype=np.uint32), seg


def segments(wt_start, seg):
    """[(first position, one past the last position)] of every (query, walk tile) segment, ascending."""
    p = np.flatnonzero(seg)
    if len(p) == 0:
        return []
    tile = np.searchsorted(np.asarray(wt_start[:-1], dtype=np.int64), p, side="right") - 1
    t0 = np.asarray(wt_start, dtype=np.int64)[tile]
    lo = t0 + (seg[p] & 0xFF)
    hi = t0 + (seg[p] >> 8)
    pairs = np.unique(np.stack([lo, hi], axis=1), axis=0)
    return [(int(a), int(b)) for a, b in pairs]


def xslot(Xp, wt_start, seg):
    """xslot[f][p] = the slot position p takes inside its walk tile when its segment is sorted by x_f descending: the
    segment's first slot plus the document's rank, ties to the earlier position, NaN ranked as -inf.  Xp[p] = the feature
    row at position p.  Positions without a document read 0 here (the device leaves them unwritten)."""
    npos, d = Xp.shape
    out = np.zeros((d, npos), dtype=np.uint8)
    starts = np.asarray(wt_start, dtype=np.int64)
    for lo, hi in segments(wt_start, seg):
        t0 = int(starts[np.searchsorted(starts[:-1], lo, side="right") - 1])
        x = Xp[lo:hi].astype(np.float64)
        x = np.where(np.isnan(x), -np.inf, x)
        order = np.argsort(-x, axis=0, kind="stable")        # order[r, f] = the segment's document of rank r under f
        rank = np.empty_like(order)
        np.put_along_axis(rank, order, np.arange(hi - lo)[:, None].repeat(d, axis=1), axis=0)
        out[:, lo:hi] = (lo - t0 + rank).T
    return out


def colmax(X):
    """Per column max |x| over the uploaded rows as f64; inf for a column that holds inf or NaN."""
    a = np.abs(X.astype(np.float64))
    bad = ~np.isfinite(a).all(axis=0)
    out = np.where(np.isnan(a), 0.0, a).max(axis=0)
    out[bad] = np.inf
    return out


def gain_tables(gain_by_position, has_document):
    """(gexp[p] = 2^gain - 1 in f64 (libm pow on the f32 gain widened; 0 without a document), class id per position with
    classes numbered by DESCENDING gain and +-0 one class, dcgtab[class][i] = (2^g - 1) / log2(i + 2))."""
    g = np.where(has_document, gain_by_position, np.float32(0.0)).astype(np.float32)
    gexp = np.zeros(len(g), dtype=np.float64)
    for v in np.unique(g[has_document]):
        gexp[has_document & (g == v)] = math.pow(2.0, float(v)) - 1.0
    canon = g + np.float32(0.0)
    classes = np.unique(canon[has_document])[::-1]
    cls = np.zeros(len(g), dtype=np.uint32)
    for c, v in enumerate(classes):
        cls[has_document & (canon == v)] = c
    dcgtab = np.array([[(math.pow(2.0, float(v)) - 1.0) / math.log2(i + 2.0) for i in range(DCG_RANKS)] for v in classes])
    return gexp, cls, dcgtab


def duplicate_groups(X, groups):
    """Two documents share a group iff they are in one query and their feature rows are equal BIT FOR BIT (a row that
    differs from another only in the sign of a zero is a different row).  Returns {instance id: group label} for the
    documents that have a duplicate (labels are arbitrary, unique over the dataset) and the number of groups."""
    label, ngroups = {}, 0
    for ids in groups:
        rows = {}
        for i in ids:
            rows.setdefault(X[int(i)].tobytes(), []).append(int(i))
        for members in rows.values():
            if len(members) > 1:
                for i in members:
                    label[i] = ngroups
                ngroups += 1
    return label, ngroups


def column_stats(Xdocs):
    """Per column over the dataset's documents, by float value (-0.0 == 0.0): mn, mx, and how many documents sit at each;
    colmode bit 0 / 1 = more than a tenth of the documents at the maximum / minimum."""
    n = Xdocs.shape[0]
    mn, mx = Xdocs.min(axis=0), Xdocs.max(axis=0)
    at_min = (Xdocs == mn[None, :]).sum(axis=0).astype(np.uint64)
    at_max = (Xdocs == mx[None, :]).sum(axis=0).astype(np.uint64)
    mode = np.array([(1 if float(a) > 0.1 * float(n) else 0) | (2 if float(b) > 0.1 * float(n) else 0) for a, b in zip(at_max, at_min)],
                    dtype=np.uint8)
    return mn, mx, at_min, at_max, mode


def colstd_from_sums(total, total_sq, n):
    """The host's formula on the device's sums: sqrt(sumsq / n - mean^2), 0 where that is not positive."""
    out = np.zeros(len(total))
    for j in range(len(total)):
        mean = float(total[j]) / float(n)
        var = float(total_sq[j]) / float(n) - mean * mean
        out[j] = math.sqrt(var) if var > 0.0 else 0.0
    return out


class Form:
    """The restated device form of the dataset (X, y, qid), or of the rows `rows` of it."""

    def __init__(self, X, y, qid, rows=None, order_tables=True):
        self.X = X
        self.n = X.shape[0] if rows is None else len(rows)
        self.d = X.shape[1]
        self.dq = (self.d + 3) // 4
        self.keys, self.groups = regroup(y, qid, rows)
        self.lay = layout([len(g) for g in self.groups])
        self.np = self.lay["np"]
        self.perm = position_map(self.lay, self.groups)
        self.has_document = self.perm != NO_DOCUMENT
        self.wt_start, self.run_wt0, self.segtab = walk_tiles(self.lay)
        gain = np.zeros(self.np, dtype=np.float32)
        gain[self.has_document] = np.asarray(y, dtype=np.float64).astype(np.float32)[self.perm[self.has_document]]
        self.gain = gain
        self.gexp, self.gcls, self.dcgtab = gain_tables(gain, self.has_document)
        self.Xp = np.zeros((self.np, self.d), dtype=np.float32)   # rows by position; +0.0 where there is no document
        self.Xp[self.has_document] = X[self.perm[self.has_document]]
        self.xslot = xslot(self.Xp, self.wt_start, self.segtab) if order_tables else None

    def tiles(self):
        """The raw tile buffer: zero-padded to 4 * dq columns and to np positions."""
        xb = np.zeros(self.np // TILE * self.dq * 256, dtype=np.float32)
        p = np.arange(self.np, dtype=np.int64)[:, None]
        j = np.arange(self.d, dtype=np.int64)[None, :]
        xb[xb_index(p, j, self.dq)] = self.Xp
        return xb
