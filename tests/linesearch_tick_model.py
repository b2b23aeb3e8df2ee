"""What a captured line search must have published, from the oracle alone (no device, no product code).

A capture log (native.CoordinateAscentRun.take_capture) is a list of events in the order the device dataset met them:

  {"type": "store", "slot", "v"}        resident slot <- the exact ordered sums of the un-normalised weight vector v
  {"type": "tick", "ctx", "kind", "measure", "depth", "groups", "gorder", "nverify", "approx", "resident", "ready",
   "inst", "redo", "redo_groups", "means", "matrix", "resident_sums"}

The model turns the log, the (X, y, qid) arrays and the device form's `perm` (position -> instance) into
  * the expected per-query matrix of every tick: staged column k * 64 + c holds the oracle's metric of the weights of
    caller's group gorder[k] with [feature] = candidate c (only c < the group's candidate count is defined),
  * the expected means (caller's order) in the device's two-level summation shape,
  * the expected resident sums: per slot, the last store's score_linear(v), then one oracle.resident_update per tick
    whose line search read the resident sums and whose group carried has_update,
  * the split of a tick's (query, group) pairs into "decided by the verify kernel" and "recomputed" (the redo list).
"""
import numpy as np

from oracle import pyoracle as o

MEASURES = {0: "ndcg", 1: "map", 2: "mrr"}
NO_DOCUMENT = 0xFFFFFFFF


def measure_name(measure, depth):
    base = MEASURES[int(measure)]
    return base if int(depth) < 0 else "%s@%d" % (base, int(depth))


def device_mean(values):
    """The mean in the device's shape: 256-query segments summed on their own, then the segment sums."""
    before = int(o.lib().oracle_get_mean_segment())
    o.set_mean_segment(o.DEVICE_MEAN_SEGMENT)
    try:
        return o.mean(values)
    finally:
        o.set_mean_segment(before)


class TickModel:
    def __init__(self, X, y, qid, perm):
        self.ds = o.Dataset(X, y, qid)
        self.X = self.ds.X
        self.perm = np.asarray(perm, dtype=np.int64)
        self.valid = (self.perm != NO_DOCUMENT) & (self.perm < self.ds.n)
        off = self.ds.query_offsets().astype(np.int64)
        self.qlen = np.diff(off)
        self._scores = {}   # weights bytes -> score_linear
        self._cols = {}     # (measure name, weights bytes) -> per-query metric
        self.reset()

    def reset(self):
        """Forgets the replay of a log (the caches of oracle scores and columns stay)."""
        self._sums = {}     # slot -> resident sums by instance
        self.updates_in_verify = 0   # pending updates applied inside a verify launch / by resident_update_kernel
        self.updates_by_kernel = 0
        self.unreplayed = 0          # resident groups met before any store of their slot (a capture switched on late)

    # ---- expected values ------------------------------------------------------------------------------------------
    def column(self, name, w):
        w = np.ascontiguousarray(w, dtype=np.float64)
        key = w.tobytes()
        got = self._cols.get((name, key))
        if got is None:
            s = self._scores.get(key)
            if s is None:
                s = self._scores[key] = self.ds.score_linear(w)
            got, err = self.ds.metric_from_scores(name, s)
            assert err == 0, (name, err)
            self._cols[(name, key)] = got
        return got

    def group_columns(self, tick, g):
        """[candidates] per-query columns of caller's group g."""
        name = measure_name(tick["measure"], tick["depth"])
        grp = tick["groups"][g]
        out = []
        for cand in grp["candidates"]:
            w = np.array(grp["weights"], dtype=np.float64)
            w[grp["feature"]] = cand
            out.append(self.column(name, w))
        return out

    def expected_matrix(self, tick):
        """(E, defined): the staged nq x ldm matrix and which of its columns are defined."""
        G = len(tick["groups"])
        E = np.full((self.ds.nq, G * 64), np.nan)
        defined = np.zeros(G * 64, dtype=bool)
        for k, g in enumerate(tick["gorder"]):
            for c, col in enumerate(self.group_columns(tick, g)):
                E[:, k * 64 + c] = col
                defined[k * 64 + c] = True
        return E, defined

    def expected_means(self, tick):
        """(means, defined) in the caller's order."""
        G = len(tick["groups"])
        means = np.full(G * 64, np.nan)
        defined = np.zeros(G * 64, dtype=bool)
        for g in range(G):
            for c, col in enumerate(self.group_columns(tick, g)):
                means[g * 64 + c] = device_mean(col)
                defined[g * 64 + c] = True
        return means, defined

    # ---- resident sums ---------------------------------------------------------------------------------------------
    def apply(self, event):
        """Advances the replay by one event; a tick returns {slot: expected sums by instance} of its resident groups."""
        if event["type"] == "store":
            self._sums[int(event["slot"])] = self.ds.score_linear(np.asarray(event["v"], dtype=np.float64)).copy()
            return None
        if not event["resident"]:
            return {}
        done, out = set(), {}
        staged = {g: k for k, g in enumerate(event["gorder"])}
        for g, grp in enumerate(event["groups"]):
            slot = int(grp["resident_slot"])
            if slot < 0:
                continue
            if slot not in self._sums:
                self.unreplayed += 1
                continue
            if grp["has_update"] and slot not in done:   # (groups of one restart share the slot: one update per tick)
                done.add(slot)
                xf = np.ascontiguousarray(self.X[:, int(grp["upd_feature"])])
                o.resident_update(self._sums[slot], xf, grp["upd_cand"], grp["upd_base_f"], 1.0 / grp["upd_norm"])
                if event["approx"] and staged[g] < event["nverify"]:
                    self.updates_in_verify += 1
                else:
                    self.updates_by_kernel += 1
            out[slot] = self._sums[slot]
        return out

    def by_position(self, sums):
        """Sums by instance -> by position of the device form (positions that hold no document: 0, see `valid`)."""
        out = np.zeros(len(self.perm))
        out[self.valid] = sums[self.perm[self.valid]]
        return out

    # ---- who decided a pair ----------------------------------------------------------------------------------------
    def split(self, tick):
        """{(query, caller's group): slice mask} of the pairs the exact kernels recomputed from the redo list, and the number
        of pairs the verify kernel decided.  A line search the exact kernels took whole has neither."""
        if not tick["approx"]:
            return {}, 0
        G = int(tick["redo_groups"])
        redone = {}
        for e in np.asarray(tick["redo"], dtype=np.int64):
            item, mask = (e >> 4, int(e & 15)) if tick["kind"] == "topk" else (e, 15)
            k, q = int(item % G), int(item // G)
            g = int(tick["gorder"][k])
            redone[(q, g)] = redone.get((q, g), 0) | mask
        return redone, self.ds.nq * int(tick["nverify"]) - len(redone)


def check_tick(model, tick, index, expected_sums):
    """Every defined cell, every mean and every resident sum of one captured line search against the model; raises with
    the first offending cell spelled out.  Returns (pairs decided by the verify kernel, pairs recomputed, 1 if the matrix
    was absent)."""
    redone, verified = model.split(tick)
    means, mdef = model.expected_means(tick)
    got_means = np.asarray(tick["means"])
    bad = np.nonzero(mdef & ~(got_means == means))[0]
    if len(bad):
        j = int(bad[0])
        raise AssertionError("tick %d (%s %s, context %d): mean of group %d candidate %d is %r, the oracle's %r" % (
            index, tick["kind"], measure_name(tick["measure"], tick["depth"]), tick["ctx"], j // 64, j % 64, got_means[j], means[j]))
    absent = 0
    if tick["matrix"] is None:
        assert tick["ready"], "tick %d: only a line search evaluated at submit may come without its matrix" % index
        absent = 1
    else:
        E, cdef = model.expected_matrix(tick)
        M = np.asarray(tick["matrix"])
        assert M.shape == E.shape, (index, M.shape, E.shape)
        wrong = ~(M == E) & cdef[None, :]   # (np.array_equal's notion of equal, cell by cell)
        if wrong.any():
            q, j = (int(v) for v in np.argwhere(wrong)[0])
            g = int(tick["gorder"][j // 64])
            staged_verify = tick["approx"] and j // 64 < tick["nverify"]
            how = "exact kernel" if not staged_verify else ("redone, slices %s" % bin(redone[(q, g)]) if (q, g) in redone else "verified")
            raise AssertionError(
                "tick %d (%s %s, context %d, inst %r): group %d (staged %d, feature %d) candidate %d query %d (length %d, %s): published %r, the oracle's %r; %d cells differ"
                % (index, tick["kind"], measure_name(tick["measure"], tick["depth"]), tick["ctx"], tick["inst"], g, j // 64,
                   tick["groups"][g]["feature"], j % 64, q, int(model.qlen[q]), how, M[q, j], E[q, j], int(wrong.sum())))
    got = tick["resident_sums"]
    if tick["resident"]:
        assert set(expected_sums) <= set(got), (index, sorted(got), sorted(expected_sums))
    for slot, sums in got.items():
        if slot not in expected_sums:
            continue
        exp = model.by_position(expected_sums[slot])
        diff = np.nonzero(model.valid & ~_same(np.asarray(sums), exp))[0]
        if len(diff):
            p = int(diff[0])
            raise AssertionError("tick %d: resident sum of slot %d at position %d (instance %d) is %r, the replay's %r; %d differ" % (
                index, slot, p, int(model.perm[p]), sums[p], exp[p], len(diff)))
    return verified, len(redone), absent


def _same(a, b):
    """Bitwise equality of two float64 arrays (a NaN equals the same NaN, -0.0 differs from 0.0)."""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64) == np.ascontiguousarray(b, dtype=np.float64).view(np.uint64)


def check_log(model, log):
    """The whole log in order.  Returns the totals: ticks and stores, all (query, group) pairs and how many of them the
    verify kernel decided / the exact kernels recomputed from the redo list (the rest: line searches or groups the exact
    kernels took whole), matrices absent, resident groups that could not be replayed, the context indices seen."""
    tot = {"ticks": 0, "stores": 0, "pairs": 0, "verified": 0, "redone": 0, "absent": 0, "unreplayed": 0, "contexts": set()}
    for i, ev in enumerate(log):
        exp = model.apply(ev)
        if ev["type"] == "store":
            tot["stores"] += 1
            continue
        v, r, a = check_tick(model, ev, i, exp)
        tot["ticks"] += 1
        tot["pairs"] += model.ds.nq * len(ev["groups"])
        tot["verified"] += v
        tot["redone"] += r
        tot["absent"] += a
        tot["contexts"].add(int(ev["ctx"]))
    tot["unreplayed"] = model.unreplayed
    return tot
