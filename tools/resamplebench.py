"""resamplebench.py -- model comparison's resampling kernels on tables of per-query values of the 30K
shape's size (31 000 queries), uniform values in [0, 1):

    shapes       Q = 31 000 with M = 2 and M = 8 systems, T = 10 000 and T = 100 000 trials: --runs alternating rounds of
                 fr_resample over the four, per call the two kernels' times, upload, download, the host's report and the wall
                 time of the whole call
    --paths      the bootstrap kernel's two forms (rows gathered from LDS / from global memory; FR_RESAMPLE_BOOT=global
                 selects the second) at Q = 16 384 / M = 1 and Q = 31 000 / M = 2 (which no workgroup's LDS holds: both runs take
                 the global form there), T = 100 000, --runs alternating rounds; only meaningful while both forms exist
    numpy        for information: the vectorised restatement (tests/resample_model.py) at T = 200, and that time scaled
                 linearly to the shapes' trial counts, labelled as scaled

    python tools/resamplebench.py --out profiles/resample_30k_bench.json

One JSON line (and the file).  There is no threshold: the feature has no parent to be compared with.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STAT_KEYS = ("boot_path", "boot_ms", "perm_ms", "upload_ms", "download_ms", "device_call_ms", "report_ms")


def one_call(native, V, trials, seed, perm=True):
    t = time.perf_counter()
    rep, _, _ = native.resample(V, trials, seed, perm=perm)
    out = {k: rep[k] for k in STAT_KEYS}
    out["wall_ms"] = (time.perf_counter() - t) * 1e3
    return out


def spread(runs, key):
    vals = [r[key] for r in runs]
    return {"min": min(vals), "median": float(np.median(vals)), "max": max(vals)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=31000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--paths", action="store_true", help="also time the bootstrap kernel's LDS form against its global form")
    ap.add_argument("--numpy-trials", type=int, default=200, help="trials the numpy restatement is timed at (0: skip)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from fastrank_amd import native

    rng = np.random.default_rng(20261021)
    tables = {m: rng.random((args.queries, m)) for m in (2, 8)}
    first = one_call(native, tables[2][:64], 64, 0)  # (pays the runtime's start-up)
    shapes = [(m, t) for m in (2, 8) for t in (10000, 100000)]
    runs = {"M%d_T%d" % s: [] for s in shapes}
    for r in range(args.runs):
        for m, t in shapes:
            runs["M%d_T%d" % (m, t)].append(one_call(native, tables[m], t, r))
    result = {"queries": args.queries, "first_call": first, "runs": runs,
              "summary": {name: {k: spread(rs, k) for k in ("boot_ms", "perm_ms", "wall_ms", "report_ms")} for name, rs in runs.items()}}
    if args.paths:
        cases = {"Q16384_M1": rng.random((16384, 1)), "Q%d_M2" % args.queries: tables[2]}
        paths = {name: {"default": [], "forced_global": []} for name in cases}
        for r in range(args.runs):
            for name, V in cases.items():
                for side in ("default", "forced_global"):
                    if side == "forced_global":
                        os.environ["FR_RESAMPLE_BOOT"] = "global"
                    try:
                        paths[name][side].append(one_call(native, V, 100000, r, perm=False))
                    finally:
                        os.environ.pop("FR_RESAMPLE_BOOT", None)
        result["paths"] = {"trials": 100000, "runs": paths,
                           "boot_ms": {name: {side: spread(rs, "boot_ms") for side, rs in sides.items()} for name, sides in paths.items()}}
    if args.numpy_trials > 0:
        from tests import resample_model as rm

        timed = {}
        for m in (2, 8):
            t = time.perf_counter()
            rm.boot(tables[m], args.numpy_trials, 0)
            tb = time.perf_counter() - t
            t = time.perf_counter()
            rm.perm(tables[m], args.numpy_trials, 0)
            tp = time.perf_counter() - t
            timed["M%d" % m] = {"trials": args.numpy_trials, "boot_seconds": tb, "perm_seconds": tp,
                                "scaled_linearly_to_T10000_seconds": (tb + tp) * 10000 / args.numpy_trials,
                                "scaled_linearly_to_T100000_seconds": (tb + tp) * 100000 / args.numpy_trials}
        result["numpy_restatement"] = dict(timed, note="for information: one host thread, vectorised over trials; the T = 10 000 and "
                                                       "T = 100 000 figures are the measured time scaled linearly, not measured")
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
