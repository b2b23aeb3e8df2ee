"""normbench.py -- feature normalisation on an MSLR-WEB30K-shaped matrix (bench.py's generator), three
runs each:

    Normalizer.fit(ds, "zscore")               the chunk records and their fold on the device, d records downloaded
    Normalizer.fit(...).apply(ds)              kernel, download of the matrix through the pinned slabs, building the new core, and
                                               the rest of the call: the instance list, the new matrix's host memory, device buffers
    Normalizer.per_query("zscore").apply(ds)   the same three for the query scope
    for information: the vectorised numpy restatement (tests/normalize_model.py) of fit + apply on the host, on the first
    --numpy-share of the rows (the whole matrix takes several temporaries of its size)

    python tools/normbench.py --shape 30k --out profiles/normalize_30k_bench.json

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

from bench import SHAPES, gen_mslr_shaped  # noqa: E402

# dataset_query_json("normalization_stats"): where an apply's time went (wall: the Python call around it)
STAGES = ("wall_seconds", "prepare_seconds", "allocate_seconds", "kernel_seconds", "download_seconds", "device_other_seconds", "core_build_seconds",
          "total_seconds")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="30k", choices=sorted(SHAPES))
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--numpy-share", type=float, default=0.1, help="share of the rows the numpy restatement is timed on (0: skip)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import fastrank_amd as fr
    from fastrank_amd import native

    n, d, q, seed = SHAPES[args.shape]
    X, y, qid = gen_mslr_shaped(seed, n, d, q)
    ds = fr.CDataset.from_numpy(X, y, qid)
    t0 = time.perf_counter()
    native.num_queries(ds)
    ds.feature_stats()  # (builds the device form, pays the runtime's start-up)
    first_s = time.perf_counter() - t0

    fits, applies, queries = [], [], []
    for _ in range(args.runs):
        t = time.perf_counter()
        norm = fr.Normalizer.fit(ds, "zscore")
        fits.append({"wall_seconds": time.perf_counter() - t})
        for runs, nm in ((applies, norm), (queries, fr.Normalizer.per_query("zscore"))):
            t = time.perf_counter()
            out = nm.apply(ds)
            wall = time.perf_counter() - t
            st = out._query_json("normalization_stats")
            runs.append(dict(st, wall_seconds=wall))
            del out

    def med(runs, key):
        return float(np.median([r[key] for r in runs]))

    result = {"shape": {"name": args.shape, "instances": n, "features": d, "queries": q, "matrix_bytes": int(X.nbytes)},
              "first_call_seconds": first_s, "fit": fits, "apply": applies, "per_query": queries,
              "median": {"fit_seconds": med(fits, "wall_seconds"),
                         "apply": {k: med(applies, k) for k in STAGES}, "per_query": {k: med(queries, k) for k in STAGES}}}
    result["median"]["apply"]["dominant"] = max(STAGES[1:-1], key=lambda k: result["median"]["apply"][k])
    if args.numpy_share > 0:
        from tests import normalize_model as nmod

        rows = max(2, int(n * args.numpy_share))
        Xs = np.ascontiguousarray(X[:rows])
        H = np.ones(Xs.shape, dtype=bool)
        t = time.perf_counter()
        st = nmod.fit(Xs, H, np.arange(rows), range(d))
        fit_np = time.perf_counter() - t
        t = time.perf_counter()
        nmod.apply(Xs, H, st, "zscore")
        result["numpy_restatement"] = {"rows": rows, "share": rows / n, "fit_seconds": fit_np, "apply_seconds": time.perf_counter() - t,
                                       "note": "for information: vectorised across chunks and features, one host thread"}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
