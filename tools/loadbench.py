"""Times CDataset.open_ranksvm on one generated MSLR-like text file ("Text loading").

    python tools/loadbench.py --lines 380000 --parent-root /path/to/a/built/checkout/of/the/parent --out-dir profiles

The file is generated here (nothing is downloaded): `--lines` lines of 136 features, %.6g and integer values, a label, a qid
and a docid comment per line.  To keep the generator quick it formats a block of 20 000 distinct feature rows once and
repeats it; the label, qid and docid differ on every line.  380 000 lines are a tenth of the 30K shape (3.8 M documents).

In one session it alternates three times over: the parent commit's open_ranksvm (when --parent-root names a built tree of
it), this tree's parser="host", parser="device", and parser="device" on the gzipped file.  Every measurement is a fresh
child process that first loads a twenty-line file with the same parser (so the HIP runtime's start-up is not in the number)
and then times the load.  Writes load_text_bench.json and load_text_parent.json with the per-stage seconds.
"""
import argparse
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import json, sys, time
root, path, tiny, parser = sys.argv[1:5]
sys.path.insert(0, root)
import fastrank_amd as fr
kw = {} if parser == "parent" else {"parser": parser}
fr.CDataset.open_ranksvm(tiny, **kw)
t0 = time.perf_counter()
ds = fr.CDataset.open_ranksvm(path, **kw)
wall = time.perf_counter() - t0
out = {"wall_seconds": wall, "instances": ds.num_instances(), "features": ds.num_features()}
if parser != "parent":
    from fastrank_amd import native
    st = native.last_load_stats()
    out.update(parser=st["parser"], reason=st["reason"], bytes=st["bytes"], lines=st["lines"], host_lines=st["host_lines"],
               host_line_reasons=st["host_line_reasons"], seconds=st["seconds"])
print("LOADBENCH " + json.dumps(out))
"""


def generate(path, lines, feats=136, block=20000, seed=7):
    rng = np.random.default_rng(seed)
    vals, ints, pick = rng.uniform(0, 1000, (block, feats)), rng.integers(0, 5000, (block, feats)), rng.random((block, feats)) < 0.4
    bodies = [" ".join("%d:%s" % (j + 1, str(int(ints[i, j])) if pick[i, j] else "%.6g" % vals[i, j]) for j in range(feats)) for i in range(block)]
    labels = rng.integers(0, 5, lines)
    with open(path, "w") as fh:
        for at in range(0, lines, block):
            fh.write("".join("%d qid:%d %s # doc-%d\n" % (labels[i], i // 120, bodies[i - at], i) for i in range(at, min(lines, at + block))))
    return os.path.getsize(path)


def run_child(root, path, tiny, parser):
    proc = subprocess.run([sys.executable, "-c", CHILD, root, path, tiny, parser], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    for line in proc.stdout.splitlines():
        if line.startswith("LOADBENCH "):
            return json.loads(line[len("LOADBENCH "):])
    raise RuntimeError("load failed (%s):\n%s" % (parser, proc.stdout))


def span(runs):
    t = [r["wall_seconds"] for r in runs]  # (the parent reports nothing else; "seconds" holds this tree's own stages)
    return [min(t), max(t)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lines", type=int, default=380000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit (its open_ranksvm is timed too)")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--parsers", default="host,device,device_gz", help="which of this tree's runs to make (a machine without a device: host)")
    ap.add_argument("--keep", default=None, help="keep the generated file here")
    args = ap.parse_args()
    work = tempfile.mkdtemp(prefix="loadbench_")
    try:
        path, tiny = os.path.join(work, "train.txt"), os.path.join(work, "tiny.txt")
        t0 = time.perf_counter()
        size = generate(path, args.lines)
        generate(tiny, 20, block=20)
        with open(path, "rb") as src, gzip.open(path + ".gz", "wb", compresslevel=1) as dst:
            shutil.copyfileobj(src, dst, 1 << 24)
        print("generated %d lines, %.1f MB (+ .gz %.1f MB) in %.1f s" % (args.lines, size / 1e6, os.path.getsize(path + ".gz") / 1e6,
                                                                           time.perf_counter() - t0), flush=True)
        runs = {"parent": [], "host": [], "device": [], "device_gz": []}
        for rep in range(args.repeats):
            for name in ("parent", "host", "device", "device_gz"):
                if (name == "parent" and not args.parent_root) or (name != "parent" and name not in args.parsers.split(",")):
                    continue
                r = run_child(args.parent_root if name == "parent" else ROOT, path + (".gz" if name == "device_gz" else ""), tiny,
                              "device" if name == "device_gz" else name)
                runs[name].append(r)
                print(rep, name, json.dumps(r), flush=True)
        shape = {"lines": args.lines, "features": 136, "bytes": size, "gz_bytes": os.path.getsize(path + ".gz"),
                 "share_of_30k_shape": args.lines / 3.8e6}
        os.makedirs(args.out_dir, exist_ok=True)
        bench = {"shape": shape, "runs": {k: v for k, v in runs.items() if k != "parent"},
                 "total_seconds_range": {k: span(v) for k, v in runs.items() if k != "parent" and v}}
        dev = runs["device"]
        if dev:
            stages = {k: float(np.median([r["seconds"][k] for r in dev])) for k in dev[0]["seconds"] if k != "total"}
            bench["device_stage_medians"] = stages
            bench["dominant_stage"] = max(stages, key=stages.get)
        if runs["parent"]:
            lo, hi = span(runs["parent"])
            bench["parent_total_seconds_range"] = [lo, hi]
            bench["device_wholly_below_parent"] = bool(dev) and span(dev)[1] < lo and bool(runs["device_gz"]) and span(runs["device_gz"])[1] < lo
            if runs["host"]:
                bench["host_inside_parent_range_widened_by_its_width"] = lo - (hi - lo) <= span(runs["host"])[0] and span(runs["host"])[1] <= hi + (hi - lo)
            with open(os.path.join(args.out_dir, "load_text_parent.json"), "w") as fh:
                json.dump({"shape": shape, "runs": runs["parent"], "total_seconds_range": [lo, hi]}, fh, indent=1)
        with open(os.path.join(args.out_dir, "load_text_bench.json"), "w") as fh:
            json.dump(bench, fh, indent=1)
        print(json.dumps({k: v for k, v in bench.items() if k != "runs"}))
        if args.keep:
            shutil.copy(path, args.keep)
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
