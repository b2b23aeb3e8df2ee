"""grambench.py -- the linear LambdaRank trainer's Gram kernel on an MSLR-WEB30K-shaped matrix (bench.py's generator), one
JSON line.

    python tools/grambench.py --shape 30k            # three alternating runs: the kernel pair / the same H formed by torch
    python tools/grambench.py --shape 30k --l2-sweep # also train with lambda_l2 = 1e-6, 1e-3 and 1.0 and report the measures

Reports, per run: the device time of weighted_gram_kernel and of gram_fold_kernel (the library's event timing); the device time
of torch forming H = X64.T @ (w[:, None] * X64) from an f64 copy of X, and of making that copy, timed apart; the floor: the
tile bytes one call streams over the achievable HBM rate; and a 20-iteration training run stage by stage.
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

HBM_ACHIEVABLE_GBS = 6300.0  # the achievable HBM read rate BASELINE.md and DESIGN.md use (8 000 GB/s is the spec peak)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="30k", choices=sorted(SHAPES))
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--l2-sweep", action="store_true", help="train with lambda_l2 = 1e-6, 1e-3, 1.0 and report the training measures")
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    if not args.no_torch:  # (torch brings its device up first, as in bench.py: after the library has it finds none)
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("grambench.py needs an MI355X: torch.cuda.is_available() is False")
        torch.cuda.init()
    import fastrank_amd as fr
    from fastrank_amd import native

    n, d, q, seed = SHAPES[args.shape]
    X, y, qid = gen_mslr_shaped(seed, n, d, q)
    ds = fr.CDataset.from_numpy(X, y, qid)
    native.device_info(ds)
    rng = np.random.default_rng(1)
    lam, wt = rng.normal(0.0, 1.0, n), rng.random(n)
    plan = {}
    H, g = native.weighted_gram(ds, lam, wt, plan=plan)  # warm-up: tables, slabs, code objects
    out = {"metric": "weighted Gram kernel pair, device ms", "shape": args.shape, "n": n, "d": d, "queries": q, "plan": plan,
           "floor_ms": plan["tile_bytes"] / (HBM_ACHIEVABLE_GBS * 1e9) * 1e3, "hbm_achievable_gbs": HBM_ACHIEVABLE_GBS, "runs": []}
    torch_state = None
    if not args.no_torch:
        xt = torch.from_numpy(X).cuda()
        wtt = torch.from_numpy(wt).cuda()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]

        def torch_once():
            ev[0].record()
            x64 = xt.double()
            ev[1].record()
            h = x64.T @ (wtt[:, None] * x64)
            ev[2].record()
            torch.cuda.synchronize()
            return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]), h

        torch_once()  # warm-up
        torch_state = torch_once
    for _ in range(args.runs):
        native.profile_enable(True)
        native.profile_reset()
        H, g = native.weighted_gram(ds, lam, wt)
        prof = native.profile_stats()
        native.profile_enable(False)
        run = {"gram_ms": prof["weighted_gram_kernel"]["total_ms"], "fold_ms": prof["gram_fold_kernel"]["total_ms"]}
        if torch_state is not None:
            conv_ms, mm_ms, h = torch_state()
            ht = h.cpu().numpy()
            run.update(torch_convert_ms=conv_ms, torch_matmul_ms=mm_ms,
                       max_rel_diff_vs_torch=float(np.max(np.abs(ht - H)) / np.max(np.abs(ht))))
        out["runs"].append(run)
    gm = float(np.median([r["gram_ms"] for r in out["runs"]]))
    out["gram_ms_median"] = gm
    out["gram_over_floor"] = gm / out["floor_ms"]
    if torch_state is not None:
        out["gram_over_torch_matmul"] = gm / float(np.median([r["torch_matmul_ms"] for r in out["runs"]]))

    def train(l2=None):
        req = fr.TrainRequest.linear_lambdarank()
        req.measure, req.params.quiet, req.params.num_iterations = "ndcg@10", True, args.iterations
        if l2 is not None:
            req.params.lambda_l2 = l2
        t0 = time.perf_counter()
        ds.train_model(req)
        st = native.last_train_stats()["linear_lambdarank"]
        st.pop("weights")
        st["wall_seconds"] = time.perf_counter() - t0
        return st

    out["training"] = train()
    if args.l2_sweep:
        out["l2_sweep"] = {str(l2): {k: v for k, v in train(l2).items() if k in ("train_measure", "best_iteration", "zero_measure")} for l2 in (1e-6, 1e-3, 1.0)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
