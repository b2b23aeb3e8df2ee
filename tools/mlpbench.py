"""mlpbench.py -- the NeuralNet kernels on an MSLR-WEB30K-shaped matrix (bench.py's generator), one JSON line (DESIGN.md
section 19).

    python tools/mlpbench.py --shape 30k            # three alternating runs: the kernels / the same net in torch's f64

Reports, per run: the device time of mlp_score_kernel, mlp_backprop_kernel and mlp_fold_kernel (the library's event timing); the
device time of torch's torch.relu(X64 @ W1.T + b1) @ w2 and of its autograd backward on an f64 copy of X, and of making that
copy, timed apart; the two derived floors (MFMAs per tile x 64 cycles over 1 024 SIMDs at 2.4 GHz) and the HBM floor of the
tiles; and a training run stage by stage.
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

HBM_ACHIEVABLE_GBS = 6300.0  # the achievable HBM read rate BASELINE.md and DESIGN.md use
SIMDS, CLOCK_HZ, MFMA_CYCLES = 1024, 2.4e9, 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="30k", choices=sorted(SHAPES))
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    if not args.no_torch:  # (torch brings its device up first, as in bench.py)
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("mlpbench.py needs an MI355X: torch.cuda.is_available() is False")
        torch.cuda.init()
    import fastrank_amd as fr
    from fastrank_amd import native

    n, d, q, seed = SHAPES[args.shape]
    h = args.hidden
    X, y, qid = gen_mslr_shaped(seed, n, d, q)
    raw = fr.CDataset.from_numpy(X, y, qid)
    ds = fr.Normalizer.fit(raw, "zscore").apply(raw)
    native.device_info(ds)
    rng = np.random.default_rng(1)
    W1, b1, w2, b2 = rng.normal(0.0, 0.1, (h, d)), rng.normal(0.0, 0.1, h), rng.normal(0.0, 0.3, h), 0.25
    lam = rng.normal(0.0, 1.0, n)
    model = fr.CModel.from_dict({"NeuralNet": {"activation": "relu", "hidden_weights": W1.tolist(), "hidden_bias": b1.tolist(),
                                               "output_weights": w2.tolist(), "output_bias": b2}})
    plan = {}
    native.mlp_gradients(ds, model, lam, plan=plan)  # warm-up: tables, records, code objects
    scores = native.predict_scores_dense(model, ds)
    kpanels = -(-d // 144) * 36
    fwd = plan["hidden_panels"] * 4 * 4 * kpanels
    bwd = fwd * plan["feature_panels"] + plan["hidden_panels"] * plan["feature_panels"] * 9 * 4 * 16
    floor = lambda mfmas: plan["tiles"] * mfmas * MFMA_CYCLES / SIMDS / CLOCK_HZ * 1e3  # noqa: E731
    out = {"metric": "NeuralNet kernels, device ms", "shape": args.shape, "n": n, "d": d, "hidden": h, "queries": q, "plan": plan,
           "mfma_per_tile": {"score": fwd, "backprop": bwd}, "score_mfma_floor_ms": floor(fwd), "backprop_mfma_floor_ms": floor(bwd),
           "hbm_floor_ms": plan["tile_bytes"] / (HBM_ACHIEVABLE_GBS * 1e9) * 1e3, "runs": []}
    torch_once = None
    if not args.no_torch:
        Xn = native.loaded_arrays(ds)["x"]
        xt = torch.from_numpy(np.ascontiguousarray(Xn)).cuda()
        tw1, tb1, tw2 = (torch.from_numpy(a).cuda().requires_grad_() for a in (W1, b1, w2))
        tlam = torch.from_numpy(lam).cuda()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]

        def torch_once():
            ev[0].record()
            x64 = xt.double()
            ev[1].record()
            s = torch.relu(x64 @ tw1.T + tb1) @ tw2 + b2
            ev[2].record()
            gw1, gb1, gw2 = torch.autograd.grad(s, (tw1, tb1, tw2), tlam)
            ev[3].record()
            torch.cuda.synchronize()
            return [ev[k].elapsed_time(ev[k + 1]) for k in range(3)], s.detach().cpu().numpy(), gw1.cpu().numpy()

        torch_once()  # warm-up
    for _ in range(args.runs):
        native.profile_enable(True)
        native.profile_reset()
        scores = native.predict_scores_dense(model, ds)
        g = native.mlp_gradients(ds, model, lam)
        prof = native.profile_stats()
        native.profile_enable(False)
        run = {"score_ms": prof["mlp_score_kernel"]["total_ms"], "backprop_ms": prof["mlp_backprop_kernel"]["total_ms"],
               "fold_ms": prof["mlp_fold_kernel"]["total_ms"]}
        if torch_once is not None:
            (conv_ms, fwd_ms, bwd_ms), ts, tg = torch_once()
            run.update(torch_convert_ms=conv_ms, torch_forward_ms=fwd_ms, torch_backward_ms=bwd_ms,
                       max_rel_score_diff_vs_torch=float(np.max(np.abs(ts - scores)) / np.max(np.abs(ts))),
                       max_rel_grad_diff_vs_torch=float(np.max(np.abs(tg - g["hidden_weights"])) / np.max(np.abs(tg))))
        out["runs"].append(run)
    for key in out["runs"][0]:
        if key.endswith("_ms"):
            out[key + "_median"] = float(np.median([r[key] for r in out["runs"]]))
    out["score_over_mfma_floor"] = out["score_ms_median"] / out["score_mfma_floor_ms"]
    out["backprop_over_mfma_floor"] = out["backprop_ms_median"] / out["backprop_mfma_floor_ms"]
    req = fr.TrainRequest.neural_lambdarank()
    req.measure, req.params.quiet, req.params.num_iterations, req.params.hidden = "ndcg@10", True, args.iterations, h
    t0 = time.perf_counter()
    ds.train_model(req)
    st = native.last_train_stats()["neural_lambdarank"]
    st["wall_seconds"] = time.perf_counter() - t0
    out["training"] = st
    print(json.dumps(out))


if __name__ == "__main__":
    main()
