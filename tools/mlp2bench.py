"""mlp2bench.py -- the two-hidden-layer NeuralNet kernels on an MSLR-WEB30K-shaped matrix (bench.py's generator), one JSON line
("Two hidden layers"; the one-layer kernels: tools/mlpbench.py).

    python tools/mlp2bench.py --shape 30k --hidden 64 --hidden2 32     # three alternating runs: the kernels / the same net in torch's f64
    python tools/mlp2bench.py --shape 30k --hidden 256 --hidden2 64

Reports, per run: the device time of mlp2_score_kernel, mlp2_backprop_kernel and mlp2_fold_kernel (the library's event timing);
the device time of torch's forward and autograd backward on an f64 copy of X; the derived floors (MFMAs per tile that the kernels
issue x 64 cycles over 1 024 SIMDs at 2.4 GHz) and the HBM floor of the tiles; and a training run stage by stage.
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


def mfma_per_tile(d, h, h2):
    """MFMAs a workgroup's four waves issue per tile: (scoring, back-propagation summed over its passes).  Skipped k-steps and
    waves (units the model does not have) are not counted; first-layer panels are always whole."""
    nfp, nhp, w2 = -(-d // 144), -(-h // 64), -(-h2 // 16)
    first = nhp * nfp * 4 * 4 * 36
    second = sum(w2 * 4 * -(-min(64, h - 64 * p) // 4) for p in range(nhp))
    back = 0
    for p in range(nhp):
        w1 = -(-min(64, h - 64 * p) // 16)  # waves that own a unit of this panel
        per_pass = first + second + w1 * (4 * -(-h2 // 4) + 9 * 16)
        back += nfp * per_pass + w2 * 4 * 16  # (G_W2 in feature panel 0's pass only)
    return first + second, back


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="30k", choices=sorted(SHAPES))
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--hidden2", type=int, default=32)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    if not args.no_torch:  # (torch brings its device up first, as in bench.py)
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("mlp2bench.py needs an MI355X: torch.cuda.is_available() is False")
        torch.cuda.init()
    import fastrank_amd as fr
    from fastrank_amd import native

    n, d, q, seed = SHAPES[args.shape]
    h, h2 = args.hidden, args.hidden2
    X, y, qid = gen_mslr_shaped(seed, n, d, q)
    raw = fr.CDataset.from_numpy(X, y, qid)
    ds = fr.Normalizer.fit(raw, "zscore").apply(raw)
    native.device_info(ds)
    rng = np.random.default_rng(1)
    W1, b1, W2, c = rng.normal(0.0, 0.1, (h, d)), rng.normal(0.0, 0.1, h), rng.normal(0.0, 0.2, (h2, h)), rng.normal(0.0, 0.1, h2)
    w3, b_out, lam = rng.normal(0.0, 0.3, h2), 0.25, rng.normal(0.0, 1.0, n)
    model = fr.CModel.from_dict({"NeuralNet": {"activation": "relu", "hidden_weights": W1.tolist(), "hidden_bias": b1.tolist(),
                                               "hidden2_weights": W2.tolist(), "hidden2_bias": c.tolist(), "output_weights": w3.tolist(),
                                               "output_bias": b_out}})
    plan = {}
    native.mlp2_gradients(ds, model, lam, plan=plan)  # warm-up: tables, records, code objects
    scores = native.predict_scores_dense(model, ds)
    fwd, bwd = mfma_per_tile(d, h, h2)
    floor = lambda mfmas: plan["tiles"] * mfmas * MFMA_CYCLES / SIMDS / CLOCK_HZ * 1e3  # noqa: E731
    out = {"metric": "two-hidden-layer NeuralNet kernels, device ms", "shape": args.shape, "n": n, "d": d, "hidden": h, "hidden2": h2, "queries": q,
           "plan": plan, "mfma_per_tile": {"score": fwd, "backprop": bwd}, "score_mfma_floor_ms": floor(fwd), "backprop_mfma_floor_ms": floor(bwd),
           "hbm_floor_ms": plan["tile_bytes"] / (HBM_ACHIEVABLE_GBS * 1e9) * 1e3, "runs": []}
    torch_once = None
    if not args.no_torch:
        xt = torch.from_numpy(np.ascontiguousarray(native.loaded_arrays(ds)["x"])).cuda()
        tp = [torch.from_numpy(a).cuda().requires_grad_() for a in (W1, b1, W2, c, w3)]
        tlam = torch.from_numpy(lam).cuda()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]

        def torch_once():
            ev[0].record()
            x64 = xt.double()
            ev[1].record()
            s = torch.relu(torch.relu(x64 @ tp[0].T + tp[1]) @ tp[2].T + tp[3]) @ tp[4] + b_out
            ev[2].record()
            g = torch.autograd.grad(s, tp, tlam)
            ev[3].record()
            torch.cuda.synchronize()
            return [ev[k].elapsed_time(ev[k + 1]) for k in range(3)], s.detach().cpu().numpy(), g[0].cpu().numpy(), g[2].cpu().numpy()

        torch_once()  # warm-up
    for _ in range(args.runs):
        native.profile_enable(True)
        native.profile_reset()
        scores = native.predict_scores_dense(model, ds)
        g = native.mlp2_gradients(ds, model, lam)
        prof = native.profile_stats()
        native.profile_enable(False)
        run = {"score_ms": prof["mlp2_score_kernel"]["total_ms"], "backprop_ms": prof["mlp2_backprop_kernel"]["total_ms"],
               "fold_ms": prof["mlp2_fold_kernel"]["total_ms"]}
        if torch_once is not None:
            (conv_ms, fwd_ms, bwd_ms), ts, tg1, tg2 = torch_once()
            rel = lambda a, b: float(np.max(np.abs(a - b)) / np.max(np.abs(a)))  # noqa: E731
            run.update(torch_convert_ms=conv_ms, torch_forward_ms=fwd_ms, torch_backward_ms=bwd_ms, max_rel_score_diff_vs_torch=rel(ts, scores),
                       max_rel_w1_grad_diff_vs_torch=rel(tg1, g["hidden_weights"]), max_rel_w2_grad_diff_vs_torch=rel(tg2, g["hidden2_weights"]))
        out["runs"].append(run)
    for key in out["runs"][0]:
        if key.endswith("_ms"):
            out[key + "_median"] = float(np.median([r[key] for r in out["runs"]]))
    out["score_over_mfma_floor"] = out["score_ms_median"] / out["score_mfma_floor_ms"]
    out["backprop_over_mfma_floor"] = out["backprop_ms_median"] / out["backprop_mfma_floor_ms"]
    req = fr.TrainRequest.neural_lambdarank()
    req.measure, req.params.quiet, req.params.num_iterations, req.params.hidden, req.params.hidden2 = "ndcg@10", True, args.iterations, h, h2
    t0 = time.perf_counter()
    ds.train_model(req)
    st = native.last_train_stats()["neural_lambdarank"]
    st["wall_seconds"] = time.perf_counter() - t0
    out["training"] = st
    print(json.dumps(out))


if __name__ == "__main__":
    main()
