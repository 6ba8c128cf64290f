#!/usr/bin/env python3
"""Times the GRU cell of the interval fusion (--rnnCell gru) against the LSTM it stands beside, in one
process on one GPU:

  1. the recurrent forward alone on 1.5 M rows at d in {32, 64} and T in {2, 6, 16}: the fused GRU kernel (exact fp32 MFMA
     under every engine), the exact-fp32 LSTM (ops.engine("f32"): lstm_fwd_mfma_kernel) and the default-engine LSTM
     (f16 x 2). HIP events around each call after warm-up, the three alternated round by round; medians.
  2. a training step on the Gowalla-shaped synthetic set of tools/time_train_epoch.py under both cells (default engine,
     device sampler, --fusion_rows all): each cell's model is built, warmed up and timed in turn, twice over, wall clock
     around whole epochs ending in a device synchronise.

The one timing condition (stated in the output): at d = 64, T = 16 the fused GRU forward takes at most 1.03 x the
exact-fp32 LSTM forward of the same run. Writes what it prints to --out (profiles/gru_bench.txt)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from sa_gnn_amd import ops                                  # noqa: E402
from sa_gnn_amd.model import random_fusion_params           # noqa: E402

ROWS = 1_500_000
MARGIN = 1.03


def time_forward(dev, emit, rounds=7):
    res = {}
    for d in (32, 64):
        lstm = random_fusion_params(d, dev, 1)
        gru = random_fusion_params(d, dev, 1, cell="gru")
        gw = [gru[k] for k in ops.GRU_KEYS]
        for T in (2, 6, 16):
            x = torch.randn((T, ROWS, d), device=dev).permute(1, 0, 2)       # the GNN slab's layout
            h = torch.empty((ROWS, T, d), device=dev)

            def run_gru():
                ops.gru_fwd(x, *gw, out=h)

            def run_f32():
                with ops.engine("f32"):
                    ops.lstm_fwd(x, lstm["lstm_W"], lstm["lstm_b"], out=h)

            def run_f16():
                ops.lstm_fwd(x, lstm["lstm_W"], lstm["lstm_b"], out=h)

            runs = {"gru f32": run_gru, "lstm f32": run_f32, "lstm f16x2": run_f16}
            for fn in runs.values():                                         # warm-up: code objects, LDS limits
                fn(), fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in runs}
            for _ in range(rounds):                                          # alternated: the same machine state for all
                for k, fn in runs.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fn()
                    b.record()
                    b.synchronize()
                    ms[k].append(a.elapsed_time(b))
            med = {k: float(np.median(v)) for k, v in ms.items()}
            res[(d, T)] = med
            emit(f"forward, {ROWS} rows, d = {d}, T = {T} (ms, median of {rounds}; min .. max): " + "; ".join(
                f"{k} {med[k]:.3f} ({min(ms[k]):.3f} .. {max(ms[k]):.3f})" for k in runs) +
                f"; gru / lstm f32 = {med['gru f32'] / med['lstm f32']:.3f}, gru / lstm f16x2 = {med['gru f32'] / med['lstm f16x2']:.3f}")
            del x, h
    g, l = res[(64, 16)]["gru f32"], res[(64, 16)]["lstm f32"]
    emit(f"TIMING CONDITION (d = 64, T = 16: fused GRU forward <= {MARGIN} x exact-fp32 LSTM forward): "
         f"{g:.3f} ms vs {l:.3f} ms, ratio {g / l:.3f}: {'MET' if g <= MARGIN * l else 'MISSED'}")


def time_training(dev, emit, rounds=2):
    from time_train_epoch import gowalla_shaped_handler
    from sa_gnn_amd.Params import args
    from sa_gnn_amd.Utils import NNLayers as NNs
    from sa_gnn_amd.model import Recommender
    handler = gowalla_shaped_handler()
    args.sampler, args.fusion_rows = "device", "all"
    steps = int(np.ceil(args.trnNum / args.batch))
    for r in range(rounds):
        for cell in ("lstm", "gru"):
            args.rnnCell = cell
            rec = Recommender(dev, handler)
            rec.prepareModel()
            rec.trainEpoch()                                                 # warm-up: kernels, workspaces, sampler tables
            torch.cuda.synchronize()
            ep = []
            for _ in range(3):
                t0 = time.perf_counter()
                rec.trainEpoch()
                torch.cuda.synchronize()
                ep.append(time.perf_counter() - t0)
            finite = all(bool(torch.isfinite(p).all()) for p in NNs.params.values())
            emit(f"training, Gowalla-shaped, d = {args.latdim}, T = {args.graphNum}, default engine, --rnnCell {cell} (round {r}): "
                 f"epoch {1e3 * float(np.median(ep)):.1f} ms = {steps} steps of {1e3 * float(np.median(ep)) / steps:.2f} ms "
                 f"(median of 3; all: {[round(1e3 * v, 1) for v in ep]}); every parameter finite: {finite}")
    args.rnnCell = "lstm"


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=os.path.join(__file__.rsplit("/", 2)[0], "profiles", "gru_bench.txt"))
    ap.add_argument("--skip-training", action="store_true", help="the forward kernels only")
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_gru.py needs a GPU: nothing here is measured without one")
    dev = torch.device("cuda:0")
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    emit(f"tools/bench_gru.py on {torch.cuda.get_device_name(0)}; engines: gru f32 = exact-fp32 MFMA (the GRU's only form), "
         "lstm f32 = SAGNN_ENGINE_F32 (lstm_fwd_mfma_kernel), lstm f16x2 = the default engine")
    time_forward(dev, emit)
    if not opt.skip_training:
        time_training(dev, emit)
    with open(opt.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
