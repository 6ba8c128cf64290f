#!/usr/bin/env python3
"""Observation behind DESIGN.md §26: trains the Gowalla-shaped synthetic set (tools/time_train_epoch.py's) for the same
number of epochs from the same seed under seqAtt full / seqTargets last, causal / last and causal / all (device sampler,
--fusion_rows batch, --predLoss softmax --softmaxNegs N) and prints preLoss per epoch and Recommender.testEpochFull()'s
full-ranking HR / NDCG after each. Not a pass condition: the set's test items are uniform draws."""
import argparse
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
sys.path.insert(0, __file__.rsplit("/", 1)[0])
from time_train_epoch import gowalla_shaped_handler   # noqa: E402
from sa_gnn_amd.Params import args            # noqa: E402
from sa_gnn_amd.Utils import NNLayers as NNs  # noqa: E402
from sa_gnn_amd.model import Recommender      # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--epochs", type=int, default=6)
    ap.add_argument("--softmaxNegs", type=int, default=4096)
    ap.add_argument("--lr", type=float, default=5e-4)
    ap.add_argument("--seed", type=int, default=7)
    opt = ap.parse_args()
    h = gowalla_shaped_handler()
    for att, tgt in (("full", "last"), ("causal", "last"), ("causal", "all")):
        args.seqAtt, args.seqTargets, args.predLoss, args.softmaxNegs = att, tgt, "softmax", opt.softmaxNegs
        args.sampler, args.fusion_rows, args.evaluator, args.lr = "device", "batch", "device", opt.lr
        np.random.seed(opt.seed)
        torch.manual_seed(opt.seed)
        rec = Recommender(torch.device("cuda:0"), h)
        rec.prepareModel()
        t0 = time.perf_counter()
        losses = [rec.trainEpoch()["preLoss"] for _ in range(opt.epochs)]
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        res = rec.testEpochFull()
        print(f"[seqAtt {att}, seqTargets {tgt}] {opt.epochs} epochs in {dt:.1f} s; preLoss per epoch "
              f"{[round(float(v), 4) for v in losses]}; full ranking {({k: round(float(v), 5) for k, v in res.items()})}; finite "
              f"{all(bool(torch.isfinite(p).all()) for p in NNs.params.values())}", flush=True)


if __name__ == "__main__":
    main()
