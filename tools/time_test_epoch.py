#!/usr/bin/env python3
"""Times Recommender.testEpoch / testEpochFull under both evaluators (--evaluator host / device) on the Gowalla-shaped
synthetic dataset and hyper-parameters of tools/time_train_epoch.py (U = 48,653, I = 52,619, 3 intervals x 600 k edges,
d = 64, batch 512, 10,000 test users, testSize 1000). The evaluators run in the same process, alternated epoch by
epoch after warm-up; every device result is checked equal (==) to the host result of the same parameters. --seqAtt
both times the head's two forms (the collapsed sum / attention over every sequence item) one after the other in the
same process; --seqPool both does so for the full head's two poolings (the plain sum / additive attention; it implies
--seqAtt full) on one model that holds the additive variables."""
import argparse
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from sa_gnn_amd import Params, synthetic      # noqa: E402
from sa_gnn_amd.DataHandler import DataHandler   # noqa: E402
from sa_gnn_amd.Params import args            # noqa: E402
from sa_gnn_amd.model import Recommender      # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--epoch-only", action="store_true", help="one warm-up and one device test epoch (for a profiler)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seqAtt", choices=("sum", "full", "both"), default="sum", help="the head's form(s) to time")
    ap.add_argument("--seqPool", choices=("sum", "additive", "both"), default="sum",
                    help="the full head's pooling(s) to time (implies --seqAtt full)")
    ap.add_argument("--seqHeads", type=int, default=0, help="--seqHeads of the full head (needs --seqAtt full or both)")
    opt = ap.parse_args()
    if opt.seqHeads and opt.seqAtt == "sum" and opt.seqPool == "sum":
        sys.exit(f"--seqHeads {opt.seqHeads} needs --seqAtt full or both")
    if opt.seqPool != "sum" and opt.seqAtt == "sum":
        opt.seqAtt = "full"
    Params.parse_args("--data gowalla --lr 2e-3 --reg 1e-2 --ssl_reg 1e-6 --epoch 150 --batch 512 --sslNum 40 --graphNum 3 "
                      "--gnn_layer 2 --att_layer 1 --testSize 1000 --ssldim 48 --keepRate 0.5".split(), namespace=args)
    np.random.seed(100)
    U, I = 48653, 52619
    tmt = synthetic.make_trn_mat_time(U, I, [600000] * 3)
    seq = synthetic.make_sequence(tmt)
    rng = np.random.default_rng(1)
    tst = [None] * U
    for u in rng.choice(U, 10000, replace=False):
        tst[u] = int(rng.integers(0, I))
    test_dict = {u + 1: list(rng.integers(1, I + 1, size=1000)) for u in range(U)}
    h = DataHandler.from_memory(tmt, seq, tst, test_dict)
    rec = Recommender(torch.device("cuda:0"), h)
    if opt.seqPool != "sum":       # the additive variables are defined last: every other one starts where it always does
        args.seqAtt, args.seqPool = "full", "additive"
    rec.prepareModel()
    args.seqAtt = "sum"
    if opt.epoch_only:
        args.evaluator = "device"
        args.seqAtt = "full" if opt.seqAtt == "full" else "sum"
        args.seqPool = "additive" if opt.seqPool == "additive" else "sum"
        args.seqHeads = opt.seqHeads if args.seqAtt == "full" else 0
        for _ in range(2):
            rec.testEpoch()
        torch.cuda.synchronize()
        print("two device test epochs done")
        return
    pools = ("sum", "additive") if opt.seqPool == "both" else (opt.seqPool,)
    for att in (("sum", "full") if opt.seqAtt == "both" else (opt.seqAtt,)):
        for pool in (pools if att == "full" else ("sum",)):
            args.seqAtt, args.seqPool = att, pool
            args.seqHeads = opt.seqHeads if att == "full" else 0
            if opt.seqAtt != "sum":
                print(f"---- --seqAtt {att}" + (f" --seqPool {pool}" if opt.seqPool != "sum" else "") +
                      (f" --seqHeads {args.seqHeads}" if args.seqHeads else ""))
            time_evaluators(rec, h, opt)
    args.seqAtt, args.seqPool, args.seqHeads = "sum", "sum", 0


def time_evaluators(rec, h, opt):
    names = ("host", "device")
    kinds = {"testEpoch": rec.testEpoch, "testEpochFull": rec.testEpochFull}
    # first calls: the host path builds its candidate / sequence caches on its first test epoch, the device path its
    # tables (once per dataset and flag set)
    args.evaluator = "host"
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rec.testEpoch()
    torch.cuda.synchronize()
    print(f"[host] first testEpoch (its caches built inside) {1e3 * (time.perf_counter() - t0):.1f} ms")
    args.evaluator = "device"
    t0 = time.perf_counter()
    rec._device_evaluator()
    print(f"[device] evaluator tables built in {1e3 * (time.perf_counter() - t0):.1f} ms")
    results = {}
    for name in names:          # warm-up: kernels, workspaces, caches
        args.evaluator = name
        for kind, fn in kinds.items():
            for _ in range(2):
                results[(name, kind)] = fn()
    torch.cuda.synchronize()
    times = {(n, k): [] for n in names for k in kinds}
    for _ in range(opt.rounds):   # alternated, so both see the same machine state
        for kind, fn in kinds.items():
            for name in names:
                args.evaluator = name
                torch.cuda.synchronize()
                t = time.perf_counter()
                res = fn()
                torch.cuda.synchronize()
                times[(name, kind)].append(time.perf_counter() - t)
                assert res == results[(name, kind)]
    args.evaluator = "host"
    n = len(h.tstUsrs)
    for kind in kinds:
        same = results[("host", kind)] == results[("device", kind)]
        for name in names:
            v = times[(name, kind)]
            print(f"[{name}] {kind} ({n} users) {1e3 * float(np.median(v)):.1f} ms (median of {len(v)}; all: "
                  f"{[round(1e3 * x, 1) for x in v]})")
        host, dev = (float(np.median(times[(nm, kind)])) for nm in names)
        print(f"{kind}: device / host = 1 / {host / dev:.1f}; dicts equal: {same}",
              {k: round(v, 4) for k, v in results[("device", kind)].items()})
        if not same:
            sys.exit(1)


if __name__ == "__main__":
    main()
