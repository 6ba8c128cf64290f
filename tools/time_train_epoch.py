#!/usr/bin/env python3
"""Times Recommender.trainEpoch / testEpoch on a Gowalla-shaped synthetic dataset with the reference's
gowalla.sh hyper-parameters (U = 48,653, I = 52,619, 3 intervals x 600 k edges, d = 64, batch 512,
trnNum 10000 -> 20 steps per epoch, keepRate 0.5) and prints where a training step spends its time
(sampling / forward + loss / backward / optimiser), wall clock with a device sync after each part. Both samplers
(--sampler host / device) run in the same process, alternated epoch by epoch; --fusion_rows both alternates the two
fusion modes as well (all rows / the rows the batch reads) and reports the touched rows per step and the f16 x 2
kernels' fp32 re-evaluations per epoch of each mode. --seqAtt both alternates the head's two forms (the collapsed sum /
attention over every sequence item) and reports the device time of the sequence-attention entries per step
(sagnn_profile_read, kind 5). --predLoss both alternates the head's two training losses (the sampled hinge loss / the
full-catalogue softmax) and reports the device time of the softmax entries per step (kind 6). --seqPool both alternates
the two poolings of the full head (the plain sum / additive attention; it implies --seqAtt full) on one model that holds
the additive variables, every timed epoch from the initial parameters, and reports kind 5 per step for each.
--softmaxNegs N runs the softmax loss over N sampled candidates (kind 7 instead of 6), which also lets --predLoss softmax
combine with --fusion_rows batch; with --predLoss both it is a third loss beside the hinge loss and the full-catalogue
softmax (which then runs under --fusion_rows all only). --softmaxNegDist pop draws those candidates by popularity with
the logQ offsets; both alternates the uniform and the weighted draw as two losses. --sampler restricts the run to one
sampler. --seqAtt causal runs the token head with causal attention; with it --seqTargets all trains every sequence
position (it needs --predLoss softmax) and both alternates the two target modes; the loss terms per step of every softmax
configuration are reported beside the loss entries' device time."""
import argparse
import ctypes
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from sa_gnn_amd import Params, ops, synthetic      # noqa: E402
from sa_gnn_amd.DataHandler import DataHandler   # noqa: E402
from sa_gnn_amd.Params import args            # noqa: E402
from sa_gnn_amd.Utils import NNLayers as NNs  # noqa: E402
from sa_gnn_amd.model import Recommender      # noqa: E402


def gowalla_shaped_handler():
    """Sets gowalla.sh's hyper-parameters in Params.args and returns the Gowalla-shaped synthetic DataHandler (also what
    tools/bench_gru.py trains on)."""
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
    return DataHandler.from_memory(tmt, seq, tst, test_dict)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--epoch-only", action="store_true", help="one warm-up and one device-sampler epoch (for a profiler)")
    ap.add_argument("--fusion_rows", choices=("all", "batch", "both"), default="all",
                    help="fusion mode(s) to time; both alternates them in one process")
    ap.add_argument("--edge_keep", type=float, default=1.0,
                    help="--edgeKeepRate of the run: below 1 the training steps drop edges of the interval graphs")
    ap.add_argument("--seqAtt", choices=("sum", "full", "causal", "both"), default="sum",
                    help="the head's form(s) to time; both alternates sum and full in one process")
    ap.add_argument("--seqTargets", choices=("last", "all", "both"), default="last",
                    help="the positions the head trains on (all needs --seqAtt causal and --predLoss softmax); both "
                         "alternates them in one process")
    ap.add_argument("--predLoss", choices=("hinge", "softmax", "both"), default="hinge",
                    help="the head's training loss(es) to time; both alternates them in one process")
    ap.add_argument("--seqPool", choices=("sum", "additive", "both"), default="sum",
                    help="the full head's pooling(s) to time (implies --seqAtt full); both alternates them in one process")
    ap.add_argument("--softmaxNegs", type=int, default=0,
                    help="candidates of --predLoss softmax (0 = the whole catalogue); > 0 allows --fusion_rows batch with it")
    ap.add_argument("--softmaxNegDist", choices=("uniform", "pop", "both"), default="uniform",
                    help="how the --softmaxNegs candidates are drawn; both alternates the two in one process")
    ap.add_argument("--sampler", choices=("host", "device", "both"), default="both", help="the sampler(s) to time")
    ap.add_argument("--seqHeads", default="0",
                    help="--seqHeads of the token head (needs --seqAtt full or causal): one count, or a comma-separated "
                         "list such as 0,2 whose entries alternate in one process")
    ap.add_argument("--seqFFN", default="0",
                    help="--seqFFN of the token head (needs --seqAtt full or causal): one hidden width, or 0,F whose "
                         "entries alternate in one process (the blocks' variables are defined once, at width F)")
    opt = ap.parse_args()
    if opt.seqPool != "sum" and opt.seqAtt == "sum":
        opt.seqAtt = "full"
    if opt.seqTargets != "last" and (opt.seqAtt != "causal" or opt.predLoss != "softmax" or opt.seqPool != "sum"):
        sys.exit(f"--seqTargets {opt.seqTargets} needs --seqAtt causal, --predLoss softmax and --seqPool sum")
    heads = tuple(int(v) for v in opt.seqHeads.split(","))
    if any(heads) and opt.seqAtt not in ("full", "causal"):
        sys.exit(f"--seqHeads {opt.seqHeads} needs --seqAtt full or causal")
    ffns = tuple(int(v) for v in opt.seqFFN.split(","))
    if any(ffns) and opt.seqAtt not in ("full", "causal"):
        sys.exit(f"--seqFFN {opt.seqFFN} needs --seqAtt full or causal")
    if len({v for v in ffns if v}) > 1:
        sys.exit(f"--seqFFN {opt.seqFFN}: one hidden width besides 0")
    h = gowalla_shaped_handler()
    args.edgeKeepRate = opt.edge_keep
    rec = Recommender(torch.device("cuda:0"), h)
    if opt.seqPool != "sum":       # the additive variables are defined last: every other one starts where it always does
        args.seqAtt, args.seqPool = "full", "additive"
    if any(ffns):                  # the blocks' variables are defined after those: the same holds for them
        args.seqAtt, args.seqFFN = opt.seqAtt, max(ffns)
    rec.prepareModel()
    args.seqAtt = "sum"
    if opt.softmaxNegs < 0 or opt.softmaxNegs > args.item:
        sys.exit(f"--softmaxNegs {opt.softmaxNegs}: need 0 <= N <= {args.item}")
    if opt.softmaxNegDist != "uniform" and (opt.softmaxNegs == 0 or opt.predLoss == "hinge"):
        sys.exit(f"--softmaxNegDist {opt.softmaxNegDist} needs --softmaxNegs > 0 and --predLoss softmax or both")
    if opt.epoch_only:
        args.sampler = "device"
        args.fusion_rows = "batch" if opt.fusion_rows == "batch" else "all"
        args.seqAtt = opt.seqAtt if opt.seqAtt in ("full", "causal") else "sum"
        args.seqTargets = "all" if opt.seqTargets == "all" else "last"
        args.predLoss = "softmax" if opt.predLoss == "softmax" else "hinge"
        args.softmaxNegs = opt.softmaxNegs if args.predLoss == "softmax" else 0
        args.softmaxNegDist = "pop" if opt.softmaxNegDist == "pop" and args.softmaxNegs else "uniform"
        args.seqPool = "additive" if opt.seqPool == "additive" else "sum"
        args.seqHeads = heads[0]
        args.seqFFN = ffns[0]      # _seq_att_full reads it at every call: 0 runs the head without the blocks
        for _ in range(2):
            rec.trainEpoch()
        torch.cuda.synchronize()
        print(f"two device-sampler epochs done (--fusion_rows {args.fusion_rows}, --edge_keep {args.edgeKeepRate}, "
              f"--seqAtt {args.seqAtt}, --seqHeads {args.seqHeads}, --seqFFN {args.seqFFN}, --seqTargets {args.seqTargets}, --seqPool {args.seqPool}, --predLoss {args.predLoss}, --softmaxNegs {args.softmaxNegs}, "
              f"--softmaxNegDist {args.softmaxNegDist}); "
              "every parameter finite:",
              all(bool(torch.isfinite(p).all()) for p in NNs.params.values()))
        return
    modes = ("all", "batch") if opt.fusion_rows == "both" else (opt.fusion_rows,)
    atts = ("sum", "full") if opt.seqAtt == "both" else (opt.seqAtt,)
    negs = f"softmax, softmaxNegs {opt.softmaxNegs}"       # the third loss: the softmax over sampled candidates
    negs_pop = negs + ", pop"                              # a fourth: those candidates drawn by popularity
    cand_losses = {"uniform": (negs,), "pop": (negs_pop,), "both": (negs, negs_pop)}[opt.softmaxNegDist]
    losses = ("hinge", "softmax") if opt.predLoss == "both" else (opt.predLoss,)
    if opt.softmaxNegs and "softmax" in losses:
        losses = losses + cand_losses if opt.predLoss == "both" else cand_losses
    pools = ("sum", "additive") if opt.seqPool == "both" else (opt.seqPool,)
    if "softmax" in losses and modes == ("batch",):
        sys.exit("--predLoss softmax does not combine with --fusion_rows batch without --softmaxNegs")
    samplers = ("host", "device") if opt.sampler == "both" else (opt.sampler,)
    tgts = ("last", "all") if opt.seqTargets == "both" else (opt.seqTargets,)
    tokens = ("full", "causal")                            # the head forms in which every sequence item is a token
    configs = [(sampler, mode, att, loss, pool, tgt, hd, fw) for loss in losses for att in atts for pool in pools for tgt in tgts
               for hd in heads for fw in ffns for mode in modes for sampler in samplers
               if (att in tokens or pool == "sum") and not (loss == "softmax" and mode == "batch")]
    label = lambda c: ", ".join([c[0]] + ([f"{c[1]} rows"] if len(modes) > 1 else []) +   # noqa: E731
                                ([f"seqAtt {c[2]}"] if atts != ("sum",) else []) +
                                ([f"seqPool {c[4]}"] if pools != ("sum",) else []) +
                                ([f"predLoss {c[3]}"] if losses != ("hinge",) else []) +
                                ([f"seqTargets {c[5]}"] if tgts != ("last",) else []) +
                                ([f"seqHeads {c[6]}"] if heads != (0,) else []) +
                                ([f"seqFFN {c[7]}"] if ffns != (0,) else []))

    initial = {k: p.detach().clone() for k, p in NNs.params.items()}
    finite = {}

    def use(c, fresh=False):
        # fresh: the initial parameters and a new optimiser. Step times depend on the parameters (the f16 x 2 kernels'
        # fp32 re-evaluations), and at gowalla.sh's learning rate this synthetic set's training goes non-finite after a
        # few hundred steps, with or without --seqAtt full (non-finite epochs run at half the time): with several head
        # forms every timed epoch is therefore the first epoch of its own training (profiles/seq_att_epoch.txt holds a
        # parent-commit run that shows the default path's divergence). A run without --seqAtt both keeps training its
        # parameters as before, so its lines, not a `both` run's sum lines, are what compares with an earlier commit.
        args.sampler, args.fusion_rows, args.seqAtt, loss, args.seqPool, args.seqTargets, hd, fw = c
        args.seqHeads = hd if args.seqAtt in tokens else 0
        args.seqFFN = fw if args.seqAtt in tokens else 0
        args.predLoss = "hinge" if loss == "hinge" else "softmax"
        args.softmaxNegs = opt.softmaxNegs if loss in cand_losses else 0
        args.softmaxNegDist = "pop" if loss == negs_pop else "uniform"
        if fresh and len(atts) * len(losses) * len(pools) * len(tgts) * len(heads) * len(ffns) > 1:
            with torch.no_grad():
                for k, p in NNs.params.items():
                    p.copy_(initial[k])
            rec.optimizer = None

    def note_finite(c):
        finite[c] = finite.get(c, True) and all(bool(torch.isfinite(p).all()) for p in NNs.params.values())

    for c in configs:              # warm-up: kernels, workspaces, the device sampler's tables
        use(c, fresh=True)
        for _ in range(2):
            rec.trainEpoch()
    torch.cuda.synchronize()
    steps = int(np.ceil(args.trnNum / args.batch))
    rounds = 3
    epoch = {c: [] for c in configs}
    redo = {c: [] for c in configs}
    for r in range(rounds):        # alternated, so every configuration sees the same machine state
        for c in configs:
            use(c, fresh=True)
            torch.cuda.synchronize()
            ops.range_redo_count(reset=True)
            t0 = time.perf_counter()
            rec.trainEpoch()
            torch.cuda.synchronize()
            epoch[c].append(time.perf_counter() - t0)
            redo[c].append(ops.range_redo_count())
            note_finite(c)
    for c in configs:
        ep = float(np.median(epoch[c]))
        print(f"[{label(c)}] train epoch {ep * 1e3:.1f} ms = {steps} steps of {ep / steps * 1e3:.2f} ms "
              f"(median of {rounds}; all: {[round(1e3 * v, 1) for v in epoch[c]]}); "
              f"range redo count per epoch {redo[c]}; every parameter finite after each: {finite[c]}")
    # one step, by part
    parts = {c: {"sample": 0.0, "forward+loss": 0.0, "backward": 0.0, "optimiser": 0.0} for c in configs}
    touched = {c: [] for c in configs}
    for r in range(rounds):
        for c in configs:
            use(c, fresh=True)
            sf = np.random.permutation(args.user)[:args.trnNum]
            seed = int(np.random.randint(0, 2 ** 63, dtype=np.int64))
            part = parts[c]
            if getattr(rec, "optimizer", None) is None:
                rec.optimizer = rec._make_optimizer()
            for i in range(steps):
                bat = sf[i * args.batch:(i + 1) * args.batch]
                torch.cuda.synchronize(); t = time.perf_counter()
                if c[0] == "device":
                    batch = rec.sample_batch_device(bat, seed, i)
                else:
                    batch = rec._host_train_batch(bat)
                torch.cuda.synchronize(); part["sample"] += time.perf_counter() - t; t = time.perf_counter()
                params = rec._trainable()
                for p in params.values():
                    p.grad = None
                pre, ssl = rec.train_loss(batch)
                loss = pre + args.ssl_reg * ssl
                torch.cuda.synchronize(); part["forward+loss"] += time.perf_counter() - t; t = time.perf_counter()
                if c[1] == "batch":
                    touched[c].append(rec.fusion_rows_counts)
                loss.backward()
                torch.cuda.synchronize(); part["backward"] += time.perf_counter() - t; t = time.perf_counter()
                rec.optimizer.step({k: p.grad for k, p in params.items()})
                torch.cuda.synchronize(); part["optimiser"] += time.perf_counter() - t
            note_finite(c)
    for c in configs:
        print(f"[{label(c)}] per step (ms, synced between parts, mean of {rounds} epochs):",
              {k: round(v / (steps * rounds) * 1e3, 3) for k, v in parts[c].items()})
        if touched[c]:
            tu, ti = np.mean(np.asarray(touched[c], dtype=np.float64), axis=0)
            print(f"[{label(c)}] touched rows per step (mean of {len(touched[c])}): users {tu:.1f} of {args.user} "
                  f"({100 * tu / args.user:.2f} %), items {ti:.1f} of {args.item} ({100 * ti / args.item:.2f} %)")
    # device time of the sequence-attention entries (kind 5), one device-sampler epoch per token form, pooling and target mode
    for att, pool, tgt, hd, fw in [(a, po, t, hd, fw) for a in atts if a in tokens for po in pools for t in tgts for hd in heads
                                   for fw in ffns]:
        lib = ops._lib.load()
        use(("device", modes[0], att, losses[0], pool, tgt, hd, fw), fresh=True)
        cap = 4096 * steps
        lib.sagnn_profile_enable(cap)
        rec.trainEpoch()
        ms, kind, n = np.zeros(cap, np.float32), np.zeros(cap, np.int32), ctypes.c_int(0)
        ops.check(lib.sagnn_profile_read(ms.ctypes.data, kind.ctypes.data, None, None, cap, ctypes.byref(n)))
        lib.sagnn_profile_enable(0)
        sel = kind[:n.value] == 5
        print(f"[device, seqAtt {att}{', seqPool ' + pool if pools != ('sum',) else ''}{', seqTargets ' + tgt if tgts != ('last',) else ''}{', seqHeads ' + str(hd) if heads != (0,) else ''}{', seqFFN ' + str(fw) if ffns != (0,) else ''}] "
              f"sequence-attention entries (gather, attention, feed-forward blocks, pool or prefix queries and their backwards): "
              f"{int(sel.sum()) / steps:.0f} calls and {float(ms[:n.value][sel].sum()) / steps:.3f} ms of device time per step; "
              f"layer-norm entries (profile kind 3): {float(ms[:n.value][kind[:n.value] == 3].sum()) / steps:.3f} ms per step")
        print("every parameter finite after that epoch:", all(bool(torch.isfinite(p).all()) for p in NNs.params.values()))
    # device time of the softmax-loss entries (kind 6; 7 over candidates), one device-sampler epoch per loss and mode
    for loss, mode, tgt in [(lo, m, t) for lo in losses for m in modes for t in tgts
                            if lo != "hinge" and not (lo == "softmax" and m == "batch")]:
        lib = ops._lib.load()
        use(("device", mode, atts[0], loss, pools[0] if atts[0] in tokens else "sum", tgt, heads[0], ffns[0]), fresh=True)
        cap = 4096 * steps
        terms, entries = [], {k: getattr(ops, k) for k in ("softmax_loss", "softmax_loss_cand")}

        def counted(fn, at):           # the loss terms of a call: its rows with a target (a read-back of this tool's own)
            def call(*a, **k):
                terms.append(int((a[at] >= 0).sum()))
                return fn(*a, **k)
            return call
        ops.softmax_loss, ops.softmax_loss_cand = counted(entries["softmax_loss"], 2), counted(entries["softmax_loss_cand"], 3)
        lib.sagnn_profile_enable(cap)
        try:
            rec.trainEpoch()
        finally:
            ops.softmax_loss, ops.softmax_loss_cand = entries["softmax_loss"], entries["softmax_loss_cand"]
        ms, kind, n = np.zeros(cap, np.float32), np.zeros(cap, np.int32), ctypes.c_int(0)
        ops.check(lib.sagnn_profile_read(ms.ctypes.data, kind.ctypes.data, None, None, cap, ctypes.byref(n)))
        lib.sagnn_profile_enable(0)
        sel = np.flatnonzero(kind[:n.value] == (7 if loss in cand_losses else 6))
        print(f"[device, {mode} rows, predLoss {loss}{', seqTargets ' + tgt if tgts != ('last',) else ''}] softmax-loss entries: "
              f"{len(sel) / steps:.0f} calls per step; forward "
              f"{float(ms[sel[0::2]].sum()) / steps:.3f} ms and backward {float(ms[sel[1::2]].sum()) / steps:.3f} ms of device "
              f"time per step; loss terms per step {np.mean(terms):.1f}")
    print("every parameter finite after every timed epoch above:", finite)
    args.fusion_rows = "all"
    args.predLoss = "hinge"
    args.softmaxNegs = 0
    args.softmaxNegDist = "uniform"
    args.sampler = "host"
    args.seqAtt = "sum"
    args.seqPool = "sum"
    args.seqTargets = "last"
    args.seqHeads = 0
    args.seqFFN = 0
    t0 = time.perf_counter()
    res = rec.testEpoch()
    torch.cuda.synchronize()
    print(f"test epoch ({len(h.tstUsrs)} users) {1e3 * (time.perf_counter() - t0):.1f} ms", {k: round(v, 4) for k, v in res.items()})


if __name__ == "__main__":
    main()
