#!/usr/bin/env python3
"""Times the interval SpMM with and without edge weights, in one process:
  - the batched stack (forward + backward) on the Gowalla-shaped synthetic set (U = 48,653, I = 52,619, 3 intervals x
    600 k edges, d = 64, 2 layers);
  - one per-interval SpMM on a quarter-scale synthetic graph of the roofline workload (250 k x 250 k, 25 M edges).
Each is run three ways, alternated round by round so that all see the same machine state: unweighted (the existing
entry on a plan without weights), all-ones weights on the same pattern (the cost of the weight stream alone), and the
sym normalisation (graph.sym_norm_weights; for the stack graph.interval_pair(norm="sym")). Median of --rounds rounds and
each form's min - max.

--parent-lib PATH: afterwards the unweighted entries are timed on the library at PATH (a build of the parent commit)
and on this build, in child processes alternated --pairs times in the same job. A library from before
sagnn_spmm_plan_set_weights existed is loaded without that symbol (--baseline-only does this).

--redo: the f16 x 2 engine's fp32 re-evaluations (sagnn_range_redo_count) over one Amazon-shaped L = 3 training step,
with --adjNorm none and with sym. A finding, not a criterion.

Numbers of different machines are not comparable."""
import argparse
import ctypes
import os
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from sa_gnn_amd import _lib      # noqa: E402


def timed(fn, rounds, inner):
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / inner * 1e3)
    return out


def report(title, runs, rounds, inner, out):
    times = {name: [] for name, _ in runs}
    for name, fn in runs:                      # warm-up
        timed(fn, 1, 3)
    for _ in range(rounds):                    # alternated
        for name, fn in runs:
            times[name] += timed(fn, 1, inner)
    base = float(np.median(times[runs[0][0]]))
    for name, _ in runs:
        v = times[name]
        line = (f"{title}: {name:<28} median {np.median(v):8.3f} ms  min {min(v):8.3f}  max {max(v):8.3f}  "
                f"ratio to unweighted {np.median(v) / base:5.3f}  ({rounds} rounds of {inner})")
        print(line, flush=True)
        out.append(line)


def bench(opt, lines):
    from sa_gnn_amd import graph, ops, synthetic
    dev = torch.device("cuda:0")
    weighted = not opt.baseline_only

    # ---- the batched stack, Gowalla-shaped
    np.random.seed(100)
    U, I, T, L, d = 48653, 52619, 3, 2, 64
    mats = synthetic.make_trn_mat_time(U, I, [600000] * T)[1]

    def batch_of(pairs):
        return ops.SpmmBatch([a.plan for a, _ in pairs], [t.plan for _, t in pairs]), pairs

    def ones_pair(m):
        out = []
        for mat, shape in ((m, (U, I)), (graph.transpose(m), (I, U))):
            rp, ci = graph.csr_arrays(mat)
            out.append(graph.IntervalAdj(rp, ci, shape, dev, weights=np.ones(ci.size, np.float32)))
        return tuple(out)

    batches = [("unweighted (existing entry)", batch_of([graph.interval_pair(m, dev) for m in mats]))]
    if weighted:
        batches += [("all-ones weights", batch_of([ones_pair(m) for m in mats])),
                    ("sym", batch_of([graph.interval_pair(m, dev, norm="sym") for m in mats]))]
        assert all(b.nnz == batches[0][1][0].nnz for _, (b, _) in batches)      # no duplicated entries: one pattern
    g = torch.Generator(device="cpu").manual_seed(0)
    ue = (torch.randn((T, U, d), generator=g) * 0.1).to(dev)
    ie = (torch.randn((T, I, d), generator=g) * 0.1).to(dev)
    gu, gi = torch.randn((T, U, d), generator=g).to(dev), torch.randn((T, I, d), generator=g).to(dev)
    ou, oi, du, di = (torch.empty_like(x) for x in (ue, ie, ue, ie))
    mu = torch.empty((T, L, U, d // 4), dtype=torch.uint8, device=dev)
    mi = torch.empty((T, L, I, d // 4), dtype=torch.uint8, device=dev)
    su, si = torch.empty(4 * T * U * d, device=dev), torch.empty(4 * T * I * d, device=dev)

    def stack(batch):
        def run():
            ops.gnn_stack(batch, ue, ie, L, 0.5, ou, oi, su, si, mask_u=mu, mask_i=mi)
            ops.gnn_stack_bwd(batch, gu, gi, L, 0.5, mu, mi, du, di, su, si)
        return run

    report("stack fwd+bwd (Gowalla-shaped, d=64, L=2)", [(n, stack(b)) for n, (b, _) in batches], opt.rounds, 10, lines)
    del batches, ue, ie, gu, gi, ou, oi, du, di, mu, mi, su, si

    # ---- one per-interval SpMM, quarter-scale roofline graph (power-law degrees: all three row classes)
    n, nnz = 250_000, 25_000_000
    eu, ei = synthetic.powerlaw_edges(n, n, nnz, seed=3, device=dev)
    (rp, ci), _ = synthetic.csr_pair_from_edges(eu, ei, n, n)
    del eu, ei
    plans = [("unweighted (existing entry)", ops.SpmmPlan(rp, ci, n, n, device=dev, validate=False))]
    if weighted:
        rp_h, ci_h = torch.as_tensor(rp).cpu().numpy(), torch.as_tensor(ci).cpu().numpy()
        plans += [("all-ones weights", ops.SpmmPlan(rp, ci, n, n, device=dev, validate=False,
                                                    weights=np.ones(ci_h.size, np.float32))),
                  ("sym", ops.SpmmPlan(rp, ci, n, n, device=dev, validate=False,
                                       weights=graph.sym_norm_weights(rp_h, ci_h, n, n)))]
    x = torch.randn((n, d), generator=g).to(dev)
    res = torch.randn((n, d), generator=g).to(dev)
    out = torch.empty((n, d), device=dev)
    one = lambda plan: (lambda: ops.spmm_ex(plan, x, 0.5, residual=res, out=out))      # noqa: E731
    report(f"one SpMM ({n} rows, {plans[0][1].nnz} edges, d=64)", [(nm, one(p)) for nm, p in plans], opt.rounds, 5, lines)


def redo_counts(lines):
    """One Amazon-shaped training step (T = 5, L = 3, d = 64) per normalisation: the count after the step."""
    from sa_gnn_amd import Params, ops, synthetic
    from sa_gnn_amd.DataHandler import DataHandler
    from sa_gnn_amd.Params import args
    from sa_gnn_amd.model import Recommender
    Params.parse_args("--lr 2e-3 --reg 1e-2 --ssl_reg 1e-6 --batch 512 --sslNum 40 --graphNum 5 --gnn_layer 3 --att_layer 1 "
                      "--testSize 100 --ssldim 48 --keepRate 0.5 --trnNum 512".split(), namespace=args)
    np.random.seed(100)
    U, I = 11_199, 30_821
    tmt = synthetic.make_trn_mat_time(U, I, [72280, 78997, 79692, 78096, 45651])
    seq = synthetic.make_sequence(tmt)
    rng = np.random.default_rng(1)
    tst = [None] * U
    for u in rng.choice(U, 1000, replace=False):
        tst[u] = int(rng.integers(0, I))
    h = DataHandler.from_memory(tmt, seq, tst, {u + 1: list(rng.integers(1, I + 1, size=100)) for u in range(U)})
    for norm in ("none", "sym"):
        args.adjNorm = norm
        rec = Recommender(torch.device("cuda:0"), h)
        rec.prepareModel()
        counts = []
        for _ in range(3):                 # the same first step three times over: parameters re-drawn by prepareModel's seed
            np.random.seed(7)
            torch.manual_seed(7)
            bat = np.random.permutation(args.user)[:args.batch]
            batch = rec._host_train_batch(bat)
            params = rec._trainable()
            for p in params.values():
                p.grad = None
            torch.cuda.synchronize()
            ops.range_redo_count(reset=True)
            pre, ssl = rec.train_loss(batch)
            (pre + args.ssl_reg * ssl).backward()
            torch.cuda.synchronize()
            counts.append(ops.range_redo_count())
        fu = rec.forward()[0]
        line = (f"range redo count, one Amazon-shaped training step (T=5, L=3, d=64, batch 512), --adjNorm {norm}: {counts} "
                f"(three evaluations of the same step); max |final user vector| {float(fu.abs().max()):.3f}, loss {float(pre):.4f}")
        print(line, flush=True)
        lines.append(line)
    args.adjNorm = "none"


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--baseline-only", action="store_true", help="time the unweighted entries only")
    ap.add_argument("--parent-lib", default=None, help="a build of the parent commit to time the unweighted entries on")
    ap.add_argument("--pairs", type=int, default=3, help="alternated (parent, this build) child runs for --parent-lib")
    ap.add_argument("--redo", action="store_true", help="also record the range redo counts with none and sym")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    opt = ap.parse_args()
    lines = []
    if opt.baseline_only:
        probe = ctypes.CDLL(_lib.LIB_PATH)
        if not hasattr(probe, "sagnn_spmm_plan_set_weights"):       # a library from before the entry
            _lib.SIGNATURES.pop("sagnn_spmm_plan_set_weights")
    bench(opt, lines)
    if opt.redo:
        redo_counts(lines)
    if opt.parent_lib:
        torch.cuda.empty_cache()
        me = os.path.abspath(__file__)
        for r in range(opt.pairs):
            for name, lib in (("parent library", opt.parent_lib), ("this build", None)):
                env = dict(os.environ)
                env.pop("SAGNN_LIB", None)
                if lib:
                    env["SAGNN_LIB"] = lib
                res = subprocess.run([sys.executable, me, "--baseline-only", "--rounds", str(opt.rounds)], env=env,
                                     capture_output=True, text=True, timeout=600)
                if res.returncode != 0:
                    raise SystemExit(f"{name} child failed ({res.returncode}): {res.stderr[-2000:]}")
                for line in res.stdout.splitlines():
                    line = f"[pair {r + 1}, {name}] {line}"
                    print(line, flush=True)
                    lines.append(line)
    if opt.out:
        with open(opt.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
